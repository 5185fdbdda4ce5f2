#!/bin/bash
# One GPU-box session: parity tests, smoke, the bench line, rocprofv3 kernel traces.  Usage (through gpurun):
#   EMAGLS_OUT_DIR=<dir> bash tools/gpu_round.sh <tag> [tests|notests|testsonly] [pmc]      (testsonly: the whole gpu suite without -x, nothing else)
# Everything lands in $EMAGLS_OUT_DIR/<tag>_*; copy what should be judged into profiles/.  PYTEST_K='expr' selects tests (-k).
# The first bench line and the trace that tools/sweep_launches.py reads are --full runs (parity, CPU baseline, roofline).
tag=${1:-r}; what=${2:-tests}; pmc=${3:-}
export EMAGLS_BUILD_TAG=$tag
R=$(cd "$(dirname "$0")/.." && pwd); cd $R
O=$(mkdir -p "${EMAGLS_OUT_DIR:?the folder the outputs go to}" && cd "$EMAGLS_OUT_DIR" && pwd)
if [ "$what" = "tests" ]; then
  timeout 1500 python -m pytest tests -m gpu -q -rP -x --durations=40 ${PYTEST_K:+-k "$PYTEST_K"} > $O/${tag}_tests_full.log 2>&1
  tail -5 $O/${tag}_tests_full.log > $O/${tag}_tests.log
  grep -h "norm_diff=\|rel = \|^case (\|rel L\|worst rel" $O/${tag}_tests_full.log > $O/${tag}_parity.log
  timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/${tag}_smoke.log 2>&1
fi
if [ "$what" = "testsonly" ]; then
  timeout 2400 python -m pytest tests -m gpu -q -rP --durations=40 ${PYTEST_K:+-k "$PYTEST_K"} > $O/${tag}_tests_full.log 2>&1
  tail -15 $O/${tag}_tests_full.log > $O/${tag}_tests.log
  grep -h "norm_diff=\|rel = \|^case (\|rel L\|worst rel" $O/${tag}_tests_full.log > $O/${tag}_parity.log
  cat $O/${tag}_tests.log; exit 0
fi
timeout 900 python bench.py --full --steps 20 --warmup 5 > $O/${tag}_bench20.json 2> $O/${tag}_bench20.err
timeout 600 python bench.py --steps 128 --warmup 32 --no-cpu-baseline --no-sh-roofline --no-secondary > $O/${tag}_bench128.json 2> $O/${tag}_bench128.err
export TMPDIR=/tmp; cd /tmp
timeout 300 rocprofv3 --kernel-trace --stats -d $O/${tag}_prof_single -o bench -- python3 $R/bench.py --steps 8 --warmup 0 --slots 1 --batch 1 --no-cpu-baseline --no-sh-roofline --no-secondary > $O/${tag}_prof_single.log 2>&1
timeout 300 rocprofv3 --kernel-trace --stats -d $O/${tag}_prof_batch -o bench -- python3 $R/bench.py --steps 32 --warmup 0 --slots 1 --batch 8 --no-cpu-baseline --no-sh-roofline --no-secondary > $O/${tag}_prof_batch.log 2>&1
timeout 300 rocprofv3 --kernel-trace --stats -d $O/${tag}_prof_batch16 -o bench -- python3 $R/bench.py --steps 128 --warmup 0 --slots 1 --batch 32 --no-cpu-baseline --no-sh-roofline --no-secondary > $O/${tag}_prof_batch16.log 2>&1
timeout 300 rocprofv3 --kernel-trace -d $O/${tag}_prof_slots4 -o bench -- python3 $R/bench.py --steps 128 --warmup 0 --no-cpu-baseline --no-sh-roofline --no-secondary > $O/${tag}_prof_slots4.log 2>&1
timeout 300 rocprofv3 --kernel-trace --stats -d $O/${tag}_prof_hrirsets -o hs -- python3 $R/tools/experiments/hrir_sets_prof.py 4 > $O/${tag}_prof_hrirsets.log 2>&1
timeout 300 rocprofv3 --kernel-trace --stats -d $O/${tag}_prof_default20 -o bench -- python3 $R/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-sh-roofline --no-secondary > $O/${tag}_prof_default20.log 2>&1
if [ "$pmc" = "pmc" ]; then
  # counters in passes of their own (kernel-trace only next to --pmc); one chunk of 32 designs in flight (the bench's default shape:
  # two lane groups of 16 before one 32-design sweep launch), 4 chunks executed after the three set-up runs
  PMCCMD="python3 $R/bench.py --steps 128 --warmup 0 --slots 1 --batch 32 --no-cpu-baseline --no-sh-roofline --no-secondary"
  for c in FETCH_SIZE WRITE_SIZE SQ_INSTS_VALU_MFMA_MOPS_F64 SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU; do
    timeout 400 rocprofv3 --kernel-trace --pmc $c -d $O/${tag}_pmc_$c -o pmc -- $PMCCMD > $O/${tag}_pmc_$c.log 2>&1
  done
  cd $R
  python tools/pmc_summary.py $O/${tag}_pmc_traffic.json $O/${tag}_pmc.md $O/${tag}_pmc_* > $O/${tag}_pmc_summary.log 2>&1
  rm -rf $O/${tag}_pmc_FETCH_SIZE $O/${tag}_pmc_WRITE_SIZE $O/${tag}_pmc_SQ_*
fi
cd $R
python tools/kernel_avgs.py $O/${tag}_prof_single 1 > $O/${tag}_kernels_single.md 2>&1
python tools/kernel_avgs.py $O/${tag}_prof_batch 8 > $O/${tag}_kernels_batch.md 2>&1
python tools/kernel_avgs.py $O/${tag}_prof_batch > $O/${tag}_kernels_batch_all.md 2>&1
python tools/kernel_avgs.py $O/${tag}_prof_batch16 16 > $O/${tag}_kernels_batch16_groups.md 2>&1
python tools/kernel_avgs.py $O/${tag}_prof_batch16 > $O/${tag}_kernels_batch16_all.md 2>&1
python tools/sweep_launches.py $O/${tag}_prof_default20 $O/${tag}_prof_default20.log > $O/${tag}_default20_sweep_launches.md 2>&1
python tools/kernel_avgs.py $O/${tag}_prof_default20 > $O/${tag}_default20_kernels.md 2>&1
python tools/fill_timeline.py $O/${tag}_prof_default20 2 > $O/${tag}_fill_timeline20.md 2>&1
python tools/timeline.py $O/${tag}_prof_slots4 10 > $O/${tag}_timeline_slots4.md 2>&1
python tools/timeline.py $O/${tag}_prof_batch 3 > $O/${tag}_timeline_slots1.md 2>&1
python tools/kernel_avgs.py $O/${tag}_prof_hrirsets > $O/${tag}_hrir_sets_kernels.md 2>&1
python tools/timeline.py $O/${tag}_prof_hrirsets 12 > $O/${tag}_hrir_sets_timeline.md 2>&1
# the raw databases are large: keep the summaries
rm -rf $O/${tag}_prof_hrirsets $O/${tag}_prof_single $O/${tag}_prof_batch $O/${tag}_prof_slots4 $O/${tag}_prof_batch16 $O/${tag}_prof_default20
cat $O/${tag}_tests.log $O/${tag}_smoke.log 2>/dev/null; cut -c1-600 $O/${tag}_bench20.json; echo; cut -c1-300 $O/${tag}_bench128.json; echo; tail -3 $O/${tag}_bench20.err; head -32 $O/${tag}_kernels_batch.md; head -12 $O/${tag}_timeline_slots4.md
