"""Wall and stage times of getEMagLsFiltersFromAtf designs with more than 4096 matched directions whose bins take the dense route's
tiled form (near-copy microphone, as tests/from_atf_tiled_cases.py), next to the same shapes on the Gram route (no near-copy).

    python tools/from_atf_tiled_timing.py [reps] [Dm] [taps] [widths ...]     # default: 10 16384 2048 8 16 32
    EMAGLS_WA_LEAF_ROWS=4096 python tools/from_atf_tiled_timing.py 10 8192 2048 16      # another leaf height (1024 .. 4096)
    rocprofv3 --kernel-trace --stats -- python tools/from_atf_tiled_timing.py 3 8192 2048 16
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FS, F_TRANS = 48000.0, 2000.0


def inputs(nmics, dm, taps, dense):
    from emagls_amd import synth
    azi, zen = synth.fibonacci_grid(dm)
    hL, hR = synth.rigid_sphere_hrirs(azi, zen)
    atf, aazi, azen = synth.glasses_atfs(natf=dm, nmics=nmics, taps=min(taps, 256), noise=1e-4)
    if dense and nmics > 1:
        rng = np.random.default_rng(3)
        atf[:, nmics - 1, :] = atf[:, nmics - 2, :] + 1e-9 * rng.standard_normal(atf[:, nmics - 2, :].shape)
    return hL, hR, np.column_stack([azi, zen]), atf, np.column_stack([aazi, azen])


def time_case(inp, taps, reps):
    from emagls_amd import Plan, _lib as L
    hL, hR, hg, atf, ag = inp
    p = Plan(L.KIND_FROM_ATF, "real", 0, FS, taps, hL.shape[0], hL.shape[1], nmics=atf.shape[1], f_trans=F_TRANS, atf_taps=atf.shape[0],
             natf=atf.shape[2])
    p.set_hrir_grid(hg[:, 0], hg[:, 1])
    p.set_hrirs(hL, hR)
    p.set_atfs(atf, ag[:, 0], ag[:, 1])
    for _ in range(3):          # flag and re-run (the flag is read when the filters are fetched), capture, first replay
        p.execute()
        p.get_filters()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        p.execute()
        p.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    i = p.info()
    p.set_profiling(1)          # eager, events around the stages
    st = {}
    for _ in range(3):
        p.execute()
        p.synchronize()
        for k, v in p.stage_times():
            st.setdefault(k, []).append(v)
    p.close()
    gf = i.gram_from
    dense = (gf if gf > 0 else i.num_pos_freqs) - 1
    return float(np.median(ts)), float(np.min(ts)), dense, int(i.device_bytes), {k: float(np.median(v)) for k, v in st.items()}


def main():
    a = sys.argv[1:]
    reps = int(a[0]) if a else 10
    dm = int(a[1]) if len(a) > 1 else 16384
    taps = int(a[2]) if len(a) > 2 else 2048
    widths = [int(x) for x in a[3:]] or [8, 16, 32]
    for m in widths:
        for dense in (True, False):
            med, best, nd, nbytes, st = time_case(inputs(m, dm, taps, dense), taps, reps)
            print("%2d mics x %5d, %4d taps, %-5s median %8.3f ms  min %8.3f ms  dense bins %4d  device bytes %d  factor_bins %.3f ms  [%s]"
                  % (m, dm, taps, "dense" if dense else "gram", med, best, nd, nbytes, st.get("factor_bins", float("nan")),
                     " ".join("%s %.3f" % kv for kv in st.items())), flush=True)


if __name__ == "__main__":
    main()
