"""Wall time of getEMagLsFiltersFromAtf designs whose low bins (or all bins) take the dense route at 9..32 microphones, next to the
same shapes on the Gram route (glasses_atfs' 1e-4 noise floor, no near-copy), and the two-waves-per-column kernels for more than
3072 matched directions next to the plain forms (EMAGLS_WA_TALL=0).  The inputs are those of tests/from_atf_dense_cases.py.

    python tools/from_atf_dense_timing.py [reps]          # one line per case: ms per execute (median, min), dense bins
    rocprofv3 --kernel-trace --stats -- python tools/from_atf_dense_timing.py 3 copy16     # the kernels of the dense stage
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import from_atf_dense_cases as C  # noqa: E402


def gram_case(nmics, tall=False):
    """The yardstick: the same shape with the 1e-4 noise floor and no near-copy (every bin on the Gram route)."""
    from emagls_amd import synth
    g = C.fib_grid() if tall else C.thin_grid()
    atf, aazi, azen = synth.glasses_atfs(natf=4000 if tall else C.NATF, nmics=nmics, taps=C.ATF_TAPS, noise=1e-4)
    return g["hL"], g["hR"], np.column_stack([g["azi"], g["zen"]]), atf, np.column_stack([aazi, azen])


def time_case(inputs, reps):
    from emagls_amd import Plan, _lib as L
    hL, hR, hg, atf, ag = inputs
    p = Plan(L.KIND_FROM_ATF, "real", 0, C.FS, C.LEN, hL.shape[0], hL.shape[1], nmics=atf.shape[1], f_trans=C.F_TRANS,
             atf_taps=atf.shape[0], natf=atf.shape[2])
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
    p.close()
    gf = i.gram_from
    dense = (gf if gf > 0 else i.num_pos_freqs) - 1
    return float(np.median(ts)), float(np.min(ts)), dense, int(i.device_bytes)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    only = sys.argv[2:]
    rows = [("copy9", lambda: C.case("copy9"), None), ("copy16", lambda: C.case("copy16"), None), ("copy32", lambda: C.case("copy32"), None),
            ("below_cut", lambda: C.case("below_cut"), None), ("above_cut", lambda: C.case("above_cut"), None),
            ("gram9", lambda: gram_case(9), None), ("gram16", lambda: gram_case(16), None), ("gram32", lambda: gram_case(32), None),
            ("tall", lambda: C.case("tall"), None), ("tall_plain", lambda: C.case("tall"), "0"), ("gram16_tall", lambda: gram_case(16, True), None)]
    for name, make, wa_tall in rows:
        if only and name not in only:
            continue
        if wa_tall is None:
            os.environ.pop("EMAGLS_WA_TALL", None)
        else:
            os.environ["EMAGLS_WA_TALL"] = wa_tall
        med, best, dense, nbytes = time_case(make(), reps)
        print("%-12s median %8.3f ms  min %8.3f ms  dense bins %3d  device bytes %d" % (name, med, best, dense, nbytes), flush=True)
    os.environ.pop("EMAGLS_WA_TALL", None)


if __name__ == "__main__":
    main()
