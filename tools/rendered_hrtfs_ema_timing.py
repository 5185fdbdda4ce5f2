"""Wall time of getRenderedHrtfs for the two equatorial-array models on config 3's shape (2702 directions, len 512, nfft 1024, order 4,
16 microphones at 4.2 cm: S = 400; 9 channels for 'ema_ch', 25 for 'ema_sh'), metrics only, for 1 and 20 filter sets, next to the
'emagls' model on that shape (32 microphones, 25 channels) and to the NumPy composition of the same result, the way
tests/test_gpu_rendered_hrtfs_ema.py states it, on the same machine.  Host arrays in, host arrays out: a call includes its copies.
The share of an 'ema_sh' call that builds the rotated order terms QT' is estimated from calls with nfft 8 (five bins: spectra,
left operand and product are then next to nothing), 'ema_sh' minus 'ema_ch'.  Writes the tables profiles/r16_rendered_hrtfs_ema.md
quotes.  EMAGLS_LIB_PATH selects another build of the library (the parent commit's, for the 'emagls' row).

    python tools/rendered_hrtfs_ema_timing.py [reps] [out.md] [models, comma separated] [numpy: 0/1]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FS, LEN, NFFT, ORDER, M_EMA, RADIUS = 48000.0, 512, 1024, 4, 16, 0.042


def timed(fn, reps):
    for _ in range(2):      # code objects, the first allocations
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()                # (returns host arrays: synchronised)
        ts.append((time.perf_counter() - t) * 1e3)
    return ts


def numpy_composition(model, wL, wR, dirs, hL, hR):
    import test_gpu_rendered_hrtfs_ema as T
    from test_rendered_hrtfs_host import rendered_metrics
    t0 = time.perf_counter()
    H = T.expected(model, wL, wR, dirs, RADIUS, ORDER, "real", M_EMA, NFFT)
    rendered_metrics(H, np.stack([np.fft.rfft(hL, NFFT, axis=0), np.fft.rfft(hR, NFFT, axis=0)], axis=2))
    return time.perf_counter() - t0


def main():
    import emagls_amd as E
    from emagls_amd import synth
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    out = sys.argv[2] if len(sys.argv) > 2 else None
    models = sys.argv[3].split(",") if len(sys.argv) > 3 else ["emagls", "ema_ch", "ema_sh"]
    with_numpy = len(sys.argv) <= 4 or sys.argv[4] != "0"
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_fixtures.npz"))
    dirs = np.column_stack([g["grid/hrirGridAziRad"], g["grid/hrirGridZenRad"]])
    mics = {"emagls": np.column_stack([g["grid/micGridAziRad"], g["grid/micGridZenRad"]])}
    mics["ema_ch"] = mics["ema_sh"] = 2.0 * np.pi * np.arange(M_EMA) / M_EMA
    nch = {"emagls": 25, "ema_ch": 2 * ORDER + 1, "ema_sh": 25}
    hL, hR = synth.rigid_sphere_hrirs(dirs[:, 0], dirs[:, 1])
    rng = np.random.default_rng(16)
    lines = ["library: %s" % E._lib.LIB_PATH, "", "| model | sets | median ms per call | min ms | max ms | ms per set |", "|---|---|---|---|---|---|"]
    for model in models:
        ws = [(rng.standard_normal((LEN, nch[model])), rng.standard_normal((LEN, nch[model]))) for _ in range(20)]
        kw = dict(order=ORDER, micRadius=RADIUS, micGridAziZenRad=mics[model], nfft=NFFT, hL=hL, hR=hR, returnResponse=False)
        for nsets in (1, 20):
            wl, wr = [w[0] for w in ws[:nsets]], [w[1] for w in ws[:nsets]]
            ts = timed(lambda: E.getRenderedHrtfs(wl, wr, model, dirs, FS, **kw), reps)
            lines.append("| %s | %d | %.2f | %.2f | %.2f | %.2f |" % (model, nsets, np.median(ts), np.min(ts), np.max(ts), np.median(ts) / nsets))
            print(lines[-1], flush=True)
    if "ema_sh" in models and "ema_ch" in models:
        lines += ["", "Five bins (len 4, nfft 8, HRIRs cut to 8 samples), one set, the same directions and array:", ""]
        small = {}
        for model in ("ema_ch", "ema_sh"):
            w = rng.standard_normal((4, nch[model]))
            kw = dict(order=ORDER, micRadius=RADIUS, micGridAziZenRad=mics[model], nfft=8, hL=hL[:8], hR=hR[:8], returnResponse=False)
            ts = timed(lambda: E.getRenderedHrtfs(w, w, model, dirs, FS, **kw), reps)
            small[model] = float(np.median(ts))
            lines.append("* `%s`: median %.2f ms, min %.2f ms" % (model, np.median(ts), np.min(ts)))
            print(lines[-1], flush=True)
        lines.append("* difference (the rotation fit and the order terms QT'): %.2f ms" % (small["ema_sh"] - small["ema_ch"]))
    if with_numpy:
        lines.append("")
        for model in [m for m in models if m != "emagls"]:
            w = rng.standard_normal((LEN, nch[model]))
            lines.append("NumPy composition of `%s`, one set, array model and rotations built: %.0f ms." % (model, numpy_composition(model, w, w, dirs, hL, hR) * 1e3))
            print(lines[-1], flush=True)
    text = "\n".join(lines)
    print(text, flush=True)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
