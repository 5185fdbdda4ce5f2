"""Wall time of getRenderedHrtfs on config 3's shape (2702 directions, 32 microphones at 4.2 cm: S = 400, 25 channels, len 512,
nfft 1024) for 1 and 20 filter sets, with and without the response output, next to the NumPy composition of the same result
(fft, the oracle's getSMAIRMatrix, getSH, einsum, the metrics) on the same machine.  Host arrays in, host arrays out: a call
includes its copies.  Writes the table that profiles/r14_rendered_hrtfs.md quotes.

    python tools/rendered_hrtfs_timing.py [reps] [out.md]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FS, LEN, NFFT, ORDER = 48000.0, 512, 1024, 4


def numpy_composition(wL, wR, dirs, mics, radius, hL, hR):
    """One set, the way the tests state it; returns (seconds with the array model built, seconds with it given)."""
    from oracle import emagls_oracle as O
    from test_rendered_hrtfs_host import rendered_metrics
    t0 = time.perf_counter()
    sm, sim = O.getSMAIRMatrix(ORDER, FS, NFFT, radius, mics, "real")
    Yc = np.conj(O.getSH(sim, dirs, "real"))
    t1 = time.perf_counter()
    H = np.stack([np.einsum("ks,ds->kd", np.einsum("kc,csk->ks", np.fft.fft(w, NFFT, axis=0)[:NFFT // 2 + 1], sm), Yc) for w in (wL, wR)], axis=2)
    ref = np.stack([np.fft.rfft(hL, NFFT, axis=0), np.fft.rfft(hR, NFFT, axis=0)], axis=2)
    rendered_metrics(H, ref)
    t2 = time.perf_counter()
    return t2 - t0, t2 - t1


def main():
    import emagls_amd as E
    from emagls_amd import synth
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    out = sys.argv[2] if len(sys.argv) > 2 else None
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_fixtures.npz"))
    dirs = np.column_stack([g["grid/hrirGridAziRad"], g["grid/hrirGridZenRad"]])
    mics = np.column_stack([g["grid/micGridAziRad"], g["grid/micGridZenRad"]])
    radius = float(g["real_eMagLS_woDC/micRadius"])
    hL, hR = synth.rigid_sphere_hrirs(dirs[:, 0], dirs[:, 1])
    rng = np.random.default_rng(14)
    ws = [(rng.standard_normal((LEN, 25)), rng.standard_normal((LEN, 25))) for _ in range(20)]
    kw = dict(order=ORDER, micRadius=radius, micGridAziZenRad=mics, nfft=NFFT, hL=hL, hR=hR)
    lines = ["| sets | response returned | median ms per call | min ms | ms per set |", "|---|---|---|---|---|"]
    for nsets in (1, 20):
        wl, wr = [w[0] for w in ws[:nsets]], [w[1] for w in ws[:nsets]]
        for resp in (True, False):
            for _ in range(2):      # code objects, the first allocations
                E.getRenderedHrtfs(wl, wr, "emagls", dirs, FS, returnResponse=resp, **kw)
            ts = []
            for _ in range(reps):
                t = time.perf_counter()
                E.getRenderedHrtfs(wl, wr, "emagls", dirs, FS, returnResponse=resp, **kw)    # (returns host arrays: synchronised)
                ts.append((time.perf_counter() - t) * 1e3)
            lines.append("| %d | %s | %.2f | %.2f | %.2f |" % (nsets, "yes" if resp else "no", np.median(ts), np.min(ts), np.median(ts) / nsets))
    full, given = numpy_composition(ws[0][0], ws[0][1], dirs, mics, radius, hL, hR)
    lines.append("")
    lines.append("NumPy composition, one set: %.0f ms with the array model and the basis built, %.0f ms with both given." % (full * 1e3, given * 1e3))
    text = "\n".join(lines)
    print(text, flush=True)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
