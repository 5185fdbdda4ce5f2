"""Timing of the GPU resampler (MATLAB's resample(x, p, q), DESIGN.md sections 7 and 9): median wall-clock of `reps` calls of
emagls_resample_device after three warm ones (each timed call ends in a device synchronise), buffers resident in HBM.

  standalone   100 s x 32 channels (an array recording) at 44.1 -> 48, 48 -> 44.1, 96 -> 48, 48 -> 8 kHz and x3, plus 47999/48000
               (a bank too large for LDS: the taps are read through the caches)
  decode       binauralDecode with 512-tap filters 48 -> 44.1 kHz, a 1 s order-4 SH response and a 60 s signal
               (emagls_binaural_decode_render_fs_device), against the same call at matched rates (_ypr_device)

Bytes are derived from shapes: the resampler reads every input and writes every output once (8 B per real value); the share of
HBM peak is those bytes over the median time and the 6.3 TB/s a streaming copy achieves on the MI355X.  Where scipy is present,
scipy.signal.resample_poly(..., window=('kaiser', 5.0)) on the host CPU (one call) is the baseline of the first three cases.

    python tools/resample_timing.py [--reps 20] [--seconds 100] [--json resample_timing.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_ACHIEVABLE_GBPS = 6300.0     # MI355X, float4 streaming copy


def _median_ms(call, reps):
    import torch
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, float(np.min(ts)) * 1e3, float(np.max(ts)) * 1e3


def standalone(lib, L, reps, seconds, nch=32):
    import torch
    cases = [("44.1 -> 48 kHz", 44100, 160, 147), ("48 -> 44.1 kHz", 48000, 147, 160), ("96 -> 48 kHz", 96000, 1, 2),
             ("48 -> 8 kHz", 48000, 1, 6), ("x3 (16 -> 48 kHz)", 16000, 3, 1), ("47999/48000", 48000, 47999, 48000)]
    rows = []
    for name, fs_in, p, q in cases:
        n = int(seconds * fs_in)
        ny = int(lib.emagls_resample_length(n, p, q))
        x = torch.randn((nch, n), dtype=torch.float64, device="cuda")
        y = torch.empty((nch, ny), dtype=torch.float64, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def call():
            L.check(lib.emagls_resample_device(C.c_void_p(x.data_ptr()), 0, n, nch, p, q, C.c_void_p(y.data_ptr()), st))
        med, lo, hi = _median_ms(call, reps)
        gb = 8.0 * nch * (n + ny) / 1e9
        row = dict(case=name, p=p, q=q, nsamp=n, nch=nch, out=ny, ms=med, ms_min=lo, ms_max=hi, gb=gb,
                   gbps=gb / (med * 1e-3), hbm_frac=gb / (med * 1e-3) / HBM_ACHIEVABLE_GBPS)
        if len(rows) < 3:
            try:
                from scipy import signal as ss
                xh = x.cpu().numpy().T
                t0 = time.perf_counter()
                ss.resample_poly(xh, p, q, axis=0, window=("kaiser", 5.0))
                row["scipy_cpu_ms"] = (time.perf_counter() - t0) * 1e3
            except ImportError:
                pass
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, y
        torch.cuda.empty_cache()
    return rows


def decode(lib, L, reps, sig_seconds=60.0, nch=25, ln=512, fs=44100, fs_filter=48000):
    import torch
    n = fs                       # a 1 s SH response
    nsig = int(sig_seconds * fs)
    dev = "cuda"
    x = torch.randn(nch * n, dtype=torch.float64, device=dev)
    wL, wR = (torch.randn(nch * ln, dtype=torch.float64, device=dev) for _ in range(2))
    s = torch.randn(nsig, dtype=torch.float64, device=dev)
    out = torch.empty(2 * nsig, dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = []
    for name, ffs in [("matched rates (_ypr_device)", None), ("filters 48 -> 44.1 kHz (_fs_device)", fs_filter)]:
        if ffs is None:
            def call():
                L.check(lib.emagls_binaural_decode_render_ypr_device(p(x), 0, n, nch, p(wL), p(wR), 0, ln, 0, 0, None, 0, None, 0, None, 0,
                                                                     p(s), nsig, p(out), None, st))
        else:
            def call():
                L.check(lib.emagls_binaural_decode_render_fs_device(p(x), 0, n, nch, p(wL), p(wR), 0, ln, 0, 0, None, 0, None, 0, None, 0,
                                                                    p(s), nsig, float(fs), float(ffs), float(fs), p(out), None, st))
        med, lo, hi = _median_ms(call, reps)
        row = dict(case="binauralDecode " + name, nch=nch, n=n, taps=ln, nsig=nsig, ms=med, ms_min=lo, ms_max=hi)
        rows.append(row)
        print(json.dumps(row), flush=True)
    rows[1]["ratio_to_matched"] = rows[1]["ms"] / rows[0]["ms"]
    print(json.dumps(dict(decode_resampled_over_matched=rows[1]["ratio_to_matched"])), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=100.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (first: the library then shares torch's HIP runtime)
    from emagls_amd import _lib as L
    lib = L.load()
    rows = standalone(lib, L, a.reps, a.seconds) + decode(lib, L, a.reps)
    print("\n| case | ms (median) | GB moved | GB/s | share of 6.3 TB/s | scipy CPU ms |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        if "gb" in r:
            print("| %s (%d/%d) | %.3f | %.2f | %.0f | %.0f %% | %s |" % (r["case"], r["p"], r["q"], r["ms"], r["gb"], r["gbps"],
                                                                        100 * r["hbm_frac"], "%.0f" % r["scipy_cpu_ms"] if "scipy_cpu_ms" in r else "-"))
        else:
            print("| %s | %.3f | | | | |" % (r["case"], r["ms"]))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    assert math.isfinite(rows[0]["ms"])


if __name__ == "__main__":
    main()
