"""Timing of binauralDecode with head rotation and source signal (emagls_binaural_decode_render_device) against the plain render
loop (emagls_binaural_decode_device), buffers resident in HBM, median wall-clock of `reps` calls after three warm ones (every
call synchronises its stream before returning).

  plain        100 s x 25 channels x 512 taps (bench_secondary's binaural_decode_100s shape), no rotation
  fixed        the same with one yaw angle (the filters are rotated: 2 x 512 x 25 values)
  trajectory   the same with one yaw angle per sample (a separate rotation pass over the signal before the decode)
  source       a 1 s SH impulse response (48 000 samples x 25 channels) rendered, then convolved with 60 s of dry signal

    python tools/decode_render_timing.py [--reps 10] [--out profiles/r07_decode_render.md]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0   # MI355X HBM3E, nominal


def _median_ms(call, reps):
    import torch
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def run(reps=10, nsamp=4_800_000, nch=25, length=512, ir_len=48_000, sig_len=2_880_000):
    import torch
    from emagls_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng(7)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    res = {"shape": {"samples": nsamp, "channels": nch, "taps": length}, "device": torch.cuda.get_device_name(0)}
    for kind, cplx in (("real", False), ("complex", True)):
        dt = torch.complex128 if cplx else torch.float64
        mk = lambda r, c: (torch.randn((c, r), dtype=dt, device="cuda"))     # noqa: E731  [c][r] row-major == [r x c] column-major
        d_sig, d_wl, d_wr = mk(nsamp, nch), mk(length, nch), mk(length, nch)
        d_out = torch.zeros((2, nsamp), dtype=torch.float64, device="cuda")
        d_yaw1 = torch.tensor([0.7], dtype=torch.float64, device="cuda")
        d_traj = torch.from_numpy(np.cumsum(rng.normal(0, 1e-3, nsamp))).cuda()
        basis = L.BASIS["complex" if cplx else "real"]
        plain = lambda: L.check(lib.emagls_binaural_decode_device(p(d_sig), int(cplx), nsamp, nch, p(d_wl), p(d_wr), int(cplx), length,   # noqa: E731
                                                                  p(d_out), None, None))
        rend = lambda yaw, ny: L.check(lib.emagls_binaural_decode_render_device(p(d_sig), int(cplx), nsamp, nch, p(d_wl), p(d_wr),   # noqa: E731
                                                                                int(cplx), length, L.LAYOUT["sh"], basis, p(yaw), ny, None, 0,
                                                                                p(d_out), None, None))
        t_plain = _median_ms(plain, reps)
        t_fixed = _median_ms(lambda: rend(d_yaw1, 1), reps)
        t_traj = _median_ms(lambda: rend(d_traj, nsamp), reps)
        es = 16 if cplx else 8
        rot_bytes = 2.0 * es * nsamp * nch + 8.0 * nsamp          # read C values and one angle per sample, write C values
        t_rot = t_traj - t_plain
        res[kind] = {"plain_ms": round(t_plain, 4), "fixed_ms": round(t_fixed, 4), "trajectory_ms": round(t_traj, 4),
                     "fixed_over_plain": round(t_fixed / t_plain, 4), "trajectory_over_plain": round(t_traj / t_plain, 4),
                     "rotation_pass_ms": round(t_rot, 4), "rotation_pass_bytes": rot_bytes,
                     "rotation_pass_frac_of_hbm_peak": round(rot_bytes / (t_rot * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4) if t_rot > 0 else None}
        del d_sig, d_out, d_traj
        torch.cuda.empty_cache()
    # the source-signal convolution: 1 s impulse response, 60 s signal (real SH)
    d_ir = torch.randn((nch, ir_len), dtype=torch.float64, device="cuda")
    d_wl, d_wr = torch.randn((nch, length), dtype=torch.float64, device="cuda"), torch.randn((nch, length), dtype=torch.float64, device="cuda")
    d_src = torch.randn(sig_len, dtype=torch.float64, device="cuda")
    d_o1 = torch.zeros((2, ir_len), dtype=torch.float64, device="cuda")
    d_o2 = torch.zeros((2, sig_len), dtype=torch.float64, device="cuda")
    first = lambda: L.check(lib.emagls_binaural_decode_device(p(d_ir), 0, ir_len, nch, p(d_wl), p(d_wr), 0, length, p(d_o1), None, None))   # noqa: E731
    both = lambda: L.check(lib.emagls_binaural_decode_render_device(p(d_ir), 0, ir_len, nch, p(d_wl), p(d_wr), 0, length, 0, 0, None, 0,   # noqa: E731
                                                                    p(d_src), sig_len, p(d_o2), None, None))
    t_first = _median_ms(first, reps)
    t_both = _median_ms(both, reps)
    res["source"] = {"ir_samples": ir_len, "signal_samples": sig_len, "render_ir_ms": round(t_first, 4), "render_and_convolve_ms": round(t_both, 4),
                     "convolution_ms": round(t_both - t_first, 4), "realtime_factor_48k": round(sig_len / 48000.0 / (t_both * 1e-3), 1)}
    return res


def markdown(res):
    s = res["shape"]
    lines = ["# binauralDecode with rotation and source signal: timings", "",
             "`python tools/decode_render_timing.py` on %s; median wall-clock per call, buffers in HBM." % res["device"], "",
             "%d samples (100 s at 48 kHz) x %d SH channels x %d taps, both ears:" % (s["samples"], s["channels"], s["taps"]), "",
             "| signal | plain decode ms | fixed angle ms (ratio) | trajectory ms (ratio) | rotation pass ms | pass share of HBM peak |",
             "|---|---|---|---|---|---|"]
    for k in ("real", "complex"):
        r = res[k]
        lines.append("| %s | %.3f | %.3f (%.3f) | %.3f (%.3f) | %.3f | %s |" % (
            k, r["plain_ms"], r["fixed_ms"], r["fixed_over_plain"], r["trajectory_ms"], r["trajectory_over_plain"], r["rotation_pass_ms"],
            "%.1f %%" % (100 * r["rotation_pass_frac_of_hbm_peak"]) if r["rotation_pass_frac_of_hbm_peak"] else "-"))
    src = res["source"]
    lines += ["", "Source signal: a %d-sample response rendered (%.3f ms), then convolved with %d samples of signal: %.3f ms in all, "
              "%.3f ms for the convolution (%.0f x real time)." % (src["ir_samples"], src["render_ir_ms"], src["signal_samples"],
                                                                  src["render_and_convolve_ms"], src["convolution_ms"], src["realtime_factor_48k"]),
              "", "```json", json.dumps(res, indent=1), "```", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="markdown report (profiles/r07_decode_render.md)")
    a = ap.parse_args()
    res = run(a.reps)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(markdown(res))


if __name__ == "__main__":
    main()
