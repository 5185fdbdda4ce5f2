"""Timing of the three-axis rotation (DESIGN.md sections 7 and 9), on the model of tools/decode_render_timing.py: median wall-clock
of `reps` calls after three warm ones (every call synchronises its stream before returning), buffers resident in HBM.

  order 4     100 s x 25 channels x 512 taps (bench_secondary's binaural_decode_100s shape), real and complex SH:
              plain decode; a fixed yaw-pitch-roll (the filters are rotated); one yaw-pitch-roll per sample (a separate
              rotation pass over the signal before the decode); the yaw-only trajectory for comparison
  order 15    10 s x 256 channels, real SH, one rotation per sample: emagls_rotate_sh from host arrays (the wall-clock includes
              the copies; the kernel's own time comes from a rocprofv3 --kernel-trace --stats run of this tool)

Bytes and FMAs are derived from shapes: a pass reads and writes every value once and reads one value of each per-sample angle;
per sample and order n it does 2 x nnz(J_n) multiply-adds with J_n (nnz = n^2 + n + 1) plus the three z rotations (4 FMAs per
(m, -m) pair each) and their angle additions, times 2 for complex values.

    python tools/rotate3_timing.py [--reps 10] [--out profiles/r08_rotate3.md]
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

HBM_PEAK_GBPS = 8000.0      # MI355X HBM3E, nominal
FP64_PEAK_TFLOPS = 78.6     # MI355X vector FP64


def fma_per_sample(N, cplx):
    f = sum(2 * (n * n + n + 1) + 3 * (4 * n + 4 * max(n - 1, 0)) for n in range(1, N + 1))
    return f * (2 if cplx else 1)


def pass_bytes(nsamp, nch, cplx, n_angle_arrays=3):
    es = 16 if cplx else 8
    return 2.0 * es * nsamp * nch + 8.0 * n_angle_arrays * nsamp


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


def run(reps=10, nsamp=4_800_000, nch=25, length=512, n15=480_000):
    import torch
    from emagls_amd import _lib as L
    lib = L.load()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    res = {"shape": {"samples": nsamp, "channels": nch, "taps": length}, "device": torch.cuda.get_device_name(0)}
    t = np.linspace(0, 100, nsamp)
    traj = [np.ascontiguousarray(a) for a in (2.0 * np.sin(0.3 * t), 1.7 * np.sin(0.21 * t), 0.8 * np.cos(0.17 * t))]
    for kind, cplx in (("real", False), ("complex", True)):
        dt = torch.complex128 if cplx else torch.float64
        mk = lambda r, c: (torch.randn((c, r), dtype=dt, device="cuda"))     # noqa: E731  [c][r] row-major == [r x c] column-major
        d_sig, d_wl, d_wr = mk(nsamp, nch), mk(length, nch), mk(length, nch)
        d_out = torch.zeros((2, nsamp), dtype=torch.float64, device="cuda")
        d_one = [torch.tensor([v], dtype=torch.float64, device="cuda") for v in (0.7, -1.1, 0.4)]
        d_traj = [torch.from_numpy(a).cuda() for a in traj]
        basis = L.BASIS["complex" if cplx else "real"]
        plain = lambda: L.check(lib.emagls_binaural_decode_device(p(d_sig), int(cplx), nsamp, nch, p(d_wl), p(d_wr), int(cplx), length,   # noqa: E731
                                                                  p(d_out), None, None))

        def ypr(angles, n):
            L.check(lib.emagls_binaural_decode_render_ypr_device(p(d_sig), int(cplx), nsamp, nch, p(d_wl), p(d_wr), int(cplx), length,
                                                                 L.LAYOUT["sh"], basis, p(angles[0]), n, p(angles[1]), n, p(angles[2]), n,
                                                                 None, 0, p(d_out), None, None))
        yaw_traj = lambda: L.check(lib.emagls_binaural_decode_render_device(p(d_sig), int(cplx), nsamp, nch, p(d_wl), p(d_wr), int(cplx),   # noqa: E731
                                                                            length, L.LAYOUT["sh"], basis, p(d_traj[0]), nsamp, None, 0,
                                                                            p(d_out), None, None))
        t_plain = _median_ms(plain, reps)
        t_fixed = _median_ms(lambda: ypr(d_one, 1), reps)
        t_traj = _median_ms(lambda: ypr(d_traj, nsamp), reps)
        t_yaw = _median_ms(yaw_traj, reps)
        t_rot = t_traj - t_plain
        b = pass_bytes(nsamp, nch, cplx)
        res[kind] = {"plain_ms": round(t_plain, 4), "fixed_ms": round(t_fixed, 4), "trajectory_ms": round(t_traj, 4),
                     "yaw_trajectory_ms": round(t_yaw, 4), "fixed_over_plain": round(t_fixed / t_plain, 4),
                     "trajectory_over_plain": round(t_traj / t_plain, 4), "yaw_trajectory_over_plain": round(t_yaw / t_plain, 4),
                     "rotation_pass_ms": round(t_rot, 4), "rotation_pass_bytes": b,
                     "rotation_pass_fma": fma_per_sample(4, cplx) * nsamp,
                     "rotation_pass_frac_of_hbm_peak": round(b / (t_rot * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4) if t_rot > 0 else None}
        del d_sig, d_out, d_traj
        torch.cuda.empty_cache()
    # order 15, real, one rotation per sample, host arrays
    N, C15 = 15, 256
    x = np.asfortranarray(np.random.default_rng(15).standard_normal((n15, C15)))
    y = np.zeros_like(x)
    t = np.linspace(0, 10, n15)
    a15 = [np.ascontiguousarray(a) for a in (2.0 * np.sin(0.3 * t), 1.7 * np.sin(0.21 * t), 0.8 * np.cos(0.17 * t))]
    call = lambda: L.check(lib.emagls_rotate_sh(x.ctypes.data_as(C.c_void_p), 0, n15, C15, 0,   # noqa: E731
                                                *[q for a in a15 for q in (a.ctypes.data_as(C.c_void_p), n15)], y.ctypes.data_as(C.c_void_p)))
    t15 = _median_ms(call, max(3, reps // 2))
    b15, f15 = pass_bytes(n15, C15, False), fma_per_sample(N, False) * n15
    res["order15"] = {"samples": n15, "channels": C15, "host_call_ms": round(t15, 4), "bytes": b15, "fma": f15,
                      "hbm_bound_ms": round(b15 / (HBM_PEAK_GBPS * 1e9) * 1e3, 4),
                      "fp64_bound_ms": round(2 * f15 / (FP64_PEAK_TFLOPS * 1e12) * 1e3, 4)}
    return res


def markdown(res):
    s = res["shape"]
    lines = ["# Three-axis rotation: timings", "",
             "`python tools/rotate3_timing.py` on %s; median wall-clock per call, buffers in HBM." % res["device"], "",
             "Order 4: %d samples (100 s at 48 kHz) x %d SH channels x %d taps, both ears:" % (s["samples"], s["channels"], s["taps"]), "",
             "| signal | plain decode ms | fixed ypr ms (ratio) | ypr trajectory ms (ratio) | yaw trajectory ms (ratio) | pass ms | pass share of HBM peak |",
             "|---|---|---|---|---|---|---|"]
    for k in ("real", "complex"):
        r = res[k]
        lines.append("| %s | %.3f | %.3f (%.3f) | %.3f (%.3f) | %.3f (%.3f) | %.3f | %s |" % (
            k, r["plain_ms"], r["fixed_ms"], r["fixed_over_plain"], r["trajectory_ms"], r["trajectory_over_plain"], r["yaw_trajectory_ms"],
            r["yaw_trajectory_over_plain"], r["rotation_pass_ms"],
            "%.1f %%" % (100 * r["rotation_pass_frac_of_hbm_peak"]) if r["rotation_pass_frac_of_hbm_peak"] else "-"))
    o = res["order15"]
    lines += ["", "Order 15, real, %d samples x %d channels, one rotation per sample: %.3f ms per host call (copies included); "
              "%.2f GB and %.2f G FMA, bounds %.3f ms (HBM) and %.3f ms (FP64)." % (o["samples"], o["channels"], o["host_call_ms"],
                                                                                  o["bytes"] / 1e9, o["fma"] / 1e9, o["hbm_bound_ms"], o["fp64_bound_ms"]),
              "", "```json", json.dumps(res, indent=1), "```", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="markdown report (profiles/r08_rotate3.md)")
    a = ap.parse_args()
    res = run(a.reps)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(markdown(res))


if __name__ == "__main__":
    main()
