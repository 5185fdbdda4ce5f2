"""Timing of the decode stream (emagls_decode_stream_push_device) against what the library offered before it for the same job:
emagls_binaural_decode_render_ypr_device on the window of the last len - 1 + B samples with their angles, once per block.  Both in
one process, alternating, buffers resident in HBM; device events around runs of `run` pushes, `blocks` blocks per shape and side
after `warm` warm ones.  Per shape (C, len, B), without rotation and with a three-axis trajectory:

  (a) stream   median / p99 time per block of push_device (enqueued back to back, no synchronise inside a run)
  (b) window   the same of the offline device entry (which synchronises its stream at every call)

Gates (exit status 1 when one fails): median (a) < median (b), and median (a) < B / 48000 s, the block's own duration.

    python tools/decode_stream_timing.py [--blocks 2000] [--warm 50] [--run 100] [--shapes 25,512,64 ...] [--stream-only]
                                         [--dry-run] [--out profiles/r10_decode_stream.md]
                                         [--bank [--sets 3]] [--group [--listeners 1 8 64 256] [--sets 1]]
                                         [--encoded [--enc-shapes 32,25,512,64 ...] [--listeners 1 8 64]]
                                         [--field [--field-shapes 1,25,48000,64,1 ...]]
                                         [--field-bank [--field-shapes 1,25,48000,64 ...] [--sets 3 64]]
--dry-run prints the shapes and the bytes a push moves, computed from the shapes, without a device.

--bank times the bank of filter sets (emagls_decode_stream_create_bank / _push_sets_device) instead, without
rotation, per shape and alternating in one process, every side on streams of its own:

  plain    the plain stream (emagls_decode_stream_create): the kernel instance without the bank
  const    a bank stream of --sets sets with a constant index read from device memory (the kernels decide that it stands)
  keep     a bank stream pushed without an index (the host knows that the set stands and runs the plain instance)
  switch   a bank stream with a new set in EVERY block
  three    what a caller has to do without the bank for the output of `switch`: three plain streams, the block weighted by r and
           by 1 - r on the device (two torch.mul) for the new and the old set, a zero block for the third (its pending tails
           still have to come out), and the three outputs added on the device (two torch.add)

spread = p90 - p10 of a side's run averages.  Gates: (a) median(const) <= median(plain) + its spread: a constant index is meant to
be the plain stream's arithmetic; (b) median(switch) <= median(three) + the spread of `three`.  A shape that misses a gate is
reported as such and the exit status is 1.

--group times the listener group (emagls_decode_group_push_device) per shape, number of listeners
(--listeners) and rotation, alternating in one process on one HIP stream:

  group    one push of the common block for L listeners
  loop     what a caller does without the group: L plain decode streams (bank streams with --sets > 1) pushed one after the other

Every listener has angles of their own; with --sets S > 1 every listener switches to a new set in every block (indices in device
memory).  --run pushes per run average (default 100), --blocks / --run run averages per side (default 2000 / 100 = 20); median and
spread = p90 - p10 of the run averages.  Gates: L >= 8: median(loop) - median(group) > spread(loop) + spread(group); L == 1:
median(group) <= median(loop) + spread(loop).  Also reported: loop / group, the listeners one device serves in real time at 48 kHz,
block duration / (group time / L), and the traffic of a push of the whole group, from the shapes.

--encoded times the encoder inside the stream (emagls_decode_stream_create_encoded / emagls_decode_group_create_encoded, DESIGN.md
section 9.6) per shape (M, C, len, B) (--enc-shapes) and number of listeners (--listeners; 1: a stream), with three-axis
trajectories, alternating in one process on one HIP stream:

  encoded  the encoded stream (group) pushed the microphone block [M][B]
  matmul   what a caller does without it: torch.matmul(enc, block) and a push of the result on a plain stream (group)
  plain    the plain stream (group) alone, pushed an SH block: the instances this feature leaves untouched

Median and spread = p90 - p10 of the run averages.  Expected, reported and not gated: median(matmul) - median(encoded) >
spread(matmul) + spread(encoded) at the launch-bound shapes.

--field times the field stream (emagls_field_stream_push_device) per shape (nsrc, nch, nr, B, listeners)
(--field-shapes), alternating in one process on one HIP stream:

  field    the field stream alone: its two launches per block
  chain    the field stream into a decode stream (listeners == 1) or a listener group of 512-tap filters with a three-axis
           trajectory per listener, the field block handed over on the device

Median and spread = p90 - p10 of the run averages.  The one condition: median(chain) < B / 48000 s, the block's own duration; a
shape that misses it is reported as such and the exit status is 1.  Also reported: the share of the block's duration the chain
takes, and the bytes of the response spectra Rf the product kernel streams per block over the time of `field` (both launches: a
lower bound of that kernel's own rate), as a share of the HBM peak.

--field-bank times the bank of response sets on a field stream (emagls_field_stream_create_bank / _push_sets_device, DESIGN.md
section 9.8) per shape (nsrc, nch, nr, B) (--field-shapes) and bank size (--sets), alternating in one process, every side on
objects of its own:

  plain    a plain field stream: the kernel instances without the bank
  const    a bank stream with a constant index per source read from device memory
  keep     a bank stream pushed without indices
  switch   a bank stream with a new set for every source in EVERY block
  streams  what a caller does without the bank for the output of `switch`: three plain field streams, the source blocks weighted
           by r and by 1 - r on the device for the new and the old set, a zero block for the third (its tail still has to come
           out), and the three outputs added on the device.  A lower bound: with P blocks of history more positions are audible

Median and spread = p90 - p10 of the run averages, as --bank.  Reported and not gated: const / plain and keep / plain against the
plain stream's spread, and whether switch is below streams.  A bank beyond the library's 4 GiB of response spectra is listed as
refused.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0   # MI355X HBM3E, nominal
FS = 48000.0
SHAPES = [(25, 512, 64), (25, 512, 256), (25, 2048, 64), (25, 2048, 1024), (64, 2048, 128), (256, 512, 128)]


def push_bytes(Cc, ln, B, rotated):
    """Bytes one block moves, from the shapes (real signal): the partition spectra once, the ring read and written, the block and
    the previous block read, the block kept, the output; with a rotation its pass over the block and the three angles."""
    P, Pf = -(-ln // B), B + 1
    filt = 16 * 2 * P * Cc * Pf
    ring = 2 * 16 * 2 * P * Pf
    sig = 8 * Cc * B * 3 + 8 * 2 * B
    rot = (2 * 8 * Cc * B + 3 * 8 * B) if rotated else 0
    return {"filters": filt, "ring": ring, "signal": sig, "rotation": rot, "total": filt + ring + sig + rot}


def parse_shapes(items):
    if not items:
        return SHAPES
    out = []
    for it in items:
        c, ln, b = (int(v) for v in it.split(","))
        if b < 64 or b > 2048 or b & (b - 1):
            raise SystemExit("block size %d is not a power of two from 64 to 2048" % b)
        if c < 1 or ln < 1:
            raise SystemExit("bad shape %s" % it)
        out.append((c, ln, b))
    return out


def run_shape(lib, L, torch, Cc, ln, B, rotated, blocks, warm, run, stream_only):
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(Cc + ln + B)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)   # noqa: E731
    wL, wR = rnd(Cc, ln), rnd(Cc, ln)                       # [C][len] row-major == [len x C] column-major
    nwin = ln - 1 + B
    d_win, d_wL, d_wR = rnd(Cc, nwin).to(dev), wL.to(dev), wR.to(dev)
    d_blk = d_win[:, -B:].contiguous()
    ang = [(0.3 + 0.01 * torch.cumsum(rnd(nwin), 0)).to(dev) for _ in range(3)]
    ang_blk = [a[-B:].contiguous() for a in ang]
    d_out_a = torch.zeros((2, B), dtype=torch.float64, device=dev)
    d_out_b = torch.zeros((2, nwin), dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    h = C.c_void_p()
    L.check(lib.emagls_decode_stream_create(Cc, C.c_void_p(wL.data_ptr()), C.c_void_p(wR.data_ptr()), 0, ln, 0, L.LAYOUT["sh"], L.BASIS["real"],
                                            B, C.byref(h)))
    st = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(st.cuda_stream)
    na, nb = (B, nwin) if rotated else (0, 0)
    aa = [p(a) if rotated else None for a in ang_blk]
    ab = [p(a) if rotated else None for a in ang]

    def side_a():
        L.check(lib.emagls_decode_stream_push_device(h, p(d_blk), B, aa[0], na, aa[1], na, aa[2], na, p(d_out_a), sp))

    def side_b():
        L.check(lib.emagls_binaural_decode_render_ypr_device(p(d_win), 0, nwin, Cc, p(d_wL), p(d_wR), 0, ln, L.LAYOUT["sh"], L.BASIS["real"],
                                                             ab[0], nb, ab[1], nb, ab[2], nb, None, 0, p(d_out_b), None, sp))

    sides = [("stream", side_a)] + ([] if stream_only else [("window", side_b)])
    times = {k: [] for k, _ in sides}
    with torch.cuda.stream(st):
        for _, f in sides:
            for _ in range(warm):
                f()
        st.synchronize()
        for _ in range(max(1, blocks // run)):
            for k, f in sides:                       # alternating
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(run):
                    f()
                e1.record(st)
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / run)   # us per block
    L.check(lib.emagls_decode_stream_destroy(h))
    res = {"shape": [Cc, ln, B], "rotation": "ypr" if rotated else "none", "block_us": round(B / FS * 1e6, 1),
           "bytes": push_bytes(Cc, ln, B, rotated)}
    for k, v in times.items():
        res[k] = {"median_us": round(float(np.median(v)), 2), "p99_us": round(float(np.percentile(v, 99)), 2), "min_us": round(float(np.min(v)), 2),
                  "spread_us": round(float(np.percentile(v, 90) - np.percentile(v, 10)), 2)}
    if "window" in res:
        res["window_over_stream"] = round(res["window"]["median_us"] / res["stream"]["median_us"], 2)
    return res


def _spread(v):
    return float(np.percentile(v, 90) - np.percentile(v, 10))


def run_bank_shape(lib, L, torch, Cc, ln, B, S, blocks, warm, run):
    """The sides of --bank for one shape."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(Cc + ln + B)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)   # noqa: E731
    wL, wR = rnd(S, Cc, ln), rnd(S, Cc, ln)                 # [S][C][len] row-major == S column-major [len x C] arrays
    d_blk = rnd(Cc, B).to(dev)
    r = ((torch.arange(B, dtype=torch.float64) + 1) / B).to(dev)
    omr = 1.0 - r
    xa, xb, zero = torch.empty_like(d_blk), torch.empty_like(d_blk), torch.zeros_like(d_blk)
    outs = [torch.zeros((2, B), dtype=torch.float64, device=dev) for _ in range(4)]
    d_idx = torch.arange(S, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    st = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(st.cuda_stream)
    sh, re = L.LAYOUT["sh"], L.BASIS["real"]

    def plain_stream(s):
        h = C.c_void_p()
        L.check(lib.emagls_decode_stream_create(Cc, p(wL[s]), p(wR[s]), 0, ln, 0, sh, re, B, C.byref(h)))
        return h

    def push(h, x, out):
        L.check(lib.emagls_decode_stream_push_device(h, p(x), B, None, 0, None, 0, None, 0, p(out), sp))

    def bank_stream():
        h = C.c_void_p()
        L.check(lib.emagls_decode_stream_create_bank(Cc, S, p(wL), p(wR), 0, ln, 0, sh, re, B, C.byref(h)))
        return h

    h_plain = plain_stream(0)
    h_three = [plain_stream(s) for s in range(3)]
    h_const, h_keep, h_switch = bank_stream(), bank_stream(), bank_stream()   # (a stream each: a side's index history is its own)
    count = [0]

    def side_const():
        L.check(lib.emagls_decode_stream_push_sets_device(h_const, p(d_blk), B, C.c_void_p(d_idx.data_ptr() + 4), 1, None, 0, None, 0, None, 0,
                                                          p(outs[0]), sp))

    def side_keep():
        L.check(lib.emagls_decode_stream_push_sets_device(h_keep, p(d_blk), B, None, 0, None, 0, None, 0, None, 0, p(outs[0]), sp))

    def side_switch():
        count[0] += 1
        L.check(lib.emagls_decode_stream_push_sets_device(h_switch, p(d_blk), B, C.c_void_p(d_idx.data_ptr() + 4 * (count[0] % S)), 1, None, 0, None,
                                                          0, None, 0, p(outs[0]), sp))

    def side_three():
        count[0] += 1
        new, prev, third = count[0] % 3, (count[0] - 1) % 3, (count[0] + 1) % 3
        torch.mul(d_blk, r, out=xa)
        torch.mul(d_blk, omr, out=xb)
        push(h_three[new], xa, outs[1])
        push(h_three[prev], xb, outs[2])
        push(h_three[third], zero, outs[3])
        torch.add(outs[1], outs[2], out=outs[0])
        outs[0].add_(outs[3])

    sides = [("plain", lambda: push(h_plain, d_blk, outs[0])), ("const", side_const), ("keep", side_keep), ("switch", side_switch),
             ("three", side_three)]
    times = {k: [] for k, _ in sides}
    with torch.cuda.stream(st):
        for _, f in sides:
            for _ in range(warm):
                f()
        st.synchronize()
        for _ in range(max(1, blocks // run)):
            for k, f in sides:                       # alternating
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(run):
                    f()
                e1.record(st)
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / run)   # us per block
    for h in [h_plain, h_const, h_keep, h_switch] + h_three:
        lib.emagls_decode_stream_destroy(h)
    res = {"shape": [Cc, ln, B], "sets": S, "block_us": round(B / FS * 1e6, 1)}
    for k, v in times.items():
        res[k] = {"median_us": round(float(np.median(v)), 2), "min_us": round(float(np.min(v)), 2), "max_us": round(float(np.max(v)), 2),
                  "spread_us": round(_spread(v), 2)}
    base = res["plain"]
    res["const_over_plain"] = round(res["const"]["median_us"] / base["median_us"], 3)
    res["keep_over_plain"] = round(res["keep"]["median_us"] / base["median_us"], 3)
    res["three_over_switch"] = round(res["three"]["median_us"] / res["switch"]["median_us"], 2)
    res["switch_over_const"] = round(res["switch"]["median_us"] / res["const"]["median_us"], 2)
    res["gate_a"] = res["const"]["median_us"] <= base["median_us"] + base["spread_us"]
    res["gate_b"] = res["switch"]["median_us"] <= res["three"]["median_us"] + res["three"]["spread_us"]
    return res


def group_bytes(Cc, ln, B, L, S, rotated):
    """Bytes a push of the group moves, from the shapes (real signal).  `state`: per listener, L times -- ring read and written,
    the previous block read, the block read twice and kept, the output; with a rotation the rotated block written and the three
    angles read.  `filters`: the spectra of one set, which every listener's workgroups read but which are stored once (after the
    first listener they can come from the caches).  `common`: the block itself, once."""
    P, Pf = -(-ln // B), B + 1
    filt = 16 * 2 * P * Cc * Pf
    per = 2 * 16 * 2 * P * Pf + 8 * Cc * B * 4 + 8 * 2 * B + ((8 * Cc * B + 3 * 8 * B) if rotated else 0)
    return {"filters_once": filt, "state": L * per, "common": 8 * Cc * B, "compulsory": filt + L * per + 8 * Cc * B,
            "requested": L * filt + L * per + 8 * Cc * B}


def run_group_shape(lib, L, torch, Cc, ln, B, nl, S, rotated, blocks, warm, run):
    """The sides of --group for one shape, nl listeners."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(Cc + ln + B)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)   # noqa: E731
    wL, wR = rnd(S, Cc, ln), rnd(S, Cc, ln)                 # [S][C][len] row-major == S column-major [len x C] arrays
    d_blk = rnd(Cc, B).to(dev)
    ang = [(0.3 + 0.01 * torch.cumsum(rnd(nl, B), 1)).to(dev) for _ in range(3)]          # [L][B] per angle
    d_idx = (torch.arange(S, dtype=torch.int32)[:, None] + torch.arange(nl, dtype=torch.int32)[None, :]).remainder(S).to(dev).contiguous()
    out_g = torch.zeros((nl, 2, B), dtype=torch.float64, device=dev)
    out_l = torch.zeros((nl, 2, B), dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    st = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(st.cuda_stream)
    sh, re = L.LAYOUT["sh"], L.BASIS["real"]
    hg = C.c_void_p()
    L.check(lib.emagls_decode_group_create(Cc, S, p(wL), p(wR), 0, ln, 0, sh, re, B, nl, C.byref(hg)))
    hs = []
    for _ in range(nl):
        h = C.c_void_p()
        L.check(lib.emagls_decode_stream_create_bank(Cc, S, p(wL), p(wR), 0, ln, 0, sh, re, B, C.byref(h)))
        hs.append(h)
    na_g, na_l = (nl * B, B) if rotated else (0, 0)
    ag = [p(a) if rotated else None for a in ang]
    al = [[C.c_void_p(a.data_ptr() + 8 * B * l) if rotated else None for a in ang] for l in range(nl)]
    outs = [C.c_void_p(out_l.data_ptr() + 8 * 2 * B * l) for l in range(nl)]
    count = [0, 0]

    def side_group():
        count[0] += 1
        idx = C.c_void_p(d_idx.data_ptr() + 4 * nl * (count[0] % S)) if S > 1 else None   # row count % S: [L] indices, a new set each
        L.check(lib.emagls_decode_group_push_device(hg, p(d_blk), B, idx, nl if S > 1 else 0, ag[0], na_g, ag[1], na_g, ag[2], na_g,
                                                    p(out_g), sp))

    def side_loop():
        count[1] += 1
        for l in range(nl):
            idx = C.c_void_p(d_idx.data_ptr() + 4 * (nl * (count[1] % S) + l)) if S > 1 else None
            L.check(lib.emagls_decode_stream_push_sets_device(hs[l], p(d_blk), B, idx, 1 if S > 1 else 0, al[l][0], na_l, al[l][1], na_l,
                                                              al[l][2], na_l, outs[l], sp))

    sides = [("group", side_group), ("loop", side_loop)]
    times = {k: [] for k, _ in sides}
    with torch.cuda.stream(st):
        for _, f in sides:
            for _ in range(warm):
                f()
        st.synchronize()
        same = bool(torch.equal(out_g, out_l))              # equal histories so far: the two sides hold the same bits
        for _ in range(max(1, blocks // run)):
            for k, f in sides:                               # alternating
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(run):
                    f()
                e1.record(st)
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / run)   # us per block of the whole group
    lib.emagls_decode_group_destroy(hg)
    for h in hs:
        lib.emagls_decode_stream_destroy(h)
    res = {"shape": [Cc, ln, B], "listeners": nl, "sets": S, "rotation": "ypr" if rotated else "none", "block_us": round(B / FS * 1e6, 1),
           "bits_equal": same, "bytes": group_bytes(Cc, ln, B, nl, S, rotated)}
    for k, v in times.items():
        res[k] = {"median_us": round(float(np.median(v)), 2), "min_us": round(float(np.min(v)), 2), "max_us": round(float(np.max(v)), 2),
                  "spread_us": round(_spread(v), 2)}
    gm, lm = res["group"]["median_us"], res["loop"]["median_us"]
    res["loop_over_group"] = round(lm / gm, 2)
    res["listeners_in_real_time"] = int(res["block_us"] / (gm / nl))
    res["compulsory_gbps"] = round(res["bytes"]["compulsory"] / gm / 1e3, 1)
    res["requested_gbps"] = round(res["bytes"]["requested"] / gm / 1e3, 1)
    if nl >= 8:
        res["gate"] = lm - gm > res["loop"]["spread_us"] + res["group"]["spread_us"]
    elif nl == 1:
        res["gate"] = gm <= lm + res["loop"]["spread_us"]
    else:
        res["gate"] = True
    return res


def group_markdown(rows, device):
    lines = ["`python tools/decode_stream_timing.py --group` on %s: time per block of the WHOLE group in us, median of the run averages" % device,
             "(spread = p90 - p10).  group: one push of `emagls_decode_group_push_device`; loop: L decode streams pushed one after the other",
             "on the same HIP stream.  real time: the listeners one device serves at 48 kHz, block duration / (group / L).  GB/s: the",
             "traffic of a push from the shapes over the group's time; compulsory counts the filter spectra once, requested once per",
             "listener (what the workgroups load, most of it from the caches), against an HBM peak of %.0f GB/s." % HBM_PEAK_GBPS, "",
             "| (C, len, B) | S | rotation | L | group | spread | loop | spread | loop / group | gate | real time | compulsory GB/s | requested GB/s | bits |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %d | %s | %d | %.1f | %.2f | %.1f | %.2f | %.2f | %s | %d | %.0f (%.1f %%) | %.0f (%.1f %%) | %s |" % (
            tuple(r["shape"]), r["sets"], r["rotation"], r["listeners"], r["group"]["median_us"], r["group"]["spread_us"], r["loop"]["median_us"],
            r["loop"]["spread_us"], r["loop_over_group"], "ok" if r["gate"] else "MISS", r["listeners_in_real_time"], r["compulsory_gbps"],
            100 * r["compulsory_gbps"] / HBM_PEAK_GBPS, r["requested_gbps"], 100 * r["requested_gbps"] / HBM_PEAK_GBPS,
            "equal" if r["bits_equal"] else "DIFFER"))
    return "\n".join(lines) + "\n"


def run_encoded_shape(lib, L, torch, M, Cc, ln, B, nl, blocks, warm, run):
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(M + Cc + ln + B + nl)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)   # noqa: E731
    wL, wR = rnd(Cc, ln), rnd(Cc, ln)                       # [C][len] row-major == [len x C] column-major
    enc = rnd(Cc, M) / M ** 0.5                             # [C][M]; the library takes [C x M] column-major: its transpose's memory
    enc_cm = enc.t().contiguous()
    d_enc = enc.to(dev)
    d_mic = rnd(M, B).to(dev)                               # [M][B] == [B x M] column-major
    d_sh = torch.matmul(d_enc, d_mic)
    ang = [(0.3 + 0.01 * torch.cumsum(rnd(nl, B), 1)).to(dev) for _ in range(3)]
    d_out = [torch.zeros((nl, 2, B), dtype=torch.float64, device=dev) for _ in range(3)]
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    hp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    sh, real = L.LAYOUT["sh"], L.BASIS["real"]
    h = [C.c_void_p() for _ in range(3)]                    # encoded, the plain one behind the matmul, plain
    if nl == 1:
        L.check(lib.emagls_decode_stream_create_encoded(M, hp(enc_cm), 0, Cc, 1, hp(wL), hp(wR), 0, ln, sh, real, B, C.byref(h[0])))
        for k in (1, 2):
            L.check(lib.emagls_decode_stream_create(Cc, hp(wL), hp(wR), 0, ln, 0, sh, real, B, C.byref(h[k])))
    else:
        L.check(lib.emagls_decode_group_create_encoded(M, hp(enc_cm), 0, Cc, 1, hp(wL), hp(wR), 0, ln, sh, real, B, nl, C.byref(h[0])))
        for k in (1, 2):
            L.check(lib.emagls_decode_group_create(Cc, 1, hp(wL), hp(wR), 0, ln, 0, sh, real, B, nl, C.byref(h[k])))
    st = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(st.cuda_stream)
    na = nl * B
    aa = [p(a) for a in ang]

    def push(k, x):
        if nl == 1:
            L.check(lib.emagls_decode_stream_push_device(h[k], p(x), B, aa[0], na, aa[1], na, aa[2], na, p(d_out[k]), sp))
        else:
            L.check(lib.emagls_decode_group_push_device(h[k], p(x), B, None, 0, aa[0], na, aa[1], na, aa[2], na, p(d_out[k]), sp))

    def side_matmul():
        push(1, torch.matmul(d_enc, d_mic))

    sides = [("encoded", lambda: push(0, d_mic)), ("matmul", side_matmul), ("plain", lambda: push(2, d_sh))]
    times = {k: [] for k, _ in sides}
    with torch.cuda.stream(st):
        for _, f in sides:
            for _ in range(warm):
                f()
        st.synchronize()
        for _ in range(max(1, blocks // run)):
            for k, f in sides:                       # alternating
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(run):
                    f()
                e1.record(st)
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / run)   # us per block
    st.synchronize()
    err = float((d_out[0] - d_out[1]).abs().max() / d_out[1].abs().max())   # (both sides have seen the same pushes)
    for k in range(3):
        L.check((lib.emagls_decode_stream_destroy if nl == 1 else lib.emagls_decode_group_destroy)(h[k]))
    res = {"shape": [M, Cc, ln, B], "listeners": nl, "block_us": round(B / FS * 1e6, 1), "encoded_vs_matmul_rel": err}
    for k, v in times.items():
        res[k] = {"median_us": round(float(np.median(v)), 2), "spread_us": round(float(np.percentile(v, 90) - np.percentile(v, 10)), 2)}
    res["gain_us"] = round(res["matmul"]["median_us"] - res["encoded"]["median_us"], 2)
    res["beyond_spreads"] = res["gain_us"] > res["matmul"]["spread_us"] + res["encoded"]["spread_us"]
    return res


def encoded_markdown(rows, device):
    lines = ["`python tools/decode_stream_timing.py --encoded` on %s: time per block in us, median of the run averages (spread = p90 - p10)," % device,
             "three-axis trajectories.  encoded: the encoded stream (group) pushed the microphone block; matmul: torch.matmul(enc, block) and",
             "a push on a plain stream (group), on the same HIP stream; plain: the plain stream (group) alone.", "",
             "| (M, C, len, B) | listeners | encoded | spread | matmul | spread | matmul - encoded | beyond the spreads | plain | spread |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %d | %.1f | %.2f | %.1f | %.2f | %.2f | %s | %.1f | %.2f |" % (
            tuple(r["shape"]), r["listeners"], r["encoded"]["median_us"], r["encoded"]["spread_us"], r["matmul"]["median_us"],
            r["matmul"]["spread_us"], r["gain_us"], "yes" if r["beyond_spreads"] else "no", r["plain"]["median_us"], r["plain"]["spread_us"]))
    return "\n".join(lines) + "\n"


FIELD_SHAPES = ["1,25,48000,64,1", "1,25,96000,256,1", "4,64,48000,128,1", "1,25,48000,64,8"]
FIELD_BANK_SHAPES = ["1,25,48000,64", "1,25,96000,256", "4,64,48000,128"]
FIELD_DECODE_TAPS = 512


def field_bytes(nsrc, nch, nr, B):
    """Bytes one block of the field stream moves, from the shapes (real response): the response spectra once, the ring read by
    every pair of planes (stored once: `ring_once`) and one slot written, the blocks and the previous blocks, the output."""
    P, Pf = -(-nr // B), B + 1
    rf = 16 * nsrc * P * nch * Pf
    ring = 16 * nsrc * P * Pf
    return {"response": rf, "ring_once": ring, "ring_requested": ring * ((nch + 1) // 2), "slot": 16 * nsrc * Pf, "signal": 8 * nsrc * B * 3,
            "output": 8 * nch * B, "compulsory": rf + ring + 16 * nsrc * Pf + 8 * nsrc * B * 3 + 8 * nch * B}


def run_field_shape(lib, L, torch, nsrc, nch, nr, B, nl, blocks, warm, run):
    """The sides of --field for one shape."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(nsrc + nch + nr + B + nl)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)   # noqa: E731
    rir = rnd(nsrc, nch, nr) / nr ** 0.5                    # [nsrc][nch][nr] row-major == nsrc column-major [nr x nch] arrays
    ln = FIELD_DECODE_TAPS
    wL, wR = rnd(nch, ln), rnd(nch, ln)
    d_src = rnd(nsrc, B).to(dev)
    ang = [(0.3 + 0.01 * torch.cumsum(rnd(nl, B), 1)).to(dev) for _ in range(3)]
    d_field = [torch.zeros((nch, B), dtype=torch.float64, device=dev) for _ in range(2)]
    d_out = torch.zeros((nl, 2, B), dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    sh, real = L.LAYOUT["sh"], L.BASIS["real"]
    hf = [C.c_void_p(), C.c_void_p()]                       # a field stream per side: a side's history is its own
    for h in hf:
        L.check(lib.emagls_field_stream_create(nsrc, nch, p(rir), 0, nr, B, C.byref(h)))
    hd = C.c_void_p()
    if nl == 1:
        L.check(lib.emagls_decode_stream_create(nch, p(wL), p(wR), 0, ln, 0, sh, real, B, C.byref(hd)))
    else:
        L.check(lib.emagls_decode_group_create(nch, 1, p(wL), p(wR), 0, ln, 0, sh, real, B, nl, C.byref(hd)))
    st = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(st.cuda_stream)
    na = nl * B
    aa = [p(a) for a in ang]

    def side_field():
        L.check(lib.emagls_field_stream_push_device(hf[0], p(d_src), B, p(d_field[0]), sp))

    def side_chain():
        L.check(lib.emagls_field_stream_push_device(hf[1], p(d_src), B, p(d_field[1]), sp))
        if nl == 1:
            L.check(lib.emagls_decode_stream_push_device(hd, p(d_field[1]), B, aa[0], na, aa[1], na, aa[2], na, p(d_out), sp))
        else:
            L.check(lib.emagls_decode_group_push_device(hd, p(d_field[1]), B, None, 0, aa[0], na, aa[1], na, aa[2], na, p(d_out), sp))

    sides = [("field", side_field), ("chain", side_chain)]
    times = {k: [] for k, _ in sides}
    with torch.cuda.stream(st):
        for _, f in sides:
            for _ in range(warm):
                f()
        st.synchronize()
        for _ in range(max(1, blocks // run)):
            for k, f in sides:                       # alternating
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(run):
                    f()
                e1.record(st)
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / run)   # us per block
    st.synchronize()
    same = bool(torch.equal(d_field[0], d_field[1]))        # (both field streams have seen the same pushes)
    for h in hf:
        L.check(lib.emagls_field_stream_destroy(h))
    L.check((lib.emagls_decode_stream_destroy if nl == 1 else lib.emagls_decode_group_destroy)(hd))
    res = {"shape": [nsrc, nch, nr, B], "listeners": nl, "partitions": -(-nr // B), "block_us": round(B / FS * 1e6, 1), "bits_equal": same,
           "bytes": field_bytes(nsrc, nch, nr, B)}
    for k, v in times.items():
        res[k] = {"median_us": round(float(np.median(v)), 2), "min_us": round(float(np.min(v)), 2), "max_us": round(float(np.max(v)), 2),
                  "spread_us": round(_spread(v), 2)}
    res["chain_share_of_block"] = round(res["chain"]["median_us"] / res["block_us"], 4)
    res["response_gbps"] = round(res["bytes"]["response"] / res["field"]["median_us"] / 1e3, 1)
    res["response_share_of_hbm_peak"] = round(res["response_gbps"] / HBM_PEAK_GBPS, 4)
    res["gate_realtime"] = res["chain"]["median_us"] < res["block_us"]
    return res


def field_markdown(rows, device):
    lines = ["`python tools/decode_stream_timing.py --field` on %s: time per block in us, median of the run averages (spread = p90 - p10)." % device,
             "field: `emagls_field_stream_push_device` alone (two launches); chain: the same into a decode stream, or a listener group of L",
             "listeners, of %d-tap filters with a three-axis trajectory per listener.  share: chain over the block's duration at 48 kHz" % FIELD_DECODE_TAPS,
             "(the condition: below 100 %).  Rf GB/s: the bytes of the response spectra the product kernel streams per block over the time",
             "of `field` (both launches, so a lower bound of that kernel's rate), against an HBM peak of %.0f GB/s." % HBM_PEAK_GBPS, "",
             "| (nsrc, nch, nr, B) | L | P | block us | field | spread | chain | spread | share | real time | Rf MB | Rf GB/s | of HBM peak |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %d | %d | %.0f | %.1f | %.2f | %.1f | %.2f | %.1f %% | %s | %.1f | %.0f | %.1f %% |" % (
            tuple(r["shape"]), r["listeners"], r["partitions"], r["block_us"], r["field"]["median_us"], r["field"]["spread_us"],
            r["chain"]["median_us"], r["chain"]["spread_us"], 100 * r["chain_share_of_block"], "ok" if r["gate_realtime"] else "MISS",
            r["bytes"]["response"] / 1e6, r["response_gbps"], 100 * r["response_share_of_hbm_peak"]))
    return "\n".join(lines) + "\n"


def parse_field_shapes(items):
    out = []
    for it in items:
        nsrc, nch, nr, b, nl = (int(v) for v in it.split(","))
        parse_shapes(["%d,%d,%d" % (nch, nr, b)])
        if not (1 <= nsrc <= 16 and nch <= 256 and nr <= 1048576 and 1 <= nl <= 4096):
            raise SystemExit("--field-shapes: 1 <= nsrc <= 16, nch <= 256, nr <= 1048576, listeners from 1 to 4096")
        if int(round(nch ** 0.5)) ** 2 != nch or nch > 256:
            raise SystemExit("--field-shapes: the chain's rotation needs (N+1)^2 channels, N <= 15")
        out.append((nsrc, nch, nr, b, nl))
    return out


def run_field_bank_shape(lib, L, torch, nsrc, nch, nr, B, S, blocks, warm, run):
    """The sides of --field-bank for one shape."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(nsrc + nch + nr + B + S)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)   # noqa: E731
    rir = rnd(S, nsrc, nch, nr) / nr ** 0.5                 # [S][nsrc][nch][nr] row-major == S groups of nsrc column-major [nr x nch] arrays
    d_src = rnd(nsrc, B).to(dev)
    r = ((torch.arange(B, dtype=torch.float64) + 1) / B).to(dev)
    omr = 1.0 - r
    xa, xb, zero = torch.empty_like(d_src), torch.empty_like(d_src), torch.zeros_like(d_src)
    outs = [torch.zeros((nch, B), dtype=torch.float64, device=dev) for _ in range(4)]
    d_const = torch.ones(nsrc, dtype=torch.int32, device=dev)
    # row c: the indices of block c, a new set for every source
    d_idx = ((torch.arange(S).reshape(S, 1) + torch.arange(nsrc).reshape(1, nsrc)) % S).to(torch.int32).to(dev).contiguous()
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    st = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(st.cuda_stream)

    def plain_stream(s):
        h = C.c_void_p()
        L.check(lib.emagls_field_stream_create(nsrc, nch, p(rir[s]), 0, nr, B, C.byref(h)))
        return h

    def bank_stream():
        h = C.c_void_p()
        L.check(lib.emagls_field_stream_create_bank(nsrc, nch, S, p(rir), 0, nr, B, C.byref(h)))
        return h

    def push(h, x, out):
        L.check(lib.emagls_field_stream_push_device(h, p(x), B, p(out), sp))

    def push_sets(h, sets):
        L.check(lib.emagls_field_stream_push_sets_device(h, p(d_src), B, sets, nsrc if sets else 0, p(outs[0]), sp))

    h_plain = plain_stream(0)
    h_three = [plain_stream(s) for s in range(3)]
    h_const, h_keep, h_switch = bank_stream(), bank_stream(), bank_stream()   # (an object each: a side's index history is its own)
    count = [0]

    def side_switch():
        count[0] += 1
        push_sets(h_switch, C.c_void_p(d_idx.data_ptr() + 4 * nsrc * (count[0] % S)))

    def side_streams():
        count[0] += 1
        new, prev, third = count[0] % 3, (count[0] - 1) % 3, (count[0] + 1) % 3
        torch.mul(d_src, r, out=xa)
        torch.mul(d_src, omr, out=xb)
        push(h_three[new], xa, outs[1])
        push(h_three[prev], xb, outs[2])
        push(h_three[third], zero, outs[3])
        torch.add(outs[1], outs[2], out=outs[0])
        outs[0].add_(outs[3])

    sides = [("plain", lambda: push(h_plain, d_src, outs[0])), ("const", lambda: push_sets(h_const, p(d_const))),
             ("keep", lambda: push_sets(h_keep, None)), ("switch", side_switch), ("streams", side_streams)]
    times = {k: [] for k, _ in sides}
    with torch.cuda.stream(st):
        for _, f in sides:
            for _ in range(warm):
                f()
        st.synchronize()
        for _ in range(max(1, blocks // run)):
            for k, f in sides:                       # alternating
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(run):
                    f()
                e1.record(st)
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / run)   # us per block
    for h in [h_plain, h_const, h_keep, h_switch] + h_three:
        lib.emagls_field_stream_destroy(h)
    fb = field_bytes(nsrc, nch, nr, B)
    res = {"shape": [nsrc, nch, nr, B], "sets": S, "partitions": -(-nr // B), "block_us": round(B / FS * 1e6, 1),
           "response_mb_per_set": round(fb["response"] / 1e6, 1)}
    for k, v in times.items():
        res[k] = {"median_us": round(float(np.median(v)), 2), "min_us": round(float(np.min(v)), 2), "max_us": round(float(np.max(v)), 2),
                  "spread_us": round(_spread(v), 2)}
    base = res["plain"]
    res["const_over_plain"] = round(res["const"]["median_us"] / base["median_us"], 3)
    res["keep_over_plain"] = round(res["keep"]["median_us"] / base["median_us"], 3)
    res["const_within_spread"] = res["const"]["median_us"] <= base["median_us"] + base["spread_us"]
    res["keep_within_spread"] = res["keep"]["median_us"] <= base["median_us"] + base["spread_us"]
    res["streams_over_switch"] = round(res["streams"]["median_us"] / res["switch"]["median_us"], 2)
    res["switch_over_const"] = round(res["switch"]["median_us"] / res["const"]["median_us"], 2)
    res["bank_wins"] = res["switch"]["median_us"] < res["streams"]["median_us"]
    return res


def field_bank_markdown(rows, device):
    lines = ["`python tools/decode_stream_timing.py --field-bank` on %s: time per block in us, median of the run averages (spread = p90 - p10)." % device,
             "plain: a plain field stream; const: a bank stream with a constant index from device memory; keep: a bank stream pushed",
             "without indices; switch: a new set for every source in every block; streams: three plain field streams fed the",
             "gain-weighted source blocks, outputs added on the device -- a lower bound of what a caller needs without the bank.", "",
             "| (nsrc, nch, nr, B) | sets | P | Rf MB / set | plain | spread | const | spread | const / plain | within | keep | keep / plain | within | switch | spread | streams | spread | streams / switch | bank wins | switch / const |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if "refused" in r:
            lines.append("| %s | %d | %d | %.1f | %s |" % (tuple(r["shape"]), r["sets"], r["partitions"], r["response_mb_per_set"], r["refused"]))
            continue
        lines.append("| %s | %d | %d | %.1f | %.1f | %.2f | %.1f | %.2f | %.3f | %s | %.1f | %.3f | %s | %.1f | %.2f | %.1f | %.2f | %.2f | %s | %.2f |" % (
            tuple(r["shape"]), r["sets"], r["partitions"], r["response_mb_per_set"], r["plain"]["median_us"], r["plain"]["spread_us"],
            r["const"]["median_us"], r["const"]["spread_us"], r["const_over_plain"], "yes" if r["const_within_spread"] else "no",
            r["keep"]["median_us"], r["keep_over_plain"], "yes" if r["keep_within_spread"] else "no", r["switch"]["median_us"],
            r["switch"]["spread_us"], r["streams"]["median_us"], r["streams"]["spread_us"], r["streams_over_switch"],
            "yes" if r["bank_wins"] else "NO", r["switch_over_const"]))
    return "\n".join(lines) + "\n"


def bank_markdown(rows, device):
    lines = ["`python tools/decode_stream_timing.py --bank` on %s: time per block in us, median of the run averages (spread = p90 - p10)." % device,
             "plain: the plain stream; const: a bank stream with a constant index from device memory; keep: a bank stream pushed without",
             "an index; switch: a new set in every block; three: three plain streams fed the gain-weighted blocks, outputs added on the",
             "device.", "",
             "| (C, len, B) | plain | spread | const | spread | const / plain | (a) | keep | keep / plain | switch | three | spread | three / switch | (b) | switch / const |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %.1f | %.2f | %.1f | %.2f | %.3f | %s | %.1f | %.3f | %.1f | %.1f | %.2f | %.2f | %s | %.2f |" % (
            tuple(r["shape"]), r["plain"]["median_us"], r["plain"]["spread_us"], r["const"]["median_us"], r["const"]["spread_us"],
            r["const_over_plain"], "ok" if r["gate_a"] else "MISS", r["keep"]["median_us"], r["keep_over_plain"], r["switch"]["median_us"],
            r["three"]["median_us"], r["three"]["spread_us"], r["three_over_switch"], "ok" if r["gate_b"] else "MISS", r["switch_over_const"]))
    return "\n".join(lines) + "\n"


def markdown(rows, device):
    lines = ["`python tools/decode_stream_timing.py` on %s: time per block in us (median and p99 of the run averages).  stream:" % device,
             "`emagls_decode_stream_push_device`; window: `emagls_binaural_decode_render_ypr_device` on the last len - 1 + B samples.", "",
             "| (C, len, B) | rotation | block us | stream median | stream p99 | window median | window p99 | window / stream | bytes per push |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        w = r.get("window", {"median_us": float("nan"), "p99_us": float("nan")})
        lines.append("| %s | %s | %.0f | %.1f | %.1f | %.1f | %.1f | %s | %d |" % (
            tuple(r["shape"]), r["rotation"], r["block_us"], r["stream"]["median_us"], r["stream"]["p99_us"], w["median_us"], w["p99_us"],
            r.get("window_over_stream", "-"), r["bytes"]["total"]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=2000)
    ap.add_argument("--warm", type=int, default=50)
    ap.add_argument("--run", type=int, default=100)
    ap.add_argument("--shapes", nargs="*", default=None, help="C,len,B ...")
    ap.add_argument("--stream-only", action="store_true", help="only side (a): for a kernel trace of the stream alone")
    ap.add_argument("--rotation", choices=["both", "none", "ypr"], default="both")
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--out", default=None, help="markdown table")
    ap.add_argument("--bank", action="store_true", help="time the bank of filter sets (see above)")
    ap.add_argument("--sets", type=int, nargs="*", default=None,
                    help="--bank: filter sets of the bank stream (at least 3; default 3); --group: default 1; --field-bank: one or more bank sizes, "
                         "each at least 3 (default 3 64)")
    ap.add_argument("--group", action="store_true", help="time the listener group against a loop over streams (see above)")
    ap.add_argument("--listeners", type=int, nargs="*", default=None, help="--group: numbers of listeners (default 1 8 64 256); --encoded: default 1")
    ap.add_argument("--encoded", action="store_true", help="time the encoder inside the stream against matmul + plain stream (see above)")
    ap.add_argument("--enc-shapes", nargs="*", default=["32,25,512,64", "32,25,512,256", "64,64,2048,128"], help="--encoded: M,C,len,B ...")
    ap.add_argument("--field", action="store_true", help="time the field stream alone and its chain into a decode stream (see above)")
    ap.add_argument("--field-shapes", nargs="*", default=None, help="--field: nsrc,nch,nr,B,listeners ...; --field-bank: nsrc,nch,nr,B ...")
    ap.add_argument("--field-bank", action="store_true", help="time the bank of response sets on a field stream (see above)")
    a = ap.parse_args()
    if a.field_bank:
        a.sets = a.sets or [3, 64]
    elif a.sets is not None and len(a.sets) != 1:
        raise SystemExit("--sets takes one number here")
    else:
        a.sets = a.sets[0] if a.sets else (1 if a.group else 3)
    if a.field_shapes is None:
        a.field_shapes = FIELD_BANK_SHAPES if a.field_bank else FIELD_SHAPES
    if a.listeners is None:
        a.listeners = [1] if a.encoded else [1, 8, 64, 256]
    if a.blocks < a.run or a.run < 1 or a.warm < 0:
        raise SystemExit("--blocks must be at least --run, --run at least 1")
    if a.field_bank:
        fshapes = [fs_[:4] for fs_ in parse_field_shapes([it if it.count(",") == 4 else it + ",1" for it in a.field_shapes])]
        if any(S < 3 or S > 65536 for S in a.sets):
            raise SystemExit("--field-bank: --sets from 3 to 65536")
        cases = [(fs_, S) for fs_ in fshapes for S in a.sets]
        if a.dry_run:
            for (nsrc, nch, nr, b), S in cases:
                rf = field_bytes(nsrc, nch, nr, b)["response"]
                print(json.dumps({"shape": [nsrc, nch, nr, b], "sets": S, "partitions": -(-nr // b), "response_bytes": S * rf,
                                  "fits_4_gib": S * rf <= 4 << 30}))
            return 0
        import torch
        from emagls_amd import _lib as L
        lib = L.load()
        rows = []
        for (nsrc, nch, nr, b), S in cases:
            rf = field_bytes(nsrc, nch, nr, b)["response"]
            if S * rf > 4 << 30:    # the library refuses such a bank: the row says so
                res = {"shape": [nsrc, nch, nr, b], "sets": S, "partitions": -(-nr // b), "response_mb_per_set": round(rf / 1e6, 1),
                       "refused": "the bank's response spectra exceed 4 GiB (%.1f GB)" % (S * rf / 1e9)}
            else:
                res = run_field_bank_shape(lib, L, torch, nsrc, nch, nr, b, S, a.blocks, a.warm, a.run)
            rows.append(res)
            print(json.dumps(res), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(field_bank_markdown(rows, torch.cuda.get_device_name(0)))
        return 0
    if a.field:
        fshapes = parse_field_shapes(a.field_shapes)
        if a.dry_run:
            for nsrc, nch, nr, b, nl in fshapes:
                print(json.dumps({"shape": [nsrc, nch, nr, b], "listeners": nl, "partitions": -(-nr // b), "block_us": round(b / FS * 1e6, 1),
                                  "bytes": field_bytes(nsrc, nch, nr, b)}))
            return 0
        import torch
        from emagls_amd import _lib as L
        lib = L.load()
        rows, ok = [], True
        for fs_ in fshapes:
            res = run_field_shape(lib, L, torch, *fs_, a.blocks, a.warm, a.run)
            ok = ok and res["gate_realtime"] and res["bits_equal"]
            rows.append(res)
            print(json.dumps(res), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(field_markdown(rows, torch.cuda.get_device_name(0)))
        print("condition:", "met" if ok else "MISSED")
        return 0 if ok else 1
    shapes = parse_shapes(a.shapes)
    rots = {"both": (False, True), "none": (False,), "ypr": (True,)}[a.rotation]
    if a.dry_run:
        for s in shapes:
            for r in rots:
                print(json.dumps({"shape": s, "rotation": "ypr" if r else "none", "partitions": -(-s[1] // s[2]), "window": s[1] - 1 + s[2],
                                  "block_us": round(s[2] / FS * 1e6, 1), "bytes": push_bytes(*s, r)}))
        return 0
    import torch
    from emagls_amd import _lib as L
    lib = L.load()
    rows, ok = [], True
    if a.encoded:
        for it in a.enc_shapes:
            M, Cc, ln, B = (int(v) for v in it.split(","))
            parse_shapes(["%d,%d,%d" % (Cc, ln, B)])
            if not (1 <= M <= 64 and 1 <= Cc <= 64) or any(nl < 1 or nl > 4096 for nl in a.listeners):
                raise SystemExit("--encoded: 1 <= M, C <= 64, --listeners from 1 to 4096")
            for nl in a.listeners:
                res = run_encoded_shape(lib, L, torch, M, Cc, ln, B, nl, a.blocks, a.warm, a.run)
                rows.append(res)
                print(json.dumps(res), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(encoded_markdown(rows, torch.cuda.get_device_name(0)))
        return 0
    if a.group:
        if a.sets < 1 or any(nl < 1 or nl > 4096 for nl in a.listeners):
            raise SystemExit("--sets must be at least 1, --listeners from 1 to 4096")
        for s in shapes:
            for r in rots:
                for nl in a.listeners:
                    res = run_group_shape(lib, L, torch, *s, nl, a.sets, r, a.blocks, a.warm, a.run)
                    ok = ok and res["gate"] and res["bits_equal"]
                    rows.append(res)
                    print(json.dumps(res), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(group_markdown(rows, torch.cuda.get_device_name(0)))
        print("gates:", "pass" if ok else "MISS")
        return 0 if ok else 1
    if a.bank:
        if a.sets < 3:
            raise SystemExit("--sets must be at least 3")
        for s in shapes:
            res = run_bank_shape(lib, L, torch, *s, a.sets, a.blocks, a.warm, a.run)
            ok = ok and res["gate_a"] and res["gate_b"]
            rows.append(res)
            print(json.dumps(res), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(bank_markdown(rows, torch.cuda.get_device_name(0)))
        print("gates:", "pass" if ok else "MISS")
        return 0 if ok else 1
    for s in shapes:
        for r in rots:
            res = run_shape(lib, L, torch, *s, r, a.blocks, a.warm, a.run, a.stream_only)
            res["gate_realtime"] = res["stream"]["median_us"] < res["block_us"]
            res["gate_faster"] = a.stream_only or res["stream"]["median_us"] < res["window"]["median_us"]
            ok = ok and res["gate_realtime"] and res["gate_faster"]
            rows.append(res)
            print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(markdown(rows, torch.cuda.get_device_name(0)))
    print("gates:", "pass" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
