"""Time of getArrayIrs (emagls_array_irs) on three shapes, em32 (32 microphones at 4.2 cm) at 48 kHz:
  1. a bank of 2702 directions, one plane wave each, nfft = irLen = 512
  2. the same behind the order-4 encoder (25 channels)
  3. one room source of 20 000 components (delays up to 8000 samples, random gains) at nfft = 16384, irLen = 8192
Seeded synthetic inputs; warm-up calls first; no profiler.  Per shape: the wall time of a call (host arrays in and out: a call
includes its copies), the device-event time of the main kernel (emagls_array_irs_kernel_time), the real FMAs of the main kernel from
the shapes -- 2 ncomp M (nfft/2 + 1) (N + 1) -- over that time as a share of the FP64 vector peak (README.md: 78.6 TFLOP/s, 39.3e12 FMA/s),
and the time of the same spectra in NumPy (the Legendre sum of the definition; shape 3 on 64 of its bins, scaled).  Writes the table
that profiles/r19_array_irs.md quotes, stamped with the kernel sources' hash.

    python tools/array_irs_timing.py [reps] [out.md] [numpy: 0/1]

With --room: getArrayRoomIrs (emagls_array_room_irs) on a shoebox room of 5.2 x 4.1 x 2.9 m, walls 0.9 .. 0.6, one
source, the same array, raw microphones:
  1. max_delay 6000 samples, nfft = irLen = 8192
  2. max_delay 24000 samples, nfft = 65536, irLen = 32768
Per shape: candidates and components, the wall time of the fused call, the device-event times of the enumeration passes
(emagls_shoebox_kernel_time) and of the main kernel, the wall times of getShoeboxComponents and of getArrayIrs on its lists (the
listed path, whose copies the fused call saves), and the time of the same enumeration in NumPy (vectorised).  The table of
profiles/r20_array_room_irs.md.

    python tools/array_irs_timing.py --room [reps] [out.md]

With --spectral: the main kernel on the two room shapes of --room three ways -- flat (emagls_array_room_irs), spectral with flat spectra of
the same coefficients, and the same with the air of 20 degrees and 50 percent (emagls_array_room_irs_spectral) --
alternating in one process after warm-up calls, at least five repetitions each: medians, extremes, and the ratio to the flat kernel.
The table of profiles/r27_room_spectral.md.

    python tools/array_irs_timing.py --spectral [reps] [out.md]

With --point: the main kernel on the same two room shapes as plane waves (emagls_array_room_irs, the flat kernel) and as point sources
(emagls_array_room_irs_point) -- flat walls, and the data-sheet form with flat spectra and air -- alternating in
one process after warm-up calls, at least five repetitions each: medians, extremes, the ratio to the flat kernel, and how far the
point-source response lies from the plane-wave one.  The table of profiles/r28_point_sources.md; a variant built with other
AIR_POINT_BINS / AIR_POINT_MICS is run through EMAGLS_LIB_PATH.

    python tools/array_irs_timing.py --point [reps] [out.md]

With --directive: the main kernel on the same two room shapes with directive sources (emagls_array_room_irs_directive, DESIGN.md section
15) at Nd = 1, 4 and 8 -- plane waves with flat walls, with flat spectra and air, and point sources -- next to the three undirected
kernels, alternating in one process after warm-up calls, at least five repetitions each: medians, extremes, the ratio to the undirected
kernel of the same model and to the flat kernel, and the operation-count estimate.  The table of profiles/r29_source_directivity.md; a variant built with other
AIR_POINT_BINS / AIR_POINT_MICS or with AIR_DIR_UNROLL is run through EMAGLS_LIB_PATH, on the first room alone with rooms = 1.

    python tools/array_irs_timing.py --directive [reps] [out.md] [rooms: 1/2]
"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS, RADIUS, PEAK_FMA = 48000.0, 0.042, 39.3e12


def unit(d):
    return np.column_stack([np.sin(d[:, 1]) * np.cos(d[:, 0]), np.sin(d[:, 1]) * np.sin(d[:, 0]), np.cos(d[:, 1])])


def random_dirs(rng, n):
    return np.column_stack([rng.uniform(0, 2 * np.pi, n), np.arccos(rng.uniform(-1, 1, n))])


def numpy_spectra(mics, comps, owner, nsrc, N, nfft, pre, bins):
    """H [nsrc x len(bins) x M] of the definition for the components comps [J x 4] of the sources owner [J]; seconds."""
    from oracle import emagls_oracle as O
    t0 = time.perf_counter()
    k = np.asarray(bins)
    bn = -O.sphModalCoeffs(N, 2 * np.pi * (k * FS / nfft) / 343.0 * RADIUS).T * ((2 * np.arange(N + 1) + 1) / (4 * np.pi))[:, None]
    last = k == nfft // 2
    bn[:, last] = bn[:, last].real
    x = unit(comps[:, :2]) @ unit(mics).T
    p0, p1 = np.ones_like(x), x
    A = bn[0][:, None, None] * p0
    for n in range(1, N + 1):
        A += bn[n][:, None, None] * p1
        p0, p1 = p1, ((2 * n + 1) * x * p1 - n * p0) / (n + 1)
    A *= (comps[:, 3][None, :] * np.exp(-2j * np.pi * k[:, None] * (comps[:, 2] + pre)[None, :] / nfft))[:, :, None]
    H = np.zeros((nsrc, k.size, mics.shape[0]), dtype=complex)
    np.add.at(H, owner, A.transpose(1, 0, 2))
    H[:, last] = H[:, last].real
    return H, time.perf_counter() - t0


def numpy_shoebox(room, beta, src, pos, max_delay):
    """The definition of DESIGN.md section 12 for one source, vectorised: ([J x 4], candidates, seconds)."""
    t0 = time.perf_counter()
    L, beta, s, a = (np.asarray(v, dtype=np.float64) for v in (room, beta, src, pos))
    box = [int(np.floor(max_delay * 343.0 / FS / (2 * L[i]))) + 1 for i in range(3)]
    ax = [np.arange(-b, b + 1) for b in box]
    nz, ny, nx, pz, py, px = (g.ravel() for g in np.meshgrid(ax[2], ax[1], ax[0], [0, 1], [0, 1], [0, 1], indexing="ij"))
    g, v = np.ones(nx.size), []
    for i, (n, p) in enumerate(((nx, px), (ny, py), (nz, pz))):
        g = g * beta[2 * i] ** np.abs(n - p) * beta[2 * i + 1] ** np.abs(n)
        v.append(((1 - 2 * p) * s[i] + 2 * n * L[i]) - a[i])
    d = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    tau, g = d / 343.0 * FS, g / d
    keep = (g != 0.0) & (tau <= max_delay)
    comps = np.column_stack([np.arctan2(v[1], v[0]), np.arccos(v[2] / d), tau, g])[keep]
    return comps, nx.size, time.perf_counter() - t0


def main_room(argv):
    import emagls_amd as E
    from emagls_amd import _lib as L
    from oracle import emagls_oracle as O
    from tools.csrc_hash import csrc_sha16
    reps = int(argv[0]) if argv else 5
    out = argv[1] if len(argv) > 1 else None
    mics = random_dirs(np.random.default_rng(19), 32)
    room, beta, src, pos, pre = (5.2, 4.1, 2.9), (0.9, 0.85, 0.8, 0.75, 0.7, 0.6), (1.3, 2.2, 1.1), (3.4, 1.7, 1.6), 64.0
    N = O.simulation_order(4, FS, RADIUS)
    lines = ["Kernel sources: csrc_sha16 %s.  Simulation order N = %d, 32 microphones; %d calls per shape after 2 warm-up calls; medians." %
             (csrc_sha16(), N, reps), "",
             "| max_delay | nfft | candidates | components | fused call ms | enumeration passes ms | main kernel ms | getShoeboxComponents ms | "
             "getArrayIrs on its lists ms | listed path ms | NumPy enumeration ms | lists equal NumPy's |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    ms = C.c_double(0.0)

    def timed(f):
        t = time.perf_counter()
        r = f()
        return r, (time.perf_counter() - t) * 1e3

    for max_delay, nfft, ir_len in ((6000.0, 8192, 8192), (24000.0, 65536, 32768)):
        fused = lambda: E.getArrayRoomIrs(room, beta, src, pos, FS, ir_len, pre, RADIUS, mics, nfft=nfft, maxDelay=max_delay)   # noqa: E731
        lists = lambda: E.getShoeboxComponents(room, beta, src, pos, FS, max_delay)   # noqa: E731
        for _ in range(2):
            fused()
            E.getArrayIrs(lists(), FS, ir_len, pre, RADIUS, mics, nfft=nfft)
        t_f, t_e, t_m, t_c, t_l, t_n = [], [], [], [], [], []
        for _ in range(reps):
            a, t = timed(fused)
            t_f.append(t)
            L.check(L.load().emagls_shoebox_kernel_time(C.byref(ms)))
            t_e.append(ms.value)
            L.check(L.load().emagls_array_irs_kernel_time(C.byref(ms)))
            t_m.append(ms.value)
            comps, t = timed(lists)
            t_c.append(t)
            b, t = timed(lambda: E.getArrayIrs(comps, FS, ir_len, pre, RADIUS, mics, nfft=nfft))
            t_l.append(t)
            want, ncand, sec = numpy_shoebox(room, beta, src, pos, max_delay)
            t_n.append(sec * 1e3)
        same = comps[0].shape == want.shape and np.allclose(comps[0][:, 1:], want[:, 1:], rtol=1e-12, atol=1e-12) and np.array_equal(a, b)
        med = lambda v: float(np.median(v))   # noqa: E731
        lines.append("| %d | %d | %d | %d | %.2f | %.3f | %.3f | %.2f | %.2f | %.2f | %.1f | %s |" %
                     (max_delay, nfft, ncand, comps[0].shape[0], med(t_f), med(t_e), med(t_m), med(t_c), med(t_l), med(t_c) + med(t_l), med(t_n),
                      "yes, and fused = listed bit for bit" if same else "NO"))
    text = "\n".join(lines)
    print(text, flush=True)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


def main_spectral(argv):
    import emagls_amd as E
    from emagls_amd import _lib as L
    from oracle import emagls_oracle as O
    from tools.csrc_hash import csrc_sha16
    reps = max(int(argv[0]) if argv else 5, 5)
    out = argv[1] if len(argv) > 1 else None
    mics = random_dirs(np.random.default_rng(19), 32)
    room, beta, src, pos, pre = (5.2, 4.1, 2.9), (0.9, 0.85, 0.8, 0.75, 0.7, 0.6), (1.3, 2.2, 1.1), (3.4, 1.7, 1.6), 64.0
    N = O.simulation_order(4, FS, RADIUS)
    lines = ["Kernel sources: csrc_sha16 %s.  Simulation order N = %d, 32 microphones, one source; the three forms alternate in one process, "
             "%d calls each after 2 warm-up calls each; device-event time of the main kernel (emagls_array_irs_kernel_time)." % (csrc_sha16(), N, reps), "",
             "| max_delay | nfft | components | form | main kernel ms: median | min | max | over flat (medians) | largest difference from flat |",
             "|---|---|---|---|---|---|---|---|---|"]
    ms = C.c_double(0.0)
    for max_delay, nfft, ir_len in ((6000.0, 8192, 8192), (24000.0, 65536, 32768)):
        walls, air = np.repeat(np.array(beta)[:, None], nfft // 2 + 1, axis=1), E.airAttenuation(FS, nfft)
        forms = [("flat", beta, None), ("spectral, flat spectra of the same coefficients", walls, None), ("spectral, the same with air", walls, air)]
        call = lambda w, a: E.getArrayRoomIrs(room, w, src, pos, FS, ir_len, pre, RADIUS, mics, nfft=nfft, maxDelay=max_delay,   # noqa: E731
                                              airAttenuation=a, returnCounts=True)
        times, res = [[] for _ in forms], [None] * len(forms)
        for i in range(2 + reps):
            for f, (_name, w, a) in enumerate(forms):
                res[f], counts = call(w, a)
                L.check(L.load().emagls_array_irs_kernel_time(C.byref(ms)))
                if i >= 2:
                    times[f].append(ms.value)
        flat = float(np.median(times[0]))
        for f, (name, _w, _a) in enumerate(forms):
            diff = "" if f == 0 else "%.3g" % (np.abs(res[f] - res[0]).max() / np.abs(res[0]).max())
            lines.append("| %d | %d | %d | %s | %.3f | %.3f | %.3f | %.3f | %s |" % (max_delay, nfft, counts[0], name, np.median(times[f]), np.min(times[f]),
                                                                               np.max(times[f]), np.median(times[f]) / flat, diff))
    text = "\n".join(lines)
    print(text, flush=True)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


def main_point(argv):
    import emagls_amd as E
    from emagls_amd import _lib as L
    from oracle import emagls_oracle as O
    from tools.csrc_hash import csrc_sha16
    reps = max(int(argv[0]) if argv else 5, 5)
    out = argv[1] if len(argv) > 1 else None
    mics = random_dirs(np.random.default_rng(19), 32)
    room, beta, src, pos, pre = (5.2, 4.1, 2.9), (0.9, 0.85, 0.8, 0.75, 0.7, 0.6), (1.3, 2.2, 1.1), (3.4, 1.7, 1.6), 64.0
    N = O.simulation_order(4, FS, RADIUS)
    lines = ["Kernel sources: csrc_sha16 %s; library %s.  Simulation order N = %d, 32 microphones, one source; the forms alternate in one "
             "process, %d calls each after 2 warm-up calls each; device-event time of the main kernel (emagls_array_irs_kernel_time)." %
             (csrc_sha16(), os.path.basename(L.LIB_PATH), N, reps), "",
             "| max_delay | nfft | components | form | main kernel ms: median | min | max | over flat (medians) | largest difference from the plane waves |",
             "|---|---|---|---|---|---|---|---|---|"]
    ms = C.c_double(0.0)
    for max_delay, nfft, ir_len in ((6000.0, 8192, 8192), (24000.0, 65536, 32768)):
        walls, air = np.repeat(np.array(beta)[:, None], nfft // 2 + 1, axis=1), E.airAttenuation(FS, nfft)
        forms = [("plane waves, flat", beta, None, "planeWave"), ("point sources, flat", beta, None, "pointSource"),
                 ("point sources, flat spectra of the same coefficients and air", walls, air, "pointSource")]
        call = lambda w, a, m: E.getArrayRoomIrs(room, w, src, pos, FS, ir_len, pre, RADIUS, mics, nfft=nfft, maxDelay=max_delay,   # noqa: E731
                                                 airAttenuation=a, returnCounts=True, waveModel=m)
        times, res = [[] for _ in forms], [None] * len(forms)
        for i in range(2 + reps):
            for f, (_name, w, a, m) in enumerate(forms):
                res[f], counts = call(w, a, m)
                L.check(L.load().emagls_array_irs_kernel_time(C.byref(ms)))
                if i >= 2:
                    times[f].append(ms.value)
        flat = float(np.median(times[0]))
        for f, (name, _w, _a, _m) in enumerate(forms):
            diff = "" if f == 0 else "%.3g" % (np.abs(res[f] - res[0]).max() / np.abs(res[0]).max())
            lines.append("| %d | %d | %d | %s | %.3f | %.3f | %.3f | %.3f | %s |" % (max_delay, nfft, counts[0], name, np.median(times[f]), np.min(times[f]),
                                                                               np.max(times[f]), np.median(times[f]) / flat, diff))
    text = "\n".join(lines)
    print(text, flush=True)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


def main_directive(argv):
    import emagls_amd as E
    from emagls_amd import _lib as L
    from oracle import emagls_oracle as O
    from tools.csrc_hash import csrc_sha16
    reps = max(int(argv[0]) if argv else 5, 5)
    out = argv[1] if len(argv) > 1 else None
    mics_per_wave = 4                              # (the estimate's; the kept AIR_POINT_MICS)
    rng = np.random.default_rng(19)
    mics = random_dirs(rng, 32)
    room, beta, src, pos, pre = (5.2, 4.1, 2.9), (0.9, 0.85, 0.8, 0.75, 0.7, 0.6), (1.3, 2.2, 1.1), (3.4, 1.7, 1.6), 64.0
    N = O.simulation_order(4, FS, RADIUS)
    lines = ["Kernel sources: csrc_sha16 %s; library %s.  Simulation order N = %d, 32 microphones, one source turned by a random rotation, random "
             "complex coefficients per bin; the forms alternate in one process, %d calls each after 2 warm-up calls each; device-event time of the "
             "main kernel (emagls_array_irs_kernel_time; a directive call's span includes its basis pass).  Estimate: 1 + (2 Kd + 4) / (2 (N + 1) x %d "
             "microphones per wave), over the flat kernel." % (csrc_sha16(), os.path.basename(L.LIB_PATH), N, reps, mics_per_wave), "",
             "| max_delay | nfft | components | form | Nd | main kernel ms: median | min | max | over its undirected kernel | over flat | estimate |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    ms = C.c_double(0.0)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    R = (q if np.linalg.det(q) > 0 else q * np.array([1.0, 1.0, -1.0]))[None]
    shapes = ((6000.0, 8192, 8192), (24000.0, 65536, 32768))[:int(argv[2]) if len(argv) > 2 else 2]
    for max_delay, nfft, ir_len in shapes:
        P = nfft // 2 + 1
        walls, air = np.repeat(np.array(beta)[:, None], P, axis=1), E.airAttenuation(FS, nfft)
        base = [("plane waves, flat", beta, None, "planeWave"), ("plane waves, flat spectra and air", walls, air, "planeWave"),
                ("point sources, flat", beta, None, "pointSource")]
        forms = [(name, w, a, m, None) for name, w, a, m in base]
        for Nd in (1, 4, 8):
            coef = rng.standard_normal((1, (Nd + 1) ** 2, P)) + 1j * rng.standard_normal((1, (Nd + 1) ** 2, P))
            forms += [(name, w, a, m, coef) for name, w, a, m in base]
        call = lambda w, a, m, c: E.getArrayRoomIrs(room, w, src, pos, FS, ir_len, pre, RADIUS, mics, nfft=nfft, maxDelay=max_delay,   # noqa: E731
                                                    airAttenuation=a, returnCounts=True, waveModel=m, directivity=c,
                                                    sourceOrientation=None if c is None else R)
        times = [[] for _ in forms]
        for i in range(2 + reps):
            for f, (_name, w, a, m, c) in enumerate(forms):
                _res, counts = call(w, a, m, c)
                L.check(L.load().emagls_array_irs_kernel_time(C.byref(ms)))
                if i >= 2:
                    times[f].append(ms.value)
        med = [float(np.median(t)) for t in times]
        for f, (name, _w, _a, _m, c) in enumerate(forms):
            Kd = 0 if c is None else c.shape[1]
            est = "" if c is None else "%.2f" % (1.0 + (2.0 * Kd + 4.0) / (2.0 * (N + 1) * mics_per_wave))
            lines.append("| %d | %d | %d | %s | %s | %.3f | %.3f | %.3f | %.3f | %.3f | %s |" %
                         (max_delay, nfft, counts[0], name, "" if c is None else str(int(round(np.sqrt(Kd))) - 1), med[f], np.min(times[f]), np.max(times[f]),
                          med[f] / med[f % 3], med[f] / med[0], est))
    text = "\n".join(lines)
    print(text, flush=True)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--directive":
        return main_directive(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--point":
        return main_point(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--room":
        return main_room(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--spectral":
        return main_spectral(sys.argv[2:])
    import emagls_amd as E
    from emagls_amd import _lib as L
    from oracle import emagls_oracle as O
    from tools.csrc_hash import csrc_sha16
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    out = sys.argv[2] if len(sys.argv) > 2 else None
    with_numpy = (sys.argv[3] != "0") if len(sys.argv) > 3 else True
    rng = np.random.default_rng(19)
    mics = random_dirs(rng, 32)
    bank = random_dirs(rng, 2702)
    room = [np.column_stack([random_dirs(rng, 20000), rng.uniform(0, 8000, 20000), rng.standard_normal(20000)])]
    enc = E.arrayEncoder("sma", 4, mics[:, 0], mics[:, 1])
    N = O.simulation_order(4, FS, RADIUS)
    shapes = [("bank of 2702 directions, raw", bank, 512, 512, 64.0, None), ("bank of 2702 directions, order-4 encoder", bank, 512, 512, 64.0, enc),
              ("room source of 20000 components", room, 8192, 16384, 64.0, None)]
    lines = ["Kernel sources: csrc_sha16 %s.  Simulation order N = %d; %d calls per shape after 2 warm-up calls." % (csrc_sha16(), N, reps), "",
             "| shape | nfft | ms per call (median) | min | main kernel ms | real FMAs | share of the FP64 vector peak | NumPy, same spectra |",
             "|---|---|---|---|---|---|---|---|"]
    ms = C.c_double(0.0)
    for name, src, ir_len, nfft, pre, e in shapes:
        call = lambda: E.getArrayIrs(src, FS, ir_len, pre, RADIUS, mics, encoder=e, nfft=nfft)   # noqa: E731  (returns host arrays: synchronised)
        for _ in range(2):
            call()
        ts, ks = [], []
        for _ in range(reps):
            t = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t) * 1e3)
            L.check(L.load().emagls_array_irs_kernel_time(C.byref(ms)))
            ks.append(ms.value)
        if isinstance(src, np.ndarray):      # directions: one unit component per source
            comps, nsrc = np.column_stack([src, np.zeros(len(src)), np.ones(len(src))]), len(src)
            owner = np.arange(nsrc)
        else:
            comps, nsrc = np.vstack(src), len(src)
            owner = np.repeat(np.arange(nsrc), [len(s) for s in src])
        P = nfft // 2 + 1
        fmas = 2.0 * comps.shape[0] * 32 * P * (N + 1)
        k_ms = float(np.median(ks))
        if not with_numpy:
            np_text = "not measured"
        elif comps.shape[0] * P > 5e6:
            bins = np.arange(0, P, P // 64)[:64]
            _, sec = numpy_spectra(mics, comps, owner, nsrc, N, nfft, pre, bins)
            np_text = "%.0f s (from %.1f s on 64 of %d bins)" % (sec * P / 64, sec, P)
        else:
            _, sec = numpy_spectra(mics, comps, owner, nsrc, N, nfft, pre, np.arange(P))
            np_text = "%.2f s" % sec
        lines.append("| %s | %d | %.2f | %.2f | %.3f | %.3g | %.1f %% | %s |" % (name, nfft, np.median(ts), np.min(ts), k_ms, fmas,
                                                                              100.0 * fmas / (k_ms * 1e-3) / PEAK_FMA, np_text))
    text = "\n".join(lines)
    print(text, flush=True)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
