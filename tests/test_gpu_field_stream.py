"""The field stream (SourceFieldStream, emagls_field_stream_*) on the GPU.  Expected values: the sum over
the sources of oracle.emagls_oracle.fftfilt of each response column with its source.  Bound: 1e-12 relative to the largest output
magnitude, the bound tests/test_gpu_decode_stream.py holds the decode stream to.  The chains into a decode stream are compared with
oracle.binauralDecode on the oracle's field, rotated by a rotation that does not share the kernel's algorithm: per sample the
matrix fitted by least squares on a Fibonacci lattice (tests/test_gpu_decode_stream.py's FittedRotation, restated here)."""
import functools
import math

import numpy as np
import pytest

from oracle import emagls_oracle as O

gpu = pytest.mark.gpu
TOL = 1e-12
# (nsrc, nch, nr, B, complex response)
SHAPES = [(1, 4, 1, 64, False), (1, 25, 300, 64, False), (2, 9, 700, 128, False), (3, 5, 4100, 2048, False), (1, 64, 1000, 256, False),
          (16, 2, 130, 64, False), (1, 1, 2561, 64, False), (2, 9, 300, 64, True), (1, 25, 600, 512, True), (3, 3, 2049, 1024, False)]


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def oracle_field(s, rirs):
    """sum_q oracle.fftfilt(rir_q(:, c), s_q)"""
    return sum(np.column_stack([O.fftfilt(rirs[q][:, c], s[:, q]) for c in range(rirs.shape[2])]) for q in range(rirs.shape[0]))


@functools.lru_cache(maxsize=None)
def case(nsrc, nch, nr, cplx, n, seed=0):
    """Sources [n x nsrc], responses [nsrc x nr x nch] and the oracle's field, made once and shared (read only)."""
    rng = np.random.default_rng(1000 * nsrc + 10 * nch + nr + n + seed)
    rirs = rng.standard_normal((nsrc, nr, nch))
    if cplx:
        rirs = rirs + 1j * rng.standard_normal((nsrc, nr, nch))
    s = rng.standard_normal((n, nsrc))
    want = oracle_field(s, rirs)
    for a in (s, rirs, want):
        a.setflags(write=False)
    return s, rirs, want


def run_field(E, s, rirs, B, group=1):
    """Push s through a fresh field stream `group` blocks at a time (host entry)."""
    with E.SourceFieldStream(rirs, B) as f:
        return np.vstack([f.push(s[i:i + B * group]) for i in range(0, s.shape[0], B * group)])


def on_device(torch, a):
    """A device tensor of a (shared, read-only) array."""
    return torch.from_numpy(np.array(a)).to(torch.device("cuda:0"))


def walk(rng, n, step, start=0.0):
    return start + np.cumsum(rng.normal(0, step, n))


# ---- an independent rotation: least squares on a point set that resolves order N
def _rz(t):
    c, s = math.cos(t), math.sin(t)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def _ry(t):
    c, s = math.cos(t), math.sin(t)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def _rx(t):
    c, s = math.cos(t), math.sin(t)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def rmat(yaw, pitch, roll):
    return _rz(yaw) @ _ry(pitch) @ _rx(roll)


def _dirs(v):
    return np.column_stack([np.arctan2(v[:, 1], v[:, 0]), np.arctan2(np.hypot(v[:, 0], v[:, 1]), v[:, 2])])


def pw(N, v, basis):
    """Rows: the signal of a plane wave from each unit vector, conj(Y)."""
    return np.conj(O.getSH(N, _dirs(np.atleast_2d(v)), basis))


class FittedRotation:
    """x M^T with S(u) M^T = S(R u), M^T by least squares on a Fibonacci lattice of 3 (N+1)^2 points (pinv(S(u)) once)."""

    def __init__(self, N, basis):
        i = np.arange(3 * (N + 1) ** 2) + 0.5
        azi, zen = np.pi * (1 + 5 ** 0.5) * i, np.arccos(1 - 2 * i / i.size)
        self.u = np.column_stack([np.sin(zen) * np.cos(azi), np.sin(zen) * np.sin(azi), np.cos(zen)])
        self.N, self.basis = N, basis
        self.pinv = np.linalg.pinv(pw(N, self.u, basis))

    def apply(self, x, yaw, pitch, roll):
        y = np.zeros(x.shape, dtype=np.complex128 if (self.basis == "complex" or np.iscomplexobj(x)) else np.float64)
        for t in range(x.shape[0]):
            y[t] = x[t] @ (self.pinv @ pw(self.N, self.u @ rmat(yaw[t], pitch[t], roll[t]).T, self.basis))
        return y


# ---------------------------------------------------------------------------------------------------------------------------
# 1. parity
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nsrc,nch,nr,B,cplx", SHAPES)
def test_parity(nsrc, nch, nr, B, cplx):
    import emagls_amd as E
    n = B * (-(-nr // B) + 3)                       # the ring wraps
    s, rirs, want = case(nsrc, nch, nr, cplx, n)
    got = run_field(E, s, rirs, B)
    err = rel(got, want)
    print("parity", (nsrc, nch, nr, B, cplx), "%.2e" % err)
    assert got.shape == (n, nch) and np.iscomplexobj(got) == cplx and err <= TOL


# ---------------------------------------------------------------------------------------------------------------------------
# 2. blocking does not matter
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("B", [64, 256, 2048])
def test_blocking_does_not_matter(B):
    import emagls_amd as E
    nb = 4 * -(-(-(-700 // B) + 3) // 4)            # blocks: a multiple of 4 that wraps the ring
    s, rirs, want = case(2, 9, 700, False, nb * B)
    one = run_field(E, s, rirs, B, 1)
    err = rel(one, want)
    print("blocking B=%d" % B, "%.2e" % err)
    assert err <= TOL
    for group in (2, 4):
        assert np.array_equal(run_field(E, s, rirs, B, group), one), (B, group)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. state
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_reset_fresh_objects_and_cache_clear():
    import emagls_amd as E
    from emagls_amd import _lib as L
    B = 128
    s, rirs, want = case(2, 9, 700, False, 12 * B)
    solo = run_field(E, s, rirs, B)
    assert np.array_equal(run_field(E, s, rirs, B), solo)          # two fresh objects: equal bits
    with E.SourceFieldStream(rirs, B) as f:
        for i in range(0, 3 * B, B):                               # a few blocks, then reset: the bits of a fresh object
            f.push(s[i:i + B])
        f.reset()
        out = []
        for i in range(0, s.shape[0], B):
            out.append(f.push(s[i:i + B]))
            if i == 5 * B:
                L.check(L.load().emagls_cache_clear())             # ... and a cache clear between pushes changes nothing
        assert np.array_equal(np.vstack(out), solo)
    assert rel(solo, want) <= TOL


@gpu
def test_create_destroy_leaves_no_device_memory_behind():
    import torch
    import emagls_amd as E
    s, rirs, _ = case(2, 25, 2048, False, 256)
    free = []
    for i in range(50):
        with E.SourceFieldStream(rirs, 64) as f:
            f.push(s)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert free[49] >= free[1], (free[1], free[49])


# ---------------------------------------------------------------------------------------------------------------------------
# 4. device entry
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cplx", [False, True])
def test_device_entry_matches_host_entry(cplx):
    import torch
    import emagls_amd as E
    B, nb = 64, 40
    s, rirs, want = case(3, 9, 500, cplx, nb * B)
    host = run_field(E, s, rirs, B)
    dev = torch.device("cuda:0")
    ts = on_device(torch, s)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    outs = []
    with E.SourceFieldStream(rirs, B) as f:
        assert f.info["launches_per_block"] == 2
        with torch.cuda.stream(st):
            for k in range(nb):       # every push enqueued, no synchronise in between
                outs.append(f.push(ts[k * B:(k + 1) * B]))
        st.synchronize()
        got = torch.cat(outs).cpu().numpy()
    assert isinstance(outs[0], torch.Tensor) and outs[0].shape == (B, 9) and outs[0].is_complex() == cplx
    assert outs[0].t().is_contiguous()                             # the [nch][n] buffer the kernel wrote, as a decode push reads it
    assert np.array_equal(got, host) and rel(got, want) <= TOL


# ---------------------------------------------------------------------------------------------------------------------------
# 5. - 7. chains
# ---------------------------------------------------------------------------------------------------------------------------
CH_B, CH_NB, CH_N = 64, 14, 4     # 700 taps at B = 64: 11 partitions, the ring wraps


@functools.lru_cache(maxsize=None)
def chain_case():
    """The chain's inputs: (2, 25, 700, 64) into 25 channels x 512 taps, and three listeners' per-sample yaw, pitch and roll."""
    n = CH_B * CH_NB
    s, rirs, field = case(2, 25, 700, False, n)
    rng = np.random.default_rng(77)
    wL, wR = rng.standard_normal((512, 25)), rng.standard_normal((512, 25))
    ang = np.stack([np.stack([walk(rng, n, 0.02, 0.5 * l), walk(rng, n, 0.01, 0.4 - l), walk(rng, n, 0.02, -0.3 * l)]) for l in range(3)])
    for a in (wL, wR, ang):
        a.setflags(write=False)
    return s, rirs, field, wL, wR, ang      # ang [listener][yaw, pitch, roll][n]


def device_chain(E, torch, l):
    """Listener l's chain on the device: torch tensors in both objects, no host synchronisation between the pushes."""
    s, rirs, _, wL, wR, ang = chain_case()
    ts, ta = on_device(torch, s), on_device(torch, ang[l])
    outs = []
    with E.SourceFieldStream(rirs, CH_B) as f, E.BinauralDecodeStream(wL, wR, CH_B) as d:
        for k in range(CH_NB):
            sl = slice(k * CH_B, (k + 1) * CH_B)
            outs.append(d.push(f.push(ts[sl]), ta[0, sl], ta[1, sl], ta[2, sl]))
        return torch.cat(outs).cpu().numpy()


@gpu
def test_chain_on_the_device():
    import torch
    import emagls_amd as E
    s, rirs, field, wL, wR, ang = chain_case()
    got = device_chain(E, torch, 0)
    staged = []
    with E.SourceFieldStream(rirs, CH_B) as f, E.BinauralDecodeStream(wL, wR, CH_B) as d:
        for k in range(CH_NB):                                    # the same chain staged through NumPy
            sl = slice(k * CH_B, (k + 1) * CH_B)
            staged.append(d.push(f.push(s[sl]), ang[0, 0, sl], ang[0, 1, sl], ang[0, 2, sl]))
    assert np.array_equal(got, np.vstack(staged))
    want = O.binauralDecode(FittedRotation(CH_N, "real").apply(field, *ang[0]), wL, wR)
    err = rel(got, want)
    print("chain", "%.2e" % err)
    assert got.shape == (CH_B * CH_NB, 2) and err <= TOL


@gpu
def test_chain_into_a_group():
    import torch
    import emagls_amd as E
    s, rirs, _, wL, wR, ang = chain_case()
    ts, ta = on_device(torch, s), on_device(torch, ang)
    outs = []
    with E.SourceFieldStream(rirs, CH_B) as f, E.BinauralDecodeGroup(wL, wR, CH_B, 3) as g:
        for k in range(CH_NB):
            sl = slice(k * CH_B, (k + 1) * CH_B)
            outs.append(g.push(f.push(ts[sl]), ta[:, 0, sl], ta[:, 1, sl], ta[:, 2, sl]))
        got = torch.cat(outs, dim=1).cpu().numpy()               # [3 x n x 2]
    for l in range(3):
        assert np.array_equal(got[l], device_chain(E, torch, l)), l


@gpu
def test_chain_with_microphone_domain_responses():
    import torch
    import emagls_amd as E
    M, N, B, nb = 32, 4, 64, 8                                   # 300 taps at B = 64: 5 partitions
    s, rirs, _ = case(1, M, 300, False, nb * B)
    i = np.arange(M) + 0.5
    enc = E.arrayEncoder("sma", N, np.pi * (1 + 5 ** 0.5) * i, np.arccos(1 - 2 * i / M))
    rng = np.random.default_rng(78)
    Cc = (N + 1) ** 2
    wL, wR = rng.standard_normal((200, Cc)), rng.standard_normal((200, Cc))
    yaw, pitch, roll = walk(rng, nb * B, 0.02), walk(rng, nb * B, 0.01, 0.3), walk(rng, nb * B, 0.02, -0.2)
    mics = run_field(E, s, rirs, B)                              # the field stream's host output
    with E.BinauralDecodeStream(wL, wR, B, encoder=enc) as d:
        want = np.vstack([d.push(mics[k * B:(k + 1) * B], yaw[k * B:(k + 1) * B], pitch[k * B:(k + 1) * B], roll[k * B:(k + 1) * B])
                          for k in range(nb)])
    ts, ty, tp, tr = (on_device(torch, a) for a in (s, yaw, pitch, roll))
    outs = []
    with E.SourceFieldStream(rirs, B) as f, E.BinauralDecodeStream(wL, wR, B, encoder=enc) as d:
        for k in range(nb):
            sl = slice(k * B, (k + 1) * B)
            outs.append(d.push(f.push(ts[sl, 0]), ty[sl], tp[sl], tr[sl]))      # ([n]: one source's block)
        got = torch.cat(outs).cpu().numpy()
    assert np.abs(want).max() > 0 and np.array_equal(got, want)
