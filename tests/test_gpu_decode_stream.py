"""The block-streaming binauralDecode (BinauralDecodeStream, emagls_decode_stream_*) on the GPU.  Expected values:
oracle.emagls_oracle.binauralDecode on the concatenated signal, rotated -- where a push has angles -- by a rotation that does not
share the kernel's algorithm: per sample the matrix fitted by least squares on a Fibonacci lattice (tests/test_gpu_rotate3.py's
fitted_mt, restated here), or the plane-wave identity.  Bound: 1e-12 relative to the largest output magnitude, the bound
tests/test_gpu_decode_render.py holds the offline decode to."""
import math

import numpy as np
import pytest

from oracle import emagls_oracle as O

gpu = pytest.mark.gpu
TOL = 1e-12
SHAPES = [(25, 512, 64), (25, 512, 1024), (64, 2048, 256), (9, 4096, 64), (25, 512, 2048), (256, 512, 128), (25, 300, 64)]   # (C, len, B)


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def randn(rng, r, c, cplx=False):
    return rng.standard_normal((r, c)) + 1j * rng.standard_normal((r, c)) if cplx else rng.standard_normal((r, c))


def run_stream(E, x, wL, wR, B, group=1, angles=None, basis="real", domain="sh", **kw):
    """Push x through a fresh stream `group` blocks at a time; angles: per-sample (yaw, pitch, roll) arrays or None each."""
    out = []
    with E.BinauralDecodeStream(wL, wR, B, shDefinition=basis, rotationDomain=domain, complexInput=np.iscomplexobj(x), **kw) as s:
        step = B * group
        for i in range(0, x.shape[0], step):
            a = [None if v is None else v[i:i + step] for v in (angles or (None, None, None))]
            out.append(s.push(x[i:i + step], *a))
    return np.vstack(out)


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
        n = x.shape[0]
        y = np.zeros(x.shape, dtype=np.complex128 if (self.basis == "complex" or np.iscomplexobj(x)) else np.float64)
        b = lambda a: np.broadcast_to(np.zeros(1) if a is None else np.asarray(a, dtype=float).reshape(-1), (n,))   # noqa: E731
        yaw, pitch, roll = b(yaw), b(pitch), b(roll)
        last, mt = None, None
        for t in range(n):
            key = (yaw[t], pitch[t], roll[t])
            if key != last:
                mt = self.pinv @ pw(self.N, self.u @ rmat(*key).T, self.basis)
                last = key
            y[t] = x[t] @ mt
        return y


def ch_rotate(x, yaw, N, basis):
    """Yaw of a CH signal by the fitted matrix per sample: S(a) Rot^T = S(a + yaw) on 4N + 4 equiangular azimuths."""
    azi = np.arange(4 * N + 4) * 2 * np.pi / (4 * N + 4)
    pinv = np.linalg.pinv(np.conj(O.getCH(N, azi, basis)))
    y = np.zeros(x.shape, dtype=np.complex128 if basis == "complex" else np.float64)
    for t in range(x.shape[0]):
        y[t] = x[t] @ (pinv @ np.conj(O.getCH(N, azi + yaw[t], basis)))
    return y


def walk(rng, n, step, start=0.0):
    return start + np.cumsum(rng.normal(0, step, n))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. parity without rotation
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("Cc,ln,B", SHAPES + [(25, 1, 64), (4, 40, 128)])
@pytest.mark.parametrize("kind", ["real", "complex_signal", "complex_filters", "complex_both"])
def test_parity_without_rotation(Cc, ln, B, kind):
    import emagls_amd as E
    rng = np.random.default_rng(Cc * 7 + ln + B)
    n = B * max(3, -(-ln // B) + 2)
    x = randn(rng, n, Cc, kind in ("complex_signal", "complex_both"))
    wL, wR = (randn(rng, ln, Cc, kind in ("complex_filters", "complex_both")) for _ in range(2))
    got = run_stream(E, x, wL, wR, B)
    err = rel(got, O.binauralDecode(x, wL, wR))
    print("parity", (Cc, ln, B), kind, "%.2e" % err)
    assert got.shape == (n, 2) and err <= TOL


# ---------------------------------------------------------------------------------------------------------------------------
# 2. blocking does not matter
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_blocking_does_not_matter():
    import emagls_amd as E
    rng = np.random.default_rng(11)
    n, Cc, ln = 8192, 16, 700
    x, wL, wR = randn(rng, n, Cc), randn(rng, ln, Cc), randn(rng, ln, Cc)
    want = O.binauralDecode(x, wL, wR)
    for B in (64, 256, 1024, 2048):
        one = run_stream(E, x, wL, wR, B, 1)
        err = rel(one, want)
        print("blocking B=%d" % B, "%.2e" % err)
        assert err <= TOL
        for group in (2, 4):
            assert np.array_equal(run_stream(E, x, wL, wR, B, group), one), (B, group)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. trajectories
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N", [1, 4, 7, 15])
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_trajectories_sh(N, basis):
    import emagls_amd as E
    rng = np.random.default_rng(100 + N)
    Cc, B, ln = (N + 1) ** 2, 64, 150
    n = 4 * B if N < 15 else 2 * B
    x, wL, wR = randn(rng, n, Cc), randn(rng, ln, Cc, basis == "complex"), randn(rng, ln, Cc, basis == "complex")
    rot = FittedRotation(N, basis)
    yaw = walk(rng, n, 0.02, 0.5)
    h = n // 2                                                   # a smooth walk across pitch = pi / 2, then one across -pi / 2
    pitch = np.concatenate([np.linspace(1.2, 2.0, h), -np.linspace(1.2, 2.0, n - h)]) + walk(rng, n, 0.002)
    roll = walk(rng, n, 0.02, -0.3)
    assert pitch[:n // 2].min() < np.pi / 2 < pitch[:n // 2].max() and pitch[n // 2:].min() < -np.pi / 2 < pitch[n // 2:].max()
    for name, ang in (("yaw", (yaw, None, None)), ("ypr", (yaw, pitch, roll))):
        got = run_stream(E, x, wL, wR, B, 1, ang, basis)
        err = rel(got, O.binauralDecode(rot.apply(x, *ang), wL, wR))
        print("trajectory N=%d %s %s" % (N, basis, name), "%.2e" % err)
        assert err <= TOL, (name, err)


@gpu
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_trajectory_ch_yaw(basis):
    import emagls_amd as E
    rng = np.random.default_rng(5)
    N, B, ln = 6, 64, 100
    Cc, n = 2 * N + 1, 4 * B
    x, wL, wR = randn(rng, n, Cc), randn(rng, ln, Cc), randn(rng, ln, Cc)
    yaw = walk(rng, n, 0.03, -1.0)
    got = run_stream(E, x, wL, wR, B, 2, (yaw, None, None), basis, "ch")
    err = rel(got, O.binauralDecode(ch_rotate(x, yaw, N, basis), wL, wR))
    print("trajectory CH %s" % basis, "%.2e" % err)
    assert err <= TOL


@gpu
def test_angle_forms_are_bit_identical():
    import emagls_amd as E
    rng = np.random.default_rng(9)
    N, B, ln = 3, 128, 300
    Cc, n = (N + 1) ** 2, 4 * B
    x, wL, wR = randn(rng, n, Cc), randn(rng, ln, Cc), randn(rng, ln, Cc)
    per_push = [(0.3 * k, -0.2 * k, 0.1 + k) for k in range(n // B)]
    a, b = [], []
    with E.BinauralDecodeStream(wL, wR, B) as s1, E.BinauralDecodeStream(wL, wR, B) as s2:
        for k, (y, p, r) in enumerate(per_push):
            blk = x[k * B:(k + 1) * B]
            a.append(s1.push(blk, y, p, r))                                          # one value per push
            b.append(s2.push(blk, np.full(B, y), np.full(B, p), np.full(B, r)))      # the same value per sample
    assert np.array_equal(np.vstack(a), np.vstack(b))
    yaw = walk(rng, n, 0.02)
    only = run_stream(E, x, wL, wR, B, 1, (yaw, None, None))
    zeros = run_stream(E, x, wL, wR, B, 1, (yaw, np.zeros(n), np.zeros(n)))
    assert np.array_equal(only, zeros)


@gpu
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_plane_wave_with_a_rotation_per_block(basis):
    """A plane wave from u, rotated by R_k in block k: the stream's input after the rotation IS the plane wave from R_k u, so the
    output is the oracle's decode of those signals -- each block's response with the tails of the earlier blocks."""
    import emagls_amd as E
    rng = np.random.default_rng(21)
    N, B, ln = 4, 64, 200
    Cc, nb = (N + 1) ** 2, 6
    u = np.array([0.6, -0.48, 0.64])
    env = rng.standard_normal(nb * B)
    x = env[:, None] * pw(N, u, basis)
    if basis == "real":
        x = x.real
    wL, wR = randn(rng, ln, Cc, basis == "complex"), randn(rng, ln, Cc, basis == "complex")
    angs = [(rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-3, 3)) for _ in range(nb)]
    want_in = np.vstack([env[k * B:(k + 1) * B, None] * pw(N, rmat(*angs[k]) @ u, basis) for k in range(nb)])
    got = []
    with E.BinauralDecodeStream(wL, wR, B, shDefinition=basis, complexInput=basis == "complex") as s:
        for k in range(nb):
            got.append(s.push(x[k * B:(k + 1) * B], *angs[k]))
    err = rel(np.vstack(got), O.binauralDecode(want_in, wL, wR))
    print("plane wave %s" % basis, "%.2e" % err)
    assert err <= TOL


# ---------------------------------------------------------------------------------------------------------------------------
# 4. state
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_reset_alternation_and_cache_clear():
    import emagls_amd as E
    from emagls_amd import _lib as L
    rng = np.random.default_rng(31)
    B, Cc, n = 128, 9, 1024
    x = randn(rng, n, Cc)
    f1, f2 = (randn(rng, 500, Cc), randn(rng, 500, Cc)), (randn(rng, 260, Cc), randn(rng, 260, Cc))
    yaw = walk(rng, n, 0.01)
    solo1, solo2 = run_stream(E, x, *f1, B, 1, (yaw, None, None)), run_stream(E, x, *f2, B)
    with E.BinauralDecodeStream(*f1, B) as s1, E.BinauralDecodeStream(*f2, B) as s2:
        o1, o2 = [], []
        for i in range(0, n, B):                       # two streams with different filters, pushed alternately
            o1.append(s1.push(x[i:i + B], yaw[i:i + B]))
            o2.append(s2.push(x[i:i + B]))
            if i == 3 * B:
                L.check(L.load().emagls_cache_clear())   # ... and a cache clear in between changes nothing
        assert np.array_equal(np.vstack(o1), solo1) and np.array_equal(np.vstack(o2), solo2)
        s1.reset()                                     # reset, then the same pushes: the bits of a fresh stream
        again = np.vstack([s1.push(x[i:i + B], yaw[i:i + B]) for i in range(0, n, B)])
        assert np.array_equal(again, solo1)


@gpu
def test_create_destroy_leaves_no_device_memory_behind():
    import torch
    import emagls_amd as E
    rng = np.random.default_rng(41)
    wL, wR, x = randn(rng, 2048, 25), randn(rng, 2048, 25), randn(rng, 256, 25)
    free = []
    for i in range(50):
        with E.BinauralDecodeStream(wL, wR, 64) as s:
            s.push(x, 0.1, 0.2, 0.3)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert free[49] >= free[1], (free[1], free[49])


# ---------------------------------------------------------------------------------------------------------------------------
# 5. device entry
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cplx", [False, True])
def test_device_entry_matches_host_entry(cplx):
    import torch
    import emagls_amd as E
    rng = np.random.default_rng(51)
    N, B, ln, nb = 4, 64, 512, 200
    Cc, n = (N + 1) ** 2, 200 * 64
    basis = "complex" if cplx else "real"
    x, wL, wR = randn(rng, n, Cc, cplx), randn(rng, ln, Cc, cplx), randn(rng, ln, Cc, cplx)
    yaw, pitch, roll = walk(rng, n, 0.01), walk(rng, n, 0.01, 1.0), walk(rng, n, 0.01)
    host = run_stream(E, x, wL, wR, B, 1, (yaw, pitch, roll), basis)
    dev = torch.device("cuda:0")
    tx, ty, tp, tr = (torch.from_numpy(a).to(dev) for a in (x, yaw, pitch, roll))
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    outs = []
    with E.BinauralDecodeStream(wL, wR, B, shDefinition=basis, complexInput=cplx) as s:
        assert s.info["launches_per_block"] <= (4 if cplx else 3)
        with torch.cuda.stream(st):
            for k in range(nb):       # 200 pushes enqueued, no synchronise in between
                sl = slice(k * B, (k + 1) * B)
                outs.append(s.push(tx[sl], ty[sl], tp[sl], tr[sl]))
        st.synchronize()
        got = torch.cat(outs).cpu().numpy()
    assert isinstance(outs[0], torch.Tensor) and outs[0].shape == (B, 2)
    assert np.array_equal(got, host)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. consistency with the offline call (a cross-check of two library paths, not the parity test)
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_consistency_with_the_offline_call(basis):
    import warnings
    import emagls_amd as E
    rng = np.random.default_rng(61)
    N, B, ln = 5, 256, 512
    Cc, n = (N + 1) ** 2, 8 * B
    x, wL, wR = randn(rng, n, Cc), randn(rng, ln, Cc, basis == "complex"), randn(rng, ln, Cc, basis == "complex")
    yaw, pitch, roll = walk(rng, n, 0.01), walk(rng, n, 0.01, 0.4), walk(rng, n, 0.01, -0.2)
    got = run_stream(E, x, wL, wR, B, 2, (yaw, pitch, roll), basis)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        off = E.binauralDecode(x, 48000, wL, wR, 48000, False, horRotAngleRad=yaw, pitchRad=pitch, rollRad=roll, shDefinition=basis)
    err = rel(got, off)
    print("offline %s" % basis, "%.2e" % err)
    assert err <= TOL
