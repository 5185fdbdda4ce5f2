"""Three-axis rotation of SH signals (rotateSH, shRotationMatrix, binauralDecode with pitchRad / rollRad) against expected values
that do not share the kernel's algorithm: the plane-wave identity on oracle.emagls_oracle.getSH (rotateSH(conj(Y(u))) ==
conj(Y(R u))), and a matrix fitted by least squares on a Fibonacci lattice of 3 (N+1)^2 points (M^T = pinv(S(u)) S(R u)).
Specification: DESIGN.md section 7."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import emagls_oracle as O

gpu = pytest.mark.gpu
PI = np.pi


def Rx(t):
    c, s = math.cos(t), math.sin(t)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def Ry(t):
    c, s = math.cos(t), math.sin(t)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def Rz(t):
    c, s = math.cos(t), math.sin(t)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def rmat(yaw, pitch, roll):
    return Rz(yaw) @ Ry(pitch) @ Rx(roll)


def ypr_of(R):
    """(yaw, pitch, roll) of R = Rz(yaw) Ry(pitch) Rx(roll)."""
    return math.atan2(R[1, 0], R[0, 0]), math.atan2(-R[2, 0], math.hypot(R[0, 0], R[1, 0])), math.atan2(R[2, 1], R[2, 2])


def dirs(v):
    return np.column_stack([np.arctan2(v[:, 1], v[:, 0]), np.arctan2(np.hypot(v[:, 0], v[:, 1]), v[:, 2])])


def pw(N, v, basis):
    """Rows: the signal of a plane wave from each unit vector, conj(Y)."""
    return np.conj(O.getSH(N, dirs(np.atleast_2d(v)), basis))


def unit(rng, k):
    v = rng.standard_normal((k, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def fib(N):
    i = np.arange(3 * (N + 1) ** 2) + 0.5
    azi, zen = np.pi * (1 + 5 ** 0.5) * i, np.arccos(1 - 2 * i / i.size)
    return np.column_stack([np.sin(zen) * np.cos(azi), np.sin(zen) * np.sin(azi), np.cos(zen)])


def fitted_mt(N, R, basis):
    """M^T with S(u) M^T = S(R u), by least squares on a Fibonacci lattice."""
    u = fib(N)
    return np.linalg.pinv(pw(N, u, basis)) @ pw(N, u @ np.asarray(R).T, basis)


ROTATIONS = [(0.3, -1.2, 2.5), (-2.0, 0.7, -0.4), (1.1, 2.9, 0.2),            # random-looking
             (PI / 2, 0, 0), (0, PI / 2, 0), (0, 0, PI / 2),                    # the three fixed points' rotations
             (0.4, PI / 2, -0.3), (0.4, -PI / 2, 1.0), (0, 0, PI), (2.0, PI, 0.1),   # gimbal, roll = pi
             (1e-9, 0, 0), (0, 1e-9, 0), (0, 0, 1e-9), (1e-9, -1e-9, 1e-9), (0, PI - 1e-9, 0)]


def tol(N):
    return 1e-12 if N <= 7 else 1e-11


# ---------------------------------------------------------------------------------------------------------------------------
# 1. plane-wave identity
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N", [1, 2, 4, 7, 15])
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_plane_wave_identity(N, basis):
    import emagls_amd as E
    rng = np.random.default_rng(N)
    u = unit(rng, 48)
    x = pw(N, u, basis)
    scale = np.abs(x).max()
    for yaw, pitch, roll in ROTATIONS:
        got = E.rotateSH(x, yaw, pitch, roll, basis)
        want = pw(N, u @ rmat(yaw, pitch, roll).T, basis)
        assert np.abs(got - want).max() <= tol(N) * scale, ((yaw, pitch, roll), np.abs(got - want).max())
    # one rotation per sample, each angle its own array (and a scalar mixed in)
    yaw, pitch = rng.uniform(-PI, PI, u.shape[0]), rng.uniform(-PI, PI, u.shape[0])
    pitch[:4] = [PI / 2, -PI / 2, 0.0, 1e-9]
    got = E.rotateSH(x, yaw, pitch, 0.7, basis)
    want = np.vstack([pw(N, u[i] @ rmat(yaw[i], pitch[i], 0.7).T, basis) for i in range(u.shape[0])])
    assert np.abs(got - want).max() <= tol(N) * scale


@gpu
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_fixed_points(basis):
    import emagls_amd as E
    N = 3
    front, left, top, floor = [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, -1]
    for src, ypr, dst in [(front, (PI / 2, 0, 0), left), (front, (0, PI / 2, 0), floor), (left, (0, 0, PI / 2), top)]:
        got = E.rotateSH(pw(N, np.array([src], float), basis), *ypr, shDefinition=basis)
        assert np.abs(got - pw(N, np.array([dst], float), basis)).max() < 1e-14


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the matrix
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N", [1, 4, 8, 15])
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_rotation_matrix(N, basis):
    import emagls_amd as E
    C_ = (N + 1) ** 2
    for ypr in [(0.3, -1.2, 2.5), (0.4, PI / 2, -0.3), (0, 1e-9, 0)]:
        M = E.shRotationMatrix(N, *ypr, shDefinition=basis)
        assert M.shape == (C_, C_)
        if N <= 8:    # the fit's own conditioning limits it beyond
            assert np.abs(M - fitted_mt(N, rmat(*ypr), basis).T).max() < 1e-12
        assert np.abs(M @ M.conj().T - np.eye(C_)).max() < 1e-13
        for n in range(N + 1):   # zero across orders
            blk = slice(n * n, (n + 1) ** 2)
            off = M[blk].copy()
            off[:, blk] = 0
            assert not off.any()
        x = pw(N, unit(np.random.default_rng(1), 10), basis)
        assert np.abs(x @ M.T - E.rotateSH(x, *ypr, shDefinition=basis)).max() < 1e-13
    R1, R2 = rmat(0.3, -1.2, 2.5), rmat(-2.0, 0.7, -0.4)
    M12 = E.shRotationMatrix(N, *ypr_of(R2 @ R1), shDefinition=basis)
    M1, M2 = E.shRotationMatrix(N, 0.3, -1.2, 2.5, basis), E.shRotationMatrix(N, -2.0, 0.7, -0.4, basis)
    assert np.abs(M12 - M2 @ M1).max() < 1e-12


# ---------------------------------------------------------------------------------------------------------------------------
# 3. yaw only
# ---------------------------------------------------------------------------------------------------------------------------
def _wf(rng, shape, cplx):
    return rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0)


@gpu
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_yaw_only_is_rotate_yaw(basis):
    import emagls_amd as E
    rng = np.random.default_rng(3)
    x = rng.standard_normal((500, 25))
    th = rng.uniform(-4, 4, 500)
    assert np.array_equal(E.rotateSH(x, 0.8, 0.0, 0.0, basis), E.rotateYaw(x, 0.8, basis))
    assert np.array_equal(E.rotateSH(x, th, np.zeros(500), 0, basis), E.rotateYaw(x, th, basis))
    wL, wR = rng.standard_normal((512, 25)), rng.standard_normal((512, 25))
    for yaw in (0.8, th):
        assert np.array_equal(E.binauralDecode(x, 48000, wL, wR, 48000, True, horRotAngleRad=yaw, shDefinition=basis, pitchRad=0, rollRad=0),
                              E.binauralDecode(x, 48000, wL, wR, 48000, True, horRotAngleRad=yaw, shDefinition=basis))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. / 5. the decode with a trajectory and with a fixed rotation
# ---------------------------------------------------------------------------------------------------------------------------
def trajectory(n):
    t = np.linspace(0, 1, n)
    return 2.0 * np.sin(2 * PI * t), (PI / 2 + 0.3) * np.sin(2 * PI * 1.5 * t), 0.8 * np.cos(2 * PI * t)   # pitch passes +-pi/2


def rotate_np(x, yaw, pitch, roll, N, basis):
    """Per-sample rotation with fitted matrices (all rotated lattices in one getSH call)."""
    n = x.shape[0]
    u = fib(N)
    P = np.linalg.pinv(pw(N, u, basis))
    Rs = np.stack([rmat(yaw[i], pitch[i], roll[i]) for i in range(n)])
    S = pw(N, np.einsum("nij,kj->nki", Rs, u).reshape(-1, 3), basis).reshape(n, u.shape[0], -1)
    return np.einsum("ck,nkd,nc->nd", P, S, x)


def oracle_render(x, wL, wR, comp=False, signal=None):
    ear = np.zeros((x.shape[0], 2), dtype=np.complex128)
    for c in range(x.shape[1]):
        ear[:, 0] += O.fftfilt(wL[:, c], x[:, c])
        ear[:, 1] += O.fftfilt(wR[:, c], x[:, c])
    if signal is not None:
        ear = np.column_stack([O.fftfilt(ear[:, 0], signal), O.fftfilt(ear[:, 1], signal)])
    if comp:
        ear = ear[wL.shape[0] // 2 - 1:]
    return ear.real


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@gpu
@pytest.mark.parametrize("length", [512, 3000])
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_trajectory_decode(length, basis):
    import warnings

    import emagls_amd as E
    N, n = 4, 4000
    rng = np.random.default_rng(length)
    x = _wf(rng, (n, 25), basis == "complex")
    wL, wR = _wf(rng, (length, 25), basis == "complex"), _wf(rng, (length, 25), basis == "complex")
    yaw, pitch, roll = trajectory(n)
    xr = rotate_np(x, yaw, pitch, roll, N, basis)
    sig = rng.standard_normal(6000)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for comp, s in [(False, None), (True, sig)]:
            got = E.binauralDecode(x, 48000, wL, wR, 48000, comp, s, None, yaw, shDefinition=basis, pitchRad=pitch, rollRad=roll)
            assert rel(got, oracle_render(xr, wL, wR, comp, s)) <= 1e-10


@gpu
@pytest.mark.parametrize("length", [512, 3000])
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_fixed_rotation_decode(length, basis):
    import warnings

    import emagls_amd as E
    N, n = 4, 4000
    rng = np.random.default_rng(length + 1)
    x = _wf(rng, (n, 25), basis == "complex")
    wL, wR = _wf(rng, (length, 25), basis == "complex"), _wf(rng, (length, 25), basis == "complex")
    ypr = (0.4, -1.1, 2.2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fixed = E.binauralDecode(x, 48000, wL, wR, 48000, True, None, None, ypr[0], shDefinition=basis, pitchRad=ypr[1], rollRad=ypr[2])
        const = E.binauralDecode(x, 48000, wL, wR, 48000, True, None, None, np.full(n, ypr[0]), shDefinition=basis,
                                 pitchRad=np.full(n, ypr[1]), rollRad=ypr[2])
    assert rel(fixed, const) <= 1e-12
    assert rel(fixed, oracle_render(x @ fitted_mt(N, rmat(*ypr), basis), wL, wR, True)) <= 1e-10


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the device entry
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_device_entry(basis):
    import torch

    from emagls_amd import _lib as L
    rng = np.random.default_rng(6)
    n, ln, cb = 3000, 512, basis == "complex"
    x = np.asfortranarray(rng.standard_normal((n, 25)))
    wL, wR = np.asfortranarray(rng.standard_normal((ln, 25))), np.asfortranarray(rng.standard_normal((ln, 25)))
    yaw, pitch, roll = trajectory(n)
    sig = rng.standard_normal(5000)
    dev = torch.device("cuda")

    def d(a):   # column-major host array -> device tensor with the same memory layout
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a).T).reshape(-1)).to(dev)

    lib = L.load()
    for angles, s in [((yaw, pitch, roll), None), ((yaw[:1], pitch[:1], roll[:1]), sig)]:
        nout = s.size if s is not None else n
        host = np.zeros((nout, 2), order="F")
        him = (C.c_double * 2)()
        hv = [np.ascontiguousarray(a) for a in angles]
        L.check(lib.emagls_binaural_decode_render_ypr(
            x.ctypes.data_as(C.c_void_p), 0, n, 25, wL.ctypes.data_as(C.c_void_p), wR.ctypes.data_as(C.c_void_p), 0, ln, 0, 0, L.BASIS[basis],
            *[q for a in hv for q in (a.ctypes.data_as(C.c_void_p), a.size)],
            None if s is None else s.ctypes.data_as(C.c_void_p), 0 if s is None else s.size, host.ctypes.data_as(C.c_void_p), him))
        dx, dL, dR = d(x), d(wL), d(wR)
        da = [torch.from_numpy(a).to(dev) for a in hv]
        ds = None if s is None else torch.from_numpy(s).to(dev)
        dout = torch.zeros(2 * nout, dtype=torch.float64, device=dev)
        dim = (C.c_double * 2)()
        torch.cuda.synchronize()
        L.check(lib.emagls_binaural_decode_render_ypr_device(
            C.c_void_p(dx.data_ptr()), 0, n, 25, C.c_void_p(dL.data_ptr()), C.c_void_p(dR.data_ptr()), 0, ln, 0, L.BASIS[basis],
            *[q for a in da for q in (C.c_void_p(a.data_ptr()), a.numel())],
            None if ds is None else C.c_void_p(ds.data_ptr()), 0 if ds is None else ds.numel(), C.c_void_p(dout.data_ptr()), dim,
            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        got = dout.cpu().numpy().reshape(2, nout).T
        assert np.array_equal(got, host) and (cb or (dim[0], dim[1]) == (him[0], him[1]))
    # explicit zero pitch / roll arrays take the three-axis path; the yaw path (n_pitch = n_roll = 0) agrees to 1e-14
    z = torch.zeros(n, dtype=torch.float64, device=dev)
    dy = torch.from_numpy(yaw.copy()).to(dev)
    outs = []
    for npr in (n, 0):
        dout = torch.zeros(2 * n, dtype=torch.float64, device=dev)
        dim = (C.c_double * 2)()
        L.check(lib.emagls_binaural_decode_render_ypr_device(
            C.c_void_p(dx.data_ptr()), 0, n, 25, C.c_void_p(dL.data_ptr()), C.c_void_p(dR.data_ptr()), 0, ln, 0, L.BASIS[basis],
            C.c_void_p(dy.data_ptr()), n, C.c_void_p(z.data_ptr()), npr, C.c_void_p(z.data_ptr()), npr, None, 0,
            C.c_void_p(dout.data_ptr()), dim, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        outs.append(dout.cpu().numpy())
    assert rel(outs[0], outs[1]) <= 1e-14


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the MEX gateway
# ---------------------------------------------------------------------------------------------------------------------------
from test_mex_gateway import mex  # noqa: E402,F401  (the stub mex.h harness)


@gpu
def test_mex_rotate3(mex):
    import emagls_amd as E
    rng = np.random.default_rng(7)
    x = rng.standard_normal((300, 16))
    yaw, pitch, roll = trajectory(300)
    for basis in ("real", "complex"):
        assert np.array_equal(mex(1, "rotate3", x, yaw.reshape(-1, 1), pitch.reshape(-1, 1), 0.3, basis)[0],
                              E.rotateSH(x, yaw, pitch, 0.3, basis))
        assert np.array_equal(mex(1, "shrotmtx", 3, 0.1, 0.2, 0.3, basis)[0], E.shRotationMatrix(3, 0.1, 0.2, 0.3, basis))
    wL, wR = rng.standard_normal((512, 16)), rng.standard_normal((512, 16))
    sig = rng.standard_normal((800, 1))
    assert np.array_equal(mex(1, "decode", x, wL, wR, True, yaw.reshape(-1, 1), sig, "real", "sh", pitch.reshape(-1, 1), 0.3)[0],
                          E.binauralDecode(x, 48000, wL, wR, 48000, True, sig, 48000, yaw, pitchRad=pitch, rollRad=0.3))
    assert np.array_equal(mex(1, "decode", x, wL, wR, True, 0.5, np.zeros((0, 0)), "real", "sh", 0.0, 0.0)[0],
                          E.binauralDecode(x, 48000, wL, wR, 48000, True, horRotAngleRad=0.5))
    with pytest.raises(mex.Error, match="orders 0 to 15"):
        mex(1, "shrotmtx", 16, 0.1, 0.2, 0.3)


# ---------------------------------------------------------------------------------------------------------------------------
# 8. order 15 on 10^5 samples, one rotation per sample
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_order15_trajectory():
    import emagls_amd as E
    N, n = 15, 100_000
    rng = np.random.default_rng(15)
    u = unit(rng, n)
    yaw, pitch, roll = trajectory(n)
    x = pw(N, u, "real")
    Rs = np.einsum("nij,njk,nkl->nil", np.stack([Rz(a) for a in yaw]), np.stack([Ry(a) for a in pitch]), np.stack([Rx(a) for a in roll]))
    want = pw(N, np.einsum("nij,nj->ni", Rs, u), "real")
    got = E.rotateSH(x, yaw, pitch, roll)
    assert np.abs(got - want).max() <= 1e-11 * np.abs(x).max()
