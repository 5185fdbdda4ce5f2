"""The listener group on the GPU (BinauralDecodeGroup): many listeners of one sound field in one push.
Its defining property is checked as such: listener l's output equals, with np.array_equal, what a fresh BinauralDecodeStream of
the same bank returns for the same blocks with listener l's angles and set indices.  Parity is checked against the oracle, not
the library: sum_s oracle.binauralDecode(g_s x_rot_l, wL_s, wR_s) with the gains of the written cross-fade rule and the rotation
fitted by least squares on a Fibonacci lattice (both restated from tests/test_gpu_decode_bank.py), to 1e-12 relative to the largest
output magnitude, the bound of that file and of tests/test_gpu_decode_stream.py.
Shapes (C, len, B, L): the smallest that reach each path of the forward kernel (see SHAPES)."""
import math

import numpy as np
import pytest

from oracle import emagls_oracle as O

gpu = pytest.mark.gpu
TOL = 1e-12
SHAPES = [
    (4, 100, 64, 3),        # thread groups share the pairs (G > 1), P = 2, odd pair count
    (9, 300, 128, 5),       # three-axis rotation, order 2
    (5, 40, 64, 2),         # P = 1: the store-only partition
    (4, 1500, 1024, 2),     # KU = 3, G = 1
    (3, 2500, 2048, 2),     # KU = 5: with S = 3 the instance that spills
    (25, 512, 64, 1),       # the group of one
]


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def randn(rng, shape, cplx=False):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape) if cplx else rng.standard_normal(shape)


def num_blocks(ln, B):
    """max(6, P + 3) blocks, so the ring wraps; rounded up to a multiple of 3 for the pushes of three blocks."""
    nb = max(6, -(-ln // B) + 3)
    return -(-nb // 3) * 3


def set_gains(sigma, B, S):
    """g [S x n]: block t gives sigma_t the gain 1 when it equals sigma_(t-1); else r[i] = (i + 1) / B to sigma_t and 1 - r[i] to
    sigma_(t-1); sigma_(-1) := sigma_0."""
    r = (np.arange(B) + 1.0) / B
    g = np.zeros((S, len(sigma) * B))
    prev = sigma[0]
    for t, s in enumerate(sigma):
        sl = slice(t * B, (t + 1) * B)
        if s == prev:
            g[s, sl] = 1.0
        else:
            g[s, sl] = r
            g[prev, sl] = 1.0 - r
        prev = s
    return g


def oracle_sum(x, wL, wR, sigma, B):
    g = set_gains(sigma, B, wL.shape[0])
    return sum(O.binauralDecode(g[s][:, None] * x, wL[s], wR[s]) for s in range(wL.shape[0]) if np.any(g[s]))


def random_sigma(rng, nb, S):
    """Index sequences that hold still for some blocks and switch in consecutive blocks for others."""
    sigma = [int(rng.integers(S))]
    while len(sigma) < nb:
        if rng.random() < 0.5:
            sigma += [sigma[-1]] * int(rng.integers(1, 4))                 # hold
        else:
            for _ in range(int(rng.integers(2, 5))):                      # a new set in every block
                sigma.append(int((sigma[-1] + rng.integers(1, max(S, 2))) % S))
    return sigma[:nb]


def listener_sigmas(rng, nl, nb, S):
    """[L x nb]: listener 0 switches in every block, the last listener (of more than one) never does, the others at random."""
    sig = np.array([random_sigma(rng, nb, S) for _ in range(nl)], dtype=np.int64)
    if S > 1:
        sig[0] = (sig[0, 0] + np.arange(nb)) % S
        if nl > 1:
            sig[-1] = sig[-1, 0]
    return sig


def _rz(t):
    c, s = math.cos(t), math.sin(t)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def _ry(t):
    c, s = math.cos(t), math.sin(t)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def _rx(t):
    c, s = math.cos(t), math.sin(t)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def pw(N, v, basis):
    """Rows: the signal of a plane wave from each unit vector, conj(Y)."""
    v = np.atleast_2d(v)
    dirs = np.column_stack([np.arctan2(v[:, 1], v[:, 0]), np.arctan2(np.hypot(v[:, 0], v[:, 1]), v[:, 2])])
    return np.conj(O.getSH(N, dirs, basis))


def fitted_rotation(x, yaw, pitch, roll, N, basis):
    """x M^T per sample with S(u) M^T = S(R u), R = Rz(yaw) Ry(pitch) Rx(roll), M^T by least squares on a Fibonacci lattice of
    3 (N+1)^2 points."""
    i = np.arange(3 * (N + 1) ** 2) + 0.5
    azi, zen = np.pi * (1 + 5 ** 0.5) * i, np.arccos(1 - 2 * i / i.size)
    u = np.column_stack([np.sin(zen) * np.cos(azi), np.sin(zen) * np.sin(azi), np.cos(zen)])
    pinv = np.linalg.pinv(pw(N, u, basis))
    y = np.zeros(x.shape, dtype=np.complex128 if (basis == "complex" or np.iscomplexobj(x)) else np.float64)
    for t in range(x.shape[0]):
        R = _rz(yaw[t]) @ _ry(pitch[t]) @ _rx(roll[t])
        y[t] = x[t] @ (pinv @ pw(N, u @ R.T, basis))
    return y


# ---- the two sides of the defining property
ANGLES = ["none", "yaw_scalar", "yaw", "ypr"]


def make_angles(rng, case, nl, n):
    """(yaw, pitch, roll), each None, [L] (one value per listener and push: `yaw_scalar` keeps it over the whole run) or [L x n]."""
    if case == "none":
        return None, None, None
    if case == "yaw_scalar":
        return rng.uniform(-3, 3, nl), None, None
    traj = lambda start: start[:, None] + np.cumsum(rng.normal(0, 0.02, (nl, n)), axis=1)   # noqa: E731
    if case == "yaw":
        return traj(rng.uniform(-3, 3, nl)), None, None
    return traj(rng.uniform(-3, 3, nl)), traj(rng.uniform(-1, 1, nl)), traj(rng.uniform(-1, 1, nl))


def cut(a, i, step):
    return None if a is None else (a if a.ndim == 1 else a[:, i:i + step])


def run_group(E, x, wL, wR, B, nl, sig, angles, step, basis="real", domain="sh", device=False, group=None):
    """x through a fresh group (or `group`), `step` samples per push; sig [L x nb] or None.  Returns [L x n x 2]."""
    g = group or E.BinauralDecodeGroup(wL, wR, B, nl, shDefinition=basis, rotationDomain=domain, complexInput=np.iscomplexobj(x))
    out = []
    try:
        if device:
            import torch
            dev = torch.device("cuda:0")
            to = lambda a, dt=None: None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev).to(dt or torch.float64)  # noqa: E731
            tx = torch.as_tensor(x, device=dev)
        for k, i in enumerate(range(0, x.shape[0], step)):
            a = [cut(v, i, step) for v in angles]
            idx = None if sig is None else sig[:, k * (step // B):(k + 1) * (step // B)]
            if device:
                o = g.push(tx[i:i + step], *[to(v) for v in a], setIndex=None if idx is None else to(idx, torch.int32))
                torch.cuda.synchronize()
                out.append(o.cpu().numpy())
            else:
                out.append(g.push(x[i:i + step], *a, setIndex=idx))
    finally:
        if group is None:
            g.close()
    return np.concatenate(out, axis=1)


def run_stream(E, x, wL, wR, B, sigma, angles, basis="real", domain="sh", first=0):
    """A fresh BinauralDecodeStream fed one listener's data from block `first` on, a block per push."""
    out = []
    with E.BinauralDecodeStream(wL, wR, B, shDefinition=basis, rotationDomain=domain, complexInput=np.iscomplexobj(x)) as s:
        for k in range(first, x.shape[0] // B):
            a = [None if v is None else (float(v) if np.ndim(v) == 0 else v[k * B:(k + 1) * B]) for v in angles]
            out.append(s.push(x[k * B:(k + 1) * B], *a, setIndex=None if sigma is None else int(sigma[k])))
    return np.vstack(out)


def listener_angles(angles, l):
    return [None if v is None else v[l] for v in angles]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. bit equality with single streams
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("Cc,ln,B,nl", SHAPES)
def test_every_listener_is_a_single_stream_bit_for_bit(Cc, ln, B, nl):
    import emagls_amd as E
    rng = np.random.default_rng(Cc * 7 + ln + B + nl)
    nb = num_blocks(ln, B)
    n = nb * B
    sh = int(round(math.sqrt(Cc))) ** 2 == Cc            # an SH channel count: else the yaw cases turn a CH signal (2N + 1 channels)
    domain = "sh" if sh else "ch"
    combo = 0
    for kind in ("real", "complex_signal", "complex_filters", "complex_both"):
        x = randn(rng, (n, Cc), kind in ("complex_signal", "complex_both"))
        w = [randn(rng, (3, ln, Cc), kind in ("complex_filters", "complex_both")) for _ in range(2)]
        for case in ANGLES:
            if case == "ypr" and not sh:
                continue                                   # (pitch and roll need an SH signal)
            for S in (1, 3):
                combo += 1
                basis = "complex" if (case != "none" and combo % 4 == 3) else "real"
                wL, wR = (w[0][0], w[1][0]) if S == 1 else (w[0], w[1])
                sig = listener_sigmas(rng, nl, nb, S) if S > 1 else None
                angles = make_angles(rng, case, nl, n)
                want = np.stack([run_stream(E, x, wL, wR, B, None if sig is None else sig[l], listener_angles(angles, l), basis, domain)
                                 for l in range(nl)])
                # host and device entry, pushes of one block and of three: each pairing in turn
                for device, blocks in ((False, 1), (True, 3)) if combo % 2 else ((False, 3), (True, 1)):
                    got = run_group(E, x, wL, wR, B, nl, sig, angles, blocks * B, basis, domain, device)
                    assert got.shape == (nl, n, 2)
                    for l in range(nl):
                        assert np.array_equal(got[l], want[l]), (kind, case, S, basis, "device" if device else "host", blocks, l)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. parity against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("Cc,ln,B,nl", [(9, 300, 128, 5), (4, 100, 64, 3)])
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_parity_against_the_oracle(Cc, ln, B, nl, basis):
    import emagls_amd as E
    rng = np.random.default_rng(Cc + ln + nl)
    N, S, nb = int(round(math.sqrt(Cc))) - 1, 3, num_blocks(ln, B)
    n = nb * B
    x = randn(rng, (n, Cc))
    wL, wR = randn(rng, (S, ln, Cc), basis == "complex"), randn(rng, (S, ln, Cc), basis == "complex")
    sig = listener_sigmas(rng, nl, nb, S)
    angles = make_angles(rng, "ypr", nl, n)
    got = run_group(E, x, wL, wR, B, nl, sig, angles, 3 * B, basis)
    for l in range(nl):
        xr = fitted_rotation(x, angles[0][l], angles[1][l], angles[2][l], N, basis)
        err = rel(got[l], oracle_sum(xr, wL, wR, list(sig[l]), B))
        print("group parity", (Cc, ln, B, nl), basis, "listener %d" % l, "%.2e" % err)
        assert err <= TOL


# ---------------------------------------------------------------------------------------------------------------------------
# 3. - 5. independence, reset, determinism
# ---------------------------------------------------------------------------------------------------------------------------
def small_case(seed):
    rng = np.random.default_rng(seed)
    Cc, ln, B, nl, S = 4, 100, 64, 3, 3
    nb = num_blocks(ln, B)
    x, wL, wR = randn(rng, (nb * B, Cc)), randn(rng, (S, ln, Cc)), randn(rng, (S, ln, Cc))
    return rng, B, nl, S, nb, x, wL, wR, listener_sigmas(rng, nl, nb, S), make_angles(rng, "ypr", nl, nb * B)


@gpu
def test_listeners_are_independent():
    import emagls_amd as E
    rng, B, nl, S, nb, x, wL, wR, sig, angles = small_case(3)
    base = run_group(E, x, wL, wR, B, nl, sig, angles, B)
    sig2, angles2 = sig.copy(), [a.copy() for a in angles]
    sig2[1] = (sig[1] + 1) % S
    for a in angles2:
        a[1] += 0.5
    other = run_group(E, x, wL, wR, B, nl, sig2, angles2, B)
    assert np.array_equal(other[0], base[0]) and np.array_equal(other[2], base[2])
    assert not np.array_equal(other[1], base[1])


@gpu
def test_reset_of_one_listener_and_of_all():
    import emagls_amd as E
    rng, B, nl, S, nb, x, wL, wR, sig, angles = small_case(4)
    whole = run_group(E, x, wL, wR, B, nl, sig, angles, B)
    k = 4                                                # reset in mid-stream, the ring partly filled
    with E.BinauralDecodeGroup(wL, wR, B, nl) as g:
        head = run_group(E, x[:k * B], wL, wR, B, nl, sig[:, :k], [a[:, :k * B] for a in angles], B, group=g)
        g.reset(1)
        tail = run_group(E, x[k * B:], wL, wR, B, nl, sig[:, k:], [a[:, k * B:] for a in angles], B, group=g)
        assert np.array_equal(head, whole[:, :k * B])
        for l in (0, 2):                                 # the others run on uninterrupted
            assert np.array_equal(tail[l], whole[l, k * B:])
        fresh = run_stream(E, x, wL, wR, B, sig[1], listener_angles(angles, 1), first=k)
        assert np.array_equal(tail[1], fresh)            # the listener who joined: a fresh stream from that block on
        assert not np.array_equal(tail[1], whole[1, k * B:])
        g.reset()                                        # all of them
        again = run_group(E, x, wL, wR, B, nl, sig, angles, B, group=g)
        assert np.array_equal(again, whole)


@gpu
def test_equal_pushes_give_equal_bits():
    import emagls_amd as E
    rng, B, nl, S, nb, x, wL, wR, sig, angles = small_case(5)
    one = run_group(E, x, wL, wR, B, nl, sig, angles, B)
    assert np.array_equal(run_group(E, x, wL, wR, B, nl, sig, angles, B), one)            # two fresh groups
    assert np.array_equal(run_group(E, x, wL, wR, B, nl, sig, angles, 3 * B), one)        # three pushes of one block == one of three
    assert np.array_equal(run_group(E, x, wL, wR, B, nl, sig, angles, 3 * B, device=True), one)
