"""The decode stream's bank of filter sets on the GPU (BinauralDecodeStream with [numSets x len x numChannels] filters and
push(..., setIndex=...)).  Expected values never come from the library: they are
sum_s oracle.binauralDecode(g_s x, wL_s, wR_s) with the gains of the written rule (set_gains below), on a signal rotated -- where a
push has angles -- by the rotation fitted by least squares on a Fibonacci lattice (tests/test_gpu_decode_stream.py's, restated
here).  Bound: 1e-12 relative to the largest output magnitude, the bound of tests/test_gpu_decode_stream.py; the designs of
designYawBank are held to 1e-6, the bound tests/test_gpu_ls_magls.py and tests/test_gpu_emagls.py hold single designs to.
No test gives the device entry an index outside the bank: the clamp in the kernels is shown by reading them."""
import math

import numpy as np
import pytest

from oracle import emagls_oracle as O

gpu = pytest.mark.gpu
TOL = 1e-12
DESIGN_TOL = 1e-6
SHAPES = [(25, 512, 64), (25, 512, 1024), (64, 2048, 256), (9, 4096, 64), (25, 512, 2048), (256, 512, 128), (25, 300, 64)]   # (C, len, B)


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def randn(rng, shape, cplx=False):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape) if cplx else rng.standard_normal(shape)


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


def run_bank(E, x, wL, wR, B, sigma, group=1, angles=None, basis="real", form="array"):
    """Push x through a fresh bank stream `group` blocks at a time.  form: 'array' (one index per block), 'scalar' (group 1
    only: an int per push) or 'none' (no setIndex at all)."""
    out = []
    with E.BinauralDecodeStream(wL, wR, B, shDefinition=basis, complexInput=np.iscomplexobj(x)) as s:
        step = B * group
        for k, i in enumerate(range(0, x.shape[0], step)):
            a = [None if v is None else v[i:i + step] for v in (angles or (None, None, None))]
            idx = {"array": sigma[k * group:(k + 1) * group], "scalar": int(sigma[k]), "none": None}[form]
            out.append(s.push(x[i:i + step], *a, setIndex=idx))
    return np.vstack(out)


def run_plain(E, x, wL, wR, B, angles=None, basis="real"):
    out = []
    with E.BinauralDecodeStream(wL, wR, B, shDefinition=basis, complexInput=np.iscomplexobj(x)) as s:
        for i in range(0, x.shape[0], B):
            a = [None if v is None else v[i:i + B] for v in (angles or (None, None, None))]
            out.append(s.push(x[i:i + B], *a))
    return np.vstack(out)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. parity
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("Cc,ln,B", SHAPES)
@pytest.mark.parametrize("S", [1, 2, 5])
@pytest.mark.parametrize("kind", ["real", "complex_signal", "complex_filters", "complex_both"])
def test_parity_with_random_indices(Cc, ln, B, S, kind):
    import emagls_amd as E
    rng = np.random.default_rng(Cc * 7 + ln + B + S)
    nb = max(6, -(-ln // B) + 3)
    sigma = random_sigma(rng, nb, S)
    x = randn(rng, (nb * B, Cc), kind in ("complex_signal", "complex_both"))
    wL, wR = (randn(rng, (S, ln, Cc), kind in ("complex_filters", "complex_both")) for _ in range(2))
    got = run_bank(E, x, wL, wR, B, sigma)
    err = rel(got, oracle_sum(x, wL, wR, sigma, B))
    print("bank parity", (Cc, ln, B), "S=%d" % S, kind, "switches=%d" % sum(a != b for a, b in zip(sigma, sigma[1:])), "%.2e" % err)
    assert got.shape == (nb * B, 2) and err <= TOL


@gpu
def test_parity_short_filters_and_named_sequences():
    """len < B, len = 1; A -> B -> A, a switch in the first and in the last block, a switch in every block."""
    import emagls_amd as E
    rng = np.random.default_rng(77)
    for Cc, ln, B in ((25, 1, 64), (4, 40, 128), (7, 64, 64)):
        for sigma in ([0, 1, 0, 0, 2, 0, 2, 2], [0, 1, 1, 1, 1, 1, 1, 2], [0, 1, 2, 0, 1, 2, 1, 0], [1, 0, 0, 0, 0, 0, 0, 0]):
            x, wL, wR = randn(rng, (8 * B, Cc)), randn(rng, (3, ln, Cc)), randn(rng, (3, ln, Cc))
            err = rel(run_bank(E, x, wL, wR, B, sigma), oracle_sum(x, wL, wR, sigma, B))
            print("bank named", (Cc, ln, B), sigma, "%.2e" % err)
            assert err <= TOL


# ---------------------------------------------------------------------------------------------------------------------------
# 5. bit equalities
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("Cc,ln,B", [(16, 700, 64), (25, 512, 1024), (9, 300, 2048), (256, 512, 128)])
def test_constant_index_is_the_plain_stream(Cc, ln, B):
    import emagls_amd as E
    rng = np.random.default_rng(5 + B)
    nb, S = 6, 5
    x, wL, wR = randn(rng, (nb * B, Cc)), randn(rng, (S, ln, Cc)), randn(rng, (S, ln, Cc))
    for j in (0, 3):
        plain = run_plain(E, x, wL[j], wR[j], B)
        assert np.array_equal(run_bank(E, x, wL, wR, B, [j] * nb), plain), j
        assert np.array_equal(run_bank(E, x, wL, wR, B, [j] * nb, form="scalar"), plain), j
    assert np.array_equal(run_bank(E, x, wL, wR, B, [0] * nb, form="none"), run_plain(E, x, wL[0], wR[0], B))   # a fresh stream: set 0
    one = run_bank(E, x, wL[2:3], wR[2:3], B, [0] * nb)                                 # a bank of one set
    assert np.array_equal(one, run_plain(E, x, wL[2], wR[2], B))


@gpu
@pytest.mark.parametrize("cplx", [False, True])
def test_index_forms_and_grouping_are_bit_identical(cplx):
    import emagls_amd as E
    rng = np.random.default_rng(15)
    Cc, ln, B, S, nb = 16, 700, 128, 4, 16
    sigma = random_sigma(rng, nb, S)
    x, wL, wR = randn(rng, (nb * B, Cc), cplx), randn(rng, (S, ln, Cc), cplx), randn(rng, (S, ln, Cc), cplx)
    one = run_bank(E, x, wL, wR, B, sigma)
    assert rel(one, oracle_sum(x, wL, wR, sigma, B)) <= TOL
    assert np.array_equal(run_bank(E, x, wL, wR, B, sigma, form="scalar"), one)         # an int == the same value per block
    for group in (2, 4):
        assert np.array_equal(run_bank(E, x, wL, wR, B, sigma, group), one), group     # blocks pushed 1, 2, 4 at a time
    # None keeps the set of the previous block, across pushes
    with E.BinauralDecodeStream(wL, wR, B, complexInput=cplx) as s:
        held = [s.push(x[:B], setIndex=2)] + [s.push(x[k * B:(k + 1) * B]) for k in range(1, 4)]
    assert np.array_equal(np.vstack(held), run_bank(E, x[:4 * B], wL, wR, B, [2] * 4))


@gpu
def test_device_entry_matches_host_entry():
    import torch
    import emagls_amd as E
    rng = np.random.default_rng(51)
    N, B, ln, nb, S = 4, 64, 512, 200, 5
    Cc, n = (N + 1) ** 2, nb * B
    sigma = random_sigma(rng, nb, S)
    x, wL, wR = randn(rng, (n, Cc)), randn(rng, (S, ln, Cc)), randn(rng, (S, ln, Cc))
    yaw = np.cumsum(rng.normal(0, 0.01, n))
    host = run_bank(E, x, wL, wR, B, sigma, angles=(yaw, None, None))
    dev = torch.device("cuda:0")
    tx, ty = torch.from_numpy(x).to(dev), torch.from_numpy(yaw).to(dev)
    ts = torch.tensor(sigma, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    outs = []
    with E.BinauralDecodeStream(wL, wR, B) as s:
        assert s.numSets == S and s.info["launches_per_block"] <= 3
        with torch.cuda.stream(st):
            for k in range(nb):       # 200 pushes enqueued, no synchronise in between; the index is never read on the host
                sl = slice(k * B, (k + 1) * B)
                outs.append(s.push(tx[sl], ty[sl], setIndex=ts[k:k + 1]))
        st.synchronize()
        got = torch.cat(outs).cpu().numpy()
        assert np.array_equal(got, host)
        s.reset()                     # reset forgets the selection too: the same pushes give the same bits
        with torch.cuda.stream(st):
            again = torch.cat([s.push(tx[k * B:(k + 4) * B], ty[k * B:(k + 4) * B], setIndex=ts[k:k + 4]) for k in range(0, nb, 4)])
        st.synchronize()
        assert np.array_equal(again.cpu().numpy(), host)


@gpu
def test_host_and_device_pushes_mixed_on_one_stream():
    """The host keeps a copy of the selection to run a standing set on the plain kernel; indices it never saw (device tensors)
    make that copy unknown until two blocks it does know have passed.  Any mix of the entries gives the bits of the host entry."""
    import torch
    import emagls_amd as E
    rng = np.random.default_rng(71)
    Cc, ln, B, S = 9, 300, 64, 3
    sigma = [1, 1, 1, 1, 2, 2, 2, 2, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2]
    nb = len(sigma)
    x, wL, wR = randn(rng, (nb * B, Cc)), randn(rng, (S, ln, Cc)), randn(rng, (S, ln, Cc))
    want = run_bank(E, x, wL, wR, B, sigma)
    assert rel(want, oracle_sum(x, wL, wR, sigma, B)) <= TOL
    dev = torch.device("cuda:0")
    tx, ts = torch.from_numpy(x).to(dev), torch.tensor(sigma, dtype=torch.int32, device=dev)
    for pattern in ("hdk", "dhh", "kdh", "dkk"):      # h: host entry, d: device entry with a device index, k: device entry, no index
        got = []
        with E.BinauralDecodeStream(wL, wR, B) as s:
            for k in range(nb):
                sl = slice(k * B, (k + 1) * B)
                how = pattern[k % 3]
                if how == "k" and (k == 0 or sigma[k] != sigma[k - 1]):
                    how = "d"                          # (no index keeps the set: only where the sequence does)
                if how == "h":
                    got.append(s.push(x[sl], setIndex=sigma[k]))
                else:
                    out = s.push(tx[sl], setIndex=ts[k:k + 1] if how == "d" else None)
                    torch.cuda.synchronize()
                    got.append(out.cpu().numpy())
        assert np.array_equal(np.vstack(got), want), pattern


@gpu
def test_reset_forgets_the_selection():
    import emagls_amd as E
    rng = np.random.default_rng(31)
    Cc, ln, B, S = 9, 500, 128, 3
    sigma = [2, 2, 0, 1, 1, 0, 2, 2]
    x, wL, wR = randn(rng, (8 * B, Cc)), randn(rng, (S, ln, Cc)), randn(rng, (S, ln, Cc))
    fresh = run_bank(E, x, wL, wR, B, sigma)
    with E.BinauralDecodeStream(wL, wR, B) as s:
        first = np.vstack([s.push(x[k * B:(k + 1) * B], setIndex=sigma[k]) for k in range(8)])
        s.reset()      # the stream stood on set 2 with set 2 before it; after the reset block 0 on set 2 must not fade from anything
        again = np.vstack([s.push(x[k * B:(k + 1) * B], setIndex=sigma[k]) for k in range(8)])
        s.reset()
        zero = np.vstack([s.push(x[k * B:(k + 1) * B]) for k in range(2)])             # and without an index the set is 0 again
    assert np.array_equal(first, fresh) and np.array_equal(again, fresh)
    assert np.array_equal(zero, run_plain(E, x[:2 * B], wL[0], wR[0], B))


# ---------------------------------------------------------------------------------------------------------------------------
# 6. rotation first, then the bank
# ---------------------------------------------------------------------------------------------------------------------------
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


@gpu
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_three_axis_trajectory_on_an_sh_bank(basis):
    import emagls_amd as E
    rng = np.random.default_rng(100)
    N, B, ln, S = 4, 64, 150, 3
    Cc, nb = (N + 1) ** 2, 8
    n = nb * B
    sigma = [0, 0, 1, 2, 2, 0, 1, 1]
    x = randn(rng, (n, Cc))
    wL, wR = randn(rng, (S, ln, Cc), basis == "complex"), randn(rng, (S, ln, Cc), basis == "complex")
    yaw, pitch, roll = (start + np.cumsum(rng.normal(0, 0.02, n)) for start in (0.5, 1.2, -0.3))
    got = run_bank(E, x, wL, wR, B, sigma, 2, (yaw, pitch, roll), basis)
    err = rel(got, oracle_sum(fitted_rotation(x, yaw, pitch, roll, N, basis), wL, wR, sigma, B))
    print("bank trajectory %s" % basis, "%.2e" % err)
    assert err <= TOL


# ---------------------------------------------------------------------------------------------------------------------------
# 7. designYawBank
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    from emagls_amd import synth
    azi, zen = synth.fibonacci_grid(900)
    hL, hR = synth.rigid_sphere_hrirs(azi, zen, taps=64)
    maz, mzn = synth.em32_grid()
    return dict(azi=azi, zen=zen, hL=hL, hR=hR, maz=maz, mzn=mzn, radius=synth.EM32_RADIUS)


@gpu
@pytest.mark.parametrize("kind", ["ls", "magls", "emagls2", "emagls", "fromatf"])
def test_design_yaw_bank_against_the_oracle(scene, kind):
    import emagls_amd as E
    c = scene
    yaw = np.array([0.0, 0.7, -2.1])
    if kind == "ls":
        wL, wR = E.designYawBank("ls", c["hL"], c["hR"], c["azi"], c["zen"], yaw, order=3)
        want = [O.getLsFilters(c["hL"], c["hR"], c["azi"] - t, c["zen"], 3, "real") for t in yaw]
    elif kind == "magls":
        wL, wR = E.designYawBank("magls", c["hL"], c["hR"], c["azi"], c["zen"], yaw, order=3, fs=48000.0, len=64)
        want = [O.getMagLsFilters(c["hL"], c["hR"], c["azi"] - t, c["zen"], 3, 48000.0, 64, "real") for t in yaw]
    elif kind == "emagls":
        yaw = yaw[:2]
        wL, wR = E.designYawBank("emagls", c["hL"], c["hR"], c["azi"], c["zen"], yaw, order=4, fs=48000.0, len=64, micRadius=c["radius"],
                                 micGridAziRad=c["maz"], micGridZenRad=c["mzn"], shDefinition="complex")
        want = [O.getEMagLsFilters(c["hL"], c["hR"], c["azi"] - t, c["zen"], c["radius"], c["maz"], c["mzn"], 4, 48000.0, 64, "complex")
                for t in yaw]
    elif kind == "fromatf":
        from emagls_amd import synth
        yaw = yaw[:2]
        atf, aazi, azen = synth.glasses_atfs(natf=1024, nmics=6, taps=48)
        ag = np.column_stack([aazi, azen])
        wL, wR = E.designYawBank("fromatf", c["hL"], c["hR"], c["azi"], c["zen"], yaw, fs=48000.0, len=64, atfIrs=atf, atfGridAziZenRad=ag,
                                 fTrans=2000.0)
        want = [O.getEMagLsFiltersFromAtf(c["hL"], c["hR"], np.column_stack([c["azi"] - t, c["zen"]]), atf, ag, 48000.0, 64, 2000.0)[:2]
                for t in yaw]
    else:
        yaw = yaw[:2]
        wL, wR = E.designYawBank("emagls2", c["hL"], c["hR"], c["azi"], c["zen"], yaw, order=4, fs=48000.0, len=64, micRadius=c["radius"],
                                 micGridAziRad=c["maz"], micGridZenRad=c["mzn"])
        want = [O.getEMagLs2Filters(c["hL"], c["hR"], c["azi"] - t, c["zen"], c["radius"], c["maz"], c["mzn"], 4, 48000.0, 64, "real")
                for t in yaw]
    assert wL.shape == (yaw.size,) + want[0][0].shape and wR.shape == wL.shape
    for j in range(yaw.size):
        eL, eR = rel(wL[j], want[j][0]), rel(wR[j], want[j][1])
        print("designYawBank %s yaw=%.2f" % (kind, yaw[j]), "%.2e %.2e" % (eL, eR))
        assert eL <= DESIGN_TOL and eR <= DESIGN_TOL
    assert rel(wL[1], wL[0]) > 1e-3       # the sets do differ


@gpu
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_ls_yaw_bank_equals_the_rotated_stream(scene, basis):
    """Set j with a constant index renders what the plain stream on the set for 0 renders when it is given yawRad[j] as its
    angle: the sign of the bank is the stream's yaw rule."""
    import emagls_amd as E
    c = scene
    rng = np.random.default_rng(9)
    N, B = 3, 64
    S = 8
    yaw = 2 * np.pi * np.arange(S) / S
    wL, wR = E.designYawBank("ls", c["hL"], c["hR"], c["azi"], c["zen"], yaw, order=N, shDefinition=basis)
    x = randn(rng, (4 * B, (N + 1) ** 2))
    for j in (1, 5):
        assert E.yawBankIndex(yaw[j] + 0.01, S) == j
        bank = run_bank(E, x, wL, wR, B, [j] * 4, basis=basis)
        turned = run_plain(E, x, wL[0], wR[0], B, (np.full(4 * B, yaw[j]), None, None), basis)
        err = rel(bank, turned)
        print("LS yaw bank vs rotated stream", basis, j, "%.2e" % err)
        assert err <= DESIGN_TOL
        assert rel(bank, run_plain(E, x, wL[0], wR[0], B, (np.full(4 * B, -yaw[j]), None, None), basis)) > 1e-2   # not the other sign


# ---------------------------------------------------------------------------------------------------------------------------
# 8. memory
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_create_destroy_of_a_bank_leaves_no_device_memory_behind():
    import torch
    import emagls_amd as E
    rng = np.random.default_rng(41)
    wL, wR, x = randn(rng, (6, 2048, 25)), randn(rng, (6, 2048, 25)), randn(rng, (256, 25))
    free = []
    for i in range(50):
        with E.BinauralDecodeStream(wL, wR, 64) as s:
            s.push(x, 0.1, 0.2, 0.3, setIndex=[0, 5, 5, 2])
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert free[49] >= free[1], (free[1], free[49])
