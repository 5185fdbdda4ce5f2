"""The bank of room responses on a field stream (SourceFieldStream with 4-D rirs and setIndex, emagls_field_stream_create_bank /
_push_sets / _push_sets_device) on the GPU.  Expected values: the oracle's sum
sum_q sum_s oracle.fftfilt(rir[s][q][:, c], g_sq x_q) with the gains of the cross-fade rule (tests/test_field_bank_host.py).  Bound:
1e-12 relative to the largest output magnitude, the bound tests/test_gpu_field_stream.py holds the plain stream to.
Every parity case runs n = B (P + 4) samples, P = ceil(nr / B), so that the ring wraps -- but no fewer than six blocks: a standing
run of three blocks and three consecutive blocks that each change set do not fit into the five blocks P = 1 would give."""
import functools
import itertools

import numpy as np
import pytest

from oracle import emagls_oracle as O
from test_field_bank_host import gains, oracle_bank, rel
from test_gpu_field_stream import FittedRotation, on_device, walk
from test_mex_gateway import mex  # noqa: F401  (the stub mex.h harness)

gpu = pytest.mark.gpu
TOL = 1e-12
# (n_sets, nsrc, nch, nr, B, complex response)
SHAPES = [(2, 1, 1, 1, 64, False), (3, 2, 3, 130, 64, False), (5, 3, 2, 200, 64, False), (2, 1, 2, 300, 64, True),
          (4, 16, 2, 130, 64, False), (3, 1, 5, 700, 256, False), (2, 2, 3, 2049, 1024, False), (2, 1, 2, 4100, 2048, False)]


def blocks_of(nr, B):
    return max(-(-nr // B) + 4, 6)


def index_sequences(n_sets, nsrc, P, nb):
    """idx [nsrc][nb], deterministic: source q stands on A, goes A -> B -> C -> B in three consecutive blocks placed so that they
    cover block P - 1, whose spectrum goes into ring slot 0 (the wrap), and then stands on B.  (A, B, C) is the q-th ordered triple
    of sets (C = A in a bank of two), so the sources differ."""
    triples = list(itertools.permutations(range(n_sets), min(3, n_sets)))
    c = max(1, P - 2)
    idx = np.zeros((nsrc, nb), dtype=np.int32)
    for q in range(nsrc):
        t = triples[q % len(triples)]
        A, B_, C_ = t[0], t[1], t[2] if len(t) == 3 else t[0]
        idx[q] = [A] * c + [B_, C_] + [B_] * (nb - c - 2)
    return idx


def check_sequences(idx, n_sets, P):
    """The properties the parity test relies on, so that it cannot quietly degenerate."""
    nsrc, nb = idx.shape
    assert len({tuple(r) for r in idx}) == nsrc                                   # the sources differ
    for s in idx:
        change = [t > 0 and s[t] != s[t - 1] for t in range(nb)]
        assert any(s[t] == s[t + 1] == s[t + 2] for t in range(nb - 2))            # a standing run of three blocks
        runs = [t for t in range(1, nb - 2) if change[t] and change[t + 1] and change[t + 2]]
        assert runs                                                                # three consecutive blocks that each change set
        if n_sets >= 3:
            assert any(len({s[t - 1], s[t], s[t + 1], s[t + 2]}) >= 3 for t in runs)   # ... through three distinct sets
        assert any(s[t] != s[t + 1] and s[t + 2] == s[t] for t in range(nb - 2))    # A -> B -> A
        # block t goes into slot (t + 1) mod P: the ring wraps at t = P - 1 (with P = 1 at every block)
        assert (change[P - 1] if P > 1 else any(change))
        assert 0 <= s.min() and s.max() < n_sets


@functools.lru_cache(maxsize=None)
def case(n_sets, nsrc, nch, nr, B, cplx, nb=None):
    """Sources [n x nsrc], responses [n_sets x nsrc x nr x nch], indices [nsrc x nb] and the oracle's field, made once and shared."""
    rng = np.random.default_rng(10000 * n_sets + 1000 * nsrc + 10 * nch + nr + B)
    P = -(-nr // B)
    nb = nb or blocks_of(nr, B)
    rirs = rng.standard_normal((n_sets, nsrc, nr, nch))
    if cplx:
        rirs = rirs + 1j * rng.standard_normal((n_sets, nsrc, nr, nch))
    s = rng.standard_normal((nb * B, nsrc))
    idx = index_sequences(n_sets, nsrc, P, nb)
    check_sequences(idx, n_sets, P)
    want = oracle_bank(s, rirs, gains(idx, B, n_sets))
    for a in (s, rirs, idx, want):
        a.setflags(write=False)
    return s, rirs, idx, want


def run_bank(E, s, rirs, idx, B, group=1, f=None):
    """Push s through a (fresh) bank stream `group` blocks at a time with the indices of every block (host entry)."""
    def go(f):
        return np.vstack([f.push(s[i * B:(i + group) * B], None if idx is None else idx[:, i:i + group]) for i in range(0, s.shape[0] // B, group)])
    if f is not None:
        return go(f)
    with E.SourceFieldStream(rirs, B) as f:
        return go(f)


def run_plain(E, s, rirs, B):
    with E.SourceFieldStream(rirs, B) as f:
        return np.vstack([f.push(s[i:i + B]) for i in range(0, s.shape[0], B)])


# ---------------------------------------------------------------------------------------------------------------------------
# 1. parity
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n_sets,nsrc,nch,nr,B,cplx", SHAPES)
def test_parity(n_sets, nsrc, nch, nr, B, cplx):
    import emagls_amd as E
    s, rirs, idx, want = case(n_sets, nsrc, nch, nr, B, cplx)
    got = run_bank(E, s, rirs, idx, B)
    err = rel(got, want)
    print("bank parity", (n_sets, nsrc, nch, nr, B, cplx), "%.2e" % err)
    assert got.shape == (s.shape[0], nch) and np.iscomplexobj(got) == cplx and err <= TOL


# ---------------------------------------------------------------------------------------------------------------------------
# 2. bit equalities
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n_sets,nsrc,nch,nr,B,cplx", [SHAPES[1], SHAPES[3], SHAPES[4], SHAPES[6]])
def test_constant_index_gives_the_plain_streams_bits(n_sets, nsrc, nch, nr, B, cplx):
    import emagls_amd as E
    s, rirs, _, _ = case(n_sets, nsrc, nch, nr, B, cplx)
    nb = s.shape[0] // B
    for j in (0, n_sets - 1):
        plain = run_plain(E, s, rirs[j], B)
        assert np.abs(plain).max() > 0
        with E.SourceFieldStream(rirs, B) as f:
            every = np.vstack([f.push(s[i * B:(i + 1) * B], j) for i in range(nb)])          # the index in every push
        with E.SourceFieldStream(rirs, B) as f:
            first = np.vstack([f.push(s[i * B:(i + 1) * B], j if i == 0 else None) for i in range(nb)])   # ... and kept after the first
        assert np.array_equal(every, plain) and np.array_equal(first, plain), j


@gpu
def test_grouping_reset_and_fresh_objects():
    import emagls_amd as E
    n_sets, nsrc, nch, nr, B, cplx = SHAPES[2]
    s, rirs, idx, want = case(n_sets, nsrc, nch, nr, B, cplx, nb=9)
    one = run_bank(E, s, rirs, idx, B, 1)
    err = rel(one, want)
    print("bank grouping", "%.2e" % err)
    assert err <= TOL
    assert np.array_equal(run_bank(E, s, rirs, idx, B, 3), one)                    # 1 block against 3 blocks per push
    assert np.array_equal(run_bank(E, s, rirs, idx, B, 1), one)                    # equal pushes on two fresh objects
    with E.SourceFieldStream(rirs, B) as f:
        kept = run_bank(E, s, rirs, None, B, 1, f)                                 # a fresh object without indices: set 0
        assert np.array_equal(kept, run_plain(E, s, rirs[0], B))
        f.push(s[:2 * B], n_sets - 1)                                              # leave it on another set, in a fade
        f.reset()
        assert np.array_equal(run_bank(E, s, rirs, None, B, 1, f), kept)           # the selection is forgotten: set 0 again
        f.push(s[:3 * B], idx[:, :3])
        f.reset()
        assert np.array_equal(run_bank(E, s, rirs, idx, B, 1, f), one)             # a reset object equals a fresh one


@gpu
def test_bank_of_one_set_is_the_plain_stream():
    import emagls_amd as E
    _, nsrc, nch, nr, B, cplx = SHAPES[1]
    s, rirs, _, _ = case(3, nsrc, nch, nr, B, cplx)
    with E.SourceFieldStream(rirs[1], B) as f3, E.SourceFieldStream(rirs[1:2], B) as f4:
        assert (f3.numSets, f4.numSets) == (1, 1) and f3.info == f4.info
        a = np.vstack([f3.push(s[i:i + B]) for i in range(0, s.shape[0], B)])
        b = np.vstack([f4.push(s[i:i + B], 0) for i in range(0, s.shape[0], B)])
    assert np.abs(a).max() > 0 and np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. device entry
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]])
def test_device_entry_matches_host_entry(shape):
    import torch
    import emagls_amd as E
    n_sets, nsrc, nch, nr, B, cplx = shape
    s, rirs, idx, want = case(*shape)
    nb = s.shape[0] // B
    host = run_bank(E, s, rirs, idx, B)
    ts, ti = on_device(torch, s), on_device(torch, idx)
    assert ti.dtype == torch.int32
    outs = []
    with E.SourceFieldStream(rirs, B) as f:
        assert f.info["launches_per_block"] == 2
        for k in range(0, nb - 2):                                                  # every push enqueued, no synchronise in between
            outs.append(f.push(ts[k * B:(k + 1) * B], ti[:, k]))
        outs.append(f.push(ts[(nb - 2) * B:], ti[:, nb - 2:]))                      # ... and one of two blocks, [numSources x 2]
        got = torch.cat(outs).cpu().numpy()
    assert outs[0].shape == (B, nch) and outs[0].is_complex() == cplx and outs[0].t().is_contiguous()
    assert np.array_equal(got, host) and rel(got, want) <= TOL
    # indices outside the bank are clamped by the kernels: -5 is 0, n_sets + 7 is n_sets - 1
    wild = np.where(idx == 0, -5, np.where(idx == n_sets - 1, n_sets + 7, idx)).astype(np.int32)
    assert (wild < 0).any() and (wild >= n_sets).any()
    tw = on_device(torch, wild)
    with E.SourceFieldStream(rirs, B) as f:
        got = torch.cat([f.push(ts[k * B:(k + 1) * B], tw[:, k]) for k in range(nb)]).cpu().numpy()
    assert np.array_equal(got, host)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. chain
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_chain_into_a_decode_stream():
    import torch
    import emagls_amd as E
    n_sets, nsrc, nch, nr, B = 3, 2, 9, 300, 64
    s, rirs, idx, field = case(n_sets, nsrc, nch, nr, B, False)
    n = s.shape[0]
    rng = np.random.default_rng(79)
    wL, wR = rng.standard_normal((128, nch)), rng.standard_normal((128, nch))
    yaw = walk(rng, n, 0.02, 0.3)
    ts, ti, ty = on_device(torch, s), on_device(torch, idx), on_device(torch, yaw)
    outs = []
    with E.SourceFieldStream(rirs, B) as f, E.BinauralDecodeStream(wL, wR, B) as d:
        for k in range(n // B):                                                     # on the device, no host copy in between
            sl = slice(k * B, (k + 1) * B)
            outs.append(d.push(f.push(ts[sl], ti[:, k]), ty[sl]))
        got = torch.cat(outs).cpu().numpy()
    zero = np.zeros(n)
    want = O.binauralDecode(FittedRotation(2, "real").apply(field, yaw, zero, zero), wL, wR)
    err = rel(got, want)
    print("bank chain", "%.2e" % err)
    assert got.shape == (n, 2) and err <= TOL


# ---------------------------------------------------------------------------------------------------------------------------
# 5. memory
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_memory_and_cache_clear():
    import torch
    import emagls_amd as E
    from emagls_amd import _lib as L
    shape = SHAPES[1]
    s, rirs, idx, _ = case(*shape)
    B = shape[4]
    one = run_bank(E, s, rirs, idx, B)
    free = []
    for i in range(30):
        with E.SourceFieldStream(rirs, B) as f:
            f.push(s[:2 * B], idx[:, :2])
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert free[29] >= free[1], (free[1], free[29])
    with E.SourceFieldStream(rirs, B) as f:
        out = []
        for k in range(s.shape[0] // B):
            out.append(f.push(s[k * B:(k + 1) * B], idx[:, k]))
            if k == 2:
                L.check(L.load().emagls_cache_clear())                              # a cache clear leaves a live bank alone
        assert np.array_equal(np.vstack(out), one)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. MEX
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_mex_bank_matches_the_python_object(mex):  # noqa: F811
    import emagls_amd as E
    n_sets, nsrc, nch, nr, B = 3, 2, 3, 130, 64
    s, rirs, idx, _ = case(n_sets, nsrc, nch, nr, B, False)
    nb = s.shape[0] // B
    h = mex(1, "field_create", rirs.transpose(2, 3, 1, 0), B)[0].item()            # [nr x nch x 2 x 3]
    try:
        with E.SourceFieldStream(rirs, B) as f:
            for k in range(0, nb - 2):
                sl = slice(k * B, (k + 1) * B)
                got = mex(1, "field_push", h, s[sl], idx[:, k] + 1)[0]              # ONE-based, [numSources]
                assert np.array_equal(got, f.push(s[sl], idx[:, k])) and np.abs(got).max() > 0, k
            sl = slice((nb - 2) * B, nb * B)
            got = mex(1, "field_push", h, s[sl], idx[:, nb - 2:] + 1)[0]            # [numSources x 2]
            assert np.array_equal(got, f.push(s[sl], idx[:, nb - 2:]))
            got = mex(1, "field_push", h, s[:B], 3)[0]                              # a scalar: every source
            assert np.array_equal(got, f.push(s[:B], 2))
            got = mex(1, "field_push", h, s[:B])[0]                                 # none: kept
            assert np.array_equal(got, f.push(s[:B]))
    finally:
        mex(0, "field_destroy", h)
