"""CPU-side checks of the decode stream's bank of filter sets (emagls_decode_stream_create_bank / _push_sets, DESIGN.md section
9.4): the written specification of the cross-faded state update in NumPy against the oracle's sum over the sets, the sign of the
yaw bank on the oracle's LS filters, every argument error of the new entries (reported before a device is needed), and
yawBankIndex at the wrap-around."""
import ctypes as C

import numpy as np
import pytest

from oracle import emagls_oracle as O

NEW = ["emagls_decode_stream_create_bank", "emagls_decode_stream_push_sets", "emagls_decode_stream_push_sets_device",
       "emagls_decode_stream_sets"]


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def set_gains(sigma, B, S):
    """g [S x n]: the gain of every set per sample.  Block t: 1 for sigma_t when it equals sigma_(t-1); else r[i] = (i + 1) / B for
    sigma_t and 1 - r[i] for sigma_(t-1); sigma_(-1) := sigma_0."""
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
    """sum_s binauralDecode(g_s x, wL_s, wR_s): the expected output of a bank stream."""
    g = set_gains(sigma, B, wL.shape[0])
    return sum(O.binauralDecode(g[s][:, None] * x, wL[s], wR[s]) for s in range(wL.shape[0]) if np.any(g[s]))


def bank_spec(x, wL, wR, sigma, B):
    """The state update of the bank stream in NumPy: tests/test_decode_stream_host.py's stream_spec (a ring of P pending output
    spectra per ear) with the rule of section 9.4: the window [x_(t-1), x_t] meets the sets sigma_(t-2), sigma_(t-1), sigma_t; for
    every DISTINCT one, oldest role first, the window is transformed under that set's gain shapes (each half one of 0, 1, r,
    1 - r) and multiplied with that set's partition spectra into the same sums.  wL, wR [S x len x C].  Returns the output and
    the largest number of distinct sets a window met."""
    n, Cc = x.shape
    S, ln, Nf = wL.shape[0], wL.shape[1], 2 * B
    P = -(-ln // B)
    Wf = np.zeros((S, 2, P, Nf, Cc), dtype=np.complex128)
    for s in range(S):
        for e, w in enumerate((wL[s], wR[s])):
            for p in range(P):
                Wf[s, e, p] = np.fft.fft(w[p * B:(p + 1) * B], Nf, axis=0)
    ring = np.zeros((2, P, Nf), dtype=np.complex128)
    prev = np.zeros((B, Cc), dtype=x.dtype)
    out = np.zeros((n, 2))
    r = (np.arange(B) + 1.0) / B
    shape = {"0": np.zeros(B), "1": np.ones(B), "r": r, "1-r": 1.0 - r}
    pos, s1, s2, most = 0, -1, -1, 0
    for j in range(n // B):
        s0 = sigma[j]
        s1 = s0 if s1 < 0 else s1
        s2 = s1 if s2 < 0 else s2
        blk = x[j * B:(j + 1) * B]
        sets = []
        for u in (s2, s1, s0):
            if u not in sets:
                sets.append(u)
        most = max(most, len(sets))
        acc = np.zeros((2, P, Nf), dtype=np.complex128)
        for u in sets:
            a = ("1" if s1 == s2 else "r") if u == s1 else ("1-r" if u == s2 else "0")      # the gain of u in block t - 1
            b = ("1" if s0 == s1 else "r") if u == s0 else ("1-r" if u == s1 else "0")      # ... and in block t
            X = np.fft.fft(np.vstack([shape[a][:, None] * prev, shape[b][:, None] * blk]), axis=0)
            for e in range(2):
                for p in range(P):
                    acc[e, p] += (X * Wf[u, e, p]).sum(axis=1)
        for e in range(2):
            for p in range(P):
                slot = (pos + p) % P
                ring[e, slot] = acc[e, p] if p == P - 1 else ring[e, slot] + acc[e, p]
            out[j * B:(j + 1) * B, e] = np.fft.ifft(ring[e, pos])[B:].real
        pos = (pos + 1) % P
        prev = blk
        s2, s1 = s1, s0
    return out, most


def randn(rng, shape, cplx=False):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape) if cplx else rng.standard_normal(shape)


SEQS = {
    "constant": [2, 2, 2, 2, 2, 2, 2, 2],
    "every_block": [0, 1, 2, 3, 4, 0, 2, 4],          # three sets in every window
    "a_b_a": [0, 0, 1, 0, 0, 3, 0, 3],
    "first_and_last": [0, 1, 1, 1, 1, 1, 1, 4],       # a switch in block 1 (the first that can fade) and in the last block
    "hold_then_run": [3, 3, 3, 1, 4, 4, 0, 0],
}


@pytest.mark.parametrize("name", sorted(SEQS))
@pytest.mark.parametrize("Cc,ln,B", [(8, 300, 64), (4, 64, 64), (6, 40, 64), (3, 1, 64), (5, 200, 128)])
def test_numpy_specification_against_oracle_sum(name, Cc, ln, B):
    """len not a multiple of B (300, 200), len = B, len < B (40), len = 1."""
    sigma = SEQS[name]
    rng = np.random.default_rng(Cc + ln + B)
    x, wL, wR = randn(rng, (len(sigma) * B, Cc)), randn(rng, (5, ln, Cc)), randn(rng, (5, ln, Cc))
    got, most = bank_spec(x, wL, wR, sigma, B)
    err = rel(got, oracle_sum(x, wL, wR, sigma, B))
    print("bank spec", name, (Cc, ln, B), "%.2e" % err, "sets per window <= %d" % most)
    assert err <= 1e-12
    assert most == {"constant": 1, "every_block": 3}.get(name, most) and most <= 3


def test_numpy_specification_complex_signal_and_filters():
    rng = np.random.default_rng(7)
    sigma = [1, 0, 0, 2, 1, 2]
    x, wL, wR = randn(rng, (6 * 64, 9), True), randn(rng, (3, 100, 9), True), randn(rng, (3, 100, 9), True)
    assert rel(bank_spec(x, wL, wR, sigma, 64)[0], oracle_sum(x, wL, wR, sigma, 64)) <= 1e-12


def test_constant_index_is_the_plain_specification():
    from test_decode_stream_host import stream_spec
    rng = np.random.default_rng(8)
    x, wL, wR = randn(rng, (5 * 64, 4)), randn(rng, (3, 150, 4)), randn(rng, (3, 150, 4))
    got, most = bank_spec(x, wL, wR, [1] * 5, 64)
    assert most == 1 and np.array_equal(got, stream_spec(x, wL[1], wR[1], 64))


# ---- the sign of the yaw bank, on the oracle alone
def _fibonacci(n):
    i = np.arange(n) + 0.5
    return np.mod(np.pi * (1 + 5 ** 0.5) * i, 2 * np.pi), np.arccos(1 - 2 * i / n)


@pytest.mark.parametrize("basis", ["real", "complex"])
def test_ls_filters_on_the_turned_grid_pin_the_sign(basis):
    """Set theta = LS filters on azi - theta.  It decodes the plane wave from azimuth a as the set for 0 decodes the plane wave
    from a + theta (an identity for LS filters: both are the order-limited HRIR of direction a + theta); azi + theta must not."""
    rng = np.random.default_rng(12)
    N, D, taps, theta = 3, 240, 32, 0.7
    azi, zen = _fibonacci(D)
    hL, hR = rng.standard_normal((taps, D)), rng.standard_normal((taps, D))
    w0 = O.getLsFilters(hL, hR, azi, zen, N, basis)
    wm = O.getLsFilters(hL, hR, azi - theta, zen, N, basis)
    wp = O.getLsFilters(hL, hR, azi + theta, zen, N, basis)
    src = np.array([[0.4, 1.1], [2.9, 0.6], [5.0, 2.2]])
    n = 8

    def wave(shift):
        y = np.conj(O.getSH(N, np.column_stack([src[:, 0] + shift, src[:, 1]]), basis))    # [3 x C]
        x = np.zeros((n, y.shape[1]), dtype=y.dtype)
        x[0], x[3], x[5] = y[0], -0.5 * y[1], 2.0 * y[2]
        return x.real if basis == "real" else x
    want = O.binauralDecode(wave(theta), w0[0], w0[1])
    good = rel(O.binauralDecode(wave(0.0), wm[0], wm[1]), want)
    bad = rel(O.binauralDecode(wave(0.0), wp[0], wp[1]), want)
    print("yaw bank sign", basis, "%.2e" % good, "%.2e" % bad)
    assert good <= 1e-12
    assert bad > 1e-2


# ---- the library's host side
@pytest.fixture(scope="module")
def lib():
    from emagls_amd import build, _lib
    build.build(jobs=4, verbose=False)
    return _lib.load()


def test_new_symbols_are_exported(lib):
    import os
    import re
    from emagls_amd import _lib as L
    raw = C.CDLL(L.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "emagls.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(emagls_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in L.SYMBOLS and name in declared


def create_bank(lib, nch, n_sets, ln=8, block=64, null=False):
    w = np.zeros((max(n_sets, 1) * ln * nch,))
    pw = None if null else w.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()
    rc = lib.emagls_decode_stream_create_bank(nch, n_sets, pw, w.ctypes.data_as(C.c_void_p), 0, ln, 0, 0, 0, block, C.byref(h))
    return rc, h


def push_sets(lib, h, nch, nsamp, sets, n_set=None):
    x, out = np.zeros((max(nsamp, 1), nch), order="F"), np.zeros((max(nsamp, 1), 2), order="F")
    a = None if sets is None else np.ascontiguousarray(sets, dtype=np.int32)
    return lib.emagls_decode_stream_push_sets(h, x.ctypes.data_as(C.c_void_p), nsamp, None if a is None else a.ctypes.data_as(C.c_void_p),
                                              (0 if a is None else a.size) if n_set is None else n_set, None, 0, None, 0, None, 0,
                                              out.ctypes.data_as(C.c_void_p))


def test_entry_point_argument_errors(lib):
    """Every check runs before the device is touched: with or without a GPU."""
    from emagls_amd import _lib as L
    for n_sets in (0, -3):
        rc, h = create_bank(lib, 4, n_sets)
        assert rc == L.ERR_ARG and not h.value, n_sets
    assert b"filter set" in lib.emagls_last_error()
    assert create_bank(lib, 4, 2, null=True)[0] == L.ERR_ARG
    assert create_bank(lib, 4, 65537)[0] == L.ERR_UNSUPPORTED
    assert create_bank(lib, 4, 2, block=48)[0] == L.ERR_UNSUPPORTED
    assert create_bank(lib, 0, 2)[0] == L.ERR_ARG
    n = L.c_i64(0)
    assert lib.emagls_decode_stream_sets(None, C.byref(n)) == L.ERR_ARG
    assert push_sets(lib, None, 4, 64, [0]) == L.ERR_ARG
    rc, h = create_bank(lib, 4, 3, ln=200)
    assert rc == L.OK and h.value
    try:
        assert lib.emagls_decode_stream_sets(h, C.byref(n)) == L.OK and n.value == 3
        assert lib.emagls_decode_stream_sets(h, None) == L.ERR_ARG
        b, p, sb, fb, nl = L.c_i64(0), L.c_i64(0), L.c_i64(0), L.c_i64(0), C.c_int(0)
        assert lib.emagls_decode_stream_info(h, C.byref(b), C.byref(p), C.byref(sb), C.byref(fb), C.byref(nl)) == L.OK
        assert (b.value, p.value, nl.value) == (64, 4, 3)                      # still at most three launches per block
        assert fb.value == 3 * 16 * 2 * 4 * 4 * 65                             # the spectra of three sets
        assert sb.value == 16 * 2 * 4 * 65 + 8 * 4 * 64 + 4 + 2 * 4            # ... and the two previous indices beside the position
        for bad in ([3], [-1], [0, 5], [2, -2]):                              # an index outside [0, S - 1]
            assert push_sets(lib, h, 4, 128, bad) == L.ERR_ARG, bad
            assert b"set index" in lib.emagls_last_error()
        for count in (3, 4, -1):                                              # counts outside {0, 1, nsamp / block}
            assert push_sets(lib, h, 4, 128, [0, 0, 0, 0], n_set=count) == L.ERR_ARG, count
        assert push_sets(lib, h, 4, 128, None, n_set=1) == L.ERR_ARG           # a null array with a count
        assert push_sets(lib, h, 4, 100, [0]) == L.ERR_ARG                     # not a multiple of the block
        assert push_sets(lib, h, 4, 0, None) == L.OK                           # nothing to do is no error
    finally:
        assert lib.emagls_decode_stream_destroy(h) == L.OK
    rc, h = create_bank(lib, 4, 1)                                             # the bank of one set is the plain stream
    assert rc == L.OK and lib.emagls_decode_stream_sets(h, C.byref(n)) == L.OK and n.value == 1
    assert push_sets(lib, h, 4, 64, [1]) == L.ERR_ARG
    lib.emagls_decode_stream_destroy(h)


def test_python_argument_errors(lib):
    import emagls_amd as E
    w3 = np.zeros((3, 8, 16))
    with pytest.raises(ValueError, match="equal shape"):
        E.BinauralDecodeStream(w3, np.zeros((2, 8, 16)), 64)
    with pytest.raises(ValueError, match="equal shape"):
        E.BinauralDecodeStream(np.zeros((2, 3, 8, 16)), np.zeros((2, 3, 8, 16)), 64)
    with pytest.raises(ValueError, match="at least one filter set"):
        E.BinauralDecodeStream(np.zeros((0, 8, 16)), np.zeros((0, 8, 16)), 64)
    with E.BinauralDecodeStream(w3[0], w3[0], 64) as s:
        assert s.numSets == 1
        with pytest.raises(ValueError, match="numSets - 1"):
            s.push(np.zeros((64, 16)), setIndex=1)
    with E.BinauralDecodeStream(w3, w3, 64) as s:
        assert s.numSets == 3 and s.numChannels == 16 and s.info["launches_per_block"] <= 3
        x = np.zeros((128, 16))
        with pytest.raises(ValueError, match="numSets - 1"):
            s.push(x, setIndex=3)
        with pytest.raises(ValueError, match="numSets - 1"):
            s.push(x, setIndex=[0, -1])
        with pytest.raises(ValueError, match="one index per block"):
            s.push(x, setIndex=[0, 1, 2])
        with pytest.raises(ValueError, match="integer"):
            s.push(x, setIndex=0.5)
        with pytest.raises(ValueError, match="multiple of blockSize"):
            s.push(np.zeros((100, 16)), setIndex=0)
    with pytest.raises(ValueError, match="kind must be one of"):
        E.designYawBank("emainch", np.zeros((8, 4)), np.zeros((8, 4)), np.zeros(4), np.zeros(4), [0.0])
    with pytest.raises(ValueError, match="at least one angle"):
        E.designYawBank("ls", np.zeros((8, 4)), np.zeros((8, 4)), np.zeros(4), np.zeros(4), [])
    with pytest.raises(ValueError, match="micGridAziRad"):
        E.designYawBank("emagls2", np.zeros((8, 4)), np.zeros((8, 4)), np.zeros(4), np.zeros(4), [0.0])
    with pytest.raises(ValueError, match="numSets"):
        E.yawBankIndex(0.0, 0)


def test_yaw_bank_index_wraps():
    import emagls_amd as E
    S, step, eps = 360, 2 * np.pi / 360, 1e-9
    assert E.yawBankIndex(0.0, S) == 0 and isinstance(E.yawBankIndex(0.0, S), int)
    assert E.yawBankIndex(-eps, S) == 0                       # just below 0: set 0, not S
    assert E.yawBankIndex(2 * np.pi - eps, S) == 0            # just below a full turn: set 0, not S
    assert E.yawBankIndex(2 * np.pi - 0.6 * step, S) == S - 1
    assert E.yawBankIndex(-0.6 * step, S) == S - 1
    assert E.yawBankIndex(0.4 * step, S) == 0 and E.yawBankIndex(0.6 * step, S) == 1
    assert E.yawBankIndex(-np.pi / 2, 8) == 6                 # negative angles
    assert E.yawBankIndex(6 * np.pi + np.pi / 4, 8) == 1      # multi-turn, both ways
    assert E.yawBankIndex(-8 * np.pi - np.pi / 4, 8) == 7
    a = E.yawBankIndex(np.array([[-eps, 2 * np.pi - eps], [np.pi, -40 * np.pi + step]]), S)
    assert a.dtype == np.int32 and a.shape == (2, 2) and a.tolist() == [[0, 0], [180, 1]]
    j = E.yawBankIndex(np.linspace(-50, 50, 20001), 7)
    assert j.min() == 0 and j.max() == 6
    assert E.yawBankIndex(123.4, 1) == 0
