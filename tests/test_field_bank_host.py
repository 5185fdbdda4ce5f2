"""CPU-side checks of the bank of room responses on a field stream (emagls_field_stream_create_bank / _push_sets / _sets,
SourceFieldStream with 4-D rirs and setIndex): the cross-fade rule in its block form in NumPy -- a ring of
tagged window spectra, each multiplied with its own set's partition spectra -- against the oracle's sum
sum_q sum_s fftfilt(rir[s][q][:, c], g_sq x_q); that no window meets more than three sets; and every argument error, which the
library reports before it touches a device."""
import ctypes as C

import numpy as np
import pytest

from oracle import emagls_oracle as O

NEW = ["emagls_field_stream_create_bank", "emagls_field_stream_push_sets", "emagls_field_stream_push_sets_device", "emagls_field_stream_sets"]
TOL = 1e-13
# (n_sets, nsrc, nch, nr, B, complex response)
SHAPES = [(2, 1, 1, 1, 64, False), (3, 2, 3, 130, 64, False), (5, 3, 2, 200, 64, True), (4, 2, 2, 300, 128, False)]


def gains(idx, B, n_sets):
    """g [n_sets][nsrc][nb B] of the rule: idx [nsrc][nb]; sample i of block t of source q has the gain 1 for s_t when
    s_t == s_(t-1), otherwise r[i] = (i + 1) / B for s_t and 1 - r[i] for s_(t-1); s_(-1) := s_0."""
    nsrc, nb = idx.shape
    r = (np.arange(B) + 1.0) / B
    g = np.zeros((n_sets, nsrc, nb * B))
    for q in range(nsrc):
        for t in range(nb):
            now, before = idx[q, t], idx[q, max(t - 1, 0)]
            sl = slice(t * B, (t + 1) * B)
            if now == before:
                g[now, q, sl] = 1.0
            else:
                g[now, q, sl] = r
                g[before, q, sl] = 1.0 - r
    return g


def oracle_bank(s, rirs, g):
    """sum_q sum_s oracle.fftfilt(rir[s][q][:, c], g[s][q] x_q) (sets a source never visits add nothing and are left out)."""
    n_sets, nsrc, _, nch = rirs.shape
    out = np.zeros((s.shape[0], nch), dtype=rirs.dtype)
    for q in range(nsrc):
        for k in range(n_sets):
            if g[k, q].any():
                out += np.column_stack([O.fftfilt(rirs[k, q][:, c], g[k, q] * s[:, q]) for c in range(nch)])
    return out


def bank_spec(s, rirs, g, B):
    """The block form.  Per block and source the window [previous block, block] is transformed once under every set whose gains
    over the window are not all zero, and the spectra go into the ring slot as entries tagged with their set; the output block is
    the last B samples of IFFT(sum_q sum_p sum_entries ring[q][(pos - p) mod P][e] Rf[tag][q][p]).  Returns the output and the
    largest number of entries a slot ever held."""
    n, nsrc = s.shape
    n_sets, _, nr, nch = rirs.shape
    Nf, P = 2 * B, -(-nr // B)
    Rf = np.zeros((n_sets, nsrc, P, nch, Nf), dtype=np.complex128)
    for p in range(P):
        Rf[:, :, p] = np.fft.fft(rirs[:, :, p * B:(p + 1) * B].transpose(0, 1, 3, 2), Nf, axis=3)
    ring = [[[] for _ in range(P)] for _ in range(nsrc)]
    x = np.vstack([np.zeros((B, nsrc)), s])                       # (the block before the first is silence)
    gz = np.concatenate([np.zeros((n_sets, nsrc, B)), g], axis=2)
    out = np.zeros((n, nch), dtype=np.complex128)
    pos, most = 0, 0
    for t in range(n // B):
        pos = (pos + 1) % P
        w = slice(t * B, (t + 2) * B)                             # the window in x
        for q in range(nsrc):
            ring[q][pos] = [(k, np.fft.fft(gz[k, q, w] * x[w, q])) for k in range(n_sets) if gz[k, q, w].any()]
            most = max(most, len(ring[q][pos]))
        Y = np.zeros((nch, Nf), dtype=np.complex128)
        for q in range(nsrc):
            for p in range(P):
                for k, X in ring[q][(pos - p) % P]:
                    Y += X[None, :] * Rf[k, q, p]
        out[t * B:(t + 1) * B] = np.fft.ifft(Y, axis=1)[:, B:].T
    return (out if np.iscomplexobj(rirs) else out.real), most


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("n_sets,nsrc,nch,nr,B,cplx", SHAPES)
def test_block_form_of_the_rule(n_sets, nsrc, nch, nr, B, cplx):
    rng = np.random.default_rng(100 * n_sets + 10 * nsrc + nr)
    nb = -(-nr // B) + 9
    rirs = rng.standard_normal((n_sets, nsrc, nr, nch))
    if cplx:
        rirs = rirs + 1j * rng.standard_normal((n_sets, nsrc, nr, nch))
    s = rng.standard_normal((nb * B, nsrc))
    idx = rng.integers(0, n_sets, (nsrc, nb))
    g = gains(idx, B, n_sets)
    assert np.allclose(g.sum(axis=0), 1.0, rtol=0, atol=1e-15)    # the gains of a sample add up to 1
    spec, most = bank_spec(s, rirs, g, B)
    want = oracle_bank(s, rirs, g)
    err = rel(spec, want)
    print("block form", (n_sets, nsrc, nch, nr, B, cplx), "%.2e" % err, "entries", most)
    assert np.iscomplexobj(spec) == cplx and err <= TOL
    assert most <= 3 and most == min(3, n_sets)                   # no window meets more than three sets (and random indices reach that)


def test_no_window_meets_more_than_three_sets():
    """Every sequence of indices: the sets with a gain in the window of block t are among s_(t-2), s_(t-1), s_t."""
    rng = np.random.default_rng(5)
    B, n_sets = 4, 7
    idx = rng.integers(0, n_sets, (6, 200))
    g = gains(idx, B, n_sets)
    for q in range(idx.shape[0]):
        for t in range(idx.shape[1]):
            live = {k for k in range(n_sets) if g[k, q, max(t - 1, 0) * B:(t + 1) * B].any()}
            assert live <= {idx[q, max(t - 2, 0)], idx[q, max(t - 1, 0)], idx[q, t]} and 1 <= len(live) <= 3


@pytest.fixture(scope="module")
def lib():
    from emagls_amd import build, _lib
    build.build(jobs=4, verbose=False)
    return _lib.load()


def test_new_symbols_are_exported(lib):
    from emagls_amd import _lib as L
    raw = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in L.SYMBOLS


def create(lib, n_sets, nsrc=2, nch=3, nr=100, block=64, cplx=0):
    r = np.zeros(64)   # (an argument error is reported before the responses are read)
    if 1 <= n_sets * nsrc * nch * nr <= 1 << 20:
        r = np.zeros(n_sets * nsrc * nch * nr * (2 if cplx else 1))
    h = C.c_void_p()
    return lib.emagls_field_stream_create_bank(nsrc, nch, n_sets, r.ctypes.data_as(C.c_void_p), cplx, nr, block, C.byref(h)), h


def push_sets(lib, h, nsrc, nch, nsamp, sets, n_set=None):
    x, y = np.zeros(max(nsamp, 1) * nsrc), np.zeros(max(nsamp, 1) * nch * 2)
    a = None if sets is None else np.ascontiguousarray(sets, dtype=np.int32)
    return lib.emagls_field_stream_push_sets(h, x.ctypes.data_as(C.c_void_p), nsamp, None if a is None else a.ctypes.data_as(C.c_void_p),
                                             (0 if a is None else a.size) if n_set is None else n_set, y.ctypes.data_as(C.c_void_p))


def test_entry_point_argument_errors(lib):
    """Every check runs before the device is touched: with or without a GPU."""
    from emagls_amd import _lib as L
    for n_sets, code, text in ((0, L.ERR_ARG, b"at least one response set"), (-2, L.ERR_ARG, b"at least one response set"),
                               (65537, L.ERR_UNSUPPORTED, b"65536 response sets")):
        rc, h = create(lib, n_sets)
        assert rc == code and not h.value and text in lib.emagls_last_error(), (n_sets, rc, lib.emagls_last_error())
    # 25 channels, 48 000 taps at B = 64: 750 x 25 x 65 x 16 B = 19.5 MB per set, so 300 sets exceed 4 GiB
    rc, h = create(lib, 300, nsrc=1, nch=25, nr=48000, block=64)
    assert rc == L.ERR_UNSUPPORTED and not h.value and b"4 GiB" in lib.emagls_last_error()
    rc, h = create(lib, 3, nsrc=17)                               # every other limit as the plain stream's
    assert rc == L.ERR_UNSUPPORTED and b"16 sources" in lib.emagls_last_error()
    n = L.c_i64(0)
    assert lib.emagls_field_stream_sets(None, C.byref(n)) == L.ERR_ARG
    assert lib.emagls_field_stream_push_sets(None, None, 64, None, 0, None) == L.ERR_ARG
    assert lib.emagls_field_stream_push_sets_device(None, None, 64, None, 0, None, None) == L.ERR_ARG
    for cplx in (0, 1):
        n_sets, nsrc, nch, nr, B = 5, 3, 4, 200, 64               # P = 4
        rc, h = create(lib, n_sets, nsrc, nch, nr, B, cplx)
        assert rc == L.OK and h.value
        try:
            assert lib.emagls_field_stream_sets(h, C.byref(n)) == L.OK and n.value == n_sets
            assert lib.emagls_field_stream_sets(h, None) == L.ERR_ARG
            b, p, sb, rb, nl = L.c_i64(0), L.c_i64(0), L.c_i64(0), L.c_i64(0), C.c_int(0)
            assert lib.emagls_field_stream_info(h, C.byref(b), C.byref(p), C.byref(sb), C.byref(rb), C.byref(nl)) == L.OK
            assert (b.value, p.value, nl.value) == (64, 4, 2)
            # the ring with three entries per slot, the previous blocks, the position, the tags, the two previous indices
            assert sb.value == 16 * nsrc * 4 * 3 * 65 + 8 * nsrc * 64 + 4 + 4 * nsrc * 4 * 3 + 4 * nsrc * 2
            assert rb.value == 16 * n_sets * nsrc * 4 * (nch * (1 + cplx)) * 65
            for count in (1, 2, nsrc + 1, 2 * nsrc - 1, 2 * nsrc + 1, 4 * nsrc):       # a push of two blocks: 0, nsrc or 2 nsrc
                assert push_sets(lib, h, nsrc, nch, 2 * B, np.zeros(count)) == L.ERR_ARG, count
                assert b"set indices" in lib.emagls_last_error()
            assert push_sets(lib, h, nsrc, nch, 2 * B, None, n_set=nsrc) == L.ERR_ARG and b"null set index" in lib.emagls_last_error()
            some = C.cast(C.byref(b), C.c_void_p)                 # (not null: a wrong count or a null index array is refused before any is used)
            assert lib.emagls_field_stream_push_sets_device(h, some, 2 * B, None, 2 * nsrc, some, None) == L.ERR_ARG
            assert lib.emagls_field_stream_push_sets_device(h, some, 2 * B, some, nsrc + 1, some, None) == L.ERR_ARG
            for bad in (n_sets, -1):                                                  # named, and not a failure of the device
                for sets in ([0, bad, 0], [[0, 0], [0, 0], [0, bad]]):
                    assert push_sets(lib, h, nsrc, nch, 2 * B, sets) == L.ERR_ARG, (bad, sets)
                    assert b"set index %d outside [0, 4]" % bad in lib.emagls_last_error()
            assert push_sets(lib, h, nsrc, nch, 100, None) == L.ERR_ARG and b"multiple of the block size" in lib.emagls_last_error()
            assert push_sets(lib, h, nsrc, nch, 0, None) == L.OK                       # an empty push is no work
        finally:
            assert lib.emagls_field_stream_destroy(h) == L.OK
    # the bank of one set is the plain object: its state has no tags and one entry per slot, and only index 0 exists
    rc, h = create(lib, 1, nsrc=3, nch=5, nr=200, block=64)
    assert rc == L.OK
    try:
        sb, rb = L.c_i64(0), L.c_i64(0)
        assert lib.emagls_field_stream_info(h, None, None, C.byref(sb), C.byref(rb), None) == L.OK
        assert sb.value == 16 * 3 * 4 * 65 + 8 * 3 * 64 + 4 and rb.value == 16 * 3 * 4 * 5 * 65
        assert lib.emagls_field_stream_sets(h, C.byref(n)) == L.OK and n.value == 1
        assert push_sets(lib, h, 3, 5, 64, [0, 1, 0]) == L.ERR_ARG and b"set index 1 outside [0, 0]" in lib.emagls_last_error()
    finally:
        assert lib.emagls_field_stream_destroy(h) == L.OK


def test_python_set_index_errors(lib):
    import emagls_amd as E
    with pytest.raises(ValueError, match="numSets x numSources x nr x numChannels"):
        E.SourceFieldStream(np.zeros((2, 2, 2, 8, 4)), 64)
    with pytest.raises(ValueError, match="a bank needs at least one response set"):
        E.SourceFieldStream(np.zeros((0, 2, 8, 4)), 64)
    B = 64
    with E.SourceFieldStream(np.zeros((5, 3, 100, 4)), B) as f:
        assert (f.numSets, f.numSources, f.numChannels) == (5, 3, 4)
        assert f.info["response_bytes"] == 16 * 5 * 3 * 2 * 4 * 65
        x = np.zeros((2 * B, 3))
        for bad in (np.zeros(2, int), np.zeros((3, 3), int), np.zeros((2, 3), int), np.zeros((3, 2, 1), int), np.zeros(6, int)):
            with pytest.raises(ValueError, match=r"setIndex must be a scalar, \[numSources\] or \[numSources x n / blockSize\] = \[3 x 2\], not"):
                f.push(x, bad)
        with pytest.raises(ValueError, match="setIndex must be an integer or integers"):
            f.push(x, 1.0)
        for bad in (5, -1, [0, 5, 0], [[0, 0], [0, -1], [0, 0]]):
            with pytest.raises(ValueError, match=r"setIndex must lie in \[0, numSets - 1\] = \[0, 4\]"):
                f.push(x, bad)
    with E.SourceFieldStream(np.zeros((3, 100, 4)), B) as f:                         # a stream of one set takes the index 0 alone
        assert f.numSets == 1
        with pytest.raises(ValueError, match=r"= \[0, 0\]"):
            f.push(np.zeros((B, 3)), 1)
