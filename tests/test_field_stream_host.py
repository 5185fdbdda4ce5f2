"""CPU-side checks of the field stream (emagls_field_stream_*, SourceFieldStream): the written specification
of its state update in NumPy, checked against the oracle's fftfilt sum and against np.convolve, the exports, and every argument
error, which the library reports before it touches a device."""
import ctypes as C

import numpy as np
import pytest

from oracle import emagls_oracle as O

NEW = ["emagls_field_stream_create", "emagls_field_stream_push", "emagls_field_stream_push_device", "emagls_field_stream_reset",
       "emagls_field_stream_info", "emagls_field_stream_destroy"]
# (nsrc, nch, nr, B, complex response)
SHAPES = [(1, 4, 1, 64, False), (1, 25, 300, 64, False), (2, 9, 700, 128, False), (3, 5, 4100, 2048, False), (1, 64, 1000, 256, False),
          (16, 2, 130, 64, False), (1, 1, 2561, 64, False), (2, 9, 300, 64, True), (1, 25, 600, 512, True), (3, 3, 2049, 1024, False)]
TOL = 1e-12   # the bound the GPU tests hold the kernels to (tests/test_gpu_field_stream.py); the three agree to 7e-16 here


def field_spec(s, rirs, B):
    """The state update of the field stream, in NumPy.  s [n x nsrc] real with n = k B; rirs [nsrc x nr x nch], real or complex.
    The responses are cut into P = ceil(nr / B) partitions, as `planes` real planes (a complex response: plane 2c its real, 2c + 1
    its imaginary taps), each transformed at Nf = 2B and kept up to bin B.  The state is the ring of the last P INPUT spectra per
    source, the previous block and the position.  Per block: the windows [hist_q, block_q], two real sources per packed transform,
    go into ring slot pos + 1 and pos moves on; then, per pair of planes (a, b), A = sum_q sum_p ring[q][(pos - p) mod P] Rf[q][p][a]
    and B likewise, A + iB goes back in one inverse transform, and the last B samples are plane a (real part) and plane b
    (imaginary part): two columns, or the real and the imaginary part of one complex column."""
    n, nsrc = s.shape
    nr, nch = rirs.shape[1:]
    cplx = np.iscomplexobj(rirs)
    Nf, P, Pf = 2 * B, -(-nr // B), B + 1
    planes = 2 * nch if cplx else nch
    rpl = np.zeros((nsrc, planes, nr))
    for q in range(nsrc):
        if cplx:
            rpl[q, 0::2], rpl[q, 1::2] = rirs[q].real.T, rirs[q].imag.T
        else:
            rpl[q] = rirs[q].T
    Rf = np.zeros((nsrc, P, planes, Pf), dtype=np.complex128)
    for p in range(P):
        Rf[:, p] = np.fft.fft(rpl[:, :, p * B:(p + 1) * B], Nf, axis=2)[:, :, :Pf]
    ring = np.zeros((nsrc, P, Pf), dtype=np.complex128)
    hist = np.zeros((nsrc, B))
    pos = 0
    out = np.zeros((n, planes))
    k = np.arange(Pf)
    for j in range(n // B):
        blk = s[j * B:(j + 1) * B].T                                           # [nsrc][B]
        slot = (pos + 1) % P
        for qa in range(0, nsrc, 2):                                           # two real sources per packed transform
            qb = qa + 1
            win = np.concatenate([hist[qa], blk[qa]]) + (1j * np.concatenate([hist[qb], blk[qb]]) if qb < nsrc else 0)
            Z = np.fft.fft(win)
            Zr = np.conj(Z[(Nf - k) % Nf])
            ring[qa, slot] = 0.5 * (Z[k] + Zr)
            if qb < nsrc:
                ring[qb, slot] = -0.5j * (Z[k] - Zr)
        hist = blk.copy()
        pos = slot
        for a in range(0, planes, 2):
            acc = np.zeros((2, Pf), dtype=np.complex128)
            for q in range(nsrc):
                for p in range(P):
                    x = ring[q, (pos - p) % P]
                    acc[0] += x * Rf[q, p, a]
                    if a + 1 < planes:
                        acc[1] += x * Rf[q, p, a + 1]
            Y = np.zeros(Nf, dtype=np.complex128)
            Y[:Pf] = acc[0] + 1j * acc[1]
            Y[Pf:] = (np.conj(acc[0]) + 1j * np.conj(acc[1]))[B - 1:0:-1]       # Y[Nf - k], 0 < k < B
            y = np.fft.ifft(Y)[B:]
            out[j * B:(j + 1) * B, a] = y.real
            if a + 1 < planes:
                out[j * B:(j + 1) * B, a + 1] = y.imag
    return out[:, 0::2] + 1j * out[:, 1::2] if cplx else out


def make(nsrc, nch, nr, B, cplx, seed=0):
    rng = np.random.default_rng(1000 * nsrc + 10 * nch + nr + B + seed)
    n = B * (-(-nr // B) + 3)                                                   # the ring wraps
    rirs = rng.standard_normal((nsrc, nr, nch))
    if cplx:
        rirs = rirs + 1j * rng.standard_normal((nsrc, nr, nch))
    return rng.standard_normal((n, nsrc)), rirs


def oracle_field(s, rirs):
    """sum_q oracle.fftfilt(rir_q(:, c), s_q)"""
    return sum(np.column_stack([O.fftfilt(rirs[q][:, c], s[:, q]) for c in range(rirs.shape[2])]) for q in range(rirs.shape[0]))


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("nsrc,nch,nr,B,cplx", SHAPES)
def test_numpy_specification(nsrc, nch, nr, B, cplx):
    s, rirs = make(nsrc, nch, nr, B, cplx)
    n = s.shape[0]
    spec = field_spec(s, rirs, B)
    want = oracle_field(s, rirs)
    conv = sum(np.column_stack([np.convolve(rirs[q][:, c], s[:, q])[:n] for c in range(nch)]) for q in range(nsrc))
    e1, e2, e3 = rel(spec, want), rel(spec, conv), rel(want, conv)
    print("spec", (nsrc, nch, nr, B, cplx), "%.2e %.2e %.2e" % (e1, e2, e3))
    assert spec.shape == (n, nch) and np.iscomplexobj(spec) == cplx
    assert e1 <= TOL and e2 <= TOL and e3 <= TOL


@pytest.fixture(scope="module")
def lib():
    from emagls_amd import build, _lib
    build.build(jobs=4, verbose=False)
    return _lib.load()


def test_new_symbols_are_exported(lib):
    import emagls_amd as E
    from emagls_amd import _lib as L
    raw = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in L.SYMBOLS
    assert "SourceFieldStream" in E.__all__ and callable(E.SourceFieldStream)


def test_header_and_binding_agree(lib):
    import os
    import re
    from emagls_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "emagls.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(emagls_[a-z0-9_]+)\s*\(", hdr))
    assert set(NEW) <= declared and declared == set(L.SYMBOLS)


def create(lib, nsrc=1, nch=4, nr=8, block=64, cplx=0, rir=True, out=True):
    r = np.zeros(64)   # (an argument error is reported before the responses are read)
    if nsrc >= 1 and nch >= 1 and nr >= 1 and nsrc * nch * nr * (2 if cplx else 1) <= 1 << 20:
        r = np.zeros(nsrc * nch * nr * (2 if cplx else 1))
    h = C.c_void_p()
    rc = lib.emagls_field_stream_create(nsrc, nch, r.ctypes.data_as(C.c_void_p) if rir else None, cplx, nr, block, C.byref(h) if out else None)
    return rc, h


def push(lib, h, nsrc, nch, nsamp, src=True, out=True):
    x, y = np.zeros(max(nsamp, 1) * nsrc), np.zeros(max(nsamp, 1) * nch * 2)
    return lib.emagls_field_stream_push(h, x.ctypes.data_as(C.c_void_p) if src else None, nsamp, y.ctypes.data_as(C.c_void_p) if out else None)


def test_entry_point_argument_errors(lib):
    """Every check runs before the device is touched: with or without a GPU."""
    from emagls_amd import _lib as L

    def refused(code, text, **kw):
        rc, h = create(lib, **kw)
        msg = lib.emagls_last_error()
        assert rc == code and not h.value and text in msg, (kw, rc, msg)

    for block in (48, 32, 4096, 0, -64):
        refused(L.ERR_UNSUPPORTED, b"block size", block=block)
    refused(L.ERR_UNSUPPORTED, b"16 sources", nsrc=17)
    refused(L.ERR_UNSUPPORTED, b"256 channels", nch=257)
    refused(L.ERR_UNSUPPORTED, b"1048576 taps", nr=1048577)
    refused(L.ERR_UNSUPPORTED, b"4 GiB", nsrc=16, nch=256, nr=1048576, block=64)
    # 16 x 1024 x 256 x 65 x 16 B = 4 GiB + 64 MiB with a real response; a complex one doubles the planes
    refused(L.ERR_UNSUPPORTED, b"4 GiB", nsrc=16, nch=256, nr=65536, block=64)
    refused(L.ERR_UNSUPPORTED, b"4 GiB", nsrc=8, nch=256, nr=65536, block=64, cplx=1)
    for kw in (dict(nsrc=0), dict(nch=0), dict(nr=0), dict(nsrc=-1), dict(nch=-3), dict(nr=-5)):
        refused(L.ERR_ARG, b"invalid shape", **kw)
    refused(L.ERR_ARG, b"null pointer", rir=False)
    assert create(lib, out=False)[0] == L.ERR_ARG and b"null pointer" in lib.emagls_last_error()
    # null handle
    assert push(lib, None, 1, 4, 64) == L.ERR_ARG and b"null field stream" in lib.emagls_last_error()
    assert lib.emagls_field_stream_push_device(None, None, 64, None, None) == L.ERR_ARG
    assert lib.emagls_field_stream_reset(None) == L.ERR_ARG
    assert lib.emagls_field_stream_info(None, None, None, None, None, None) == L.ERR_ARG
    assert lib.emagls_field_stream_destroy(None) == L.OK
    # the object exists without a device: created, queried and destroyed
    for cplx in (0, 1):
        rc, h = create(lib, nsrc=3, nch=5, nr=200, block=64, cplx=cplx)
        assert rc == L.OK and h.value
        try:
            b, p, sb, rb, nl = L.c_i64(0), L.c_i64(0), L.c_i64(0), L.c_i64(0), C.c_int(0)
            assert lib.emagls_field_stream_info(h, C.byref(b), C.byref(p), C.byref(sb), C.byref(rb), C.byref(nl)) == L.OK
            assert (b.value, p.value, nl.value) == (64, 4, 2)
            assert sb.value == 16 * 3 * 4 * 65 + 8 * 3 * 64 + 4 and rb.value == 16 * 3 * 4 * (5 * (1 + cplx)) * 65
            assert lib.emagls_field_stream_info(h, None, None, None, None, None) == L.OK      # each output is optional
            assert push(lib, h, 3, 5, 100) == L.ERR_ARG and b"multiple of the block size" in lib.emagls_last_error()
            assert push(lib, h, 3, 5, -64) == L.ERR_ARG
            assert push(lib, h, 3, 5, 64, src=False) == L.ERR_ARG and b"null pointer" in lib.emagls_last_error()
            assert push(lib, h, 3, 5, 64, out=False) == L.ERR_ARG
            assert lib.emagls_field_stream_push_device(h, None, 64, None, None) == L.ERR_ARG
            assert push(lib, h, 3, 5, 0) == L.OK                                               # an empty push is no work
        finally:
            assert lib.emagls_field_stream_destroy(h) == L.OK


def test_python_argument_errors(lib):
    import emagls_amd as E
    from emagls_amd import _lib as L
    r = np.zeros((8, 16))
    for bad, code, text in ((dict(rirs=r, blockSize=48), L.ERR_UNSUPPORTED, "block size"),
                            (dict(rirs=np.zeros((17, 2, 2)), blockSize=64), L.ERR_UNSUPPORTED, "16 sources"),
                            (dict(rirs=np.zeros((2, 257)), blockSize=64), L.ERR_UNSUPPORTED, "256 channels"),
                            (dict(rirs=np.zeros((1048577, 1)), blockSize=64), L.ERR_UNSUPPORTED, "1048576 taps"),
                            (dict(rirs=np.zeros((0, 4)), blockSize=64), L.ERR_ARG, "invalid shape"),
                            (dict(rirs=np.zeros((4, 0)), blockSize=64), L.ERR_ARG, "invalid shape"),
                            (dict(rirs=np.zeros((0, 4, 4)), blockSize=64), L.ERR_ARG, "invalid shape")):
        with pytest.raises(L.EmaglsError, match=text) as e:
            E.SourceFieldStream(**bad)
        assert e.value.code == code
    with pytest.raises(ValueError, match="numSources x nr x numChannels"):
        E.SourceFieldStream(np.zeros(8), 64)
    with pytest.raises(ValueError, match="blockSize must be an integer"):
        E.SourceFieldStream(r, 64.5)
    with E.SourceFieldStream(np.zeros((2, 100, 16)), 64) as f:
        assert f.info == {"block": 64, "partitions": 2, "state_bytes": 16 * 2 * 2 * 65 + 8 * 2 * 64 + 4,
                          "response_bytes": 16 * 2 * 2 * 16 * 65, "launches_per_block": 2}
        assert (f.numSources, f.numChannels, f.complexOutput) == (2, 16, False)
        with pytest.raises(ValueError, match="multiple of blockSize"):
            f.push(np.zeros((100, 2)))
        with pytest.raises(ValueError, match="source count"):
            f.push(np.zeros((64, 3)))
        with pytest.raises(ValueError, match="source count"):
            f.push(np.zeros(64))                                  # [n] is one source's block
        with pytest.raises(ValueError, match="real source signals"):
            f.push(np.zeros((64, 2), dtype=complex))
    with pytest.raises(ValueError, match="closed"):
        f.push(np.zeros((64, 2)))
    with E.SourceFieldStream(r + 0j, 64) as f:
        assert f.complexOutput and f.info["response_bytes"] == 16 * 1 * 1 * 32 * 65


def test_python_closed_and_host_tensor_texts(lib):
    import torch
    import emagls_amd as E
    f = E.SourceFieldStream(np.zeros((8, 4)), 64)
    with pytest.raises(ValueError, match=r"^a torch block must be on the GPU \(pass a NumPy array for the host entry\)$"):
        f.push(torch.zeros(64, dtype=torch.float64))
    with pytest.raises(ValueError, match="multiple of blockSize"):      # (the shape is looked at first)
        f.push(torch.zeros(100, dtype=torch.float64))
    f.close()
    f.close()
    for call in (lambda: f.push(np.zeros(64)), lambda: f.info, f.reset):
        with pytest.raises(ValueError, match="^the field stream is closed$"):
            call()
