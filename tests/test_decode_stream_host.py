"""CPU-side checks of the decode stream (emagls_decode_stream_*, BinauralDecodeStream): the written specification of its state
update in NumPy, checked against the oracle, and every argument error, which the library reports before it touches a device."""
import ctypes as C

import numpy as np
import pytest

from oracle import emagls_oracle as O

NEW = ["emagls_decode_stream_create", "emagls_decode_stream_push", "emagls_decode_stream_push_device", "emagls_decode_stream_reset",
       "emagls_decode_stream_info", "emagls_decode_stream_destroy"]
SHAPES = [(25, 512, 64), (25, 512, 1024), (64, 2048, 256), (9, 4096, 64), (25, 512, 2048), (256, 512, 128), (25, 300, 64)]   # (C, len, B)


def stream_spec(x, wL, wR, B):
    """The state update of the decode stream, in NumPy: uniformly partitioned overlap-save with a ring of P = ceil(len / B)
    pending output spectra per ear.  Block j, behind its predecessor, has the spectrum X_j (length 2B); X_j W_p is added into
    the slot of output block j + p -- partition P - 1 stores, its slot has just been given up -- and the block's own slot is
    transformed back; its last B samples go out.  x [n x C] with n = k B, filters [len x C]; real part of the result."""
    n, Cc = x.shape
    ln, Nf = wL.shape[0], 2 * B
    P = -(-ln // B)
    Wf = np.zeros((2, P, Nf, Cc), dtype=np.complex128)
    for e, w in enumerate((wL, wR)):
        for p in range(P):
            Wf[e, p] = np.fft.fft(w[p * B:(p + 1) * B], Nf, axis=0)
    ring = np.zeros((2, P, Nf), dtype=np.complex128)
    prev = np.zeros((B, Cc), dtype=x.dtype)
    out = np.zeros((n, 2))
    pos = 0
    for j in range(n // B):
        blk = x[j * B:(j + 1) * B]
        X = np.fft.fft(np.vstack([prev, blk]), axis=0)
        for e in range(2):
            for p in range(P):
                acc = (X * Wf[e, p]).sum(axis=1)
                slot = (pos + p) % P
                ring[e, slot] = acc if p == P - 1 else ring[e, slot] + acc
            out[j * B:(j + 1) * B, e] = np.fft.ifft(ring[e, pos])[B:].real
        pos = (pos + 1) % P
        prev = blk
    return out


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("Cc,ln,B", SHAPES)
def test_numpy_specification_against_oracle(Cc, ln, B):
    rng = np.random.default_rng(Cc + ln + B)
    n = B * max(3, -(-ln // B) + 2)
    x, wL, wR = rng.standard_normal((n, Cc)), rng.standard_normal((ln, Cc)), rng.standard_normal((ln, Cc))
    assert rel(stream_spec(x, wL, wR, B), O.binauralDecode(x, wL, wR)) <= 1e-12


def test_numpy_specification_complex_and_one_tap():
    rng = np.random.default_rng(3)
    cx = lambda r, c: rng.standard_normal((r, c)) + 1j * rng.standard_normal((r, c))   # noqa: E731
    x, wL, wR = cx(256, 9), cx(100, 9), cx(100, 9)
    assert rel(stream_spec(x, wL, wR, 64), O.binauralDecode(x, wL, wR)) <= 1e-12
    x, wL, wR = rng.standard_normal((192, 4)), rng.standard_normal((1, 4)), rng.standard_normal((1, 4))
    assert rel(stream_spec(x, wL, wR, 64), O.binauralDecode(x, wL, wR)) <= 1e-12


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


def test_header_and_binding_agree(lib):
    import os
    import re
    from emagls_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "emagls.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(emagls_[a-z0-9_]+)\s*\(", hdr))
    assert set(NEW) <= declared and declared == set(L.SYMBOLS)


def create(lib, nch, ln=8, block=64, layout=0, basis=0, in_c=0):
    w = np.zeros((ln, nch), order="F")
    h = C.c_void_p()
    rc = lib.emagls_decode_stream_create(nch, w.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), 0, ln, in_c, layout, basis, block,
                                         C.byref(h))
    return rc, h


def push(lib, h, nch, nsamp, ny=0, npi=0, nr=0):
    x, out = np.zeros((max(nsamp, 1), nch), order="F"), np.zeros((max(nsamp, 1), 2), order="F")
    ang = np.full(max(nsamp, 4), 0.25)
    pa = ang.ctypes.data_as(C.c_void_p)
    return lib.emagls_decode_stream_push(h, x.ctypes.data_as(C.c_void_p), nsamp, pa if ny else None, ny, pa if npi else None, npi,
                                         pa if nr else None, nr, out.ctypes.data_as(C.c_void_p))


def test_entry_point_argument_errors(lib):
    """Every check runs before the device is touched: with or without a GPU."""
    from emagls_amd import _lib as L
    for block in (48, 32, 4096):
        rc, h = create(lib, 16, block=block)
        assert rc == L.ERR_UNSUPPORTED and not h.value, block
        assert b"block size" in lib.emagls_last_error()
    assert create(lib, 0)[0] == L.ERR_ARG
    assert create(lib, 16, ln=16385)[0] == L.ERR_UNSUPPORTED
    assert create(lib, 16, basis=5)[0] == L.ERR_ARG
    assert create(lib, 16, layout=2)[0] == L.ERR_ARG
    # null handle
    assert push(lib, None, 16, 64) == L.ERR_ARG
    assert lib.emagls_decode_stream_reset(None) == L.ERR_ARG
    assert lib.emagls_decode_stream_info(None, None, None, None, None, None) == L.ERR_ARG
    rc, h = create(lib, 16, ln=200)
    assert rc == L.OK and h.value
    try:
        b, p, sb, fb, nl = L.c_i64(0), L.c_i64(0), L.c_i64(0), L.c_i64(0), C.c_int(0)
        assert lib.emagls_decode_stream_info(h, C.byref(b), C.byref(p), C.byref(sb), C.byref(fb), C.byref(nl)) == L.OK
        assert (b.value, p.value, nl.value) == (64, 4, 3)
        assert sb.value == 16 * 2 * 4 * 65 + 8 * 16 * 64 + 4 and fb.value == 16 * 2 * 4 * 16 * 65
        assert push(lib, h, 16, 100) == L.ERR_ARG                 # not a multiple of the block
        assert push(lib, h, 16, -64) == L.ERR_ARG
        for counts in ((3, 0, 0), (1, 5, 0), (1, 1, 127), (-1, 0, 0), (0, 2, 0)):   # angle counts outside {0, 1, nsamp}
            assert push(lib, h, 16, 128, *counts) == L.ERR_ARG, counts
    finally:
        assert lib.emagls_decode_stream_destroy(h) == L.OK
    rc, h = create(lib, 15)                                       # fits no SH order
    assert rc == L.OK
    assert push(lib, h, 15, 64, 1, 0, 0) == L.ERR_ARG             # ... while an angle is given
    assert push(lib, h, 15, 64, 0, 1, 0) == L.ERR_ARG
    lib.emagls_decode_stream_destroy(h)
    rc, h = create(lib, 7, layout=1)                              # CH: yaw only
    assert push(lib, h, 7, 64, 1, 1, 0) == L.ERR_ARG
    assert b"CH signal" in lib.emagls_last_error()
    lib.emagls_decode_stream_destroy(h)
    rc, h = create(lib, 6, layout=1)                              # an even count is no CH layout
    assert push(lib, h, 6, 64, 1, 0, 0) == L.ERR_ARG
    lib.emagls_decode_stream_destroy(h)
    rc, h = create(lib, 17 * 17)                                  # order 16: yaw only
    assert rc == L.OK
    assert push(lib, h, 289, 64, 1, 1, 0) == L.ERR_UNSUPPORTED
    assert push(lib, h, 289, 64, 0, 0, 64) == L.ERR_UNSUPPORTED
    lib.emagls_decode_stream_destroy(h)
    assert lib.emagls_decode_stream_destroy(None) == L.OK


def test_python_argument_errors(lib):
    import emagls_amd as E
    w = np.zeros((8, 16))
    with pytest.raises(ValueError, match="shDefinition"):
        E.BinauralDecodeStream(w, w, 64, shDefinition="n3d")
    with pytest.raises(ValueError, match="rotation domain"):
        E.BinauralDecodeStream(w, w, 64, rotationDomain="xy")
    with pytest.raises(ValueError, match="equal shape"):
        E.BinauralDecodeStream(w, np.zeros((8, 9)), 64)
    with pytest.raises(E._lib.EmaglsError, match="block size"):
        E.BinauralDecodeStream(w, w, 48)
    with E.BinauralDecodeStream(w, w, 64) as s:
        assert s.info["block"] == 64 and s.info["partitions"] == 1 and s.info["launches_per_block"] <= 3
        with pytest.raises(ValueError, match="multiple of blockSize"):
            s.push(np.zeros((100, 16)))
        with pytest.raises(ValueError, match="channel count"):
            s.push(np.zeros((64, 9)))
        with pytest.raises(ValueError, match="horRotAngleRad must be a scalar or have one angle per input sample"):
            s.push(np.zeros((64, 16)), np.zeros(3))
        with pytest.raises(ValueError, match="pitchRad"):
            s.push(np.zeros((64, 16)), 0.1, np.zeros(5))
        with pytest.raises(ValueError, match="rollRad"):
            s.push(np.zeros((64, 16)), 0.1, 0.2, np.zeros(65))
        with pytest.raises(ValueError, match="real blocks"):
            s.push(np.zeros((64, 16), dtype=complex))
    with pytest.raises(ValueError, match="closed"):
        s.push(np.zeros((64, 16)))
    wh = np.zeros((8, 7))
    with E.BinauralDecodeStream(wh, wh, 64, rotationDomain="ch") as s:
        with pytest.raises(ValueError, match="CH signal can only be turned about z"):
            s.push(np.zeros((64, 7)), 0.3, 0.2)
    w15 = np.zeros((8, 15))
    with E.BinauralDecodeStream(w15, w15, 64) as s:
        with pytest.raises(ValueError, match="SH channels"):
            s.push(np.zeros((64, 15)), 0.3, 0.0, 0.2)


def test_python_closed_and_host_tensor_texts(lib):
    import torch
    import emagls_amd as E
    w = np.zeros((8, 16))
    s = E.BinauralDecodeStream(w, w, 64)
    with pytest.raises(ValueError, match=r"^a torch block must be on the GPU \(pass a NumPy array for the host entry\)$"):
        s.push(torch.zeros(64, 16, dtype=torch.float64))
    with pytest.raises(ValueError, match="multiple of blockSize"):      # (the shape is looked at first)
        s.push(torch.zeros(100, 16, dtype=torch.float64))
    s.close()
    s.close()
    for call in (lambda: s.push(np.zeros((64, 16))), lambda: s.info, s.reset):
        with pytest.raises(ValueError, match="^the decode stream is closed$"):
            call()
