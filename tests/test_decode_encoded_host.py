"""The host side of the encoded decode stream and listener group (emagls_decode_stream_create_encoded,
emagls_decode_group_create_encoded), through ctypes and without a device: the new entries in the header, the
binding and the library, every argument rule reported before the device is touched, and `info` on an object that has no device.
The two arrayEncoder checks against the oracle sit here with the encoder's other rules, but carry the gpu mark: arrayEncoder is
formed from the library's own getSH / getCH, which are device code."""
import ctypes as C

import numpy as np
import pytest

NEW = ["emagls_decode_stream_create_encoded", "emagls_decode_group_create_encoded"]
SH, CH, REAL = 0, 1, 0
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from emagls_amd import build, _lib
    build.build(jobs=4, verbose=False)
    return _lib.load()


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def create(lib, M=6, nch=4, n_sets=1, ln=8, block=64, layout=SH, enc="zeros", enc_c=0, listeners=None):
    w = np.zeros((max(n_sets, 1) * ln * max(nch, 1),))
    e = np.zeros((max(M, 1) * max(nch, 1) * 2,)) if isinstance(enc, str) else enc
    h = C.c_void_p()
    if listeners is None:
        rc = lib.emagls_decode_stream_create_encoded(M, vp(e), enc_c, nch, n_sets, vp(w), vp(w), 0, ln, layout, REAL, block, C.byref(h))
    else:
        rc = lib.emagls_decode_group_create_encoded(M, vp(e), enc_c, nch, n_sets, vp(w), vp(w), 0, ln, layout, REAL, block, listeners, C.byref(h))
    return rc, h


def destroy(lib, h, group):
    from emagls_amd import _lib as L
    assert (lib.emagls_decode_group_destroy if group else lib.emagls_decode_stream_destroy)(h) == L.OK


def test_new_symbols_are_exported_and_declared(lib):
    import os
    import re
    from emagls_amd import _lib as L
    raw = C.CDLL(L.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "emagls.h")).read(), flags=re.S)
    declared = {m.group(1): m.group(2) for m in re.finditer(r"\b(emagls_[a-z0-9_]+)\s*\(([^)]*)\)", hdr)}
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in L.SYMBOLS and name in declared
        assert len(L.SYMBOLS[name][1]) == declared[name].count(",") + 1, name     # as many arguments bound as declared


@pytest.mark.parametrize("listeners", [None, 3])
@pytest.mark.parametrize("M,nch", [(0, 4), (65, 4), (6, 0), (6, 65), (-1, 4)])
def test_counts_outside_1_to_64_are_unsupported(lib, M, nch, listeners):
    from emagls_amd import _lib as L
    rc, h = create(lib, M=M, nch=nch, listeners=listeners)
    assert rc == L.ERR_UNSUPPORTED and not h.value
    assert b"64" in lib.emagls_last_error()


@pytest.mark.parametrize("listeners", [None, 3])
def test_both_caps_and_more_channels_than_microphones_are_accepted(lib, listeners):
    from emagls_amd import _lib as L
    for M, nch in ((64, 64), (1, 1), (3, 9)):
        rc, h = create(lib, M=M, nch=nch, listeners=listeners)
        assert rc == L.OK and h.value, (M, nch)
        destroy(lib, h, listeners)


@pytest.mark.parametrize("listeners", [None, 3])
def test_null_encoder(lib, listeners):
    from emagls_amd import _lib as L
    rc, h = create(lib, enc=None, listeners=listeners)
    assert rc == L.ERR_ARG and not h.value
    assert b"null" in lib.emagls_last_error()


def test_the_stream_s_own_limits_still_hold(lib):
    from emagls_amd import _lib as L
    assert create(lib, block=96)[0] == L.ERR_UNSUPPORTED
    assert create(lib, nch=1, ln=16385)[0] == L.ERR_UNSUPPORTED
    assert create(lib, n_sets=0)[0] == L.ERR_ARG
    assert create(lib, listeners=0)[0] == L.ERR_ARG
    assert create(lib, listeners=4097)[0] == L.ERR_UNSUPPORTED


def test_pitch_on_a_ch_layout(lib):
    from emagls_amd import _lib as L
    x, out, pitch = np.zeros((64, 8), order="F"), np.zeros((2, 2, 64)), np.array([0.1, 0.2])
    rc, h = create(lib, M=8, nch=5, layout=CH)
    assert rc == L.OK
    try:
        assert lib.emagls_decode_stream_push(h, vp(x), 64, None, 0, vp(pitch), 1, None, 0, vp(out)) == L.ERR_ARG
        assert b"CH signal" in lib.emagls_last_error()
    finally:
        destroy(lib, h, False)
    rc, g = create(lib, M=8, nch=5, layout=CH, listeners=2)
    assert rc == L.OK
    try:
        assert lib.emagls_decode_group_push(g, vp(x), 64, None, 0, None, 0, vp(pitch), 2, None, 0, vp(out)) == L.ERR_ARG
        assert b"CH signal" in lib.emagls_last_error()
    finally:
        destroy(lib, g, True)


def test_pitch_needs_an_sh_channel_count_of_the_filters_not_of_the_microphones(lib):
    """9 microphones and 5 channels: 9 = (2+1)^2 would fit, but the rotation turns the 5 encoded channels."""
    from emagls_amd import _lib as L
    x, out, pitch = np.zeros((64, 9), order="F"), np.zeros((2, 64)), np.array([0.1])
    rc, h = create(lib, M=9, nch=5)
    assert rc == L.OK
    try:
        assert lib.emagls_decode_stream_push(h, vp(x), 64, None, 0, vp(pitch), 1, None, 0, vp(out)) == L.ERR_ARG
        assert lib.emagls_decode_stream_push(h, vp(x), 100, None, 0, None, 0, None, 0, vp(out)) == L.ERR_ARG
        assert b"multiple of the block" in lib.emagls_last_error()
    finally:
        destroy(lib, h, False)


def test_info_counts_the_encoder_in_filter_bytes(lib):
    """On an object without a device: three launches per block, the plain stream's state, the spectra plus enc."""
    from emagls_amd import _lib as L
    for enc_c in (0, 1):
        rc, h = create(lib, M=6, nch=4, n_sets=3, ln=200, enc_c=enc_c)
        assert rc == L.OK
        b, p, sb, fb, k = L.c_i64(0), L.c_i64(0), L.c_i64(0), L.c_i64(0), C.c_int(0)
        assert lib.emagls_decode_stream_info(h, C.byref(b), C.byref(p), C.byref(sb), C.byref(fb), C.byref(k)) == L.OK
        planes = 8 if enc_c else 4                      # a complex encoder: 2C planes, as a complexInput stream
        assert (b.value, p.value, k.value) == (64, 4, 3)
        assert fb.value == 3 * 16 * 2 * 4 * planes * 65 + (16 if enc_c else 8) * 4 * 6
        assert sb.value == 16 * 2 * 4 * 65 + (16 if enc_c else 8) * 4 * 64 + 4 + 2 * 4
        destroy(lib, h, False)
    got = {}
    for nl in (1, 7):
        rc, g = create(lib, M=6, nch=4, n_sets=3, ln=200, listeners=nl)
        assert rc == L.OK
        b, p, n, sb, fb, k = L.c_i64(0), L.c_i64(0), L.c_i64(0), L.c_i64(0), L.c_i64(0), C.c_int(0)
        assert lib.emagls_decode_group_info(g, C.byref(b), C.byref(p), C.byref(n), C.byref(sb), C.byref(fb), C.byref(k)) == L.OK
        got[nl] = (n.value, sb.value, fb.value, k.value)
        destroy(lib, g, True)
    assert got[1][2] == got[7][2] == 3 * 16 * 2 * 4 * 4 * 65 + 8 * 4 * 6
    assert got[7][1] == 7 * got[1][1] and got[1][3] == got[7][3] == 3 and got[7][0] == 7


def test_python_argument_errors(lib):
    import emagls_amd as E
    L = E._lib
    w, enc = np.zeros((8, 4)), np.zeros((4, 6))
    with pytest.raises(ValueError, match="numChannels x numMics"):
        E.BinauralDecodeStream(w, w, 64, encoder=np.zeros((6, 4)))
    with pytest.raises(ValueError, match="complexInput"):
        E.BinauralDecodeStream(w, w, 64, complexInput=True, encoder=enc)
    with pytest.raises(L.EmaglsError) as ei:
        E.BinauralDecodeStream(np.zeros((8, 65)), np.zeros((8, 65)), 64, encoder=np.zeros((65, 6)))
    assert ei.value.code == L.ERR_UNSUPPORTED
    with pytest.raises(L.EmaglsError) as ei:
        E.BinauralDecodeGroup(w, w, 64, 2, encoder=np.zeros((4, 65)))
    assert ei.value.code == L.ERR_UNSUPPORTED
    for make in (lambda: E.BinauralDecodeStream(w, w, 64, encoder=enc), lambda: E.BinauralDecodeGroup(w, w, 64, 2, encoder=enc)):
        with make() as s:
            assert s.numChannels == 4 and s.numMics == 6
            info = s.info if isinstance(s, E.BinauralDecodeStream) else s.info()
            assert info["launches_per_block"] == 3
            with pytest.raises(L.EmaglsError) as ei:            # a complex block
                s.push(np.zeros((64, 6), dtype=complex))
            assert ei.value.code == L.ERR_ARG
            with pytest.raises(ValueError, match="numMics"):     # numChannels columns instead of numMics
                s.push(np.zeros((64, 4)))
            with pytest.raises(ValueError, match="multiple of blockSize"):
                s.push(np.zeros((100, 6)))
    with E.BinauralDecodeStream(np.zeros((8, 5)), np.zeros((8, 5)), 64, rotationDomain="ch", encoder=np.zeros((5, 8))) as s:
        with pytest.raises(ValueError, match="CH signal"):
            s.push(np.zeros((64, 8)), pitchRad=0.1)
    with E.BinauralDecodeStream(w, w, 64) as s:                  # a plain stream is what it was
        assert s.numMics is None and s.numChannels == 4
        with pytest.raises(ValueError, match="numChannels"):
            s.push(np.zeros((64, 6)))


# ---- arrayEncoder against the oracle (device code behind getSH / getCH)
def mic_grid(M, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 2 * np.pi, M), np.arccos(rng.uniform(-1, 1, M))


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@gpu
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_array_encoder_sma_is_what_encode_sh_applies(basis):
    import emagls_amd as E
    from oracle import emagls_oracle as O
    azi, zen = mic_grid(32, 1)
    x = np.random.default_rng(2).standard_normal((200, 32))
    enc = E.arrayEncoder("sma", 4, azi, zen, basis)
    assert enc.shape == (25, 32) and np.iscomplexobj(enc) == (basis == "complex")
    err = rel(x @ enc.T, O.encodeSH(x, azi, zen, 4, basis))
    print("arrayEncoder sma", basis, "%.2e" % err)
    assert err <= 1e-13
    assert rel(x @ enc.T, E.encodeSH(x, azi, zen, 4, basis)) <= 1e-13


@gpu
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_array_encoder_ema(basis):
    import emagls_amd as E
    from oracle import emagls_oracle as O
    azi = mic_grid(16, 3)[0]
    ch = np.linalg.pinv(O.getCH(5, azi, basis).T).T
    got = E.arrayEncoder("ema_ch", 5, azi, shDefinition=basis)
    assert got.shape == (11, 16)
    err_ch = rel(got, ch)
    got = E.arrayEncoder("ema_sh", 5, azi, shDefinition=basis)
    assert got.shape == (36, 16)
    err_sh = rel(got, O.getChToShExpansionMatrix(5, basis) @ ch)
    print("arrayEncoder ema_ch %.2e ema_sh %.2e" % (err_ch, err_sh), basis)
    assert err_ch <= 1e-13 and err_sh <= 1e-13
    with pytest.raises(ValueError, match="kind"):
        E.arrayEncoder("ema", 5, azi)
