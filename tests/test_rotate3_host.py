"""CPU-side checks of the three-axis rotation: the built library exports its entry points, they fail loudly without a GPU (no CPU
fallback), and the Python layer rejects bad arguments before it calls the library."""
import ctypes as C

import numpy as np
import pytest

NEW = ["emagls_sh_rotation_matrix", "emagls_rotate_sh", "emagls_binaural_decode_render_ypr", "emagls_binaural_decode_render_ypr_device"]


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


@pytest.fixture
def no_library(monkeypatch):
    """Any call into the library fails the test: the argument checks must come first."""
    from emagls_amd import _lib as L

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(L, "load", boom)


def test_rotate_sh_argument_errors(no_library):
    import emagls_amd as E
    x = np.zeros((10, 16))
    with pytest.raises(ValueError, match="pitchRad"):
        E.rotateSH(x, 0.1, np.zeros(3), 0.0)
    with pytest.raises(ValueError, match="yawRad"):
        E.rotateSH(x, np.zeros(9), 0.0, 0.0)
    with pytest.raises(ValueError, match="rollRad"):
        E.rotateSH(x, 0.0, 0.0, np.zeros(11))
    with pytest.raises(ValueError, match="SH channels"):
        E.rotateSH(np.zeros((10, 15)), 0.1, 0.2, 0.3)
    with pytest.raises(ValueError, match="numSamples x numChannels"):
        E.rotateSH(np.zeros(16), 0.1, 0.2, 0.3)
    with pytest.raises(ValueError, match="shDefinition"):
        E.rotateSH(x, 0.1, 0.2, 0.3, "n3d")
    with pytest.raises(ValueError, match="order"):
        E.shRotationMatrix(-1, 0.1, 0.2, 0.3)


def test_binaural_decode_argument_errors(no_library):
    import emagls_amd as E
    x, w = np.zeros((10, 16)), np.zeros((8, 16))
    with pytest.raises(ValueError, match="pitchRad"):
        E.binauralDecode(x, 48000, w, w, 48000, pitchRad=np.ones(4))
    with pytest.raises(ValueError, match="rollRad"):
        E.binauralDecode(x, 48000, w, w, 48000, pitchRad=0.1, rollRad=np.ones(9))
    xh, wh = np.zeros((10, 7)), np.zeros((8, 7))
    with pytest.raises(ValueError, match="CH signal can only be turned about z"):
        E.binauralDecode(xh, 48000, wh, wh, 48000, horRotAngleRad=0.3, rotationDomain="ch", pitchRad=0.2)
    with pytest.raises(ValueError, match="SH channels"):
        E.binauralDecode(np.zeros((10, 15)), 48000, np.zeros((8, 15)), np.zeros((8, 15)), 48000, rollRad=0.2)


def test_entry_point_argument_errors(lib):
    """The checks that need no device come first, with or without a GPU."""
    from emagls_amd import _lib as L
    out = np.zeros(16 * 16)
    assert lib.emagls_sh_rotation_matrix(16, 0, 0.1, 0.2, 0.3, out.ctypes.data_as(C.c_void_p)) == L.ERR_UNSUPPORTED
    assert lib.emagls_sh_rotation_matrix(3, 5, 0.1, 0.2, 0.3, out.ctypes.data_as(C.c_void_p)) == L.ERR_ARG
    x = np.zeros((4, 16))
    a = np.array([0.1])
    pa = a.ctypes.data_as(C.c_void_p)
    y = np.zeros((4, 16))
    po = y.ctypes.data_as(C.c_void_p)
    assert lib.emagls_rotate_sh(x.ctypes.data_as(C.c_void_p), 0, 4, 15, 0, pa, 1, pa, 1, pa, 1, po) == L.ERR_ARG
    assert lib.emagls_rotate_sh(x.ctypes.data_as(C.c_void_p), 0, 4, 16, 0, pa, 1, pa, 3, pa, 1, po) == L.ERR_ARG
    big = np.zeros((2, 17 * 17))
    big_out = np.zeros_like(big)
    assert lib.emagls_rotate_sh(big.ctypes.data_as(C.c_void_p), 0, 2, 17 * 17, 0, pa, 1, pa, 1, pa, 1,
                                big_out.ctypes.data_as(C.c_void_p)) == L.ERR_UNSUPPORTED
