"""The host side of the listener group (emagls_decode_group_*), through ctypes and without a device: every
argument rule of the new entries, reported before the device is touched, and what `info` says of an object that has no device."""
import ctypes as C

import numpy as np
import pytest

NEW = ["emagls_decode_group_create", "emagls_decode_group_push", "emagls_decode_group_push_device", "emagls_decode_group_reset",
       "emagls_decode_group_info", "emagls_decode_group_destroy"]
SH, CH, REAL = 0, 1, 0


@pytest.fixture(scope="module")
def lib():
    from emagls_amd import build, _lib
    build.build(jobs=4, verbose=False)
    return _lib.load()


def create(lib, L, nch=4, n_sets=1, ln=8, block=64, layout=SH):
    w = np.zeros((max(n_sets, 1) * ln * nch,))
    h = C.c_void_p()
    rc = lib.emagls_decode_group_create(nch, n_sets, w.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), 0, ln, 0, layout, REAL, block,
                                        L, C.byref(h))
    return rc, h


def push(lib, h, nch, L, nsamp, sets=None, n_set=None, yaw=None, n_yaw=None, pitch=None, n_pitch=None):
    x, out = np.zeros((max(nsamp, 1), nch), order="F"), np.zeros((L, 2, max(nsamp, 1)))
    s = None if sets is None else np.ascontiguousarray(sets, dtype=np.int32)
    y = None if yaw is None else np.ascontiguousarray(yaw, dtype=np.float64)
    q = None if pitch is None else np.ascontiguousarray(pitch, dtype=np.float64)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    cnt = lambda a, n: (0 if a is None else a.size) if n is None else n   # noqa: E731
    return lib.emagls_decode_group_push(h, vp(x), nsamp, vp(s), cnt(s, n_set), vp(y), cnt(y, n_yaw), vp(q), cnt(q, n_pitch), None, 0, vp(out))


def info(lib, h):
    from emagls_amd import _lib as L
    b, p, nl, sb, fb, k = L.c_i64(0), L.c_i64(0), L.c_i64(0), L.c_i64(0), L.c_i64(0), C.c_int(0)
    assert lib.emagls_decode_group_info(h, C.byref(b), C.byref(p), C.byref(nl), C.byref(sb), C.byref(fb), C.byref(k)) == L.OK
    return dict(block=b.value, partitions=p.value, listeners=nl.value, state_bytes=sb.value, filter_bytes=fb.value, launches=k.value)


@pytest.fixture()
def group(lib):
    """3 listeners of a bank of 2 sets, 4 SH channels, blocks of 64."""
    from emagls_amd import _lib as L
    rc, h = create(lib, 3, n_sets=2, ln=100)
    assert rc == L.OK and h.value
    yield h
    assert lib.emagls_decode_group_destroy(h) == L.OK


def test_new_symbols_are_exported_and_declared(lib):
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


def test_no_listener_is_an_argument_error(lib):
    from emagls_amd import _lib as L
    rc, h = create(lib, 0)
    assert rc == L.ERR_ARG and not h.value
    assert b"listener" in lib.emagls_last_error()
    assert create(lib, -2)[0] == L.ERR_ARG


def test_more_than_4096_listeners_are_unsupported(lib):
    from emagls_amd import _lib as L
    rc, h = create(lib, 4097)
    assert rc == L.ERR_UNSUPPORTED and not h.value
    assert b"4096" in lib.emagls_last_error()


def test_block_size_96_is_unsupported(lib):
    from emagls_amd import _lib as L
    assert create(lib, 3, block=96)[0] == L.ERR_UNSUPPORTED


def test_filters_of_16385_taps_are_unsupported(lib):
    from emagls_amd import _lib as L
    assert create(lib, 3, nch=1, ln=16385)[0] == L.ERR_UNSUPPORTED


def test_angle_count_of_listeners_plus_one(lib, group):
    from emagls_amd import _lib as L
    assert push(lib, group, 4, 3, 128, yaw=np.zeros(4)) == L.ERR_ARG
    assert b"angle" in lib.emagls_last_error()
    assert push(lib, group, 4, 3, 128, yaw=np.zeros(3 * 128 + 1)) == L.ERR_ARG
    assert push(lib, group, 4, 3, 128, yaw=np.zeros(128)) == L.ERR_ARG        # one listener's worth is not a count of a group


def test_set_count_of_listeners_times_blocks_plus_one(lib, group):
    from emagls_amd import _lib as L
    assert push(lib, group, 4, 3, 128, sets=np.zeros(3 * 2 + 1)) == L.ERR_ARG
    assert b"set ind" in lib.emagls_last_error()
    assert push(lib, group, 4, 3, 128, sets=np.zeros(2)) == L.ERR_ARG


def test_index_equal_to_the_number_of_sets(lib, group):
    from emagls_amd import _lib as L
    assert push(lib, group, 4, 3, 128, sets=[0, 2, 1]) == L.ERR_ARG
    assert b"set index" in lib.emagls_last_error()
    assert push(lib, group, 4, 3, 128, sets=[0, 1, 0, 1, 0, -1]) == L.ERR_ARG


def test_null_array_with_a_positive_count(lib, group):
    from emagls_amd import _lib as L
    assert push(lib, group, 4, 3, 128, n_yaw=3) == L.ERR_ARG
    assert push(lib, group, 4, 3, 128, n_set=3) == L.ERR_ARG
    assert push(lib, group, 4, 3, 128, n_pitch=3 * 128) == L.ERR_ARG


def test_samples_that_are_no_multiple_of_the_block(lib, group):
    from emagls_amd import _lib as L
    assert push(lib, group, 4, 3, 100) == L.ERR_ARG
    assert b"multiple of the block" in lib.emagls_last_error()
    assert push(lib, group, 4, 3, 0) == L.OK                                   # nothing to do is no error


def test_pitch_on_a_ch_layout(lib):
    from emagls_amd import _lib as L
    rc, h = create(lib, 2, nch=5, layout=CH)
    assert rc == L.OK
    try:
        assert push(lib, h, 5, 2, 64, pitch=[0.1, 0.2]) == L.ERR_ARG
        assert b"CH signal" in lib.emagls_last_error()
    finally:
        lib.emagls_decode_group_destroy(h)


def test_reset_of_a_listener_outside_the_group(lib, group):
    from emagls_amd import _lib as L
    for bad in (-2, 3, 4096):
        assert lib.emagls_decode_group_reset(group, bad) == L.ERR_ARG, bad
        assert b"listener" in lib.emagls_last_error()
    assert lib.emagls_decode_group_reset(None, 0) == L.ERR_ARG


def test_null_group(lib):
    from emagls_amd import _lib as L
    assert push(lib, None, 4, 3, 64) == L.ERR_ARG
    assert lib.emagls_decode_group_info(None, None, None, None, None, None, None) == L.ERR_ARG
    assert lib.emagls_decode_group_destroy(None) == L.OK


def test_info_filters_once_state_per_listener(lib):
    """filter_bytes does not depend on the listeners; state_bytes is proportional to them."""
    from emagls_amd import _lib as L
    got = {}
    for nl in (1, 7):
        rc, h = create(lib, nl, n_sets=3, ln=200)
        assert rc == L.OK
        got[nl] = info(lib, h)
        lib.emagls_decode_group_destroy(h)
    one, seven = got[1], got[7]
    assert (one["block"], one["partitions"], one["listeners"], one["launches"]) == (64, 4, 1, 3)
    assert (seven["block"], seven["partitions"], seven["listeners"], seven["launches"]) == (64, 4, 7, 3)
    assert one["filter_bytes"] == seven["filter_bytes"] == 3 * 16 * 2 * 4 * 4 * 65
    assert one["state_bytes"] == 16 * 2 * 4 * 65 + 8 * 4 * 64 + 4 + 2 * 4       # a bank stream's: ring, overlap, position, two indices
    assert seven["state_bytes"] == 7 * one["state_bytes"]


def test_python_argument_errors(lib):
    import emagls_amd as E
    w = np.zeros((2, 8, 4))
    with pytest.raises(E._lib.EmaglsError):
        E.BinauralDecodeGroup(w, w, 64, 0)
    with pytest.raises(ValueError, match="equal shape"):
        E.BinauralDecodeGroup(w, w[:1], 64, 2)
    with E.BinauralDecodeGroup(w, w, 64, 3) as g:
        assert g.numListeners == 3 and g.numSets == 2 and g.info()["listeners"] == 3
        x = np.zeros((128, 4))
        with pytest.raises(ValueError, match="numListeners"):
            g.push(x, horRotAngleRad=np.zeros(4))
        with pytest.raises(ValueError, match="numListeners"):
            g.push(x, setIndex=np.zeros((3, 3), dtype=int))
        with pytest.raises(ValueError, match="numSets - 1"):
            g.push(x, setIndex=2)
        with pytest.raises(ValueError, match="multiple of blockSize"):
            g.push(np.zeros((100, 4)))


def test_python_closed_and_host_tensor_texts(lib):
    import torch
    import emagls_amd as E
    w = np.zeros((8, 4))
    g = E.BinauralDecodeGroup(w, w, 64, 2)
    with pytest.raises(ValueError, match=r"^a torch block must be on the GPU \(pass a NumPy array for the host entry\)$"):
        g.push(torch.zeros(64, 4, dtype=torch.float64))
    g.close()
    g.close()
    for call in (lambda: g.push(np.zeros((64, 4))), g.info, g.reset):
        with pytest.raises(ValueError, match="^the decode group is closed$"):
            call()
