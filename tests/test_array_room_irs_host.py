"""The host side of the shoebox entries (emagls_shoebox_components, emagls_array_room_irs,
emagls_shoebox_kernel_time), through ctypes and without a device: the header, the binding and the built library agree on the three
entries, every argument rule is reported before the device is touched with its code and message, and valid arguments without a
GPU fail on the device (there is no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOM_ARGS = ["room_dim", "wall_refl", "array_pos", "nsrc", "src_pos"]
ARGS = {
    "emagls_shoebox_components": ROOM_ARGS + ["fs", "max_delay", "max_order", "capacity", "comp_ptr", "comp_azi", "comp_zen", "comp_delay",
                                              "comp_gain"],
    "emagls_array_room_irs": ["fs", "mic_radius", "order", "mic_azi", "mic_zen", "nmics", "enc", "enc_is_complex", "nch"] + ROOM_ARGS +
                             ["max_delay", "max_order", "pre_delay", "nfft", "nr", "comp_count", "out"],
    "emagls_shoebox_kernel_time": ["ms"],
}


@pytest.fixture(scope="module")
def lib():
    from emagls_amd import build, _lib
    build.build(jobs=4, verbose=False)
    return _lib.load()


def room(nsrc=2, **over):
    """Room A of the tests on the GPU, the source twice; arrays of the right sizes for both entries."""
    a = dict(room_dim=np.array([3.1, 2.3, 2.7]), wall_refl=np.array([0.9, 0.85, 0.8, 0.75, 0.7, 0.6]), array_pos=np.array([2.02, 1.41, 1.17]),
             nsrc=nsrc, src_pos=np.tile([1.13, 0.71, 1.52], nsrc), fs=16000.0, max_delay=100.0, max_order=-1)
    a.update(over)
    return a


def components(cap=64, **over):
    return dict(room(**over), capacity=cap, comp_ptr=np.full(over.get("nsrc", 2) + 1, -7, dtype=np.int64), comp_azi=np.zeros(max(cap, 1)),
                comp_zen=np.zeros(max(cap, 1)), comp_delay=np.zeros(max(cap, 1)), comp_gain=np.zeros(max(cap, 1)))


def responses(M=6, nfft=256, nr=120, **over):
    a = dict(room(**over), mic_radius=0.042, order=1, mic_azi=np.zeros(M), mic_zen=np.zeros(M), nmics=M, enc=None, enc_is_complex=0, nch=M,
             pre_delay=4.0, nfft=nfft, nr=nr, comp_count=np.zeros(over.get("nsrc", 2), dtype=np.int64))
    a["out"] = np.full(a["nsrc"] * M * nr, 7.0)
    return a


def call(lib, name, a):
    vals = [a[k].ctypes.data_as(C.c_void_p) if isinstance(a[k], np.ndarray) else a[k] for k in ARGS[name]]
    return getattr(lib, name)(*vals)


def expect(lib, a, code, word, names=("emagls_shoebox_components", "emagls_array_room_irs")):
    """The rule holds in both entries (a: the room's arguments to change, over the valid sets)."""
    for name in names:
        full = dict(components() if name == "emagls_shoebox_components" else responses(), **a)
        rc = call(lib, name, full)
        msg = lib.emagls_last_error()
        assert rc == code, (name, rc, msg)
        assert word in msg, (name, msg)
        if full.get("out") is not None:
            assert np.all(full["out"] == 7.0)


def test_header_binding_and_library_agree(lib):
    from emagls_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "emagls.h")).read(), flags=re.S)

    def ctype(p):
        if p.split()[-1] == "ms":
            return C.POINTER(C.c_double)
        if "*" in p:
            return C.c_void_p
        return {"int": C.c_int, "int64_t": L.c_i64, "double": C.c_double}[p.split()[0]]

    for name, args in ARGS.items():
        assert hasattr(C.CDLL(L.LIB_PATH), name) and name in L.SYMBOLS, name
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S)
        assert m, name + " is not declared"
        params = [p.strip() for p in m.group(1).split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == args
        res, argtypes = L.SYMBOLS[name]
        assert res is C.c_int and argtypes == [ctype(p) for p in params], name


def test_python_exports():
    import emagls_amd as E
    assert callable(E.getShoeboxComponents) and callable(E.getArrayRoomIrs)
    assert {"getShoeboxComponents", "getArrayRoomIrs"} <= set(E.__all__)


def test_a_valid_call_gets_as_far_as_the_device(lib):
    """The argument sets the tests below spoil are valid: without a device the calls fail on the device, loudly, not on an argument
    and not by computing on the CPU."""
    from emagls_amd import _lib as L
    n = C.c_int(0)
    if lib.emagls_device_count(C.byref(n)) == L.OK and n.value > 0:
        return      # (with a device the call would run; the rule is about machines without one)
    for a in (components(), components(cap=0), dict(components(), max_order=0), components(nsrc=1)):
        assert call(lib, "emagls_shoebox_components", a) == L.ERR_HIP
        assert lib.emagls_last_error() and np.all(a["comp_ptr"] == -7)
    count_only = dict(components(cap=0), comp_azi=None, comp_zen=None, comp_delay=None, comp_gain=None)
    assert call(lib, "emagls_shoebox_components", count_only) == L.ERR_HIP
    for a in (responses(), dict(responses(), comp_count=None), dict(responses(), nfft=0), dict(responses(), max_delay=251.0),
              dict(responses(), max_order=3)):
        assert call(lib, "emagls_array_room_irs", a) == L.ERR_HIP
        assert lib.emagls_last_error() and np.all(a["out"] == 7.0)


@pytest.mark.parametrize("name", ROOM_ARGS[:3] + ["src_pos"])
def test_null_pointers_of_the_room(lib, name):
    from emagls_amd import _lib as L
    expect(lib, {name: None}, L.ERR_ARG, b"null pointer")


def test_null_pointers_of_the_results(lib):
    from emagls_amd import _lib as L
    expect(lib, dict(comp_ptr=None), L.ERR_ARG, b"null pointer: comp_ptr", names=["emagls_shoebox_components"])
    expect(lib, dict(comp_gain=None), L.ERR_ARG, b"null pointer: component arrays", names=["emagls_shoebox_components"])
    expect(lib, dict(capacity=-1), L.ERR_ARG, b"capacity", names=["emagls_shoebox_components"])
    expect(lib, dict(out=None), L.ERR_ARG, b"null pointer: out", names=["emagls_array_room_irs"])
    expect(lib, dict(mic_azi=None), L.ERR_ARG, b"null pointer: microphone grid", names=["emagls_array_room_irs"])


def test_nsrc_fs_and_the_room(lib):
    from emagls_amd import _lib as L
    expect(lib, dict(nsrc=0), L.ERR_ARG, b"nsrc")
    expect(lib, dict(fs=0.0), L.ERR_ARG, b"must be positive")
    expect(lib, dict(fs=np.inf), L.ERR_ARG, b"must be positive")
    for bad in (0.0, -2.3, np.nan, np.inf):
        expect(lib, dict(room_dim=np.array([3.1, bad, 2.7])), L.ERR_ARG, b"room_dim must be positive and finite")


@pytest.mark.parametrize("bad", [1.0000001, -1.5, np.nan, np.inf])
def test_reflection_coefficients_outside_minus_one_to_one(lib, bad):
    from emagls_amd import _lib as L
    for i in range(6):
        w = np.array([0.9, 0.85, 0.8, 0.75, 0.7, 0.6])
        w[i] = bad
        expect(lib, dict(wall_refl=w), L.ERR_ARG, b"[-1, 1]")


def test_the_ends_of_the_coefficient_range_are_valid(lib):
    from emagls_amd import _lib as L
    n = C.c_int(0)
    if lib.emagls_device_count(C.byref(n)) == L.OK and n.value > 0:
        return
    a = components()
    a["wall_refl"] = np.array([1.0, -1.0, 0.0, 1.0, -1.0, 0.0])
    assert call(lib, "emagls_shoebox_components", a) == L.ERR_HIP


def test_a_source_outside_the_room(lib):
    from emagls_amd import _lib as L
    for axis, bad in [(0, 0.0), (0, 3.1), (1, -0.2), (1, 2.4), (2, 2.7), (2, np.nan), (0, np.inf)]:
        s = np.tile([1.13, 0.71, 1.52], 2)
        s[3 + axis] = bad
        expect(lib, dict(src_pos=s), L.ERR_ARG, b"source 1 does not lie strictly inside the room")


def test_a_source_inside_the_sphere(lib):
    from emagls_amd import _lib as L
    s = np.array([1.13, 0.71, 1.52, 2.02 + 0.03, 1.41, 1.17 - 0.02])       # 3.6 cm from the centre of a 4.2 cm sphere
    expect(lib, dict(src_pos=s), L.ERR_ARG, b"source 1 lies inside the array's sphere", names=["emagls_array_room_irs"])
    s[3:] = [2.02, 1.41, 1.17]                                                 # the lists have no sphere, but a direction needs a distance
    expect(lib, dict(src_pos=s), L.ERR_ARG, b"source 1 lies inside the array's sphere")


def test_the_sphere_through_a_wall(lib):
    from emagls_amd import _lib as L
    for axis, bad in [(0, 0.04), (0, 3.1 - 0.04), (1, 0.0), (2, 2.7 - 0.041), (2, np.nan)]:
        p = np.array([2.02, 1.41, 1.17])
        p[axis] = bad
        expect(lib, dict(array_pos=p), L.ERR_ARG, b"sphere must lie inside the room", names=["emagls_array_room_irs"])
    # the lists have no sphere: the centre on a wall is allowed, outside is not
    expect(lib, dict(array_pos=np.array([2.02, -0.01, 1.17])), L.ERR_ARG, b"must lie inside the room", names=["emagls_shoebox_components"])
    expect(lib, dict(array_pos=np.array([3.2, 1.41, 1.17])), L.ERR_ARG, b"must lie inside the room", names=["emagls_shoebox_components"])


@pytest.mark.parametrize("bad", [0.0, -5.0, np.nan, np.inf])
def test_max_delay(lib, bad):
    from emagls_amd import _lib as L
    expect(lib, dict(max_delay=float(bad)), L.ERR_ARG, b"max_delay must be positive and finite")


def test_max_order_below_minus_one(lib):
    from emagls_amd import _lib as L
    expect(lib, dict(max_order=-2), L.ERR_ARG, b"max_order")


def test_a_max_delay_that_would_wrap(lib):
    from emagls_amd import _lib as L
    one = ["emagls_array_room_irs"]
    expect(lib, dict(max_delay=251.5), L.ERR_ARG, b"would wrap", names=one)       # 251.5 + 4 > 255
    expect(lib, dict(max_delay=60.0, nfft=64, nr=30), L.ERR_ARG, b"would wrap", names=one)
    expect(lib, dict(max_delay=200.0, nfft=0, nr=60), L.ERR_ARG, b"would wrap", names=one)      # the default nfft: 128
    expect(lib, dict(pre_delay=300.0), L.ERR_ARG, b"would wrap", names=one)


def test_the_rules_shared_with_array_irs(lib):
    from emagls_amd import _lib as L
    one = ["emagls_array_room_irs"]
    expect(lib, dict(nfft=48), L.ERR_ARG, b"power of two", names=one)
    expect(lib, dict(nfft=131072), L.ERR_UNSUPPORTED, b"65536", names=one)
    expect(lib, dict(nr=300), L.ERR_ARG, b"nr exceeds nfft", names=one)
    expect(lib, dict(nch=4), L.ERR_ARG, b"nch must equal nmics", names=one)
    expect(lib, dict(mic_radius=0.0), L.ERR_ARG, b"must be positive", names=one)
    expect(lib, dict(order=86), L.ERR_UNSUPPORTED, b"simulation order", names=one)
    expect(lib, dict(pre_delay=-1.0), L.ERR_ARG, b"pre_delay", names=one)


def test_the_candidate_cap(lib):
    """2^28 candidates in a call.  Room A at fs = 16000: max_delay = 40000 samples reach 857.5 m, a box of 279 x 375 x 319 cells times
    8 parities: 2.67e8 candidates per source (just under 2.68e8), so two sources pass it; 1e9 samples pass it on their own."""
    from emagls_amd import _lib as L
    expect(lib, dict(max_delay=40000.0), L.ERR_UNSUPPORTED, b"2^28 image-source candidates", names=["emagls_shoebox_components"])
    expect(lib, dict(max_delay=1e9), L.ERR_UNSUPPORTED, b"2^28 image-source candidates", names=["emagls_shoebox_components"])
    expect(lib, dict(max_delay=1e300), L.ERR_UNSUPPORTED, b"2^28 image-source candidates", names=["emagls_shoebox_components"])
    expect(lib, dict(max_delay=40000.0, nfft=65536, nr=8), L.ERR_UNSUPPORTED, b"2^28 image-source candidates", names=["emagls_array_room_irs"])
    # an order limit bounds the box whatever the delay: order 200 is 201^3 x 8 = 6.5e7 candidates per source, five sources are 3.2e8 ...
    a = dict(max_delay=1e9, max_order=200)
    n = C.c_int(0)
    if not (lib.emagls_device_count(C.byref(n)) == L.OK and n.value > 0):
        assert call(lib, "emagls_shoebox_components", dict(components(), **a)) == L.ERR_HIP           # ... two are not
    five = components(nsrc=5)
    assert call(lib, "emagls_shoebox_components", dict(five, **a)) == L.ERR_UNSUPPORTED


def test_the_24_gib_estimate_before_the_count(lib):
    """The part of the estimate that does not need the component count is applied before the device is touched: 4096 source
    positions on 64 microphones at nfft = 65536 are 1.4e11 bytes of spectra."""
    from emagls_amd import _lib as L
    a = responses(M=64, nfft=65536, nr=8, nsrc=4096)
    assert call(lib, "emagls_array_room_irs", a) == L.ERR_UNSUPPORTED
    assert b"24 GiB" in lib.emagls_last_error()


def test_kernel_time_entry(lib):
    from emagls_amd import _lib as L
    assert lib.emagls_shoebox_kernel_time(None) == L.ERR_ARG and b"null pointer" in lib.emagls_last_error()
    ms = C.c_double(-1.0)
    rc = lib.emagls_shoebox_kernel_time(C.byref(ms))
    assert (rc == L.OK and ms.value >= 0.0) or (rc == L.ERR_ARG and b"no emagls_shoebox_components" in lib.emagls_last_error())


def test_python_shapes_the_arguments(lib, monkeypatch):
    """What the wrappers hand to the C calls (which are replaced: no device here): one position or one per row, maxOrder None as -1,
    the default maxDelay irLen - 1 - preDelay, two calls for the lists (count, then fill)."""
    import emagls_amd as E
    from emagls_amd import api
    seen = []

    def arr(p, n, t=C.c_double):
        return None if p is None else np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), shape=(n,))

    class Fake:
        def emagls_shoebox_components(self, dim, refl, pos, Q, src, fs, max_delay, max_order, cap, ptr, azi, zen, delay, gain):
            seen.append(("components", arr(dim, 3).copy(), arr(refl, 6).copy(), arr(pos, 3).copy(), Q, arr(src, 3 * Q).copy(), fs, max_delay,
                         max_order, cap, azi is None))
            arr(ptr, Q + 1, C.c_int64)[:] = [0, 2, 2, 3][:Q + 1]
            if cap:
                for k, p in enumerate((azi, zen, delay, gain)):
                    arr(p, cap)[:] = 10.0 * k + np.arange(cap)
            return 0

        def emagls_array_room_irs(self, *a):
            seen.append(("irs",) + tuple(a[:3]) + (a[5], a[7], a[8], arr(a[9], 3).copy(), a[12], arr(a[13], 3 * a[12]).copy()) + tuple(a[14:19]))
            arr(a[19], a[12], C.c_int64)[:] = 5
            return 0

    monkeypatch.setattr(api.L, "load", lambda: Fake())
    src = [[1.0, 1.1, 1.2], [0.5, 0.6, 0.7], [2.0, 2.1, 2.2]]
    out = E.getShoeboxComponents((3.1, 2.3, 2.7), [0.9] * 6, src, (2.0, 1.4, 1.2), 16000.0, 100.0)
    assert [s[0] for s in seen] == ["components", "components"] and seen[0][9] == 0 and seen[0][10] and seen[1][9] == 3 and not seen[1][10]
    assert seen[0][4] == 3 and list(seen[0][5]) == [1.0, 1.1, 1.2, 0.5, 0.6, 0.7, 2.0, 2.1, 2.2] and seen[0][6:9] == (16000.0, 100.0, -1)
    assert [o.shape for o in out] == [(2, 4), (0, 4), (1, 4)]
    assert np.array_equal(out[0], [[0.0, 10.0, 20.0, 30.0], [1.0, 11.0, 21.0, 31.0]]) and np.array_equal(out[2], [[2.0, 12.0, 22.0, 32.0]])
    del seen[:]
    assert len(E.getShoeboxComponents((3.1, 2.3, 2.7), [0.9] * 6, src[0], (2.0, 1.4, 1.2), 16000.0, 100.0, maxOrder=2)) == 1
    assert seen[0][4] == 1 and seen[0][8] == 2
    del seen[:]
    mics = np.zeros((6, 2))
    ir, counts = E.getArrayRoomIrs((3.1, 2.3, 2.7), [0.9] * 6, src, (2.0, 1.4, 1.2), 16000.0, 120, 4.5, 0.042, mics, returnCounts=True)
    assert ir.shape == (3, 120, 6) and list(counts) == [5, 5, 5]
    assert seen[0][1:7] == (16000.0, 0.042, 4, 6, 0, 6) and seen[0][8] == 3 and seen[0][10:] == (114.5, -1, 4.5, 0, 120)
    enc = np.ones((4, 6)) * (1 + 1j)
    ir = E.getArrayRoomIrs((3.1, 2.3, 2.7), [0.9] * 6, src[1], (2.0, 1.4, 1.2), 16000.0, 120, 4.5, 0.042, mics, order=2, encoder=enc, nfft=512,
                           maxOrder=3, maxDelay=300)
    assert ir.shape == (1, 120, 4) and np.iscomplexobj(ir)
    assert seen[1][1:7] == (16000.0, 0.042, 2, 6, 1, 4) and seen[1][8] == 1 and seen[1][10:] == (300.0, 3, 4.5, 512, 120)
    for bad, word in [(dict(roomDim=(3.1, 2.3)), "roomDim"), (dict(wallReflection=[0.9] * 5), "wallReflection"), (dict(arrayPos=(1.0,)), "arrayPos"),
                      (dict(sourcePos=[[1.0, 2.0]]), "numSources x 3")]:
        kw = dict(dict(roomDim=(3.1, 2.3, 2.7), wallReflection=[0.9] * 6, sourcePos=src, arrayPos=(2.0, 1.4, 1.2)), **bad)
        with pytest.raises(ValueError, match=word):
            E.getShoeboxComponents(fs=16000.0, maxDelay=100.0, **kw)
        with pytest.raises(ValueError, match=word):
            E.getArrayRoomIrs(fs=16000.0, irLen=120, preDelay=4.0, micRadius=0.042, micGridAziZenRad=mics, **kw)


def test_python_forwards_the_librarys_errors(lib):
    import emagls_amd as E
    room_a = ((3.1, 2.3, 2.7), [0.9] * 6)
    with pytest.raises(E._lib.EmaglsError, match="strictly inside the room"):
        E.getShoeboxComponents(*room_a, (1.0, 2.5, 1.0), (2.0, 1.4, 1.2), 16000.0, 100.0)
    with pytest.raises(E._lib.EmaglsError, match="would wrap"):
        E.getArrayRoomIrs(*room_a, (1.0, 1.0, 1.0), (2.0, 1.4, 1.2), 16000.0, 120, 4.0, 0.042, np.zeros((6, 2)), maxDelay=252.0)
    with pytest.raises(E._lib.EmaglsError, match="sphere must lie inside the room"):
        E.getArrayRoomIrs(*room_a, (1.0, 1.0, 1.0), (2.0, 1.4, 0.02), 16000.0, 120, 4.0, 0.042, np.zeros((6, 2)))
