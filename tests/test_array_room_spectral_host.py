"""The host side of the spectral entries (emagls_array_irs_spectral, emagls_shoebox_images,
emagls_array_room_irs_spectral), through ctypes and without a device: the header, the binding and the built library agree on the
three entries, every argument rule is reported before the device is touched with its code and message, valid arguments without a
GPU fail on the device (there is no CPU fallback); and the two host-only helpers wallReflectionSpectra and airAttenuation."""
import ctypes as C
import os
import re

import numpy as np
import pytest

HEAD = ["fs", "mic_radius", "order", "mic_azi", "mic_zen", "nmics", "enc", "enc_is_complex", "nch"]
ARGS = {
    "emagls_array_irs_spectral": HEAD + ["nsrc", "comp_ptr", "comp_azi", "comp_zen", "comp_delay", "comp_gain", "nsurf", "surf_refl", "comp_exp",
                                         "air_atten", "comp_path", "pre_delay", "nfft", "nr", "out"],
    "emagls_shoebox_images": ["room_dim", "array_pos", "nsrc", "src_pos", "fs", "max_delay", "max_order", "capacity", "comp_ptr", "comp_azi",
                              "comp_zen", "comp_delay", "comp_gain", "comp_exp", "comp_path"],
    "emagls_array_room_irs_spectral": HEAD + ["room_dim", "wall_refl_spec", "air_atten", "array_pos", "nsrc", "src_pos", "max_delay", "max_order",
                                              "pre_delay", "nfft", "nr", "comp_count", "out"],
}
M, NFFT, P, NR = 6, 256, 129, 120


@pytest.fixture(scope="module")
def lib():
    from emagls_amd import build, _lib
    build.build(jobs=4, verbose=False)
    return _lib.load()


def array_side():
    return dict(fs=16000.0, mic_radius=0.042, order=1, mic_azi=np.zeros(M), mic_zen=np.zeros(M), nmics=M, enc=None, enc_is_complex=0, nch=M,
                pre_delay=4.0, nfft=NFFT, nr=NR)


def listed(**over):
    """Two sources of 3 and 2 components, 2 surfaces, air."""
    a = dict(array_side(), nsrc=2, comp_ptr=np.array([0, 3, 5], dtype=np.int64), comp_azi=np.zeros(5), comp_zen=np.ones(5),
             comp_delay=np.arange(5.0), comp_gain=np.ones(5), nsurf=2, surf_refl=np.full(2 * P, -0.5), comp_exp=np.arange(10, dtype=np.int32),
             air_atten=np.full(P, 0.01), comp_path=np.arange(5.0), out=np.full(2 * M * NR, 7.0))
    a.update(over)
    return a


def room(**over):
    a = dict(array_side(), room_dim=np.array([3.1, 2.3, 2.7]), wall_refl_spec=np.full(6 * P, 0.8), air_atten=np.full(P, 0.01),
             array_pos=np.array([2.02, 1.41, 1.17]), nsrc=2, src_pos=np.tile([1.13, 0.71, 1.52], 2), max_delay=100.0, max_order=-1,
             comp_count=np.zeros(2, dtype=np.int64), out=np.full(2 * M * NR, 7.0))
    a.update(over)
    return a


def images(cap=64, **over):
    a = dict(room_dim=np.array([3.1, 2.3, 2.7]), array_pos=np.array([2.02, 1.41, 1.17]), nsrc=2, src_pos=np.tile([1.13, 0.71, 1.52], 2),
             fs=16000.0, max_delay=100.0, max_order=-1, capacity=cap, comp_ptr=np.full(3, -7, dtype=np.int64), comp_azi=np.zeros(max(cap, 1)),
             comp_zen=np.zeros(max(cap, 1)), comp_delay=np.zeros(max(cap, 1)), comp_gain=np.zeros(max(cap, 1)),
             comp_exp=np.zeros(6 * max(cap, 1), dtype=np.int32), comp_path=np.zeros(max(cap, 1)))
    a.update(over)
    return a


VALID = {"emagls_array_irs_spectral": listed, "emagls_shoebox_images": images, "emagls_array_room_irs_spectral": room}


def call(lib, name, a):
    vals = [a[k].ctypes.data_as(C.c_void_p) if isinstance(a[k], np.ndarray) else a[k] for k in ARGS[name]]
    return getattr(lib, name)(*vals)


def expect(lib, name, a, code, word):
    full = dict(VALID[name](), **a)
    rc = call(lib, name, full)
    msg = lib.emagls_last_error()
    assert rc == code, (name, rc, msg)
    assert word in msg, (name, msg)
    if full.get("out") is not None:
        assert np.all(full["out"] == 7.0)


def no_device(lib):
    from emagls_amd import _lib as L
    n = C.c_int(0)
    return not (lib.emagls_device_count(C.byref(n)) == L.OK and n.value > 0)


def test_header_binding_and_library_agree(lib):
    from emagls_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "emagls.h")).read(), flags=re.S)

    def ctype(p):
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
    names = {"getShoeboxImages", "wallReflectionSpectra", "airAttenuation"}
    assert names <= set(E.__all__) and all(callable(getattr(E, n)) for n in names)


def test_a_valid_call_gets_as_far_as_the_device(lib):
    from emagls_amd import _lib as L
    if not no_device(lib):
        return      # (with a device the call would run; the rule is about machines without one)
    for a in (listed(), listed(air_atten=None, comp_path=None), listed(nsurf=0, surf_refl=None, comp_exp=None),
              listed(nsurf=0, surf_refl=None, comp_exp=None, air_atten=None, comp_path=None),
              listed(nsurf=8, surf_refl=np.tile([1.0, -1.0, 0.0], 8 * P // 3 + 1)[:8 * P].copy(), comp_exp=np.zeros(40, dtype=np.int32))):
        assert call(lib, "emagls_array_irs_spectral", a) == L.ERR_HIP, lib.emagls_last_error()
        assert np.all(a["out"] == 7.0)
    for a in (images(), images(cap=0), dict(images(cap=0), comp_azi=None, comp_zen=None, comp_delay=None, comp_gain=None, comp_exp=None,
                                            comp_path=None)):
        assert call(lib, "emagls_shoebox_images", a) == L.ERR_HIP and np.all(a["comp_ptr"] == -7)
    for a in (room(), room(air_atten=None), room(comp_count=None), room(wall_refl_spec=np.zeros(6 * P))):
        assert call(lib, "emagls_array_room_irs_spectral", a) == L.ERR_HIP and np.all(a["out"] == 7.0)


def test_nfft_must_be_given(lib):
    from emagls_amd import _lib as L
    expect(lib, "emagls_array_irs_spectral", dict(nfft=0), L.ERR_ARG, b"nfft must be given")
    expect(lib, "emagls_array_room_irs_spectral", dict(nfft=0), L.ERR_ARG, b"nfft must be given")


def test_the_number_of_surfaces(lib):
    from emagls_amd import _lib as L
    expect(lib, "emagls_array_irs_spectral", dict(nsurf=9, surf_refl=np.zeros(9 * P), comp_exp=np.zeros(45, dtype=np.int32)), L.ERR_ARG, b"0 .. 8")
    expect(lib, "emagls_array_irs_spectral", dict(nsurf=-1), L.ERR_ARG, b"0 .. 8")


def test_null_pointers(lib):
    from emagls_amd import _lib as L
    expect(lib, "emagls_array_irs_spectral", dict(surf_refl=None), L.ERR_ARG, b"null pointer: surf_refl")
    expect(lib, "emagls_array_irs_spectral", dict(comp_exp=None), L.ERR_ARG, b"null pointer: comp_exp")
    expect(lib, "emagls_array_irs_spectral", dict(comp_ptr=None), L.ERR_ARG, b"null pointer: comp_ptr")
    expect(lib, "emagls_array_irs_spectral", dict(out=None), L.ERR_ARG, b"null pointer: out")
    expect(lib, "emagls_array_room_irs_spectral", dict(wall_refl_spec=None), L.ERR_ARG, b"null pointer: wall_refl_spec")
    expect(lib, "emagls_array_room_irs_spectral", dict(room_dim=None), L.ERR_ARG, b"null pointer")
    expect(lib, "emagls_shoebox_images", dict(comp_ptr=None), L.ERR_ARG, b"null pointer: comp_ptr")
    expect(lib, "emagls_shoebox_images", dict(comp_exp=None), L.ERR_ARG, b"null pointer: component arrays")
    expect(lib, "emagls_shoebox_images", dict(comp_path=None), L.ERR_ARG, b"null pointer: component arrays")
    expect(lib, "emagls_shoebox_images", dict(capacity=-1), L.ERR_ARG, b"capacity")


def test_the_air_pair(lib):
    from emagls_amd import _lib as L
    expect(lib, "emagls_array_irs_spectral", dict(air_atten=None), L.ERR_ARG, b"both be given or both be NULL")
    expect(lib, "emagls_array_irs_spectral", dict(comp_path=None), L.ERR_ARG, b"both be given or both be NULL")


@pytest.mark.parametrize("bad", [1.0000001, -1.5, np.nan, np.inf])
def test_reflection_spectra_outside_minus_one_to_one(lib, bad):
    from emagls_amd import _lib as L
    for i in (0, P - 1, 2 * P - 1):
        r = np.full(2 * P, -0.5)
        r[i] = bad
        expect(lib, "emagls_array_irs_spectral", dict(surf_refl=r), L.ERR_ARG, b"[-1, 1]")
    for i in (0, 6 * P - 1):
        r = np.full(6 * P, 0.8)
        r[i] = bad
        expect(lib, "emagls_array_room_irs_spectral", dict(wall_refl_spec=r), L.ERR_ARG, b"[-1, 1]")


@pytest.mark.parametrize("bad", [-1e-9, np.nan, np.inf])
def test_attenuation_and_paths(lib, bad):
    from emagls_amd import _lib as L
    for name in ("emagls_array_irs_spectral", "emagls_array_room_irs_spectral"):
        a = np.full(P, 0.01)
        a[P - 1] = bad
        expect(lib, name, dict(air_atten=a), L.ERR_ARG, b"air attenuation must be non-negative and finite")
    p = np.arange(5.0)
    p[4] = bad
    expect(lib, "emagls_array_irs_spectral", dict(comp_path=p), L.ERR_ARG, b"path lengths must be non-negative and finite")


def test_negative_exponents(lib):
    from emagls_amd import _lib as L
    e = np.arange(10, dtype=np.int32)
    e[9] = -1
    expect(lib, "emagls_array_irs_spectral", dict(comp_exp=e), L.ERR_ARG, b"exponents must be non-negative")


def test_the_rules_shared_with_the_flat_entries(lib):
    from emagls_amd import _lib as L
    one = "emagls_array_irs_spectral"
    expect(lib, one, dict(nfft=48), L.ERR_ARG, b"power of two")
    expect(lib, one, dict(nr=300), L.ERR_ARG, b"nr exceeds nfft")
    expect(lib, one, dict(comp_ptr=np.array([1, 3, 5], dtype=np.int64)), L.ERR_ARG, b"comp_ptr must start at 0")
    expect(lib, one, dict(comp_delay=np.array([0.0, 1.0, 2.0, 3.0, 252.0])), L.ERR_ARG, b"would wrap")
    expect(lib, one, dict(comp_gain=np.array([1.0, 1.0, np.nan, 1.0, 1.0])), L.ERR_ARG, b"gains must be finite")
    two = "emagls_array_room_irs_spectral"
    expect(lib, two, dict(max_delay=251.5), L.ERR_ARG, b"would wrap")
    expect(lib, two, dict(max_delay=0.0), L.ERR_ARG, b"max_delay must be positive and finite")
    expect(lib, two, dict(src_pos=np.array([1.13, 0.71, 1.52, 1.0, 2.4, 1.0])), L.ERR_ARG, b"source 1 does not lie strictly inside the room")
    expect(lib, two, dict(array_pos=np.array([0.04, 1.41, 1.17])), L.ERR_ARG, b"sphere must lie inside the room")
    expect(lib, "emagls_shoebox_images", dict(max_order=-2), L.ERR_ARG, b"max_order")
    expect(lib, "emagls_shoebox_images", dict(max_delay=40000.0), L.ERR_UNSUPPORTED, b"2^28 image-source candidates")


def test_the_24_gib_estimate_before_the_count(lib):
    """As in the flat room: 4096 source positions on 64 microphones at nfft = 65536 are 1.4e11 bytes of spectra."""
    from emagls_amd import _lib as L
    room_a = room(nmics=64, mic_azi=np.zeros(64), mic_zen=np.zeros(64), nch=64, nfft=65536, nr=8, nsrc=4096,
                  src_pos=np.tile([1.13, 0.71, 1.52], 4096), wall_refl_spec=np.zeros(6 * 32769), air_atten=None, out=np.full(4096 * 64 * 8, 7.0))
    assert call(lib, "emagls_array_room_irs_spectral", room_a) == L.ERR_UNSUPPORTED and b"24 GiB" in lib.emagls_last_error()


def test_wall_reflection_spectra_by_hand():
    """Three bands at 250, 1000 and 4000 Hz with a = 0.1, 0.3, 0.5; fs 16000, nfft 64: bins of 250 Hz.  Bin 0 (0 Hz) and bin 1 (250 Hz, the
    first centre): 0.1.  Bin 2 (500 Hz): half way in log2 between 250 and 1000, 0.2.  Bin 4 (1000 Hz): 0.3.  Bin 8 (2000 Hz): 0.4.
    Bin 16 (4000 Hz) and all above: 0.5.  Bin 3 (750 Hz): 0.1 + 0.2 log2(3) / 2."""
    import emagls_amd as E
    R = E.wallReflectionSpectra([[0.1, 0.3, 0.5], [0.0, 0.0, 1.0]], [250.0, 1000.0, 4000.0], 16000.0, 64)
    assert R.shape == (2, 33)
    a = 1.0 - R[0] ** 2
    want = {0: 0.1, 1: 0.1, 2: 0.2, 4: 0.3, 8: 0.4, 16: 0.5, 17: 0.5, 32: 0.5, 3: 0.1 + 0.2 * np.log2(3.0) / 2.0}
    for k, v in want.items():
        assert abs(a[k] - v) < 1e-14, (k, a[k], v)
    assert R[1, 0] == 1.0 and R[1, 4] == 1.0 and R[1, 16] == 0.0 and R[1, 32] == 0.0
    with pytest.raises(ValueError, match="ascending"):
        E.wallReflectionSpectra([[0.1, 0.3]], [1000.0, 250.0], 16000.0, 64)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        E.wallReflectionSpectra([[0.1, 1.3]], [250.0, 1000.0], 16000.0, 64)


def db_per_km(f, **kw):
    """airAttenuation at exactly f: bin 1 of a two-point transform at fs = 2 f."""
    import emagls_amd as E
    a = E.airAttenuation(2.0 * f, 2, **kw)
    assert a.shape == (2,) and a[0] == 0.0
    return float(a[1]) * 20.0 / np.log(10.0) * 1000.0


def test_air_attenuation_against_iso_9613_2_table_2():
    """20 degrees, 70 percent, 101.325 kPa at the exact mid-band frequencies 1000 * 10^(0.3 n), n = -4 .. 3."""
    got = [round(db_per_km(1000.0 * 10.0 ** (0.3 * n), temperatureC=20.0, relHumidityPercent=70.0, pressureKPa=101.325), 1) for n in range(-4, 4)]
    assert got == [0.1, 0.3, 1.1, 2.8, 5.0, 9.0, 22.9, 76.6]


def test_air_attenuation_at_1_khz():
    assert abs(db_per_km(1000.0, temperatureC=20.0, relHumidityPercent=50.0) - 4.665) < 0.001
    import emagls_amd as E
    a = E.airAttenuation(16000.0, 1024)
    assert a.shape == (513,) and a[0] == 0.0 and np.all(np.diff(a) > 0)


def test_python_shapes_the_arguments(lib, monkeypatch):
    """What the wrappers hand to the C calls (which are replaced: no device here)."""
    import emagls_amd as E
    from emagls_amd import api
    seen = []

    def arr(p, n, t=C.c_double):
        return None if p is None else np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), shape=(n,))

    class Fake:
        def emagls_array_irs(self, *a):
            seen.append(("flat",))
            return 0

        def emagls_array_room_irs(self, *a):
            seen.append(("flat room",))
            return 0

        def emagls_array_irs_spectral(self, *a):
            n = int(arr(a[10], a[9] + 1, C.c_int64)[-1])
            seen.append(("spectral", a[15], arr(a[16], a[15] * 129).copy() if a[15] else None,
                         arr(a[17], n * a[15], C.c_int32).copy() if a[15] else None, None if a[18] is None else arr(a[18], 129).copy(),
                         None if a[19] is None else arr(a[19], n).copy(), a[21]))
            return 0

        def emagls_shoebox_images(self, dim, pos, Q, src, fs, max_delay, max_order, cap, ptr, azi, zen, delay, gain, ex, path):
            seen.append(("images", Q, fs, max_delay, max_order, cap))
            arr(ptr, Q + 1, C.c_int64)[:] = [0, 2, 2, 3][:Q + 1]
            if cap:
                for k, p in enumerate((azi, zen, delay, gain, path)):
                    arr(p, cap)[:] = 10.0 * k + np.arange(cap)
                arr(ex, 6 * cap, C.c_int32)[:] = np.arange(6 * cap)
            return 0

        def emagls_array_room_irs_spectral(self, *a):
            seen.append(("room", arr(a[10], 6 * 129).copy(), None if a[11] is None else arr(a[11], 129).copy(), a[13], a[15], a[18], a[19]))
            return 0

    monkeypatch.setattr(api.L, "load", lambda: Fake())
    mics, src = np.zeros((6, 2)), [np.zeros((2, 4)), np.zeros((0, 4)), np.zeros((1, 4))]
    assert E.getArrayIrs(src, 16000.0, 120, 4.0, 0.042, mics).shape == (3, 120, 6) and seen == [("flat",)]
    del seen[:]
    refl, ex = np.linspace(-1, 1, 2 * 129).reshape(2, 129), [[[1, 2], [3, 4]], np.zeros((0, 2)), [[5, 6]]]
    att, path = np.linspace(0, 0.1, 129), [[1.0, 2.0], [], [3.0]]
    E.getArrayIrs(src, 16000.0, 120, 4.0, 0.042, mics, surfaceReflection=refl, exponents=ex, airAttenuation=att, pathLength=path)
    s = seen[0]
    assert s[0] == "spectral" and s[1] == 2 and np.array_equal(s[2], refl.ravel()) and list(s[3]) == [1, 2, 3, 4, 5, 6]
    assert np.array_equal(s[4], att) and list(s[5]) == [1.0, 2.0, 3.0] and s[6] == 256            # nfft: the smallest power of two >= 2 irLen
    del seen[:]
    E.getArrayIrs(src, 16000.0, 120, 4.0, 0.042, mics, airAttenuation=att, pathLength=path)
    assert seen[0][1] == 0 and seen[0][2] is None and list(seen[0][5]) == [1.0, 2.0, 3.0]
    for kw, word in [(dict(surfaceReflection=refl), "exponents"), (dict(airAttenuation=att), "pathLength"),
                     (dict(surfaceReflection=refl[:, :100], exponents=ex), "129 bins"), (dict(surfaceReflection=refl, exponents=ex[:2]), "one array per source"),
                     (dict(surfaceReflection=refl, exponents=[[[1, 2], [3, 4]], [], [[5.5, 6]]]), "integers"),
                     (dict(airAttenuation=att, pathLength=[[1.0], [], [3.0]]), "pathLength")]:
        with pytest.raises(ValueError, match=word):
            E.getArrayIrs(src, 16000.0, 120, 4.0, 0.042, mics, **kw)
    del seen[:]
    cs, es, ps = E.getShoeboxImages((3.1, 2.3, 2.7), [[1.0, 1.1, 1.2]] * 3, (2.0, 1.4, 1.2), 16000.0, 100.0, maxOrder=2)
    assert seen == [("images", 3, 16000.0, 100.0, 2, 0), ("images", 3, 16000.0, 100.0, 2, 3)]
    assert [c.shape for c in cs] == [(2, 4), (0, 4), (1, 4)] and [e.shape for e in es] == [(2, 6), (0, 6), (1, 6)] and [p.shape for p in ps] == [(2,), (0,), (1,)]
    assert np.array_equal(cs[0], [[0.0, 10.0, 20.0, 30.0], [1.0, 11.0, 21.0, 31.0]]) and list(es[2][0]) == list(range(12, 18)) and list(ps[0]) == [40.0, 41.0]
    del seen[:]
    room_a = ((3.1, 2.3, 2.7), [0.9, 0.8, 0.7, 0.6, 0.5, 0.4], (1.0, 1.1, 1.2), (2.0, 1.4, 1.2), 16000.0, 120, 4.5, 0.042, mics)
    E.getArrayRoomIrs(*room_a)
    assert seen == [("flat room",)]
    del seen[:]
    E.getArrayRoomIrs(*room_a, airAttenuation=att)                     # six coefficients with air: repeated over the bins
    walls = np.repeat(np.array(room_a[1])[:, None], 129, axis=1)
    assert seen[0][0] == "room" and np.array_equal(seen[0][1], walls.ravel()) and np.array_equal(seen[0][2], att)
    assert seen[0][3:] == (1, 114.5, 256, 120)
    E.getArrayRoomIrs(room_a[0], walls * 0.5, *room_a[2:])
    assert np.array_equal(seen[1][1], walls.ravel() * 0.5) and seen[1][2] is None
    with pytest.raises(ValueError, match="129 bins"):
        E.getArrayRoomIrs(room_a[0], walls[:, :64], *room_a[2:])
    with pytest.raises(ValueError, match="129 bins"):
        E.getArrayRoomIrs(*room_a, airAttenuation=att[:50])


def test_python_forwards_the_librarys_errors(lib):
    import emagls_amd as E
    with pytest.raises(E._lib.EmaglsError, match=r"\[-1, 1\]"):
        E.getArrayRoomIrs((3.1, 2.3, 2.7), np.full((6, 129), 1.5), (1.0, 1.0, 1.0), (2.0, 1.4, 1.2), 16000.0, 120, 4.0, 0.042, np.zeros((6, 2)))
    with pytest.raises(E._lib.EmaglsError, match="strictly inside the room"):
        E.getShoeboxImages((3.1, 2.3, 2.7), (1.0, 2.5, 1.0), (2.0, 1.4, 1.2), 16000.0, 100.0)
    with pytest.raises(E._lib.EmaglsError, match="exponents must be non-negative"):
        E.getArrayIrs([np.zeros((1, 4))], 16000.0, 120, 4.0, 0.042, np.zeros((6, 2)), surfaceReflection=np.zeros((1, 129)), exponents=[[[-1]]])
