"""The host side of source directivity (emagls_array_irs_directive, emagls_shoebox_emission,
emagls_array_room_irs_directive), through ctypes and without a device: the header, the binding and the built library agree on the
three entries, every argument rule is reported before the device is touched with its code and message, and valid arguments without
a GPU fail on the device (there is no CPU fallback).  And the sanity of the NumPy restatement the GPU tests hold the library to
(tests/directivity_reference.py): the first-order pattern to the front and to the back, order-1 coefficients turning as a vector
(which tells R from its transpose), and the constant pattern reproducing the undirected restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest

HEAD = ["fs", "mic_radius", "order", "mic_azi", "mic_zen", "nmics", "enc", "enc_is_complex", "nch"]
ARGS = {
    "emagls_array_irs_directive": HEAD + ["nsrc", "comp_ptr", "comp_azi", "comp_zen", "comp_delay", "comp_gain", "nsurf", "surf_refl", "comp_exp",
                                          "air_atten", "comp_path", "comp_dist", "comp_emit", "src_rot", "dir_order", "dir_coef", "pre_delay",
                                          "nfft", "nr", "out"],
    "emagls_shoebox_emission": ["room_dim", "wall_refl", "array_pos", "nsrc", "src_pos", "fs", "max_delay", "max_order", "capacity", "comp_ptr",
                                "comp_emit"],
    "emagls_array_room_irs_directive": HEAD + ["room_dim", "wall_refl", "wall_is_spectral", "air_atten", "array_pos", "nsrc", "src_pos", "max_delay",
                                               "max_order", "point_source", "src_rot", "dir_order", "dir_coef", "pre_delay", "nfft", "nr",
                                               "comp_count", "out"],
}
COUNTS = {"emagls_array_irs_directive": 29, "emagls_shoebox_emission": 11, "emagls_array_room_irs_directive": 27}
M, NFFT, P, NR = 6, 256, 129, 120


@pytest.fixture(scope="module")
def lib():
    from emagls_amd import build, _lib
    build.build(jobs=4, verbose=False)
    return _lib.load()


def array_side():
    return dict(fs=16000.0, mic_radius=0.042, order=1, mic_azi=np.zeros(M), mic_zen=np.zeros(M), nmics=M, enc=None, enc_is_complex=0, nch=M,
                pre_delay=4.0, nfft=NFFT, nr=NR)


def unit_rows(n):
    e = np.random.default_rng(5).standard_normal((n, 3))
    return e / np.sqrt((e * e).sum(axis=1))[:, None]


def coefficients(nsrc, Nd):
    return np.ones(2 * nsrc * (Nd + 1) ** 2 * P)


def listed(**over):
    """Two sources of 3 and 2 components, order-1 coefficients, a quarter turn about z for the second source."""
    a = dict(array_side(), nsrc=2, comp_ptr=np.array([0, 3, 5], dtype=np.int64), comp_azi=np.zeros(5), comp_zen=np.ones(5),
             comp_delay=np.arange(5.0), comp_gain=np.ones(5), nsurf=0, surf_refl=None, comp_exp=None, air_atten=None, comp_path=None, comp_dist=None,
             comp_emit=unit_rows(5), src_rot=np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, -1, 0, 1, 0, 0, 0, 0, 1]), dir_order=1,
             dir_coef=coefficients(2, 1), out=np.full(2 * M * NR, 7.0))
    a.update(over)
    return a


def room(**over):
    a = dict(array_side(), room_dim=np.array([3.1, 2.3, 2.7]), wall_refl=np.full(6, 0.8), wall_is_spectral=0, air_atten=None,
             array_pos=np.array([2.02, 1.41, 1.17]), nsrc=2, src_pos=np.tile([1.13, 0.71, 1.52], 2), max_delay=100.0, max_order=-1, point_source=0,
             src_rot=None, dir_order=1, dir_coef=coefficients(2, 1), comp_count=np.zeros(2, dtype=np.int64), out=np.full(2 * M * NR, 7.0))
    a.update(over)
    return a


def emission(cap=64, **over):
    a = dict(room_dim=np.array([3.1, 2.3, 2.7]), wall_refl=np.full(6, 0.8), array_pos=np.array([2.02, 1.41, 1.17]), nsrc=2,
             src_pos=np.tile([1.13, 0.71, 1.52], 2), fs=16000.0, max_delay=100.0, max_order=-1, capacity=cap, comp_ptr=np.full(3, -7, dtype=np.int64),
             comp_emit=np.zeros(3 * max(cap, 1)))
    a.update(over)
    return a


VALID = {"emagls_array_irs_directive": listed, "emagls_shoebox_emission": emission, "emagls_array_room_irs_directive": room}


def call(lib, name, a):
    vals = [a[k].ctypes.data_as(C.c_void_p) if isinstance(a[k], np.ndarray) else a[k] for k in ARGS[name]]
    return getattr(lib, name)(*vals)


def expect(lib, name, a, code, word):
    full = dict(VALID[name](), **a)
    rc = call(lib, name, full)
    msg = lib.emagls_last_error().decode()
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
        assert len(params) == COUNTS[name] and [p.split()[-1].lstrip("*") for p in params] == args
        res, argtypes = L.SYMBOLS[name]
        assert res is C.c_int and argtypes == [ctype(p) for p in params], name


def test_python_exports():
    import inspect
    import emagls_amd as E
    assert "firstOrderDirectivity" in E.__all__ and callable(E.firstOrderDirectivity)
    for fn, names in ((E.getArrayIrs, ("emission", "sourceOrientation", "directivity")), (E.getArrayRoomIrs, ("sourceOrientation", "directivity")),
                      (E.getShoeboxComponents, ("returnEmission",)), (E.getShoeboxImages, ("returnEmission",))):
        assert set(names) <= set(inspect.signature(fn).parameters), fn.__name__


def test_a_valid_call_gets_as_far_as_the_device(lib):
    from emagls_amd import _lib as L
    if not no_device(lib):
        return      # (with a device the call would run; the rule is about machines without one)
    for a in (listed(), listed(src_rot=None), listed(comp_dist=np.full(5, 1.0)), listed(dir_order=8, dir_coef=coefficients(2, 8)),
              listed(dir_order=0, dir_coef=coefficients(2, 0)),
              listed(comp_emit=None, src_rot=None, dir_order=0, dir_coef=None)):          # no directivity: the existing entry
        assert call(lib, "emagls_array_irs_directive", a) == L.ERR_HIP, lib.emagls_last_error()
        assert np.all(a["out"] == 7.0)
    for a in (room(), room(point_source=1), room(wall_refl=np.full(6 * P, 0.8), wall_is_spectral=1, air_atten=np.full(P, 0.01)),
              room(dir_order=0, dir_coef=None)):
        assert call(lib, "emagls_array_room_irs_directive", a) == L.ERR_HIP, lib.emagls_last_error()
    for a in (emission(), emission(wall_refl=None), emission(0, comp_emit=None)):
        assert call(lib, "emagls_shoebox_emission", a) == L.ERR_HIP, lib.emagls_last_error()
        assert np.all(a["comp_ptr"] == -7)


def rot_scaled():
    r = np.tile(np.eye(3).ravel(), 2)
    r[9] = 1.0 + 1e-9                                              # source 1: a column that is not of unit length
    return r


def rot_sheared():
    r = np.tile(np.eye(3).ravel(), 2)
    r[1] = 1e-9                                                    # source 0: columns that are not orthogonal
    return r


def rot_reflecting():
    return np.tile(np.diag([1.0, -1.0, 1.0]).ravel(), 2)           # orthonormal, det = -1


def emit_long():
    e = unit_rows(5)
    e[3] *= 1.0 + 1e-9
    return e


def coef_with(v):
    c = coefficients(2, 1)
    c[-1] = v
    return c


RULES = [
    ("emagls_array_irs_directive", dict(src_rot=rot_scaled()), "ERR_ARG", "proper rotation"),
    ("emagls_array_irs_directive", dict(src_rot=rot_sheared()), "ERR_ARG", "proper rotation"),
    ("emagls_array_irs_directive", dict(src_rot=rot_reflecting()), "ERR_ARG", "proper rotation"),
    ("emagls_array_irs_directive", dict(comp_emit=emit_long()), "ERR_ARG", "unit length"),
    ("emagls_array_irs_directive", dict(comp_emit=np.zeros((5, 3))), "ERR_ARG", "unit length"),
    ("emagls_array_irs_directive", dict(dir_order=9, dir_coef=coefficients(2, 9)), "ERR_UNSUPPORTED", "above 8"),
    ("emagls_array_irs_directive", dict(dir_order=-1), "ERR_ARG", "dir_order"),
    ("emagls_array_irs_directive", dict(comp_emit=None), "ERR_ARG", "comp_emit"),
    ("emagls_array_irs_directive", dict(dir_coef=coef_with(np.nan)), "ERR_ARG", "finite"),
    ("emagls_array_irs_directive", dict(dir_coef=coef_with(np.inf)), "ERR_ARG", "finite"),
    ("emagls_array_irs_directive", dict(nfft=0), "ERR_ARG", "nfft must be given"),
    ("emagls_array_irs_directive", dict(dir_coef=None), "ERR_ARG", "without dir_coef"),                       # comp_emit, src_rot, dir_order still set
    ("emagls_array_irs_directive", dict(dir_coef=None, comp_emit=None, src_rot=None), "ERR_ARG", "without dir_coef"),   # dir_order 1
    ("emagls_array_irs_directive", dict(comp_dist=np.array([1.0, 1.0, 0.04, 1.0, 1.0])), "ERR_ARG", "greater than mic_radius"),
    ("emagls_array_irs_directive", dict(comp_ptr=None), "ERR_ARG", "comp_ptr"),
    ("emagls_array_room_irs_directive", dict(src_rot=rot_reflecting()), "ERR_ARG", "proper rotation"),
    ("emagls_array_room_irs_directive", dict(dir_order=9, dir_coef=coefficients(2, 9)), "ERR_UNSUPPORTED", "above 8"),
    ("emagls_array_room_irs_directive", dict(dir_coef=coef_with(np.nan)), "ERR_ARG", "finite"),
    ("emagls_array_room_irs_directive", dict(point_source=2), "ERR_ARG", "point_source"),
    ("emagls_array_room_irs_directive", dict(dir_coef=None), "ERR_ARG", "without dir_coef"),
    ("emagls_array_room_irs_directive", dict(nfft=0), "ERR_ARG", "nfft must be given"),
    ("emagls_array_room_irs_directive", dict(src_pos=np.tile([1.13, 0.71, 3.0], 2)), "ERR_ARG", "inside the room"),
    ("emagls_shoebox_emission", dict(comp_emit=None), "ERR_ARG", "comp_emit"),
    ("emagls_shoebox_emission", dict(capacity=-1), "ERR_ARG", "capacity"),
    ("emagls_shoebox_emission", dict(comp_ptr=None), "ERR_ARG", "comp_ptr"),
    ("emagls_shoebox_emission", dict(wall_refl=np.full(6, 1.5)), "ERR_ARG", "[-1, 1]"),
]


@pytest.mark.parametrize("name,over,code,word", RULES, ids=["%s-%s" % (r[0].replace("emagls_", ""), r[3].replace(" ", "_")) + str(i)
                                                             for i, r in enumerate(RULES)])
def test_argument_rules_come_before_the_device(lib, name, over, code, word):
    from emagls_amd import _lib as L
    expect(lib, name, over, getattr(L, code), word)


def test_python_checks():
    import emagls_amd as E
    from emagls_amd._lib import EmaglsError
    mics = np.zeros((M, 2))
    src = [np.array([[0.0, 1.0, 0.0, 1.0]])]
    with pytest.raises(ValueError, match="not a square"):
        E.getArrayIrs(src, 16000.0, NR, 4.0, 0.042, mics, nfft=NFFT, emission=[unit_rows(1)], directivity=np.ones(5))
    with pytest.raises(ValueError, match="sourceOrientation"):
        E.getArrayIrs(src, 16000.0, NR, 4.0, 0.042, mics, nfft=NFFT, emission=[unit_rows(1)], directivity=np.ones(4), sourceOrientation=np.eye(3))
    with pytest.raises(EmaglsError):
        E.getArrayIrs(src, 16000.0, NR, 4.0, 0.042, mics, nfft=NFFT, directivity=np.ones(4))           # no emission
    with pytest.raises(EmaglsError):
        E.getArrayIrs(src, 16000.0, NR, 4.0, 0.042, mics, nfft=NFFT, emission=[unit_rows(1)])         # no directivity


# ---- the reference's own sanity
def front_of(R):
    return R[:, 0]


def random_rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q if np.linalg.det(q) > 0 else q * np.array([1.0, 1.0, -1.0])


@pytest.mark.parametrize("a", [1.0, 0.75, 0.5, 0.25, 0.0])
def test_first_order_pattern_to_the_front_and_to_the_back(a):
    import emagls_amd as E
    from directivity_reference import directivity_factors
    R = random_rotation(np.random.default_rng(3))
    c = E.firstOrderDirectivity(a)
    assert c.shape == (4,) and c[0] == a * np.sqrt(4 * np.pi) and c[1] == c[2] == 0.0
    e = np.array([front_of(R), -front_of(R), R[:, 1], (front_of(R) + R[:, 1]) / np.sqrt(2.0)])
    D = directivity_factors(e, R, c[:, None].astype(complex))[:, 0]
    assert np.abs(D - [1.0, 2 * a - 1, a, a + (1 - a) / np.sqrt(2.0)]).max() < 1e-15 * 8


def test_orientation_forms_agree():
    from emagls_amd.api import _directive
    o = np.array([[0.3, 1.2], [-2.0, 0.4]])
    _nd, _c, rot = _directive(np.ones(4), o, 2, 3)
    R = rot.reshape(2, 3, 3)
    for q in range(2):
        want = [np.sin(o[q, 1]) * np.cos(o[q, 0]), np.sin(o[q, 1]) * np.sin(o[q, 0]), np.cos(o[q, 1])]
        assert np.abs(front_of(R[q]) - want).max() < 1e-15 and abs(R[q][2, 1]) == 0.0                  # the left axis stays horizontal: zero roll
        assert np.abs(R[q].T @ R[q] - np.eye(3)).max() < 1e-15 and np.linalg.det(R[q]) > 0


def test_order_one_coefficients_turn_as_a_vector():
    """D(e) = c . Y_1(R^T e) with Y_1 = sqrt(3 / 4 pi) (y, z, x): turning the source by R is the pattern with the vector (c_x, c_y, c_z)
    turned by R, seen from the room's axes.  With R and R^T exchanged the two sides differ by O(1)."""
    from directivity_reference import directivity_factors
    rng = np.random.default_rng(17)
    R, e = random_rotation(rng), unit_rows(7)
    c = np.zeros((4, 1), dtype=complex)
    c[1:, 0] = rng.standard_normal(3)
    turned = directivity_factors(e, R, c)[:, 0]
    vec = R @ np.array([c[3, 0], c[1, 0], c[2, 0]]).real          # (x, y, z) from (c_y, c_z, c_x) at the indices 1, 2, 3
    c2 = np.zeros((4, 1), dtype=complex)
    c2[[3, 1, 2], 0] = vec
    fixed = directivity_factors(e, None, c2)[:, 0]
    assert np.abs(turned - fixed).max() < 1e-14
    wrong = directivity_factors(e, R.T, c)[:, 0]
    assert np.abs(wrong - fixed).max() > 0.1


def test_constant_pattern_is_the_undirected_restatement():
    from directivity_reference import directive_spectra
    from test_gpu_array_irs import legendre_spectra, random_dirs
    rng = np.random.default_rng(2)
    mics = random_dirs(rng, 3)
    src = [np.column_stack([random_dirs(rng, 4), rng.uniform(0, 20, 4), rng.uniform(-1, 1, 4)]), np.zeros((0, 4))]
    coef = [np.full((1, 33), np.sqrt(4 * np.pi))] * 2
    got = directive_spectra(16000.0, 0.042, mics, src, [unit_rows(4), np.zeros((0, 3))], None, coef, 1, 64, 4.0)
    want = legendre_spectra(16000.0, 0.042, mics, src, 1, 64, 4.0)
    assert got.shape == want.shape == (2, 33, 3) and not got[1].any()
    assert np.abs(got - want).max() < 1e-14 * np.abs(want).max()
