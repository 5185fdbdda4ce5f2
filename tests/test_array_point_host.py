"""The host side of the point-source array responses (emagls_array_irs_point, emagls_shoebox_components_dist,
emagls_array_room_irs_point), without a device:

1. the NumPy restatement that serves the GPU tests as truth (tests/point_reference.py, the direct product b'_n F_n) against mpmath's
   own Bessel functions on a handful of (n, bin, rho);
2. the scaled table and recurrence of section 14, restated in NumPy, against the multiprecision fixture at N = 85
   (tests/golden/point_truth.npz), and the fixture against itself (bin 0 in closed form, the summed responses against the table);
3. the header, the binding and the built library agree on the three entries, and every argument rule is reported before the device
   is touched, with its code and message.

Bounds.  (1) 1e-12 relative: the oracle's b_n and scipy's h_n carry a few 1e-15 each at these orders (the ratio j_n'/h_n' and the
difference of two terms of size 1 at small kappa r lose up to two digits at n = 19).  (2) 1e-13 relative per entry: each of the two
85-step recurrences rounds three times per step, 85 x 3 x 1.1e-16 = 2.8e-14 at worst, twice; in the last bin, where Re b'_n is a
difference, relative to the largest entry of the bin.
"""
import ctypes as C
import os
import re

import mpmath as mp
import numpy as np
import pytest

import point_reference as R
from test_array_room_spectral_host import HEAD, M, NFFT, NR, P, array_side, no_device  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "point_truth.npz")
ARGS = {
    "emagls_array_irs_point": HEAD + ["nsrc", "comp_ptr", "comp_azi", "comp_zen", "comp_delay", "comp_gain", "nsurf", "surf_refl", "comp_exp",
                                      "air_atten", "comp_path", "comp_dist", "pre_delay", "nfft", "nr", "out"],
    "emagls_shoebox_components_dist": ["room_dim", "wall_refl", "array_pos", "nsrc", "src_pos", "fs", "max_delay", "max_order", "capacity",
                                       "comp_ptr", "comp_azi", "comp_zen", "comp_delay", "comp_gain", "comp_dist"],
    "emagls_array_room_irs_point": HEAD + ["room_dim", "wall_refl", "wall_is_spectral", "air_atten", "array_pos", "nsrc", "src_pos", "max_delay",
                                           "max_order", "pre_delay", "nfft", "nr", "comp_count", "out"],
}


# ---- 1. the restatement against mpmath
@pytest.mark.parametrize("n,k,rho", [(0, 1, 1.5), (1, 2, 0.0441), (4, 3, 0.05), (19, 1, 1.5), (19, 100, 30.0), (7, 128, 0.3)])
def test_direct_product_against_mpmath(n, k, rho):
    fs, r, nfft = 16000.0, 0.042, 256
    mp.mp.dps = 60
    jn = lambda n, x: mp.sqrt(mp.pi / (2 * x)) * mp.besselj(n + mp.mpf(1) / 2, x)   # noqa: E731
    yn = lambda n, x: mp.sqrt(mp.pi / (2 * x)) * mp.bessely(n + mp.mpf(1) / 2, x)   # noqa: E731
    h2 = lambda n, x: jn(n, x) - 1j * yn(n, x)                                     # noqa: E731
    kappa = 2 * mp.pi * (mp.mpf(k) * mp.mpf(fs) / nfft) / 343
    x, y = kappa * mp.mpf(r), kappa * mp.mpf(rho)
    bn = 4 * mp.pi * mp.mpc(0, 1) ** n * (jn(n, x) - mp.diff(lambda t: jn(n, t), x) / mp.diff(lambda t: h2(n, t), x) * h2(n, x))
    bp = -bn * (2 * n + 1) / (4 * mp.pi)
    if k == nfft // 2:
        bp = bp.real
    want = complex(bp * mp.mpc(0, -1) ** (n + 1) * y * mp.exp(1j * y) * h2(n, y))
    got = R.direct_product(19, fs, r, nfft, rho)[n, k]
    e = abs(got - want) / abs(want)
    print("direct product n=%d k=%d rho=%g: %.3g" % (n, k, rho, e))
    assert e < 1e-12


def test_bin_zero_is_the_limit():
    """b'_n F_n at kappa = 1e-5 / m in 60-digit arithmetic against -(2n+1)/(n+1) (r/rho)^n, n = 0, 1, 4, 19: the difference is of first
    order in kappa rho = 1.5e-5 (an imaginary part); twice that is allowed.  And the restatements hold the closed form in bin 0."""
    mp.mp.dps = 60
    jn = lambda n, x: mp.sqrt(mp.pi / (2 * x)) * mp.besselj(n + mp.mpf(1) / 2, x)   # noqa: E731
    yn = lambda n, x: mp.sqrt(mp.pi / (2 * x)) * mp.bessely(n + mp.mpf(1) / 2, x)   # noqa: E731
    h2 = lambda n, x: jn(n, x) - 1j * yn(n, x)                                     # noqa: E731
    r, rho, kappa = mp.mpf("0.042"), mp.mpf("1.5"), mp.mpf("1e-5")
    for n in (0, 1, 4, 19):
        x, y = kappa * r, kappa * rho
        bn = 4 * mp.pi * mp.mpc(0, 1) ** n * (jn(n, x) - mp.diff(lambda t: jn(n, t), x) / mp.diff(lambda t: h2(n, t), x) * h2(n, x))
        near = -bn * (2 * n + 1) / (4 * mp.pi) * mp.mpc(0, -1) ** (n + 1) * y * mp.exp(1j * y) * h2(n, y)
        limit = -mp.mpf(2 * n + 1) / (n + 1) * (r / rho) ** n
        assert abs(near - limit) < 2 * kappa * rho * abs(limit), n
        for got in (R.scaled_numpy(19, 16000.0, 0.042, 256, 1.5)[n, 0], R.direct_product(19, 16000.0, 0.042, 256, 1.5)[n, 0]):
            assert got.imag == 0 and abs(got.real - float(limit)) <= 1e-14 * abs(got.real)      # (the power: 19 roundings at most)


# ---- 2. the scaled form against the fixture; the fixture against itself
def test_scaled_form_against_the_multiprecision_table():
    t = np.load(GOLDEN)
    table, bins, rho = t["table"], t["bins"], t["rho"]
    assert table.shape == (86, bins.size, 4) and bins[0] == 0 and bins[-1] == 512 and np.isfinite(table).all()
    worst = 0.0
    for j in range(4):
        got = R.scaled_numpy(85, float(t["fs"]), float(t["r"]), int(t["nfft"]), float(rho[j]))[:, bins]
        assert np.isfinite(got).all()
        want = table[:, :, j]
        e = np.abs(got - want) / np.abs(want)
        e[:, -1] = np.abs(got[:, -1] - want[:, -1]) / np.abs(want[:, -1]).max()
        worst = max(worst, float(e.max()))
    print("scaled form against the table: %.3g" % worst)
    assert worst < 1e-13
    assert np.abs(table[85, 1, 0]) > 1e-8 and np.abs(table[85, 1, 3]) < 1e-200      # (r/rho)^85: 1.2 r against 20 m


def test_fixture_is_consistent():
    t = np.load(GOLDEN)
    table, bins, rho, r = t["table"], t["bins"], t["rho"], float(t["r"])
    n = np.arange(86)
    for j in range(4):
        assert np.allclose(table[:, 0, j], -(2 * n + 1) / (n + 1) * (r / rho[j]) ** n, rtol=1e-14, atol=0)
    from test_gpu_array_irs import unit
    x = unit(t["dirs"]) @ unit(t["mics"]).T                                   # [4 x 2]
    for N in (44, 85):
        p0, p1 = np.ones_like(x), x
        acc = table[0][:, :, None] * p0[None]
        for nn in range(1, N + 1):
            acc = acc + table[nn][:, :, None] * p1[None]
            p0, p1 = p1, ((2 * nn + 1) * x * p1 - nn * p0) / (nn + 1)
        want = t["resp%d" % N][:, bins, :].transpose(1, 0, 2)
        assert np.abs(acc - want).max() < 1e-12 * np.abs(want).max()


# ---- 3. the entries
@pytest.fixture(scope="module")
def lib():
    from emagls_amd import build, _lib
    build.build(jobs=4, verbose=False)
    return _lib.load()


def listed(**over):
    a = dict(array_side(), nsrc=2, comp_ptr=np.array([0, 3, 5], dtype=np.int64), comp_azi=np.zeros(5), comp_zen=np.ones(5),
             comp_delay=np.arange(5.0), comp_gain=np.ones(5), nsurf=2, surf_refl=np.full(2 * P, -0.5), comp_exp=np.arange(10, dtype=np.int32),
             air_atten=np.full(P, 0.01), comp_path=np.arange(5.0), comp_dist=np.array([0.05, 0.3, 1.0, 2.0, 30.0]), out=np.full(2 * M * NR, 7.0))
    a.update(over)
    return a


def room(**over):
    a = dict(array_side(), room_dim=np.array([3.1, 2.3, 2.7]), wall_refl=np.full(6, 0.8), wall_is_spectral=0, air_atten=None,
             array_pos=np.array([2.02, 1.41, 1.17]), nsrc=2, src_pos=np.tile([1.13, 0.71, 1.52], 2), max_delay=100.0, max_order=-1,
             comp_count=np.zeros(2, dtype=np.int64), out=np.full(2 * M * NR, 7.0))
    a.update(over)
    return a


def comps(cap=64, **over):
    a = dict(room_dim=np.array([3.1, 2.3, 2.7]), wall_refl=np.full(6, 0.8), array_pos=np.array([2.02, 1.41, 1.17]), nsrc=2,
             src_pos=np.tile([1.13, 0.71, 1.52], 2), fs=16000.0, max_delay=100.0, max_order=-1, capacity=cap, comp_ptr=np.full(3, -7, dtype=np.int64),
             comp_azi=np.zeros(max(cap, 1)), comp_zen=np.zeros(max(cap, 1)), comp_delay=np.zeros(max(cap, 1)), comp_gain=np.zeros(max(cap, 1)),
             comp_dist=np.zeros(max(cap, 1)))
    a.update(over)
    return a


VALID = {"emagls_array_irs_point": listed, "emagls_shoebox_components_dist": comps, "emagls_array_room_irs_point": room}


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


def test_a_valid_call_gets_as_far_as_the_device(lib):
    from emagls_amd import _lib as L
    if not no_device(lib):
        return      # (with a device the call would run; the rule is about machines without one)
    for a in (listed(), listed(nsurf=0, surf_refl=None, comp_exp=None, air_atten=None, comp_path=None),
              listed(nsurf=0, surf_refl=None, comp_exp=None, air_atten=None, comp_path=None, nfft=0)):
        assert call(lib, "emagls_array_irs_point", a) == L.ERR_HIP, lib.emagls_last_error()
        assert np.all(a["out"] == 7.0)
    for a in (room(), room(air_atten=np.full(P, 0.01)), room(wall_refl=np.full(6 * P, 0.8), wall_is_spectral=1)):
        assert call(lib, "emagls_array_room_irs_point", a) == L.ERR_HIP, lib.emagls_last_error()
    assert call(lib, "emagls_shoebox_components_dist", comps()) == L.ERR_HIP


def test_distance_rules(lib):
    from emagls_amd import _lib as L
    name = "emagls_array_irs_point"
    for bad in (np.nan, np.inf, -1.0, 0.0, 0.042, 0.04):                      # not finite; not beyond the sphere (mic_radius 0.042)
        d = np.array([0.05, 0.3, bad, 2.0, 30.0])
        expect(lib, name, dict(comp_dist=d), L.ERR_ARG, "distances must be finite and greater than mic_radius")
    expect(lib, name, dict(comp_dist=None), L.ERR_ARG, "comp_dist")           # components without distances
    expect(lib, name, dict(comp_path=None), L.ERR_ARG, "both")               # the rules of the spectral entry stand
    expect(lib, name, dict(comp_exp=np.full(10, -1, dtype=np.int32)), L.ERR_ARG, "exponents")
    expect(lib, name, dict(nfft=0), L.ERR_ARG, "nfft must be given")
    expect(lib, name, dict(comp_delay=np.full(5, 300.0)), L.ERR_ARG, "wrap")


def test_overflow_rule(lib):
    """N log10(kappa_max rho_max) - log10((2N-1)!!) >= 300.  At N = 85 (fs 8000): log10(169!!) = 152.82, kappa_max = 73.27, so the
    limit is rho = 10^(452.82 / 85) / 73.27 = 2900 m; at N = 7 a source at 1e9 m is at 73.0 - 5.1.  A room cannot reach the rule: the
    reach of max_delay <= nfft - 1 <= 65535 samples is x = kappa_max rho <= 65535 pi = 2.06e5 at any fs, 298.8 at N = 85 (the
    entry applies the rule all the same, before the device is touched)."""
    from emagls_amd import _lib as L
    name = "emagls_array_irs_point"
    base = dict(fs=8000.0, order=85, nsurf=0, surf_refl=None, comp_exp=None, air_atten=None, comp_path=None, comp_delay=None)
    expect(lib, name, dict(base, comp_dist=np.array([0.05, 0.3, 1.0, 2.0, 3200.0])), L.ERR_UNSUPPORTED, "range of FP64")
    if no_device(lib):
        full = dict(listed(), **dict(base, comp_dist=np.array([0.05, 0.3, 1.0, 2.0, 2500.0])))
        assert call(lib, name, full) == L.ERR_HIP, lib.emagls_last_error()
        full = dict(listed(), comp_dist=np.array([0.05, 0.3, 1.0, 2.0, 1.0e9]))        # N = 7: 7 x 11.2 - 5.1
        assert call(lib, name, full) == L.ERR_HIP, lib.emagls_last_error()


def test_room_rules(lib):
    from emagls_amd import _lib as L
    name = "emagls_array_room_irs_point"
    expect(lib, name, dict(wall_refl=None), L.ERR_ARG, "wall_refl")
    expect(lib, name, dict(wall_refl=np.full(6, 1.5)), L.ERR_ARG, "[-1, 1]")
    expect(lib, name, dict(wall_refl=np.full(6 * P, 1.5), wall_is_spectral=1), L.ERR_ARG, "[-1, 1]")
    expect(lib, name, dict(air_atten=np.full(P, -0.1)), L.ERR_ARG, "attenuation")
    expect(lib, name, dict(air_atten=np.full(P, 0.1), nfft=0), L.ERR_ARG, "nfft must be given")
    expect(lib, name, dict(src_pos=np.tile([2.03, 1.41, 1.17], 2)), L.ERR_ARG, "inside the array's sphere")
    expect(lib, name, dict(max_delay=300.0), L.ERR_ARG, "wrap")
    expect(lib, "emagls_shoebox_components_dist", dict(comp_dist=None), L.ERR_ARG, "component arrays")
    expect(lib, "emagls_shoebox_components_dist", dict(capacity=-1), L.ERR_ARG, "capacity")


def test_python_keywords():
    """Raised by the Python layer or the C entry, in both cases before the device is touched."""
    import emagls_amd as E
    from emagls_amd import _lib as L
    mics = np.array([[0.0, 1.0], [1.0, 2.0]])
    srcs = [np.array([[0.0, 1.0, 2.0, 1.0], [1.0, 1.0, 3.0, 1.0]]), np.array([[2.0, 1.0, 2.0, 1.0]])]
    with pytest.raises(L.EmaglsError) as e:
        E.getArrayIrs(srcs, 16000.0, 64, 4.0, 0.042, mics, distance=[np.array([1.0, 2.0]), None])      # only some of the components
    assert e.value.code == L.ERR_ARG and "for all components" in str(e.value)
    with pytest.raises(L.EmaglsError) as e:
        E.getArrayIrs(srcs, 16000.0, 64, 4.0, 0.042, mics, distance=[np.array([1.0]), np.array([1.0])])
    assert e.value.code == L.ERR_ARG
    with pytest.raises(L.EmaglsError) as e:
        E.getArrayIrs(srcs, 16000.0, 64, 4.0, 0.042, mics, distance=[np.array([1.0, 0.042]), np.array([1.0])])
    assert e.value.code == L.ERR_ARG and "greater than mic_radius" in str(e.value)
    with pytest.raises(L.EmaglsError) as e:
        E.getArrayRoomIrs((3.1, 2.3, 2.7), (0.8,) * 6, (1.13, 0.71, 1.52), (2.02, 1.41, 1.17), 16000.0, 128, 4.0, 0.042, mics, waveModel="sphericalWave")
    assert e.value.code == L.ERR_ARG and "waveModel" in str(e.value)
