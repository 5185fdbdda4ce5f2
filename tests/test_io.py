"""Fixture / data I/O: the harness's save() variable lists round-trip through MAT -v7, the reference's own
golden files are read back by the same loader, and the HRIR loader takes the MIRO field names as plain arrays."""
import os

import numpy as np
import pytest
import scipy.io as sio

from emagls_amd import io as IO


def test_fixture_name_matches_the_harness_pattern():
    # verifyEMagLs.m:25-32 with filterLen 512, 32 microphones, order 4
    assert IO.fixture_name(512, 32, 4, "real", "eMagLS", dc=False) == "HRIR_L2702_512samples_32channels_sh4_real_eMagLS_woDC.mat"
    assert IO.fixture_name(512, 32, 4, "complex", "LS") == "HRIR_L2702_512samples_32channels_sh4_complex_LS.mat"
    assert IO.fixture_name(512, 32, 4, "real", "MagLS", dc=True).endswith("_real_MagLS_wDC.mat")
    with pytest.raises(ValueError):
        IO.fixture_name(512, 32, 4, "real", "eMagLS3")


@pytest.mark.parametrize("cplx", [False, True])
def test_save_fixture_round_trip(tmp_path, golden, grids, cplx):
    """Write the eMagLS set the way verifyEMagLs.m:218-221 does and read it back: same variables, values, dtypes, shapes
    (grids as column vectors, scalars 1x1) -- and byte-compatible with how the reference's own fixture loads."""
    tag = ("complex" if cplx else "real") + "_eMagLS_woDC"
    wL, wR = golden[tag + "/wEMlsL"], golden[tag + "/wEMlsR"]
    assert np.iscomplexobj(wL) == cplx
    f = str(tmp_path / IO.fixture_name(512, 32, 4, "complex" if cplx else "real", "eMagLS", dc=False))
    IO.save_fixture(f, "eMagLS", wEMlsL=wL, wEMlsR=wR, hrirGridAziRad=grids["azi"], hrirGridZenRad=grids["zen"],
                    micRadius=grids["mic_radius"], micGridAziRad=grids["mic_azi"], micGridZenRad=grids["mic_zen"], shOrder=4,
                    fs=48000.0, filterLen=512)
    raw = sio.loadmat(f)
    assert sorted(k for k in raw if not k.startswith("__")) == sorted(IO.FIXTURE_FIELDS["eMagLS"])
    assert raw["hrirGridAziRad"].shape == (2702, 1) and raw["shOrder"].shape == (1, 1) and raw["wEMlsL"].shape == (512, 25)
    assert raw["wEMlsL"].dtype == (np.complex128 if cplx else np.float64)
    with open(f, "rb") as fh:
        assert fh.read(19) == b"MATLAB 5.0 MAT-file"          # '-v7' is the level-5 container (with compression)
    d = IO.load_fixture(f)
    assert np.array_equal(d["wEMlsL"], wL) and np.array_equal(d["wEMlsR"], wR)
    assert np.array_equal(d["hrirGridAziRad"], grids["azi"]) and d["micRadius"] == grids["mic_radius"] and d["filterLen"] == 512.0


def test_save_fixture_checks_the_variable_list(tmp_path):
    with pytest.raises(ValueError, match="missing"):
        IO.save_fixture(str(tmp_path / "x.mat"), "LS", wLsL=np.zeros((4, 4)), wLsR=np.zeros((4, 4)))
    with pytest.raises(ValueError, match="unexpected"):
        IO.save_fixture(str(tmp_path / "x.mat"), "LS", wLsL=np.zeros((4, 4)), wLsR=np.zeros((4, 4)), hrirGridAziRad=[0.0],
                        hrirGridZenRad=[0.0], shOrder=1, fs=48000.0)


def test_load_fixture_reads_the_reference_files(golden):
    """One of the reference's own MATLAB-written regression fixtures (resources/, stored verbatim under tests/golden/; data under
    the reference's licence, see tests/golden/make_fixtures.py) read back by the loader."""
    d = IO.load_fixture(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                     "HRIR_L2702_512samples_32channels_sh4_complex_MagLS_woDC.mat"))
    assert set(d) == set(IO.FIXTURE_FIELDS["MagLS"]) | {"applyDiffusenessConst"} and d["applyDiffusenessConst"] == 0.0
    assert np.array_equal(d["wMlsL"], golden["complex_MagLS_woDC/wMlsL"]) and d["fs"] == 48000.0 and d["shOrder"] == 4.0
    assert d["hrirGridAziRad"].shape == (2702,)


def _hrir_arrays():
    rng = np.random.default_rng(0)
    return rng.standard_normal((16, 6)), rng.standard_normal((16, 6)), np.linspace(0, 5, 6), np.linspace(0.1, 3, 6)


def test_load_hrir_set_containers(tmp_path):
    hL, hR, azi, zen = _hrir_arrays()
    # the MIRO field names at top level (save -struct) and inside a struct variable, as single precision like the original
    sio.savemat(str(tmp_path / "plain.mat"), dict(irChOne=hL.astype(np.float32), irChTwo=hR.astype(np.float32), azimuth=azi[None, :],
                                                  elevation=zen[None, :], fs=np.array([[48000]])))
    sio.savemat(str(tmp_path / "struct.mat"), dict(HRIR_L2702=dict(irChOne=hL, irChTwo=hR, azimuth=azi, elevation=zen, fs=48000.0)))
    np.savez(str(tmp_path / "a.npz"), hL=hL, hR=hR)
    np.savez(str(tmp_path / "b.npz"), irChOne=hL, irChTwo=hR, azimuth=azi, elevation=zen, fs=48000)
    for name, exact, grid in (("plain.mat", False, True), ("struct.mat", True, True), ("a.npz", True, False), ("b.npz", True, True)):
        d = IO.load_hrir_set(str(tmp_path / name))
        assert d["hL"].dtype == np.float64 and d["hL"].shape == (16, 6)
        assert np.allclose(d["hL"], hL, atol=0 if exact else 1e-6) and np.allclose(d["hR"], hR, atol=0 if exact else 1e-6)
        if grid:
            assert np.array_equal(d["azi"], azi) and np.array_equal(d["zen"], zen) and d["fs"] == 48000.0
        else:
            assert "azi" not in d


def test_load_hrir_set_errors(tmp_path):
    hL, hR, azi, zen = _hrir_arrays()
    sio.savemat(str(tmp_path / "bad.mat"), dict(something=hL))
    with pytest.raises(ValueError, match="neither"):
        IO.load_hrir_set(str(tmp_path / "bad.mat"))
    sio.savemat(str(tmp_path / "obj.mat"), dict(HRIR_L2702=np.zeros((6, 1), dtype=np.uint32)))   # what a missing class leaves (:57)
    with pytest.raises(ValueError, match="MATLAB object"):
        IO.load_hrir_set(str(tmp_path / "obj.mat"))
    sio.savemat(str(tmp_path / "grid.mat"), dict(irChOne=hL, irChTwo=hR, azimuth=azi[:3], elevation=zen, fs=1.0))
    with pytest.raises(ValueError, match="grid angles"):
        IO.load_hrir_set(str(tmp_path / "grid.mat"))
    with pytest.raises(ValueError, match="unsupported"):
        IO.load_hrir_set(str(tmp_path / "x.wav"))
    (tmp_path / "x.sofa").write_bytes(b"not an HDF5 file at all")
    with pytest.raises(ValueError, match="not an HDF5 file"):
        IO.load_hrir_set(str(tmp_path / "x.sofa"))


GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _check_set(d, e, tol=0.0):
    assert d["hL"].shape == e["hL"].shape and d["hL"].dtype == np.float64
    for k in ("hL", "hR", "azi", "zen"):
        assert np.abs(d[k] - e[k]).max() <= max(tol, 2e-15), k
    assert d["fs"] == float(e["fs"])


def test_load_hrir_set_from_the_sofa_twin_and_from_mat_v73():
    """f3: the published set's SOFA container (netCDF-4 / HDF5: creation-order-tracked root group with dense link and
    attribute storage, Data.IR chunked + shuffled + deflated) and a -v7.3 MAT file (HDF5 behind a 512-byte user block,
    column-major data) -- committed files written by libhdf5 1.10.6 (tests/h5gen.py), read by emagls_amd/hdf5_min.py."""
    e = np.load(os.path.join(GOLD, "hrir_small_expected.npz"))
    _check_set(IO.load_hrir_set(os.path.join(GOLD, "hrir_small.sofa")), e)
    _check_set(IO.load_hrir_set(os.path.join(GOLD, "hrir_small_v73.mat")), e)
    from emagls_amd import hdf5_min as H5
    f = H5.File(os.path.join(GOLD, "hrir_small.sofa"))
    assert f.attrs["SOFAConventions"] == "SimpleFreeFieldHRIR" and len(f.attrs) == 16 and len(f.keys()) == 15
    kinds = {m[0] for m in f._msgs}
    assert 0x02 in kinds and 0x11 not in kinds      # link info message, no symbol table: the dense link storage was read
    assert f["Data.IR"]._filters and f["Data.IR"].shape == (38, 2, 24)
    assert f["SourcePosition"].attrs == {"Type": "spherical", "Units": "degree, degree, metre"}


def _libhdf5():
    import h5gen
    return h5gen.find_libhdf5()


@pytest.mark.skipif("_libhdf5() is None", reason="libhdf5 (test tooling) not in this image")
@pytest.mark.parametrize("kw", [dict(latest=True), dict(vlen_attrs=True), dict(chunked=False, ir_dtype="f4"),
                                dict(position_type="cartesian")])
def test_sofa_variants_written_by_libhdf5(tmp_path, kw):
    """Newest file format (superblock 3, version-2 object headers, fixed-array chunk index), variable-length string
    attributes (global heap), contiguous single-precision data, Cartesian source positions."""
    import h5gen
    hs = h5gen.small_hrir_set(seed=11, ndirs=50, nsamp=32)
    f = str(tmp_path / "v.sofa")
    h5gen.write_sofa(f, hs, **kw)
    _check_set(IO.load_hrir_set(f), hs, tol=1e-6 if "ir_dtype" in kw else 1e-12)


@pytest.mark.skipif("_libhdf5() is None", reason="libhdf5 (test tooling) not in this image")
@pytest.mark.parametrize("latest", [False, True])
@pytest.mark.parametrize("track", [False, True])
def test_hdf5_reader_on_large_groups_and_filtered_chunks(tmp_path, latest, track):
    """300 links in one group (symbol-table B-tree with several nodes / fractal heap with indirect blocks and a version-2
    B-tree of depth > 0), 40 attributes on one object, big-endian + shuffle + deflate + fletcher32 chunks with partial edge
    chunks, a paged fixed-array index (1750 chunks), fixed-length strings, nested groups."""
    import h5gen
    from emagls_amd import hdf5_min as H5
    rng = np.random.default_rng(0)
    w = h5gen.Writer(str(tmp_path / "m.h5"), latest=latest, track_order=track)
    w.group("g")
    w.group("g/sub")
    exp = {}
    for i in range(300):
        exp["g/sub/ds_%03d_long_name_to_fill_heaps" % i] = rng.standard_normal((3, i % 5 + 1))
        w.dataset("g/sub/ds_%03d_long_name_to_fill_heaps" % i, exp["g/sub/ds_%03d_long_name_to_fill_heaps" % i])
    for i in range(40):
        w.attr("g", "attr%02d" % i, np.arange(i + 1, dtype=np.int32))
    w.dataset("be", np.arange(12, dtype="f8").reshape(3, 4), big_endian=True, chunks=(2, 3), fletcher=True, deflate=2, shuffle=True)
    big = rng.standard_normal((70, 50))
    w.dataset("paged", big, chunks=(2, 1), deflate=1)
    w.dataset("s", np.array([b"ab", b"cde"], dtype="S4"))
    w.close()
    f = H5.File(str(tmp_path / "m.h5"))
    assert sorted(f["g/sub"].keys()) == sorted(k.split("/")[-1] for k in exp)
    assert all(np.array_equal(f[k].read(), v) for k, v in exp.items())
    at = f["g"].attrs
    assert len(at) == 40 and all(np.array_equal(at["attr%02d" % i], np.arange(i + 1)) for i in range(40))
    if latest:
        assert 0x15 in {m[0] for m in f["g"]._msgs}      # attribute info message: dense attribute storage was read
    assert np.array_equal(f["be"].read(), np.arange(12.0).reshape(3, 4)) and np.array_equal(f["paged"].read(), big)
    assert f["s"].read().tolist() == ["ab", "cde"]
    with pytest.raises(KeyError):
        f["g/nothing"]


def test_mat_v73_object_variable_is_refused_with_the_way_out(tmp_path):
    if _libhdf5() is None:
        pytest.skip("libhdf5 (test tooling) not in this image")
    import h5gen
    w = h5gen.Writer(str(tmp_path / "o.mat"), userblock=512)
    w.group("HRIR_L2702")
    w.attr("HRIR_L2702", "MATLAB_class", "miro")
    w.close()
    h5gen.stamp_mat73_header(str(tmp_path / "o.mat"))
    with pytest.raises(ValueError, match="class 'miro'"):
        IO.load_hrir_set(str(tmp_path / "o.mat"))


def test_load_hrir_set_from_a_classdef_object(tmp_path):
    """A -v7 file holding the MIRO instance itself (opaque variable + subsystem element).  The file is built by
    tests/mcosgen.py from the layout emagls_amd/mcos.py describes -- a consistency test of the decoder, not a check against
    MATLAB's output (none exists in the image)."""
    import mcosgen
    hL, hR, azi, zen = _hrir_arrays()
    props = dict(irChOne=hL.astype(np.float32), irChTwo=hR.astype(np.float32), azimuth=azi[None, :], elevation=zen[None, :],
                 fs=np.array([[48000.0]]), name="HRIR_L2702")
    for version in (2, 3, 4):
        f = str(tmp_path / ("obj%d.mat" % version))
        mcosgen.write_object_mat(f, "HRIR_L2702", "miro", props, defaults=dict(radius=np.array([[3.25]])), version=version)
        d = IO.load_hrir_set(f)
        assert np.allclose(d["hL"], hL, atol=1e-6) and np.array_equal(d["azi"], azi) and np.array_equal(d["zen"], zen) and d["fs"] == 48000.0
    from emagls_amd import mcos
    objs = mcos.object_properties(sio.loadmat(f, struct_as_record=False))
    cls, p = objs["HRIR_L2702"]
    assert cls == "miro" and float(np.asarray(p["radius"]).ravel()[0]) == 3.25          # a property the object leaves unset reads as the class default
    mcosgen.write_object_mat(f, "other", "thing", dict(a=np.zeros((2, 2))))
    with pytest.raises(ValueError, match="no irChOne"):
        IO.load_hrir_set(f)
    raw = bytearray(open(f, "rb").read())
    raw[-200:] = b"\0" * 200
    (tmp_path / "broken.mat").write_bytes(bytes(raw))
    with pytest.raises(Exception):
        IO.load_hrir_set(str(tmp_path / "broken.mat"))


@pytest.mark.parametrize("name", ["hrir_small.sofa", "hrir_small_v73.mat"])
def test_damaged_hdf5_containers_fail_with_a_value_error(tmp_path, name):
    """A truncated or bit-damaged SOFA / -v7.3 file either still loads (the damage missed every structure the loader walks) or
    is refused with a ValueError (hdf5_min.Hdf5Error is one): no IndexError / struct.error / zlib.error from inside the parser,
    no endless walk (every case finishes in well under a second)."""
    import random
    import time
    raw = open(os.path.join(GOLD, name), "rb").read()
    rng = random.Random(20250311)
    ext = os.path.splitext(name)[1]
    outcomes = {"loaded": 0, "refused": 0}
    worst = 0.0
    for trial in range(120):
        b = bytearray(raw)
        if trial % 3 == 0:
            for _ in range(rng.randint(1, 8)):
                b[rng.randrange(len(b))] = rng.randrange(256)
        elif trial % 3 == 1:
            b = b[:rng.randrange(16, len(b))]
        else:
            p = rng.randrange(len(b) - 64)
            b[p:p + 8] = b"\xff" * 8          # (the "undefined address" of every offset field)
        path = tmp_path / ("damaged%d%s" % (trial, ext))
        path.write_bytes(bytes(b))
        t0 = time.perf_counter()
        try:
            IO.load_hrir_set(str(path))
            outcomes["loaded"] += 1
        except ValueError:
            outcomes["refused"] += 1
        worst = max(worst, time.perf_counter() - t0)
        path.unlink()
    print(name, outcomes, "slowest case %.3f s" % worst)
    assert outcomes["refused"] >= 20 and worst < 5.0


def test_damaged_object_files_fail_with_a_value_error(tmp_path):
    """-v7 files that hold the MIRO instance go through scipy's reader and emagls_amd/mcos.py: whatever either trips over in a
    damaged file surfaces as ValueError.  One process per case: scipy's compiled reader is known to crash on some damaged
    files (3 of 200 in a longer run), which the loader cannot intercept -- such a case is counted, not failed."""
    import random
    import subprocess
    import sys
    import mcosgen
    hL, hR, azi, zen = _hrir_arrays()
    props = dict(irChOne=hL.astype(np.float32), irChTwo=hR.astype(np.float32), azimuth=azi[None, :], elevation=zen[None, :],
                 fs=np.array([[48000.0]]), name="HRIR_L2702")
    f = str(tmp_path / "obj.mat")
    mcosgen.write_object_mat(f, "HRIR_L2702", "miro", props, defaults=dict(radius=np.array([[3.25]])), version=4)
    raw = open(f, "rb").read()
    rng = random.Random(3)
    code = ("import sys, warnings; warnings.simplefilter('ignore'); sys.path.insert(0, %r)\n"
            "from emagls_amd import io as IO\n"
            "try:\n    IO.load_hrir_set(sys.argv[1]); print('loaded')\n"
            "except ValueError:\n    print('refused')\n"
            "except Exception as e:\n    print('OTHER', type(e).__name__, e)\n") % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outcomes = {"loaded": 0, "refused": 0, "crash in scipy": 0}
    for trial in range(12):
        b = bytearray(raw)
        if trial % 3 == 0:
            for _ in range(rng.randint(1, 6)):
                b[rng.randrange(128, len(b))] = rng.randrange(256)
        elif trial % 3 == 1:
            b = b[:rng.randrange(200, len(b))]
        else:
            p = rng.randrange(128, len(b) - 8)
            b[p:p + 4] = b"\xff" * 4
        g = tmp_path / "damaged.mat"
        g.write_bytes(bytes(b))
        r = subprocess.run([sys.executable, "-c", code, str(g)], capture_output=True, text=True, timeout=120)
        out = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
        if r.returncode < 0:
            outcomes["crash in scipy"] += 1
        else:
            assert out in ("loaded", "refused"), (trial, out, r.stderr[-300:])
            outcomes[out] += 1
    print(outcomes)
    assert outcomes["refused"] >= 4
