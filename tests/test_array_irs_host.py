"""The host side of emagls_array_irs, through ctypes and without a device: the header, the binding and the
built library agree on the entry, every argument rule is reported before the device is touched with its code and message, valid
arguments without a GPU fail on the device (there is no CPU fallback), and the Python wrapper shapes the two forms of `sources`."""
import ctypes as C
import os
import re

import numpy as np
import pytest

NAME = "emagls_array_irs"
ARGS = ["fs", "mic_radius", "order", "mic_azi", "mic_zen", "nmics", "enc", "enc_is_complex", "nch", "nsrc", "comp_ptr", "comp_azi", "comp_zen",
        "comp_delay", "comp_gain", "pre_delay", "nfft", "nr", "out"]


@pytest.fixture(scope="module")
def lib():
    from emagls_amd import build, _lib
    build.build(jobs=4, verbose=False)
    return _lib.load()


def valid(M=6, C_=6, counts=(3, 0, 2), nfft=32, nr=20, enc=False, cplx=False):
    """A complete, valid argument set (arrays of zeros: no test here gets as far as the device)."""
    z = np.zeros
    n = int(sum(counts))
    return dict(fs=16000.0, mic_radius=0.042, order=1, mic_azi=z(M), mic_zen=z(M), nmics=M, enc=z(C_ * M * (2 if cplx else 1)) if enc else None,
                enc_is_complex=int(cplx), nch=C_, nsrc=len(counts), comp_ptr=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                comp_azi=z(n), comp_zen=z(n), comp_delay=z(n), comp_gain=np.ones(n), pre_delay=4.0, nfft=nfft, nr=nr,
                out=z(len(counts) * C_ * nr * (2 if cplx else 1)))


def call(lib, a):
    vals = [a[k].ctypes.data_as(C.c_void_p) if isinstance(a[k], np.ndarray) else a[k] for k in ARGS]
    return lib.emagls_array_irs(*vals)


def expect(lib, a, code, word):
    rc = call(lib, a)
    msg = lib.emagls_last_error()
    assert rc == code, (rc, msg)
    assert word in msg, msg


def test_header_binding_and_library_agree(lib):
    from emagls_amd import _lib as L
    assert hasattr(C.CDLL(L.LIB_PATH), NAME) and NAME in L.SYMBOLS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "emagls.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\((.*?)\)\s*;", hdr, flags=re.S)
    assert m, "not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ARGS

    def ctype(p):
        if "*" in p:
            return C.c_void_p
        return {"int": C.c_int, "int64_t": L.c_i64, "double": C.c_double}[p.split()[0]]

    res, argtypes = L.SYMBOLS[NAME]
    assert res is C.c_int and argtypes == [ctype(p) for p in params]


def test_a_valid_call_gets_as_far_as_the_device(lib):
    """The argument sets the tests below spoil are valid: without a device the call fails on the device, loudly, not on an argument
    and not by computing on the CPU."""
    from emagls_amd import _lib as L
    n = C.c_int(0)
    if lib.emagls_device_count(C.byref(n)) == L.OK and n.value > 0:
        return      # (with a device the call would run; the rule is about machines without one)
    for a in (valid(), valid(C_=4, enc=True), valid(C_=4, enc=True, cplx=True), dict(valid(), comp_delay=None, comp_gain=None),
              dict(valid(nr=5000), nfft=0), valid(counts=(0,))):
        out = a["out"]
        out[:] = 7.0
        assert call(lib, a) == L.ERR_HIP
        assert lib.emagls_last_error() and np.all(out == 7.0)


@pytest.mark.parametrize("name", ["mic_azi", "mic_zen", "comp_ptr", "comp_azi", "comp_zen", "out"])
def test_null_pointers(lib, name):
    from emagls_amd import _lib as L
    expect(lib, dict(valid(), **{name: None}), L.ERR_ARG, b"null pointer")


def test_microphone_and_channel_counts(lib):
    from emagls_amd import _lib as L
    expect(lib, dict(valid(), nmics=0), L.ERR_ARG, b"nmics")
    expect(lib, valid(M=65, C_=65), L.ERR_UNSUPPORTED, b"64 microphones")
    expect(lib, valid(M=6, C_=65, enc=True), L.ERR_UNSUPPORTED, b"64 channels")
    expect(lib, dict(valid(), nch=0), L.ERR_ARG, b"nch")
    expect(lib, valid(M=6, C_=4), L.ERR_ARG, b"nch must equal nmics")


def test_nfft_outside_the_supported_values(lib):
    from emagls_amd import _lib as L
    expect(lib, dict(valid(nr=4), nfft=6), L.ERR_ARG, b"power of two")
    expect(lib, dict(valid(), nfft=48), L.ERR_ARG, b"power of two")
    expect(lib, dict(valid(), nfft=131072), L.ERR_UNSUPPORTED, b"65536")
    expect(lib, dict(valid(nr=4), nfft=4), L.ERR_UNSUPPORTED, b"below 8")
    expect(lib, dict(valid(), nfft=-8), L.ERR_ARG, b"positive")
    expect(lib, dict(valid(nr=40000), nfft=0), L.ERR_UNSUPPORTED, b"65536")      # (the default: the smallest power of two from 2 nr)


def test_nr_above_nfft(lib):
    from emagls_amd import _lib as L
    expect(lib, valid(nfft=32, nr=33), L.ERR_ARG, b"nr exceeds nfft")
    expect(lib, dict(valid(), nr=0), L.ERR_ARG, b"nr")


@pytest.mark.parametrize("bad", [-0.5, np.nan, np.inf])
def test_negative_or_non_finite_delays(lib, bad):
    from emagls_amd import _lib as L
    expect(lib, dict(valid(), pre_delay=float(bad)), L.ERR_ARG, b"pre_delay")
    d = np.zeros(5)
    d[3] = bad
    expect(lib, dict(valid(), comp_delay=d), L.ERR_ARG, b"delays must be non-negative and finite")
    g = np.ones(5)
    g[4] = bad
    if not np.isfinite(bad):
        expect(lib, dict(valid(), comp_gain=g), L.ERR_ARG, b"gains must be finite")


def test_a_delay_that_would_wrap(lib):
    from emagls_amd import _lib as L
    d = np.zeros(5)
    d[2] = 27.5                                             # 27.5 + 4 > 31
    expect(lib, dict(valid(nfft=32), comp_delay=d), L.ERR_ARG, b"would wrap")
    expect(lib, dict(valid(nfft=32), pre_delay=31.5), L.ERR_ARG, b"would wrap")
    d[2] = 27.0                                             # 27 + 4 = nfft - 1: the last sample, allowed
    n = C.c_int(0)
    rc = call(lib, dict(valid(nfft=32), comp_delay=d))
    assert rc == (L.OK if lib.emagls_device_count(C.byref(n)) == L.OK and n.value > 0 else L.ERR_HIP)


def test_comp_ptr_rules(lib):
    from emagls_amd import _lib as L
    expect(lib, dict(valid(), comp_ptr=np.array([1, 3, 3, 5], dtype=np.int64)), L.ERR_ARG, b"start at 0")
    expect(lib, dict(valid(), comp_ptr=np.array([0, 3, 2, 5], dtype=np.int64)), L.ERR_ARG, b"not decrease")
    expect(lib, dict(valid(), nsrc=0), L.ERR_ARG, b"nsrc")


def test_simulation_order_above_85(lib):
    from emagls_amd import _lib as L
    expect(lib, dict(valid(), fs=48000.0, mic_radius=0.2), L.ERR_UNSUPPORTED, b"simulation order")     # ceil(48000 pi 0.2 / 343) = 88
    expect(lib, dict(valid(), order=86), L.ERR_UNSUPPORTED, b"simulation order")
    expect(lib, dict(valid(), order=-1), L.ERR_ARG, b"negative SH order")
    expect(lib, dict(valid(), mic_radius=0.0), L.ERR_ARG, b"must be positive")


def test_the_24_gib_estimate(lib):
    """2^20 sources (all empty: the offsets are the only large array) on 64 microphones at nfft = 65536: 3.5e13 bytes of spectra."""
    from emagls_amd import _lib as L
    Q = 1 << 20
    a = dict(valid(M=64, C_=64, counts=(0,), nfft=65536, nr=8), nsrc=Q, comp_ptr=np.zeros(Q + 1, dtype=np.int64))
    expect(lib, a, L.ERR_UNSUPPORTED, b"24 GiB")
    assert b"split the sources" in lib.emagls_last_error()
    # a bank that fits in the LDS regime does not in the hipFFT regime: 2702 x 32 channels x 65536 x 16 bytes
    expect(lib, dict(valid(M=32, C_=32, counts=(0,), nfft=65536, nr=8), nsrc=2702, comp_ptr=np.zeros(2703, dtype=np.int64)), L.ERR_UNSUPPORTED,
           b"24 GiB")


def test_kernel_time_entry(lib):
    """emagls_array_irs_kernel_time: a null pointer is refused; without a completed call on this thread there is no time to give."""
    from emagls_amd import _lib as L
    assert lib.emagls_array_irs_kernel_time(None) == L.ERR_ARG and b"null pointer" in lib.emagls_last_error()
    ms = C.c_double(-1.0)
    rc = lib.emagls_array_irs_kernel_time(C.byref(ms))
    assert (rc == L.OK and ms.value >= 0.0) or (rc == L.ERR_ARG and b"no emagls_array_irs call" in lib.emagls_last_error())


def test_python_source_forms(lib, monkeypatch):
    """The wrapper's CSR arrays for the two forms of `sources`, seen at the C call (which is replaced: no device here)."""
    import emagls_amd as E
    from emagls_amd import api
    seen = {}

    def arr(p, n, t=C.c_double):
        return None if p is None else np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), shape=(n,)).copy()

    class Fake:
        def emagls_array_irs(self, *a):      # (the arrays are read here: they live as long as the call)
            a = list(a)
            M, Cc, Q = a[5], a[8], a[9]
            a[3], a[4] = arr(a[3], M), arr(a[4], M)
            a[6] = arr(a[6], Cc * M * (2 if a[7] else 1))
            a[10] = arr(a[10], Q + 1, C.c_int64)
            for i in (11, 12, 13, 14):
                a[i] = arr(a[i], int(a[10][-1]))
            seen["a"] = tuple(a)
            return 0

    monkeypatch.setattr(api.L, "load", lambda: Fake())

    mics = np.column_stack([np.linspace(0, 5, 6), np.linspace(0.3, 2.8, 6)])
    dirs = np.array([[0.1, 1.0], [0.2, 1.1], [0.3, 1.2]])
    out = E.getArrayIrs(dirs, 16000.0, 20, 4.0, 0.042, mics)
    a = seen["a"]
    assert out.shape == (3, 20, 6) and out.dtype == np.float64
    assert a[:3] == (16000.0, 0.042, 4) and a[5] == 6 and a[6] is None and a[7:10] == (0, 6, 3) and a[15:18] == (4.0, 0, 20)
    assert list(a[10]) == [0, 1, 2, 3] and a[13] is None and a[14] is None
    assert np.array_equal(a[11], dirs[:, 0]) and np.array_equal(a[12], dirs[:, 1])
    assert np.array_equal(a[3], mics[:, 0]) and np.array_equal(a[4], mics[:, 1])
    assert E.getArrayIrs([[0.1, 1.0], [0.2, 1.1]], 16000.0, 20, 4.0, 0.042, mics).shape == (2, 20, 6)      # rows written as a list
    # a list: 2, 3 and 4 columns and an empty source; the missing delays are 0, the missing gains 1
    srcs = [np.array([[0.1, 1.0, 2.5, 0.5], [0.2, 1.1, 3.0, -2.0]]), np.zeros((0, 2)), np.array([[0.3, 1.2]]), np.array([[0.4, 1.3, 7.25]]), []]
    enc = np.arange(24.0).reshape(4, 6) + 1j
    out = E.getArrayIrs(srcs, 16000.0, 20, 4.5, 0.042, mics, order=2, encoder=enc, nfft=64)
    a = seen["a"]
    assert out.shape == (5, 20, 4) and out.dtype == np.complex128
    assert a[2] == 2 and a[7:10] == (1, 4, 5) and a[15:18] == (4.5, 64, 20)
    assert list(a[10]) == [0, 2, 2, 3, 4, 4]
    assert list(a[11]) == [0.1, 0.2, 0.3, 0.4] and list(a[12]) == [1.0, 1.1, 1.2, 1.3]
    assert list(a[13]) == [2.5, 3.0, 0.0, 7.25] and list(a[14]) == [0.5, -2.0, 1.0, 1.0]
    e = a[6].view(np.complex128).reshape(6, 4).T                                # column-major [C x M], interleaved complex
    assert np.array_equal(e, enc)
    for bad, word in [(np.zeros((3, 3)), "Q x 2"), ([np.zeros((2, 5))], "columns"), ([], "at least one"), ([np.zeros(3)], "columns")]:
        with pytest.raises(ValueError, match=word):
            E.getArrayIrs(bad, 16000.0, 20, 4.0, 0.042, mics)
    with pytest.raises(ValueError, match="numMics x 2"):
        E.getArrayIrs(dirs, 16000.0, 20, 4.0, 0.042, mics[:, 0])
    with pytest.raises(ValueError, match="one column per microphone"):
        E.getArrayIrs(dirs, 16000.0, 20, 4.0, 0.042, mics, encoder=np.zeros((4, 5)))
    with pytest.raises(ValueError, match="irLen"):
        E.getArrayIrs(dirs, 16000.0, 0, 4.0, 0.042, mics)


def test_python_forwards_the_librarys_errors(lib):
    import emagls_amd as E
    mics = np.zeros((6, 2))
    with pytest.raises(E._lib.EmaglsError, match="power of two"):
        E.getArrayIrs(np.zeros((2, 2)), 16000.0, 20, 4.0, 0.042, mics, nfft=48)
    with pytest.raises(E._lib.EmaglsError, match="would wrap"):
        E.getArrayIrs([np.array([[0.0, 1.0, 60.0]])], 16000.0, 20, 4.0, 0.042, mics, nfft=64)
