"""The host side of emagls_rendered_hrtfs, through ctypes and without a device: the header, the binding and
the built library agree on the entry, every argument rule is reported before the device is touched, and the NumPy statement of the
metrics -- which tests/test_gpu_rendered_hrtfs.py imports from here -- reproduces values computed by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

NAME = "emagls_rendered_hrtfs"
SH, EMAGLS, EMAGLS2, ATF = 0, 1, 2, 3
ARGS = ["model", "wL", "wR", "w_is_complex", "len", "nchan", "nsets", "dir_azi", "dir_zen", "ndirs", "fs", "order", "basis", "mic_radius",
        "mic_azi", "mic_zen", "nmics", "atf", "atf_taps", "nfft", "hL", "hR", "nsamp", "nhrir_sets", "weights", "Hhat", "mag_err_db",
        "ild_err_db", "cov_hat", "cov_ref"]


def rendered_metrics(Hhat, H, weights=None):
    """The metrics of include/emagls.h (emagls_rendered_hrtfs) in NumPy.  Hhat, H: [P x D x 2] complex; weights [D] or None.
    Returns mag_err_db [P x 2], ild_err_db [P], cov_hat [P x 4], cov_ref [P x 4], coherence_hat [P], coherence_ref [P]."""
    Hhat, H = np.asarray(Hhat, dtype=complex), np.asarray(H, dtype=complex)
    D = H.shape[1]
    w = np.full(D, 1.0 / D) if weights is None else np.asarray(weights, dtype=float) / np.sum(weights)
    db = lambda X: 20.0 * np.log10(np.maximum(np.abs(X), np.finfo(float).tiny))   # noqa: E731
    mag = np.einsum("d,kde->ke", w, np.abs(db(Hhat) - db(H)))
    ild = np.abs((db(Hhat[..., 0]) - db(Hhat[..., 1])) - (db(H[..., 0]) - db(H[..., 1]))) @ w

    def cov(X):
        lr = (X[..., 0] * np.conj(X[..., 1])) @ w
        return np.stack([np.abs(X[..., 0]) ** 2 @ w, np.abs(X[..., 1]) ** 2 @ w, lr.real, lr.imag], axis=1)

    ch, cr = cov(Hhat), cov(H)
    coh = lambda c: np.hypot(c[:, 2], c[:, 3]) / np.sqrt(c[:, 0] * c[:, 1])   # noqa: E731
    return dict(mag_err_db=mag, ild_err_db=ild, cov_hat=ch, cov_ref=cr, coherence_hat=coh(ch), coherence_ref=coh(cr))


@pytest.fixture(scope="module")
def lib():
    from emagls_amd import build, _lib
    build.build(jobs=4, verbose=False)
    return _lib.load()


def valid(model=EMAGLS2, M=32, D=10, ln=16, nsets=2, order=4):
    """A complete, valid argument set of one model (arrays of zeros: no test here gets as far as the device)."""
    nchan = {SH: (order + 1) ** 2, EMAGLS: (order + 1) ** 2, EMAGLS2: M, ATF: M}[model]
    z = np.zeros
    a = dict(model=model, wL=z(nsets * ln * nchan), wR=z(nsets * ln * nchan), w_is_complex=0, len=ln, nchan=nchan, nsets=nsets,
             dir_azi=z(D), dir_zen=z(D), ndirs=D, fs=48000.0, order=order, basis=0, mic_radius=0.042, mic_azi=z(M), mic_zen=z(M), nmics=M,
             atf=z(8 * M * D), atf_taps=8, nfft=32, hL=z(nsets * 12 * D), hR=z(nsets * 12 * D), nsamp=12, nhrir_sets=nsets, weights=np.ones(D),
             Hhat=z(2 * nsets * 2 * 17 * D), mag_err_db=z(nsets * 17 * 2), ild_err_db=z(nsets * 17), cov_hat=z(nsets * 17 * 4),
             cov_ref=z(nsets * 17 * 4))
    return a


def call(lib, a):
    vals = [a[k].ctypes.data_as(C.c_void_p) if isinstance(a[k], np.ndarray) else a[k] for k in ARGS]
    return lib.emagls_rendered_hrtfs(*vals)


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
    for k, v in dict(SH=SH, EMAGLS=EMAGLS, EMAGLS2=EMAGLS2, ATF=ATF).items():
        assert re.search(r"#define\s+EMAGLS_MODEL_%s\s+%d\b" % (k, v), hdr)
        assert L.MODEL[k.lower()] == v


def test_a_valid_call_gets_as_far_as_the_device(lib):
    """The argument sets the tests below spoil are valid: without a device the call fails on the device, not on an argument."""
    from emagls_amd import _lib as L
    n = C.c_int(0)
    if lib.emagls_device_count(C.byref(n)) == L.OK and n.value > 0:
        return      # (with a device the call would run; the rule is about machines without one)
    for model in (SH, EMAGLS, EMAGLS2, ATF):
        assert call(lib, valid(model)) == L.ERR_HIP, model


def test_odd_nfft(lib):
    from emagls_amd import _lib as L
    expect(lib, dict(valid(), nfft=33), L.ERR_ARG, b"even")


def test_len_above_nfft(lib):
    from emagls_amd import _lib as L
    expect(lib, dict(valid(ln=40), nfft=32), L.ERR_ARG, b"len exceeds nfft")
    expect(lib, dict(valid(), nsamp=33), L.ERR_ARG, b"nsamp exceeds nfft")
    expect(lib, dict(valid(ATF), atf_taps=34), L.ERR_ARG, b"atf_taps exceeds nfft")


def test_nfft_outside_the_supported_range(lib):
    from emagls_amd import _lib as L
    expect(lib, dict(valid(ln=4), nfft=6), L.ERR_UNSUPPORTED, b"below 8")
    expect(lib, dict(valid(), nfft=4096), L.ERR_UNSUPPORTED, b"2048")


def test_unknown_model(lib):
    from emagls_amd import _lib as L
    for m in (-1, 4):
        expect(lib, dict(valid(), model=m), L.ERR_ARG, b"unknown model")


def test_emagls_order_5_is_unsupported(lib):
    from emagls_amd import _lib as L
    expect(lib, valid(EMAGLS, M=64, order=5), L.ERR_UNSUPPORTED, b"order 4")
    expect(lib, valid(EMAGLS, M=20, order=4), L.ERR_UNSUPPORTED, b"fewer microphones")
    expect(lib, valid(SH, order=16), L.ERR_UNSUPPORTED, b"15")


def test_65_microphones_are_unsupported(lib):
    from emagls_amd import _lib as L
    expect(lib, valid(EMAGLS2, M=65), L.ERR_UNSUPPORTED, b"64 microphones")
    expect(lib, valid(ATF, M=65), L.ERR_UNSUPPORTED, b"64 microphones")


def test_simulation_order_above_85(lib):
    from emagls_amd import _lib as L
    expect(lib, dict(valid(), mic_radius=0.2), L.ERR_UNSUPPORTED, b"simulation order")     # ceil(48000 pi 0.2 / 343) = 88


def test_negative_weights(lib):
    from emagls_amd import _lib as L
    w = np.ones(10)
    w[3] = -0.5
    expect(lib, dict(valid(), weights=w), L.ERR_ARG, b"non-negative")
    expect(lib, dict(valid(), weights=np.zeros(10)), L.ERR_ARG, b"all be zero")
    w[3] = np.nan
    expect(lib, dict(valid(), weights=w), L.ERR_ARG, b"non-negative")


def test_hrir_set_count_neither_one_nor_nsets(lib):
    from emagls_amd import _lib as L
    for n in (0, 3):
        expect(lib, dict(valid(nsets=2), nhrir_sets=n), L.ERR_ARG, b"1 or nsets")


def test_channel_count_that_does_not_match_the_model(lib):
    from emagls_amd import _lib as L
    expect(lib, dict(valid(EMAGLS), nchan=16), L.ERR_ARG, b"channel count")
    expect(lib, dict(valid(SH, order=2), nchan=25), L.ERR_ARG, b"channel count")


@pytest.mark.parametrize("model,required", [(SH, ["wL", "wR", "dir_azi", "dir_zen"]),
                                            (EMAGLS, ["wL", "wR", "dir_azi", "dir_zen", "mic_azi", "mic_zen"]),
                                            (EMAGLS2, ["wL", "wR", "dir_azi", "dir_zen", "mic_azi", "mic_zen"]),
                                            (ATF, ["wL", "wR", "atf"])])
def test_null_pointer_for_every_required_argument(lib, model, required):
    from emagls_amd import _lib as L
    for name in required:
        expect(lib, dict(valid(model), **{name: None}), L.ERR_ARG, b"null pointer")
    # the metrics need both reference HRIRs; a call that asks for no output at all is an error too
    expect(lib, dict(valid(model), hL=None), L.ERR_ARG, b"null pointer")
    expect(lib, dict(valid(model), hR=None), L.ERR_ARG, b"null pointer")
    none = dict(valid(model), Hhat=None, mag_err_db=None, ild_err_db=None, cov_hat=None, cov_ref=None)
    expect(lib, none, L.ERR_ARG, b"no output")


def test_python_argument_errors(lib):
    import emagls_amd as E
    w, dirs = np.zeros((16, 4)), np.zeros((10, 2))
    with pytest.raises(ValueError, match="model must be"):
        E.getRenderedHrtfs(w, w, "ema", dirs, 48000.0, order=1)
    with pytest.raises(ValueError, match="needs order"):
        E.getRenderedHrtfs(w, w, "sh", dirs, 48000.0)
    with pytest.raises(ValueError, match="micRadius"):
        E.getRenderedHrtfs(w, w, "emagls2", dirs, 48000.0)
    with pytest.raises(ValueError, match="equal shape"):
        E.getRenderedHrtfs(w, w[:8], "sh", dirs, 48000.0, order=1)
    with pytest.raises(ValueError, match="go together"):
        E.getRenderedHrtfs(w, w, "sh", dirs, 48000.0, order=1, hL=np.zeros((8, 10)))
    with pytest.raises(ValueError, match="nothing to compute"):
        E.getRenderedHrtfs(w, w, "sh", dirs, 48000.0, order=1, returnResponse=False)
    with pytest.raises(E._lib.EmaglsError, match="even"):
        E.getRenderedHrtfs(w, w, "sh", dirs, 48000.0, order=1, nfft=31)


def test_numpy_metrics_reproduce_hand_computed_values():
    """2 bins, 3 directions.  Bin 0: magnitudes are powers of ten, so every dB term is a multiple of 20.  Bin 1: Hhat == H with a
    zero in it -- the clamp at DBL_MIN makes both logarithms equal, no error and no NaN."""
    Hhat = np.zeros((2, 3, 2), dtype=complex)
    H = np.zeros((2, 3, 2), dtype=complex)
    Hhat[0, :, 0], Hhat[0, :, 1] = [10, 1j, 0.1], [1, 1, 1]
    H[0, :, 0], H[0, :, 1] = [1, 1, 1], [1, 10, 1]
    H[1, :, 0], H[1, :, 1] = [0, 2j, 1], [2, 2, -1]
    Hhat[1] = H[1]
    m = rendered_metrics(Hhat, H)
    # bin 0, left: |20|, |0|, |-20| dB; right: 0, |-20|, 0; ILD hat (20, 0, -20) against ILD ref (0, -20, 0): 20, 20, |-20|
    assert np.allclose(m["mag_err_db"], [[40 / 3, 20 / 3], [0, 0]], rtol=1e-14, atol=1e-14)
    assert np.allclose(m["ild_err_db"], [20, 0], rtol=1e-14, atol=1e-14)
    assert np.allclose(m["cov_hat"], [[101.01 / 3, 1, 10.1 / 3, 1 / 3], [5 / 3, 3, -1 / 3, 4 / 3]], rtol=1e-14)
    assert np.allclose(m["cov_ref"], [[1, 34, 4, 0], [5 / 3, 3, -1 / 3, 4 / 3]], rtol=1e-14)
    assert np.allclose(m["coherence_ref"], [4 / np.sqrt(34), np.sqrt(17) / 3 / np.sqrt(5)], rtol=1e-14)
    # weights (1, 2, 1), not normalised by the caller: (1/4, 1/2, 1/4)
    mw = rendered_metrics(Hhat, H, [1, 2, 1])
    assert np.allclose(mw["mag_err_db"], [[10, 10], [0, 0]], rtol=1e-14, atol=1e-14)
    assert np.allclose(mw["ild_err_db"], [20, 0], rtol=1e-14, atol=1e-14)
    assert np.allclose(mw["cov_ref"][0], [1, 50.5, 5.5, 0], rtol=1e-14)
    assert np.all(np.isfinite(m["mag_err_db"])) and np.all(np.isfinite(m["ild_err_db"]))
