"""The host side of the two equatorial-array models of emagls_rendered_hrtfs (EMAGLS_MODEL_EMA_CH, EMAGLS_MODEL_EMA_SH; DESIGN.md
section 10), through ctypes and without a device: the header and the binding agree on the two values, and every argument rule of the
models is reported before the device is touched.  The argument sets and helpers are those of tests/test_rendered_hrtfs_host.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_rendered_hrtfs_host import call, expect, lib, valid  # noqa: F401  (lib: the fixture that builds and loads the library)

EMA_CH, EMA_SH = 5, 6


def channels(model, order):
    return 2 * order + 1 if model == EMA_CH else (order + 1) ** 2


def valid_ema(model, M=16, order=4, **kw):
    """A complete, valid argument set of one EMA model (zeros: no test here gets as far as the device)."""
    a = valid(2, M=M, order=order, **kw)          # (the emagls2 set: microphones, radius, directions, HRIRs)
    nchan, nsets, ln = channels(model, order), a["nsets"], a["len"]
    return dict(a, model=model, nchan=nchan, wL=np.zeros(nsets * ln * nchan), wR=np.zeros(nsets * ln * nchan))


def test_header_and_binding_define_the_two_models(lib):  # noqa: F811
    from emagls_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "emagls.h")).read(), flags=re.S)
    for k, v in dict(EMA_CH=EMA_CH, EMA_SH=EMA_SH).items():
        assert re.search(r"#define\s+EMAGLS_MODEL_%s\s+%d\b" % (k, v), hdr)
        assert L.MODEL[k.lower()] == v
    assert 4 not in L.MODEL.values() and "ema" not in L.MODEL


@pytest.mark.parametrize("model", [EMA_CH, EMA_SH])
def test_a_valid_call_gets_as_far_as_the_device(lib, model):  # noqa: F811
    from emagls_amd import _lib as L
    n = C.c_int(0)
    if lib.emagls_device_count(C.byref(n)) == L.OK and n.value > 0:
        return      # (with a device the call would run; the rule is about machines without one)
    assert call(lib, valid_ema(model)) == L.ERR_HIP
    assert call(lib, dict(valid_ema(model), mic_zen=None)) == L.ERR_HIP          # the zeniths are not looked at
    assert call(lib, dict(valid_ema(model, M=9), basis=1)) == L.ERR_HIP          # the fewest microphones, complex basis


@pytest.mark.parametrize("model", [EMA_CH, EMA_SH])
def test_null_pointers(lib, model):  # noqa: F811
    from emagls_amd import _lib as L
    for name in ("wL", "wR", "dir_azi", "dir_zen", "mic_azi", "hL", "hR"):
        expect(lib, dict(valid_ema(model), **{name: None}), L.ERR_ARG, b"null pointer")
    expect(lib, dict(valid_ema(model), mic_azi=None, mic_zen=None), L.ERR_ARG, b"null pointer")
    none = dict(valid_ema(model), Hhat=None, mag_err_db=None, ild_err_db=None, cov_hat=None, cov_ref=None)
    expect(lib, none, L.ERR_ARG, b"no output")


def test_orders_above_the_limits_are_unsupported(lib):  # noqa: F811
    from emagls_amd import _lib as L
    expect(lib, valid_ema(EMA_CH, M=64, order=16), L.ERR_UNSUPPORTED, b"order 15")
    expect(lib, valid_ema(EMA_SH, M=64, order=8), L.ERR_UNSUPPORTED, b"order 7")
    expect(lib, dict(valid_ema(EMA_CH), order=-1), L.ERR_ARG, b"negative")
    n = C.c_int(0)
    if not (lib.emagls_device_count(C.byref(n)) == L.OK and n.value > 0):
        assert call(lib, valid_ema(EMA_CH, M=31, order=15)) == L.ERR_HIP         # the limits themselves are inside
        assert call(lib, valid_ema(EMA_SH, M=15, order=7)) == L.ERR_HIP


@pytest.mark.parametrize("model", [EMA_CH, EMA_SH])
@pytest.mark.parametrize("order", [1, 4])
def test_fewer_microphones_than_circular_harmonics(lib, model, order):  # noqa: F811
    from emagls_amd import _lib as L
    expect(lib, valid_ema(model, M=2 * order, order=order), L.ERR_UNSUPPORTED, b"fewer microphones")


def test_channel_count_that_does_not_match_the_model(lib):  # noqa: F811
    from emagls_amd import _lib as L
    expect(lib, dict(valid_ema(EMA_CH), nchan=25), L.ERR_ARG, b"channel count")      # (order+1)^2 is the other model's
    expect(lib, dict(valid_ema(EMA_SH), nchan=9), L.ERR_ARG, b"channel count")
    expect(lib, dict(valid_ema(EMA_SH), nchan=16), L.ERR_ARG, b"channel count")      # nor the microphone count


def test_shared_limits_hold_for_the_ema_models(lib):  # noqa: F811
    from emagls_amd import _lib as L
    for model in (EMA_CH, EMA_SH):
        expect(lib, valid_ema(model, M=65), L.ERR_UNSUPPORTED, b"64 microphones")
        expect(lib, dict(valid_ema(model), mic_radius=0.2), L.ERR_UNSUPPORTED, b"simulation order")
        expect(lib, dict(valid_ema(model), nfft=4096), L.ERR_UNSUPPORTED, b"2048")
        expect(lib, dict(valid_ema(model), basis=2), L.ERR_ARG, b"shDefinition")
    # the order terms of ema_sh are built in a tile of local memory: simulation order 68 (real basis), 47 (complex)
    expect(lib, dict(valid_ema(EMA_SH), mic_radius=0.16), L.ERR_UNSUPPORTED, b"simulation order 68")              # ceil(48000 pi 0.16 / 343) = 71
    expect(lib, dict(valid_ema(EMA_SH), mic_radius=0.12, basis=1), L.ERR_UNSUPPORTED, b"simulation order 47")     # 53


def test_the_scratch_estimate_counts_the_rotation_fit(lib):  # noqa: F811
    """65536 directions at order 7 with a complex basis and a 9 cm array (simulation order 40): the SH matrix of the rotated points
    (64 x 65537 x 264 complex, 17.7 GB), Rot (65536 x 64 x 64 complex, 4.3 GB), conj(Y) of the projected grid twice (3.6 GB) and the
    order terms twice (5.5 GB) make 31 GB.  The refusal is the estimate's, before the device is touched, not an allocation failure."""
    from emagls_amd import _lib as L
    a = valid_ema(EMA_SH, M=16, order=7, D=65536)
    expect(lib, dict(a, basis=1, mic_radius=0.09), L.ERR_UNSUPPORTED, b"24 GiB")


def test_model_4_is_still_unknown(lib):  # noqa: F811
    from emagls_amd import _lib as L
    for m in (4, 7):
        expect(lib, dict(valid_ema(EMA_CH), model=m), L.ERR_ARG, b"unknown model")


def test_python_microphone_grid_forms(lib):  # noqa: F811
    import emagls_amd as E
    from emagls_amd import _lib as L
    dirs, azi = np.zeros((10, 2)), np.linspace(0, 2 * np.pi, 16, endpoint=False)
    kw = dict(order=4, micRadius=0.042)
    for model, nch in (("ema_ch", 9), ("ema_sh", 25)):
        w = np.zeros((16, nch))
        bad = np.column_stack([azi, np.full(16, np.pi / 2)])
        bad[5, 1] = 1.0
        with pytest.raises(ValueError, match="pi/2"):
            E.getRenderedHrtfs(w, w, model, dirs, 48000.0, micGridAziZenRad=bad, **kw)
        with pytest.raises(ValueError, match="pi/2"):
            E.getRenderedHrtfs(w, w, model, dirs, 48000.0, micGridAziZenRad=np.zeros((16, 3)), **kw)
        with pytest.raises(ValueError, match="needs order"):
            E.getRenderedHrtfs(w, w, model, dirs, 48000.0, micRadius=0.042, micGridAziZenRad=azi)
        with pytest.raises(ValueError, match="micRadius"):
            E.getRenderedHrtfs(w, w, model, dirs, 48000.0, order=4)
        # a 1-D azimuth vector, and [M x 2] on the equator, are accepted up to the library call: its own check answers (nfft odd)
        for grid in (azi, np.column_stack([azi, np.full(16, np.pi / 2)])):
            with pytest.raises(L.EmaglsError, match="even"):
                E.getRenderedHrtfs(w, w, model, dirs, 48000.0, micGridAziZenRad=grid, nfft=33, **kw)
    with pytest.raises(ValueError, match="model must be"):
        E.getRenderedHrtfs(np.zeros((16, 9)), np.zeros((16, 9)), "ema", dirs, 48000.0, micGridAziZenRad=azi, **kw)
