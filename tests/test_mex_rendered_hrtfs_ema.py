"""The two equatorial-array models of getRenderedHrtfs through the MATLAB gateway ('rendered_hrtfs' of mex/emagls_mex.cpp), with the
harness and the argument layout of tests/test_mex_rendered_hrtfs.py: the model names and the forms of the microphone grid without a
GPU; on the GPU the gateway returns the bits of the Python call."""
import numpy as np
import pytest

from test_mex_decode_group import mex  # noqa: F401  (the fixture that builds and loads the harness)
from test_mex_rendered_hrtfs import FS, args


def mic_azi(M):
    return 2.0 * np.pi * np.arange(M) / M


def test_ema_model_names_and_microphone_grids(mex):  # noqa: F811
    dirs, azi = np.zeros((10, 2)), mic_azi(16)
    for model, nch in (("ema_ch", 9), ("ema_sh", 25)):
        w = np.zeros((16, nch))
        # the names are known and both grid forms pass the gateway: the library's own check answers (nfft odd)
        for mics in (azi, azi.reshape(-1, 1), np.column_stack([azi, np.full(16, np.pi / 2)])):
            with pytest.raises(mex.Error, match="eMagLS:native.*even"):
                mex(1, *args(w, w, model, dirs, order=4, radius=0.042, mics=mics, nfft=33))
        off = np.column_stack([azi, np.full(16, np.pi / 2)])
        off[3, 1] = 1.0
        with pytest.raises(mex.Error, match="zenith at pi/2"):
            mex(1, *args(w, w, model, dirs, order=4, radius=0.042, mics=off, nfft=32))
        with pytest.raises(mex.Error, match="eMagLS:native.*fewer microphones"):
            mex(1, *args(w, w, model, dirs, order=4, radius=0.042, mics=mic_azi(8), nfft=32))
        with pytest.raises(mex.Error, match="eMagLS:native.*channel count"):
            mex(1, *args(np.zeros((16, 16)), np.zeros((16, 16)), model, dirs, order=4, radius=0.042, mics=azi, nfft=32))
    with pytest.raises(mex.Error, match="model must be"):
        mex(1, *args(np.zeros((16, 9)), np.zeros((16, 9)), "ema", dirs, order=4, radius=0.042, mics=azi))
    # the other models still need [n x 2]
    with pytest.raises(mex.Error, match=r"\[n x 2\]"):
        mex(1, *args(np.zeros((16, 16)), np.zeros((16, 16)), "emagls2", dirs, radius=0.042, mics=azi))


@pytest.mark.gpu
@pytest.mark.parametrize("model,nch", [("ema_ch", 9), ("ema_sh", 25)])
def test_ema_models_return_the_bits_of_the_python_call(mex, grids, hrirs, model, nch):  # noqa: F811
    """Order 4, 16 microphones given as azimuths, two filter sets with an HRIR set each, random weights, 301 directions."""
    import emagls_amd as E
    rng = np.random.default_rng(71)
    sub = slice(1, 2702, 9)
    dirs = np.column_stack([grids["azi"][sub], grids["zen"][sub]])
    dirs[0, 1] = np.pi / 2
    D, azi = dirs.shape[0], mic_azi(16)
    wL, wR = rng.standard_normal((2, 128, nch)), rng.standard_normal((2, 128, nch))
    hL = np.stack([hrirs[0][:, sub], 0.5 * hrirs[0][:, sub]])
    hR = np.stack([hrirs[1][:, sub], 2.0 * hrirs[1][:, sub]])
    weights = rng.uniform(0.1, 1.0, D)
    want = E.getRenderedHrtfs(list(wL), list(wR), model, dirs, FS, order=4, micRadius=0.042, micGridAziZenRad=azi, nfft=256, hL=list(hL),
                              hR=list(hR), weights=weights)
    H, mag, ild, ch, cr = mex(5, *args(wL.transpose(1, 2, 0), wR.transpose(1, 2, 0), model, dirs, order=4, radius=0.042, mics=azi, nfft=256,
                                       hL=hL.transpose(1, 2, 0), hR=hR.transpose(1, 2, 0), weights=weights))
    assert H.shape == (129, D, 2, 2) and np.abs(want.H).max() > 0
    assert np.array_equal(H.transpose(3, 0, 1, 2), want.H)
    assert np.array_equal(mag.transpose(2, 0, 1), want.mag_err_db) and np.array_equal(ild.reshape(129, 2).T, want.ild_err_db)
    assert np.array_equal(ch.transpose(2, 0, 1), want.cov_hat) and np.array_equal(cr.transpose(2, 0, 1), want.cov_ref)
