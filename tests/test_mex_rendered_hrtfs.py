"""getRenderedHrtfs through the MATLAB gateway: 'rendered_hrtfs' (mex/emagls_mex.cpp, mex/getRenderedHrtfs.m), compiled against the
stand-in mex.h (tests/mexstub/) with the harness of tests/test_mex_decode_group.py.  Sets run along the last dimension on the MATLAB
side: the argument errors without a GPU; on the GPU the gateway returns the bits of the C call."""
import numpy as np
import pytest

from test_mex_decode_group import mex  # noqa: F401  (the fixture that builds and loads the harness)

FS = 48000.0


def args(wL, wR, model, dirs, order=[], radius=[], mics=[], atf=[], nfft=[], basis="real", hL=[], hR=[], weights=[], response=True):
    return ("rendered_hrtfs", wL, wR, model, dirs, FS, order, radius, mics, atf, nfft, basis, hL, hR, weights, response)


def test_rendered_hrtfs_argument_errors(mex):  # noqa: F811
    w, dirs, mics = np.zeros((16, 32)), np.zeros((10, 2)), np.zeros((32, 2))
    with pytest.raises(mex.Error, match="needs 15 arguments"):
        mex(1, "rendered_hrtfs", w, w, "emagls2", dirs, FS)
    with pytest.raises(mex.Error, match="equal size"):
        mex(1, *args(w, np.zeros((16, 31)), "emagls2", dirs, radius=0.042, mics=mics))
    with pytest.raises(mex.Error, match="model must be"):
        mex(1, *args(w, w, "ema", dirs, radius=0.042, mics=mics))
    with pytest.raises(mex.Error, match=r"\[n x 2\]"):
        mex(1, *args(w, w, "emagls2", np.zeros((10, 3)), radius=0.042, mics=mics))
    with pytest.raises(mex.Error, match="go together"):
        mex(1, *args(w, w, "emagls2", dirs, radius=0.042, mics=mics, hL=np.zeros((8, 10))))
    with pytest.raises(mex.Error, match="equal size"):
        mex(1, *args(w, w, "emagls2", dirs, radius=0.042, mics=mics, hL=np.zeros((8, 10)), hR=np.zeros((8, 9))))
    with pytest.raises(mex.Error, match="one element per direction"):
        mex(1, *args(w, w, "emagls2", dirs, radius=0.042, mics=mics, hL=np.zeros((8, 10)), hR=np.zeros((8, 10)), weights=np.ones(9)))
    with pytest.raises(mex.Error, match="eMagLS:native.*even"):                     # the library's message, forwarded
        mex(1, *args(w, w, "emagls2", dirs, radius=0.042, mics=mics, nfft=33))
    with pytest.raises(mex.Error, match="eMagLS:native.*64 microphones"):
        mex(1, *args(np.zeros((16, 65)), np.zeros((16, 65)), "emagls2", dirs, radius=0.042, mics=np.zeros((65, 2))))
    with pytest.raises(mex.Error, match="eMagLS:native.*no output"):
        mex(1, *args(w, w, "emagls2", dirs, radius=0.042, mics=mics, response=False))


@pytest.mark.gpu
def test_rendered_hrtfs_returns_the_bits_of_the_c_call(mex, grids, hrirs):  # noqa: F811
    """emagls2, 32 microphones, two filter sets with an HRIR set each, random weights."""
    import emagls_amd as E
    rng = np.random.default_rng(51)
    sub = slice(1, 2702, 9)
    dirs = np.column_stack([grids["azi"][sub], grids["zen"][sub]])
    mics = np.column_stack([grids["mic_azi"], grids["mic_zen"]])
    D = dirs.shape[0]
    wL, wR = rng.standard_normal((2, 128, 32)), rng.standard_normal((2, 128, 32))
    hL = np.stack([hrirs[0][:, sub], 0.5 * hrirs[0][:, sub]])
    hR = np.stack([hrirs[1][:, sub], 2.0 * hrirs[1][:, sub]])
    weights = rng.uniform(0.1, 1.0, D)
    want = E.getRenderedHrtfs(list(wL), list(wR), "emagls2", dirs, FS, micRadius=0.042, micGridAziZenRad=mics, nfft=256, hL=list(hL), hR=list(hR),
                              weights=weights)
    H, mag, ild, ch, cr = mex(5, *args(wL.transpose(1, 2, 0), wR.transpose(1, 2, 0), "emagls2", dirs, radius=0.042, mics=mics, nfft=256,
                                       hL=hL.transpose(1, 2, 0), hR=hR.transpose(1, 2, 0), weights=weights))
    assert H.shape == (129, D, 2, 2) and mag.shape == (129, 2, 2) and ild.shape[0] == 129 and ch.shape == cr.shape == (129, 4, 2)
    assert np.array_equal(H.transpose(3, 0, 1, 2), want.H)
    assert np.array_equal(mag.transpose(2, 0, 1), want.mag_err_db) and np.array_equal(ild.reshape(129, 2).T, want.ild_err_db)
    assert np.array_equal(ch.transpose(2, 0, 1), want.cov_hat) and np.array_equal(cr.transpose(2, 0, 1), want.cov_ref)
