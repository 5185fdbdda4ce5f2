"""getArrayIrs through the MATLAB gateway: 'array_irs' (mex/emagls_mex.cpp, mex/getArrayIrs.m), with the harness of
tests/test_mex_decode_group.py.  The sources cross the gateway as mex/getArrayIrs.m lays them: zero-based offsets and one [J x 4]
array of components.  Without a GPU the argument errors; on the GPU the gateway returns the bits of the Python call."""
import numpy as np
import pytest

from test_mex_decode_group import mex  # noqa: F401  (the fixture that builds and loads the harness)

FS = 16000.0


def args(sources, irLen, preDelay, mics, order=4, encoder=[], nfft=[], radius=0.042):
    """What mex/getArrayIrs.m hands over for a list of [J x 4] sources."""
    ptr = np.concatenate([[0.0], np.cumsum([s.shape[0] for s in sources])])
    return ("array_irs", ptr, np.vstack(sources), FS, irLen, preDelay, radius, mics, order, encoder, nfft)


def test_array_irs_argument_errors(mex):  # noqa: F811
    mics = np.zeros((6, 2))
    src = [np.array([[0.1, 1.0, 0.0, 1.0], [0.2, 1.1, 3.5, 0.5]]), np.zeros((0, 4)), np.array([[0.3, 1.2, 0.0, 1.0]])]
    with pytest.raises(mex.Error, match="needs 10 arguments"):
        mex(1, "array_irs", np.array([0.0, 1.0]), np.zeros((1, 4)), FS)
    a = list(args(src, 20, 4.0, mics))
    with pytest.raises(mex.Error, match="numSources \\+ 1"):
        mex(1, *(a[:1] + [np.array([0.0])] + a[2:]))
    with pytest.raises(mex.Error, match="integers"):
        mex(1, *(a[:1] + [np.array([0.0, 1.5, 2.0, 3.0])] + a[2:]))
    with pytest.raises(mex.Error, match="end at the number of rows"):
        mex(1, *(a[:1] + [np.array([0.0, 2.0, 2.0, 4.0])] + a[2:]))
    with pytest.raises(mex.Error, match=r"\[J x 4\]"):
        mex(1, *(a[:2] + [np.zeros((3, 3))] + a[3:]))
    with pytest.raises(mex.Error, match=r"\[n x 2\]"):
        mex(1, *args(src, 20, 4.0, np.zeros((6, 3))))
    with pytest.raises(mex.Error, match="one column per microphone"):
        mex(1, *args(src, 20, 4.0, mics, encoder=np.zeros((4, 5))))
    with pytest.raises(mex.Error, match="eMagLS:native.*power of two"):                   # the library's messages, forwarded
        mex(1, *args(src, 20, 4.0, mics, nfft=48))
    with pytest.raises(mex.Error, match="eMagLS:native.*would wrap"):
        mex(1, *args(src, 20, 60.0, mics, nfft=64))
    with pytest.raises(mex.Error, match="eMagLS:native.*not decrease"):
        mex(1, *(a[:1] + [np.array([0.0, 2.0, 1.0, 3.0])] + a[2:]))
    with pytest.raises(mex.Error, match="eMagLS:native.*64 microphones"):
        mex(1, *args(src, 20, 4.0, np.zeros((65, 2))))


@pytest.mark.gpu
@pytest.mark.parametrize("cplx", [False, True])
def test_array_irs_returns_the_bits_of_the_python_call(mex, cplx):  # noqa: F811
    """7 microphones behind a [4 x 7] encoder; sources of 40, 0, 1 and 17 components (both kernel forms), fractional delays."""
    import emagls_amd as E
    rng = np.random.default_rng(91)
    mics = np.column_stack([rng.uniform(0, 2 * np.pi, 7), np.arccos(rng.uniform(-1, 1, 7))])
    src = [np.column_stack([rng.uniform(0, 2 * np.pi, J), np.arccos(rng.uniform(-1, 1, J)), rng.uniform(0, 30, J), rng.standard_normal(J)])
           for J in (40, 0, 1, 17)]
    enc = rng.standard_normal((4, 7)) + (1j * rng.standard_normal((4, 7)) if cplx else 0.0)
    want = E.getArrayIrs(src, FS, 90, 6.25, 0.042, mics, order=2, encoder=enc, nfft=128)          # [Q x irLen x C]
    got, = mex(1, *args(src, 90, 6.25, mics, order=2, encoder=enc, nfft=128))                      # [irLen x C x Q]
    assert got.shape == (90, 4, 4) and np.iscomplexobj(got) == cplx and np.abs(want).max() > 0
    assert np.array_equal(got.transpose(2, 0, 1), want)
    raw, = mex(1, *args(src, 90, 6.25, mics, order=2))                                             # no encoder, the default nfft (256)
    assert np.array_equal(raw.transpose(2, 0, 1), E.getArrayIrs(src, FS, 90, 6.25, 0.042, mics, order=2))
