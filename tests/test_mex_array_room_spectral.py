"""The spectral room through the MATLAB gateway: 'array_room_irs' with wallReflection [6 x P] and airAttenuation, 'shoebox_images', and
'array_irs' with the spectral gain (mex/emagls_mex.cpp, mex/getArrayRoomIrs.m, mex/getShoeboxImages.m, mex/getArrayIrs.m; DESIGN.md
section 13), with the harness of tests/test_mex_decode_group.py.  Without a GPU the argument errors; on the GPU the commands return
the bits of the Python calls."""
import numpy as np
import pytest

from test_mex_decode_group import mex  # noqa: F401  (the fixture that builds and loads the harness)

FS = 16000.0
ROOM, BETA, POS = np.array([3.1, 2.3, 2.7]), np.array([0.9, 0.85, 0.8, 0.75, 0.7, 0.6]), np.array([2.02, 1.41, 1.17])
SRC = np.array([[1.13, 0.71, 1.52]])                                  # room A of tests/test_gpu_array_room_irs.py
P = 513
WALLS = np.linspace(0.95, 0.4, 6)[:, None] * np.linspace(1.0, 0.5, P)[None, :]
AIR = np.linspace(0.0, 0.02, P)


def irs_args(irLen, preDelay, mics, walls=WALLS, air=AIR, src=SRC, order=4, encoder=[], nfft=1024, maxOrder=[], maxDelay=[], room=ROOM, pos=POS,
             radius=0.042):
    return ("array_room_irs", room, walls, src, pos, FS, irLen, preDelay, radius, mics, order, encoder, nfft, maxOrder, maxDelay, air)


def test_argument_errors(mex):  # noqa: F811
    mics = np.zeros((6, 2))
    with pytest.raises(mex.Error, match=r"wallReflection must be \[6 x 513\]"):
        mex(1, *irs_args(120, 4.0, mics, walls=WALLS[:, :100]))
    with pytest.raises(mex.Error, match="wallReflection must have 6 elements"):
        mex(1, *irs_args(120, 4.0, mics, walls=WALLS[:5], air=[]))
    with pytest.raises(mex.Error, match="airAttenuation must have 513 elements"):
        mex(1, *irs_args(120, 4.0, mics, air=AIR[:100]))
    with pytest.raises(mex.Error, match=r"eMagLS:native.*\[-1, 1\]"):           # the library's messages, forwarded
        mex(1, *irs_args(120, 4.0, mics, walls=WALLS * 2))
    with pytest.raises(mex.Error, match="eMagLS:native.*air attenuation must be non-negative"):
        mex(1, *irs_args(120, 4.0, mics, walls=BETA, air=-AIR))
    with pytest.raises(mex.Error, match="eMagLS:native.*would wrap"):
        mex(1, *irs_args(120, 4.0, mics, nfft=[], walls=np.ones((6, 129)), air=[], maxDelay=252.0))       # the default nfft: 256
    with pytest.raises(mex.Error, match="needs 6 arguments"):
        mex(4, "shoebox_images", ROOM, SRC, POS)
    with pytest.raises(mex.Error, match=r"\[numSources x 3\]"):
        mex(4, "shoebox_images", ROOM, SRC[:, :2], POS, FS, 100.0, [])
    with pytest.raises(mex.Error, match="eMagLS:native.*strictly inside the room"):
        mex(4, "shoebox_images", ROOM, np.array([[1.0, 2.5, 1.0]]), POS, FS, 100.0, [])
    comps = np.array([[0.1, 1.0, 3.0, 1.0], [0.2, 1.1, 4.0, 0.5]])
    listed = ("array_irs", np.array([0.0, 2.0]), comps, FS, 120, 4.0, 0.042, mics, 4, [], 256)
    with pytest.raises(mex.Error, match="surfaceReflection and exponents must both be given"):
        mex(1, *listed, np.ones((2, 129)), [], [], [])
    with pytest.raises(mex.Error, match="airAttenuation and pathLength must both be given"):
        mex(1, *listed, [], [], np.zeros(129), [])
    with pytest.raises(mex.Error, match=r"surfaceReflection must be \[numSurfaces x 129\]"):
        mex(1, *listed, np.ones((2, 100)), np.ones((2, 2)), [], [])
    with pytest.raises(mex.Error, match=r"exponents must be \[J x numSurfaces\]"):
        mex(1, *listed, np.ones((2, 129)), np.ones((3, 2)), [], [])
    with pytest.raises(mex.Error, match="exponents must hold integers"):
        mex(1, *listed, np.ones((2, 129)), np.array([[1.0, 0.5], [0.0, 2.0]]), [], [])
    with pytest.raises(mex.Error, match="eMagLS:native.*exponents must be non-negative"):
        mex(1, *listed, np.ones((2, 129)), np.array([[1.0, -1.0], [0.0, 2.0]]), [], [])


@pytest.mark.gpu
@pytest.mark.parametrize("cplx", [False, True])
def test_spectral_room_returns_the_bits_of_the_python_call(mex, cplx):  # noqa: F811
    import emagls_amd as E
    rng = np.random.default_rng(93)
    mics = np.column_stack([rng.uniform(0, 2 * np.pi, 7), np.arccos(rng.uniform(-1, 1, 7))])
    enc = rng.standard_normal((4, 7)) + (1j * rng.standard_normal((4, 7)) if cplx else 0.0)
    want, n = E.getArrayRoomIrs(ROOM, WALLS, SRC, POS, FS, 512, 16.0, 0.042, mics, encoder=enc, nfft=1024, maxDelay=400.0, airAttenuation=AIR,
                                returnCounts=True)
    got, counts = mex(2, *irs_args(512, 16.0, mics, encoder=enc, maxDelay=400.0))                         # [irLen x C x Q]
    assert got.shape == (512, 4, 1) and np.iscomplexobj(got) == cplx and np.abs(want).max() > 0 and list(n) == [136]
    assert np.array_equal(got.transpose(2, 0, 1), want) and list(counts[:, 0]) == [136]
    raw, = mex(1, *irs_args(512, 16.0, mics, walls=BETA, maxOrder=3))                                     # six coefficients with air; the default maxDelay
    assert np.array_equal(raw.transpose(2, 0, 1), E.getArrayRoomIrs(ROOM, BETA, SRC, POS, FS, 512, 16.0, 0.042, mics, nfft=1024, maxOrder=3,
                                                                   airAttenuation=AIR))
    raw, = mex(1, *irs_args(512, 16.0, mics, air=[], maxDelay=400.0))                                     # spectra without air
    assert np.array_equal(raw.transpose(2, 0, 1), E.getArrayRoomIrs(ROOM, WALLS, SRC, POS, FS, 512, 16.0, 0.042, mics, nfft=1024, maxDelay=400.0))


@pytest.mark.gpu
def test_images_and_the_listed_form_return_the_bits_of_the_python_calls(mex):  # noqa: F811
    import emagls_amd as E
    src = np.array([[1.13, 0.71, 1.52], [0.15, 0.2, 2.5], [2.5, 1.0, 1.0]])                               # the second has no image at 100 samples
    cs, es, ps = E.getShoeboxImages(ROOM, src, POS, FS, 100.0)
    ptr, comps, exps, paths = mex(4, "shoebox_images", ROOM, src, POS, FS, 100.0, [])
    assert list(ptr[:, 0]) == [0, 1, 1, 3] and comps.shape == (3, 4) and exps.shape == (3, 6) and paths.shape == (3, 1)
    assert np.array_equal(comps, np.vstack(cs)) and np.array_equal(exps, np.vstack(es)) and np.array_equal(paths[:, 0], np.concatenate(ps))
    mics = np.column_stack([np.linspace(0.1, 6.0, 5), np.linspace(0.3, 2.8, 5)])
    want = E.getArrayIrs(cs, FS, 200, 8.0, 0.042, mics, nfft=1024, surfaceReflection=WALLS, exponents=es, airAttenuation=AIR, pathLength=ps)
    got, = mex(1, "array_irs", ptr, comps, FS, 200, 8.0, 0.042, mics, 4, [], 1024, WALLS, exps, AIR, paths)
    assert got.shape == (200, 5, 3) and want.any() and np.array_equal(got.transpose(2, 0, 1), want)
