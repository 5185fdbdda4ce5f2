"""The shoebox room through the MATLAB gateway: 'shoebox_components' and 'array_room_irs' (mex/emagls_mex.cpp,
mex/getShoeboxComponents.m, mex/getArrayRoomIrs.m), with the harness of tests/test_mex_decode_group.py.  The arguments cross the
gateway as the two wrappers lay them: positions [numSources x 3], [] for an absent encoder and for the defaults.  Without a GPU
the argument errors; on the GPU both commands return the bits of the Python calls."""
import numpy as np
import pytest

from test_mex_decode_group import mex  # noqa: F401  (the fixture that builds and loads the harness)

FS = 16000.0
ROOM, BETA, POS = np.array([3.1, 2.3, 2.7]), np.array([0.9, 0.85, 0.8, 0.75, 0.7, 0.6]), np.array([2.02, 1.41, 1.17])
SRC = np.array([[1.13, 0.71, 1.52], [2.5, 1.0, 1.0], [0.15, 0.2, 2.5]])


def comp_args(maxDelay, src=SRC, maxOrder=[], room=ROOM, beta=BETA, pos=POS):
    return ("shoebox_components", room, beta, src, pos, FS, maxDelay, maxOrder)


def irs_args(irLen, preDelay, mics, src=SRC, order=4, encoder=[], nfft=[], maxOrder=[], maxDelay=[], room=ROOM, beta=BETA, pos=POS, radius=0.042):
    return ("array_room_irs", room, beta, src, pos, FS, irLen, preDelay, radius, mics, order, encoder, nfft, maxOrder, maxDelay)


def test_argument_errors(mex):  # noqa: F811
    mics = np.zeros((6, 2))
    with pytest.raises(mex.Error, match="needs 7 arguments"):
        mex(2, "shoebox_components", ROOM, BETA, SRC)
    with pytest.raises(mex.Error, match="needs 14 arguments"):
        mex(1, "array_room_irs", ROOM, BETA, SRC, POS, FS, 120.0, 4.0)
    for make in (lambda **k: comp_args(100.0, **k), lambda **k: irs_args(120, 4.0, mics, **k)):
        with pytest.raises(mex.Error, match="must have 3 elements"):
            mex(1, *make(room=ROOM[:2]))
        with pytest.raises(mex.Error, match="must have 3 elements"):
            mex(1, *make(pos=np.zeros(4)))
        with pytest.raises(mex.Error, match="must have 6 elements"):
            mex(1, *make(beta=BETA[:5]))
        with pytest.raises(mex.Error, match=r"\[numSources x 3\]"):
            mex(1, *make(src=SRC[:, :2]))
        with pytest.raises(mex.Error, match="eMagLS:native.*strictly inside the room"):           # the library's messages, forwarded
            mex(1, *make(src=np.array([[1.0, 2.5, 1.0]])))
        with pytest.raises(mex.Error, match=r"eMagLS:native.*\[-1, 1\]"):
            mex(1, *make(beta=BETA * 2))
        with pytest.raises(mex.Error, match="eMagLS:native.*max_order"):
            mex(1, *make(maxOrder=-3))
    with pytest.raises(mex.Error, match="eMagLS:native.*max_delay must be positive"):
        mex(2, *comp_args(0.0))
    with pytest.raises(mex.Error, match="eMagLS:native.*2\\^28"):
        mex(2, *comp_args(1e9))
    with pytest.raises(mex.Error, match=r"\[n x 2\]"):
        mex(1, *irs_args(120, 4.0, np.zeros((6, 3))))
    with pytest.raises(mex.Error, match="one column per microphone"):
        mex(1, *irs_args(120, 4.0, mics, encoder=np.zeros((4, 5))))
    with pytest.raises(mex.Error, match="eMagLS:native.*would wrap"):
        mex(1, *irs_args(120, 4.0, mics, maxDelay=252.0))
    with pytest.raises(mex.Error, match="eMagLS:native.*sphere must lie inside the room"):
        mex(1, *irs_args(120, 4.0, mics, pos=np.array([2.02, 1.41, 0.03])))
    with pytest.raises(mex.Error, match="eMagLS:native.*power of two"):
        mex(1, *irs_args(120, 4.0, mics, nfft=48))


@pytest.mark.gpu
def test_shoebox_components_returns_the_bits_of_the_python_call(mex):  # noqa: F811
    """Three positions at 100 samples, the third without a component; and an order limit."""
    import emagls_amd as E
    for md, mo in ((100.0, None), (400.0, 2)):
        want = E.getShoeboxComponents(ROOM, BETA, SRC, POS, FS, md, maxOrder=mo)
        ptr, comps = mex(2, *comp_args(md, maxOrder=[] if mo is None else mo))
        assert ptr.shape == (4, 1) and list(ptr[:, 0]) == list(np.concatenate([[0], np.cumsum([w.shape[0] for w in want])]))
        assert comps.shape == (int(ptr[-1, 0]), 4) and np.array_equal(comps, np.vstack(want))
    assert want[0].shape[0] == 25 and E.getShoeboxComponents(ROOM, BETA, SRC, POS, FS, 100.0)[2].shape[0] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("cplx", [False, True])
def test_array_room_irs_returns_the_bits_of_the_python_call(mex, cplx):  # noqa: F811
    import emagls_amd as E
    rng = np.random.default_rng(92)
    mics = np.column_stack([rng.uniform(0, 2 * np.pi, 7), np.arccos(rng.uniform(-1, 1, 7))])
    enc = rng.standard_normal((4, 7)) + (1j * rng.standard_normal((4, 7)) if cplx else 0.0)
    want, n = E.getArrayRoomIrs(ROOM, BETA, SRC, POS, FS, 200, 6.25, 0.042, mics, order=2, encoder=enc, nfft=512, maxDelay=100.0, returnCounts=True)
    got, counts = mex(2, *irs_args(200, 6.25, mics, order=2, encoder=enc, nfft=512, maxDelay=100.0))      # [irLen x C x Q]
    assert got.shape == (200, 4, 3) and np.iscomplexobj(got) == cplx and np.abs(want).max() > 0
    assert np.array_equal(got.transpose(2, 0, 1), want) and list(counts[:, 0]) == list(n) and n[2] == 0
    raw, = mex(1, *irs_args(200, 6.25, mics, order=2, maxOrder=3))                                          # the defaults: nfft 512, maxDelay 192.75
    assert np.array_equal(raw.transpose(2, 0, 1), E.getArrayRoomIrs(ROOM, BETA, SRC, POS, FS, 200, 6.25, 0.042, mics, order=2, maxOrder=3))
