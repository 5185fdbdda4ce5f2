"""Point sources through the MATLAB gateway: 'array_irs' with a distance per component, 'shoebox_components' with its third output and
'array_room_irs' with waveModel (mex/emagls_mex.cpp, mex/getArrayIrs.m, mex/getShoeboxComponents.m, mex/getArrayRoomIrs.m; DESIGN.md
section 14), with the harness of tests/test_mex_decode_group.py.  Without a GPU the argument errors; on the GPU the commands return
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


def room_args(irLen, preDelay, mics, walls=BETA, air=[], model="pointSource", nfft=1024, maxDelay=[]):
    return ("array_room_irs", ROOM, walls, SRC, POS, FS, irLen, preDelay, 0.042, mics, 4, [], nfft, [], maxDelay, air, model)


def test_argument_errors(mex):  # noqa: F811
    mics = np.zeros((6, 2))
    with pytest.raises(mex.Error, match="unknown waveModel"):
        mex(1, *room_args(120, 4.0, mics, model="sphericalWave"))
    with pytest.raises(mex.Error, match=r"wallReflection must be \[6 x 513\]"):
        mex(1, *room_args(120, 4.0, mics, walls=WALLS[:, :100]))
    comps = np.array([[0.1, 1.0, 3.0, 1.0], [0.2, 1.1, 4.0, 0.5]])
    listed = ("array_irs", np.array([0.0, 2.0]), comps, FS, 120, 4.0, 0.042, mics, 4, [], 256, [], [], [], [])
    with pytest.raises(mex.Error, match="distance must have one element per component"):
        mex(1, *listed, np.array([1.0]))
    with pytest.raises(mex.Error, match="eMagLS:native.*greater than mic_radius"):           # the library's message, forwarded
        mex(1, *listed, np.array([1.0, 0.042]))
    with pytest.raises(mex.Error, match="eMagLS:native.*greater than mic_radius"):
        mex(1, *listed, np.array([np.inf, 1.0]))


@pytest.mark.gpu
def test_the_three_commands_return_the_bits_of_the_python_calls(mex):  # noqa: F811
    import emagls_amd as E
    rng = np.random.default_rng(94)
    mics = np.column_stack([rng.uniform(0, 2 * np.pi, 7), np.arccos(rng.uniform(-1, 1, 7))])
    ptr, comps, dists = mex(3, "shoebox_components", ROOM, BETA, SRC, POS, FS, 400.0, [])
    (want_c,), (want_d,) = E.getShoeboxComponents(ROOM, BETA, SRC, POS, FS, 400.0, returnDistance=True)
    assert list(ptr[:, 0]) == [0, 136] and np.array_equal(comps, want_c) and np.array_equal(dists[:, 0], want_d)
    got, = mex(1, "array_irs", ptr, comps, FS, 512, 16.0, 0.042, mics, 4, [], 1024, [], [], [], [], dists)
    want = E.getArrayIrs([want_c], FS, 512, 16.0, 0.042, mics, nfft=1024, distance=[want_d])
    assert got.shape == (512, 7, 1) and np.abs(want).max() > 0 and np.array_equal(got.transpose(2, 0, 1), want)
    room, counts = mex(2, *room_args(512, 16.0, mics, maxDelay=400.0))
    assert np.array_equal(room, got) and list(counts[:, 0]) == [136]                               # and the fused call, flat walls
    room, = mex(1, *room_args(512, 16.0, mics, walls=WALLS, air=AIR, maxDelay=400.0))
    assert np.array_equal(room.transpose(2, 0, 1), E.getArrayRoomIrs(ROOM, WALLS, SRC, POS, FS, 512, 16.0, 0.042, mics, nfft=1024, maxDelay=400.0,
                                                                    airAttenuation=AIR, waveModel="pointSource"))
    plane, = mex(1, *room_args(512, 16.0, mics, model="planeWave", maxDelay=400.0))
    assert np.array_equal(plane.transpose(2, 0, 1), E.getArrayRoomIrs(ROOM, BETA, SRC, POS, FS, 512, 16.0, 0.042, mics, nfft=1024, maxDelay=400.0))
