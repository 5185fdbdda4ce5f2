"""Directive sources through the MATLAB gateway: 'array_irs' with emission, sourceOrientation and directivity, 'shoebox_components' and
'shoebox_images' with their further output, 'array_room_irs' with sourceOrientation and directivity (mex/emagls_mex.cpp,
mex/getArrayIrs.m, mex/getShoeboxComponents.m, mex/getShoeboxImages.m, mex/getArrayRoomIrs.m, mex/emaglsDirectiveArgs.m; DESIGN.md
section 15), with the harness of tests/test_mex_decode_group.py.  Without a GPU the argument errors; on the GPU the commands return the
bits of the Python calls.  The gateway takes the rotations as [Q x 9] rows and the coefficients as [Q Kd x P] rows, as the wrappers
build them."""
import numpy as np
import pytest

from test_mex_decode_group import mex  # noqa: F401  (the fixture that builds and loads the harness)

FS = 16000.0
ROOM, BETA, POS = np.array([3.1, 2.3, 2.7]), np.array([0.9, 0.85, 0.8, 0.75, 0.7, 0.6]), np.array([2.02, 1.41, 1.17])
SRC = np.array([[1.13, 0.71, 1.52]])                                  # room A of tests/test_gpu_array_room_irs.py
P = 513
WALLS = np.linspace(0.95, 0.4, 6)[:, None] * np.linspace(1.0, 0.5, P)[None, :]
AIR = np.linspace(0.0, 0.02, P)


def room_args(irLen, preDelay, mics, walls=BETA, air=[], model="planeWave", nfft=1024, maxDelay=[], rot=[], coef=[]):
    return ("array_room_irs", ROOM, walls, SRC, POS, FS, irLen, preDelay, 0.042, mics, 4, [], nfft, [], maxDelay, air, model, rot, coef)


def rows(coef):
    """[Q x Kd x P] as the gateway's [Q Kd x P]."""
    return np.ascontiguousarray(coef.reshape(-1, coef.shape[2]))


def test_argument_errors(mex):  # noqa: F811
    mics = np.zeros((6, 2))
    comps = np.array([[0.1, 1.0, 3.0, 1.0], [0.2, 1.1, 4.0, 0.5]])
    emit = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    listed = ("array_irs", np.array([0.0, 2.0]), comps, FS, 120, 4.0, 0.042, mics, 4, [], 256, [], [], [], [], [])
    coef = np.ones((4, 129))
    with pytest.raises(mex.Error, match="come with a directivity"):
        mex(1, *listed, emit, [], [])
    with pytest.raises(mex.Error, match=r"needs emission \[J x 3\]"):
        mex(1, *listed, [], [], coef)
    with pytest.raises(mex.Error, match=r"needs emission \[J x 3\]"):
        mex(1, *listed, emit[:1], [], coef)
    with pytest.raises(mex.Error, match="not a square"):
        mex(1, *listed, emit, [], np.ones((5, 129)))
    with pytest.raises(mex.Error, match=r"directivity must be \[numSources\*Kd x 129\]"):
        mex(1, *listed, emit, [], np.ones((4, 100)))
    with pytest.raises(mex.Error, match=r"sourceOrientation must be \[numSources x 9\]"):
        mex(1, *listed, emit, np.eye(3), coef)
    with pytest.raises(mex.Error, match="eMagLS:native.*proper rotation"):                   # the library's messages, forwarded
        mex(1, *listed, emit, np.diag([1.0, -1.0, 1.0]).reshape(1, 9), coef)
    with pytest.raises(mex.Error, match="eMagLS:native.*unit length"):
        mex(1, *listed, 2.0 * emit, [], coef)
    with pytest.raises(mex.Error, match="eMagLS:native.*above 8"):
        mex(1, *listed, emit, [], np.ones((100, 129)))
    with pytest.raises(mex.Error, match="sourceOrientation comes with a directivity"):
        mex(1, *room_args(120, 4.0, mics, rot=np.eye(3).reshape(1, 9)))
    with pytest.raises(mex.Error, match="not a square"):
        mex(1, *room_args(120, 4.0, mics, coef=np.ones((3, P))))
    with pytest.raises(mex.Error, match="eMagLS:native.*finite"):
        mex(1, *room_args(120, 4.0, mics, coef=np.full((4, P), np.nan)))


@pytest.mark.gpu
def test_the_commands_return_the_bits_of_the_python_calls(mex):  # noqa: F811
    import emagls_amd as E
    rng = np.random.default_rng(95)
    mics = np.column_stack([rng.uniform(0, 2 * np.pi, 7), np.arccos(rng.uniform(-1, 1, 7))])
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    R = (q if np.linalg.det(q) > 0 else q * np.array([1.0, 1.0, -1.0]))[None]
    coef = rng.standard_normal((1, 9, P)) + 1j * rng.standard_normal((1, 9, P))
    real_coef = np.ascontiguousarray(coef.real)
    # the lists and their emission vectors
    ptr, comps, dists, emit = mex(4, "shoebox_components", ROOM, BETA, SRC, POS, FS, 400.0, [])
    (want_c,), (want_d,), (want_e,) = E.getShoeboxComponents(ROOM, BETA, SRC, POS, FS, 400.0, returnDistance=True, returnEmission=True)
    assert list(ptr[:, 0]) == [0, 136] and np.array_equal(comps, want_c) and np.array_equal(dists[:, 0], want_d)
    assert emit.shape == (136, 3) and np.array_equal(emit, want_e)
    iptr, icomps, iexps, ipaths, iemit = mex(5, "shoebox_images", ROOM, SRC, POS, FS, 400.0, [])
    (ic,), (ie,), (ip,), (iem,) = E.getShoeboxImages(ROOM, SRC, POS, FS, 400.0, returnEmission=True)
    assert np.array_equal(icomps, ic) and np.array_equal(iexps, ie) and np.array_equal(ipaths[:, 0], ip) and np.array_equal(iemit, iem)
    # listed: plane waves with a complex directivity and a rotation; point sources with a real one and the room's axes
    got, = mex(1, "array_irs", ptr, comps, FS, 512, 16.0, 0.042, mics, 4, [], 1024, [], [], [], [], [], emit, R.reshape(1, 9), rows(coef))
    want = E.getArrayIrs([want_c], FS, 512, 16.0, 0.042, mics, nfft=1024, emission=[want_e], sourceOrientation=R, directivity=coef)
    assert got.shape == (512, 7, 1) and np.abs(want).max() > 0 and np.array_equal(got.transpose(2, 0, 1), want)
    plain = E.getArrayIrs([want_c], FS, 512, 16.0, 0.042, mics, nfft=1024)
    assert np.abs(want - plain).max() > 0.1 * np.abs(want).max()                                  # the directivity is there
    pt, = mex(1, "array_irs", ptr, comps, FS, 512, 16.0, 0.042, mics, 4, [], 1024, [], [], [], [], dists, emit, [], rows(real_coef))
    assert np.array_equal(pt.transpose(2, 0, 1), E.getArrayIrs([want_c], FS, 512, 16.0, 0.042, mics, nfft=1024, distance=[want_d], emission=[want_e],
                                                              directivity=real_coef))
    # the fused calls: flat walls (the listed call's bits), spectral walls with air as point sources
    room, counts = mex(2, *room_args(512, 16.0, mics, maxDelay=400.0, rot=R.reshape(1, 9), coef=rows(coef)))
    assert np.array_equal(room, got) and list(counts[:, 0]) == [136]
    room, = mex(1, *room_args(512, 16.0, mics, walls=WALLS, air=AIR, model="pointSource", maxDelay=400.0, rot=R.reshape(1, 9), coef=rows(coef)))
    assert np.array_equal(room.transpose(2, 0, 1), E.getArrayRoomIrs(ROOM, WALLS, SRC, POS, FS, 512, 16.0, 0.042, mics, nfft=1024, maxDelay=400.0,
                                                                    airAttenuation=AIR, waveModel="pointSource", sourceOrientation=R, directivity=coef))
    # without the new arguments: today's calls
    today, = mex(1, *room_args(512, 16.0, mics, maxDelay=400.0))
    assert np.array_equal(today.transpose(2, 0, 1), E.getArrayRoomIrs(ROOM, BETA, SRC, POS, FS, 512, 16.0, 0.042, mics, nfft=1024, maxDelay=400.0))
