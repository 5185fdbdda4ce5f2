"""The encoder argument of 'stream_create' and 'group_create' through the MATLAB gateway (mex/emagls_mex.cpp,
mex/binauralDecodeStream.m, mex/binauralDecodeGroup.m), compiled against the stand-in mex.h and driven
from Python: the argument errors without a GPU; on the GPU an encoded stream and an encoded group of two listeners equal the
Python objects bit for bit."""
import numpy as np
import pytest

from test_mex_decode_group import mex  # noqa: F401  (the stub mex.h harness)


def test_encoder_argument_errors(mex):  # noqa: F811
    w = np.zeros((40, 4))
    with pytest.raises(mex.Error, match="encoder must be"):                     # [numMics x numChannels]: the transpose
        mex(1, "stream_create", w, w, 64, "real", "sh", False, np.zeros((6, 4)))
    with pytest.raises(mex.Error, match="complexInput must be false"):
        mex(1, "stream_create", w, w, 64, "real", "sh", True, np.zeros((4, 6)))
    with pytest.raises(mex.Error, match="eMagLS:native.*64 microphones"):       # the library's message, forwarded
        mex(1, "group_create", w, w, 64, 2, "real", "sh", False, np.zeros((4, 65)))
    h = mex(1, "stream_create", w, w, 64, "real", "sh", False, np.zeros((4, 6)))[0].item()
    with pytest.raises(mex.Error, match="channel count"):                       # numChannels columns instead of numMics
        mex(1, "stream_push", h, np.zeros((64, 4)))
    with pytest.raises(mex.Error, match="must be real"):
        mex(1, "stream_push", h, np.zeros((64, 6), dtype=complex))
    mex(0, "stream_destroy", h)
    h = mex(1, "stream_create", w, w, 64, "real", "sh", False, [])[0].item()    # []: a plain stream
    with pytest.raises(mex.Error, match="channel count"):
        mex(1, "stream_push", h, np.zeros((64, 6)))
    mex(0, "stream_destroy", h)


@pytest.mark.gpu
def test_encoded_stream_and_group_match_the_python_objects(mex):  # noqa: F811
    import emagls_amd as E
    rng = np.random.default_rng(21)
    B, M, Cc, n, S, nl = 64, 12, 9, 384, 2, 2
    x, enc = rng.standard_normal((n, M)), rng.standard_normal((Cc, M))
    wL, wR = rng.standard_normal((S, 150, Cc)), rng.standard_normal((S, 150, Cc))
    mL, mR = wL.transpose(1, 2, 0), wR.transpose(1, 2, 0)                       # MATLAB: [len x numChannels x numSets]
    yaw, pitch, roll = (rng.uniform(-1, 1, (nl, 1)) + np.cumsum(rng.normal(0, 0.02, (nl, n)), axis=1) for _ in range(3))
    sig = rng.integers(0, S, (nl, n // B))
    h = mex(1, "stream_create", mL, mR, B, "real", "sh", False, enc)[0].item()
    with E.BinauralDecodeStream(wL, wR, B, encoder=enc) as s:
        for k in range(0, n // B, 2):
            sl = slice(k * B, (k + 2) * B)
            got = mex(1, "stream_push", h, x[sl], yaw[0, sl], pitch[0, sl], roll[0, sl], sig[0, k:k + 2] + 1)[0]
            assert np.array_equal(got, s.push(x[sl], yaw[0, sl], pitch[0, sl], roll[0, sl], setIndex=sig[0, k:k + 2])), k
        assert np.array_equal(mex(1, "stream_push", h, x[:B])[0], s.push(x[:B]))                  # the encoder alone
    mex(0, "stream_destroy", h)
    g_h = mex(1, "group_create", mL, mR, B, nl, "real", "sh", False, enc)[0].item()
    with E.BinauralDecodeGroup(wL, wR, B, nl, encoder=enc) as g:
        for k in range(0, n // B, 2):
            sl = slice(k * B, (k + 2) * B)
            got = mex(1, "group_push", g_h, x[sl], yaw[:, sl].T, pitch[:, sl].T, roll[:, sl].T, sig[:, k:k + 2].T + 1)[0]
            want = g.push(x[sl], yaw[:, sl], pitch[:, sl], roll[:, sl], setIndex=sig[:, k:k + 2])
            assert got.shape == (2 * B, 2, nl) and np.array_equal(got.transpose(2, 0, 1), want), k
        assert np.array_equal(mex(1, "group_push", g_h, x[:B])[0].transpose(2, 0, 1), g.push(x[:B]))
    mex(0, "group_destroy", g_h)
