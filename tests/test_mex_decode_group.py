"""The listener group through the MATLAB gateway: 'group_create', 'group_push', 'group_reset' and 'group_destroy' (mex/emagls_mex.cpp,
mex/binauralDecodeGroup.m), compiled against the stand-in mex.h (tests/mexstub/) and driven from Python on the model of
tests/test_mex_decode_bank.py.  Listeners run along the last dimension on the MATLAB side and the set index is ONE-based: the
argument errors without a GPU; on the GPU a push through the gateway equals the Python class bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "mexstub")
LIBDIR = os.path.join(ROOT, "emagls_amd", "lib")


@pytest.fixture(scope="module")
def mex():
    assert os.path.exists(os.path.join(LIBDIR, "libemagls.so")), "libemagls.so is not built (python -m emagls_amd.build)"
    out = os.path.join(STUB, "_build", "libmexharness.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(ROOT, "mex", "emagls_mex.cpp"), os.path.join(STUB, "mexstub.cpp")]
    deps = srcs + [os.path.join(STUB, "mex.h"), os.path.join(ROOT, "include", "emagls.h")]
    if not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in deps):
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + STUB] + srcs + \
              ["-L" + LIBDIR, "-lemagls", "-Wl,-rpath," + LIBDIR, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    import torch  # noqa: F401  (first: the library then shares torch's HIP runtime, as in emagls_amd/_lib.py)
    h = C.CDLL(out)
    h.stub_array.restype = C.c_void_p
    h.stub_array.argtypes = [C.c_int, C.POINTER(C.c_size_t), C.c_void_p, C.c_int]
    h.stub_string.restype = C.c_void_p
    h.stub_string.argtypes = [C.c_char_p]
    h.stub_logical.restype = C.c_void_p
    h.stub_logical.argtypes = [C.c_int]
    h.stub_free.argtypes = [C.c_void_p]
    h.stub_ndim.argtypes = [C.c_void_p]
    h.stub_dims.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    h.stub_is_complex.argtypes = [C.c_void_p]
    h.stub_data.restype = C.c_void_p
    h.stub_data.argtypes = [C.c_void_p]
    h.stub_call.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]

    class MexCallError(RuntimeError):
        pass

    def to_mx(v):
        if isinstance(v, str):
            return h.stub_string(v.encode())
        if isinstance(v, (bool, np.bool_)):
            return h.stub_logical(int(v))
        a = np.asarray(v)
        a = np.asfortranarray(a.astype(np.complex128 if np.iscomplexobj(a) else np.float64))
        if a.ndim < 2:
            a = a.reshape((1, 1) if a.ndim == 0 else (-1, 1), order="F")
        dims = (C.c_size_t * a.ndim)(*a.shape)
        return h.stub_array(a.ndim, dims, a.ctypes.data_as(C.c_void_p), int(np.iscomplexobj(a)))

    def from_mx(p):
        nd = h.stub_ndim(p)
        dims = (C.c_size_t * nd)()
        h.stub_dims(p, dims)
        shape = tuple(int(d) for d in dims)
        n = int(np.prod(shape))
        cplx = bool(h.stub_is_complex(p))
        raw = np.ctypeslib.as_array(C.cast(h.stub_data(p), C.POINTER(C.c_double)), shape=(n * (2 if cplx else 1),)).copy()
        return (raw.view(np.complex128) if cplx else raw).reshape(shape, order="F")

    def call(nlhs, *args):
        ins = [to_mx(a) for a in args]
        prhs = (C.c_void_p * len(ins))(*ins)
        plhs = (C.c_void_p * max(nlhs, 1))()
        err = C.create_string_buffer(2048)
        rc = h.stub_call(nlhs, plhs, len(ins), prhs, err, len(err))
        for p in ins:
            h.stub_free(p)
        if rc:
            raise MexCallError(err.value.decode())
        outs = [from_mx(plhs[i]) for i in range(nlhs)]
        for i in range(nlhs):
            h.stub_free(plhs[i])
        return outs

    call.Error = MexCallError
    return call


def test_group_commands_argument_errors(mex):
    w = np.zeros((40, 4, 3))
    with pytest.raises(mex.Error, match="group_create needs"):
        mex(1, "group_create", w, w, 64)
    with pytest.raises(mex.Error, match="equal size"):
        mex(1, "group_create", w, np.zeros((40, 4, 2)), 64, 2)
    with pytest.raises(mex.Error, match="eMagLS:native.*at least one listener"):
        mex(1, "group_create", w, w, 64, 0)
    with pytest.raises(mex.Error, match="eMagLS:native.*4096"):
        mex(1, "group_create", w, w, 64, 4097)
    with pytest.raises(mex.Error, match="integer"):
        mex(1, "group_create", w, w, 64, 2.5)
    with pytest.raises(mex.Error, match="invalid decode group handle"):
        mex(1, "group_push", 99, np.zeros((64, 4)))
    h = mex(1, "group_create", w, w, 64, 2)[0].item()
    assert h >= 1
    x = np.zeros((128, 4))
    with pytest.raises(mex.Error, match="channel count"):
        mex(1, "group_push", h, np.zeros((64, 12)))
    with pytest.raises(mex.Error, match="one column per listener"):           # listeners are the LAST dimension: [n x L], not [L x n]
        mex(1, "group_push", h, x, np.zeros((2, 128)))
    with pytest.raises(mex.Error, match="one column per listener"):
        mex(1, "group_push", h, x, [], [], [], np.ones((2, 3)))
    with pytest.raises(mex.Error, match="eMagLS:native.*angle"):              # [3 x L]: neither one value per listener nor one per sample
        mex(1, "group_push", h, x, np.zeros((3, 2)))
    with pytest.raises(mex.Error, match="count from 1"):                      # one-based: 0 is no set
        mex(1, "group_push", h, x, [], [], [], np.array([[0, 1]]))
    with pytest.raises(mex.Error, match="eMagLS:native.*set index outside"):  # 4 of 3 sets: the library's message, forwarded
        mex(1, "group_push", h, x, [], [], [], np.array([[1, 4]]))
    with pytest.raises(mex.Error, match="eMagLS:native.*set indices"):        # [3 x L] for two blocks
        mex(1, "group_push", h, x, [], [], [], np.ones((3, 2)))
    with pytest.raises(mex.Error, match="count from 1"):                      # listeners count from 1 too
        mex(0, "group_reset", h, 0)
    with pytest.raises(mex.Error, match="eMagLS:native.*listener outside"):
        mex(0, "group_reset", h, 3)
    mex(0, "group_destroy", h)
    with pytest.raises(mex.Error, match="invalid decode group handle"):
        mex(0, "group_destroy", h)


@pytest.mark.gpu
def test_group_push_matches_the_python_class(mex):
    import emagls_amd as E
    rng = np.random.default_rng(18)
    B, Cc, n, S, nl = 64, 9, 512, 3, 3
    x, wL, wR = rng.standard_normal((n, Cc)), rng.standard_normal((S, 150, Cc)), rng.standard_normal((S, 150, Cc))
    mL, mR = wL.transpose(1, 2, 0), wR.transpose(1, 2, 0)                     # MATLAB: [len x numChannels x numSets]
    yaw, pitch, roll = (rng.uniform(-1, 1, (nl, 1)) + np.cumsum(rng.normal(0, 0.02, (nl, n)), axis=1) for _ in range(3))
    sig = rng.integers(0, S, (nl, n // B))
    h = mex(1, "group_create", mL, mR, B, nl)[0].item()
    with E.BinauralDecodeGroup(wL, wR, B, nl) as g:
        for k in range(0, n // B, 2):
            sl = slice(k * B, (k + 2) * B)
            got = mex(1, "group_push", h, x[sl], yaw[:, sl].T, pitch[:, sl].T, roll[:, sl].T, sig[:, k:k + 2].T + 1)[0]     # [n x L], one-based
            want = g.push(x[sl], yaw[:, sl], pitch[:, sl], roll[:, sl], setIndex=sig[:, k:k + 2])
            assert got.shape == (2 * B, 2, nl) and np.array_equal(got.transpose(2, 0, 1), want), k
        got = mex(1, "group_push", h, x[:B], yaw[:, :1].T, [], [], np.array([[3, 1, 2]]))[0]    # [1 x L]: one value per listener
        assert np.array_equal(got.transpose(2, 0, 1), g.push(x[:B], yaw[:, 0], setIndex=[2, 0, 1]))
        mex(0, "group_reset", h, 2)                                                            # one-based: the second listener
        g.reset(1)
        assert np.array_equal(mex(1, "group_push", h, x[B:2 * B])[0].transpose(2, 0, 1), g.push(x[B:2 * B]))
        mex(0, "group_reset", h)
        g.reset()
        assert np.array_equal(mex(1, "group_push", h, x[:B])[0].transpose(2, 0, 1), g.push(x[:B]))
    mex(0, "group_destroy", h)
