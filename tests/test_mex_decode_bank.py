"""The bank of filter sets through the MATLAB gateway: 'stream_create' with 3-D filter arrays [len x numChannels x numSets] and
'stream_push' with a set index, ONE-based on the MATLAB side; compiled against the stand-in mex.h (tests/mexstub/) and driven from
Python on the model of tests/test_mex_decode_stream.py: the argument errors without a GPU; on the GPU a push through the
gateway equals the Python class (zero-based) bit for bit."""
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


def test_bank_commands_argument_errors(mex):
    w = np.zeros((40, 16, 3))
    with pytest.raises(mex.Error, match="equal size"):
        mex(1, "stream_create", w, np.zeros((40, 16, 2)), 64)
    with pytest.raises(mex.Error, match="equal size"):
        mex(1, "stream_create", w, np.zeros((40, 16)), 64)
    with pytest.raises(mex.Error, match="numSets"):
        mex(1, "stream_create", np.zeros((40, 16, 3, 2)), np.zeros((40, 16, 3, 2)), 64)
    h = mex(1, "stream_create", w, w, 64)[0].item()
    assert h >= 1
    x = np.zeros((128, 16))
    with pytest.raises(mex.Error, match="channel count"):                     # the channels are the second dimension, not 16 * 3
        mex(1, "stream_push", h, np.zeros((64, 48)))
    with pytest.raises(mex.Error, match="count from 1"):                      # one-based: 0 is no set
        mex(1, "stream_push", h, x, [], [], [], 0)
    with pytest.raises(mex.Error, match="count from 1"):
        mex(1, "stream_push", h, x, [], [], [], [1, 1.5])
    with pytest.raises(mex.Error, match="eMagLS:native.*set index outside"):  # 4 of 3 sets: the library's message, forwarded
        mex(1, "stream_push", h, x, [], [], [], 4)
    with pytest.raises(mex.Error, match="eMagLS:native.*0 set indices, 1, or one per block"):
        mex(1, "stream_push", h, x, [], [], [], [1, 2, 3])
    mex(0, "stream_destroy", h)
    h = mex(1, "stream_create", w[:, :, 0], w[:, :, 0], 64)[0].item()          # a 2-D array stays one set
    with pytest.raises(mex.Error, match="eMagLS:native.*set index outside"):
        mex(1, "stream_push", h, x, [], [], [], 2)
    mex(0, "stream_destroy", h)


@pytest.mark.gpu
@pytest.mark.parametrize("cplx", [False, True])
def test_bank_push_matches_the_python_class(mex, cplx):
    import emagls_amd as E
    rng = np.random.default_rng(8)
    rn = lambda *s: rng.standard_normal(s) + (1j * rng.standard_normal(s) if cplx else 0)   # noqa: E731
    B, Cc, n, S = 128, 16, 1024, 3
    x, wL, wR = rn(n, Cc), rn(S, 300, Cc), rn(S, 300, Cc)                     # Python: [numSets x len x numChannels]
    mL, mR = wL.transpose(1, 2, 0), wR.transpose(1, 2, 0)                     # MATLAB: [len x numChannels x numSets]
    basis = "complex" if cplx else "real"
    yaw = np.cumsum(rng.normal(0, 0.01, n))
    sigma = [0, 2, 2, 1, 0, 0, 1, 2]
    h = mex(1, "stream_create", mL, mR, B, basis, "sh", cplx)[0].item()
    with E.BinauralDecodeStream(wL, wR, B, shDefinition=basis, complexInput=cplx) as s:
        for rep in range(2):
            for k in range(0, n // B, 2):
                sl = slice(k * B, (k + 2) * B)
                idx = np.array(sigma[k:k + 2])
                got = mex(1, "stream_push", h, x[sl], yaw[sl], [], [], idx + 1)[0]          # one-based
                want = s.push(x[sl], yaw[sl], setIndex=idx)
                assert got.shape == (2 * B, 2) and np.array_equal(got, want), (rep, k)
            got = mex(1, "stream_push", h, x[:B], [], [], [], 3)[0]                          # a scalar, and then no index: the set is kept
            assert np.array_equal(got, s.push(x[:B], setIndex=2))
            assert np.array_equal(mex(1, "stream_push", h, x[B:2 * B])[0], s.push(x[B:2 * B]))
            mex(0, "stream_reset", h)
            s.reset()
    mex(0, "stream_destroy", h)
    # a constant one-based index on the bank == the plain stream on that set
    h = mex(1, "stream_create", mL, mR, B, basis, "sh", cplx)[0].item()
    with E.BinauralDecodeStream(wL[1], wR[1], B, shDefinition=basis, complexInput=cplx) as s:
        assert np.array_equal(mex(1, "stream_push", h, x, [], [], [], 2)[0], s.push(x))
    mex(0, "stream_destroy", h)
