"""The decode-stream commands of the MATLAB gateway ('stream_create' | 'stream_push' | 'stream_reset' | 'stream_destroy'),
compiled against the stand-in mex.h (tests/mexstub/) and driven from Python like the other commands (tests/test_mex_gateway.py):
the argument errors without a GPU; on the GPU a push through the gateway equals the Python class bit for bit."""
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


def test_stream_commands_argument_errors(mex):
    w = np.zeros((40, 16))
    with pytest.raises(mex.Error, match="stream_create needs"):
        mex(1, "stream_create", w, w)
    with pytest.raises(mex.Error, match="equal size"):
        mex(1, "stream_create", w, np.zeros((40, 9)), 64)
    with pytest.raises(mex.Error, match="eMagLS:native.*block size"):         # the library's message, forwarded
        mex(1, "stream_create", w, w, 48)
    with pytest.raises(mex.Error, match="shDefinition must be 'real' or 'complex'"):
        mex(1, "stream_create", w, w, 64, "n3d")
    with pytest.raises(mex.Error, match="rotation domain"):
        mex(1, "stream_create", w, w, 64, "real", "xy")
    with pytest.raises(mex.Error, match="invalid decode stream handle"):
        mex(1, "stream_push", 7, np.zeros((64, 16)))
    h = mex(1, "stream_create", w, w, 64)[0].item()
    assert h >= 1
    with pytest.raises(mex.Error, match="channel count"):
        mex(1, "stream_push", h, np.zeros((64, 9)))
    with pytest.raises(mex.Error, match="in must be real"):
        mex(1, "stream_push", h, np.zeros((64, 16), dtype=complex))
    with pytest.raises(mex.Error, match="eMagLS:native.*multiple of the block size"):
        mex(1, "stream_push", h, np.zeros((100, 16)))
    with pytest.raises(mex.Error, match="eMagLS:native.*pitch needs no value, one value or one value per input sample"):
        mex(1, "stream_push", h, np.zeros((64, 16)), 0.1, np.zeros(5))
    mex(0, "stream_destroy", h)
    with pytest.raises(mex.Error, match="invalid decode stream handle"):
        mex(0, "stream_reset", h)
    h2 = mex(1, "stream_create", w, w, 64)[0].item()
    assert h2 == h                                                            # the freed slot is taken again
    mex(0, "stream_destroy", h2)


@pytest.mark.gpu
@pytest.mark.parametrize("cplx", [False, True])
def test_stream_push_matches_the_python_class(mex, cplx):
    import emagls_amd as E
    rng = np.random.default_rng(8)
    rn = lambda r, c: rng.standard_normal((r, c)) + (1j * rng.standard_normal((r, c)) if cplx else 0)   # noqa: E731
    B, Cc, n = 128, 16, 1024
    x, wL, wR = rn(n, Cc), rn(300, Cc), rn(300, Cc)
    basis = "complex" if cplx else "real"
    yaw, pitch = np.cumsum(rng.normal(0, 0.01, n)), 0.4 + np.cumsum(rng.normal(0, 0.01, n))
    h = mex(1, "stream_create", wL, wR, B, basis, "sh", cplx)[0].item()
    with E.BinauralDecodeStream(wL, wR, B, shDefinition=basis, complexInput=cplx) as s:
        for rep in range(2):
            for i in range(0, n, 2 * B):
                sl = slice(i, i + 2 * B)
                got = mex(1, "stream_push", h, x[sl], yaw[sl], pitch[sl], 0.25)[0]
                want = s.push(x[sl], yaw[sl], pitch[sl], 0.25)
                assert got.shape == (2 * B, 2) and np.array_equal(got, want), (rep, i)
            mex(0, "stream_reset", h)
            s.reset()
    mex(0, "stream_destroy", h)
