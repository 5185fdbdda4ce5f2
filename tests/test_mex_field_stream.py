"""The field-stream commands of the MATLAB gateway ('field_create' | 'field_push' | 'field_reset' | 'field_destroy'), compiled
against the stand-in mex.h (tests/mexstub/) and driven from Python like the decode stream's (tests/test_mex_decode_stream.py):
the argument errors and their identifiers without a GPU; on the GPU a push through the gateway equals the C entry bit for bit."""
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


def test_field_commands_argument_errors(mex):
    r = np.zeros((40, 16))
    with pytest.raises(mex.Error, match="eMagLS:arg.*field_create needs"):
        mex(1, "field_create", r)
    with pytest.raises(mex.Error, match="eMagLS:arg.*blockSize must be an integer"):
        mex(1, "field_create", r, 64.5)
    with pytest.raises(mex.Error, match="eMagLS:native.*block size"):          # the library's message, forwarded
        mex(1, "field_create", r, 48)
    with pytest.raises(mex.Error, match="eMagLS:native.*16 sources"):
        mex(1, "field_create", np.zeros((4, 2, 17)), 64)
    with pytest.raises(mex.Error, match="eMagLS:native.*256 channels"):
        mex(1, "field_create", np.zeros((4, 257)), 64)
    with pytest.raises(mex.Error, match="eMagLS:arg.*invalid field stream handle"):
        mex(1, "field_push", 7, np.zeros((64, 1)))
    with pytest.raises(mex.Error, match="eMagLS:arg.*field_push needs"):
        mex(1, "field_push", 1)
    h = mex(1, "field_create", np.zeros((40, 16, 2)), 64)[0].item()
    assert h >= 1
    with pytest.raises(mex.Error, match="eMagLS:arg.*source count"):
        mex(1, "field_push", h, np.zeros((64, 3)))
    with pytest.raises(mex.Error, match="eMagLS:arg.*source count"):
        mex(1, "field_push", h, np.zeros((64, 2), dtype=complex))
    with pytest.raises(mex.Error, match="eMagLS:native.*multiple of the block size"):
        mex(1, "field_push", h, np.zeros((100, 2)))
    mex(0, "field_destroy", h)
    with pytest.raises(mex.Error, match="eMagLS:arg.*invalid field stream handle"):
        mex(0, "field_reset", h)
    with pytest.raises(mex.Error, match="eMagLS:arg.*field_destroy needs"):
        mex(0, "field_destroy")
    h2 = mex(1, "field_create", r + 0j, 64)[0].item()
    assert h2 == h                                                            # the freed slot is taken again
    mex(0, "field_destroy", h2)


@pytest.mark.gpu
@pytest.mark.parametrize("cplx", [False, True])
def test_field_push_matches_the_c_entry(mex, cplx):
    from emagls_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng(18)
    B, nsrc, nch, nr, n = 128, 2, 9, 300, 1024
    rirs = rng.standard_normal((nr, nch, nsrc)) + (1j * rng.standard_normal((nr, nch, nsrc)) if cplx else 0)   # MATLAB's order
    s = rng.standard_normal((n, nsrc))
    h = mex(1, "field_create", rirs, B)[0].item()
    flat = np.ascontiguousarray(rirs.transpose(2, 1, 0))                      # the sources one after the other, each column-major
    f = C.c_void_p()
    L.check(lib.emagls_field_stream_create(nsrc, nch, flat.ctypes.data_as(C.c_void_p), int(cplx), nr, B, C.byref(f)))
    try:
        for rep in range(2):
            for i in range(0, n, 2 * B):
                blk = np.asfortranarray(s[i:i + 2 * B])
                got = mex(1, "field_push", h, blk)[0]
                want = np.zeros((2 * B, nch), dtype=complex if cplx else float, order="F")
                L.check(lib.emagls_field_stream_push(f, blk.ctypes.data_as(C.c_void_p), 2 * B, want.ctypes.data_as(C.c_void_p)))
                assert got.shape == (2 * B, nch) and np.iscomplexobj(got) == cplx and np.array_equal(got, want), (rep, i)
                assert np.abs(want).max() > 0
            mex(0, "field_reset", h)
            L.check(lib.emagls_field_stream_reset(f))
    finally:
        mex(0, "field_destroy", h)
        L.check(lib.emagls_field_stream_destroy(f))
