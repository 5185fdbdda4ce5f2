"""CPU-side checks of the boundary: the C-ABI library builds, loads and exports every symbol that
include/emagls.h declares; without a GPU every compute entry point fails loudly (no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from emagls_amd import build, _lib
    build.build(jobs=4, verbose=False)
    return _lib.load()


def test_header_and_binding_agree(lib):
    from emagls_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "emagls.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(emagls_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name


def test_struct_layouts_match_header(tmp_path):
    """The ctypes mirrors have the size and field offsets the C compiler gives the header's structs."""
    import subprocess
    from emagls_amd import _lib
    src = tmp_path / "layout.c"
    fields_d = [f[0] for f in _lib.DesignDesc._fields_]
    fields_i = [f[0] for f in _lib.PlanInfo._fields_]
    fields_f = [f[0] for f in _lib.DebugFactorArgs._fields_]
    body = "".join('printf("%%zu\\n", offsetof(emagls_design_desc, %s));' % f for f in fields_d)
    body += "".join('printf("%%zu\\n", offsetof(emagls_plan_info, %s));' % f for f in fields_i)
    body += "".join('printf("%%zu\\n", offsetof(emagls_debug_factor_args, %s));' % f for f in fields_f)
    body += 'printf("%zu\\n", sizeof(emagls_debug_factor_args));'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "emagls.h"\nint main(void){printf("%zu %zu\\n", '
                   'sizeof(emagls_design_desc), sizeof(emagls_plan_info));' + body + 'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(out[0]), int(out[1])] == [C.sizeof(_lib.DesignDesc), C.sizeof(_lib.PlanInfo)]
    offs = [int(x) for x in out[2:]]
    want = [getattr(_lib.DesignDesc, f).offset for f in fields_d] + [getattr(_lib.PlanInfo, f).offset for f in fields_i]
    want += [getattr(_lib.DebugFactorArgs, f).offset for f in fields_f] + [C.sizeof(_lib.DebugFactorArgs)]
    assert "leaf_rows" in fields_f
    assert offs == want


def test_no_cpu_fallback(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import emagls_amd as E
    from emagls_amd._lib import EmaglsError
    with pytest.raises(EmaglsError):
        E.getSH(2, np.zeros((4, 2)), "real")
    with pytest.raises(EmaglsError):
        E.getLsFilters(np.zeros((8, 30)), np.zeros((8, 30)), np.zeros(30), np.zeros(30), 1)


def test_product_does_not_import_oracle():
    """The oracle is test infrastructure: nothing under emagls_amd/ may reference it."""
    for dp, _, fs in os.walk(os.path.join(ROOT, "emagls_amd")):
        for f in fs:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                src = open(os.path.join(dp, f), errors="replace").read()
                assert "emagls_oracle" not in src and "from oracle" not in src and "import oracle" not in src, f


def test_design_out_shape_needs_no_gpu(lib):
    """emagls_design_out_shape (include/emagls.h): the filter shape of every design kind from the descriptor alone -- what a C or MEX
    caller allocates for a job of emagls_jobs_run (lib/getLsFilters.m:33 keeps the HRIR length; lib/getEMagLs2Filters.m:132-135 one
    filter per microphone; getMagLsFilters2D / EMAinCH 2N+1 circular harmonics; FromAtf real whatever the basis)."""
    import ctypes as C
    from emagls_amd import _lib as L
    cases = [  # kind, basis, order, len, nsamp, nmics -> rows, cols, complex
        (L.KIND_LS, "complex", 3, 512, 128, 0, (128, 16, True)), (L.KIND_MAGLS, "real", 4, 512, 128, 0, (512, 25, False)),
        (L.KIND_MAGLS_2D, "complex", 7, 256, 64, 0, (256, 15, True)), (L.KIND_EMAGLS, "complex", 4, 512, 128, 32, (512, 25, True)),
        (L.KIND_EMAGLS2, "complex", 4, 1024, 128, 32, (1024, 32, True)), (L.KIND_EMAGLS2, "real", 1, 1024, 128, 64, (1024, 64, False)),
        (L.KIND_EMA_CH, "real", 5, 512, 128, 16, (512, 11, False)), (L.KIND_EMA_SH, "real", 3, 512, 128, 16, (512, 16, False)),
        (L.KIND_FROM_ATF, "complex", 0, 2048, 256, 8, (2048, 8, False))]
    for kind, basis, order, ln, nsamp, nmics, want in cases:
        d = L.DesignDesc(kind, L.BASIS[basis], order, 48000.0, ln, nsamp, 2702, 0.042, nmics, 0.0, 0, 0, 0, 0, 0)
        r, c, z = C.c_int64(0), C.c_int64(0), C.c_int(0)
        assert lib.emagls_design_out_shape(C.byref(d), C.byref(r), C.byref(c), C.byref(z)) == 0
        assert (r.value, c.value, bool(z.value)) == want, (kind, basis)
    bad = L.DesignDesc(99, 0, 1, 48000.0, 16, 16, 10, 0.0, 0, 0.0, 0, 0, 0, 0, 0)
    r, c, z = C.c_int64(0), C.c_int64(0), C.c_int(0)
    assert lib.emagls_design_out_shape(C.byref(bad), C.byref(r), C.byref(c), C.byref(z)) != 0


def test_debug_synth_operand_rejects_bad_arguments(lib):
    """emagls_debug_synth_operand validates before it touches the device: the row length is even, 2 ... 96 (SY_NORD), the group
    size 2, 3 or 4, the counts positive, the pointers set."""
    from emagls_amd import _lib as L
    bsc = np.zeros((1, 98), dtype=np.complex128)
    x = np.zeros(4)
    gp, gm = np.zeros((1, 4), dtype=np.complex128), np.zeros((1, 4), dtype=np.complex128)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def call(nbins=1, nord_pad=4, nx=4, gs=3, a=bsc, b=x, c=gp, d=gm):
        return lib.emagls_debug_synth_operand(p(a) if a is not None else None, nbins, nord_pad, p(b) if b is not None else None, nx, gs,
                                              p(c) if c is not None else None, p(d) if d is not None else None)
    for kw in (dict(nord_pad=0), dict(nord_pad=-2), dict(nord_pad=3), dict(nord_pad=95), dict(nord_pad=98), dict(gs=1), dict(gs=5), dict(nbins=0),
               dict(nbins=65536), dict(nx=0), dict(nx=(1 << 24) + 1), dict(a=None), dict(b=None), dict(c=None), dict(d=None)):
        assert call(**kw) == L.ERR_ARG, kw
    assert call(nord_pad=3) == L.ERR_ARG and b"nord_pad" in lib.emagls_last_error()
    ang, out = np.zeros(4), np.zeros(16)
    for nd, nm, a in ((0, 4, ang), ((1 << 20) + 1, 4, ang), (4, 0, ang), (4, 65, ang), (4, 4, None)):
        assert lib.emagls_debug_synth_cosines(p(a) if a is not None else None, p(ang), nd, p(ang), p(ang), nm, p(out)) == L.ERR_ARG


def test_debug_factor_rejects_bad_arguments(lib):
    """emagls_debug_factor and emagls_debug_factor_gram validate before they touch the device (no GPU is needed to be refused): one input
    form, the sizes within their ranges, the modes and selectors among their values, the wide path's restrictions, the pointers set."""
    from emagls_amd import _lib as L
    S, Cc, ldS = 6, 3, 8
    X = np.zeros((1, Cc, ldS), dtype=np.complex128)
    Z = np.zeros((1, Cc, ldS), dtype=np.complex128)
    Tn = np.zeros((2, Cc, ldS)); bn = np.zeros((1, 2), dtype=np.complex128)
    Hq = np.zeros((2, 1, ldS), dtype=np.complex128); W = np.zeros((2, 1, Cc), dtype=np.complex128)
    p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731

    def call(**kw):
        d = dict(S=S, C=Cc, ldS=ldS, nbins=1, kb0=0, P=1, Xd=p(X), xd_stride=Cc * ldS, Tn=None, tn_cplx=0, bn=None, nOrders=0, reg_mode=0,
                 reg_c=0.01, tol_dim=0.0, Hq=None, ldHq=0, ls_end=0, hq_conj=0, phases=3, path=0, Z=p(Z))
        d.update(kw)
        return lib.emagls_debug_factor(C.byref(L.DebugFactorArgs(**d)))
    for kw in (dict(Z=None), dict(Xd=None), dict(Tn=p(Tn), bn=p(bn), nOrders=2), dict(path=2), dict(path=-1), dict(phases=1), dict(phases=2), dict(phases=0),
               dict(S=0), dict(C=0), dict(C=65), dict(ldS=S - 1), dict(ldS=4097), dict(nbins=0), dict(nbins=4097), dict(P=0), dict(kb0=-1), dict(kb0=1, P=2),
               dict(P=8193), dict(reg_mode=2), dict(reg_c=-0.1), dict(reg_c=1.5), dict(reg_c=float("nan")), dict(tol_dim=-1.0), dict(xd_stride=5),
               dict(Xd=None, Tn=p(Tn), bn=None, nOrders=2), dict(Xd=None, Tn=p(Tn), bn=p(bn), nOrders=0), dict(Xd=None, Tn=p(Tn), bn=p(bn), nOrders=1025),
               dict(Hq=p(Hq), W=None, ldHq=ldS, ls_end=1), dict(Hq=p(Hq), W=p(W), ldHq=S - 1, ls_end=1), dict(Hq=p(Hq), W=p(W), ldHq=ldS, ls_end=2),
               dict(path=1), dict(path=1, ldS=64, reg_mode=1), dict(path=1, ldS=64, phases=12),
               dict(path=1, ldS=64, Hq=p(Hq), W=p(W), ldHq=64, ls_end=1, hq_conj=1), dict(path=1, ldS=64, Hq=p(Hq), W=None, ldHq=64, ls_end=1),
               dict(path=1, ldS=64, Xd=None, Tn=p(Tn), bn=p(bn), nOrders=2),
               dict(path=3)):
        assert call(**kw) == L.ERR_ARG, kw
    # the tiled path (xd_stride = 0 is right for every ldS, so each case is refused for the reason it names): its own limits, the
    # restrictions of the wide paths, the leaf bound, the memory cap with Hq counted
    for frag, kw in ((b"tiled path", dict(path=2, ldS=64, C=33, S=40)), (b"tiled path", dict(path=2, ldS=16448)), (b"tiled path", dict(path=2, ldS=64, nbins=9, P=9)),
                     (b"wide paths", dict(path=2, ldS=8)), (b"wide paths", dict(path=2, ldS=64, reg_mode=1)), (b"wide paths", dict(path=2, ldS=64, phases=12)),
                     (b"wide paths", dict(path=2, ldS=64, Hq=p(Hq), W=p(W), ldHq=64, ls_end=1, hq_conj=1)),
                     (b"wide paths", dict(path=1, ldS=64, Hq=p(Hq), W=p(W), ldHq=64, ls_end=1, hq_conj=1)),
                     (b"wide paths", dict(path=2, ldS=64, Xd=None, Tn=p(Tn), bn=p(bn), nOrders=2)),
                     (b"leaf_rows", dict(path=2, ldS=64, leaf_rows=1023)), (b"leaf_rows", dict(path=2, ldS=64, leaf_rows=4097)),
                     (b"leaf_rows", dict(path=2, ldS=64, leaf_rows=-1)), (b"leaf_rows", dict(path=0, leaf_rows=1024)),
                     (b"leaf_rows", dict(path=1, ldS=64, leaf_rows=1024)),
                     (b"1 GiB", dict(path=2, ldS=16384, S=16384, C=32, nbins=8, P=8192, Hq=p(Hq), W=p(W), ldHq=16384, ls_end=1))):
        assert call(xd_stride=0, **kw) == L.ERR_ARG and frag in lib.emagls_last_error(), (kw, lib.emagls_last_error())
    # a leaf with fewer rows than columns is the launcher's refusal, made before the device is touched
    assert call(xd_stride=0, path=2, ldS=15424, S=15361, C=3, leaf_rows=1024) == L.ERR_UNSUPPORTED and b"fewer rows than columns" in lib.emagls_last_error()
    assert call(phases=1) == L.ERR_ARG and b"phases" in lib.emagls_last_error()
    assert lib.emagls_debug_factor(None) == L.ERR_ARG

    A = np.zeros((2, Cc, Cc), dtype=np.complex128); M = np.zeros_like(A)
    route = np.ones(2, dtype=np.int32); sv = np.zeros((2, Cc)); sw = np.zeros(2, dtype=np.int32); status = np.zeros(4, dtype=np.int32)

    def gram(nbins=2, Cn=Cc, jrun=1, reg_c=0.01, cond_limit=1e5, a=A, r=route, m=M, s=sv, w=sw, t=status):
        return lib.emagls_debug_factor_gram(p(a), nbins, Cn, p(r), jrun, reg_c, cond_limit, p(m), p(s), p(w), p(t))
    bad_route = np.array([1, 0], dtype=np.int32)
    for kw in (dict(nbins=0), dict(nbins=4097), dict(Cn=0), dict(Cn=65), dict(jrun=0), dict(jrun=17), dict(reg_c=-1.0), dict(reg_c=2.0), dict(cond_limit=0.5),
               dict(cond_limit=float("nan")), dict(r=bad_route), dict(a=None), dict(r=None), dict(m=None), dict(s=None), dict(w=None), dict(t=None)):
        assert gram(**kw) == L.ERR_ARG, kw
    assert gram(r=bad_route) == L.ERR_ARG and b"route" in lib.emagls_last_error()


def test_debug_wa_yri_rejects_bad_arguments(lib):
    """emagls_debug_wa_yri validates before it touches the device: 1 <= C <= 64, 1 <= S <= ldS, S <= ldQ, 1 <= D <= ldD, the bins, the memory
    cap, the pointers set"""
    from emagls_amd import _lib as L
    p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    Q, Z, Y = np.zeros((3, 64)), np.zeros((1, 5, 64), dtype=np.complex128), np.zeros((1, 5, 64), dtype=np.complex128)

    def call(q=Q, ldQ=64, z=Z, S=33, Cn=5, ldS=64, D=3, ldD=64, nbins=1, y=Y):
        return lib.emagls_debug_wa_yri(p(q), ldQ, p(z), S, Cn, ldS, D, ldD, nbins, p(y))
    for kw in (dict(q=None), dict(z=None), dict(y=None), dict(Cn=0), dict(Cn=65), dict(S=0), dict(S=65), dict(ldS=16448, S=16448, ldQ=16448), dict(ldQ=32),
               dict(D=0), dict(D=65), dict(ldD=65537, D=65537), dict(nbins=0), dict(nbins=4097),
               dict(Cn=64, S=16384, ldS=16384, ldQ=16384, D=65536, ldD=65536, nbins=1)):   # (8 GiB of Q)
        assert call(**kw) == L.ERR_ARG, kw
    assert call(Cn=65) == L.ERR_ARG and b"wa_yri" in lib.emagls_last_error()


def test_debug_fft_entries_reject_bad_arguments(lib):
    """emagls_debug_filter_epilogue, emagls_debug_hrir_spectra, emagls_debug_real_spectra and emagls_debug_twiddles validate before they
    touch the device (no GPU is needed to be refused): the sizes within their ranges, the modes among their values, the mirror rules'
    channel counts, indices inside the input, the paddings large enough, the pointers set."""
    from emagls_amd import _lib as L
    p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    nfft, ln, Cc = 16, 8, 9
    W = np.zeros((2, nfft // 2 + 1, 25), dtype=np.complex128)
    g = np.array([1.5, -2.0])
    oL, oR = np.zeros((25, nfft), dtype=np.complex128), np.zeros((25, nfft), dtype=np.complex128)

    def epi(w=W, C_=Cc, n=nfft, length=ln, grpd=g, conj=0, dc=1, shift=0, cplx=0, ears=2, fade=0.15, a=oL, b=oR):
        return lib.emagls_debug_filter_epilogue(p(w), C_, n, length, p(grpd), conj, dc, shift, cplx, ears, fade, p(a), p(b))
    for kw in (dict(w=None), dict(a=None), dict(b=None), dict(grpd=None), dict(n=2), dict(n=15), dict(n=4098), dict(n=0), dict(length=0), dict(length=7),
               dict(length=nfft + 2), dict(C_=0), dict(C_=1025), dict(conj=3), dict(conj=-1), dict(conj=1, C_=7), dict(conj=2, C_=4), dict(dc=2), dict(shift=2),
               dict(shift=-1), dict(cplx=2), dict(ears=0), dict(ears=3), dict(fade=-0.01), dict(fade=0.51), dict(fade=float("nan")),
               dict(grpd=np.array([np.inf, 0.0])), dict(grpd=np.array([0.0, np.nan]))):
        assert epi(**kw) == L.ERR_ARG, kw
    assert epi(conj=1, C_=7) == L.ERR_ARG and b"conj_mode 1" in lib.emagls_last_error()

    Lt, D = 5, 3
    hL, hR = np.zeros((D, Lt)), np.zeros((D, Lt))
    P = nfft // 2 + 1
    idx, bad_idx = np.array([0, 2, 2], dtype=np.int64), np.array([0, 3, 1], dtype=np.int64)
    go, phs = np.zeros(2), np.zeros((2, P), dtype=np.complex128)
    Hc, Ha, HT = np.zeros((2, P, 8), dtype=np.complex128), np.zeros((2, P, 8)), np.zeros((D, 4 * P))

    def hrir(a=hL, b=hR, L_=Lt, Ds=D, D_=D, didx=None, n=nfft, mode=0, n_c=P, kabs0=0, gin=None, ldD=8, ldT=4 * P, gout=go, ph=phs, hc=Hc, ha=Ha, ht=HT):
        return lib.emagls_debug_hrir_spectra(p(a), p(b), L_, Ds, D_, p(didx), n, mode, n_c, kabs0, p(gin), ldD, ldT, p(gout), p(ph), p(hc), p(ha), p(ht))
    for kw in (dict(a=None), dict(b=None), dict(n=2), dict(n=15), dict(n=2050), dict(L_=0), dict(L_=4097), dict(L_=nfft + 1), dict(Ds=0), dict(Ds=65537), dict(D_=0),
               dict(D_=D + 1), dict(didx=bad_idx), dict(didx=np.array([0, -1, 1], dtype=np.int64)), dict(mode=2), dict(mode=-1), dict(n_c=-1), dict(n_c=P + 1),
               dict(kabs0=-1), dict(kabs0=P + 1), dict(ldD=D - 1), dict(ldD=12), dict(ldD=1 << 18), dict(ldT=4 * P - 2), dict(ldT=4 * P + 1), dict(ldT=8194),
               dict(hc=None), dict(ha=None), dict(hc=None, ha=None, ht=None, gout=None), dict(hc=None, ha=None, ht=None, gin=g),
               dict(gin=np.array([2.0 ** 21, 0.0])), dict(gin=np.array([0.0, np.nan])), dict(n=1024, gin=g, mode=0, n_c=0, kabs0=513, ht=None)):
        assert hrir(**kw) == L.ERR_ARG, kw
    assert hrir(n=1024, gin=g, mode=0, n_c=0, kabs0=513, ht=None) == L.ERR_ARG and b"1024" in lib.emagls_last_error()

    x, out = np.zeros((4, Lt)), np.zeros((P, 8), dtype=np.complex128)

    def real(a=x, L_=Lt, src=4, nc=4, ci=None, n=nfft, ldo=8, inner=4, ldi=4, o=out):
        return lib.emagls_debug_real_spectra(p(a), L_, src, nc, p(ci), n, ldo, inner, ldi, p(o))
    for kw in (dict(a=None), dict(o=None), dict(n=2), dict(n=15), dict(n=4098), dict(L_=0), dict(L_=8193), dict(src=0), dict(nc=0), dict(nc=5), dict(nc=65537, src=65537),
               dict(nc=3, ci=np.array([0, 4, 1], dtype=np.int64)), dict(nc=3, ci=np.array([0, -1, 1], dtype=np.int64)), dict(inner=0), dict(inner=4, ldi=3),
               dict(ldi=1 << 18, inner=1), dict(ldo=3), dict(inner=2, ldi=5, ldo=6), dict(ldo=(1 << 20) + 1)):
        assert real(**kw) == L.ERR_ARG, kw
    tw = np.zeros(16, dtype=np.complex128)
    for n, t in ((1, tw), (8193, tw), (16, None)):
        assert lib.emagls_debug_twiddles(n, p(t)) == L.ERR_ARG


def test_debug_gram_entries_reject_bad_arguments(lib):
    """emagls_debug_gram, emagls_debug_gram_assemble, emagls_debug_gram_from_g and emagls_debug_gram_solve validate before they touch the
    device (no GPU is needed to be refused): the sizes within their ranges, one input form of the assembly, the 1 GiB cap, the pointers set."""
    from emagls_amd import _lib as L
    p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    S, D, ld = 5, 7, 8
    Y, Gm, Rm = np.zeros((D, ld)), np.zeros((S, S)), np.zeros((S, S))

    def gram(y=Y, D_=D, S_=S, ld_=ld, cplx=0, Sh=3, g=Gm, r=Rm):
        return lib.emagls_debug_gram(p(y), D_, S_, ld_, cplx, Sh, p(g), p(r))
    for kw in (dict(y=None), dict(g=None), dict(r=None), dict(cplx=2), dict(cplx=-1), dict(S_=0), dict(ld_=S - 1), dict(ld_=8193), dict(Sh=0), dict(Sh=S + 1),
               dict(D_=0), dict(D_=65537), dict(S_=8192, ld_=8192, cplx=1)):
        assert gram(**kw) == L.ERR_ARG, kw
    assert gram(S_=8192, ld_=8192, cplx=1) == L.ERR_ARG and b"1 GiB" in lib.emagls_last_error()

    C_, nO, P = 2, 3, 4
    Gy, E, bn = np.zeros((9, 9)), np.zeros((C_, 16)), np.zeros((P, nO), dtype=np.complex128)
    F, K, Cf, A = np.zeros((nO, C_, 16)), np.zeros((12, 64)), np.zeros((12, 64)), np.zeros((3, 64))

    def asm(gy=Gy, e=E, ldE=16, b=bn, C=C_, nOrd=nO, P_=P, kb0=1, nbins=3, cplx=0, kin=None, f=F, k=K, cf=Cf, a=A):
        return lib.emagls_debug_gram_assemble(p(gy), p(e), ldE, p(b), C, nOrd, P_, kb0, nbins, cplx, p(kin), p(f), p(k), p(cf), p(a))
    for kw in (dict(b=None), dict(k=None), dict(cf=None), dict(a=None), dict(gy=None), dict(e=None), dict(kin=K), dict(kin=K, gy=None, e=None), dict(cplx=2),
               dict(C=0), dict(C=33), dict(nOrd=0), dict(nOrd=97), dict(nbins=0), dict(kb0=-1), dict(kb0=2), dict(P_=8193), dict(ldE=8), dict(ldE=16385)):
        assert asm(**kw) == L.ERR_ARG, kw
    assert asm(kin=K) == L.ERR_ARG and b"Kmat_in" in lib.emagls_last_error()

    Gk, Ak = np.zeros((4, C_, 8), dtype=np.complex128), np.zeros((3, 64))

    def from_g(g=Gk, D_=5, C=C_, ldD=8, kb0=2, g0=1, nbins=3, a=Ak):
        return lib.emagls_debug_gram_from_g(p(g), D_, C, ldD, kb0, g0, nbins, p(a))
    for kw in (dict(g=None), dict(a=None), dict(C=0), dict(C=33), dict(D_=0), dict(ldD=4), dict(ldD=65537), dict(g0=-1), dict(g0=3), dict(nbins=0),
               dict(nbins=8193), dict(kb0=8193, g0=8193), dict(C=32, D_=65536, ldD=65536, nbins=64)):
        assert from_g(**kw) == L.ERR_ARG, kw

    Ap, Mw, R2, sv = np.zeros((3, 64)), np.zeros((4, C_, C_), dtype=np.complex128), np.zeros((4, C_, C_), dtype=np.complex128), np.zeros((4, C_))
    rt, sw = np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.int32)

    def solve(a=Ap, ldA=64, C=C_, kb0=1, nbins=3, reg_c=0.01, m=Mw, r2=R2, s=sv, r=rt, w=sw):
        return lib.emagls_debug_gram_solve(p(a), ldA, C, kb0, nbins, reg_c, p(m), p(r2), p(s), p(r), p(w))
    for kw in (dict(a=None), dict(m=None), dict(r2=None), dict(s=None), dict(r=None), dict(w=None), dict(C=0), dict(C=33), dict(ldA=3), dict(ldA=4097),
               dict(kb0=0), dict(nbins=0), dict(kb0=8000, nbins=193), dict(reg_c=0.0), dict(reg_c=-0.01), dict(reg_c=1.5), dict(reg_c=float("nan"))):
        assert solve(**kw) == L.ERR_ARG, kw
    assert solve(kb0=0) == L.ERR_ARG and b"kb0" in lib.emagls_last_error()
