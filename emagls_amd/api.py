"""Host-side mirror of the reference's MATLAB entry points (same names, argument order and error
behaviour), calling the C ABI in include/emagls.h.  NumPy arrays in MATLAB layout:
hL/hR are [numSamples x numDirections]; filters come back [len x numChannels].

    getLsFilters            lib/getLsFilters.m:1-2
    getMagLsFilters         lib/getMagLsFilters.m:1-2
    getEMagLsFilters        lib/getEMagLsFilters.m:1-2
    getEMagLs2Filters       lib/getEMagLs2Filters.m:1-2
    getEMagLsFiltersEMAinCH lib/getEMagLsFiltersEMAinCH.m:1-2
    getEMagLsFiltersEMAinSH lib/getEMagLsFiltersEMAinSH.m:1-2
    getEMagLsFiltersFromAtf lib/getEMagLsFiltersFromAtf.m:1
    binauralDecode          dependencies/binauralDecode.m:1-2
    getMagLsFilters2D       lib/getMagLsFilters2D.m:1
    getRadialFilter         dependencies/getRadialFilter.m:1   (params struct -> dict or keywords)
    applyRadialFilter       dependencies/applyRadialFilter.m:1
    encodeSH                verifyEMagLs.m:235-236             (smaRecording * pinv(getSH(order, micGrid).'))
    getMagLsSphericalHeadFilter  lib/getMagLsSphericalHeadFilter.m:1
    getMagLsArrayDiffuseFilter   lib/getMagLsArrayDiffuseFilter.m:1
    getSH / sphModalCoeffs  the un-vendored third-party functions the above call
    getCH / getSMAIRMatrix  dependencies/getCH.m:1, dependencies/getSMAIRMatrix.m:1 (the array model materialised)
    getRenderedHrtfs        this project's: what a filter set renders per direction, and its error metrics
    getArrayIrs             this project's: impulse responses of the simulated array to plane-wave components
    getShoeboxComponents / getArrayRoomIrs   this project's: those components, and the responses, from a shoebox room (section 12)
    getShoeboxImages / wallReflectionSpectra / airAttenuation   this project's: walls as reflection spectra and air absorption (section 13)

A custom `shFunction` (a callable with getSH's signature: shFunction(N, [azi zen], shDefinition) -> [dirs x (N+1)^2]) cannot
cross the C ABI as a handle: it is evaluated here, at the simulation order the library reports, and its matrices go through the
emagls_*_with_basis entry points -- exactly what the MEX wrappers do with a MATLAB function handle.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib as L


def _f(a):
    """MATLAB-layout (column-major) float64 copy and its pointer."""
    a = np.asfortranarray(np.asarray(a, dtype=np.float64))
    return a, a.ctypes.data_as(C.c_void_p)


def _vec(a, n=None, name="vector"):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel())
    if n is not None and a.size != n:
        raise ValueError("%s must have %d elements, got %d" % (name, n, a.size))
    return a, a.ctypes.data_as(C.c_void_p)


def _out(rows, cols, cplx):
    w = np.zeros((rows, cols), dtype=np.complex128 if cplx else np.float64, order="F")
    return w, w.ctypes.data_as(C.c_void_p)


def _basis(shDefinition, shFunction=None):
    if shDefinition is None or shDefinition == "":
        shDefinition = "real"
    if shDefinition not in L.BASIS:
        raise ValueError("shDefinition must be 'real' or 'complex'")
    return L.BASIS[shDefinition], shDefinition == "complex"


def _hrirs(hL, hR):
    hL, pL = _f(hL)
    hR, pR = _f(hR)
    if hL.ndim != 2 or hL.shape != hR.shape:
        raise ValueError("hL and hR must be [numSamples x numDirections] arrays of equal shape")
    return hL, hR, pL, pR


def getSH(N, dirs, basisType="real"):
    dirs = np.asarray(dirs, dtype=np.float64)
    D = dirs.shape[0]
    azi, pa = _vec(dirs[:, 0])
    zen, pz = _vec(dirs[:, 1])
    b, cplx = _basis(basisType, None)
    Y, pY = _out(D, (N + 1) ** 2, cplx)
    L.check(L.load().emagls_sh_basis(int(N), D, pa, pz, b, pY))
    return Y


def sphModalCoeffs(N, kr, arrayType="rigid", dirCoeff=0.0):
    if arrayType != "rigid":
        raise NotImplementedError("only the rigid-sphere model is on the eMagLS path (lib/getEMagLsFilters.m:38)")
    kr, pk = _vec(kr)
    b, pb = _out(kr.size, N + 1, True)
    L.check(L.load().emagls_modal_bn(int(N), kr.size, pk, pb))
    return b


def getCH(N, aziRad, basisType="real"):
    """dependencies/getCH.m:1: circular harmonics [numDirs x 2N+1], ordered [C_0, C_-1, C_1, ..., C_-N, C_N]."""
    azi, pa = _vec(aziRad)
    b, cplx = _basis(basisType)
    Y, pY = _out(azi.size, 2 * int(N) + 1, cplx)
    L.check(L.load().emagls_ch_basis(int(N), azi.size, pa, b, pY))
    return Y


# the reference's own struct defaults (dependencies/getSMAIRMatrix.m:36-84); regulConst: getRadialFilter.m:49-51
_SMAIR_DEFAULTS = {"order": 4, "fs": 48000, "smaRadius": 0.042, "arrayType": "rigid", "radialFilter": "regul", "sourceDist": 2,
                   "dirCoeff": 0, "waveModel": "planeWave", "noiseGainDb": 20, "oversamplingFactor": 4, "irLen": 2048,
                   "returnRawMicSigs": False, "shDefinition": "real", "regulConst": 1e-2}


def getSMAIRMatrix(params=None, **kw):
    """dependencies/getSMAIRMatrix.m:1: the array model itself, [numShsOut | numMics x numShsSimulation x numFreqs] complex.
    `params` is the reference's struct as a dict (order, fs, irLen, oversamplingFactor, smaRadius, smaDesignAziZenRad,
    shDefinition, returnRawMicSigs, radialFilter, ...; plane-wave model, rigid sphere, built-in getSH).  Fields left out take
    the reference's defaults (:36-84) -- including radialFilter 'regul', which getRadialFilter.m:63-64 rejects: like there, a
    call that wants the SH-domain model must name its radial filter ('none', 'tikhonov', 'softlimit', 'full').  The one field
    without a default here is smaDesignAziZenRad (the reference loads a t-design file that is not part of its repository).
    Returns (smairMat, params) like the reference, with params['simulationOrder'] added."""
    p = dict(_SMAIR_DEFAULTS)
    p.update(params or {})
    p.update(kw)
    if "smaDesignAziZenRad" not in p:
        raise KeyError("params.smaDesignAziZenRad is required")
    if str(p["waveModel"]).lower() != "planewave" or p["arrayType"] != "rigid" or p["dirCoeff"] != 0:
        raise NotImplementedError("only the plane-wave model of a rigid sphere is built in (what the filter designs use)")
    if p.get("shFunction") is not None:
        raise NotImplementedError("getSMAIRMatrix with a custom shFunction is not supported")
    kind = str(p["radialFilter"]).lower()
    if p["returnRawMicSigs"]:
        kind = "none"          # (:124-126: the radial filter is never looked at for raw microphone signals)
    elif kind not in L.RADIAL:
        raise ValueError('Unkown radialFilter parameter "%s".' % p["radialFilter"])   # getRadialFilter.m:64, spelling kept
    grid = np.asarray(p["smaDesignAziZenRad"], dtype=np.float64)
    azi, pa = _vec(grid[:, 0])
    zen, pz = _vec(grid[:, 1])
    b, _ = _basis(p["shDefinition"])
    nfft = int(p["oversamplingFactor"]) * int(p["irLen"])
    order, M = int(p["order"]), azi.size
    so = int(max(order, np.ceil(float(p["fs"]) * np.pi * float(p["smaRadius"]) / 343.0)))
    rows = M if p["returnRawMicSigs"] else (order + 1) ** 2
    out = np.zeros((rows, (so + 1) ** 2, nfft // 2 + 1), dtype=np.complex128, order="F")
    sim = C.c_int(0)
    L.check(L.load().emagls_get_smair_matrix(order, float(p["fs"]), int(p["irLen"]), int(p["oversamplingFactor"]), float(p["smaRadius"]),
                                             pa, pz, M, b, 1 if p["returnRawMicSigs"] else 0, L.RADIAL[kind], float(p["regulConst"]),
                                             float(p["noiseGainDb"]), out.ctypes.data_as(C.c_void_p), C.byref(sim)))
    assert sim.value == so
    p["simulationOrder"] = so
    return out, p


def _sh_matrix(shFunction, n, azi, zen, shDefinition, cplx, rows):
    """Evaluate a custom shFunction and check its result: [rows x (n+1)^2], real or complex like the basis."""
    Y = np.asarray(shFunction(int(n), np.column_stack([azi, zen]), shDefinition if shDefinition else "real"))
    if Y.shape != (rows, (n + 1) ** 2):
        raise ValueError("shFunction returned %s, expected (%d, %d)" % (Y.shape, rows, (n + 1) ** 2))
    if np.iscomplexobj(Y) != cplx:
        raise ValueError("shFunction returned a %s matrix for shDefinition=%r" % ("complex" if np.iscomplexobj(Y) else "real", shDefinition))
    Y = np.asfortranarray(Y, dtype=np.complex128 if cplx else np.float64)
    return Y, Y.ctypes.data_as(C.c_void_p)


def getLsFilters(hL, hR, hrirGridAziRad, hrirGridZenRad, order, shDefinition="real", shFunction=None):
    b, cplx = _basis(shDefinition, shFunction)
    hL, hR, pL, pR = _hrirs(hL, hR)
    n, D = hL.shape
    azi, pa = _vec(hrirGridAziRad, D, "hrirGridAziRad")
    zen, pz = _vec(hrirGridZenRad, D, "hrirGridZenRad")
    wL, pwL = _out(n, (order + 1) ** 2, cplx)
    wR, pwR = _out(n, (order + 1) ** 2, cplx)
    if shFunction is not None:
        Y, pY = _sh_matrix(shFunction, order, azi, zen, shDefinition, cplx, D)
        L.check(L.load().emagls_get_ls_filters_with_basis(pL, pR, n, D, pY, int(order), b, pwL, pwR))
        return wL, wR
    L.check(L.load().emagls_get_ls_filters(pL, pR, n, D, pa, pz, int(order), b, pwL, pwR))
    return wL, wR


def _no_handle_with_dc(shFunction, applyDiffusenessConst):
    if applyDiffusenessConst and shFunction is not None:
        raise NotImplementedError("applyDiffusenessConst with a custom shFunction is not supported")


def getMagLsFilters(hL, hR, hrirGridAziRad, hrirGridZenRad, order, fs, len, shDefinition="real", shFunction=None,
                    applyDiffusenessConst=False):
    """lib/getMagLsFilters.m:1-2.  applyDiffusenessConst: the option the reference removed (its stale docstring :4 still lists
    it); specification: DESIGN.md section 7."""
    _no_handle_with_dc(shFunction, applyDiffusenessConst)
    b, cplx = _basis(shDefinition, shFunction)
    hL, hR, pL, pR = _hrirs(hL, hR)
    n, D = hL.shape
    azi, pa = _vec(hrirGridAziRad, D, "hrirGridAziRad")
    zen, pz = _vec(hrirGridZenRad, D, "hrirGridZenRad")
    wL, pwL = _out(int(len), (order + 1) ** 2, cplx)
    wR, pwR = _out(int(len), (order + 1) ** 2, cplx)
    if shFunction is not None:
        Y, pY = _sh_matrix(shFunction, order, azi, zen, shDefinition, cplx, D)
        L.check(L.load().emagls_get_magls_filters_with_basis(pL, pR, n, D, pY, int(order), float(fs), int(len), b, pwL, pwR))
        return wL, wR
    if applyDiffusenessConst:
        L.check(L.load().emagls_get_magls_filters_dc(pL, pR, n, D, pa, pz, int(order), float(fs), int(len), 1, b, pwL, pwR))
        return wL, wR
    L.check(L.load().emagls_get_magls_filters(pL, pR, n, D, pa, pz, int(order), float(fs), int(len), b, pwL, pwR))
    return wL, wR


def _sma(fn_name, raw, hL, hR, azi, zen, micRadius, micAzi, micZen, order, fs, len, shDefinition, shFunction, dc=False):
    _no_handle_with_dc(shFunction, dc)
    b, cplx = _basis(shDefinition, shFunction)
    hL, hR, pL, pR = _hrirs(hL, hR)
    n, D = hL.shape
    azi, pa = _vec(azi, D, "hrirGridAziRad")
    zen, pz = _vec(zen, D, "hrirGridZenRad")
    micAzi, pma = _vec(micAzi)
    micZen, pmz = _vec(micZen, micAzi.size, "micGridZenRad")
    M = micAzi.size
    C_ = M if raw else (order + 1) ** 2
    wL, pwL = _out(int(len), C_, cplx)
    wR, pwR = _out(int(len), C_, cplx)
    if shFunction is not None:
        # lib/getEMagLsFilters.m:68 and dependencies/getSMAIRMatrix.m:101 call the handle at the simulation order
        so = L.load().emagls_simulation_order(L.KIND_EMAGLS2 if raw else L.KIND_EMAGLS, int(order), float(fs), float(micRadius))
        Yh, pYh = _sh_matrix(shFunction, so, azi, zen, shDefinition, cplx, D)
        Ym, pYm = _sh_matrix(shFunction, so, micAzi, micZen, shDefinition, cplx, M)
        fn = getattr(L.load(), fn_name + "_with_basis")
        L.check(fn(pL, pR, n, D, pYh, float(micRadius), pYm, M, int(order), float(fs), int(len), b, pwL, pwR))
        return wL, wR
    if dc:
        fn = getattr(L.load(), fn_name + "_dc")
        L.check(fn(pL, pR, n, D, pa, pz, float(micRadius), pma, pmz, M, int(order), float(fs), int(len), 1, b, pwL, pwR))
        return wL, wR
    fn = getattr(L.load(), fn_name)
    L.check(fn(pL, pR, n, D, pa, pz, float(micRadius), pma, pmz, M, int(order), float(fs), int(len), b, pwL, pwR))
    return wL, wR


def getEMagLsFilters(hL, hR, hrirGridAziRad, hrirGridZenRad, micRadius, micGridAziRad, micGridZenRad, order, fs, len,
                     shDefinition="real", shFunction=None, applyDiffusenessConst=False):
    return _sma("emagls_get_emagls_filters", False, hL, hR, hrirGridAziRad, hrirGridZenRad, micRadius, micGridAziRad,
                micGridZenRad, order, fs, len, shDefinition, shFunction, applyDiffusenessConst)


def getEMagLs2Filters(hL, hR, hrirGridAziRad, hrirGridZenRad, micRadius, micGridAziRad, micGridZenRad, order, fs, len,
                      shDefinition="real", shFunction=None, applyDiffusenessConst=False):
    return _sma("emagls_get_emagls2_filters", True, hL, hR, hrirGridAziRad, hrirGridZenRad, micRadius, micGridAziRad,
                micGridZenRad, order, fs, len, shDefinition, shFunction, applyDiffusenessConst)


def designHrirSets(kind, hL, hR, hrirGridAziRad, hrirGridZenRad=None, micRadius=0.0, micGridAziRad=None, micGridZenRad=None, order=4,
                   fs=48000.0, len=512, shDefinition="real"):
    """The loop over HRIR sets around one of the reference's design functions, as ONE call (emagls_design_hrir_sets): hL, hR
    [numSamples x numDirections x numSets] on one grid (and one array); kind in 'ls', 'magls', 'magls2d', 'emagls', 'emagls2',
    'emainch', 'emainsh'.  Returns wL, wR [len x channels x numSets] -- the filters nsets single calls return (lib/getLsFilters.m:30,
    getMagLsFilters.m:30, getMagLsFilters2D.m:1, getEMagLsFilters.m:32, getEMagLs2Filters.m:32, getEMagLsFiltersEMAinCH.m:32)."""
    kinds = {"ls": L.KIND_LS, "magls": L.KIND_MAGLS, "magls2d": L.KIND_MAGLS_2D, "emagls": L.KIND_EMAGLS, "emagls2": L.KIND_EMAGLS2,
             "emainch": L.KIND_EMA_CH, "emainsh": L.KIND_EMA_SH}
    if kind not in kinds:
        raise ValueError("kind must be one of %s" % sorted(kinds))
    b, cplx = _basis(shDefinition)
    hL = np.asfortranarray(hL, dtype=np.float64)
    hR = np.asfortranarray(hR, dtype=np.float64)
    if hL.ndim != 3 or hL.shape != hR.shape:
        raise ValueError("hL / hR must be equal-shaped [numSamples x numDirections x numSets] arrays")
    n, D, nsets = hL.shape
    azi, pa = _vec(hrirGridAziRad, D, "hrirGridAziRad")
    zen, pz = (None, None) if hrirGridZenRad is None else _vec(hrirGridZenRad, D, "hrirGridZenRad")
    arr = kind in ("emagls", "emagls2", "emainch", "emainsh")
    micAzi, pma = _vec(micGridAziRad) if arr else (None, None)
    micZen, pmz = (None, None) if (not arr or micGridZenRad is None) else _vec(micGridZenRad, micAzi.size, "micGridZenRad")
    N = int(order)
    C_ = {"ls": (N + 1) ** 2, "magls": (N + 1) ** 2, "magls2d": 2 * N + 1, "emagls": (N + 1) ** 2, "emainch": 2 * N + 1, "emainsh": (N + 1) ** 2}.get(kind)
    if kind == "emagls2":
        C_ = micAzi.size
    rows = n if kind == "ls" else int(len)
    dt = np.complex128 if cplx else np.float64      # (complex SH definition: complex filters for every kind, eMagLS2 included)
    wL = np.zeros((rows, C_, nsets), dtype=dt, order="F")
    wR = np.zeros((rows, C_, nsets), dtype=dt, order="F")
    L.check(L.load().emagls_design_hrir_sets(kinds[kind], hL.ctypes.data, hR.ctypes.data, n, D, nsets, pa, pz, float(micRadius), pma, pmz,
                                             micAzi.size if arr else 0, N, float(fs), int(len), b, wL.ctypes.data, wR.ctypes.data))
    return wL, wR


def fromAtfHrirSets(hL, hR, hrirGridAziZenRad, atfIrs, atfGridAziZenRad, fs, filterLen, fTrans):
    """getEMagLsFiltersFromAtf (lib/getEMagLsFiltersFromAtf.m:1) for every HRIR set (subject) of hL, hR [numSamples x
    numDirections x numSets] on ONE ATF set, as one call (emagls_from_atf_hrir_sets): the ATF set is uploaded once and its side
    computed once per batch of up to 16 subjects.  Returns wL, wR [filterLen x numMics x numSets], meanGridDevDeg."""
    hL = np.asfortranarray(hL, dtype=np.float64)
    hR = np.asfortranarray(hR, dtype=np.float64)
    if hL.ndim != 3 or hL.shape != hR.shape:
        raise ValueError("hL / hR must be equal-shaped [numSamples x numDirections x numSets] arrays")
    n, D, nsets = hL.shape
    hg = np.asarray(hrirGridAziZenRad, dtype=np.float64)
    ag = np.asarray(atfGridAziZenRad, dtype=np.float64)
    atf = np.asfortranarray(atfIrs, dtype=np.float64)
    taps, M, Da = atf.shape
    azi, pa = _vec(hg[:, 0], D, "hrirGridAziZenRad(:,1)")
    zen, pz = _vec(hg[:, 1], D, "hrirGridAziZenRad(:,2)")
    aazi, paa = _vec(ag[:, 0], Da, "atfGridAziZenRad(:,1)")
    azen, paz = _vec(ag[:, 1], Da, "atfGridAziZenRad(:,2)")
    wL = np.zeros((int(filterLen), M, nsets), dtype=np.float64, order="F")
    wR = np.zeros((int(filterLen), M, nsets), dtype=np.float64, order="F")
    dev = C.c_double(0.0)
    L.check(L.load().emagls_from_atf_hrir_sets(hL.ctypes.data, hR.ctypes.data, n, D, nsets, pa, pz, atf.ctypes.data, taps, M, Da, paa, paz, float(fs),
                                               int(filterLen), float(fTrans), wL.ctypes.data, wR.ctypes.data, C.byref(dev)))
    return wL, wR, dev.value


def getEMagLsFiltersEMAinCH(hL, hR, hrirGridAziRad, hrirGridZenRad, micRadius, micGridAziRad, order, fs, len,
                            shDefinition="real", shFunction=None, chFunction=None):
    """lib/getEMagLsFiltersEMAinCH.m:1-2: eMagLS filters in circular harmonics for an equatorial microphone array;
    returns [len x (2*order+1)] per ear, channels ordered [C_0, C_-1, C_1, ..., C_-N, C_N] (dependencies/getCH.m)."""
    if chFunction is not None or shFunction is not None:
        raise NotImplementedError("custom chFunction / shFunction handles are not supported for the EMA variant; the defaults "
                                  "@getCH / @getSH are built in")
    b, cplx = _basis(shDefinition)
    hL, hR, pL, pR = _hrirs(hL, hR)
    n, D = hL.shape
    azi, pa = _vec(hrirGridAziRad, D, "hrirGridAziRad")
    zen, pz = _vec(hrirGridZenRad, D, "hrirGridZenRad")
    micAzi, pma = _vec(micGridAziRad)
    C_ = 2 * int(order) + 1
    wL, pwL = _out(int(len), C_, cplx)
    wR, pwR = _out(int(len), C_, cplx)
    L.check(L.load().emagls_get_emagls_filters_ema_in_ch(pL, pR, n, D, pa, pz, float(micRadius), pma, micAzi.size, int(order),
                                                         float(fs), int(len), b, pwL, pwR))
    return wL, wR


def getEMagLsFiltersEMAinSH(hL, hR, hrirGridAziRad, hrirGridZenRad, micRadius, micGridAziRad, order, fs, len,
                            shDefinition="real", shFunction=None, chFunction=None):
    """lib/getEMagLsFiltersEMAinSH.m:1-2: eMagLS filters in spherical harmonics for an equatorial microphone array (the
    horizontal sound field is expanded from circular to spherical harmonics and rotated to every HRIR direction's elevation);
    returns [len x (order+1)^2] per ear."""
    if chFunction is not None or shFunction is not None:
        raise NotImplementedError("custom chFunction / shFunction handles are not supported for the EMA variants; the defaults "
                                  "@getCH / @getSH are built in")
    b, cplx = _basis(shDefinition)
    hL, hR, pL, pR = _hrirs(hL, hR)
    n, D = hL.shape
    azi, pa = _vec(hrirGridAziRad, D, "hrirGridAziRad")
    zen, pz = _vec(hrirGridZenRad, D, "hrirGridZenRad")
    micAzi, pma = _vec(micGridAziRad)
    C_ = (int(order) + 1) ** 2
    wL, pwL = _out(int(len), C_, cplx)
    wR, pwR = _out(int(len), C_, cplx)
    L.check(L.load().emagls_get_emagls_filters_ema_in_sh(pL, pR, n, D, pa, pz, float(micRadius), pma, micAzi.size, int(order),
                                                         float(fs), int(len), b, pwL, pwR))
    return wL, wR


def getEMagLsFiltersFromAtf(hL, hR, hrirGridAziZenRad, atfIrs, atfGridAziZenRad, fs, filterLen, fTrans, verbose=True):
    hL, hR, pL, pR = _hrirs(hL, hR)
    n, D = hL.shape
    hg = np.asarray(hrirGridAziZenRad, dtype=np.float64)
    ag = np.asarray(atfGridAziZenRad, dtype=np.float64)
    azi, pa = _vec(hg[:, 0], D, "hrirGridAziZenRad")
    zen, pz = _vec(hg[:, 1], D, "hrirGridAziZenRad")
    atf, patf = _f(atfIrs)
    if atf.ndim != 3:
        raise ValueError("atfIrs must be [taps x numMics x numDirections]")
    taps, M, Da = atf.shape
    aazi, paa = _vec(ag[:, 0], Da, "atfGridAziZenRad")
    azen, paz = _vec(ag[:, 1], Da, "atfGridAziZenRad")
    wL, pwL = _out(int(filterLen), M, False)
    wR, pwR = _out(int(filterLen), M, False)
    dev = C.c_double(0.0)
    L.check(L.load().emagls_get_emagls_filters_from_atf(pL, pR, n, D, pa, pz, patf, taps, M, Da, paa, paz, float(fs),
                                                        int(filterLen), float(fTrans), pwL, pwR, C.byref(dev)))
    if verbose:  # the reference prints this line (lib/getEMagLsFiltersFromAtf.m:96)
        print("Matching HRTF and ATF grids, average grid deviation: %.5g deg" % dev.value)
    return wL, wR


def _layout(domain):
    key = str(domain).lower()
    if key not in L.LAYOUT:
        raise ValueError("rotation domain must be 'sh' or 'ch'")
    return L.LAYOUT[key]


def rotateYaw(sig, angleRad, shDefinition="real", domain="sh"):
    """Yaw rotation of an SH (ACN, (N+1)^2 channels) or CH ([C_0, C_-1, C_1, ..., C_-N, C_N], 2N+1 channels) signal
    [numSamples x numChannels]: the yaw part of the rotateHOA_N3D call in dependencies/binauralDecode.m:27-31, own
    specification.  The signal of a plane wave from azimuth a, conj(getSH(N, [a zen], shDefinition))
    or conj(getCH(N, a, shDefinition)), becomes the one of the plane wave from a + angleRad.  angleRad: a scalar, or one angle
    per sample.  The result is complex when the signal is or the basis is 'complex', real otherwise."""
    b, cb = _basis(shDefinition)
    lay = _layout(domain)
    in_c = np.iscomplexobj(sig)
    x = np.asfortranarray(np.asarray(sig, dtype=np.complex128 if in_c else np.float64))
    if x.ndim != 2:
        raise ValueError("sig must be [numSamples x numChannels]")
    n, Cc = x.shape
    yaw = np.ascontiguousarray(np.asarray(angleRad, dtype=np.float64).reshape(-1))
    if yaw.size not in (1, n):
        raise ValueError("angleRad must be a scalar or have one angle per sample (%d), not %d" % (n, yaw.size))
    out, po = _out(n, Cc, in_c or cb)
    L.check(L.load().emagls_rotate_yaw(x.ctypes.data_as(C.c_void_p), 1 if in_c else 0, n, Cc, lay, b,
                                       yaw.ctypes.data_as(C.c_void_p), yaw.size, po))
    return out


def _angles(a, n, name):
    """None, or a contiguous float64 vector of one angle or one angle per sample (n)."""
    if a is None:
        return None
    v = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    if v.size not in (1, n):
        raise ValueError("%s must be a scalar or have one angle per sample (%d), not %d" % (name, n, v.size))
    return v


def _sh_order(Cc):
    N = int(round(math.sqrt(Cc))) - 1
    if N < 0 or (N + 1) ** 2 != Cc:
        raise ValueError("the three-axis rotation needs (N+1)^2 SH channels in ACN order, not %d" % Cc)
    return N


def _vp(v):
    return (v.ctypes.data_as(C.c_void_p), v.size) if v is not None else (None, 0)


def rotateSH(sig, yawRad=0.0, pitchRad=0.0, rollRad=0.0, shDefinition="real"):
    """Three-axis rotation of an SH signal [numSamples x (N+1)^2] (ACN), N <= 15: rotateHOA_N3D(in, yaw, pitch, roll) of
    dependencies/binauralDecode.m:27-31, own specification.  R = Rz(yaw) Ry(pitch) Rx(roll) with getSH's
    axes (x front, y left, z up); the signal of a plane wave from u, conj(getSH(N, u, shDefinition)), becomes the one from R u.
    Each angle: a scalar or one angle per sample.  With pitch and roll all zero this is rotateYaw, bit for bit.  The result is
    complex when the signal is or the basis is 'complex'."""
    b, cb = _basis(shDefinition)
    in_c = np.iscomplexobj(sig)
    x = np.asfortranarray(np.asarray(sig, dtype=np.complex128 if in_c else np.float64))
    if x.ndim != 2:
        raise ValueError("sig must be [numSamples x numChannels]")
    n, Cc = x.shape
    _sh_order(Cc)
    yaw, pitch, roll = _angles(yawRad, n, "yawRad"), _angles(pitchRad, n, "pitchRad"), _angles(rollRad, n, "rollRad")
    out, po = _out(n, Cc, in_c or cb)
    L.check(L.load().emagls_rotate_sh(x.ctypes.data_as(C.c_void_p), 1 if in_c else 0, n, Cc, b, *_vp(yaw), *_vp(pitch), *_vp(roll), po))
    return out


def shRotationMatrix(order, yawRad, pitchRad, rollRad, shDefinition="real"):
    """The matrix M [(N+1)^2 x (N+1)^2] of rotateSH: rotateSH(x, yaw, pitch, roll) == x @ M.T.  Block-diagonal by order, orthogonal
    (real basis) or unitary (complex basis); the closed form of an SH rotation matrix from angles (getSHrotMtx takes the 3 x 3
    matrix instead).  N <= 15."""
    b, cb = _basis(shDefinition)
    if int(order) != order or order < 0:
        raise ValueError("order must be a non-negative integer")
    Cc = (int(order) + 1) ** 2
    out, po = _out(Cc, Cc, cb)
    L.check(L.load().emagls_sh_rotation_matrix(int(order), b, float(yawRad), float(pitchRad), float(rollRad), po))
    return out


def _rate(v, name):
    """A sample rate or resampling factor as MATLAB's resample takes it: a positive integer value (int or integer-valued float)."""
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError("%s must be a positive integer, not %r" % (name, v)) from None
    if not math.isfinite(f) or f < 1 or f != math.floor(f) or f > 9e15:
        raise ValueError("%s must be a positive integer, not %r" % (name, v))
    return int(f)


def _resampled_length(n, p, q):
    return -(-n * p // q)


def resample(x, p, q):
    """MATLAB's resample(x, p, q) with its defaults N = 10, bta = 5 (Signal Processing Toolbox; called by
    dependencies/binauralDecode.m:15,21-22), on the GPU.  Own restatement of resample.m: a Kaiser-windowed
    sinc of 20 max(p, q) + 1 taps, polyphase, with resample.m's alignment; MATLAB's exact tap values are not pinned.  p and q:
    positive integers (reduced by their gcd; max(p, q) <= 65536 after that).  x: a vector (1-D, or a 1 x n row) is resampled along
    its length, a matrix [numSamples x numChannels] per column; real or complex.  The result has ceil(numSamples * p / q) samples
    and x's shape otherwise."""
    p, q = _rate(p, "p"), _rate(q, "q")
    a = np.asarray(x)
    cplx = np.iscomplexobj(a)
    a = a.astype(np.complex128 if cplx else np.float64, copy=False)
    if a.ndim > 2:
        raise ValueError("x must be a vector or a [numSamples x numChannels] matrix")
    row = a.ndim == 2 and a.shape[0] == 1
    m = a.reshape(-1, 1) if a.ndim < 2 else (a.reshape(-1, 1) if row else a)
    m = np.asfortranarray(m)
    n, Cc = m.shape
    ny = _resampled_length(n, p, q)
    out, po = _out(ny, Cc, cplx)
    if n and Cc:
        L.check(L.load().emagls_resample(m.ctypes.data_as(C.c_void_p), 1 if cplx else 0, n, Cc, p, q, po))
    if a.ndim < 2:
        return out.reshape(-1)
    return out.reshape(1, -1) if row else out


def binauralDecode(sig, inFs, decodingFilterLeft, decodingFilterRight, decodingFilterFs, compensateDelay=False,
                   signal=None, signalFs=None, horRotAngleRad=None, *, shDefinition="real", rotationDomain="sh", pitchRad=None,
                   rollRad=None, allowResampling=False):
    """dependencies/binauralDecode.m:1-64.  The resampling of :12-23 (decodingFilterFs or signalFs != inFs; the rates then
    positive integers) runs only with allowResampling=True, because its taps are our restatement of MATLAB's resample (see
    `resample`), not checked against MATLAB; without it such a call raises NotImplementedError.  It runs on the device before
    everything else, and compensateDelay then cuts half the resampled filters' length.  Real or complex (complex-SH) signals and filters; the output
    is real: the reference forces it and warns with the absolute sum of the discarded imaginary part (:59-64), and so does this
    function.  horRotAngleRad: a scalar (the reference's fixed yaw) or one angle per input sample (a head-tracker trajectory),
    applied as rotateYaw(sig, horRotAngleRad, shDefinition, rotationDomain); shDefinition is the basis of `sig` ('real' is the
    one rotateHOA_N3D assumes).  signal: the dry source the rendered impulse response is convolved with (:44-48); only its
    first column is used, and the output then has as many samples as it.  pitchRad, rollRad: the other two angles of
    rotateHOA_N3D (rotateSH's rotation with yaw = horRotAngleRad), each a scalar or one angle per input sample; SH signals only.
    With both None, or all zero, the call is the yaw-only one, bit for bit."""
    import warnings
    rs_filter = decodingFilterFs != inFs
    rs_signal = signal is not None and signalFs is not None and signalFs != inFs
    if (rs_filter or (signalFs is not None and signalFs != inFs)) and not allowResampling:
        raise NotImplementedError("resampling (decodingFilterFs or signalFs != inFs) is outside the accelerated path unless "
                                  "allowResampling=True")
    fs = None
    if rs_filter or rs_signal:
        fs = (_rate(inFs, "inFs"), _rate(decodingFilterFs, "decodingFilterFs"), _rate(signalFs, "signalFs") if rs_signal else _rate(inFs, "inFs"))
    in_c = np.iscomplexobj(sig)
    w_c = np.iscomplexobj(decodingFilterLeft) or np.iscomplexobj(decodingFilterRight)

    def arr(a, cplx):
        a = np.asfortranarray(np.asarray(a, dtype=np.complex128 if cplx else np.float64))
        return a, a.ctypes.data_as(C.c_void_p)

    sig, ps = arr(sig, in_c)
    wL, pwL = arr(decodingFilterLeft, w_c)
    wR, pwR = arr(decodingFilterRight, w_c)
    n, Cc = sig.shape
    ln = wL.shape[0]
    if wL.shape != wR.shape or wL.shape[1] != Cc:
        raise ValueError("filters must be [len x numChannels] matching the signal's channel count")
    yaw = None
    if horRotAngleRad is not None:
        yaw = np.ascontiguousarray(np.asarray(horRotAngleRad, dtype=np.float64).reshape(-1))
        if yaw.size == 1 and yaw[0] == 0:      # :28: `horRotAngleRad ~= 0`
            yaw = None
        elif yaw.size not in (1, n):
            raise ValueError("horRotAngleRad must be a scalar or have one angle per input sample (%d), not %d" % (n, yaw.size))
    src = None
    if signal is not None:
        s = np.asarray(signal)
        if s.size:
            if np.iscomplexobj(s):
                raise ValueError("signal must be real")
            src = np.ascontiguousarray((s.reshape(s.shape[0], -1)[:, 0] if s.ndim > 1 else s.reshape(-1)).astype(np.float64))
    if fs is not None and fs[2] != fs[0] and src is not None:
        print("binauralDecode: resampling signal")                 # :14 (the resampled signal, then its first column)
    if fs is not None and fs[1] != fs[0]:
        print("binauralDecode: resampling decoding filter")        # :20
        ln = _resampled_length(ln, fs[0] // math.gcd(fs[0], fs[1]), fs[1] // math.gcd(fs[0], fs[1]))
    ypr = None
    if pitchRad is not None or rollRad is not None:
        pitch, roll = _angles(pitchRad, n, "pitchRad"), _angles(rollRad, n, "rollRad")
        if any(a is not None and np.any(a != 0) for a in (pitch, roll)):
            if _layout(rotationDomain) != L.LAYOUT["sh"]:
                raise ValueError("a CH signal can only be turned about z: pitchRad and rollRad must be 0")
            _sh_order(Cc)
            ypr = (pitch, roll)
    skip = (ln // 2 - 1) if (compensateDelay and ln // 2 > 0) else 0
    b, lay = L.BASIS["real"], L.LAYOUT["sh"]     # (not looked at without rotation and signal)
    if ypr is not None or yaw is not None or src is not None:
        b = _basis(shDefinition)[0]
        lay = _layout(rotationDomain)
    pitch, roll = ypr or (None, None)
    nout = src.size if src is not None else n
    if fs is not None and src is not None:
        nout = _resampled_length(nout, fs[0] // math.gcd(fs[0], fs[2]), fs[2] // math.gcd(fs[0], fs[2]))
    out, po = _out(max(nout - skip, 0), 2, False)
    im = (C.c_double * 2)(0.0, 0.0)
    lnf = wL.shape[0]     # (the filters' length before the resampling; ln is the one after it)
    if fs is None:
        L.check(L.load().emagls_binaural_decode_render_ypr(
            ps, 1 if in_c else 0, n, Cc, pwL, pwR, 1 if w_c else 0, lnf, 1 if compensateDelay else 0, lay, b, *_vp(yaw), *_vp(pitch),
            *_vp(roll), *_vp(src), po, im))
    else:
        L.check(L.load().emagls_binaural_decode_render_fs(
            ps, 1 if in_c else 0, n, Cc, pwL, pwR, 1 if w_c else 0, lnf, 1 if compensateDelay else 0, lay, b, *_vp(yaw), *_vp(pitch),
            *_vp(roll), *_vp(src), float(fs[0]), float(fs[1]), float(fs[2]), po, im))
    # binauralDecode.m:59-63: `if ~isreal(binauralOut)` -- whenever the accumulated result is a complex array, which it is as
    # soon as a signal or a filter is complex (MATLAB only drops an all-zero imaginary part at the end of an arithmetic
    # operation; a sum that happens to be exactly real is the one case in which the reference stays silent, and so do we)
    if im[0] != 0.0 or im[1] != 0.0:
        warnings.warn("discarding imaginary part with sum of [%.2g, %.2g] in rendering result." % (im[0], im[1]))
    return out


def _encoder(encoder, numChannels):
    """encoder [numChannels x numMics] as a column-major array, its pointer, whether it is complex, and numMics."""
    e_c = np.iscomplexobj(encoder)
    enc = np.asfortranarray(np.asarray(encoder, dtype=np.complex128 if e_c else np.float64))
    if enc.ndim != 2 or enc.shape[0] != numChannels:
        raise ValueError("encoder must be [numChannels x numMics] with the filters' channel count (%d) of rows" % numChannels)
    return enc, enc.ctypes.data_as(C.c_void_p), e_c, enc.shape[1]


def _real_mic_block(is_complex, what):
    if is_complex:
        raise L.EmaglsError(L.ERR_ARG, "an encoded %s takes real microphone blocks" % what)


_ANGLE_NAMES = ("horRotAngleRad", "pitchRad", "rollRad")


class _BlockStreamObject:
    """What the block-stream objects share: the handle's life, the NumPy-or-torch dispatch of a push, the block-multiple check,
    the set indices of a push into a bank and the frame of a torch push.  A subclass names itself (_kind) and its C destroy entry
    (_destroy), sets blockSize and numSets and has _push_numpy(h, block, ...), _push_torch(h, block, ...) and
    _shape_sets(a, nb, xp)."""

    _h = None

    def _handle(self):
        if self._h is None:
            raise ValueError("the %s is closed" % self._kind)
        return self._h

    def _check_multiple(self, n):
        if n % self.blockSize:
            raise ValueError("block must have a multiple of blockSize (%d) samples, not %d" % (self.blockSize, n))
        return n

    def _set_index(self, setIndex, n, device=None):
        """setIndex in the shape of the push, as int32 (None: None): a host array checked against the bank or, with `device`, a
        tensor there.  A tensor that is given is not read on the host."""
        if setIndex is None:
            return None
        nb = n // self.blockSize
        if device is not None:
            import torch
            if torch.is_tensor(setIndex):
                if setIndex.dtype != torch.int32:
                    raise ValueError("a setIndex tensor must be int32")
                return self._shape_sets(setIndex.to(device=device), nb, torch).contiguous()
        a = np.asarray(setIndex)
        if a.dtype.kind not in "iu":
            raise ValueError("setIndex must be an integer or integers")
        a = self._shape_sets(a, nb, np)
        if a.size and (a.min() < 0 or a.max() >= self.numSets):
            raise ValueError("setIndex must lie in [0, numSets - 1] = [0, %d]" % (self.numSets - 1))
        a = np.ascontiguousarray(a, dtype=np.int32)
        return a if device is None else torch.as_tensor(a, device=device)

    def push(self, block, *args):
        h = self._handle()
        if type(block).__module__.split(".")[0] == "torch":
            return self._push_torch(h, block, *args)
        return self._push_numpy(h, block, *args)

    @staticmethod
    def _need_gpu(block):
        if not block.is_cuda:
            raise ValueError("a torch block must be on the GPU (pass a NumPy array for the host entry)")

    @staticmethod
    def _on_current_stream(block, inputs, call):
        """call(stream) on torch's current stream of the block's device, not synchronised."""
        import torch
        with torch.cuda.device(block.device):
            call(C.c_void_p(torch.cuda.current_stream().cuda_stream))
        for t in inputs:      # (their memory may be reused only after the stream has passed the enqueued kernels)
            if t is not None:
                t.record_stream(torch.cuda.current_stream(block.device))

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            L.check(getattr(L.load(), self._destroy)(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _DecodeObject(_BlockStreamObject):
    """What BinauralDecodeStream and BinauralDecodeGroup share, which is the library's one object behind both: the filters and the
    encoder of the creation, the checks of a pushed block, and the host and the torch push.  A subclass names
    its kind (_what) and the C entries it calls (_create, _create_encoded, _push, _push_device, _destroy), shapes the angles and
    the set indices of a push (_shape_angles, _shape_sets) and makes the output (_new_out)."""

    _kind = property(lambda self: "decode " + self._what)

    def __init__(self, decodingFilterLeft, decodingFilterRight, blockSize, shDefinition, rotationDomain, complexInput, encoder,
                 numListeners=None):
        self._basis, self._cb = _basis(shDefinition)
        self._layout = _layout(rotationDomain)
        w_c = np.iscomplexobj(decodingFilterLeft) or np.iscomplexobj(decodingFilterRight)
        wL = np.asfortranarray(np.asarray(decodingFilterLeft, dtype=np.complex128 if w_c else np.float64))
        wR = np.asfortranarray(np.asarray(decodingFilterRight, dtype=np.complex128 if w_c else np.float64))
        if wL.ndim not in (2, 3) or wL.shape != wR.shape:
            raise ValueError("filters must be [len x numChannels] or [numSets x len x numChannels] arrays of equal shape")
        if int(blockSize) != blockSize or (numListeners is not None and int(numListeners) != numListeners):
            raise ValueError("blockSize must be an integer" if numListeners is None else "blockSize and numListeners must be integers")
        self.numSets = wL.shape[0] if wL.ndim == 3 else 1
        if self.numSets < 1:
            raise ValueError("a bank needs at least one filter set")
        if wL.ndim == 3:    # the library takes the sets one after the other, each column-major [len x numChannels]
            wL, wR = (np.ascontiguousarray(w.transpose(0, 2, 1)) for w in (wL, wR))
            ln, self.numChannels = wL.shape[2], wL.shape[1]
        else:
            ln, self.numChannels = wL.shape
        self.blockSize, self.complexInput = int(blockSize), bool(complexInput)
        listeners = ()
        if numListeners is not None:
            self.numListeners = int(numListeners)
            listeners = (self.numListeners,)
        self.numMics = None
        h = C.c_void_p()
        filters = (wL.ctypes.data_as(C.c_void_p), wR.ctypes.data_as(C.c_void_p), 1 if w_c else 0, ln)
        if encoder is not None:
            if complexInput:
                raise ValueError("an encoded %s takes real microphone blocks: complexInput must be False" % self._what)
            enc, pe, e_c, self.numMics = _encoder(encoder, self.numChannels)
            L.check(getattr(L.load(), self._create_encoded)(self.numMics, pe, 1 if e_c else 0, self.numChannels, self.numSets, *filters,
                                                            self._layout, self._basis, self.blockSize, *listeners, C.byref(h)))
        else:
            L.check(getattr(L.load(), self._create)(self.numChannels, self.numSets, *filters, 1 if complexInput else 0, self._layout,
                                                    self._basis, self.blockSize, *listeners, C.byref(h)))
        self._h = h

    def _check_block(self, shape, ndim):
        if self.numMics is not None:
            if ndim != 2 or shape[1] != self.numMics:
                raise ValueError("block must be [numSamples x numMics] matching the encoder's microphone count (%d)" % self.numMics)
        elif ndim != 2 or shape[1] != self.numChannels:
            raise ValueError("block must be [numSamples x numChannels] matching the filters' channel count (%d)" % self.numChannels)
        return self._check_multiple(shape[0])

    def _check_complex(self, is_complex):
        if self.numMics is not None:
            _real_mic_block(is_complex, self._what)
        if is_complex and not self.complexInput:
            raise ValueError("the %s was created for real blocks (complexInput=False)" % self._what)

    def _check_three_axis(self, turned):
        """turned: the push has a pitch or a roll."""
        if turned:
            if self._layout != L.LAYOUT["sh"]:
                raise ValueError("a CH signal can only be turned about z: pitchRad and rollRad must be 0")
            _sh_order(self.numChannels)

    def _push_numpy(self, h, block, horRotAngleRad, pitchRad, rollRad, setIndex):
        self._check_complex(np.iscomplexobj(block))
        x = np.asfortranarray(np.asarray(block, dtype=np.complex128 if self.complexInput else np.float64))
        n = self._check_block(x.shape, x.ndim)
        given = [None if a is None else np.asarray(a, dtype=np.float64) for a in (horRotAngleRad, pitchRad, rollRad)]
        yaw, pitch, roll = (None if a is None else np.ascontiguousarray(a) for a in self._shape_angles(n, given, np))
        self._check_three_axis(any(a is not None and np.any(a != 0) for a in (pitch, roll)))
        sets = self._set_index(setIndex, n)
        out, result = self._new_out(n, np.zeros)
        L.check(getattr(L.load(), self._push)(h, x.ctypes.data_as(C.c_void_p), n, *_vp(sets), *_vp(yaw), *_vp(pitch), *_vp(roll),
                                              out.ctypes.data_as(C.c_void_p)))
        return result

    def _push_torch(self, h, block, hor, pitch, roll, setIndex):
        import torch
        n = self._check_block(tuple(block.shape), block.dim())
        self._need_gpu(block)
        self._check_complex(block.is_complex())
        xt = block.to(torch.complex128 if self.complexInput else torch.float64).t().contiguous()   # [numChannels][n]: column-major

        def dev(a):
            if a is None:
                return None
            if torch.is_tensor(a):
                return a.to(device=block.device, dtype=torch.float64)
            return torch.as_tensor(np.asarray(a, dtype=np.float64), device=block.device)
        ty, tp, tr = (None if t is None else t.contiguous() for t in self._shape_angles(n, [dev(a) for a in (hor, pitch, roll)], torch))
        count = lambda t: 0 if t is None else t.numel()   # noqa: E731
        self._check_three_axis(count(tp) or count(tr))
        ts = self._set_index(setIndex, n, block.device)
        out, result = self._new_out(n, lambda shape: torch.empty(shape, dtype=torch.float64, device=block.device))
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
        self._on_current_stream(block, (xt, ty, tp, tr, ts), lambda st: L.check(getattr(L.load(), self._push_device)(
            h, p(xt), n, p(ts), count(ts), p(ty), count(ty), p(tp), count(tp), p(tr), count(tr), p(out), st)))
        return result


class BinauralDecodeStream(_DecodeObject):
    """binauralDecode a block at a time, for a listener whose head moves while the sound plays.  Created
    once from the decoding filters [len x numChannels] (real or complex); then `push` takes consecutive blocks of the SH (or CH)
    signal, each with the head orientation for that block, and returns the two ear signals of that block, [n x 2].  With x the
    concatenation of the pushed blocks and the angles concatenated per sample, the concatenated outputs equal
    binauralDecode(x, fs, wL, wR, fs, False, horRotAngleRad=yaw, pitchRad=pitch, rollRad=roll, shDefinition=..., rotationDomain=...)
    to rounding: no delay cut (offset your read by len/2 - 1 yourself), no resampling; a dry source signal goes through
    a SourceFieldStream first (whose torch output a push here takes as it lies); for complex signals or
    filters the output is the real part and the discarded imaginary sum is not reported.
    blockSize: a power of two from 64 to 2048.  complexInput: the pushed blocks are complex.  Uniformly partitioned overlap-save
    with its state on the GPU; `info` gives block, partitions, state_bytes, filter_bytes and launches_per_block.
    A bank: filters [numSets x len x numChannels] make a stream of `numSets` filter sets, and `push`
    takes a set index per block.  A change of set is cross-faded over the block that changes: its sample i goes to the new set
    with the gain (i + 1) / blockSize and to the old one with the rest; the first block after creation or reset does not fade.
    The outputs equal sum_s binauralDecode(g_s * x, wL[s], wR[s]) with g_s the gain of set s per sample; a constant index gives
    the bits of the plain stream on that set.  For designs on raw microphone signals, which no rotation can turn, a bank of
    one set per head orientation (`designYawBank`, `yawBankIndex`) is what follows the head.
    An encoder: with encoder [numChannels x numMics] (real or complex; `arrayEncoder` makes the usual
    ones) the stream takes blocks of REAL microphone signals [n x numMics] and returns what the plain stream returns for
    block @ encoder.T, with the encoder inside the rotation launch: still three launches per block.  numChannels stays the
    filters' channel count; 1 <= numMics, numChannels <= 64.  A complex encoder makes the stream run as one with complexInput.
    A renderer that never turns needs no encoded stream: fold the encoder into the filters yourself,
    w2 = np.einsum("...tc,cm->...tm", w, encoder), and push the microphone blocks to a plain stream of w2.  The library does not
    do so by itself, because the stream's history would change domain between a push with angles and one without."""

    _what = "stream"
    _create, _create_encoded, _push, _push_device, _destroy = (
        "emagls_decode_stream_" + e for e in ("create_bank", "create_encoded", "push_sets", "push_sets_device", "destroy"))

    def __init__(self, decodingFilterLeft, decodingFilterRight, blockSize, shDefinition="real", rotationDomain="sh", complexInput=False,
                 encoder=None):
        super().__init__(decodingFilterLeft, decodingFilterRight, blockSize, shDefinition, rotationDomain, complexInput, encoder)

    @property
    def info(self):
        b, p, sb, fb, nl = L.c_i64(0), L.c_i64(0), L.c_i64(0), L.c_i64(0), C.c_int(0)
        L.check(L.load().emagls_decode_stream_info(self._handle(), C.byref(b), C.byref(p), C.byref(sb), C.byref(fb), C.byref(nl)))
        return {"block": b.value, "partitions": p.value, "state_bytes": sb.value, "filter_bytes": fb.value, "launches_per_block": nl.value}

    def _shape_angles(self, n, angles, xp):
        """The argument errors of binauralDecode, in its wording; each angle as a vector of 1 or n values."""
        for a, name in zip(angles, _ANGLE_NAMES):
            if a is not None and math.prod(a.shape) not in (1, n):
                raise ValueError("%s must be a scalar or have one angle per input sample (%d), not %d" % (name, n, math.prod(a.shape)))
        return [None if a is None else a.reshape(-1) for a in angles]

    def _shape_sets(self, a, nb, xp):
        a = a.reshape(-1)
        if math.prod(a.shape) not in (1, nb):
            raise ValueError("setIndex must be an integer or have one index per block (%d), not %d" % (nb, math.prod(a.shape)))
        return a

    def _new_out(self, n, new):
        out = new((2, n))   # the library's column-major [n x 2]
        return out, out.T

    def push(self, block, horRotAngleRad=None, pitchRad=None, rollRad=None, setIndex=None):
        """block [n x numChannels], n a multiple of blockSize: a NumPy array (host entry; returns a NumPy array), or a torch tensor
        on the stream's device (device entry on torch's current stream, not synchronised; returns a torch tensor).  Each angle:
        None (0), a scalar (constant over this push) or one value per sample; with torch blocks also device tensors.
        setIndex: None (every block keeps the set of the block before it; set 0 on a fresh stream), an int (every block of this
        push) or one int per block; with torch blocks also a device int32 tensor, which is not read on the host: the kernels then
        clamp its values into [0, numSets - 1]."""
        return super().push(block, horRotAngleRad, pitchRad, rollRad, setIndex)

    def reset(self):
        """Zero history: what follows equals a fresh stream bit for bit."""
        L.check(L.load().emagls_decode_stream_reset(self._handle()))


class BinauralDecodeGroup(_DecodeObject):
    """Many listeners of one sound field in one push: one bank of filter sets, stored once, and
    `numListeners` listeners, each with the state a BinauralDecodeStream has.  `push` takes one block of the common signal and, per
    listener, their head orientation and their set index, and returns [numListeners x n x 2].  Listener l's output is, bit for bit,
    what a BinauralDecodeStream of the same filters returns when it is fed the same blocks with listener l's angles and indices;
    a block costs at most three kernel launches for the whole group.  One choice is made per push rather than per listener: the
    push takes the yaw rule when no listener has a pitch or a roll, otherwise every listener goes through the three-axis rotation.
    Filters [len x numChannels] or [numSets x len x numChannels]; everything else as BinauralDecodeStream.  1 <= numListeners <= 4096.
    With encoder [numChannels x numMics] the common block is one of real microphone signals [n x numMics], encoded inside the
    rotation launch: listener l equals, bit for bit, an encoded BinauralDecodeStream of its own."""

    _what = "group"
    _create, _create_encoded, _push, _push_device, _destroy = (
        "emagls_decode_group_" + e for e in ("create", "create_encoded", "push", "push_device", "destroy"))

    def __init__(self, decodingFilterLeft, decodingFilterRight, blockSize, numListeners, shDefinition="real", rotationDomain="sh",
                 complexInput=False, encoder=None):
        super().__init__(decodingFilterLeft, decodingFilterRight, blockSize, shDefinition, rotationDomain, complexInput, encoder,
                         numListeners=numListeners)

    def info(self):
        b, p, nl, sb, fb, k = L.c_i64(0), L.c_i64(0), L.c_i64(0), L.c_i64(0), L.c_i64(0), C.c_int(0)
        L.check(L.load().emagls_decode_group_info(self._handle(), C.byref(b), C.byref(p), C.byref(nl), C.byref(sb), C.byref(fb), C.byref(k)))
        return {"block": b.value, "partitions": p.value, "listeners": nl.value, "state_bytes": sb.value, "filter_bytes": fb.value,
                "launches_per_block": k.value}

    def _per_listener(self, a, per, name, what, xp):
        """An argument of push as [L] or [L x per]: a scalar is the same for every listener."""
        nl = self.numListeners
        shape = tuple(a.shape)
        if len(shape) == 0 or (len(shape) == 1 and shape[0] == 1):
            return xp.broadcast_to(a.reshape(1), (nl,))
        if shape == (nl,) or shape == (nl, 1):
            return a.reshape(nl)
        if shape == (nl, per):
            return a
        if nl == 1 and shape == (per,):
            return a.reshape(1, per)
        raise ValueError("%s must be a scalar, [numListeners] or [numListeners x %s] = [%d x %d], not %s" % (name, what, nl, per, list(shape)))

    def _shape_angles(self, n, angles, xp):
        return [None if a is None else self._per_listener(a, n, name, "n", xp) for a, name in zip(angles, _ANGLE_NAMES)]

    def _shape_sets(self, a, nb, xp):
        return self._per_listener(a, nb, "setIndex", "n / blockSize", xp)

    def _new_out(self, n, new):
        out = new((self.numListeners, 2, n))
        return out, out.swapaxes(1, 2)

    def push(self, block, horRotAngleRad=None, pitchRad=None, rollRad=None, setIndex=None):
        """block [n x numChannels], the common signal, n a multiple of blockSize: a NumPy array (host entry) or a torch tensor on
        the group's device (device entry on torch's current stream, not synchronised).  Each angle: None (0), a scalar (every
        listener), [numListeners] (constant over this push) or [numListeners x n].  setIndex: None (every listener keeps their
        set; set 0 on a fresh listener), an int (every listener), [numListeners] or [numListeners x n / blockSize]; a device int32
        tensor is not read on the host: the kernels then clamp its values into [0, numSets - 1].
        Returns [numListeners x n x 2]."""
        return super().push(block, horRotAngleRad, pitchRad, rollRad, setIndex)

    def reset(self, listener=None):
        """Zero history for one listener (what a listener who joins gets; the others are untouched) or, with None, for all: what
        follows equals a fresh stream bit for bit."""
        L.check(L.load().emagls_decode_group_reset(self._handle(), -1 if listener is None else int(listener)))


class SourceFieldStream(_BlockStreamObject):
    """Dry source signals through array room responses, a block at a time: what the reference's harness
    does offline with fftfilt(srir.rir, sig) (testEMagLs.m:66-70), for a head that moves while the sound plays.  Created once from
    rirs [nr x numChannels] (one source) or [numSources x nr x numChannels], real or complex, and a block size (a power of two
    from 64 to 2048); `push` takes consecutive blocks of the real source signals and returns the field block [n x numChannels].
    With s_q everything pushed for source q, the concatenated outputs equal sum_q fftfilt(rirs[q][:, c], s_q) to rounding; nothing
    is held back.  A complex response gives complex output: feed it to a stream created with complexInput=True.
    The output of a torch push lies as BinauralDecodeStream.push and BinauralDecodeGroup.push read their block: they take it
    without a copy, and the chain source -> room -> rotation -> filters runs on the device without a host synchronisation.
    numSources <= 16, numChannels <= 256, nr <= 1048576, response spectra <= 4 GiB; `info` gives block, partitions, state_bytes,
    response_bytes and launches_per_block.
    A bank, for sources that move: rirs [numSets x numSources x nr x numChannels] make a stream of
    `numSets` response sets, and `push` takes a set index per source and block.  A change of set is cross-faded over the block that
    changes: its sample i goes to the new set with the gain (i + 1) / blockSize and to the old one with the rest; the first block
    after creation or reset does not fade.  The outputs equal sum_q sum_s fftfilt(rirs[s][q][:, c], g_sq * s_q) with g_sq the gain
    of set s per sample of source q; a constant index gives the bits of the plain stream on that set.  numSets <= 65536, and the
    4 GiB hold for the whole bank."""

    _kind, _destroy = "field stream", "emagls_field_stream_destroy"

    def __init__(self, rirs, blockSize):
        r_c = np.iscomplexobj(rirs)
        r = np.asarray(rirs, dtype=np.complex128 if r_c else np.float64)
        if r.ndim == 2:
            r = r[None]
        if r.ndim == 3:
            r = r[None]
        if r.ndim != 4:
            raise ValueError("rirs must be [nr x numChannels], [numSources x nr x numChannels] or [numSets x numSources x nr x numChannels]")
        if int(blockSize) != blockSize:
            raise ValueError("blockSize must be an integer")
        self.numSets, self.numSources, nr, self.numChannels = r.shape
        if self.numSets < 1:
            raise ValueError("a bank needs at least one response set")
        self.blockSize, self.complexOutput = int(blockSize), bool(r_c)
        r = np.ascontiguousarray(r.transpose(0, 1, 3, 2))   # set by set the sources one after the other, each column-major [nr x numChannels]
        h = C.c_void_p()
        L.check(L.load().emagls_field_stream_create_bank(self.numSources, self.numChannels, self.numSets, r.ctypes.data_as(C.c_void_p),
                                                         1 if r_c else 0, nr, self.blockSize, C.byref(h)))
        self._h = h

    @property
    def info(self):
        b, p, sb, rb, nl = L.c_i64(0), L.c_i64(0), L.c_i64(0), L.c_i64(0), C.c_int(0)
        L.check(L.load().emagls_field_stream_info(self._handle(), C.byref(b), C.byref(p), C.byref(sb), C.byref(rb), C.byref(nl)))
        return {"block": b.value, "partitions": p.value, "state_bytes": sb.value, "response_bytes": rb.value, "launches_per_block": nl.value}

    def _check_block(self, shape):
        if len(shape) == 1 and self.numSources == 1:
            shape = (shape[0], 1)
        if len(shape) != 2 or shape[1] != self.numSources:
            raise ValueError("block must be [n] (one source) or [n x numSources] matching the responses' source count (%d)" % self.numSources)
        return self._check_multiple(shape[0])

    def _shape_sets(self, a, nb, xp):
        """setIndex as [numSources] or [numSources x nb]: a scalar is the same for every source."""
        ns = self.numSources
        shape = tuple(a.shape)
        if len(shape) == 0 or (len(shape) == 1 and shape[0] == 1):
            return xp.broadcast_to(a.reshape(1), (ns,))
        if shape == (ns,) or shape == (ns, 1):
            return a.reshape(ns)
        if shape == (ns, nb):
            return a
        if ns == 1 and shape == (nb,):
            return a.reshape(1, nb)
        raise ValueError("setIndex must be a scalar, [numSources] or [numSources x n / blockSize] = [%d x %d], not %s" % (ns, nb, list(shape)))

    def push(self, block, setIndex=None):
        """block [n] or [n x numSources], real, n a multiple of blockSize: a NumPy array (host entry; returns a NumPy array
        [n x numChannels]), or a torch tensor on the stream's device (device entry on torch's current stream, not synchronised;
        returns a tensor [n x numChannels] that is the transposed view of the [numChannels][n] buffer the kernel wrote).
        setIndex: None (every source keeps its set; set 0 on a fresh object), an int (every source), [numSources] (constant over
        this push) or [numSources x n / blockSize]; with torch blocks also a device int32 tensor, which is not read on the host:
        the kernels then clamp its values into [0, numSets - 1]."""
        return super().push(block, setIndex)

    def _push_numpy(self, h, block, setIndex):
        if np.iscomplexobj(block):
            raise ValueError("a field stream takes real source signals")
        x = np.asarray(block, dtype=np.float64)
        n = self._check_block(x.shape)
        x = np.asfortranarray(x.reshape(n, self.numSources))
        sets = self._set_index(setIndex, n)
        out = np.zeros((self.numChannels, n), dtype=np.complex128 if self.complexOutput else np.float64)
        L.check(L.load().emagls_field_stream_push_sets(h, x.ctypes.data_as(C.c_void_p), n, *_vp(sets), out.ctypes.data_as(C.c_void_p)))
        return out.T

    def _push_torch(self, h, block, setIndex):
        import torch
        n = self._check_block(tuple(block.shape))
        self._need_gpu(block)
        if block.is_complex():
            raise ValueError("a field stream takes real source signals")
        xt = block.to(torch.float64).reshape(n, self.numSources).t().contiguous()   # [numSources][n]: column-major
        ts = self._set_index(setIndex, n, block.device)
        out = torch.empty((self.numChannels, n), dtype=torch.complex128 if self.complexOutput else torch.float64, device=block.device)
        self._on_current_stream(block, (xt, ts), lambda st: L.check(L.load().emagls_field_stream_push_sets_device(
            h, C.c_void_p(xt.data_ptr()), n, C.c_void_p(ts.data_ptr()) if ts is not None else None, 0 if ts is None else ts.numel(),
            C.c_void_p(out.data_ptr()), st)))
        return out.t()

    def reset(self):
        """Zero history (and, for a bank, no selection): what follows equals a fresh object bit for bit."""
        L.check(L.load().emagls_field_stream_reset(self._handle()))


def designYawBank(kind, hL, hR, hrirGridAziRad, hrirGridZenRad, yawRad, *, order=4, fs=48000.0, len=512, shDefinition="real",
                  micRadius=0.0, micGridAziRad=None, micGridZenRad=None, atfIrs=None, atfGridAziZenRad=None, fTrans=0.0):
    """A bank of filter sets for BinauralDecodeStream, one per head yaw: set j is the design `kind` on the HRIR grid turned against
    the head, hrirGridAziRad - yawRad[j], one job per angle on the library's job list (jobs.JobList).  kind: 'ls', 'magls'
    (order, fs, len, shDefinition), 'emagls', 'emagls2' (also micRadius, micGridAziRad, micGridZenRad) or 'fromatf' (atfIrs
    [taps x numMics x numAtfDirections], atfGridAziZenRad, fs, len, fTrans).  Returns (wL, wR) of shape
    [len(yawRad) x len x numChannels] ('ls': the HRIRs' length).  The sign is the stream's yaw rule: set j
    renders what turning the sound field by +yawRad[j] and decoding with the set for 0 renders -- for LS filters an identity
    to rounding."""
    from .batch import _out_shape
    from .jobs import JobList
    kinds = {"ls": L.KIND_LS, "magls": L.KIND_MAGLS, "emagls": L.KIND_EMAGLS, "emagls2": L.KIND_EMAGLS2, "fromatf": L.KIND_FROM_ATF}
    if kind not in kinds:
        raise ValueError("kind must be one of %s" % sorted(kinds))
    hL = np.asfortranarray(hL, dtype=np.float64)
    hR = np.asfortranarray(hR, dtype=np.float64)
    if hL.ndim != 2 or hL.shape != hR.shape:
        raise ValueError("hL / hR must be equal-shaped [numSamples x numDirections] arrays")
    azi, _ = _vec(hrirGridAziRad, hL.shape[1], "hrirGridAziRad")
    zen, _ = _vec(hrirGridZenRad, hL.shape[1], "hrirGridZenRad")
    yaw = np.asarray(yawRad, dtype=np.float64).reshape(-1)
    if yaw.size < 1:
        raise ValueError("yawRad must hold at least one angle")
    kw = dict(kind=kinds[kind], basis=shDefinition, order=int(order), fs=float(fs), length=int(len), hL=hL, hR=hR, hrir_zen=zen)
    if kind in ("emagls", "emagls2"):
        if micGridAziRad is None or micGridZenRad is None:
            raise ValueError("kind '%s' needs micRadius, micGridAziRad and micGridZenRad" % kind)
        maz, _ = _vec(micGridAziRad)
        mzn, _ = _vec(micGridZenRad, maz.size, "micGridZenRad")
        kw.update(mic_radius=float(micRadius), mic_azi=maz, mic_zen=mzn)
    if kind == "fromatf":
        if atfIrs is None or atfGridAziZenRad is None:
            raise ValueError("kind 'fromatf' needs atfIrs and atfGridAziZenRad")
        ag = np.asarray(atfGridAziZenRad, dtype=np.float64)
        kw.update(basis="real", order=0, atf=np.asfortranarray(atfIrs, dtype=np.float64), atf_azi=np.ascontiguousarray(ag[:, 0]),
                  atf_zen=np.ascontiguousarray(ag[:, 1]), f_trans=float(fTrans))
    shape = _out_shape(dict(kw, hrir_azi=azi))
    jl = JobList()
    for t in yaw:
        jl.add(hrir_azi=azi - t, out_shape=shape, **kw)
    jl.run()
    res = jl.results()
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def yawBankIndex(yawRad, numSets):
    """The set of a uniform yaw bank (set j designed for the yaw 2 pi j / numSets, as designYawBank(..., yawRad =
    2 pi arange(numSets) / numSets)) that is nearest to yawRad, for a scalar (an int) or an array (an int32 array of its shape);
    any angle, negative and multi-turn ones included."""
    S = int(numSets)
    if S < 1:
        raise ValueError("numSets must be at least 1")
    a = np.asarray(yawRad, dtype=np.float64)
    j = np.mod(np.rint(a * (S / (2.0 * np.pi))), S).astype(np.int32)   # (mod of an integer-valued double by S: exact, in [0, S - 1])
    return int(j) if j.ndim == 0 else j


# --------------------------------------------------------------------------------------------
# render-side neighbours
# --------------------------------------------------------------------------------------------
def getMagLsFilters2D(hLHor, hRHor, horHrirGridAziRad, order, fs, len, chDefinition="real"):
    """lib/getMagLsFilters2D.m:1: MagLS filters in circular harmonics for a horizontal HRIR set; [len x (2*order+1)] per ear,
    channels [C_0, C_-1, C_1, ..., C_-N, C_N]."""
    b, cplx = _basis(chDefinition)
    hL, hR, pL, pR = _hrirs(hLHor, hRHor)
    n, D = hL.shape
    azi, pa = _vec(horHrirGridAziRad, D, "horHrirGridAziRad")
    wL, pwL = _out(int(len), 2 * int(order) + 1, cplx)
    wR, pwR = _out(int(len), 2 * int(order) + 1, cplx)
    L.check(L.load().emagls_get_magls_filters_2d(pL, pR, n, D, pa, int(order), float(fs), int(len), b, pwL, pwR))
    return wL, wR


_RADIAL_DEFAULTS = {"radialFilter": "tikhonov", "waveModel": "planeWave", "oversamplingFactor": 2, "irLen": 256, "dirCoeff": 0,
                    "regulConst": 1e-2}   # dependencies/getRadialFilter.m:27-41,58-60


def _radial_params(params, kw):
    p = dict(_RADIAL_DEFAULTS)
    p.update(params or {})
    p.update(kw)
    for k in ("order", "fs", "smaRadius", "arrayType"):
        if k not in p:
            raise KeyError("params.%s is required" % k)       # MATLAB: reference to non-existent field
    kind = str(p["radialFilter"]).lower()
    if kind != "none" and str(p["waveModel"]).lower() == "pointsource":
        raise NotImplementedError('WaveModel parameter "%s" not yet implemented.' % p["waveModel"])    # :50-52
    if kind not in L.RADIAL:
        raise ValueError('Unkown radialFilter parameter "%s".' % p["radialFilter"])                   # :76
    if kind != "none" and (p["arrayType"] != "rigid" or p["dirCoeff"] != 0):
        raise NotImplementedError("only the rigid-sphere model is built in (the harness's arrayType, verifyEMagLs.m:245)")
    if kind == "softlimit" and "noiseGainDb" not in p:
        raise KeyError("params.noiseGainDb is required for the softlimit filter")
    return p, L.RADIAL[kind]


def getRadialFilter(params=None, **kw):
    """dependencies/getRadialFilter.m:1: radFilts [nfft/2+1 x order+1] complex, nfft = oversamplingFactor * irLen.  `params`
    is the reference's struct as a dict (order, fs, smaRadius, arrayType, irLen, oversamplingFactor, radialFilter, regulConst,
    noiseGainDb); keywords override it."""
    p, kind = _radial_params(params, kw)
    nfft = int(p["oversamplingFactor"]) * int(p["irLen"])
    rad, pr = _out(nfft // 2 + 1, int(p["order"]) + 1, True)
    L.check(L.load().emagls_get_radial_filter(int(p["order"]), float(p["fs"]), float(p["smaRadius"]), int(p["irLen"]),
                                              int(p["oversamplingFactor"]), kind, float(p["regulConst"]),
                                              float(p.get("noiseGainDb", float("nan"))), pr))
    return rad


def applyRadialFilter(inSig, params=None, **kw):
    """dependencies/applyRadialFilter.m:1: inSig [numSamples x (order+1)^2] filtered per SH order with the radial-filter
    impulse responses, the delay nfft/2 removed.  params.nfft must be oversamplingFactor * irLen (verifyEMagLs.m:250)."""
    p, kind = _radial_params(params, kw)
    nfft = int(p["oversamplingFactor"]) * int(p["irLen"])
    if "nfft" not in p:
        raise KeyError("params.nfft is required")
    if int(p["nfft"]) != nfft:
        raise ValueError("params.nfft must equal oversamplingFactor * irLen (the reference's arrays do not conform otherwise)")
    sig, ps = _f(inSig)
    C_ = (int(p["order"]) + 1) ** 2
    if sig.ndim != 2 or sig.shape[1] != C_:
        raise ValueError("inSig must be [numSamples x (order+1)^2]")
    lib = L.load()
    if sig.shape[0] < nfft:
        print("applyRadialFilter: short signal, applying zero padding!")      # :21
    rows = lib.emagls_apply_radial_filter_rows(sig.shape[0], int(p["irLen"]), int(p["oversamplingFactor"]))
    out, po = _out(rows, C_, False)
    L.check(lib.emagls_apply_radial_filter(ps, sig.shape[0], int(p["order"]), float(p["fs"]), float(p["smaRadius"]), int(p["irLen"]),
                                           int(p["oversamplingFactor"]), kind, float(p["regulConst"]),
                                           float(p.get("noiseGainDb", float("nan"))), po))
    return out


def encodeSH(smaRecording, micGridAziRad, micGridZenRad, order, shDefinition="real"):
    """verifyEMagLs.m:235-236: shRecording = smaRecording * pinv(getSH(order, micGrid, shDefinition).')."""
    b, cplx = _basis(shDefinition)
    sig, ps = _f(smaRecording)
    if sig.ndim != 2:
        raise ValueError("smaRecording must be [numSamples x numMics]")
    n, M = sig.shape
    azi, pa = _vec(micGridAziRad, M, "micGridAziRad")
    zen, pz = _vec(micGridZenRad, M, "micGridZenRad")
    out, po = _out(n, (int(order) + 1) ** 2, cplx)
    L.check(L.load().emagls_sh_encode(ps, n, M, pa, pz, int(order), b, po))
    return out


def arrayEncoder(kind, order, micGridAziRad, micGridZenRad=None, shDefinition="real"):
    """The encoder matrix [numChannels x numMics] of an array, for BinauralDecodeStream / BinauralDecodeGroup(encoder=...):
    block @ arrayEncoder(...).T is the encoded signal.
      'sma'     pinv(getSH(order, mics).T).T: the matrix encodeSH applies (verifyEMagLs.m:235-236), (order+1)^2 channels
      'ema_ch'  pinv(getCH(order, micAzi).T).T: an equatorial array in circular harmonics (testEMagLs.m:98-105), 2 order + 1 channels
      'ema_sh'  J @ the 'ema_ch' encoder, J [(order+1)^2 x (2 order + 1)] the CH -> SH expansion of
                dependencies/getChToShExpansionMatrix.m: J[(n, m), m] = Y_n^m(pi/2, 0) / C_m(0) in the basis' own normalisation,
                formed from getSH at the zenith pi/2 over getCH."""
    N = int(order)
    azi = np.asarray(micGridAziRad, dtype=np.float64).ravel()
    if kind == "sma":
        if micGridZenRad is None:
            raise ValueError("an 'sma' encoder needs micGridZenRad")
        zen = np.asarray(micGridZenRad, dtype=np.float64).ravel()
        if zen.size != azi.size:
            raise ValueError("micGridZenRad must have %d elements, got %d" % (azi.size, zen.size))
        return np.linalg.pinv(getSH(N, np.column_stack([azi, zen]), shDefinition).T).T
    if kind not in ("ema_ch", "ema_sh"):
        raise ValueError("kind must be 'sma', 'ema_ch' or 'ema_sh'")
    enc = np.linalg.pinv(getCH(N, azi, shDefinition).T).T
    if kind == "ema_ch":
        return enc
    # Y_n^m(pi/2, a) = J[(n, m), m] C_m(a) for every a: one direction gives the ratio; in the real basis the direction is chosen
    # so that neither cos(m a) nor sin(m a) vanishes for m <= order
    a0 = 0.0 if shDefinition == "complex" else math.pi / (4 * N + 2)
    Y = getSH(N, np.array([[a0, math.pi / 2]]), shDefinition)[0]
    Cm = getCH(N, np.array([a0]), shDefinition)[0]
    J = np.zeros(((N + 1) ** 2, 2 * N + 1), dtype=Y.dtype)
    for n in range(N + 1):
        for m in range(-n, n + 1):
            col = 0 if m == 0 else (2 * m if m > 0 else -2 * m - 1)     # CH order [C_0, C_-1, C_1, ..., C_-N, C_N]
            J[n * n + n + m, col] = Y[n * n + n + m] / Cm[col]
    return J @ enc


def getMagLsSphericalHeadFilter(micRadius, order, fs, len):
    """lib/getMagLsSphericalHeadFilter.m:1: (wShf [len x 1], W_Shf [nfft x 1])."""
    lib = L.load()
    w, pw = _out(int(len), 1, False)
    W, pW = _out(int(lib.emagls_eq_filter_nfft(int(len))), 1, False)
    L.check(lib.emagls_get_magls_spherical_head_filter(float(micRadius), int(order), float(fs), int(len), pw, pW))
    return w, W


def getMagLsArrayDiffuseFilter(micRadius, micGridAziRad, micGridZenRad, order, fs, len, shDefinition="real", shFunction=None):
    """lib/getMagLsArrayDiffuseFilter.m:1: wAdf [len x 1].  A custom shFunction is evaluated here at the simulation order
    ceil(fs*pi*micRadius/343) (:38) and handed over as a matrix; its low-order matrix is taken as the leading columns."""
    import math
    b, cplx = _basis(shDefinition)
    azi, pa = _vec(micGridAziRad)
    zen, pz = _vec(micGridZenRad, azi.size, "micGridZenRad")
    w, pw = _out(int(len), 1, False)
    pY = None
    if shFunction is not None:
        sim = int(math.ceil(float(fs) * math.pi * float(micRadius) / 343.0))
        Y, pY = _sh_matrix(shFunction, sim, azi, zen, shDefinition, cplx, azi.size)
    L.check(L.load().emagls_get_magls_array_diffuse_filter(float(micRadius), pa, pz, azi.size, int(order), float(fs), int(len), b,
                                                           pY, pw))
    return w


class RenderedHrtfs:
    """Result of getRenderedHrtfs.  For one filter set: H [P x D x 2] complex (None with returnResponse=False), and, when reference
    HRIRs were given, mag_err_db [P x 2], ild_err_db [P], cov_hat / cov_ref [P x 4] = (R_LL, R_RR, Re R_LR, Im R_LR) and
    coherence_hat / coherence_ref [P] = |R_LR| / sqrt(R_LL R_RR).  For a list of sets every array has a leading set dimension."""
    __slots__ = ("H", "mag_err_db", "ild_err_db", "cov_hat", "cov_ref", "coherence_hat", "coherence_ref", "nfft")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def _stack_sets(a, name):
    """One [rows x cols] array, or a list / 3-D array of them -> ([nsets x cols x rows] C-order == each set column-major, was_list)."""
    many = isinstance(a, (list, tuple)) or np.ndim(a) == 3
    arrs = [np.asarray(x) for x in (a if many else [a])]
    if not arrs or any(x.ndim != 2 or x.shape != arrs[0].shape for x in arrs):
        raise ValueError("%s must be [rows x cols] arrays of equal shape" % name)
    cplx = any(np.iscomplexobj(x) for x in arrs)
    out = np.ascontiguousarray(np.stack([x.T for x in arrs]), dtype=np.complex128 if cplx else np.float64)
    return out, many, cplx


def getRenderedHrtfs(wL, wR, model, dirsAziZenRad, fs, *, order=None, micRadius=None, micGridAziZenRad=None, atfIrs=None, nfft=None,
                     shDefinition="real", hL=None, hR=None, weights=None, returnResponse=True):
    """What the decoding filters wL, wR ([len x C], or a list of such sets) render for a plane wave from each direction of
    dirsAziZenRad [D x 2]: Hhat_e(k, d) = sum_c fft(w_e, nfft)(k, c) pwGrid_k(c, d) on the bins 0..nfft/2, with pwGrid_k the operand
    of the matching reference design -- model 'sh' (LS / MagLS: order), 'emagls' (order, micRadius, micGridAziZenRad), 'emagls2'
    (micRadius, micGridAziZenRad), 'atf' (atfIrs [taps x numMics x D], given on the evaluation directions), or, for an equatorial
    array, 'ema_ch' (getEMagLsFiltersEMAinCH: 2*order+1 circular-harmonic channels) and 'ema_sh' (getEMagLsFiltersEMAinSH:
    (order+1)^2 channels); these two take order, micRadius and micGridAziZenRad as [M] azimuths, or [M x 2] with every zenith
    pi/2.  nfft defaults to
    min(2048, 2*len).  With reference HRIRs hL, hR ([numSamples x D], one pair or one per filter set) the error metrics of
    include/emagls.h (emagls_rendered_hrtfs) are returned too; weights [D] are direction weights (uniform if absent).
    returnResponse=False computes the metrics alone."""
    if model not in L.MODEL:
        raise ValueError("model must be one of %s" % ", ".join(sorted(L.MODEL)))
    b, _ = _basis(shDefinition)
    WL, many, cL = _stack_sets(wL, "wL")
    WR, manyR, cR = _stack_sets(wR, "wR")
    if WL.shape != WR.shape or many != manyR:
        raise ValueError("wL and wR must have equal shape")
    w_cplx = cL or cR
    if w_cplx:
        WL, WR = WL.astype(np.complex128), WR.astype(np.complex128)
    nsets, Cc, ln = WL.shape
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    azi = zen = maz = mzn = atf = None
    M = taps = 0
    if model == "atf":
        if atfIrs is None:
            raise ValueError("model 'atf' needs atfIrs")
        atf, _p = _f(atfIrs)
        if atf.ndim != 3:
            raise ValueError("atfIrs must be [taps x numMics x numDirections]")
        taps, M, D = atf.shape
        if dirsAziZenRad is not None and np.asarray(dirsAziZenRad).shape[0] != D:
            raise ValueError("atfIrs must be given on the evaluation directions")
    else:
        dirs = np.asarray(dirsAziZenRad, dtype=np.float64)
        D = dirs.shape[0]
        azi, _p = _vec(dirs[:, 0])
        zen, _p = _vec(dirs[:, 1])
        if model in ("sh", "emagls", "ema_ch", "ema_sh") and order is None:
            raise ValueError("model %r needs order" % model)
        if model != "sh":
            if micRadius is None or micGridAziZenRad is None:
                raise ValueError("model %r needs micRadius and micGridAziZenRad" % model)
            grid = np.asarray(micGridAziZenRad, dtype=np.float64)
            if model in ("ema_ch", "ema_sh"):          # an equatorial array: azimuths alone (the library does not look at zeniths)
                if grid.ndim == 2 and grid.shape[1] == 2 and np.all(grid[:, 1] == np.pi / 2):
                    grid = grid[:, 0]
                elif grid.ndim == 2 and grid.shape[1] == 1:
                    grid = grid[:, 0]
                if grid.ndim != 1:
                    raise ValueError("model %r needs micGridAziZenRad as [M] azimuths, or [M x 2] with every zenith pi/2" % model)
                maz, _p = _vec(grid)
            else:
                maz, _p = _vec(grid[:, 0])
                mzn, _p = _vec(grid[:, 1])
            M = maz.size
    n_fft = int(nfft) if nfft else min(2048, 2 * ln)
    P = n_fft // 2 + 1
    H = nh = wts = None
    nsamp = 0
    if (hL is None) != (hR is None):
        raise ValueError("hL and hR go together")
    have_ref = hL is not None
    if have_ref:
        HL, _m, c1 = _stack_sets(hL, "hL")
        HR, _m, c2 = _stack_sets(hR, "hR")
        if c1 or c2 or HL.shape != HR.shape or HL.shape[1] != D:
            raise ValueError("hL and hR must be real [numSamples x %d] arrays of equal shape" % D)
        nh, nsamp = HL.shape[0], HL.shape[2]
        if weights is not None:
            wts, _p = _vec(weights, D, "weights")
    elif not returnResponse:
        raise ValueError("nothing to compute: no reference HRIRs and returnResponse=False")
    if returnResponse:
        H = np.zeros((nsets, 2, P, D), dtype=np.complex128)
    mag = np.zeros((nsets, P, 2)) if have_ref else None
    ild = np.zeros((nsets, P)) if have_ref else None
    ch = np.zeros((nsets, P, 4)) if have_ref else None
    cr = np.zeros((nsets, P, 4)) if have_ref else None
    L.check(L.load().emagls_rendered_hrtfs(L.MODEL[model], vp(WL), vp(WR), 1 if w_cplx else 0, ln, Cc, nsets, vp(azi), vp(zen), D, float(fs),
                                           int(order) if order is not None else 0, b, float(micRadius) if micRadius is not None else 0.0,
                                           vp(maz), vp(mzn), M, vp(atf), taps, n_fft, vp(HL) if have_ref else None,
                                           vp(HR) if have_ref else None, nsamp, nh if have_ref else 0, vp(wts), vp(H), vp(mag), vp(ild),
                                           vp(ch), vp(cr)))
    res = dict(nfft=n_fft)
    if returnResponse:
        res["H"] = np.ascontiguousarray(H.transpose(0, 2, 3, 1))          # [set][P][D][ear]
    if have_ref:
        with np.errstate(divide="ignore", invalid="ignore"):
            coh = lambda c: np.hypot(c[..., 2], c[..., 3]) / np.sqrt(c[..., 0] * c[..., 1])   # noqa: E731
            res.update(mag_err_db=mag, ild_err_db=ild, cov_hat=ch, cov_ref=cr, coherence_hat=coh(ch), coherence_ref=coh(cr))
    if not many:
        res = {k: (v[0] if isinstance(v, np.ndarray) else v) for k, v in res.items()}
    return RenderedHrtfs(**res)


def _components(sources):
    """The two forms of `sources` as CSR: ([Q+1] int64 offsets, azi, zen, delay or None, gain or None)."""
    if not isinstance(sources, (list, tuple)) or (len(sources) and all(np.ndim(a) == 1 and np.size(a) == 2 for a in sources)):
        sources = np.asarray(sources, dtype=np.float64)    # (an array, or rows of (azi, zen) written as a list)
    if isinstance(sources, np.ndarray):
        if sources.ndim != 2 or sources.shape[1] != 2 or sources.shape[0] < 1:
            raise ValueError("sources must be a [Q x 2] array of directions, or a list of [J x 2|3|4] arrays (azi, zen, delay, gain)")
        return np.arange(sources.shape[0] + 1, dtype=np.int64), _vec(sources[:, 0])[0], _vec(sources[:, 1])[0], None, None
    arrs = [np.asarray(a, dtype=np.float64) for a in sources]
    if not arrs:
        raise ValueError("sources must hold at least one source")
    arrs = [a.reshape(0, 2) if a.size == 0 else a for a in arrs]
    if any(a.ndim != 2 or a.shape[1] not in (2, 3, 4) for a in arrs):
        raise ValueError("every source must be a [J x 2|3|4] array with the columns azi, zen, delay, gain")
    ptr = np.zeros(len(arrs) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([a.shape[0] for a in arrs])
    col = lambda i, fill: np.ascontiguousarray(np.concatenate([a[:, i] if a.shape[1] > i else np.full(a.shape[0], fill) for a in arrs]))  # noqa: E731
    delay = col(2, 0.0) if any(a.shape[1] > 2 for a in arrs) else None
    gain = col(3, 1.0) if any(a.shape[1] > 3 for a in arrs) else None
    return ptr, col(0, 0.0), col(1, 0.0), delay, gain


def _nfft_for(irLen, nfft):
    """The transform length of a spectral call, which must be given to the C ABI: nfft, or the smallest power of two >= 2 irLen."""
    if nfft:
        return int(nfft)
    n = 8
    while n < 2 * int(irLen) and n < 65536:
        n *= 2
    return n


def _spectra(what, a, rows, P):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    want = (P,) if rows is None else (rows, P)
    if a.shape != want:
        raise ValueError("%s must have the shape %s (nfft / 2 + 1 = %d bins), got %s" % (what, want, P, a.shape))
    return a


def _per_component(what, arrs, ptr, width, dtype):
    """A list shaped like `sources` ([J_q] or [J_q x width] per source) as one contiguous array over the components."""
    if not isinstance(arrs, (list, tuple)) or len(arrs) != ptr.size - 1:
        raise ValueError("%s must be a list with one array per source" % what)
    out = []
    for q, a in enumerate(arrs):
        a = np.asarray(a)
        J = int(ptr[q + 1] - ptr[q])
        if a.size != J * width:
            raise ValueError("%s[%d] must hold %d x %d values, got %d" % (what, q, J, width, a.size))
        if dtype is np.int32 and a.size and not np.array_equal(a, np.round(a)):
            raise ValueError("%s must be integers" % what)
        out.append(a.reshape(J, width))
    flat = np.concatenate(out) if out else np.zeros((0, width))
    if dtype is np.int32 and flat.size and (np.abs(flat) >= 2 ** 31).any():
        raise ValueError("%s must fit 32 bits" % what)
    return np.ascontiguousarray(flat, dtype=dtype)


def firstOrderDirectivity(a):
    """The [4] real-SH coefficients of the first-order pattern a + (1 - a) cos(gamma) about the source's front axis (host only):
    c_0 = a sqrt(4 pi), c_3 = (1 - a) sqrt(4 pi / 3) (the x term, n = 1, m = +1), the others 0.  a = 1 is omnidirectional, a = 0.5 a
    cardioid, a = 0 a figure of eight: the `directivity` of getArrayIrs and getArrayRoomIrs."""
    a = float(a)
    return np.array([a * np.sqrt(4.0 * np.pi), 0.0, 0.0, (1.0 - a) * np.sqrt(4.0 * np.pi / 3.0)])


def _directive(directivity, sourceOrientation, Q, P):
    """directivity and sourceOrientation as the C ABI takes them: (Nd, coef [Q x Kd x P] complex128, rot [Q x 9] float64 or None)."""
    c = np.asarray(directivity)
    if c.ndim == 1:
        c = c[None, :, None]
    elif c.ndim == 2:
        c = c[:, :, None]
    if c.ndim != 3 or c.shape[0] not in (1, Q) or c.shape[2] not in (1, P):
        raise ValueError("directivity must be [Q x Kd x P] (Q = %d sources, P = nfft / 2 + 1 = %d bins), [Q x Kd] or [Kd], got %s"
                         % (Q, P, np.shape(directivity)))
    Kd = c.shape[1]
    Nd = int(round(np.sqrt(Kd))) - 1
    if Kd < 1 or (Nd + 1) ** 2 != Kd:
        raise ValueError("directivity holds %d coefficients per source and bin, which is not a square (Nd + 1)^2" % Kd)
    coef = np.ascontiguousarray(np.broadcast_to(c, (Q, Kd, P)), dtype=np.complex128)
    rot = None
    if sourceOrientation is not None:
        o = np.asarray(sourceOrientation, dtype=np.float64)
        if o.shape == (Q, 2):                          # (azi, zen) of the front axis, zero roll: R = Rz(azi) Ry(zen - pi / 2)
            ca, sa, cb, sb = np.cos(o[:, 0]), np.sin(o[:, 0]), np.cos(o[:, 1] - np.pi / 2), np.sin(o[:, 1] - np.pi / 2)
            z = np.zeros(Q)
            o = np.stack([np.stack([ca * cb, -sa, ca * sb], axis=1), np.stack([sa * cb, ca, sa * sb], axis=1), np.stack([-sb, z, cb], axis=1)], axis=1)
        if o.shape != (Q, 3, 3):
            raise ValueError("sourceOrientation must be [Q x 3 x 3] rotation matrices or [Q x 2] (azi, zen) of the front axis, got %s" % (o.shape,))
        rot = np.ascontiguousarray(o.reshape(Q, 9))
    return Nd, coef, rot


def getArrayIrs(sources, fs, irLen, preDelay, micRadius, micGridAziZenRad, *, order=4, encoder=None, nfft=None, surfaceReflection=None,
                exponents=None, airAttenuation=None, pathLength=None, distance=None, emission=None, sourceOrientation=None, directivity=None):
    """Impulse responses of the simulated rigid-sphere array (the array of getSMAIRMatrix) to sources that are sums of plane-wave
    components (include/emagls.h, emagls_array_irs).  `sources` is a [Q x 2] array of directions (azi, zen),
    one unit plane wave each -- a direction bank for a moving virtual source -- or a list of Q arrays [J_q x 2|3|4] with the columns
    azi, zen, delay in samples (default 0) and gain (default 1): an array room response from the image sources the caller lists (a
    source may be empty).  preDelay (samples, required) makes the acausal part of the sphere's response causal.  micGridAziZenRad
    [M x 2]; `order` only enters the simulation order max(order, ceil(fs pi r / 343)); `encoder` [C x M] is what arrayEncoder(...)
    returns (absent: the raw microphones, C = M).  nfft: a power of two from 8 to 65536, default the smallest one >= 2 irLen.
    Returns [Q x irLen x C], complex with a complex encoder: the `rirs` of SourceFieldStream for Q sources, or [:, None] for a bank
    of Q sets of one source.
    The spectral gain (emagls_array_irs_spectral): surfaceReflection [W x P], W <= 8 real reflection spectra in
    [-1, 1] over the P = nfft / 2 + 1 bins, with `exponents`, a list shaped like `sources` of integer arrays [J_q x W]; and
    airAttenuation [P] in Np/m with pathLength, a list of [J_q] arrays in metres (both or neither).  A component's gain becomes
    gain prod_w R_w(k)^e_w exp(-alpha(k) l) in bin k.  With none of the four given, this is the call without them.
    Point sources (emagls_array_irs_point): `distance`, a list shaped like `sources` of [J_q] arrays in metres
    ([Q] for the [Q x 2] form), every value finite and greater than micRadius, for all components or (None) for none.  The order-n
    term of a component then carries the near-field factor F_n(kappa rho); delay and gain stay the caller's (rho / 343 fs and
    1 / rho make it the point source's spherical wave).  The simulation order is the plane-wave rule: raise `order` for a source
    close to the sphere.
    Directive sources (emagls_array_irs_directive): `directivity` [Q x Kd x P], real or complex, the
    coefficients of each source's directivity per bin in the real basis of getSH(Nd, ., 'real'), Kd = (Nd + 1)^2 with Nd <= 8
    ([Q x Kd] or [Kd] is repeated over bins and sources; firstOrderDirectivity makes first-order patterns); `emission`, a list shaped
    like `sources` of [J_q x 3] unit vectors in room axes along which each component's ray left the real source ([Q x 3] for the
    [Q x 2] form; getShoeboxComponents and getShoeboxImages return them with returnEmission); and sourceOrientation [Q x 3 x 3],
    rotation matrices whose columns are each source's front, left and up axes in room axes, or [Q x 2] = (azi, zen) of the front axis
    with zero roll (absent: the room's axes).  A component's gain is multiplied by sum_i c_i(k) Y_i(R^T e)."""
    ptr, azi, zen, delay, gain = _components(sources)
    maz, mzn, M, enc, pe, e_c, Cc, nr = _array_side(micGridAziZenRad, encoder, irLen)
    Q = ptr.size - 1
    out = np.zeros((Q, Cc, nr), dtype=np.complex128 if e_c else np.float64)
    dist = None
    if distance is not None:
        if isinstance(distance, (list, tuple)) and len(distance) == Q and all(a is None or np.ndim(a) >= 1 for a in distance):
            if any(a is None or np.size(a) != ptr[q + 1] - ptr[q] for q, a in enumerate(distance)):
                raise L.EmaglsError(L.ERR_ARG, "distances are given for all components of a call or for none")
            dist = _per_component("distance", distance, ptr, 1, np.float64)
        else:                                          # [Q]: one component per source
            dist = np.ascontiguousarray(np.asarray(distance, dtype=np.float64)).reshape(-1, 1)
            if dist.shape[0] != int(ptr[-1]) or not np.array_equal(np.diff(ptr), np.ones(Q, dtype=np.int64)):
                raise ValueError("distance must be a list with one array [J_q] per source (or [Q] values for sources of one component)")
        if dist.size == 0:
            dist = np.full((1, 1), np.inf)             # (no component: the pointer alone says "point sources")
    if directivity is None and (emission is not None or sourceOrientation is not None):
        raise L.EmaglsError(L.ERR_ARG, "emission and sourceOrientation come with a directivity")
    if any(a is not None for a in (surfaceReflection, exponents, airAttenuation, pathLength, distance, directivity)):
        if (surfaceReflection is None) != (exponents is None):
            raise ValueError("surfaceReflection and exponents must both be given or both be absent")
        if (airAttenuation is None) != (pathLength is None):
            raise ValueError("airAttenuation and pathLength must both be given or both be absent")
        n_fft = _nfft_for(nr, nfft)
        P = n_fft // 2 + 1
        refl = ex = att = path = None
        W = 0
        if surfaceReflection is not None:
            refl = np.ascontiguousarray(np.atleast_2d(np.asarray(surfaceReflection, dtype=np.float64)))
            W = refl.shape[0]
            refl = _spectra("surfaceReflection", refl, W, P)
            ex = _per_component("exponents", exponents, ptr, W, np.int32)
        if airAttenuation is not None:
            att = _spectra("airAttenuation", airAttenuation, None, P)
            path = _per_component("pathLength", pathLength, ptr, 1, np.float64)
            if path.size == 0:
                path = np.zeros((1, 1))        # (the pair rule is on the pointers)
        head = (float(fs), float(micRadius), int(order), _addr(maz), _addr(mzn), M, pe, 1 if e_c else 0, Cc, Q, _addr(ptr), _addr(azi),
                _addr(zen), _addr(delay), _addr(gain), W, _addr(refl), _addr(ex) if ex is not None and ex.size else None, _addr(att), _addr(path))
        if directivity is not None:
            if emission is None:
                raise L.EmaglsError(L.ERR_ARG, "a directivity needs the emission vectors of the components (emission=)")
            if isinstance(emission, np.ndarray) and emission.shape == (Q, 3):
                emission = list(emission)              # (one component per source)
            emit = _per_component("emission", emission, ptr, 3, np.float64)
            Nd, coef, rot = _directive(directivity, sourceOrientation, Q, P)
            L.check(L.load().emagls_array_irs_directive(*head, _addr(dist), _addr(emit) if emit.size else None, _addr(rot), Nd, _addr(coef),
                                                        float(preDelay), n_fft, nr, _addr(out)))
        elif dist is not None:
            L.check(L.load().emagls_array_irs_point(*head, _addr(dist), float(preDelay), n_fft, nr, _addr(out)))
        else:
            L.check(L.load().emagls_array_irs_spectral(*head, float(preDelay), n_fft, nr, _addr(out)))
        return np.ascontiguousarray(out.transpose(0, 2, 1))
    L.check(L.load().emagls_array_irs(float(fs), float(micRadius), int(order), _addr(maz), _addr(mzn), M, pe, 1 if e_c else 0, Cc, Q, _addr(ptr),
                                      _addr(azi), _addr(zen), _addr(delay), _addr(gain), float(preDelay), int(nfft) if nfft else 0, nr, _addr(out)))
    return np.ascontiguousarray(out.transpose(0, 2, 1))


def _addr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _array_side(micGridAziZenRad, encoder, irLen):
    """The microphone grid, the encoder and the length of getArrayIrs / getArrayRoomIrs as the C ABI takes them (enc is returned to
    keep the array behind its pointer pe alive)."""
    grid = np.asarray(micGridAziZenRad, dtype=np.float64)
    if grid.ndim != 2 or grid.shape[1] != 2:
        raise ValueError("micGridAziZenRad must be [numMics x 2]")
    maz, _p = _vec(grid[:, 0])
    mzn, _p = _vec(grid[:, 1])
    M, nr = maz.size, int(irLen)
    enc, Cc, e_c, pe = None, M, False, None
    if encoder is not None:
        if np.ndim(encoder) != 2 or np.shape(encoder)[1] != M:
            raise ValueError("encoder must be [numChannels x numMics] with one column per microphone (%d)" % M)
        enc, pe, e_c, _m = _encoder(encoder, np.shape(encoder)[0])
        Cc = enc.shape[0]
    if nr < 1:
        raise ValueError("irLen must be positive")
    return maz, mzn, M, enc, pe, e_c, Cc, nr


def _room(roomDim, wallReflection, sourcePos, arrayPos, maxOrder):
    """A shoebox room as the C ABI takes it: room_dim [3], wall_refl [6], array_pos [3], src_pos [Q x 3] (one position, or one per
    row) and max_order (None: -1, no limit)."""
    dim, _p = _vec(roomDim, 3, "roomDim")
    refl, _p = _vec(wallReflection, 6, "wallReflection")
    pos, _p = _vec(arrayPos, 3, "arrayPos")
    src = np.ascontiguousarray(np.atleast_2d(np.asarray(sourcePos, dtype=np.float64)))
    if src.ndim != 2 or src.shape[1] != 3 or src.shape[0] < 1:
        raise ValueError("sourcePos must be [numSources x 3] (x, y, z per row)")
    return dim, refl, pos, src, -1 if maxOrder is None else int(maxOrder)


def _shoebox_emission(lib, dim, refl, pos, src, fs, maxDelay, mo, ptr):
    """The emission vectors of the lists whose offsets are ptr (refl None: the images): a list of [J_q x 3] arrays."""
    n, Q = int(ptr[-1]), src.shape[0]
    emit, p2 = np.zeros((max(n, 1), 3)), np.zeros(Q + 1, dtype=np.int64)
    if n:
        L.check(lib.emagls_shoebox_emission(_addr(dim), _addr(refl), _addr(pos), Q, _addr(src), float(fs), float(maxDelay), mo, n, _addr(p2),
                                            _addr(emit)))
    return [np.ascontiguousarray(emit[ptr[q]:ptr[q + 1]]) for q in range(Q)]


def getShoeboxComponents(roomDim, wallReflection, sourcePos, arrayPos, fs, maxDelay, *, maxOrder=None, returnDistance=False, returnEmission=False):
    """The image sources of a shoebox room as plane-wave components at the array's centre (include/emagls.h,
    emagls_shoebox_components), enumerated on the device.  roomDim (Lx, Ly, Lz) in metres, one corner at the origin, axes as getSH's
    (x front, y left, z up); wallReflection: six amplitude reflection coefficients in [-1, 1] for the walls x=0, x=Lx, y=0, y=Ly,
    z=0, z=Lz; sourcePos [Q x 3] (or one position) and arrayPos inside the room; maxDelay in samples; maxOrder: the largest
    reflection order kept (None: no limit).  Returns a list of Q arrays [J_q x 4] with the columns azi, zen, delay in samples and
    gain (1 / distance times the walls' coefficients), in the definition's order: the `sources` of getArrayIrs.  With returnDistance
    also a list of Q arrays [J_q], the components' distances in metres: the `distance` of getArrayIrs.  With
    returnEmission a further list of Q arrays [J_q x 3] comes last: the unit vectors in room axes along which the components' rays
    left the real source, the `emission` of getArrayIrs (emagls_shoebox_emission)."""
    dim, refl, pos, src, mo = _room(roomDim, wallReflection, sourcePos, arrayPos, maxOrder)
    Q = src.shape[0]
    ptr = np.zeros(Q + 1, dtype=np.int64)
    lib = L.load()
    head = (_addr(dim), _addr(refl), _addr(pos), Q, _addr(src), float(fs), float(maxDelay), mo)
    L.check(lib.emagls_shoebox_components(*head, 0, _addr(ptr), None, None, None, None))          # the counts
    n = int(ptr[-1])
    cols = np.zeros((4, max(n, 1)))
    if returnDistance:
        dist = np.zeros(max(n, 1))
        if n:
            L.check(lib.emagls_shoebox_components_dist(*head, n, _addr(ptr), _addr(cols[0]), _addr(cols[1]), _addr(cols[2]), _addr(cols[3]),
                                                       _addr(dist)))
        res = ([np.ascontiguousarray(cols[:, ptr[q]:ptr[q + 1]].T) for q in range(Q)],
               [np.ascontiguousarray(dist[ptr[q]:ptr[q + 1]]) for q in range(Q)])
        return res + (_shoebox_emission(lib, dim, refl, pos, src, fs, maxDelay, mo, ptr),) if returnEmission else res
    if n:
        L.check(lib.emagls_shoebox_components(*head, n, _addr(ptr), _addr(cols[0]), _addr(cols[1]), _addr(cols[2]), _addr(cols[3])))
    res = [np.ascontiguousarray(cols[:, ptr[q]:ptr[q + 1]].T) for q in range(Q)]
    return (res, _shoebox_emission(lib, dim, refl, pos, src, fs, maxDelay, mo, ptr)) if returnEmission else res


def getShoeboxImages(roomDim, sourcePos, arrayPos, fs, maxDelay, *, maxOrder=None, returnEmission=False):
    """The image sources of a shoebox room without its walls (include/emagls.h, emagls_shoebox_images): every
    candidate within maxOrder and maxDelay, for walls that are reflection spectra.  Returns (components, exponents, paths), one list
    of Q arrays each: [J_q x 4] with the columns azi, zen, delay in samples and gain = 1 / distance -- the bits of
    getShoeboxComponents with all six coefficients 1 --, [J_q x 6] int32 exponents of the walls x=0, x=Lx, y=0, y=Ly, z=0, z=Lz, and
    [J_q] distances in metres: the `sources`, `exponents` and `pathLength` of getArrayIrs.  With returnEmission a fourth list of
    [J_q x 3] emission vectors, as getShoeboxComponents returns them."""
    dim, _refl, pos, src, mo = _room(roomDim, np.ones(6), sourcePos, arrayPos, maxOrder)
    Q = src.shape[0]
    ptr = np.zeros(Q + 1, dtype=np.int64)
    lib = L.load()
    head = (_addr(dim), _addr(pos), Q, _addr(src), float(fs), float(maxDelay), mo)
    L.check(lib.emagls_shoebox_images(*head, 0, _addr(ptr), None, None, None, None, None, None))          # the counts
    n = int(ptr[-1])
    cols, ex, path = np.zeros((4, max(n, 1))), np.zeros((max(n, 1), 6), dtype=np.int32), np.zeros(max(n, 1))
    if n:
        L.check(lib.emagls_shoebox_images(*head, n, _addr(ptr), _addr(cols[0]), _addr(cols[1]), _addr(cols[2]), _addr(cols[3]), _addr(ex),
                                          _addr(path)))
    cut = lambda a: [np.ascontiguousarray(a[ptr[q]:ptr[q + 1]]) for q in range(Q)]   # noqa: E731
    res = cut(cols.T), cut(ex), cut(path)
    return res + (_shoebox_emission(lib, dim, None, pos, src, fs, maxDelay, mo, ptr),) if returnEmission else res


def wallReflectionSpectra(absorption, bandCentresHz, fs, nfft):
    """Reflection spectra [S x P] over the bins f_k = k fs / nfft, k = 0 .. nfft / 2, from absorption coefficients per band as data
    sheets give them (host only): `absorption` [S x nb] (or [nb]) in [0, 1] at the ascending band centres bandCentresHz [nb], is
    interpolated linearly in log2 f between the centres and held constant outside them (bin 0 takes the first band's value); then
    R = sqrt(1 - a)."""
    a = np.atleast_2d(np.asarray(absorption, dtype=np.float64))
    fc = np.asarray(bandCentresHz, dtype=np.float64).ravel()
    if a.shape[1] != fc.size or fc.size < 1:
        raise ValueError("absorption must be [numSurfaces x numBands] with one column per band centre")
    if not (np.all(fc > 0) and np.all(np.diff(fc) > 0)):
        raise ValueError("bandCentresHz must be positive and ascending")
    if not (np.all(a >= 0) and np.all(a <= 1)):
        raise ValueError("absorption coefficients must lie in [0, 1]")
    f = np.arange(int(nfft) // 2 + 1) * (float(fs) / int(nfft))
    x = np.full(f.size, -np.inf)
    x[1:] = np.log2(f[1:])
    return np.sqrt(1.0 - np.stack([np.interp(x, np.log2(fc), row) for row in a]))


def airAttenuation(fs, nfft, temperatureC=20.0, relHumidityPercent=50.0, pressureKPa=101.325):
    """The attenuation of sound in air over the bins f_k = k fs / nfft, k = 0 .. nfft / 2, in nepers per metre (host only): the
    pure-tone formula of ISO 9613-1, dB/m times ln(10) / 20."""
    T0, T01, pr = 293.15, 273.16, 101.325
    T, pa, hr = float(temperatureC) + 273.15, float(pressureKPa), float(relHumidityPercent)
    f = np.arange(int(nfft) // 2 + 1) * (float(fs) / int(nfft))
    psat = 10.0 ** (-6.8346 * (T01 / T) ** 1.261 + 4.6151)
    h = hr * psat / (pa / pr)
    frO = (pa / pr) * (24.0 + 4.04e4 * h * (0.02 + h) / (0.391 + h))
    frN = (pa / pr) * (T / T0) ** -0.5 * (9.0 + 280.0 * h * np.exp(-4.170 * ((T / T0) ** (-1.0 / 3.0) - 1.0)))
    db = 8.686 * f * f * (1.84e-11 * (pr / pa) * (T / T0) ** 0.5 +
                          (T / T0) ** -2.5 * (0.01275 * np.exp(-2239.1 / T) / (frO + f * f / frO) +
                                              0.1068 * np.exp(-3352.0 / T) / (frN + f * f / frN)))
    return db * (np.log(10.0) / 20.0)


def getArrayRoomIrs(roomDim, wallReflection, sourcePos, arrayPos, fs, irLen, preDelay, micRadius, micGridAziZenRad, *, order=4,
                    encoder=None, nfft=None, maxOrder=None, maxDelay=None, returnCounts=False, airAttenuation=None, waveModel="planeWave",
                    sourceOrientation=None, directivity=None):
    """Impulse responses of the simulated rigid-sphere array in a shoebox room (include/emagls.h,
    emagls_array_room_irs): getArrayIrs(getShoeboxComponents(...), ...) bit for bit, with the components enumerated on the device
    and fed to the responses' kernels there.  The room as in getShoeboxComponents (the array's whole sphere inside it), the array
    as in getArrayIrs.  maxDelay (samples): default irLen - 1 - preDelay, the last component that lands inside the returned taps.
    Returns [Q x irLen x C]; with returnCounts also the number of components of each source ([Q] int64).
    The spectral room (emagls_array_room_irs_spectral): wallReflection [6 x P], one reflection spectrum per wall
    over the P = nfft / 2 + 1 bins (wallReflectionSpectra makes them from absorption coefficients), and / or airAttenuation [P] in
    Np/m (the function airAttenuation of this module), each component's path its distance; six coefficients with an airAttenuation are
    repeated over the bins.  Then every image within maxOrder and maxDelay is a component (getShoeboxImages), also behind a wall of 0.
    waveModel (getSMAIRMatrix's parameter and default): 'planeWave', every image a plane wave at the array (a far-field model), or
    'pointSource' (emagls_array_room_irs_point), every image a point source at its distance: getArrayIrs with
    distance= on the lists of getShoeboxComponents(returnDistance=True) or getShoeboxImages (its paths), bit for bit.
    Directive sources (emagls_array_room_irs_directive): `directivity` and sourceOrientation as in getArrayIrs,
    with every wall and wave model above; the emission vectors are the enumeration's (returnEmission of the list functions), and the
    result is getArrayIrs on those lists, bit for bit."""
    if waveModel not in ("planeWave", "pointSource"):
        raise L.EmaglsError(L.ERR_ARG, "unknown waveModel %r: 'planeWave' or 'pointSource'" % (waveModel,))
    spectral = np.ndim(wallReflection) == 2 or airAttenuation is not None
    dim, refl, pos, src, mo = _room(roomDim, np.ones(6) if spectral else wallReflection, sourcePos, arrayPos, maxOrder)
    maz, mzn, M, enc, pe, e_c, Cc, nr = _array_side(micGridAziZenRad, encoder, irLen)
    Q = src.shape[0]
    if maxDelay is None:
        maxDelay = nr - 1 - float(preDelay)
    out = np.zeros((Q, Cc, nr), dtype=np.complex128 if e_c else np.float64)
    counts = np.zeros(Q, dtype=np.int64)
    if directivity is None and sourceOrientation is not None:
        raise L.EmaglsError(L.ERR_ARG, "sourceOrientation comes with a directivity")
    if directivity is not None:
        n_fft = _nfft_for(nr, nfft)
        P = n_fft // 2 + 1
        w = np.asarray(wallReflection, dtype=np.float64)
        w = _spectra("wallReflection", w, 6, P) if w.ndim == 2 else _vec(w, 6, "wallReflection")[0]
        att = None if airAttenuation is None else _spectra("airAttenuation", airAttenuation, None, P)
        Nd, coef, rot = _directive(directivity, sourceOrientation, Q, P)
        L.check(L.load().emagls_array_room_irs_directive(float(fs), float(micRadius), int(order), _addr(maz), _addr(mzn), M, pe, 1 if e_c else 0, Cc,
                                                         _addr(dim), _addr(w), 1 if w.ndim == 2 else 0, _addr(att), _addr(pos), Q, _addr(src),
                                                         float(maxDelay), mo, 1 if waveModel == "pointSource" else 0, _addr(rot), Nd, _addr(coef),
                                                         float(preDelay), n_fft, nr, _addr(counts), _addr(out)))
        out = np.ascontiguousarray(out.transpose(0, 2, 1))
        return (out, counts) if returnCounts else out
    if waveModel == "pointSource":
        n_fft = _nfft_for(nr, nfft)
        P = n_fft // 2 + 1
        w = np.asarray(wallReflection, dtype=np.float64)
        w = _spectra("wallReflection", w, 6, P) if w.ndim == 2 else _vec(w, 6, "wallReflection")[0]     # (six coefficients: the C entry repeats them)
        att = None if airAttenuation is None else _spectra("airAttenuation", airAttenuation, None, P)
        L.check(L.load().emagls_array_room_irs_point(float(fs), float(micRadius), int(order), _addr(maz), _addr(mzn), M, pe, 1 if e_c else 0, Cc,
                                                     _addr(dim), _addr(w), 1 if w.ndim == 2 else 0, _addr(att), _addr(pos), Q, _addr(src),
                                                     float(maxDelay), mo, float(preDelay), n_fft, nr, _addr(counts), _addr(out)))
        out = np.ascontiguousarray(out.transpose(0, 2, 1))
        return (out, counts) if returnCounts else out
    if spectral:
        n_fft = _nfft_for(nr, nfft)
        P = n_fft // 2 + 1
        w = np.asarray(wallReflection, dtype=np.float64)
        if w.ndim == 1:
            w = np.repeat(_vec(w, 6, "wallReflection")[0][:, None], P, axis=1)
        w = _spectra("wallReflection", w, 6, P)
        att = None if airAttenuation is None else _spectra("airAttenuation", airAttenuation, None, P)
        L.check(L.load().emagls_array_room_irs_spectral(float(fs), float(micRadius), int(order), _addr(maz), _addr(mzn), M, pe, 1 if e_c else 0, Cc,
                                                        _addr(dim), _addr(w), _addr(att), _addr(pos), Q, _addr(src), float(maxDelay), mo,
                                                        float(preDelay), n_fft, nr, _addr(counts), _addr(out)))
        out = np.ascontiguousarray(out.transpose(0, 2, 1))
        return (out, counts) if returnCounts else out
    L.check(L.load().emagls_array_room_irs(float(fs), float(micRadius), int(order), _addr(maz), _addr(mzn), M, pe, 1 if e_c else 0, Cc, _addr(dim),
                                           _addr(refl), _addr(pos), Q, _addr(src), float(maxDelay), mo, float(preDelay), int(nfft) if nfft else 0,
                                           nr, _addr(counts), _addr(out)))
    out = np.ascontiguousarray(out.transpose(0, 2, 1))
    return (out, counts) if returnCounts else out
