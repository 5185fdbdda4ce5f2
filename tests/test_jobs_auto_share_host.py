"""The job scheduler's rule for sharing a chunk's geometry (emagls_jobs_would_share_geometry, include/emagls.h), on descriptors and
host grids alone: no device needed."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    from emagls_amd import build, _lib
    build.build(jobs=4, verbose=False)
    _lib.load()
    return _lib


def make(L, n=4, kind=None, order=4, nmics=32, basis="complex", **over):
    from emagls_amd.jobs import JobList
    rng = np.random.default_rng(1)
    azi, zen = rng.uniform(0, 6.28, 50), rng.uniform(0, 3.14, 50)
    maz, mzn = rng.uniform(0, 6.28, nmics), rng.uniform(0, 3.14, nmics)
    h = np.zeros((16, 50))
    jl = JobList()
    for j in range(n):
        kw = dict(mic_radius=0.042, mic_azi=maz, mic_zen=mzn, out_shape=(64, 25, True))
        kw.update({k: (v(j) if callable(v) else v) for k, v in over.items()})
        jl.add(L.KIND_EMAGLS if kind is None else kind, basis, order, 48000.0, 64, h + j, h - j, kw.pop("hrir_azi", azi), kw.pop("hrir_zen", zen), **kw)
    return jl, (azi, zen, maz, mzn)


def test_equal_descriptors_and_grids_share(L):
    jl, (azi, zen, maz, mzn) = make(L)
    assert jl.would_share_geometry()
    assert not jl.would_share_geometry(0, 1)                  # one design has nobody to share with
    # equal grids in arrays of their own (compared by value, not by address)
    jl2, _ = make(L, mic_azi=lambda j: maz.copy(), hrir_zen=lambda j: zen.copy())
    assert jl2.would_share_geometry()
    for kind in (L.KIND_EMAGLS2, L.KIND_EMA_CH):
        assert make(L, kind=kind, order=3, nmics=9)[0].would_share_geometry()


def test_what_differs_is_not_shared(L):
    _, (azi, zen, maz, mzn) = make(L)
    assert not make(L, mic_radius=lambda j: 0.042 + (j == 2) * 1e-4)[0].would_share_geometry()       # a descriptor of its own
    assert not make(L, mic_azi=lambda j: maz + (j == 3) * 1e-9)[0].would_share_geometry()            # a microphone grid of its own
    assert not make(L, hrir_azi=lambda j: azi + (j == 1) * 1e-9)[0].would_share_geometry()           # an HRIR grid of its own
    assert not make(L, diffuseness=True)[0].would_share_geometry()                                   # the covariance constraint
    assert not make(L, kind=L.KIND_EMAGLS2, nmics=40)[0].would_share_geometry()                      # the 33..64-channel path
    assert not make(L, kind=L.KIND_EMAGLS, order=6, nmics=64)[0].would_share_geometry()
    assert not make(L, kind=L.KIND_EMA_SH, order=2, nmics=9)[0].would_share_geometry()               # kinds without the option
    from emagls_amd.jobs import JobList
    jl = JobList()
    for j in range(3):
        jl.add(L.KIND_MAGLS, "real", 3, 48000.0, 64, np.zeros((16, 50)), np.zeros((16, 50)), azi, zen, out_shape=(64, 16, False))
    assert not jl.would_share_geometry()                                                             # (MagLS: only when asked)
