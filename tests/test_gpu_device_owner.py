"""Device memory behind its owners (csrc/device_mem.hpp, csrc/block_stream.hpp): what a grown-and-kept buffer, a cache slot or a
recreated object must not change.  Every comparison is bitwise: the same kernels run on the same inputs, only the buffers they
stage through differ."""
import functools

import numpy as np
import pytest

gpu = pytest.mark.gpu
B = 64


@functools.lru_cache(maxsize=None)
def field_case():
    """nsrc = 1, nch = 2, nr = 65: sources [6 B], responses [65 x 2] (shared, read only)."""
    rng = np.random.default_rng(11)
    s, rirs = rng.standard_normal(6 * B), rng.standard_normal((65, 2))
    for a in (s, rirs):
        a.setflags(write=False)
    return s, rirs


@functools.lru_cache(maxsize=None)
def decode_case():
    """C = 4, len = 65: signal [6 B x 4], filters [65 x 4] and a yaw per sample (shared, read only)."""
    rng = np.random.default_rng(12)
    x, wL, wR = rng.standard_normal((6 * B, 4)), rng.standard_normal((65, 4)), rng.standard_normal((65, 4))
    yaw = np.cumsum(rng.normal(0, 0.01, 6 * B))
    for a in (x, wL, wR, yaw):
        a.setflags(write=False)
    return x, wL, wR, yaw


def pushes_of(n_blocks=(1, 4, 1)):
    """The sample ranges of pushes of B, 4 B and B samples."""
    edges = np.cumsum((0,) + n_blocks) * B
    return list(zip(edges[:-1], edges[1:]))


def block_by_block_on_device(torch, obj, x, yaw=None):
    """x through the device entry of obj, one block per push."""
    tx = torch.from_numpy(np.array(x)).to("cuda:0")
    ty = None if yaw is None else torch.from_numpy(np.array(yaw)).to("cuda:0")
    outs = [obj.push(tx[i:i + B]) if ty is None else obj.push(tx[i:i + B], ty[i:i + B]) for i in range(0, x.shape[0], B)]
    torch.cuda.synchronize()
    return torch.cat(outs).cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# 1. stage buffers grow and are kept
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_field_stream_stage_buffers_grow_and_are_kept():
    import torch
    import emagls_amd as E
    s, rirs = field_case()
    with E.SourceFieldStream(rirs, B) as f, E.SourceFieldStream(rirs, B) as g:
        first = np.vstack([f.push(s[a:b]) for a, b in pushes_of()])
        assert np.array_equal(first, block_by_block_on_device(torch, g, s))
        f.reset()
        assert np.array_equal(np.vstack([f.push(s[a:b]) for a, b in pushes_of()]), first)
    assert first.shape == (6 * B, 2) and np.abs(first).max() > 0


@gpu
@pytest.mark.parametrize("turned", [False, True])
def test_decode_stream_stage_buffers_grow_and_are_kept(turned):
    import torch
    import emagls_amd as E
    x, wL, wR, yaw = decode_case()

    def host(s):
        return np.vstack([s.push(x[a:b], yaw[a:b]) if turned else s.push(x[a:b]) for a, b in pushes_of()])
    with E.BinauralDecodeStream(wL, wR, B) as s, E.BinauralDecodeStream(wL, wR, B) as t:
        first = host(s)
        assert np.array_equal(first, block_by_block_on_device(torch, t, x, yaw if turned else None))
        s.reset()
        assert np.array_equal(host(s), first)
    assert first.shape == (6 * B, 2) and np.abs(first).max() > 0


# ---------------------------------------------------------------------------------------------------------------------------
# 2. work cache slots
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_decode_work_cache_slots():
    import emagls_amd as E
    from emagls_amd import _lib as L
    rng = np.random.default_rng(13)
    x = rng.standard_normal((1000, 4))
    filters = {ln: (rng.standard_normal((ln, 4)), rng.standard_normal((ln, 4))) for ln in (64, 300, 600)}   # fused, wave, hipFFT filter side

    def decode(ln):
        return E.binauralDecode(x, 48000, filters[ln][0], filters[ln][1], 48000)
    a1, b, c, a2 = decode(64), decode(300), decode(600), decode(64)
    assert np.array_equal(a1, a2)
    L.check(L.load().emagls_cache_clear())
    assert np.array_equal(decode(64), a1)
    for out in (a1, b, c):
        assert out.shape == (1000, 2) and np.isfinite(out).all() and np.abs(out).max() > 0


# ---------------------------------------------------------------------------------------------------------------------------
# 3. destroy and recreate
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_destroy_and_recreate_twenty_times():
    import emagls_amd as E
    s, rirs = field_case()
    x, wL, wR, _ = decode_case()
    seen = []
    for _ in range(20):
        with E.BinauralDecodeStream(wL, wR, B) as d, E.SourceFieldStream(rirs, B) as f:
            seen.append((d.info["state_bytes"], d.info["filter_bytes"], f.info["state_bytes"], f.info["response_bytes"],
                         d.push(x[:2 * B]), f.push(s[:2 * B])))
    for k in range(1, 20):
        assert seen[k][:4] == seen[0][:4], k
        assert np.array_equal(seen[k][4], seen[0][4]) and np.array_equal(seen[k][5], seen[0][5]), k
    assert np.abs(seen[0][4]).max() > 0 and np.abs(seen[0][5]).max() > 0
