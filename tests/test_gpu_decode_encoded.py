"""The encoded decode stream and listener group on the GPU (BinauralDecodeStream / BinauralDecodeGroup with encoder=...; DESIGN.md
section 9.6): blocks of real microphone signals in, the array encoder inside the rotation launch.
Parity is against the PLAIN stream (whose kernels this feature leaves untouched) fed x @ enc.T computed in NumPy: max abs
difference over max abs output below 1e-12, the bound tests/test_gpu_decode_stream.py and tests/test_gpu_decode_bank.py hold
against the oracle (they measure 4e-16 to 2.4e-15); the encoder adds a dot product of at most 64 FP64 terms, so three decades remain.
Measured on an MI355X: 0 in all 46 stream cases and the 4 bank cases -- the NumPy build's matrix product accumulates each element
with fma over ascending microphones too, so the plain stream was fed the very bits the kernels form; another BLAS may differ in the
last bit of the encoded signal, which the bound covers.
The fixed encode arithmetic (fma from 0, microphones ascending) is checked through its consequences, with np.array_equal: an
identity encoder gives the plain stream's bits, a listener of an encoded group the bits of an encoded stream, and the grouping of
blocks into pushes changes nothing.
Shapes (M, C, domain, basis, len, B): chosen to reach each path, see SHAPES."""
import numpy as np
import pytest

gpu = pytest.mark.gpu
TOL = 1e-12
SHAPES = [
    (32, 25, "sh", "real", 512, 64),        # the workload's own form
    (19, 16, "sh", "complex", 130, 128),    # M no multiple of anything, P = 2, complex enc -> 2C planes
    (8, 5, "ch", "real", 64, 64),           # CH, yaw only, P = 1
    (64, 64, "sh", "real", 200, 256),       # both caps, the order 7 bucket of rotate3, enc fills its LDS budget
    (3, 9, "sh", "real", 96, 64),           # C > M
    (1, 1, "sh", "real", 64, 64),           # the smallest possible
]
ANGLES = ["none", "yaw_scalar", "yaw", "ypr"]


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def randn(rng, shape, cplx=False):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape) if cplx else rng.standard_normal(shape)


def num_blocks(ln, B):
    """max(6, P + 3) blocks, so the ring wraps; rounded up to a multiple of 3 for the pushes of three blocks."""
    nb = max(6, -(-ln // B) + 3)
    return -(-nb // 3) * 3


def make_angles(rng, case, n, nl=None):
    """(yaw, pitch, roll) of one listener (nl None), or of nl listeners as [L] / [L x n]."""
    lead = () if nl is None else (nl,)
    if case == "none":
        return None, None, None
    if case == "yaw_scalar":
        return (float(rng.uniform(-3, 3)) if nl is None else rng.uniform(-3, 3, nl)), None, None
    traj = lambda lim: rng.uniform(-lim, lim, lead + (1,)) + np.cumsum(rng.normal(0, 0.02, lead + (n,)), axis=-1)   # noqa: E731
    if case == "yaw":
        return traj(3), None, None
    return traj(3), traj(1), traj(1)


def run(obj, x, angles, step, sigma=None, device=False, per_listener=False):
    """x through the open stream or group `obj`, `step` samples per push.  angles: per-sample arrays [..., n], scalars, or [L]
    vectors of a group (per_listener) that stay whole.  sigma: set indices [..., nb] or None."""
    B, out = obj.blockSize, []
    if device:
        import torch
        dev = torch.device("cuda:0")
        tx = torch.as_tensor(np.ascontiguousarray(x), device=dev)
    for k, i in enumerate(range(0, x.shape[0], step)):
        a = []
        for v in angles:
            whole = v is None or np.ndim(v) == 0 or (per_listener and np.ndim(v) == 1)
            a.append(v if whole else v[..., i:i + step])
        idx = None if sigma is None else np.asarray(sigma)[..., k * (step // B):(k + 1) * (step // B)]
        if device:
            to = lambda v, dt: None if v is None else torch.as_tensor(np.ascontiguousarray(v), device=dev).to(dt)   # noqa: E731
            o = obj.push(tx[i:i + step], *[to(v, torch.float64) for v in a], setIndex=to(idx, torch.int32))
            torch.cuda.synchronize()
            out.append(o.cpu().numpy())
        else:
            out.append(obj.push(x[i:i + step], *a, setIndex=idx))
    return np.concatenate(out, axis=-2)


def case_data(shape, seed, S=1):
    M, Cc, domain, basis, ln, B = shape
    rng = np.random.default_rng(seed)
    cplx = basis == "complex"
    n = num_blocks(ln, B) * B
    x = randn(rng, (n, M))
    enc = randn(rng, (Cc, M), cplx) / np.sqrt(M)
    wshape = (ln, Cc) if S == 1 else (S, ln, Cc)
    return rng, n, x, enc, randn(rng, wshape, cplx), randn(rng, wshape, cplx)


def stream(E, shape, wL, wR, enc=None, complexInput=False):
    M, Cc, domain, basis, ln, B = shape
    return E.BinauralDecodeStream(wL, wR, B, shDefinition=basis, rotationDomain=domain, complexInput=complexInput, encoder=enc)


def group(E, shape, wL, wR, nl, enc):
    M, Cc, domain, basis, ln, B = shape
    return E.BinauralDecodeGroup(wL, wR, B, nl, shDefinition=basis, rotationDomain=domain, encoder=enc)


def cases_of(shape):
    return [c for c in ANGLES if not (c == "ypr" and shape[2] != "sh")]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. parity with the plain stream fed x @ enc.T
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "M%d-C%d-%s-%s-len%d-B%d" % s)
def test_parity_with_the_plain_stream_fed_the_encoded_signal(shape):
    import emagls_amd as E
    rng, n, x, enc, wL, wR = case_data(shape, sum(shape[:2]) + shape[4])
    B = shape[5]
    s = x @ enc.T
    for k, case in enumerate(cases_of(shape)):
        angles = make_angles(rng, case, n)
        with stream(E, shape, wL, wR, complexInput=np.iscomplexobj(s)) as plain:
            want = run(plain, s, angles, 3 * B)
        # host and device entry, pushes of one block and of three: each pairing in turn over the cases
        for device, blocks in ((False, 1), (True, 3)) if k % 2 else ((False, 3), (True, 1)):
            with stream(E, shape, wL, wR, enc) as es:
                assert es.numMics == shape[0] and es.numChannels == shape[1] and es.info["launches_per_block"] == 3
                got = run(es, x, angles, blocks * B, device=device)
            err = rel(got, want)
            print("encoded parity", shape, case, "device" if device else "host", "%d block(s) per push" % blocks, "%.2e" % err)
            assert got.shape == (n, 2) and err <= TOL


# ---------------------------------------------------------------------------------------------------------------------------
# 2. bits
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("Cc,basis", [(25, "real"), (16, "complex")])
def test_identity_encoder_gives_the_plain_stream_s_bits(Cc, basis):
    import emagls_amd as E
    shape = (Cc, Cc, "sh", basis, 150, 64)
    rng, n, x, _, wL, wR = case_data(shape, Cc)
    for case in ANGLES:
        angles = make_angles(rng, case, n)
        with stream(E, shape, wL, wR) as plain:
            want = run(plain, x, angles, 64)
        for device in (False, True):
            with stream(E, shape, wL, wR, np.eye(Cc)) as es:
                assert np.array_equal(run(es, x, angles, 64, device=device), want), (case, device)


@gpu
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[3]], ids=lambda s: "M%d-C%d" % s[:2])
def test_equal_pushes_give_equal_bits_and_reset_is_a_fresh_stream(shape):
    import emagls_amd as E
    rng, n, x, enc, wL, wR = case_data(shape, 11)
    B = shape[5]
    for case in ("none", "ypr"):
        angles = make_angles(rng, case, n)
        with stream(E, shape, wL, wR, enc) as es:
            one = run(es, x, angles, B)
        with stream(E, shape, wL, wR, enc) as es:
            assert np.array_equal(run(es, x, angles, B), one)                    # two fresh streams
            es.reset()
            assert np.array_equal(run(es, x, angles, 3 * B), one)                # three blocks per push; after a reset
            es.reset()
            assert np.array_equal(run(es, x, angles, 3 * B, device=True), one)
            k = 2 * B                                                            # a reset in mid-stream, the ring partly filled
            es.reset()
            run(es, x[:k], [cut_to(a, 0, k) for a in angles], B)
            es.reset()
            assert np.array_equal(run(es, x, angles, B), one)


def cut_to(a, i, j):
    return a if a is None or np.ndim(a) == 0 else a[..., i:j]


# ---------------------------------------------------------------------------------------------------------------------------
# 3. a bank
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_bank_with_a_set_change_in_every_block():
    import emagls_amd as E
    shape, S = SHAPES[0], 3
    rng, n, x, enc, wL, wR = case_data(shape, 5, S)
    B = shape[5]
    sigma = (1 + np.arange(n // B)) % S
    s = x @ enc.T
    for case in ("none", "ypr"):
        angles = make_angles(rng, case, n)
        with stream(E, shape, wL, wR) as plain:
            want = run(plain, s, angles, 3 * B, sigma)
        for device, blocks in ((False, 1), (True, 3)):
            with stream(E, shape, wL, wR, enc) as es:
                err = rel(run(es, x, angles, blocks * B, sigma, device=device), want)
            print("encoded bank parity", case, "device" if device else "host", "%.2e" % err)
            assert err <= TOL


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the group
# ---------------------------------------------------------------------------------------------------------------------------
def listener_part(angles, l):
    return [None if v is None else (float(v[l]) if np.ndim(v) == 1 else v[l]) for v in angles]


@gpu
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[3]], ids=lambda s: "M%d-C%d" % s[:2])
def test_every_listener_of_an_encoded_group_is_an_encoded_stream_bit_for_bit(shape):
    import emagls_amd as E
    nl, B = 3, shape[5]
    combo = 0
    for S in (1, 3):
        rng, n, x, enc, wL, wR = case_data(shape, 17 + S, S)
        for case in ("none", "yaw_scalar", "ypr"):
            combo += 1
            angles = make_angles(rng, case, n, nl)
            sig = None if S == 1 else rng.integers(0, S, (nl, n // B))
            if sig is not None:
                sig[0] = np.arange(n // B) % S                                   # listener 0 changes set in every block
            want = []
            for l in range(nl):
                with stream(E, shape, wL, wR, enc) as es:
                    want.append(run(es, x, listener_part(angles, l), B, None if sig is None else sig[l]))
            device, blocks = ((False, 3), (True, 1))[combo % 2]
            with group(E, shape, wL, wR, nl, enc) as g:
                assert g.numMics == shape[0] and g.info()["launches_per_block"] == 3
                got = run(g, x, angles, blocks * B, sig, device=device, per_listener=True)
            assert got.shape == (nl, n, 2)
            for l in range(nl):
                assert np.array_equal(got[l], want[l]), (S, case, "device" if device else "host", blocks, l)


@gpu
def test_group_of_one_listener_and_reset_of_one_listener():
    import emagls_amd as E
    shape = SHAPES[0]
    B = shape[5]
    rng, n, x, enc, wL, wR = case_data(shape, 23)
    angles = make_angles(rng, "ypr", n, 3)
    one = listener_part(angles, 1)
    with stream(E, shape, wL, wR, enc) as es:
        want = run(es, x, one, B)
    with group(E, shape, wL, wR, 1, enc) as g:
        assert np.array_equal(run(g, x, [a[None] for a in one], B)[0], want)
    with group(E, shape, wL, wR, 3, enc) as g:
        whole = run(g, x, angles, B)
    k = 4 * B
    with group(E, shape, wL, wR, 3, enc) as g:
        head = run(g, x[:k], [a[:, :k] for a in angles], B)
        g.reset(1)
        tail = run(g, x[k:], [a[:, k:] for a in angles], B)
    assert np.array_equal(head, whole[:, :k])
    for l in (0, 2):                                                             # the others run on uninterrupted
        assert np.array_equal(tail[l], whole[l, k:])
    with stream(E, shape, wL, wR, enc) as es:                                    # the one who joined: a fresh stream from there on
        assert np.array_equal(tail[1], run(es, x[k:], [a[k:] for a in one], B))
    assert not np.array_equal(tail[1], whole[1, k:])
