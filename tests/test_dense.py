"""GPU: dense descriptor images (sift3d_amd_dense_descriptors_device and its stages) against the numpy
restatement of the contract in include/sift3d_amd.h (tests/dense_restatement.py), bit for bit; plus
properties that need no restatement (shift equivariance, mirror symmetry, unit norms)."""
import math

import numpy as np
import pytest

from tests import dense_restatement as dr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    from sift3d_amd import hip as h
    h.lib()
    assert torch.cuda.is_available()
    h.current_stream(refresh=True)
    return h


def _dev(hip, vol, sigma, units=(1, 1, 1)):
    import torch
    src = torch.from_numpy(np.ascontiguousarray(vol, np.float32)).cuda()
    out = torch.empty((12,) + tuple(src.shape), dtype=torch.float32, device="cuda")
    hip.dense_descriptors(src, out, sigma, units)
    return out.cpu().numpy()


def _dev_bin(hip, vol, units=(1, 1, 1)):
    import torch
    src = torch.from_numpy(np.ascontiguousarray(vol, np.float32)).cuda()
    out = torch.full((12,) + tuple(src.shape), float("nan"), dtype=torch.float32, device="cuda")
    hip.dense_bin(src, out, units)
    return out.cpu().numpy()


def _assert_bits(got, want, what):
    assert got.shape == want.shape, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    if bad.any():
        i = tuple(int(a[0]) for a in np.nonzero(bad))
        raise AssertionError("%s: %d of %d values differ, first at %s: %r != %r"
                             % (what, int(bad.sum()), bad.size, i, got[i], want[i]))


def _hw(sigma):
    return max(int(math.ceil(3.0 * sigma)), 1)


CASES = [
    # (shape (nx, ny, nz), units, sigma)
    ((32, 24, 20), (1.0, 1.0, 1.0), 1.6),       # nx % 4 == 0, fused y+z
    ((30, 22, 19), (1.0, 1.0, 1.0), 1.6),       # nx % 4 != 0, scalar stores, separate passes
    ((32, 24, 20), (0.7, 1.0, 2.5), 1.6),       # separate passes
    ((29, 21, 18), (0.7, 1.0, 2.5), 1.6),
    ((28, 20, 18), (1.0, 1.0, 1.0), 11.0),      # 67 taps: the chunked literal FIR
    ((16, 2, 1), (1.0, 1.0, 1.0), 1.6),         # axes of 1 and 2 voxels
    ((1, 9, 2), (1.0, 2.0, 1.0), 1.6),
    ((2, 1, 7), (1.0, 1.0, 1.0), 1.6),
    ((1, 1, 1), (1.0, 1.0, 1.0), 1.6),
]


@pytest.mark.parametrize("shape,units,sigma", CASES)
def test_bit_exact_against_restatement(hip, oracle_mod, shape, units, sigma):
    vol = oracle_mod.synth_survey(shape, nblob=max(4, int(np.prod(shape)) // 400), seed=11)
    vol += np.random.default_rng(1).random(vol.shape, dtype=np.float32) * np.float32(0.05)
    want = dr.dense_descriptors(vol, oracle_mod, sigma, units)
    got = _dev(hip, vol, sigma, units)
    _assert_bits(got, want, "dense %s units %s sigma %g" % (shape, units, sigma))
    assert np.count_nonzero(got) > 0 or max(shape) == 1


@pytest.mark.parametrize("shape,units", [((32, 24, 20), (1.0, 1.0, 1.0)), ((30, 22, 19), (0.7, 1.0, 2.5)),
                                         ((1, 2, 5), (1.0, 1.0, 1.0))])
def test_dense_bin_stage_bit_exact(hip, oracle_mod, shape, units):
    vol = oracle_mod.synth_survey(shape, nblob=8, seed=2)
    vol += np.random.default_rng(2).random(vol.shape, dtype=np.float32) * np.float32(0.05)
    want = dr.dense_bin(vol, dr.mesh(oracle_mod), units)
    got = _dev_bin(hip, vol, units)
    _assert_bits(got, want, "dense_bin %s" % (shape,))
    # at most three channels per voxel, and the rest +0.0
    assert np.count_nonzero(got, axis=0).max() <= 3


def test_dense_normalize_stage_bit_exact(hip):
    import torch
    rng = np.random.default_rng(3)
    h = rng.random((12, 7, 5, 3), dtype=np.float32) * np.float32(3)
    h[:, 0] = 0                                   # all-zero voxels stay zero
    h[:, 1, 0, 0] = np.float32(1e-30)             # tiny ones: the DBL_EPSILON term dominates
    t = torch.from_numpy(h).cuda()
    hip.dense_normalize(t)
    got = t.cpu().numpy()
    _assert_bits(got, dr.normalize(h), "dense_normalize")
    assert np.all(got[:, 0] == 0) and not np.isnan(got).any()


@pytest.mark.parametrize("units", [(1.0, 1.0, 1.0), (0.8, 0.8, 2.0)])
def test_integer_shift_shifts_output(hip, oracle_mod, units):
    sigma = 1.6
    big = oracle_mod.synth_survey((36, 30, 28), nblob=60, seed=5)
    big += np.random.default_rng(5).random(big.shape, dtype=np.float32) * np.float32(0.02)
    dz, dy, dx = 3, 2, 5
    small = big[dz:, dy:, dx:]                    # (nx = 31: the scalar path; the big one takes float4)
    A = _dev(hip, big, sigma, units)
    B = _dev(hip, small, sigma, units)
    # every stage reads at most hw / u_axis (+1 for the gradient) voxels away
    m = [int(math.ceil(_hw(sigma) / u)) + 2 for u in units]           # x, y, z margins
    nz, ny, nx = small.shape
    inner = (slice(None), slice(m[2], nz - m[2]), slice(m[1], ny - m[1]), slice(m[0], nx - m[0]))
    assert B[inner].size > 0
    _assert_bits(B[inner], A[:, dz:, dy:, dx:][inner], "shifted output")


def test_mirror_permutes_channels(hip, oracle_mod):
    V = dr.vertices(oracle_mod)
    perm = [int(np.argmin(np.abs(V - V[c] * np.float32([-1, 1, 1])).sum(1))) for c in range(12)]
    assert sorted(perm) == list(range(12)) and perm != list(range(12))
    vol = oracle_mod.synth_survey((40, 24, 20), nblob=40, seed=6)
    for units in ((1.0, 1.0, 1.0), (0.7, 1.0, 2.5)):
        D = _dev(hip, vol, 1.6, units)
        Df = _dev(hip, vol[:, :, ::-1], 1.6, units)
        # (the reference's FIR edge rules are not mirror symmetric: compare beyond the x pass's reach)
        m = int(math.ceil(_hw(1.6) / units[0])) + 2
        diff = np.abs(Df[perm][:, :, :, ::-1] - D)[:, :, :, m:-m]
        assert diff.max() < 1e-5, (units, diff.max())


def test_flat_regions_zero_and_unit_norms(hip, oracle_mod):
    const = np.full((20, 18, 24), 3.25, np.float32)
    got = _dev(hip, const, 1.6)
    assert np.all(got.view(np.uint32) == 0)
    rng = np.random.default_rng(7)
    v = np.full((20, 18, 40), 0.5, np.float32)
    v[:, :, :16] = rng.random((20, 18, 16), dtype=np.float32)
    for units in ((1.0, 1.0, 1.0), (0.8, 0.8, 2.0)):
        D = _dev(hip, v, 1.6, units)
        zero = np.all(D == 0, axis=0)
        nrm = np.sqrt((D.astype(np.float64) ** 2).sum(0))
        assert np.abs(nrm[~zero] - 1).max() < 1e-6
        # the flat part beyond the window's reach of the noise is exactly zero
        reach = 16 + int(math.ceil(_hw(1.6) / units[0])) + 1
        assert np.all(zero[:, :, reach:]) and not np.any(zero[:, :, :16])
        assert not np.isnan(D).any()


def test_output_over_2g_elements(hip, oracle_mod):
    import torch
    nx, ny, nz = 576, 576, 544                   # 12 N > 2^31: channel 11 ends at 2.17e9
    N = nx * ny * nz
    assert 12 * N > 2 ** 31 and 11 * N < 2 ** 31
    sigma, hw, K = 1.6, _hw(1.6), 4
    g = torch.Generator(device="cuda")
    g.manual_seed(123)
    src = torch.rand((nz, ny, nx), generator=g, device="cuda")
    out = torch.empty((12, nz, ny, nx), dtype=torch.float32, device="cuda")
    m = dr.mesh(oracle_mod)
    # the bin stage: the top planes of every channel (channel 11's lie beyond 2^31 elements)
    hip.dense_bin(src, out)
    top = src[nz - 8:].cpu().numpy()
    want = dr.dense_bin(top, m)[:, 1:]
    got = out[:, nz - 7:].cpu().numpy()
    _assert_bits(got, want, "dense_bin, top planes")
    # the whole image: the top K planes against the restatement on a z-slab (planes z0 .. nz - 1)
    hip.dense_descriptors(src, out, sigma)
    z0 = nz - K - hw - 1
    slab = src[z0:].cpu().numpy()
    torch.cuda.synchronize()
    h = dr.dense_bin(slab, m)
    taps = oracle_mod.gauss_taps(sigma)
    lo = slab.shape[0] - K
    blurred = np.empty((12, K) + slab.shape[1:], np.float32)
    for c in range(12):
        a, r = oracle_mod.fir_axis(h[c], taps, 0)
        assert r == 0
        a, r = oracle_mod.fir_axis(a, taps, 1)
        assert r == 0
        a, r = oracle_mod.fir_axis(a, taps, 2, n_glob=nz, off=z0, out_lo=lo, out_hi=slab.shape[0])
        assert r == 0
        blurred[c] = a[lo:]
    want = dr.normalize(blurred)
    got = out[:, nz - K:].cpu().numpy()
    _assert_bits(got[11], want[11], "last channel, top planes")
    _assert_bits(got, want, "all channels, top planes")
    del out, src
    torch.cuda.empty_cache()


def test_non_default_stream(hip, oracle_mod):
    import torch
    vol = oracle_mod.synth_survey((32, 28, 24), nblob=30, seed=8)
    want = dr.dense_descriptors(vol * np.float32(2) + np.float32(1), oracle_mod, 1.6, (1.0, 1.0, 1.5))
    base = torch.from_numpy(vol).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    try:
        with torch.cuda.stream(s):
            hip.current_stream(refresh=True)
            for _ in range(3):                       # enough queued work that a missing order would show
                src = base * 2 + 1
            out = torch.empty((12,) + tuple(src.shape), dtype=torch.float32, device="cuda")
            hip.dense_descriptors(src, out, 1.6, (1.0, 1.0, 1.5))
            host = out.to("cpu", non_blocking=False)
        s.synchronize()
    finally:
        hip.current_stream(refresh=True)
    _assert_bits(host.numpy(), want, "on a side stream")


def test_api_tensor_and_image_agree(hip, oracle_mod):
    import torch
    from sift3d_amd import api
    vol = oracle_mod.synth_survey((28, 24, 20), nblob=20, seed=9)
    units = (0.8, 0.8, 2.0)
    t = api.dense_descriptors(torch.from_numpy(vol).cuda(), sigma=1.6, units=units)
    assert isinstance(t, torch.Tensor) and tuple(t.shape) == (12, 20, 24, 28)
    im = api.Image.from_array(vol, units)
    a = api.dense_descriptors(im, sigma=1.6)           # the Image's units
    assert isinstance(a, np.ndarray) and a.shape == (12, 20, 24, 28)
    _assert_bits(t.cpu().numpy(), a, "tensor vs Image")
    _assert_bits(api.dense_descriptors(vol, 1.6, units), a, "array vs Image")
    _assert_bits(a, dr.dense_descriptors(vol, oracle_mod, 1.6, units), "Image vs restatement")
    # units default to (1, 1, 1) for tensors and arrays
    _assert_bits(api.dense_descriptors(vol), api.dense_descriptors(torch.from_numpy(vol).cuda()).cpu().numpy(),
                 "default units")
