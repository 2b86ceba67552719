"""The one-launch blur (sift3d_hip_fir_xyz, k_fir_xyz_dma) against the two launches it replaces.

The reference is hip.fir(axis 0) followed by hip.fir_yz on the same input -- where that y+z kernel refuses
a volume (an axis shorter than width + 1: nz = 3 always, nz = 9 from 9 taps on) by the y and z passes of
hip.fir, which is what its callers run then.  Those launches are pinned to the reference implementation by
test_fir_golden and the level digests; here every comparison is bit for bit.

Every edge case of the kernel sits in a small volume: one tile column (both x faces in one workgroup), first /
interior / last columns, the minimum of two tile rows and three, z extents shorter than every window
(mirrored and virtual planes overlap), shorter than the wide ones, and longer than one turn of the 17-tap ring.
"""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the octave-0 sigmas of the 512^3 benchmark (5, 7, 9, 11, 13 and 17 taps), and one that gives 3 taps
SIGMAS = [0.3, 0.5387011637869722, 0.9732939207323564, 1.2262734984654078, 1.5450077936447955,
          1.9465878414647133, 2.4525469969308156]
WIDTHS = [3, 5, 7, 9, 11, 13, 17]
SHAPES = list(itertools.product((3, 9, 40), (128, 192), (64, 128, 192)))     # (nz, ny, nx)
GUARD = 4096


def _filters():
    from sift3d_amd import api
    taps = [api.gauss_filter(s) for s in SIGMAS]
    assert [len(t) for t in taps] == WIDTHS
    return taps


def _guarded(shape, fill=None):
    """A tensor of `shape` between two NaN guard bands (16-byte aligned); returns (whole buffer, view)."""
    import torch
    n = int(np.prod(shape))
    big = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
    view = big[GUARD:GUARD + n].view(shape)
    if fill is not None:
        view.copy_(fill)
    return big, view


def _guards_intact(big):
    import torch
    return bool(torch.isnan(big[:GUARD]).all()) and bool(torch.isnan(big[-GUARD:]).all())


def _noise(shape, seed):
    import torch
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32)).cuda()


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _pair(src, taps, scale_max=None):
    """The blur by the launches the one-launch kernel replaces."""
    import torch
    from sift3d_amd import hip
    tmp, out = torch.empty_like(src), torch.empty_like(src)
    if scale_max is None:
        hip.fir(src, tmp, 0, taps)
    else:
        assert hip.fir_x_scaled(src, tmp, taps, scale_max)
    if not hip.fir_yz(tmp, out, taps):
        tmp2 = torch.empty_like(src)
        hip.fir(tmp, tmp2, 1, taps)
        hip.fir(tmp2, out, 2, taps)
    return out


def _fused(vol, taps, scale_max=None):
    """The one-launch blur with guard bands around source and destination; checks them and the output."""
    import torch
    from sift3d_amd import hip
    sbig, src = _guarded(vol.shape, vol)
    dbig, dst = _guarded(vol.shape)
    assert hip.fir_xyz(src, dst, taps, scale_max)
    torch.cuda.synchronize()
    assert _guards_intact(sbig) and _guards_intact(dbig)
    assert torch.equal(src, vol)
    assert not bool(torch.isnan(dst).any())
    return dst


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % (s[2], s[1], s[0]))
def test_fir_xyz_matches_the_pair(shape):
    vol = _noise(shape, 1234 + sum(shape))
    for taps in _filters():
        ref = _pair(vol, taps)
        got = _fused(vol, taps)
        assert np.array_equal(_bits(got), _bits(ref)), "width %d" % len(taps)


@pytest.mark.parametrize("shape", [(3, 128, 64), (9, 192, 128), (40, 128, 192)],
                         ids=lambda s: "%dx%dx%d" % (s[2], s[1], s[0]))
def test_fir_xyz_scaled_matches_the_pair(shape):
    import torch
    vol = _noise(shape, 99 + sum(shape))
    smax = vol.abs().max().reshape(1).contiguous()
    assert float(smax) != 1.0
    for taps in _filters():
        ref = _pair(vol, taps, smax)
        got = _fused(vol, taps, smax)
        assert np.array_equal(_bits(got), _bits(ref)), "width %d" % len(taps)
    # an all-zero volume: its maximum 0 leaves it alone
    zero = torch.zeros(shape, device="cuda")
    zmax = torch.zeros(1, device="cuda")
    for taps in _filters():
        ref = _pair(zero, taps, zmax)
        got = _fused(zero, taps, zmax)
        assert np.array_equal(_bits(got), _bits(ref)), "width %d" % len(taps)
        assert not _bits(got).any()


@pytest.mark.parametrize("shape,units", [((9, 128, 60), (1.0, 1.0, 1.0)), ((9, 64, 128), (1.0, 1.0, 1.0)),
                                         ((9, 128, 128), (0.5, 1.0, 1.0)), ((9, 128, 128), (1.0, 1.0, 0.5)),
                                         ((9, 128, 128), (1.0, 2.0, 1.0))])
def test_fir_xyz_refuses_what_it_does_not_cover(shape, units):
    import torch
    from sift3d_amd import hip
    vol = _noise(shape, 7)
    for taps in _filters():
        dbig, dst = _guarded(shape)
        assert hip.fir_xyz(vol, dst, taps, None, units) is False
        torch.cuda.synchronize()
        assert bool(torch.isnan(dbig).all())
    # 19 taps, an even width and source == destination are refused as well
    dbig, dst = _guarded((9, 128, 128))
    src = _noise((9, 128, 128), 8)
    for bad in (np.ones(19, np.float32) / 19, np.ones(4, np.float32) / 4):
        assert hip.fir_xyz(src, dst, bad) is False
    assert hip.fir_xyz(dst, dst, _filters()[1]) is False
    torch.cuda.synchronize()
    assert bool(torch.isnan(dbig).all())
