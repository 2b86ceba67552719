"""The two LDS-DMA blur kernels (k_fir_yz_dma behind hip.fir_yz, k_fir_xyz_dma behind hip.fir_xyz) against the
oracle, at every half width they are compiled for.

The kernels share their pipeline code (sift3d_fir_dma.h), so neither is compared with the other: the reference is
oracle_mod.fir_axis (mode 0, unit factor 1), one axis after the other, and every comparison is bit for bit.
Source and destination lie between NaN guard bands that must survive, and the source must come back unchanged.

Shapes (nz, ny, nx) are the smallest at which each mechanism can go wrong:
  y+z, whole volume   (2 hw + 2, 128, 64): the fewest planes the entry accepts -- mirrored and virtual planes
                      overlap --, one tile column, the virtual rows in the last of two or four tile rows;
                      (70, 192, 128): two z segments of 35 planes (p0 > 0, more than one turn of the 17-tap ring),
                      three tile rows, two tile columns
  y+z, as slabs       (70, 128, 64) cut in three with a halo of hw + 1 planes: both global faces and interior
                      slab faces (off, z_lo, z_hi)
  x+y+z               (3, 128, 64): both x faces in one workgroup, nz shorter than every window;
                      (70, 128, 192): first, interior and last tile columns, two z segments;
                      each unscaled and divided by max|v| (the oracle's input there is the volume divided by
                      sift3d_hip_scale, which shares no code with these kernels)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# half width -> sigma: the octave-0 sigmas of the 512^3 benchmark, 0.3 for 3 taps and 2.2 for 15
SIGMA = {1: 0.3, 2: 0.5387011637869722, 3: 0.9732939207323564, 4: 1.2262734984654078, 5: 1.5450077936447955,
         6: 1.9465878414647133, 7: 2.2, 8: 2.4525469969308156}
HALF_WIDTHS = sorted(SIGMA)
GUARD = 4096


@pytest.fixture(scope="module")
def gpu():
    import torch
    from sift3d_amd import api, hip
    if not torch.cuda.is_available() or not api.device_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    hip.lib()
    return api, hip, torch


def _taps(api, hw):
    taps = api.gauss_filter(SIGMA[hw])
    assert len(taps) == 2 * hw + 1
    return taps


def _noise(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _guarded(torch, shape, fill=None):
    """A tensor of `shape` between two NaN guard bands (16-byte aligned), itself NaN or a copy of `fill`."""
    n = int(np.prod(shape))
    big = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
    view = big[GUARD:GUARD + n].view(shape)
    if fill is not None:
        view.copy_(torch.from_numpy(fill))
    return big, view


def _intact(torch, big):
    return bool(torch.isnan(big[:GUARD]).all()) and bool(torch.isnan(big[-GUARD:]).all())


def _oracle(oracle_mod, vol, taps, axes):
    for ax in axes:
        vol, r = oracle_mod.fir_axis(vol, taps, ax, uf=np.float32(1.0), mode=0)
        assert r == 0
    return vol


def _takes_dma(shape):
    """launch_fir_yz's condition for k_fir_yz_dma (with ts <= 256, which holds for nz <= 70).  The kernel choice is
    inferred from that condition, not observed: hip.fir_yz returns True for k_fir_yz_u1 as well."""
    nz, ny, nx = shape
    return nx % 64 == 0 and ny % 64 == 0 and ny >= 128


def _run_yz(gpu, vol, taps, **slab):
    """hip.fir_yz between guard bands; returns the destination as an array (NaN where nothing was written)."""
    api, hip, torch = gpu
    assert _takes_dma(vol.shape)
    sbig, src = _guarded(torch, vol.shape, vol)
    dbig, dst = _guarded(torch, vol.shape)
    assert hip.fir_yz(src, dst, taps, **slab) is True
    torch.cuda.synchronize()
    assert _intact(torch, sbig) and _intact(torch, dbig)
    np.testing.assert_array_equal(src.cpu().numpy(), vol)
    return dst.cpu().numpy()


@pytest.mark.parametrize("hw", HALF_WIDTHS)
def test_fir_yz_dma_vs_oracle(gpu, oracle_mod, hw):
    taps = _taps(gpu[0], hw)
    for shape in ((2 * hw + 2, 128, 64), (70, 192, 128)):
        vol = _noise(shape, 100 * hw + shape[0])
        want = _oracle(oracle_mod, vol, taps, (1, 2))
        got = _run_yz(gpu, vol, taps)
        np.testing.assert_array_equal(got, want, err_msg="shape %r" % (shape,))


@pytest.mark.parametrize("hw", HALF_WIDTHS)
def test_fir_yz_dma_slabs_vs_oracle(gpu, oracle_mod, hw):
    taps = _taps(gpu[0], hw)
    shape = (70, 128, 64)
    nz = shape[0]
    vol = _noise(shape, 200 + hw)
    want = _oracle(oracle_mod, vol, taps, (1, 2))
    reach = hw + 1
    for z0, z1 in ((0, nz // 3), (nz // 3, 2 * nz // 3), (2 * nz // 3, nz)):
        lo, hi = max(0, z0 - reach), min(nz, z1 + reach)
        got = _run_yz(gpu, vol[lo:hi], taps, n_glob=nz, off=lo, z_lo=z0 - lo, z_hi=z1 - lo)
        np.testing.assert_array_equal(got[z0 - lo:z1 - lo], want[z0:z1], err_msg="slab %d:%d" % (z0, z1))
        # planes outside [z_lo, z_hi) are not the launch's to write
        assert np.isnan(got[:z0 - lo]).all() and np.isnan(got[z1 - lo:]).all()


@pytest.mark.parametrize("hw", HALF_WIDTHS)
def test_fir_xyz_dma_vs_oracle(gpu, oracle_mod, hw):
    api, hip, torch = gpu
    taps = _taps(api, hw)
    for shape in ((3, 128, 64), (70, 128, 192)):
        vol = _noise(shape, 300 * hw + shape[0])
        for scaled in (False, True):
            smax, ref_in = None, vol
            if scaled:
                smax = torch.from_numpy(np.abs(vol).max().reshape(1)).cuda()
                assert float(smax) != 1.0
                scaled_vol = torch.empty(shape, device="cuda")
                hip.scale(torch.from_numpy(vol).cuda(), scaled_vol, smax)
                ref_in = scaled_vol.cpu().numpy()
            want = _oracle(oracle_mod, ref_in, taps, (0, 1, 2))
            sbig, src = _guarded(torch, shape, vol)
            dbig, dst = _guarded(torch, shape)
            assert hip.fir_xyz(src, dst, taps, smax) is True
            torch.cuda.synchronize()
            assert _intact(torch, sbig) and _intact(torch, dbig)
            np.testing.assert_array_equal(src.cpu().numpy(), vol)
            np.testing.assert_array_equal(dst.cpu().numpy(), want,
                                          err_msg="shape %r%s" % (shape, ", scaled" if scaled else ""))
