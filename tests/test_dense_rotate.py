"""GPU: rotation-invariant dense descriptors (sift3d_amd_dense_descriptors_rotate_device and its stages).
The orientation (R2) is pinned to the oracle's assign_eig_ori at every voxel; descriptors are pinned to
the numpy restatement (tests/dense_rotate_restatement.py) bit for bit; exact lattice rotations of the
volume leave the descriptors where the non-rotating variant's change."""
import numpy as np
import pytest

from tests import dense_restatement as dr
from tests import dense_rotate_restatement as drr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    from sift3d_amd import hip as h
    h.lib()
    assert torch.cuda.is_available()
    h.current_stream(refresh=True)
    return h


def _assert_bits(got, want, what):
    assert got.shape == want.shape, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    if bad.any():
        i = tuple(int(a[0]) for a in np.nonzero(bad))
        raise AssertionError("%s: %d of %d values differ, first at %s: %r != %r"
                             % (what, int(bad.sum()), bad.size, i, got[i], want[i]))


def _vol(oracle_mod, shape, seed, flat=False):
    vol = oracle_mod.synth_survey(shape, nblob=max(4, int(np.prod(shape)) // 400), seed=seed)
    vol += np.random.default_rng(seed).random(vol.shape, dtype=np.float32) * np.float32(0.05)
    if flat:
        vol[:, :, : vol.shape[2] // 2] = np.float32(0.25)
    return vol


def _orient(hip, vol, sigma, units):
    import torch
    src = torch.from_numpy(np.ascontiguousarray(vol, np.float32)).cuda()
    R = torch.full((3, 3) + tuple(src.shape), float("nan"), device="cuda")
    keep = torch.full(tuple(src.shape), 7, dtype=torch.uint8, device="cuda")
    hip.dense_orient(src, R, keep, sigma, units)
    return R.cpu().numpy(), keep.cpu().numpy()


def _rotate(hip, vol, sigma, units):
    import torch
    src = torch.from_numpy(np.ascontiguousarray(vol, np.float32)).cuda()
    out = torch.full((12,) + tuple(src.shape), float("nan"), device="cuda")
    hip.dense_descriptors_rotate(src, out, sigma, units)
    return out.cpu().numpy()


ORIENT_CASES = [
    # (shape (nx, ny, nz), units, sigma, flat half)
    ((40, 36, 33), (1.0, 1.0, 1.0), 1.5, False),
    ((40, 36, 33), (1.0, 1.0, 1.0), 3.0, False),
    ((26, 22, 20), (0.8, 0.8, 2.0), 1.5, False),
    ((26, 22, 20), (0.8, 0.8, 2.0), 3.0, False),
    ((24, 20, 18), (1.0, 1.0, 1.0), 1.5, True),
    ((1, 9, 7), (1.0, 1.0, 1.0), 1.5, False),
    ((3, 2, 9), (1.0, 1.0, 1.0), 1.5, False),
    ((9, 3, 3), (1.0, 1.0, 1.0), 3.0, False),
    ((1, 1, 1), (1.0, 1.0, 1.0), 1.5, False),
]


@pytest.mark.parametrize("shape,units,sigma,flat", ORIENT_CASES)
def test_orientation_is_the_oracles(hip, oracle_mod, shape, units, sigma, flat):
    vol = _vol(oracle_mod, shape, 7, flat)
    R, keep = _orient(hip, vol, sigma, units)
    oR, okeep = drr.oracle_orient(vol, sigma, units)
    assert np.array_equal(keep, okeep), "keep differs at %d voxels" % int((keep != okeep).sum())
    _assert_bits(R, oR, "R %s units %s sigma %g" % (shape, units, sigma))
    if min(shape) < 3:
        assert not keep.any()


DESC_CASES = [
    ((20, 18, 16), (1.0, 1.0, 1.0), 1.5, False),
    ((19, 17, 15), (0.8, 0.8, 2.0), 1.5, False),
    ((16, 14, 13), (1.0, 1.0, 1.0), 3.0, False),
    ((18, 16, 14), (1.0, 1.0, 1.0), 1.5, True),
    ((1, 9, 7), (1.0, 1.0, 1.0), 1.5, False),
    ((9, 3, 2), (1.0, 1.0, 1.0), 1.5, False),
]


@pytest.mark.parametrize("shape,units,sigma,flat", DESC_CASES)
def test_descriptors_bit_exact_against_restatement(hip, oracle_mod, shape, units, sigma, flat):
    import torch
    vol = _vol(oracle_mod, shape, 3, flat)
    want, wR, wkeep = drr.dense_descriptors_rotate(vol, oracle_mod, sigma, units)
    got = _rotate(hip, vol, sigma, units)
    _assert_bits(got, want, "rotate %s units %s sigma %g" % (shape, units, sigma))
    # the stages one by one
    R, keep = _orient(hip, vol, sigma, units)
    _assert_bits(R, wR, "R")
    assert np.array_equal(keep, wkeep)
    src = torch.from_numpy(vol).cuda()
    h = torch.full((12,) + vol.shape, float("nan"), device="cuda")
    hip.dense_rotate_bin(src, torch.from_numpy(R).cuda(), h, sigma, units)
    raw = drr.rotate_bin(vol, wR, sigma, units, dr.mesh(oracle_mod))
    _assert_bits(h.cpu().numpy(), raw, "rotate_bin")
    if min(shape) < 3:
        assert not got.any()
    if flat:
        nx = vol.shape[2]
        assert not got[:, :, :, : nx // 2 - int(3 * sigma) - 1].any()   # flat windows: D = 0
    if min(shape) >= 3:
        assert got.any()


def test_rotate_bin_uses_R_transpose(hip, oracle_mod):
    """A non-symmetric R: the stage bins R^T g, not R g."""
    import torch
    vol = _vol(oracle_mod, (12, 11, 10), 4)
    c, s = np.float32(0.6), np.float32(0.8)
    Rm = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float32)
    R = np.ascontiguousarray(np.broadcast_to(Rm[:, :, None, None, None], (3, 3) + vol.shape))
    h = torch.empty((12,) + vol.shape, device="cuda")
    hip.dense_rotate_bin(torch.from_numpy(vol).cuda(), torch.from_numpy(R).cuda(), h, 1.5)
    m = dr.mesh(oracle_mod)
    _assert_bits(h.cpu().numpy(), drr.rotate_bin(vol, R, 1.5, (1, 1, 1), m), "R^T")
    RT = np.ascontiguousarray(R.transpose(1, 0, 2, 3, 4))
    assert not np.array_equal(h.cpu().numpy(), drr.rotate_bin(vol, RT, 1.5, (1, 1, 1), m))


def _lattice_rotations():
    # (axes of np.rot90 on [z, y, x]): quarter turns about x, y and z
    return [(0, 1), (0, 2), (1, 2)]


@pytest.mark.parametrize("axes", _lattice_rotations())
def test_rotation_invariance(hip, oracle_mod, axes):
    import torch
    sigma = 1.6
    vol = oracle_mod.synth_survey((44, 44, 44), nblob=40, seed=9)
    vol += np.random.default_rng(9).random(vol.shape, dtype=np.float32) * np.float32(0.02)
    rvol = np.ascontiguousarray(np.rot90(vol, 1, axes))
    m = int(np.ceil(3 * sigma)) + 2

    def frac(rotate):
        from sift3d_amd import api
        D = api.dense_descriptors(torch.from_numpy(vol).cuda(), sigma, rotate=rotate).cpu().numpy()
        Dr = api.dense_descriptors(torch.from_numpy(rvol).cuda(), sigma, rotate=rotate).cpu().numpy()
        back = np.rot90(Dr, -1, (axes[0] + 1, axes[1] + 1))      # D_rot(P v) at v
        _, k = api.dense_orientations(torch.from_numpy(vol).cuda(), sigma)
        _, kr = api.dense_orientations(torch.from_numpy(rvol).cuda(), sigma)
        ok = (k.cpu().numpy() == 1) & (np.rot90(kr.cpu().numpy(), -1, axes) == 1)
        inner = np.zeros_like(ok)
        inner[m:-m, m:-m, m:-m] = True
        sel = ok & inner
        assert sel.sum() > 0.5 * inner.sum()
        close = np.abs(back - D).max(axis=0) <= 1e-4
        return float(close[sel].mean())

    f_rot, f_plain = frac(True), frac(False)
    print("axes %s: rotating %.5f, non-rotating %.5f of voxels within 1e-4" % (axes, f_rot, f_plain))
    assert f_rot >= 0.999, f_rot
    assert f_plain < 0.5, f_plain


def test_output_over_2_31_elements(hip, oracle_mod):
    """12 * n > 2^31: the top planes against the restatement of a crop that holds their whole windows."""
    import torch
    nx, ny, nz = 512, 512, 688
    sigma = 1.5
    g = torch.Generator(device="cuda").manual_seed(5)
    src = torch.rand((nz, ny, nx), device="cuda", generator=g)
    assert 12 * src.numel() > 2 ** 31
    out = torch.empty((12, nz, ny, nx), device="cuda")
    hip.dense_descriptors_rotate(src, out, sigma)
    crop = src[nz - 14:, 200:224, 300:322].cpu().numpy()
    top = out[:, nz - 6:, 200:224, 300:322].cpu().numpy()
    del out
    torch.cuda.empty_cache()
    want, _, _ = drr.dense_descriptors_rotate(crop, oracle_mod, sigma)
    m = int(np.ceil(3 * sigma)) + 1
    _assert_bits(top[:, :, m:-m, m:-m], want[:, -6:, m:-m, m:-m], "top planes")


def test_side_stream_and_entry_points_agree(hip, oracle_mod):
    import torch
    from sift3d_amd import api
    vol = _vol(oracle_mod, (30, 26, 22), 6)
    ref = api.dense_descriptors(api.Image.from_array(vol, (1.0, 1.0, 1.5)), 1.5, rotate=True)
    npy = api.dense_descriptors(vol, 1.5, units=(1.0, 1.0, 1.5), rotate=True)
    _assert_bits(npy, ref, "numpy vs Image")
    s = torch.cuda.Stream()
    src = torch.from_numpy(vol).cuda()
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(s):
            hip.current_stream(refresh=True)
            out = api.dense_descriptors(src, 1.5, units=(1.0, 1.0, 1.5), rotate=True)
            R, keep = api.dense_orientations(src, 1.5, units=(1.0, 1.0, 1.5))
        s.synchronize()
    finally:
        hip.current_stream(refresh=True)
    _assert_bits(out.cpu().numpy(), ref, "side stream vs Image")
    hR, hk = api.dense_orientations(vol, 1.5, units=(1.0, 1.0, 1.5))
    assert isinstance(hR, np.ndarray) and hR.shape == (3, 3) + vol.shape and hk.dtype == np.uint8
    _assert_bits(R.cpu().numpy(), hR, "orientations")
    assert np.array_equal(keep.cpu().numpy(), hk)
    # the default is today's non-rotating image
    _assert_bits(api.dense_descriptors(vol, 1.5, units=(1.0, 1.0, 1.5)),
                 api.dense_descriptors(vol, 1.5, units=(1.0, 1.0, 1.5), rotate=False), "default")


def test_sign_rule_on_a_ramp(hip):
    """gy = gz = 0 exactly: d = 0 for the second column, whose sign is -1 (sift.c's `d > 0`)."""
    nx, ny, nz = 14, 9, 8
    x = np.arange(nx, dtype=np.float32)
    vol = np.ascontiguousarray(np.broadcast_to(x * x * np.float32(0.01) + x, (nz, ny, nx)))
    for sigma in (1.5, 3.0):
        R, keep = _orient(hip, vol, sigma, (1, 1, 1))
        oR, okeep = drr.oracle_orient(vol, sigma, (1, 1, 1))
        assert np.array_equal(keep, okeep) and keep.any()
        _assert_bits(R, oR, "ramp R sigma %g" % sigma)
        assert np.all(R[2, 1][keep == 1] == -1.0)
