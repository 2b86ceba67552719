"""Thin-plate-spline resampling on the device (sift3d_hip_warp_tps) and deformable registration end to end.

The kernel's arithmetic is fixed (include/sift3d_amd.h, "Thin-plate spline"), so the numpy restatement
(tests/tps_restatement.py) must match it bit for bit: float64 affine part, float32 radial sum in point
order, then the affine warp's sampling."""
import numpy as np
import pytest

from tests import tps_restatement as tr
from tests.test_warp import about_center, dev_warp, rand_vol, rot

pytestmark = pytest.mark.gpu


def dev_tps(src, tps, out_shape, interp="linear", fill=0.0):
    import torch
    from sift3d_amd import hip
    dst = torch.empty(out_shape, dtype=torch.float32, device=src.device)
    hip.warp_tps(src, dst, tps, interp, fill)
    return dst


def random_tps(m, src_shape, out_shape, seed, disp=2.0, reach=1.15):
    """control points over (and a little beyond) the output grid; an affine that maps the output onto the
    source with its edges outside; weights scaled so that the radial part moves samples by about `disp`
    source voxels (rms)"""
    from sift3d_amd import api
    rng = np.random.default_rng(seed)
    ext = np.array(out_shape[::-1], np.float64)
    ctrl = rng.uniform(-0.1, 1.1, (m, 3)) * ext
    w = rng.normal(0, 1, (m, 3))
    w -= w.mean(0)                                      # keeps the spline bounded far away
    probe = rng.uniform(0, 1, (64, 3)) * ext
    s = -np.sqrt(((probe[:, None, :] - ctrl[None, :, :]) ** 2).sum(-1)) @ w
    w *= disp / max(float(np.sqrt((s ** 2).mean())), 1e-30)
    M = rot((1, -2, 0.5), 17.0) * (np.array(src_shape[::-1]) / ext * reach)[:, None]
    A = about_center(M, src_shape, out_shape, (0.3, -0.6, 0.45))
    return api.TPS(ctrl, w, A)


def _sampled(src, out, tps, interp, fill, idx):
    """out at flat indices idx against the restatement"""
    oz, oy, ox = out.shape
    flat = src.reshape(-1)
    z, rem = np.divmod(idx, oy * ox)
    y, x = np.divmod(rem, ox)
    gather = lambda k: flat[k]                          # noqa: E731
    want, ins = tr.ref_tps_points(gather, src.shape, tps, x, y, z, interp, fill)
    got = out.reshape(-1)[idx]
    np.testing.assert_array_equal(got, want)
    return ins


# ---- bit for bit against the restatement ---------------------------------------------------------
@pytest.mark.parametrize("m", [1, 4, 5, 257, 1000])
@pytest.mark.parametrize("interp", ["linear", "nearest"])
def test_odd_shapes_bit_exact_against_restatement(m, interp):
    S, O = (11, 23, 37), (7, 31, 29)
    src = rand_vol(S, 100 + m)
    s = src.cpu().numpy()
    tps = random_tps(m, S, O, m, disp=2.0)
    for fill in (0.0, -3.25):
        got = dev_tps(src, tps, O, interp, fill).cpu().numpy()
        want, ins = tr.ref_tps_warp(s, tps, O, interp, fill)
        np.testing.assert_array_equal(got, want)
        assert 0.2 < ins.mean() < 0.95                  # samples inside and outside the source


def test_single_voxel_axes_against_restatement():
    for S, O in (((1, 23, 37), (7, 1, 29)), ((11, 23, 1), (1, 31, 1)), ((11, 1, 37), (5, 9, 70))):
        src = rand_vol(S, 7)
        s = src.cpu().numpy()
        tps = random_tps(9, S, O, 3, disp=1.0)
        for interp in ("linear", "nearest"):
            got = dev_tps(src, tps, O, interp, 1.5).cpu().numpy()
            want, _ = tr.ref_tps_warp(s, tps, O, interp, 1.5)
            np.testing.assert_array_equal(got, want)


# ---- zero weights: warp_affine's bits ------------------------------------------------------------
def test_zero_weights_equal_warp_affine():
    import torch
    from sift3d_amd import api
    S, O = (41, 50, 70), (37, 45, 66)
    src = rand_vol(S, 3)
    ident = np.hstack([np.eye(3), np.zeros((3, 1))])
    trans = np.hstack([np.eye(3), np.array([[3.0], [-2.5], [5.25]])])
    obl = about_center(rot((1, 2, 3), 23.0), S, O, (0.37, -0.61, 0.45))
    ctrl = np.random.default_rng(4).uniform(0, 60, (13, 3))
    for A in (ident, trans, obl):
        for interp in ("linear", "nearest"):
            got = dev_tps(src, api.TPS(ctrl, np.zeros((13, 3)), A), O, interp, -1.0)
            want = dev_warp(src, A, O, interp, -1.0)
            assert torch.equal(got, want)


# ---- large outputs, streams, launch splits, host images --------------------------------------------
def test_output_over_2_31_elements():
    import torch
    S, O = (11, 23, 37), (2049, 1024, 1024)             # 2.15e9 outputs, 8.6 GB
    assert int(np.prod(O)) > 2 ** 31
    src = rand_vol(S, 5)
    s = src.cpu().numpy()
    tps = random_tps(3, S, O, 5, disp=1.0)
    out = dev_tps(src, tps, O, "linear", -7.0)
    rng = np.random.default_rng(6)
    n = int(np.prod(O))
    idx = np.concatenate([rng.integers(0, n, 20000), rng.integers(n - 3 * 1024 * 1024, n, 20000),
                          np.arange(n - 4096, n), np.arange(2 ** 31 - 2048, 2 ** 31 + 2048)])
    idx_t = torch.from_numpy(idx).to(out.device)
    got = out.reshape(-1)[idx_t].cpu().numpy()
    del out
    torch.cuda.empty_cache()
    oz, oy, ox = O
    z, rem = np.divmod(idx, oy * ox)
    y, x = np.divmod(rem, ox)
    flat = s.reshape(-1)
    want, ins = tr.ref_tps_points(lambda k: flat[k], S, tps, x, y, z, "linear", -7.0)
    np.testing.assert_array_equal(got, want)
    assert 0.05 < ins.mean() < 0.95


def test_non_default_stream():
    import torch
    from sift3d_amd import hip
    S = (33, 45, 61)
    tps = random_tps(300, S, S, 8, disp=2.0, reach=1.0)
    src = rand_vol(S, 11)
    want = dev_tps(src, tps, S).cpu()
    # the warp's input is produced on stream s behind several milliseconds of other work
    src2 = torch.zeros_like(src)
    big = torch.ones((256, 512, 512), device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    try:
        with torch.cuda.stream(s):
            hip.current_stream(refresh=True)
            for _ in range(20):
                big.mul_(1.0001)
            src2.copy_(src)
            dst = torch.full(S, -9.0, device="cuda")
            hip.warp_tps(src2, dst, tps)
            got = dst.clone()
        hip.current_stream(refresh=True)
        torch.cuda.current_stream().wait_stream(s)
        assert torch.equal(got.cpu(), want)
    finally:
        hip.current_stream(refresh=True)
    with pytest.raises(RuntimeError):
        hip.warp_tps(src, src, tps)


def test_split_launches_equal_one_launch():
    """A grid split into several launches gives the bits of a grid computed in one: the output voxel
    (x, y, z) does not depend on the output's shape, so rows 0 .. oy_b - 1 of a tall grid (split) must equal
    a short grid (one launch), planes past the first split included."""
    from sift3d_amd import hip
    m, S = 16384, (40, 50, 60)
    ox, oz, oy_b = 64, 256, 4
    assert hip.warp_tps_launches((oz, oy_b, ox), m) == 1
    oy_a = 64
    while hip.warp_tps_launches((oz, oy_a, ox), m) < 2:
        oy_a *= 2
        assert oy_a <= 4096
    src = rand_vol(S, 13)
    tps = random_tps(m, S, (oz, oy_a, ox), 14, disp=2.0, reach=0.9)
    a = dev_tps(src, tps, (oz, oy_a, ox), "linear", -1.0).cpu().numpy()
    b = dev_tps(src, tps, (oz, oy_b, ox), "linear", -1.0).cpu().numpy()
    print("split: %d launches for %s, m = %d" % (hip.warp_tps_launches((oz, oy_a, ox), m), (oz, oy_a, ox), m))
    np.testing.assert_array_equal(a[:, :oy_b, :], b)
    # and the restatement on a sample of both grids, the last planes included
    rng = np.random.default_rng(15)
    s = src.cpu().numpy()
    for out in (a, b):
        n = out.size
        idx = np.concatenate([rng.integers(0, n, 300), np.arange(n - 64, n)])
        _sampled(s, out, tps, "linear", -1.0, idx)


def test_host_image_path_equals_device_path():
    from sift3d_amd import api
    S, O = (29, 35, 47), (31, 33, 45)
    tps = random_tps(77, S, O, 21, disp=2.0)
    src = rand_vol(S, 12)
    s = src.cpu().numpy()
    for interp in ("linear", "nearest"):
        dev = dev_tps(src, tps, O, interp, -2.0).cpu().numpy()
        np.testing.assert_array_equal(api.warp_tps(s, tps, O, interp, -2.0), dev)
        im = api.warp_tps(api.Image.from_array(s), tps, O, interp, -2.0)
        assert isinstance(im, api.Image) and im.shape == O
        np.testing.assert_array_equal(im.data(), dev)


# ---- deformable registration end to end -------------------------------------------------------------
def _known_deformation(n):
    """moving voxel -> fixed voxel: a 4-degree rotation about the centre plus eight Gaussian bumps of 4 voxels
    (sigma 24), as a TPS through a 10^3 grid of its values; its non-affine part is 1.5 voxels rms"""
    from sift3d_amd import api
    c0 = np.full(3, (n - 1) / 2.0)
    R = rot((0.4, 1.0, -0.3), 4.0)
    rng = np.random.default_rng(2024)
    mu = c0 + rng.uniform(-0.3, 0.3, (8, 3)) * n
    amp = rng.normal(0, 1, (8, 3))
    amp *= 4.0 / np.linalg.norm(amp, axis=1, keepdims=True)

    def T(p):
        out = (p - c0) @ R.T + c0
        for b in range(len(mu)):
            g = np.exp(-((p - mu[b]) ** 2).sum(1) / (2 * 24.0 ** 2))
            out += g[:, None] * amp[b]
        return out

    g = np.linspace(-0.1 * n, 1.1 * n, 10)
    grid = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return api.tps_fit(grid, T(grid), 0.0, 4096), T


def _ncc(a, b):
    a = a.astype(np.float64) - a.mean()
    b = b.astype(np.float64) - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def test_register_deformable_recovers_a_smooth_deformation():
    import torch
    from sift3d_amd import api, hip
    n = 176
    fixed = torch.empty((n, n, n), device="cuda")
    hip.synth_lattice(fixed, 0, 21)
    known, T = _known_deformation(n)
    moving = dev_tps(fixed, known, fixed.shape)
    torch.cuda.synchronize()
    res = api.register_deformable(moving, fixed)
    aff = api.register(moving, fixed)
    assert tuple(res.warped.shape) == tuple(fixed.shape)
    assert len(res.inliers) == res.num_matches == aff.num_matches
    lo, hi = n // 8, n - n // 8
    f = fixed.cpu().numpy()[lo:hi, lo:hi, lo:hi]
    ncc_d = _ncc(res.warped.cpu().numpy()[lo:hi, lo:hi, lo:hi], f)
    ncc_a = _ncc(aff.warped.cpu().numpy()[lo:hi, lo:hi, lo:hi], f)
    # the composed map known o recovered at the fixed volume's keypoints, inner region
    det, kp = api.Detector(), api.KeypointStore()
    assert det.detect_keypoints(api.Image.from_array(fixed.cpu().numpy()), kp) == 0
    r = kp.records()
    pts = np.stack([r["xd"], r["yd"], r["zd"]], 1)
    pts = pts[((pts >= lo) & (pts <= hi)).all(1)]
    err = np.linalg.norm(api.tps_apply(known, api.tps_apply(res.tps, pts)) - pts, axis=1)
    # the same for the affine: moving -> fixed is A, so fixed -> moving is its inverse
    Ai = api.affine_invert(aff.A)
    err_a = np.linalg.norm(api.tps_apply(known, pts @ Ai[:, :3].T + Ai[:, 3]) - pts, axis=1)
    print("register_deformable: %d matches, %d inliers, %d control points; NCC %.4f (affine %.4f); "
          "composed error at %d keypoints: median %.3f, p90 %.3f voxel (affine: median %.3f)"
          % (res.num_matches, res.inliers.sum(), len(res.tps.ctrl), ncc_d, ncc_a, len(pts), np.median(err),
             np.percentile(err, 90), np.median(err_a)))
    # measured on an MI355X: 611 matches, 569 inliers; NCC 0.9848 against 0.9334 for the affine; median error
    # 0.484 voxel (p90 0.887) against 1.326 for the affine
    assert res.inliers.sum() >= 100 and len(pts) >= 100
    assert ncc_d >= ncc_a + 0.03
    assert np.median(err) <= 0.75
    assert np.median(err) <= 0.6 * np.median(err_a)
