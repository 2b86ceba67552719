"""Displacement fields on the device: export (sift3d_hip_affine_field, sift3d_hip_tps_field), resampling
through a field (sift3d_hip_warp_field) and the Jacobian determinant (sift3d_hip_jacobian_det).

The arithmetic is fixed (include/sift3d_amd.h, "Displacement fields"), so the numpy restatement
(tests/field_restatement.py) must match the kernels bit for bit.  Cross-checks against warp_affine / warp_tps,
and the Jacobian against the analytic one of a thin-plate spline, pin the meaning."""
import numpy as np
import pytest

from tests import field_restatement as fr
from tests import tps_restatement as tr
from tests.test_tps import _known_deformation, dev_tps, random_tps
from tests.test_warp import about_center, dev_warp, rand_vol, rot

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits(got, want):
    """bit for bit, the sign of zero included; a NaN matches a NaN (IEEE 754 leaves the sign and payload of
    an operation's NaN result open, and the contract does not fix them)"""
    g, w = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    np.testing.assert_array_equal(np.isnan(g), np.isnan(w))
    ok = ~np.isnan(w)
    np.testing.assert_array_equal(bits(g[ok]), bits(w[ok]))


def dev_affine_field(A, out_shape):
    import torch
    from sift3d_amd import hip
    f = torch.empty((3,) + tuple(out_shape), dtype=torch.float32, device="cuda")
    return hip.affine_field(f, A)


def dev_tps_field(tps, out_shape):
    import torch
    from sift3d_amd import hip
    f = torch.empty((3,) + tuple(out_shape), dtype=torch.float32, device="cuda")
    return hip.tps_field(f, tps)


def dev_warp_field(src, field, interp="linear", fill=0.0):
    import torch
    from sift3d_amd import hip
    dst = torch.empty(tuple(src.shape[:-3]) + tuple(field.shape[1:]), dtype=torch.float32, device="cuda")
    return hip.warp_field(src, dst, field, interp, fill)


def rand_field(out_shape, src_shape, seed, nan=0):
    """a field that sends most outputs inside the source and some outside: p + u uniform over the source
    widened by 15 % on each side, blended with a smooth part; nan voxels get a NaN in one channel"""
    import torch
    rng = np.random.default_rng(seed)
    x, y, z = fr.grid(out_shape)
    u = []
    for d, (p, n, m) in enumerate(zip((x, y, z), src_shape[::-1], out_shape[::-1])):
        target = rng.uniform(-0.15 * n, 1.15 * n, p.shape) if n > 1 else rng.uniform(-0.6, 0.6, p.shape)
        u.append((0.5 * (target - p) + 0.5 * (p * (n - 1) / max(m - 1, 1) - p)).astype(np.float32))
    u = np.stack(u)
    for k in range(nan):
        d = k % 3
        u[d].reshape(-1)[rng.integers(0, u[d].size)] = np.nan
    return torch.from_numpy(u).cuda(), u


# ---- export, bit for bit -----------------------------------------------------------------------------
AFFINES = {
    "oblique": lambda S, O: about_center(rot((1, 2, 3), 23.0) * 1.1, S, O, (0.37, -0.61, 0.45)),
    "flip": lambda S, O: np.array([[0, -1.0, 0, S[1] - 1], [1.0, 0, 0, 0], [0, 0, -1.0, S[0] - 1]]),
    "shear": lambda S, O: np.array([[1.0, 0.3, -0.2, -3.3], [0.01, 0.9, 0.1, 7.1], [-0.25, 0.0, 1.2, 0.5]]),
}


@pytest.mark.parametrize("O", [(7, 31, 29), (1, 5, 3), (13, 2, 70), (9, 1, 1)])
@pytest.mark.parametrize("name", sorted(AFFINES))
def test_affine_field_bit_exact(O, name):
    A = AFFINES[name]((11, 23, 37), O)
    assert_bits(dev_affine_field(A, O).cpu().numpy(), fr.ref_affine_field(A, O))


@pytest.mark.parametrize("m", [1, 5, 257, 1000])
def test_tps_field_bit_exact(m):
    for O in ((7, 31, 29), (9, 4, 65)):
        tps = random_tps(m, (11, 23, 37), O, m, disp=2.0)
        assert_bits(dev_tps_field(tps, O).cpu().numpy(), fr.ref_tps_field(tps, O))


def test_tps_field_zero_weights_is_the_affine_field():
    from sift3d_amd import api
    S, O = (41, 50, 70), (37, 45, 66)
    ctrl = np.random.default_rng(4).uniform(0, 60, (13, 3))
    for name in sorted(AFFINES):
        A = AFFINES[name](S, O)
        got = dev_tps_field(api.TPS(ctrl, np.zeros((13, 3)), A), O).cpu().numpy()
        assert_bits(got, dev_affine_field(A, O).cpu().numpy())


def test_tps_field_split_launches_equal_one_launch():
    """as test_tps.test_split_launches_equal_one_launch: rows 0 .. oy_b - 1 of a tall grid (split) equal a
    short grid (one launch), and both equal the restatement at sampled voxels"""
    from sift3d_amd import hip
    m = 16384
    ox, oz, oy_b = 64, 256, 4
    assert hip.tps_field_launches((oz, oy_b, ox), m) == 1
    oy_a = 64
    while hip.tps_field_launches((oz, oy_a, ox), m) < 2:
        oy_a *= 2
        assert oy_a <= 4096
    assert hip.tps_field_launches((oz, oy_a, ox), m) == hip.warp_tps_launches((oz, oy_a, ox), m)
    tps = random_tps(m, (40, 50, 60), (oz, oy_a, ox), 14, disp=2.0, reach=0.9)
    a = dev_tps_field(tps, (oz, oy_a, ox)).cpu().numpy()
    b = dev_tps_field(tps, (oz, oy_b, ox)).cpu().numpy()
    assert_bits(a[:, :, :oy_b, :], b)
    rng = np.random.default_rng(15)
    for f in (a, b):
        n = f[0].size
        idx = np.concatenate([rng.integers(0, n, 200), np.arange(n - 64, n)])
        z, rem = np.divmod(idx, f.shape[2] * f.shape[3])
        y, x = np.divmod(rem, f.shape[3])
        want = fr.ref_tps_field_points(tps, x, y, z)
        for d in range(3):
            assert_bits(f[d].reshape(-1)[idx], want[d])


# ---- warp_field, bit for bit -------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [1, 3, 12])
@pytest.mark.parametrize("interp", ["linear", "nearest"])
def test_warp_field_bit_exact(nc, interp):
    S, O = (11, 23, 37), (7, 31, 29)
    for fill in (0.0, -3.25):
        src = rand_vol((nc,) + S if nc > 1 else S, 200 + nc)
        fd, fh = rand_field(O, S, nc, nan=5)
        got = dev_warp_field(src, fd, interp, fill).cpu().numpy()
        want = fr.ref_warp_field(src.cpu().numpy(), fh, interp, fill)
        assert_bits(got, want)
        nanvox = np.isnan(fh).any(0)
        assert nanvox.sum() == 5
        chans = got[None] if nc == 1 else got
        assert (chans[:, nanvox] == np.float32(fill)).all()             # a NaN in the field samples outside


def test_warp_field_degenerate_axes_and_row_tails():
    for S, O in (((1, 23, 37), (7, 1, 29)), ((11, 23, 1), (1, 31, 1)), ((2, 2, 2), (5, 9, 70)),
                 ((11, 1, 2), (3, 2, 67)), ((2, 5, 1), (2, 3, 5))):
        for nc in (1, 3):
            src = rand_vol((nc,) + S if nc > 1 else S, 7 + nc)
            fd, fh = rand_field(O, S, 9 + nc, nan=2)
            for interp in ("linear", "nearest"):
                got = dev_warp_field(src, fd, interp, 1.5).cpu().numpy()
                assert_bits(got, fr.ref_warp_field(src.cpu().numpy(), fh, interp, 1.5))


def test_channels_equal_single_channel_warps():
    import torch
    S, O = (19, 33, 41), (21, 30, 44)
    src = rand_vol((12,) + S, 31)
    fd, _ = rand_field(O, S, 32, nan=3)
    for interp in ("linear", "nearest"):
        many = dev_warp_field(src, fd, interp, -2.0)
        for c in range(12):
            one = dev_warp_field(src[c].contiguous(), fd, interp, -2.0)
            assert torch.equal(many[c], one), (interp, c)


def test_affine_field_warp_equals_warp_affine():
    """exact u: the identity, an integer translation into another shape, an axis permutation with flips"""
    S = (41, 50, 70)
    src = rand_vol(S, 3)
    cases = [(np.hstack([np.eye(3), np.zeros((3, 1))]), S),
             (np.hstack([np.eye(3), np.array([[3.0], [-2.0], [5.0]])]), (40, 48, 64)),
             (np.array([[0, 0, -1.0, S[0] - 1], [1.0, 0, 0, 2.0], [0, -1.0, 0, S[1] - 1]]), (66, 39, 45))]
    for A, O in cases:
        field = dev_affine_field(A, O)
        for interp in ("linear", "nearest"):
            for fill in (0.0, -1.5):
                got = dev_warp_field(src, field, interp, fill).cpu().numpy()
                want = dev_warp(src, A, O, interp, fill).cpu().numpy()
                assert_bits(got, want)


# ---- cross-checks against the existing warps -----------------------------------------------------------
def _rounding_bound(q, u, s):
    """|warp_field - warp| for linear sampling when u is the float rounding of q - p: the sample point moves by
    at most 2^-24 |u_d| per axis (half an ulp of u_d, and the double sum p + u is exact below 2^29); trilinear
    sampling moves by at most sum_d (max |neighbour difference| <= 2 max|s|) |dq_d|; the float fractions and
    lerps add a few ulps of max|s|: bound = 2 max|s| * 3 * 2^-24 (max|u| + 1) + 16 * 2^-24 max|s|"""
    smax = float(np.abs(s).max())
    return 2 * smax * 3 * 2.0 ** -24 * (float(np.abs(u).max()) + 1) + 16 * 2.0 ** -24 * smax


def _away_from_the_edge(q, shape, eps=1e-3):
    nz, ny, nx = shape
    ok = np.ones(q[0].shape, bool)
    for qd, n in zip(q, (nx, ny, nz)):
        ok &= (np.abs(qd) > eps) & (np.abs(qd - (n - 1)) > eps)
    return ok


def test_oblique_field_warp_agrees_with_warp_affine():
    S, O = (41, 50, 70), (37, 45, 66)
    src = rand_vol(S, 8)
    A = about_center(rot((1, 2, 3), 23.0), S, O, (0.37, -0.61, 0.45))
    field = dev_affine_field(A, O)
    got = dev_warp_field(src, field, "linear", -1.0).cpu().numpy()
    want = dev_warp(src, A, O, "linear", -1.0).cpu().numpy()
    q = fr.ref_coords(A, *fr.grid(O))
    keep = _away_from_the_edge(q, S)
    bound = _rounding_bound(q, field.cpu().numpy(), src.cpu().numpy())
    err = np.abs(got - want)[keep]
    print("oblique: max |warp_field - warp_affine| = %.3g (bound %.3g), %d of %d voxels differ"
          % (err.max(), bound, np.count_nonzero(err), err.size))
    assert err.max() <= bound
    assert 0.3 < (want[keep] != -1.0).mean() < 1.0


def test_tps_field_warp_agrees_with_warp_tps():
    S, O = (29, 35, 47), (31, 33, 45)
    src = rand_vol(S, 9)
    tps = random_tps(77, S, O, 21, disp=2.0)
    field = dev_tps_field(tps, O)
    got = dev_warp_field(src, field, "linear", -1.0).cpu().numpy()
    want = dev_tps(src, tps, O, "linear", -1.0).cpu().numpy()
    q = tr.ref_tps_coords(tps, *fr.grid(O))
    keep = _away_from_the_edge(q, S)
    bound = _rounding_bound(q, field.cpu().numpy(), src.cpu().numpy())
    err = np.abs(got - want)[keep]
    print("tps: max |warp_field - warp_tps| = %.3g (bound %.3g)" % (err.max(), bound))
    assert err.max() <= bound
    assert 0.3 < (want[keep] != -1.0).mean() < 1.0                           # samples inside and outside


# ---- Jacobian determinant ------------------------------------------------------------------------------
def dev_jac(field_np):
    import torch
    from sift3d_amd import hip
    f = torch.from_numpy(np.ascontiguousarray(field_np, np.float32)).cuda()
    det = torch.empty(tuple(f.shape[1:]), dtype=torch.float32, device="cuda")
    d, folded, mn, mx = hip.jacobian_det(f, det)
    return d.cpu().numpy(), folded, mn, mx


def assert_jac(field_np):
    det, folded, mn, mx = dev_jac(field_np)
    want = fr.ref_jacobian_det(field_np)
    assert_bits(det, want)
    wf, wmn, wmx = fr.ref_stats(want)
    assert folded == wf and mn == wmn and mx == wmx, ((folded, mn, mx), (wf, wmn, wmx))
    _, f2, mn2, mx2 = __import__("sift3d_amd").hip.jacobian_det(
        __import__("torch").from_numpy(np.ascontiguousarray(field_np, np.float32)).cuda())
    assert (f2, mn2, mx2) == (folded, mn, mx)                              # det not written: the same stats
    return det, folded


@pytest.mark.parametrize("O", [(7, 31, 29), (1, 5, 7), (2, 9, 3), (3, 1, 2), (1, 1, 1), (17, 2, 130), (9, 70, 1)])
def test_jacobian_bit_exact(O):
    rng = np.random.default_rng(sum(O))
    f = (rng.normal(0, 0.6, (3,) + O)).astype(np.float32)
    det, folded = assert_jac(f)
    assert 0 <= folded <= det.size
    if det.size > 100:
        assert 0 < folded < det.size                                        # both signs occur


def test_jacobian_nan_fields():
    rng = np.random.default_rng(5)
    O = (6, 11, 13)
    f = rng.normal(0, 0.2, (3,) + O).astype(np.float32)
    f[1, 2, 3, 4] = np.nan
    f[0, 5, 10, 12] = np.nan
    det, folded = assert_jac(f)
    assert np.isnan(det).sum() >= 2 and folded >= np.isnan(det).sum()
    _, folded, mn, mx = dev_jac(np.full((3, 2, 3, 4), np.nan, np.float32))    # no non-NaN det
    assert folded == 24 and mn == np.inf and mx == -np.inf


def test_jacobian_identity_and_affine():
    det, folded, mn, mx = dev_jac(np.zeros((3, 9, 10, 11), np.float32))
    assert (det == 1.0).all() and folded == 0 and mn == mx == 1.0
    for name in sorted(AFFINES):
        O = (40, 64, 33)
        A = AFFINES[name]((64, 64, 64), O)
        f = dev_affine_field(A, O).cpu().numpy()
        det, folded, mn, mx = dev_jac(f)
        want = float(np.linalg.det(A[:, :3]))
        assert np.abs(det - want).max() <= 1e-4 * abs(want), name
        assert folded == (det.size if want < 0 else 0)


def _tps_jacobian(tps, p):
    """the analytic Jacobian of q(p) = A p + sum_i w_i (-|p - c_i|) in double: A3 + sum_i w_i (x) (-(p - c_i)/r_i)"""
    d = p[:, None, :] - tps.ctrl[None, :, :]
    r = np.sqrt((d ** 2).sum(-1))
    J = np.broadcast_to(tps.A[:, :3], (len(p), 3, 3)).copy()
    J += np.einsum("id,nie->nde", tps.weights, -d / r[:, :, None])
    return np.linalg.det(J)


def _inner_voxels(tps, O, margin=4.0):
    x, y, z = fr.grid(O)
    p = np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], 1).astype(np.float64)
    r = np.sqrt(((p[:, None, :] - tps.ctrl[None, :, :]) ** 2).sum(-1)).min(1)
    ok = (r >= margin)
    for k, n in enumerate(O[::-1]):
        ok &= (p[:, k] >= margin) & (p[:, k] <= n - 1 - margin)
    return p, ok


def test_jacobian_against_analytic_tps():
    from sift3d_amd import api
    O = (40, 44, 48)
    tps = random_tps(24, O, O, 41, disp=2.5, reach=1.0)
    f = dev_tps_field(tps, O)
    det, folded, mn, mx = dev_jac(f.cpu().numpy())
    p, ok = _inner_voxels(tps, O)
    ana = _tps_jacobian(tps, p[ok])
    got = det.reshape(-1)[ok].astype(np.float64)
    err = np.abs(got - ana)
    print("analytic TPS Jacobian: %d voxels, max |fd - analytic| %.4f, det in [%.3f, %.3f]"
          % (ok.sum(), err.max(), ana.min(), ana.max()))
    assert ok.sum() > 1000
    assert (err <= 0.02 + 0.02 * np.abs(ana)).all()
    big = np.abs(ana) > 0.1
    assert (np.sign(got[big]) == np.sign(ana[big])).all()
    # a spline that folds: one point, q = p + w (-|p - c|), det = 1 - w . (p - c) / r < 0 where w . dir > 1
    c = np.array([[23.5, 21.5, 19.5]])
    fold = api.TPS(c, np.array([[3.0, 0.5, 0.0]]), tr.IDENT)
    f = dev_tps_field(fold, O).cpu().numpy()
    det, folded, mn, mx = dev_jac(f)
    want = fr.ref_jacobian_det(f)
    assert folded > 0 and folded == fr.ref_stats(want)[0]
    p, ok = _inner_voxels(fold, O)
    ana = _tps_jacobian(fold, p[ok])
    got = det.reshape(-1)[ok]
    big = np.abs(ana) > 0.1
    assert (ana < 0).any() and (np.sign(got[big]) == np.sign(ana[big])).all()


# ---- 64-bit offsets, streams -----------------------------------------------------------------------------
def test_field_over_2_31_floats():
    import torch
    from sift3d_amd import hip
    S, O = (64, 64, 64), (700, 1024, 1000)                # field: 2.15e9 floats, 8.6 GB
    assert 3 * int(np.prod(O)) > 2 ** 31
    A = about_center(rot((1, -2, 0.5), 17.0) * (64 / 1000 * 1.1), S, O, (0.3, -0.6, 0.45))
    src = rand_vol(S, 44)
    field = dev_affine_field(A, O)
    out = dev_warp_field(src, field, "linear", -7.0)
    _, folded, mn, mx = hip.jacobian_det(field)
    n = int(np.prod(O))
    rng = np.random.default_rng(45)
    idx = np.concatenate([rng.integers(0, n, 20000), np.arange(n - 4096, n),
                          np.arange(2 ** 31 // 3 - 1024, 2 ** 31 // 3 + 1024)])
    idx_t = torch.from_numpy(idx).cuda()
    fv = [field[d].reshape(-1)[idx_t].cpu().numpy() for d in range(3)]
    got = out.reshape(-1)[idx_t].cpu().numpy()
    oz, oy, ox = O
    z, rem = np.divmod(idx, oy * ox)
    y, x = np.divmod(rem, ox)
    want_u = fr.ref_affine_field_points(A, x, y, z)
    for d in range(3):
        assert_bits(fv[d], want_u[d])
    flat = src.cpu().numpy().reshape(-1)
    want, ins = fr.ref_field_points(lambda k: flat[k], S, want_u, x, y, z, "linear", -7.0)
    assert_bits(got, want)
    assert 0.05 < ins.mean() < 0.95
    # the Jacobian at interior sampled voxels, from each voxel's 3 x 3 x 3 neighbourhood of the device field
    inner = (x > 0) & (x < ox - 1) & (y > 0) & (y < oy - 1) & (z > 0) & (z < oz - 1)
    det = torch.empty(O, dtype=torch.float32, device="cuda")
    hip.jacobian_det(field, det)
    sel = np.nonzero(inner)[0][::50]
    for k in sel:
        blk = field[:, z[k] - 1:z[k] + 2, y[k] - 1:y[k] + 2, x[k] - 1:x[k] + 2].cpu().numpy()
        assert bits(det[z[k], y[k], x[k]].item()) == bits(fr.ref_jacobian_det(blk)[1, 1, 1])
    want_det = float(np.linalg.det(A[:, :3]))
    print("64-bit: folded %d, det in [%.6g, %.6g] (det A %.6g)" % (folded, mn, mx, want_det))
    # u is rounded to float (|u| up to ~930 here: 6e-5 per value) against J entries of ~0.07: a few per cent
    assert folded == 0 and abs(mn - want_det) <= 0.05 * want_det and abs(mx - want_det) <= 0.05 * want_det


def test_non_default_stream():
    import torch
    from sift3d_amd import hip
    S, O = (33, 45, 61), (30, 40, 50)
    tps = random_tps(300, S, O, 8, disp=2.0)
    src = rand_vol((3,) + S, 11)
    field = dev_tps_field(tps, O)
    want = dev_warp_field(src, field).cpu()
    _, wf, wmn, wmx = hip.jacobian_det(field)
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
            f2 = torch.empty_like(field)
            hip.tps_field(f2, tps)
            dst = torch.full((3,) + O, -9.0, device="cuda")
            hip.warp_field(src2, dst, f2)
            _, folded, mn, mx = hip.jacobian_det(f2)
            got = dst.clone()
        hip.current_stream(refresh=True)
        torch.cuda.current_stream().wait_stream(s)
        assert torch.equal(got.cpu(), want)
        assert (folded, mn, mx) == (wf, wmn, wmx)
    finally:
        hip.current_stream(refresh=True)
    with pytest.raises(RuntimeError):                                       # dst overlaps src and the field
        hip.warp_field(field, field, field)


# ---- the public interface --------------------------------------------------------------------------------
def test_api_forms():
    import torch
    from sift3d_amd import api
    S, O = (21, 23, 25), (19, 22, 27)
    A = AFFINES["oblique"](S, O)
    tps = random_tps(30, S, O, 3, disp=1.5)
    fa = api.displacement_field(A, O)
    ft = api.displacement_field(tps, O)
    assert fa.shape == ft.shape == (3,) + O and fa.is_cuda
    assert_bits(fa.cpu().numpy(), fr.ref_affine_field(A, O))
    assert_bits(ft.cpu().numpy(), fr.ref_tps_field(tps, O))
    src = rand_vol(S, 4)
    s = src.cpu().numpy()
    dev = api.warp_field(src, ft, "linear", -2.0)
    assert isinstance(dev, torch.Tensor) and dev.shape == O
    host = api.warp_field(s, ft.cpu().numpy(), "linear", -2.0)
    assert_bits(host, dev.cpu().numpy())
    im = api.warp_field(api.Image.from_array(s), ft.cpu().numpy(), "nearest", -2.0)
    assert isinstance(im, api.Image) and im.shape == O
    assert_bits(im.data(), api.warp_field(src, ft, "nearest", -2.0).cpu().numpy())
    many = np.stack([s, 2 * s])
    assert_bits(api.warp_field(many, ft.cpu().numpy()), api.warp_field(torch.from_numpy(many).cuda(), ft).cpu())
    jd = api.jacobian_determinant(ft)
    jh = api.jacobian_determinant(ft.cpu().numpy())
    assert isinstance(jd, api.JacobianStats) and isinstance(jd.det, torch.Tensor)
    assert_bits(jd.det.cpu().numpy(), jh.det)
    assert (jd.folded, jd.min, jd.max) == (jh.folded, jh.min, jh.max)
    assert_bits(jh.det, fr.ref_jacobian_det(ft.cpu().numpy()))
    # composition of pull maps: w = v + warp_field(u, v) reads through v first, then u
    u = api.displacement_field(np.hstack([np.eye(3), np.array([[1.0], [2.0], [-3.0]])]), O)
    v = api.displacement_field(np.hstack([np.eye(3), np.array([[0.5], [-1.0], [0.25]])]), O)
    w = v + api.warp_field(u, v)
    inner = w[:, 4:-4, 4:-4, 4:-4]
    for d, t in enumerate((1.5, 1.0, -2.75)):
        assert (inner[d] == t).all()


# ---- end to end ----------------------------------------------------------------------------------------------
def test_register_deformable_field_end_to_end():
    import torch
    from sift3d_amd import api, hip
    n = 176
    fixed = torch.empty((n, n, n), device="cuda")
    hip.synth_lattice(fixed, 0, 21)
    known, _ = _known_deformation(n)
    moving = dev_tps(fixed, known, fixed.shape)
    torch.cuda.synchronize()
    res = api.register_deformable(moving, fixed)
    field = api.displacement_field(res.tps, fixed.shape)
    got = api.warp_field(moving, field).cpu().numpy()
    want = res.warped.cpu().numpy()
    fh = field.cpu().numpy()
    q = tr.ref_tps_coords(res.tps, *fr.grid(fixed.shape))
    keep = _away_from_the_edge(q, fixed.shape)
    bound = _rounding_bound(q, fh, moving.cpu().numpy())
    err = np.abs(got - want)[keep]
    st = api.jacobian_determinant(field)
    wdet = fr.ref_jacobian_det(fh)
    wf, wmn, wmx = fr.ref_stats(wdet)
    print("register_deformable field: max |warp_field - warped| %.3g (bound %.3g); Jacobian folded %d of %d, "
          "det in [%.4f, %.4f]" % (err.max(), bound, st.folded, wdet.size, st.min, st.max))
    assert err.max() <= bound
    assert_bits(st.det.cpu().numpy(), wdet)
    assert (st.folded, st.min, st.max) == (wf, wmn, wmx)
