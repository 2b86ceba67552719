"""GPU: cubic B-spline resampling (include/sift3d_amd.h, "Cubic B-spline resampling") against its numpy restatement
(tests/bspline_restatement.py), bit for bit: the prefilter and both gathers on small and odd shapes, 1, 3 and 12
channels, misaligned buffers, grids of different shapes, a volume of more than 2^31 voxels over its channels and a
512^3 prefilter on sampled lines; the affine against its own displacement field; the round-trip quality case; and
the linear / nearest warps, which must not have moved."""
import numpy as np
import pytest

from tests import bspline_restatement as br
from tests import field_restatement as fr
from tests.test_bspline_host import SHAPES, quality_maps, quality_volume, rms_centre, sample_bound
from tests.test_warp import about_center, ref_coords, ref_warp, rot

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, want):
    np.testing.assert_array_equal(bits(got), bits(want))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def misaligned(a):
    """a copy of `a` on the device that starts 4 bytes past a 16-byte boundary"""
    import torch
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.empty(a.size + 5, dtype=torch.float32, device="cuda")
    off = 1 + (-(buf.data_ptr() // 4) % 4)
    t = buf[off:off + a.size].view(a.shape)
    assert t.data_ptr() % 16 == 4
    t.copy_(torch.from_numpy(a))
    return t


def volume(shape, seed, scale=10.0):
    return np.random.default_rng(seed).normal(0, scale, shape).astype(np.float32)


# ---- prefilter ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES + [(6, 70, 130), (40, 33, 67), (70, 5, 64)])
def test_prefilter_is_the_restatement(shape):
    from sift3d_amd import hip
    v = volume(shape, sum(shape))
    same_bits(hip.bspline_prefilter(dev(v)).cpu().numpy(), br.prefilter(v))


@pytest.mark.parametrize("nc", [1, 3, 12])
def test_prefilter_channels_and_misaligned(nc):
    import torch
    from sift3d_amd import api, hip
    v = volume((nc, 9, 21, 35), nc)
    want = br.prefilter(v)
    same_bits(api.spline_coefficients(dev(v)).cpu().numpy(), want)
    src, dst = misaligned(v), misaligned(np.zeros_like(v))
    work = misaligned(np.zeros(v.shape[1:], np.float32))
    hip.bspline_prefilter(src, dst, work)
    same_bits(dst.cpu().numpy(), want)
    same_bits(api.spline_coefficients(v[0]), want[0])                         # the blocking host form
    same_bits(api.spline_coefficients(v), want)
    with pytest.raises(RuntimeError):
        hip.bspline_prefilter(src, src)                                          # not in place
    with pytest.raises(ValueError):
        hip.bspline_prefilter(src, torch.empty((2,) + tuple(src.shape), device="cuda"))


# ---- gathers -----------------------------------------------------------------------------------------------------
def maps(src_shape, out_shape):
    """pull maps that put samples inside, on the faces and outside: the identity, an integer shift, a flip, a
    rotation about a skew axis with a sub-voxel shift, and a zoom that covers the source's faces exactly"""
    n = np.array(src_shape[::-1], np.float64)
    o = np.array(out_shape[::-1], np.float64)
    zoom = np.zeros((3, 4))
    zoom[:, :3] = np.diag((n - 1) / np.maximum(o - 1, 1))
    flip = np.hstack([-np.eye(3), (n - 1)[:, None]])
    return [np.eye(3, 4), np.hstack([np.eye(3), [[1.0], [-2.0], [1.0]]]), flip, zoom,
            about_center(rot((1, 2, 3), 25.0), src_shape, out_shape, shift=(0.3, -0.45, 0.2)),
            about_center(1.7 * rot((0, 0, 1), -40.0), src_shape, out_shape)]


GATHER_SHAPES = [((1, 1, 1), (3, 2, 5)), ((1, 5, 1), (2, 7, 3)), ((2, 2, 2), (4, 4, 4)), ((3, 3, 3), (5, 6, 7)),
                 ((2, 3, 5), (3, 5, 9)), ((5, 7, 9), (5, 7, 9)), ((9, 20, 33), (11, 17, 70)),
                 ((19, 35, 41), (8, 40, 132))]


@pytest.mark.parametrize("src_shape,out_shape", GATHER_SHAPES)
def test_affine_gather_is_the_restatement(src_shape, out_shape):
    import torch
    from sift3d_amd import hip
    c = volume(src_shape, 5 * sum(src_shape))
    d_c, d_m = dev(c), misaligned(c)
    for A in maps(src_shape, out_shape):
        want = br.warp_affine(c, A, out_shape, fill=-3.0)
        out = torch.empty(out_shape, dtype=torch.float32, device="cuda")
        same_bits(hip.bspline_warp_affine(d_c, out, A, -3.0).cpu().numpy(), want)
        out2 = misaligned(np.zeros(out_shape, np.float32))
        same_bits(hip.bspline_warp_affine(d_m, out2, A, -3.0).cpu().numpy(), want)


def random_field(src_shape, out_shape, seed):
    """an affine's field plus noise, with NaNs and samples on and past the faces"""
    rng = np.random.default_rng(seed)
    A = about_center(rot((3, 1, 2), 15.0), src_shape, out_shape, shift=(0.25, 0.5, -0.3))
    f = fr.ref_affine_field(A, out_shape) + rng.normal(0, 0.7, (3,) + tuple(out_shape)).astype(np.float32)
    flat = f.reshape(3, -1)
    n = flat.shape[1]
    x, y, z = (g.reshape(-1) for g in fr.grid(out_shape))
    k = rng.permutation(n)[:max(12, n // 10)]
    for i, j in enumerate(k):                                                    # exactly onto a face / a NaN
        d = i % 3
        p = (x, y, z)[d][j]
        hi = src_shape[::-1][d] - 1
        flat[d, j] = [0 - p, hi - p, np.nan, hi - p + 0.25][(i // 3) % 4]
    return f.astype(np.float32)


@pytest.mark.parametrize("nc", [1, 3, 12])
@pytest.mark.parametrize("src_shape,out_shape", GATHER_SHAPES)
def test_field_gather_is_the_restatement(src_shape, out_shape, nc):
    import torch
    from sift3d_amd import hip
    c = volume((nc,) + tuple(src_shape), nc + sum(src_shape))
    f = random_field(src_shape, out_shape, 7 * nc + sum(out_shape))
    want = br.warp_field(c, f, fill=2.5)
    out = torch.empty((nc,) + tuple(out_shape), dtype=torch.float32, device="cuda")
    same_bits(hip.bspline_warp_field(dev(c), out, dev(f), 2.5).cpu().numpy(), want)
    if nc == 1:
        out1 = misaligned(np.zeros(out_shape, np.float32))
        same_bits(hip.bspline_warp_field(misaligned(c[0]), out1, misaligned(f), 2.5).cpu().numpy(), want[0])


def test_more_than_2_31_voxels_and_512_cubed_lines():
    """17 channels of 512^3 are 2^31 + 2^27 voxels: the last channel's coefficients on sampled lines (the 512^3
    spot check), and a gather from it, against the restatement"""
    import torch
    from sift3d_amd import hip
    nc, n = 17, 512
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    src = torch.empty((nc, n, n, n), dtype=torch.float32, device="cuda")
    for k in range(nc):
        src[k].normal_(0, 10, generator=g)
    assert src.numel() > 2 ** 31
    coef = hip.bspline_prefilter(src)
    rng = np.random.default_rng(4)
    for k in (0, nc - 1):
        v = src[k].cpu().numpy()
        c = coef[k].cpu().numpy()
        lines = [(0, (0, 0, 0)), (1, (0, 0, 511)), (2, (511, 511, 0)), (2, (0, 300, 0)), (0, (0, 255, 256))]
        lines += [(int(rng.integers(3)), tuple(int(t) for t in rng.integers(0, n, 3))) for _ in range(8)]
        for axis, fixed in lines:
            idx = list(fixed)
            idx[axis] = slice(None)
            same_bits(c[tuple(idx)], br.prefilter_line(v, axis, fixed))
    del src
    # a small output grid whose field scatters the samples over the whole volume
    O = (6, 10, 70)
    f = rng.uniform(0, n - 1, (3,) + O).astype(np.float32) - np.stack(fr.grid(O)).astype(np.float32)
    out = torch.empty((nc,) + O, dtype=torch.float32, device="cuda")
    hip.bspline_warp_field(coef, out, dev(f), 0.0)
    q = br.field_coords(f, *fr.grid(O))
    for k in (0, nc - 1):
        flat = coef[k].reshape(-1)
        want, ins = br.sample_points(lambda i: flat[torch.from_numpy(i).cuda()].cpu().numpy(), (n, n, n), q, 0.0)
        assert ins.mean() > 0.9
        same_bits(out[k].cpu().numpy(), want)


# ---- api -----------------------------------------------------------------------------------------------------------
def test_resample_cubic_dispatch():
    from sift3d_amd import api
    v = volume((19, 35, 41), 9)
    O = (17, 30, 44)
    A = about_center(rot((1, 2, 3), 12.0), v.shape, O, shift=(0.3, 0.1, -0.2))
    c = br.prefilter(v)
    want = br.warp_affine(c, A, O, fill=1.0)
    d_v = dev(v)
    same_bits(api.resample_cubic(d_v, A, O, fill=1.0).cpu().numpy(), want)
    coef = api.spline_coefficients(d_v)
    same_bits(api.resample_cubic(coef, A, O, fill=1.0, prefiltered=True).cpu().numpy(), want)
    same_bits(api.resample_cubic(v, A, O, fill=1.0), want)                       # the blocking host forms
    im = api.resample_cubic(api.Image.from_array(v), A, O, fill=1.0)
    same_bits(im.data(), want)
    f = fr.ref_affine_field(A, O)
    want_f = br.warp_field(c, f, fill=1.0)
    same_bits(api.resample_cubic(d_v, dev(f), fill=1.0).cpu().numpy(), want_f)
    same_bits(api.resample_cubic(v, f, fill=1.0), want_f)
    # a TPS goes through its displacement field; 12 channels share one set of taps
    t = api.TPS(np.array([[3.0, 4, 5], [30, 8, 2], [12, 25, 15], [20, 20, 3], [35, 30, 16]]),
                np.random.default_rng(1).normal(0, 0.02, (5, 3)), A)
    u = api.displacement_field(t, O)
    many = volume((12,) + v.shape, 10)
    got = api.resample_cubic(dev(many), t, O)
    same_bits(got.cpu().numpy(), br.warp_field(br.prefilter(many), u.cpu().numpy()))
    with pytest.raises(ValueError):
        api.resample_cubic(dev(many), A, O)
    with pytest.raises(ValueError):
        api.resample_cubic(d_v, f)                                               # a host field with a CUDA volume


def test_affine_equals_its_field():
    """resample_cubic through A against resample_cubic through displacement_field(A).  The field holds
    u = (float)(q - p), off by at most half an ulp of |u| < 64 (spacing 2^-18): delta = 2^-19 per axis.  The interpolant's slope
    per axis is at most max|c[k] - c[k-1]| <= 2 cmax, so the two values differ by at most 3 * 2 cmax * delta, plus the
    float rounding of each evaluation (sample_bound): the weights change continuously across a voxel boundary, so a
    sample whose floor differs between the two is covered by the same slope."""
    from sift3d_amd import api
    v = volume((60, 62, 64), 12)
    O = (30, 30, 30)
    A = about_center(rot((2, 1, 3), 20.0), v.shape, O, shift=(0.3, 0.2, 0.1))
    coef = api.spline_coefficients(dev(v))
    q = ref_coords(A, *fr.grid(O))
    for t, n in zip(q, v.shape[::-1]):
        assert ((t >= 1e-3) & (t <= n - 1 - 1e-3)).all()                         # strictly inside: no fill flips
    u = api.displacement_field(A, O)
    assert float(u.abs().max()) < 64
    a = api.resample_cubic(coef, A, O, prefiltered=True).cpu().numpy().astype(np.float64)
    b = api.resample_cubic(coef, u, prefiltered=True).cpu().numpy().astype(np.float64)
    cmax = float(coef.abs().max())
    tol = 3 * 2 * cmax * 2.0 ** -19 + 2 * sample_bound(cmax)
    err = np.abs(a - b).max()
    print("affine vs field: err %.3g tol %.3g" % (err, tol))
    assert err <= tol


def test_round_trip_quality_on_the_device():
    from sift3d_amd import api, hip
    import torch
    v = quality_volume()
    A, B = quality_maps()
    lin = cub = dev(v)
    for _ in range(4):
        for T in (A, B):
            lin = hip.warp_affine(lin, torch.empty_like(lin), T, "linear", 0.0)
            cub = api.resample_cubic(cub, T, v.shape, 0.0)
    r_lin, r_cub = rms_centre(lin.cpu().numpy(), v), rms_centre(cub.cpu().numpy(), v)
    print("round trip rms on the device: linear %.4f cubic %.4f ratio %.1f" % (r_lin, r_cub, r_lin / r_cub))
    assert r_cub <= r_lin / 10


def test_linear_and_nearest_warps_did_not_move():
    from sift3d_amd import api
    v = volume((3, 19, 35, 41), 13)
    O = (17, 30, 44)
    A = about_center(rot((1, 2, 3), 12.0), v.shape[1:], O, shift=(0.3, 0.1, -0.2))
    f = random_field(v.shape[1:], O, 14)
    for interp in ("linear", "nearest"):
        same_bits(api.warp_affine(v[0], A, O, interp, -1.0), ref_warp(v[0], A, O, interp, -1.0)[0])
        same_bits(api.warp_field(dev(v), dev(f), interp, -1.0).cpu().numpy(), fr.ref_warp_field(v, f, interp, -1.0))
        same_bits(api.warp_field(v[1], f, interp, -1.0), fr.ref_warp_field(v[1], f, interp, -1.0))
