"""Affine resampling on the device (sift3d_hip_warp_affine) and registration end to end.

The kernel's arithmetic is fixed (include/sift3d_amd.h, "Resampling"), so the numpy restatement
below, which follows the same steps in IEEE float64 / float32 without contraction, must match it
bit for bit; a float64 trilinear reference bounds the float32 interpolation error."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# ---- numpy restatement of the contract ----------------------------------------------------------
def ref_coords(A, x, y, z):
    """q_d = A[d][0] x + ((A[d][1] y + A[d][2] z) + A[d][3]) in float64, for integer arrays x, y, z
    (broadcast together)."""
    A = np.asarray(A, np.float64).reshape(3, 4)
    x, y, z = (np.asarray(v).astype(np.float64) for v in (x, y, z))
    return [A[d, 0] * x + ((A[d, 1] * y + A[d, 2] * z) + A[d, 3]) for d in range(3)]


def ref_inside(q, shape):
    nz, ny, nx = shape
    qx, qy, qz = q
    return (qx >= 0) & (qx <= nx - 1) & (qy >= 0) & (qy <= ny - 1) & (qz >= 0) & (qz <= nz - 1)


def ref_warp_points(gather, shape, A, x, y, z, interp="linear", fill=0.0, f64=False):
    """The restatement at output voxels (x, y, z).  gather(flat int64 indices) -> float32 values
    of the source (shape [nz, ny, nx]).  f64=True: the float64 trilinear reference instead."""
    nz, ny, nx = shape
    q = ref_coords(A, x, y, z)
    ins = ref_inside(q, shape)
    q = [np.where(ins, v, 0.0) for v in q]

    def flat(ix, iy, iz):
        return (iz.astype(np.int64) * ny + iy) * nx + ix

    if interp == "nearest":
        i = [np.floor(v + 0.5).astype(np.int64) for v in q]
        val = gather(flat(*i)).astype(np.float32)
    else:
        i = [np.floor(v) for v in q]
        ft = np.float64 if f64 else np.float32
        f = [(v - iv).astype(ft) for v, iv in zip(q, i)]
        i = [iv.astype(np.int64) for iv in i]
        j = [np.minimum(iv + 1, n - 1) for iv, n in zip(i, (nx, ny, nz))]

        def g(ix, iy, iz):
            return gather(flat(ix, iy, iz)).astype(ft)

        def lerp(a, b, t):
            return a + t * (b - a)

        c00 = lerp(g(i[0], i[1], i[2]), g(j[0], i[1], i[2]), f[0])
        c10 = lerp(g(i[0], j[1], i[2]), g(j[0], j[1], i[2]), f[0])
        c01 = lerp(g(i[0], i[1], j[2]), g(j[0], i[1], j[2]), f[0])
        c11 = lerp(g(i[0], j[1], j[2]), g(j[0], j[1], j[2]), f[0])
        val = lerp(lerp(c00, c10, f[1]), lerp(c01, c11, f[1]), f[2])
    return np.where(ins, val, val.dtype.type(fill)), ins


def ref_warp(src, A, out_shape, interp="linear", fill=0.0, f64=False):
    oz, oy, ox = out_shape
    z, y, x = np.meshgrid(np.arange(oz), np.arange(oy), np.arange(ox), indexing="ij")
    flat = np.ascontiguousarray(src).reshape(-1)
    return ref_warp_points(lambda k: flat[k], src.shape, A, x, y, z, interp, fill, f64)


# ---- helpers --------------------------------------------------------------------------------------
def dev_warp(src, A, out_shape, interp="linear", fill=0.0):
    import torch
    from sift3d_amd import hip
    dst = torch.empty(out_shape, dtype=torch.float32, device=src.device)
    hip.warp_affine(src, dst, A, interp, fill)
    return dst


def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def about_center(M, src_shape, out_shape, shift=(0.0, 0.0, 0.0)):
    """pull map q = M (p - co) + cs + shift: output centre -> source centre (+ shift), xyz order."""
    cs = (np.array(src_shape[::-1], np.float64) - 1) / 2
    co = (np.array(out_shape[::-1], np.float64) - 1) / 2
    A = np.zeros((3, 4))
    A[:, :3] = M
    A[:, 3] = cs + np.asarray(shift) - M @ co
    return A


def rand_vol(shape, seed):
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randn(shape, generator=g, device="cuda", dtype=torch.float32)


# ---- 1-3: exact copies --------------------------------------------------------------------------
def test_identity_is_exact_copy():
    import torch
    src = rand_vol((41, 50, 70), 1)
    ident = np.hstack([np.eye(3), np.zeros((3, 1))])
    for interp in ("linear", "nearest"):
        out = dev_warp(src, ident, src.shape, interp)
        torch.cuda.synchronize()
        assert torch.equal(out, src), interp


@pytest.mark.parametrize("fill", [0.0, -1.5])
def test_integer_translation_into_other_shape(fill):
    src = rand_vol((41, 50, 70), 2)
    s = src.cpu().numpy()
    t = (3, -2, 5)                                    # source = output + t (x, y, z)
    A = np.hstack([np.eye(3), np.array(t, np.float64)[:, None]])
    oz, oy, ox = 40, 48, 64
    want = np.full((oz, oy, ox), fill, np.float32)
    # output z in [0, 35] reads source z + 5 in [5, 40]; output y >= 2 reads y - 2
    want[:36, 2:, :] = s[5:41, 0:46, 3:67]
    for interp in ("linear", "nearest"):
        out = dev_warp(src, A, (oz, oy, ox), interp, fill).cpu().numpy()
        np.testing.assert_array_equal(out, want)


def _perm_flip(src_shape, sa, fl):
    """pull map and output shape of: output xyz axis k <- source axis sa[k], flipped where fl[k]"""
    n = src_shape[::-1]                                # (nx, ny, nz)
    A = np.zeros((3, 4))
    for k in range(3):
        A[sa[k], k] = -1.0 if fl[k] else 1.0
        if fl[k]:
            A[sa[k], 3] = n[sa[k]] - 1
    out_xyz = [n[sa[k]] for k in range(3)]
    return A, tuple(out_xyz[::-1])


@pytest.mark.parametrize("sa,fl", [
    ((1, 0, 2), (1, 0, 0)),          # 90 degrees about z
    ((1, 0, 2), (0, 1, 0)),          # -90 degrees about z
    ((0, 2, 1), (0, 1, 0)),          # 90 degrees about x
    ((2, 1, 0), (0, 0, 1)),          # 90 degrees about y
    ((0, 1, 2), (1, 0, 0)),          # flips
    ((0, 1, 2), (0, 1, 0)),
    ((0, 1, 2), (0, 0, 1)),
    ((0, 1, 2), (1, 1, 1)),
    ((2, 0, 1), (0, 1, 1)),          # a 3-cycle with flips
])
def test_axis_permutations_and_flips_equal_torch(sa, fl):
    import torch
    src = rand_vol((41, 50, 70), 3)
    A, oshape = _perm_flip(src.shape, sa, fl)
    # torch: array dim i is xyz axis 2 - i
    want = src.permute([2 - sa[2 - i] for i in range(3)])
    flips = [i for i in range(3) if fl[2 - i]]
    if flips:
        want = want.flip(flips)
    assert tuple(want.shape) == oshape
    for interp in ("linear", "nearest"):
        out = dev_warp(src, A, oshape, interp)
        torch.cuda.synchronize()
        assert torch.equal(out, want), (sa, fl, interp)


# ---- 4: general maps against the restatement --------------------------------------------------
def _general_maps():
    rng = np.random.default_rng(2024)
    S = (37, 29, 43)                                   # source [nz, ny, nx]
    maps = []
    for k in range(8):
        O = tuple(int(v) for v in rng.integers(23, 48, 3) | 1) if k != 3 else (19, 15, 21)
        if k == 0:
            M = rot(rng.standard_normal(3), 33.0)
        elif k == 1:
            M = rot(rng.standard_normal(3), -71.0)
        elif k == 2:
            M = 0.5 * rot(rng.standard_normal(3), 17.0)        # output magnified 2x
        elif k == 3:
            M = 2.0 * np.eye(3)                                # output halves the source
        elif k == 4:
            M = np.array([[1.0, 0.3, -0.2], [0.0, 1.0, 0.45], [0.1, 0.0, 1.0]])   # shear
        elif k == 5:
            M = rot((1, 1, 0), 45.0) @ np.diag([1.3, 0.7, 1.1])
        else:
            M = rot(rng.standard_normal(3), float(rng.uniform(-90, 90)))
        shift = rng.uniform(-1.5, 1.5, 3)
        if k >= 6:                                             # about half the output outside
            shift = shift + 0.5 * np.array(S[::-1]) * np.sign(rng.standard_normal(3)) * np.array([1, 0, 0])
        maps.append((S, O, about_center(M, S, O, shift)))
    return maps


@pytest.mark.parametrize("k", range(8))
def test_general_maps_bit_exact_against_restatement(k):
    S, O, A = _general_maps()[k]
    src = rand_vol(S, 40 + k)
    s = src.cpu().numpy()
    amax = float(np.abs(s).max())
    fill = 1000.0                                      # never an interpolated value of this source
    for interp in ("linear", "nearest"):
        out = dev_warp(src, A, O, interp, fill).cpu().numpy()
        want, ins = ref_warp(s, A, O, interp, fill)
        np.testing.assert_array_equal(out, want)
        np.testing.assert_array_equal(out == np.float32(fill), ~ins)
        if interp == "linear":
            ref64, _ = ref_warp(s, A, O, interp, fill, f64=True)
            assert np.abs(out.astype(np.float64) - ref64).max() <= 1e-5 * amax
    if k >= 6:
        assert 0.2 < ins.mean() < 0.8


def test_degenerate_axes_against_restatement():
    """a source one voxel wide in x (the linear kernel without x pairs) and one voxel high in y"""
    for S in ((5, 7, 1), (6, 1, 9)):
        src = rand_vol(S, 50 + S[2])
        s = src.cpu().numpy()
        O = (9, 11, 13)
        A = about_center(rot((1, 2, 2), 25.0), S, O, (0.1, -0.2, 0.3))
        A[2 - S.index(1)] = 0.0                  # the singleton axis: q = 0 exactly, the only inside value
        for interp in ("linear", "nearest"):
            out = dev_warp(src, A, O, interp, 7.0).cpu().numpy()
            want, ins = ref_warp(s, A, O, interp, 7.0)
            np.testing.assert_array_equal(out, want)
            assert ins.any() and not ins.all()


# ---- 5-6: large volumes ---------------------------------------------------------------------------
def _check_sampled(src, out, A, interp, planes, npts, seed):
    """bit-exact on whole z-planes and on random voxels, source values gathered on the device"""
    import torch
    flat = src.reshape(-1)

    def gather(k):
        idx = torch.from_numpy(np.ascontiguousarray(k.reshape(-1))).to(src.device)
        return flat[idx].cpu().numpy().reshape(k.shape)

    oz, oy, ox = out.shape
    rng = np.random.default_rng(seed)
    z = np.array(planes)[:, None, None]
    y = np.arange(oy)[None, :, None]
    x = np.arange(ox)[None, None, :]
    want, _ = ref_warp_points(gather, src.shape, A, x, y, z, interp)
    np.testing.assert_array_equal(out[planes].cpu().numpy(), want)
    pz, py, px = rng.integers(0, oz, npts), rng.integers(0, oy, npts), rng.integers(0, ox, npts)
    want, ins = ref_warp_points(gather, src.shape, A, px, py, pz, interp)
    got = out[torch.from_numpy(pz).cuda(), torch.from_numpy(py).cuda(), torch.from_numpy(px).cuda()]
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    return ins


def test_512_oblique_rotation_sampled_bit_exact():
    n = 512
    src = rand_vol((n, n, n), 7)
    A = about_center(rot((1.0, -2.0, 0.7), 27.0), src.shape, src.shape, (0.37, -1.2, 2.6))
    for interp in ("linear", "nearest"):
        out = dev_warp(src, A, src.shape, interp)
        ins = _check_sampled(src, out, A, interp, [0, 1, 100, 255, 256, 400, 510, 511], 100000, 8)
        assert ins.mean() > 0.5


def test_volume_over_2gib_uses_64bit_offsets():
    import torch
    shape = (640, 1024, 1024)                         # 2.68 GB of float32
    src = rand_vol(shape, 9)
    assert src.numel() * 4 > 2 ** 31
    # a small rotation about z plus a shift: the last planes read the top of the source
    A = about_center(rot((0, 0, 1), 3.0), shape, shape, (0.25, -0.5, 0.0))
    for interp in ("linear", "nearest"):
        out = dev_warp(src, A, shape, interp)
        ins = _check_sampled(src, out, A, interp, [0, 320, 600, 638, 639], 100000, 10)
        assert ins.mean() > 0.8
        del out
    del src
    torch.cuda.empty_cache()


# ---- 7: streams and overlap -----------------------------------------------------------------------
def test_non_default_stream_and_overlap_refused():
    import torch
    from sift3d_amd import hip
    S = (33, 45, 61)
    A = about_center(rot((0.3, 1, 0.2), 40.0), S, S, (0.5, 0.25, -0.75))
    src = rand_vol(S, 11)
    want = dev_warp(src, A, S).cpu()
    # The warp's input is produced on stream s behind several milliseconds of other work.  A warp that ran on
    # any other stream would start long before that copy and read the zeros.
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
            hip.warp_affine(src2, dst, A)
            got = dst.clone()                                    # ordered after the warp by the stream
        hip.current_stream(refresh=True)
        torch.cuda.current_stream().wait_stream(s)
        assert torch.equal(got.cpu(), want)
    finally:
        hip.current_stream(refresh=True)
    buf = torch.zeros(2 * src.numel(), device="cuda")
    N = src.numel()
    with pytest.raises(RuntimeError):
        hip.warp_affine(src, src, A)
    with pytest.raises(RuntimeError):
        hip.warp_affine(buf[:N].view(S), buf[N // 2:N // 2 + N].view(S), A)
    hip.warp_affine(buf[:N].view(S), buf[N:].view(S), A)          # adjacent, not overlapping: accepted


# ---- 8: host images -------------------------------------------------------------------------------
def test_host_image_path_equals_device_path():
    from sift3d_amd import api
    S, O = (29, 35, 47), (31, 33, 45)
    A = about_center(rot((2, -1, 1), 22.0), S, O, (1.3, -0.4, 0.9))
    src = rand_vol(S, 12)
    s = src.cpu().numpy()
    for interp in ("linear", "nearest"):
        dev = dev_warp(src, A, O, interp, -2.0).cpu().numpy()
        arr = api.warp_affine(s, A, O, interp, -2.0)
        np.testing.assert_array_equal(arr, dev)
        im = api.warp_affine(api.Image.from_array(s), A, O, interp, -2.0)
        assert isinstance(im, api.Image) and im.shape == O
        np.testing.assert_array_equal(im.data(), dev)
    with pytest.raises(RuntimeError):
        api.warp_affine(api.Image(47, 35, 29, 2), A, O)


# ---- 9: registration with a general transform -----------------------------------------------------
def test_register_recovers_general_affine_and_resamples():
    import torch
    from sift3d_amd import api, hip
    n = 160
    R = rot((1, 2, 3), 20.0)
    tb = np.array([0.37, -0.61, 0.45])                 # non-integer part of the translation
    half = (n - 1) / 2.0
    reach = np.abs(R).sum(1) * half                    # half-extent of the rotated cube per axis
    pad = int(np.ceil((reach - half).max() + np.abs(tb).max())) + 2
    o = np.array([pad, pad + 1, pad + 2], np.float64)  # crop offset of `fixed` in `big` (x, y, z)
    dims = n + 2 * pad + 3
    big = torch.empty((dims, dims, dims), device="cuda")
    hip.synth_lattice(big, 0, 21)
    ox_, oy_, oz_ = (int(v) for v in o)
    fixed = big[oz_:oz_ + n, oy_:oy_ + n, ox_:ox_ + n].contiguous()
    # moving[p] = big[B p]: B rotates about the centre of the fixed crop and shifts by tb
    B = np.zeros((3, 4))
    B[:, :3] = R
    B[:, 3] = o + half + tb - R @ np.full(3, half)
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    assert ref_inside(ref_coords(B, x, y, z), big.shape).all()    # no fill edge in `moving`
    moving = dev_warp(big, B, (n, n, n))
    torch.cuda.synchronize()
    res = api.register(moving, fixed)
    true_A = B.copy()
    true_A[:, 3] -= o                                  # moving voxel p -> fixed voxel B p - o
    dlin = np.abs(res.A[:, :3] - true_A[:, :3]).max()
    dt = np.abs(res.A[:, 3] - true_A[:, 3]).max()
    print("register: %d matches, %.3f inliers, linear %.2e, translation %.3f voxel"
          % (res.num_matches, res.inliers.mean(), dlin, dt))
    assert res.num_matches >= 20 and res.inliers.mean() > 0.5
    assert dlin <= 0.01 and dt <= 0.75
    assert tuple(res.warped.shape) == tuple(fixed.shape)
    # the resampled volume against moving resampled by the true inverse, over their common inside
    Ai_est, Ai_true = api.affine_invert(res.A), api.affine_invert(true_A)
    mask = ref_inside(ref_coords(Ai_est, x, y, z), moving.shape) & ref_inside(ref_coords(Ai_true, x, y, z),
                                                                            moving.shape)
    assert mask.mean() > 0.5
    want = dev_warp(moving, Ai_true, fixed.shape).cpu().numpy()[mask].astype(np.float64)
    got = res.warped.cpu().numpy()[mask].astype(np.float64)
    a, b = got - got.mean(), want - want.mean()
    ncc = float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))
    print("register: NCC %.4f over %.2f of the grid" % (ncc, mask.mean()))
    assert ncc >= 0.99
