"""GPU: the dense demons refinement (sift3d_hip_demons_force, sift3d_amd_demons_device, api.refine_field,
api.register_dense) against the numpy restatement of the contract in include/sift3d_amd.h
(tests/demons_restatement.py): the force and the field bit for bit, the inside count exactly, the sum within the
bound of any summation order; then end to end against the spline it refines."""
import numpy as np
import pytest

from tests import demons_restatement as dm
from tests.test_warp import rot

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    from sift3d_amd import hip as h
    h.lib()
    assert torch.cuda.is_available()
    h.current_stream(refresh=True)
    return h


def _bits(got, want, what):
    got = np.ascontiguousarray(got, np.float32)
    want = np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    if bad.any():
        i = tuple(int(a[0]) for a in np.nonzero(bad))
        raise AssertionError("%s: %d of %d values differ, first at %s: %r != %r"
                             % (what, int(bad.sum()), bad.size, i, got[i], want[i]))


def _check_stats(s, c, sd, ins, what):
    want_s, want_c = dm.ref_stats(sd, ins)
    assert c == want_c, (what, c, want_c)
    assert abs(s - want_s) <= dm.gamma(want_c) * want_s, (what, s, want_s)


# (fixed (nx, ny, nz), moving (mx, my, mz)): odd sizes, and axes of 1 and 2 voxels
SHAPES = [((37, 29, 23), (31, 41, 19)), ((37, 2, 23), (31, 41, 19)), ((1, 29, 2), (31, 41, 19))]


def _case(shape, mshape, nc, seed):
    """F, M, a W near F, and a field that samples outside the moving grid at some voxels"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    mx, my, mz = mshape
    F = rng.normal(0, 1, (nc, nz, ny, nx)).astype(np.float32)
    M = rng.normal(0, 1, (nc, mz, my, mx)).astype(np.float32)
    W = (F + rng.normal(0, 0.5, F.shape)).astype(np.float32)
    u = rng.normal(0, 1.5, (3, nz, ny, nx)).astype(np.float32)
    u[0] += np.float32(2.0)
    u[1] += np.float32(3.0)
    return F, M, W, u


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("nc", [1, 3, 12])
@pytest.mark.parametrize("shape,mshape", SHAPES)
def test_force_bit_exact_against_restatement(hip, shape, mshape, nc):
    import torch
    F, _, W, u = _case(shape, mshape, nc, 10 * nc + shape[1])
    mx, my, mz = mshape
    step = torch.full((3,) + F.shape[1:], float("nan"), device="cuda")
    for alpha in (1.0, 0.3):
        stats = hip.demons_force(_t(F), _t(W), _t(u), step, alpha, (mz, my, mx))
        s, c = hip.demons_stats(stats)
        want, sd, ins = dm.ref_force(F, W, u, (mz, my, mx), alpha)
        assert 0 < ins.sum() < ins.size                    # samples inside and outside
        _bits(step.cpu().numpy(), want, "force %s / %s nc %d alpha %g" % (shape, mshape, nc, alpha))
        _check_stats(float(s[0]), int(c[0]), sd, ins, "force stats")
        print("force %s nc %d alpha %g: sum %.17g ref %.17g count %d"
              % (shape, nc, alpha, s[0], dm.ref_stats(sd, ins)[0], c[0]))


SIGMAS = [(0.0, 0.0), (1.5, 0.0), (0.0, 2.0), (1.5, 2.0), (1.5, 11.0)]    # 11.0: 67 taps, the chunked FIR


@pytest.mark.parametrize("sigmas", SIGMAS)
@pytest.mark.parametrize("nc", [1, 3, 12])
@pytest.mark.parametrize("shape,mshape", SHAPES)
def test_driver_bit_exact_against_restatement(hip, oracle_mod, shape, mshape, nc, sigmas):
    F, M, _, u = _case(shape, mshape, nc, 7 + nc + shape[1])
    sf, sdf = sigmas
    field = _t(u)
    stats = hip.demons(_t(F), _t(M), field, 3, 0.8, sf, sdf)
    s, c = hip.demons_stats(stats)
    want, per = dm.ref_demons(F, M, u, 3, 0.8, sf, sdf, oracle_mod)
    _bits(field.cpu().numpy(), want, "demons %s nc %d sigmas %s" % (shape, nc, sigmas))
    assert len(s) == 3
    for k, (sd, ins) in enumerate(per):
        _check_stats(float(s[k]), int(c[k]), sd, ins, "iteration %d" % k)
    assert not np.array_equal(want, u)


def test_zero_iterations_leave_the_field(hip):
    import torch
    F, M, _, u = _case((9, 8, 7), (6, 7, 8), 2, 1)
    field = _t(u)
    stats = hip.demons(_t(F), _t(M), field, 0, 1.0, 1.0, 1.0)
    torch.cuda.synchronize()
    assert stats.numel() == 0
    _bits(field.cpu().numpy(), u, "iterations 0")


def test_non_default_stream_and_repeat_calls(hip):
    import torch
    shape, mshape = SHAPES[0]
    F, M, _, u = _case(shape, mshape, 12, 5)
    dF, dM = _t(F), _t(M)
    runs = []
    for _ in range(2):
        field = _t(u)
        st = hip.demons(dF, dM, field, 4, 1.0, 1.5, 2.0)
        runs.append((field.cpu().numpy(), st.cpu().numpy()))
    np.testing.assert_array_equal(runs[0][0].view(np.uint32), runs[1][0].view(np.uint32))
    np.testing.assert_array_equal(runs[0][1], runs[1][1])              # sums and counts, bit for bit
    # the same call on another stream, its inputs produced there behind other work
    big = torch.ones((256, 512, 512), device="cuda")
    dF2, dM2 = torch.zeros_like(dF), torch.zeros_like(dM)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    try:
        with torch.cuda.stream(s):
            hip.current_stream(refresh=True)
            for _ in range(20):
                big.mul_(1.0001)
            dF2.copy_(dF)
            dM2.copy_(dM)
            field = _t(u)
            st = hip.demons(dF2, dM2, field, 4, 1.0, 1.5, 2.0)
            got_f, got_s = field.clone(), st.clone()
        hip.current_stream(refresh=True)
        torch.cuda.current_stream().wait_stream(s)
        np.testing.assert_array_equal(got_f.cpu().numpy().view(np.uint32), runs[0][0].view(np.uint32))
        np.testing.assert_array_equal(got_s.cpu().numpy(), runs[0][1])
    finally:
        hip.current_stream(refresh=True)


def test_over_2_31_elements_sampled(hip):
    """nc * n > 2^31: the force on blocks of rows (full x extent) near the 2^31st element of the last channel and
    at the grid's end, against the restatement of the blocks with one voxel of margin"""
    import torch
    nx, ny, nz, nc = 1024, 1024, 176, 12
    n = nx * ny * nz
    assert nc * n > 2 ** 31
    z_cross = (2 ** 31 - (nc - 1) * n) // (nx * ny)
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    F = torch.rand((nc, nz, ny, nx), device="cuda", generator=g)
    W = torch.rand((nc, nz, ny, nx), device="cuda", generator=g)
    u = (torch.rand((3, nz, ny, nx), device="cuda", generator=g) - 0.5) * 4.0
    step = torch.empty_like(u)
    stats = hip.demons_force(F, W, u, step, 1.0, (nz, ny, nx))
    s, c = hip.demons_stats(stats)
    blocks = [(z_cross - 2, z_cross + 2, 0, 3), (z_cross - 1, z_cross + 3, ny - 3, ny), (nz - 3, nz, ny - 4, ny),
              (nz - 2, nz, 500, 503)]
    for z0, z1, y0, y1 in blocks:
        a, b = max(z0 - 1, 0), min(z1 + 1, nz)
        cy, dy = max(y0 - 1, 0), min(y1 + 1, ny)
        Fb = F[:, a:b, cy:dy, :].cpu().numpy()
        Wb = W[:, a:b, cy:dy, :].cpu().numpy()
        ub = u[:, a:b, cy:dy, :].cpu().numpy()
        want, _, ins = dm.ref_force(Fb, Wb, ub, (nz, ny, nx), 1.0, origin=(0, cy, a))
        got = step[:, z0:z1, y0:y1, :].cpu().numpy()
        _bits(got, want[:, z0 - a:z1 - a, y0 - cy:y1 - cy, :], "block z %d..%d y %d..%d" % (z0, z1, y0, y1))
        assert ins[z0 - a:z1 - a, y0 - cy:y1 - cy].any()
    # the count of the whole grid: the inside test alone, on the device in torch
    zz, yy, xx = (torch.arange(k, device="cuda", dtype=torch.float64) for k in (nz, ny, nx))
    ok = torch.ones((nz, ny, nx), dtype=torch.bool, device="cuda")
    for d, (p, m) in enumerate(((xx[None, None, :], nx), (yy[None, :, None], ny), (zz[:, None, None], nz))):
        q = p + u[d].double()
        ok &= (q >= 0) & (q <= m - 1)
    assert int(c[0]) == int(ok.sum())
    # the sum: s_d per voxel in float64 on the device (float differences, channels in order), summed by numpy
    sd = torch.zeros((nz, ny, nx), dtype=torch.float64, device="cuda")
    for ch in range(nc):
        d = (F[ch] - W[ch]).double()
        sd = sd + d * d
    del F, W
    want = np.sum(sd[ok].cpu().numpy(), dtype=np.float64)
    print("over 2^31: sum %.17g ref %.17g count %d" % (s[0], want, c[0]))
    assert abs(float(s[0]) - want) <= dm.gamma(int(c[0])) * want


def test_identity_stays_zero(hip):
    """moving == fixed, zero field: the field stays bit-exactly zero through 10 iterations and every sum is 0"""
    import torch
    from sift3d_amd import api
    vol = torch.from_numpy(api.synth_survey(40)).cuda()
    for feats in ("descriptors", "intensity"):
        r = api.refine_field(vol, vol, iterations=10, features=feats)
        assert not r.field.cpu().numpy().view(np.uint32).any(), feats
        assert len(r.msd) == 10 and np.all(r.msd == 0.0), (feats, r.msd)
        assert torch.equal(r.warped, vol)
        assert r.jacobian.folded == 0 and r.jacobian.min == r.jacobian.max == 1.0


# ---- end to end: tests/test_tps.py's case ---------------------------------------------------------------------
def dev_tps(src, tps, out_shape, interp="linear", fill=0.0):
    import torch
    from sift3d_amd import hip
    dst = torch.empty(out_shape, dtype=torch.float32, device=src.device)
    hip.warp_tps(src, dst, tps, interp, fill)
    return dst


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


def composed_error(known, field, lo, hi, step=4):
    """|known(p + u(p)) - p| at every step-th voxel of [lo, hi)^3"""
    from sift3d_amd import api
    idx = np.arange(lo, hi, step)
    z, y, x = np.meshgrid(idx, idx, idx, indexing="ij")
    u = field[:, lo:hi:step, lo:hi:step, lo:hi:step].cpu().numpy().astype(np.float64)
    p = np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.float64)
    q = p + np.stack([u[0].ravel(), u[1].ravel(), u[2].ravel()], 1)
    return np.linalg.norm(api.tps_apply(known, q) - p, axis=1)


def test_register_dense_improves_on_the_spline():
    import torch
    from sift3d_amd import api, hip
    n = 176
    fixed = torch.empty((n, n, n), device="cuda")
    hip.synth_lattice(fixed, 0, 21)
    known, _ = _known_deformation(n)
    moving = dev_tps(fixed, known, fixed.shape)
    torch.cuda.synchronize()
    spl = api.register_deformable(moving, fixed)
    res = api.register_dense(moving, fixed)
    lo, hi = n // 8, n - n // 8
    u_s = api.displacement_field(spl.tps, fixed.shape)
    err_s = composed_error(known, u_s, lo, hi)
    err_d = composed_error(known, res.field, lo, hi)
    f = fixed.cpu().numpy()[lo:hi, lo:hi, lo:hi]
    ncc_s = _ncc(spl.warped.cpu().numpy()[lo:hi, lo:hi, lo:hi], f)
    ncc_d = _ncc(res.warped.cpu().numpy()[lo:hi, lo:hi, lo:hi], f)
    det = res.jacobian.det.cpu().numpy()
    inner_folded = int(np.count_nonzero(~(det[lo:hi, lo:hi, lo:hi] > 0)))
    print("register_dense: spline median %.4f p90 %.4f NCC %.5f; refined median %.4f p90 %.4f NCC %.5f; "
          "%d points; folded: %d whole grid, %d inner; det min %.4f max %.4f; msd %s"
          % (np.median(err_s), np.percentile(err_s, 90), ncc_s, np.median(err_d), np.percentile(err_d, 90), ncc_d,
             len(err_d), res.jacobian.folded, inner_folded, res.jacobian.min, res.jacobian.max,
             np.array2string(res.msd, precision=5, max_line_width=100000)))
    # measured on an MI355X: spline median 0.522, p90 1.108 voxel, NCC 0.98483; refined median 0.133, p90 0.263,
    # NCC 0.99756; 35937 points; folded 0 on the whole grid and inside; det in [0.754, 1.238]; msd 0.04788 ->
    # 0.02751 over the 50 iterations, falling at every one
    assert np.median(err_d) < np.median(err_s)
    assert np.percentile(err_d, 90) <= np.percentile(err_s, 90)
    assert ncc_d >= ncc_s
    assert inner_folded == 0
    assert res.msd[-1] < res.msd[0]
