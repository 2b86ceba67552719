"""GPU: multi-resolution demons (sift3d_hip_restrict2, sift3d_hip_field_prolong2, sift3d_amd_demons_multires_device and
the api layer) against the numpy restatement of the contract in include/sift3d_amd.h (tests/multires_restatement.py):
the transfers and the pyramid's field bit for bit, the statistics as tests/test_demons.py has them; then what the
pyramid is for: the capture-range case of tests/test_multires_host.py on the device, and tests/test_demons.py's
lattice case from a zero field."""
import numpy as np
import pytest

from tests import demons_restatement as dm
from tests import multires_restatement as mr
from tests.test_demons import SHAPES, _bits, _check_stats, _known_deformation, composed_error, dev_tps
from tests.test_multires_host import CAPTURE_ITERATIONS, capture_runs, check_capture

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def hip():
    import torch
    from sift3d_amd import hip as h
    h.lib()
    assert torch.cuda.is_available()
    h.current_stream(refresh=True)
    return h


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want, what):
    """bit for bit, but any NaN matches any NaN (numpy and the device may differ in a NaN's sign and payload)"""
    got = np.ascontiguousarray(got, F32)
    want = np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaNs differ at %d voxels" % (what, int((gn != wn).sum()))
    _bits(np.where(gn, F32(0), got), np.where(wn, F32(0), want), what)


# (nx, ny, nz): the field tests' shapes (odd axes, axes of 1 and 2), then axes of 1, 2 and 3 in every place, rows of
# a multiple of 4 (the 16-byte path), and grids wider than one tile in x (256 fine voxels) and deeper than one in z
GRIDS = [s for pair in SHAPES for s in pair] + [(3, 1, 2), (2, 3, 1), (1, 1, 1), (1, 2, 3), (64, 30, 24), (8, 7, 70),
                                                 (260, 9, 10), (263, 5, 3), (516, 3, 2)]
GRIDS = list(dict.fromkeys(GRIDS))


@pytest.mark.parametrize("nc", [1, 3, 12])
@pytest.mark.parametrize("grid", GRIDS)
def test_restrict2_bit_exact_against_restatement(hip, grid, nc):
    import torch
    nx, ny, nz = grid
    rng = np.random.default_rng(nc + nx + 7 * ny)
    src = rng.normal(0, 10, (nc, nz, ny, nx)).astype(F32)
    for scale in (1.0, 0.5):
        dst = torch.full((nc,) + mr.half_shape((nz, ny, nx)), 7.0, device="cuda")
        hip.restrict2(_t(src), dst, scale)
        _bits(dst.cpu().numpy(), mr.ref_restrict(src, scale), "restrict %s nc %d scale %g" % (grid, nc, scale))
    # 3-D input, allocated output, and a source that is not 16-byte aligned (the scalar path on the same values)
    got = hip.restrict2(_t(src[0]))
    _bits(got.cpu().numpy(), mr.ref_restrict(src[0]), "restrict 3-D %s" % (grid,))
    off = torch.empty(src.size + 1, device="cuda")[1:]
    off.copy_(_t(src).reshape(-1))
    got = hip.restrict2(off.reshape(src.shape))
    _bits(got.cpu().numpy(), mr.ref_restrict(src), "restrict misaligned %s" % (grid,))


@pytest.mark.parametrize("grid", GRIDS)
def test_prolong2_bit_exact_against_restatement(hip, grid):
    import torch
    nx, ny, nz = grid
    rng = np.random.default_rng(3 + nx + 7 * ny)
    uc = rng.normal(0, 3, (3,) + mr.half_shape((nz, ny, nx))).astype(F32)
    fine = torch.full((3, nz, ny, nx), 7.0, device="cuda")
    hip.field_prolong2(_t(uc), fine)
    want = mr.ref_prolong(uc, (nz, ny, nx))
    _bits(fine.cpu().numpy(), want, "prolong %s" % (grid,))
    # the even voxels, halved, are the coarse field
    _bits(fine.cpu().numpy()[:, ::2, ::2, ::2] * F32(0.5), uc, "prolong at even voxels %s" % (grid,))
    # an output that is not 16-byte aligned (the scalar path on the same values)
    off = torch.empty(3 * nx * ny * nz + 1, device="cuda")[1:].reshape(3, nz, ny, nx)
    hip.field_prolong2(_t(uc), off)
    _bits(off.cpu().numpy(), want, "prolong misaligned %s" % (grid,))


@pytest.mark.parametrize("grid", [(37, 29, 23), (64, 30, 24), (5, 29, 2)])
def test_nan_and_inf_propagate_as_numpy(hip, grid):
    nx, ny, nz = grid
    rng = np.random.default_rng(11)
    src = rng.normal(0, 10, (3, nz, ny, nx)).astype(F32)
    flat = src.reshape(-1)
    idx = rng.choice(flat.size, max(3, flat.size // 40), replace=False)
    flat[idx] = np.resize(np.array([np.nan, np.inf, -np.inf], F32), idx.size)
    want = mr.ref_restrict(src, 0.5)
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()
    _same(hip.restrict2(_t(src), None, 0.5).cpu().numpy(), want, "restrict nan %s" % (grid,))
    uc = src[:, :(nz + 1) // 2, :(ny + 1) // 2, :(nx + 1) // 2].copy()
    import torch
    fine = torch.empty((3, nz, ny, nx), device="cuda")
    hip.field_prolong2(_t(uc), fine)
    want = mr.ref_prolong(uc, (nz, ny, nx))
    assert np.isnan(want).any() and np.isinf(want).any()
    _same(fine.cpu().numpy(), want, "prolong nan %s" % (grid,))


def _fine_block(a, b, n):
    """the fine range a coarse range [a, b) of an axis of n needs, and the block-coarse index of coarse voxel a: the
    block starts at an even voxel one coarse voxel early (whose value the block's own clamp spoils) unless a is 0,
    and ends behind tap 2 b - 1 or at the grid's own face"""
    f0 = 2 * (a - 1) if a > 0 else 0
    return f0, min(2 * b, n), (1 if a > 0 else 0)


def test_restrict2_over_2_31_elements_sampled(hip):
    """nc * n > 2^31: blocks of coarse rows (full x extent) whose taps lie near the 2^31st source element and at the
    source's end, against the restatement of the fine blocks under them"""
    import torch
    nx, ny, nz, nc = 1024, 1024, 176, 12
    n = nx * ny * nz
    assert nc * n > 2 ** 31
    c_cross = 2 ** 31 // n
    z_cross = (2 ** 31 - c_cross * n) // (nx * ny)
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    src = torch.rand((nc, nz, ny, nx), device="cuda", generator=g)
    dst = hip.restrict2(src)
    cz, cy = (nz + 1) // 2, (ny + 1) // 2
    k = z_cross // 2
    blocks = [(c_cross, k - 1, k + 2, 0, 3), (c_cross, k - 1, k + 2, cy - 3, cy), (nc - 1, cz - 2, cz, cy - 4, cy),
              (0, 0, 2, 250, 253), (nc - 1, cz - 3, cz - 1, 100, 102)]
    for c, a, b, ya, yb in blocks:
        z0, z1, dz = _fine_block(a, b, nz)
        y0, y1, dy = _fine_block(ya, yb, ny)
        want = mr.ref_restrict(src[c, z0:z1, y0:y1, :].cpu().numpy())
        got = dst[c, a:b, ya:yb, :].cpu().numpy()
        _bits(got, want[dz:dz + b - a, dy:dy + yb - ya, :], "channel %d coarse z %d..%d y %d..%d" % (c, a, b, ya, yb))


def test_prolong2_over_2_31_elements_sampled(hip):
    """3 n > 2^31 on the fine grid: blocks of fine rows (full x extent) near the 2^31st element and at the grid's end
    against the restatement of the coarse blocks under them"""
    import torch
    nx, ny, nz = 1024, 1024, 704
    n = nx * ny * nz
    assert 3 * n > 2 ** 31
    z_cross = (2 ** 31 - 2 * n) // (nx * ny)
    g = torch.Generator(device="cuda")
    g.manual_seed(4)
    cz, cy, cx = mr.half_shape((nz, ny, nx))
    uc = (torch.rand((3, cz, cy, cx), device="cuda", generator=g) - 0.5) * 20.0
    fine = torch.empty((3, nz, ny, nx), device="cuda")
    hip.field_prolong2(uc, fine)
    k = z_cross // 2
    # coarse ranges [a, b): the fine block under them starts at 2 a and has 2 (b - a) - 1 voxels, one more at the
    # grid's own (even) high face
    blocks = [(2, k - 1, k + 2, 0, 3), (2, k - 1, k + 2, cy - 2, cy), (2, cz - 2, cz, cy - 3, cy), (0, 0, 2, 200, 202),
              (1, 100, 102, 300, 303)]
    for c, a, b, ya, yb in blocks:
        lz = 2 * (b - a) - 1 + (1 if b == cz else 0)
        ly = 2 * (yb - ya) - 1 + (1 if yb == cy else 0)
        cb = uc[:, a:b, ya:yb, :].cpu().numpy()
        want = mr.ref_prolong(cb, (lz, ly, nx))
        got = fine[c, 2 * a:2 * a + lz, 2 * ya:2 * ya + ly, :].cpu().numpy()
        _bits(got, want[c], "channel %d fine z %d.. y %d.." % (c, 2 * a, 2 * ya))
    assert 2 * (k - 1) <= z_cross < 2 * (k - 1) + 5


# ---- the pyramid driver ------------------------------------------------------------------------------------------
def _pyramid_case(shape, mshape, nc, levels, seed):
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    mx, my, mz = mshape
    F = rng.normal(0, 1, (nc, nz, ny, nx)).astype(F32)
    M = rng.normal(0, 1, (nc, mz, my, mx)).astype(F32)
    u = rng.normal(0, 1.5, (3, nz, ny, nx)).astype(F32)
    u[0] += F32(2.0)
    u[1] += F32(3.0)
    return mr.ref_pyramid(F, levels), mr.ref_pyramid(M, levels), u


# levels 1, 2, 3, uneven iterations, levels without iterations; odd grids with fixed and moving of different shapes, an
# axis of 2 that becomes 1, and 12 channels on a grid with rows of a multiple of 4
DRIVER = [(SHAPES[0][0], SHAPES[0][1], 3, levels, its)
          for levels, its in [(1, [3]), (2, [2, 1]), (3, [1, 2, 1]), (3, [2, 0, 3]), (3, [0, 2, 2]), (2, [0, 0])]]
DRIVER += [(SHAPES[1][0], SHAPES[1][1], 1, 3, [1, 2, 1]), (SHAPES[1][0], SHAPES[1][1], 1, 2, [2, 1]),
           ((40, 24, 17), (36, 30, 21), 12, 3, [2, 1, 2]), ((40, 24, 17), (36, 30, 21), 12, 1, [2])]


@pytest.mark.parametrize("update", ["additive", "diffeomorphic"])
@pytest.mark.parametrize("shape,mshape,nc,levels,its", DRIVER)
def test_driver_bit_exact_against_restatement(hip, oracle_mod, shape, mshape, nc, levels, its, update):
    Fs, Ms, u = _pyramid_case(shape, mshape, nc, levels, 5 + nc + levels)
    kw = dict(update=update, squarings=1)
    field = _t(u)
    stats = hip.demons_multires([_t(a) for a in Fs], [_t(a) for a in Ms], field, its, 0.8, 1.0, 1.5, **kw)
    s, c = hip.demons_stats(stats)
    want, per = mr.ref_multires(Fs, Ms, u, its, 0.8, 1.0, 1.5, oracle_mod, **kw)
    _bits(field.cpu().numpy(), want, "multires %s nc %d levels %d its %s %s" % (shape, nc, levels, its, update))
    assert len(s) == len(per) == sum(its)
    for k, (sd, ins) in enumerate(per):
        _check_stats(float(s[k]), int(c[k]), sd, ins, "record %d" % k)
    if levels == 1:
        # one level is the single-level driver, bit for bit
        single = _t(u)
        st1 = hip.demons(_t(Fs[0]), _t(Ms[0]), single, its[0], 0.8, 1.0, 1.5, **kw)
        _bits(field.cpu().numpy(), single.cpu().numpy(), "levels 1 against demons")
        np.testing.assert_array_equal(stats.cpu().numpy(), st1.cpu().numpy())
    # a second call gives the same bits
    again = _t(u)
    stats2 = hip.demons_multires([_t(a) for a in Fs], [_t(a) for a in Ms], again, its, 0.8, 1.0, 1.5, **kw)
    _bits(again.cpu().numpy(), field.cpu().numpy(), "second call")
    np.testing.assert_array_equal(stats2.cpu().numpy(), stats.cpu().numpy())


def test_api_layer(hip):
    """restrict_volume / prolong_field are the kernels; refine_field(levels=...) builds the pyramids by restriction and
    splits msd; levels=1 is today's call"""
    import torch
    from sift3d_amd import api
    rng = np.random.default_rng(8)
    fixed = rng.normal(0, 30, (21, 26, 31)).astype(F32)
    moving = rng.normal(0, 30, (19, 30, 27)).astype(F32)
    dF, dM = _t(fixed), _t(moving)
    _bits(api.restrict_volume(dF).cpu().numpy(), mr.ref_restrict(fixed), "restrict_volume")
    uc = rng.normal(0, 2, (3, 11, 13, 16)).astype(F32)
    _bits(api.prolong_field(_t(uc), (21, 26, 31)).cpu().numpy(), mr.ref_prolong(uc, (21, 26, 31)), "prolong_field")
    with pytest.raises(ValueError):
        api.prolong_field(_t(uc), (21, 26, 30))
    for bad in (dict(levels=0), dict(levels=7), dict(levels=2, level_iterations=[1]),
                dict(levels=2, level_iterations=[1, -1])):
        with pytest.raises(ValueError):
            api.refine_field(dM, dF, None, 2, features="intensity", **bad)
    one = api.refine_field(dM, dF, None, 3, features="intensity")
    lv1 = api.refine_field(dM, dF, None, 3, features="intensity", levels=1)
    assert type(lv1) is api.DemonsRefinement and torch.equal(one.field, lv1.field)
    r = api.refine_field(dM, dF, None, 9, 1.0, 1.0, 1.0, features="intensity", levels=3, level_iterations=[2, 0, 3])
    assert type(r) is api.MultiresRefinement
    assert r.level_slices == (slice(3, 5), slice(3, 3), slice(0, 3)) and len(r.msd) == 5
    Fs, Ms = mr.ref_pyramid(fixed, 3), mr.ref_pyramid(moving, 3)
    from oracle import sift3d_oracle as so
    want, per = mr.ref_multires(Fs, Ms, np.zeros((3,) + fixed.shape, F32), [2, 0, 3], 1.0, 1.0, 1.0, so)
    _bits(r.field.cpu().numpy(), want, "refine_field levels 3")
    for k, (sd, ins) in enumerate(per):
        s, c = np.sum(sd[ins]), int(ins.sum())
        assert abs(r.msd[k] - s / c) <= dm.gamma(c) * s / c
    # descriptors: every level's descriptors are those of that level's restricted volume
    rd = api.refine_field(dM, dF, None, 2, levels=2, sigma=1.2)
    Fd = [api.dense_descriptors(v, 1.2) for v in (dF, api.restrict_volume(dF))]
    Md = [api.dense_descriptors(v, 1.2) for v in (dM, api.restrict_volume(dM))]
    u = torch.zeros((3,) + tuple(dF.shape), device="cuda")
    hip.demons_multires(Fd, Md, u, [2, 2], api.DEMONS_ALPHA, api.DEMONS_SIGMA_FLUID, api.DEMONS_SIGMA_DIFFUSION)
    assert torch.equal(rd.field, u) and len(rd.msd) == 4 and rd.level_slices == (slice(2, 4), slice(0, 2))


# ---- what it must achieve ----------------------------------------------------------------------------------------
def test_three_levels_capture_what_one_level_cannot(hip, oracle_mod):
    """tests/test_multires_host.py's capture-range case through api.refine_field on the device: the same conditions,
    and the three-level field equal to the restatement's bit for bit (the driver test at a realistic size)"""
    from sift3d_amd import api

    def run(Fs, Ms, its, kw):
        r = api.refine_field(_t(Ms[0]), _t(Fs[0]), None, 0, kw["alpha"], kw["sigma_fluid"], kw["sigma_diffusion"],
                             features="intensity", levels=len(its), level_iterations=its)
        return r.field.cpu().numpy(), float(r.msd[-1])

    d, one, three, hundred = capture_runs(run)
    check_capture(d, one, three, hundred, "device")
    F, M, _, kw = mr.capture_case(oracle_mod)
    want, _ = mr.ref_multires(mr.ref_pyramid(F, 3), mr.ref_pyramid(M, 3), np.zeros((3,) + F.shape, F32),
                              list(CAPTURE_ITERATIONS), so=oracle_mod, **kw)
    _bits(three[0], want, "capture case, three levels")


def _lattice_case():
    import torch
    from sift3d_amd import hip
    n = 176
    fixed = torch.empty((n, n, n), device="cuda")
    hip.synth_lattice(fixed, 0, 21)
    known, _ = _known_deformation(n)
    moving = dev_tps(fixed, known, fixed.shape)
    torch.cuda.synchronize()
    return n, fixed, moving, known


def _report(name, known, r, lo, hi):
    err = composed_error(known, r.field, lo, hi)
    det = r.jacobian.det.cpu().numpy()
    inner = int(np.count_nonzero(~(det[lo:hi, lo:hi, lo:hi] > 0)))
    print("%s: median %.4f p90 %.4f voxel; folded: %d whole grid, %d inner; det min %.4f max %.4f; msd %.5f -> %.5f "
          "(%d iterations)" % (name, np.median(err), np.percentile(err, 90), r.jacobian.folded, inner, r.jacobian.min,
                               r.jacobian.max, r.msd[0], r.msd[-1], len(r.msd)))
    return float(np.median(err)), float(np.percentile(err, 90)), inner


def test_three_levels_from_zero_beat_one_level_from_zero():
    """tests/test_demons.py's 176^3 lattice case without keypoints or spline: refine_field from a zero field on three
    levels against one level with the same total iteration count.  Measured on an MI355X (35937 points):
      three levels, 50 + 50 + 50: median 0.1326, p90 0.2626 voxel; no folds; msd 0.07668 -> 0.02753
      one level, 150:             median 0.1467, p90 0.3561 voxel; no folds; msd 0.70786 -> 0.08418
      register_dense (test_demons.py): median 0.133, p90 0.263"""
    from sift3d_amd import api
    n, fixed, moving, known = _lattice_case()
    lo, hi = n // 8, n - n // 8
    r3 = api.refine_field(moving, fixed, None, levels=3)
    r1 = api.refine_field(moving, fixed, None, 3 * api.DEMONS_ITERATIONS)
    assert len(r3.msd) == len(r1.msd) == 150
    m3, _, inner3 = _report("three levels from zero", known, r3, lo, hi)
    m1, _, _ = _report("one level from zero", known, r1, lo, hi)
    assert m3 < m1
    assert r3.jacobian.folded == 0 and inner3 == 0


def test_register_dense_on_three_levels_is_not_worse():
    """register_dense starts near the answer already, so the pyramid has little to add; restricting the spline's field
    (a low-pass) must not cost accuracy either.  Both calls are deterministic (two runs give the same bits), so the
    run-to-run spread is 0 and the allowance is the resolution of the error measure instead: composed_error goes
    through tps_apply in float64 on 35937 points whose field values are float32 of magnitude <= 16 voxels, 2^-20
    voxel per value; 1e-3 voxel is far above that and far below the 0.133 voxel median.  Measured on an MI355X: one
    level median 0.1327, p90 0.2629; three levels (50 + 50 + 50) median 0.1326, p90 0.2626; no folds in either."""
    from sift3d_amd import api
    n, fixed, moving, known = _lattice_case()
    lo, hi = n // 8, n - n // 8
    d1 = api.register_dense(moving, fixed)
    d3 = api.register_dense(moving, fixed, levels=3)
    assert type(d3) is api.MultiresRegistration and len(d3.msd) == 150
    m1, p1, _ = _report("register_dense, one level", known, d1, lo, hi)
    m3, p3, inner3 = _report("register_dense, three levels", known, d3, lo, hi)
    assert m3 <= m1 + 1e-3
    assert inner3 == 0
