"""GPU: masks in demons (sift3d_hip_demons_force_masked, sift3d_amd_demons_masked_device,
sift3d_amd_logdemons_masked_device, api.refine_field / register_dense with masks) against the numpy restatement of the
contract in include/sift3d_amd.h, "Masks in demons" (tests/demons_mask_restatement.py): delta, the fields and the
counts bit for bit, the sums within the bound of any summation order; byte equality with the unmasked entries; the
mask rule's edges; the wave that counts nothing; and the guarantee a user masks for (content invariance)."""
import numpy as np
import pytest

from tests import demons_mask_restatement as dk
from tests import demons_restatement as dm
from tests import logdemons_restatement as lg
from tests import multires_restatement as mr
from tests.test_demons import SHAPES, _bits, _case, _check_stats, _t

pytestmark = pytest.mark.gpu

F32 = np.float32
# (fixed (nx, ny, nz), moving (mx, my, mz)): test_demons.py's, and one with more than one wave along x, whose end
# lanes load their neighbours with masks present
MASK_SHAPES = SHAPES + [((70, 6, 5), (66, 7, 6))]


@pytest.fixture(scope="module")
def hip():
    import torch
    from sift3d_amd import hip as h
    h.lib()
    assert torch.cuda.is_available()
    h.current_stream(refresh=True)
    return h


def _zyx(s):
    return (s[2], s[1], s[0])


def _mask(shape_zyx, seed, p=0.6):
    """random binary, p in"""
    return (np.random.default_rng(seed).random(shape_zyx) < p).astype(F32)


def _tm(w):
    return None if w is None else _t(w)


def _force(hip, F, W, u, mshape_zyx, alpha, WF, WM):
    """(delta, sum, count) of one masked force on the device"""
    import torch
    step = torch.full((3,) + tuple(F.shape[-3:]), float("nan"), device="cuda")
    stats = hip.demons_force(_t(F), _t(W), _t(u), step, alpha, mshape_zyx, mask_fixed=_tm(WF), mask_moving=_tm(WM))
    s, c = hip.demons_stats(stats)
    return step.cpu().numpy(), float(s[0]), int(c[0])


# ---- 1. the force against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["fixed", "moving", "both"])
@pytest.mark.parametrize("nc", [1, 12])
@pytest.mark.parametrize("shape,mshape", MASK_SHAPES)
def test_force_bit_exact_against_restatement(hip, shape, mshape, nc, which):
    F, _, W, u = _case(shape, mshape, nc, 10 * nc + shape[1])
    WF = _mask(_zyx(shape), 3) if which != "moving" else None
    WM = _mask(_zyx(mshape), 4) if which != "fixed" else None
    for alpha in (1.0, 0.3):
        got, s, c = _force(hip, F, W, u, _zyx(mshape), alpha, WF, WM)
        want, sd, ins = dk.ref_force(F, W, u, _zyx(mshape), alpha, WF, WM)
        plain = dm.inside(u, _zyx(mshape))
        assert 0 < ins.sum() < plain.sum() < plain.size     # the field samples outside, the masks take more away
        _bits(got, want, "masked force %s / %s nc %d %s alpha %g" % (shape, mshape, nc, which, alpha))
        _check_stats(s, c, sd, ins, "masked force stats")


# ---- 2. byte equality with the unmasked entries ----------------------------------------------------------------------
@pytest.mark.parametrize("nc", [1, 12])
@pytest.mark.parametrize("shape,mshape", MASK_SHAPES)
def test_force_with_all_in_masks_is_the_unmasked_force(hip, shape, mshape, nc):
    import torch
    F, _, W, u = _case(shape, mshape, nc, 5 + nc)
    step = torch.full((3,) + F.shape[1:], float("nan"), device="cuda")
    st = hip.demons_force(_t(F), _t(W), _t(u), step, 0.8, _zyx(mshape))
    want, want_st = step.cpu().numpy(), st.cpu().numpy()
    ones_f, ones_m = np.ones(_zyx(shape), F32), np.ones(_zyx(mshape), F32)
    for WF, WM in ((ones_f, None), (None, ones_m), (ones_f, ones_m), (np.full_like(ones_f, 0.5), ones_m * 2)):
        step.fill_(float("nan"))
        st = hip.demons_force(_t(F), _t(W), _t(u), step, 0.8, _zyx(mshape), mask_fixed=_tm(WF), mask_moving=_tm(WM))
        _bits(step.cpu().numpy(), want, "all-in masks")
        np.testing.assert_array_equal(st.cpu().numpy(), want_st)       # sum and count, bit for bit


def _run(hip, update, F, M, u0, its, WFs=None, WMs=None, sigmas=(1.0, 1.5), alpha=0.8, K=2):
    """(field or velocity, stats bytes) of one driver run; F, M: arrays, or lists of them per level"""
    Fs, Ms = (F, M) if isinstance(F, list) else ([F], [M])
    its = its if isinstance(its, list) else [its]
    field = _t(u0)
    tF, tM = [_t(a) for a in Fs], [_t(a) for a in Ms]
    kw = {}
    if WFs is not None or WMs is not None:
        kw = dict(masks_fixed=None if WFs is None else [_tm(w) for w in WFs],
                  masks_moving=None if WMs is None else [_tm(w) for w in WMs])
    if update in ("additive", "diffeomorphic"):
        st = hip.demons_multires(tF, tM, field, its, alpha, sigmas[0], sigmas[1], update=update,
                                 squarings=K if update == "diffeomorphic" else 0, **kw)
    else:
        st = hip.logdemons(tF, tM, field, its, alpha, sigmas[0], sigmas[1], symmetric=update == "symmetric", bch=1,
                           velocity_squarings=K, **kw)
    return field.cpu().numpy(), st.cpu().numpy()


def _pair(update, nc, seed):
    """shape pair 0; the symmetric update needs one shape"""
    shape, mshape = SHAPES[0]
    if update == "symmetric":
        mshape = shape
    F, M, _, u = _case(shape, mshape, nc, seed)
    if update == "symmetric":
        M = (F + np.random.default_rng(seed + 1).normal(0, 0.4, F.shape)).astype(F32)
    return F, M, (u * F32(0.5)).astype(F32)


@pytest.mark.parametrize("update", ["additive", "diffeomorphic", "logdomain", "symmetric"])
def test_drivers_with_all_in_masks_are_the_unmasked_drivers(hip, update):
    F, M, u = _pair(update, 3, 21)
    want, want_st = _run(hip, update, F, M, u, 3)
    assert not np.array_equal(want, u)
    ones_f, ones_m = np.ones(F.shape[1:], F32), np.ones(M.shape[1:], F32)
    for WF, WM in ((ones_f, None), (None, ones_m), (ones_f, ones_m)):
        got, got_st = _run(hip, update, F, M, u, 3, [WF], [WM])
        _bits(got, want, "%s, all-in masks" % update)
        np.testing.assert_array_equal(got_st, want_st)
    # hip.demons with a mask is the one-level pyramid entry
    if update in ("additive", "diffeomorphic"):
        field = _t(u)
        st = hip.demons(_t(F), _t(M), field, 3, 0.8, 1.0, 1.5, update=update, squarings=2, mask_fixed=_t(ones_f))
        _bits(field.cpu().numpy(), want, "hip.demons %s, all-in mask" % update)
        np.testing.assert_array_equal(st.cpu().numpy(), want_st)


@pytest.mark.parametrize("log", [False, True])
def test_null_mask_table_is_the_unmasked_entry(hip, log):
    """masks == NULL through the masked C entries themselves"""
    import torch
    F, M, u = _pair("additive", 2, 8)
    want, want_st = _run(hip, "logdomain" if log else "additive", F, M, u, 3)
    tF, tM, field = _t(F), _t(M), _t(u)
    tab, levels, nc, _ = hip._demons_levels("test", [tF], [tM], field, [3])
    L = hip.lib()
    nz, ny, nx = F.shape[1:]
    stats = torch.empty(3 * 2, dtype=torch.int64, device="cuda")
    if log:
        work = torch.empty(L.sift3d_amd_logdemons_work_floats(nx, ny, nz, nc, 0, 1), device="cuda")
        rc = L.sift3d_amd_logdemons_masked_device(tab, None, levels, nc, field.data_ptr(), 0.8, 1.0, 1.5, 0, 1, 2,
                                                  work.data_ptr(), stats.data_ptr(), hip.current_stream())
    else:
        work = torch.empty(L.sift3d_amd_demons_multires_work_floats(nx, ny, nz, nc, 0, 1), device="cuda")
        rc = L.sift3d_amd_demons_masked_device(tab, None, levels, nc, field.data_ptr(), 0.8, 1.0, 1.5, 0, 0,
                                               work.data_ptr(), stats.data_ptr(), hip.current_stream())
    assert rc == 0
    _bits(field.cpu().numpy(), want, "NULL mask table")
    np.testing.assert_array_equal(stats.cpu().numpy(), want_st)


# ---- 3. the mask rule's edges on the device --------------------------------------------------------------------------
EDGE = (70, 6, 5)                                            # (nx, ny, nz), fixed and moving


def _edge_images(nc=2, seed=31):
    rng = np.random.default_rng(seed)
    F = rng.normal(0, 1, (nc,) + _zyx(EDGE)).astype(F32)
    W = (F + rng.normal(0, 0.5, F.shape)).astype(F32)
    return F, W


def test_edge_mask_values(hip):
    """0.5f, 2 and +inf are in; nextafterf(0.5f, 0), NaN and -1 are out: in either mask"""
    F, W = _edge_images()
    vals = np.array([0.5, np.nextafter(F32(0.5), F32(0)), np.nan, np.inf, -1.0, 2.0], F32)
    is_in = np.array([True, False, False, True, False, True])
    n = F[0].size
    pick = np.random.default_rng(1).integers(0, 6, n)
    Wv = vals[pick].reshape(F.shape[1:])
    u = np.zeros((3,) + F.shape[1:], F32)                    # q = p: the moving mask is read at p
    for WF, WM in ((Wv, None), (None, Wv)):
        got, s, c = _force(hip, F, W, u, _zyx(EDGE), 1.0, WF, WM)
        want, sd, ins = dk.ref_force(F, W, u, _zyx(EDGE), 1.0, WF, WM)
        assert np.array_equal(ins, is_in[pick].reshape(F.shape[1:]))
        _bits(got, want, "mask values")
        _check_stats(s, c, sd, ins, "mask values")
        assert not got[:, ~ins].view(np.uint32).any()        # +0.0f where not counted
        assert got[:, ins].any()


def test_edge_half_integer_and_upper_face(hip):
    F, W = _edge_images()
    shape = F.shape[1:]
    nx = shape[2]
    # u = 0.5f exactly: q is a half-integer and the mask voxel is the upper one
    u = np.zeros((3,) + shape, F32)
    u[0] = F32(0.5)
    WM = np.zeros(shape, F32)
    WM[:, :, 40] = 1.0
    got, s, c = _force(hip, F, W, u, shape, 1.0, None, WM)
    want, sd, ins = dk.ref_force(F, W, u, shape, 1.0, None, WM)
    assert ins[:, :, 39].all() and ins.sum() == shape[0] * shape[1] == c
    _bits(got, want, "half-integer q")
    # the same along y and z
    for d, (axis, at) in ((1, (1, 3)), (2, (0, 2))):
        u = np.zeros((3,) + shape, F32)
        u[d] = F32(0.5)
        WM = np.zeros(shape, F32)
        idx = [slice(None)] * 3
        idx[axis] = at
        WM[tuple(idx)] = 1.0
        got, s, c = _force(hip, F, W, u, shape, 1.0, None, WM)
        want, sd, ins = dk.ref_force(F, W, u, shape, 1.0, None, WM)
        idx[axis] = at - 1
        assert ins[tuple(idx)].all() and ins.sum() == ins[tuple(idx)].size == c
        _bits(got, want, "half-integer q, axis %d" % d)
    # q exactly on the upper face m - 1: inside, and the mask voxel is m - 1
    u = np.zeros((3,) + shape, F32)
    u[0][:, :, nx - 2] = 1.0
    u[1][:, 4, :] = 1.0                                      # y = 4 -> q_y = 5 = my - 1
    WM = np.zeros(shape, F32)
    WM[:, 5, nx - 1] = 1.0
    got, s, c = _force(hip, F, W, u, shape, 1.0, None, WM)
    want, sd, ins = dk.ref_force(F, W, u, shape, 1.0, None, WM)
    assert ins[:, 4:, nx - 2:].all() and ins.sum() == 4 * shape[0] == c
    _bits(got, want, "q on the upper face")
    _check_stats(s, c, sd, ins, "q on the upper face")


def test_edge_outside_q_reads_voxel_0_and_the_inside_test_decides(hip):
    F, W = _edge_images()
    shape = F.shape[1:]
    rng = np.random.default_rng(2)
    u = rng.normal(0, 1.0, (3,) + shape).astype(F32)
    u[0][:, :, :6] -= F32(8.0)                               # outside
    u[2][1] = np.float32("nan")                              # a NaN is outside
    u[:, 0, 0, 0] = F32(1.0)                                 # no inside q lands on voxel 0 (checked below)
    ins0 = dm.inside(u, shape)
    assert 0 < ins0.sum() < ins0.size
    # (voxel 0 is the nearest voxel only of a q below 0.5 on every axis)
    q = [p.astype(np.float64) + ud.astype(np.float64) for p, ud in zip(np.meshgrid(*map(np.arange, shape),
                                                                                   indexing="ij")[::-1], u)]
    with np.errstate(invalid="ignore"):
        assert not (ins0 & (q[0] < 0.5) & (q[1] < 0.5) & (q[2] < 0.5)).any()
    want, sd, ins = dm.ref_force(F, W, u, shape, 1.0)
    for v0 in (0.0, 1.0):
        WM = np.ones(shape, F32)
        WM[0, 0, 0] = v0
        got, s, c = _force(hip, F, W, u, shape, 1.0, None, WM)
        _bits(got, want, "outside q, voxel 0 = %g" % v0)     # the unmasked force: the inside test decided alone
        _check_stats(s, c, sd, ins, "outside q")
        assert c == ins0.sum()


# ---- 4. the wave that counts nothing ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [1, 12])
def test_all_out_wave(hip, nc):
    """The fixed mask is out over x 64 .. 127, y 4 .. 7, z 2 .. 3: one wave's whole tile (64 x 1 x 2) four times
    over, aligned to the tile grid (64 x 4 x 2), and in elsewhere; then the same with one voxel of the block in, so
    that one of the four waves has to run"""
    shape, mshape = (130, 9, 5), (128, 10, 6)
    F, _, W, u = _case(shape, mshape, nc, 40 + nc)
    u = (u * F32(0.3)).astype(F32)
    u[:, 3, 6, 100] = 0.0                                     # inside, and its q is the voxel itself
    WF = np.ones(_zyx(shape), F32)
    WF[2:4, 4:8, 64:128] = 0.0
    for one_in in (False, True):
        if one_in:
            WF[3, 6, 100] = 1.0
        for WM in (None, _mask(_zyx(mshape), 6)):
            got, s, c = _force(hip, F, W, u, _zyx(mshape), 0.7, WF, WM)
            want, sd, ins = dk.ref_force(F, W, u, _zyx(mshape), 0.7, WF, WM)
            assert ins[2:4, 4:8, 64:128].sum() == int(ins[3, 6, 100]) and (WM is not None or ins[3, 6, 100] == one_in)
            _bits(got, want, "all-out wave, nc %d" % nc)
            _check_stats(s, c, sd, ins, "all-out wave")
            assert not got[:, 2:4, 4:8, 64:100].view(np.uint32).any()
    # a moving mask all out: every wave counts nothing
    got, s, c = _force(hip, F, W, u, _zyx(mshape), 0.7, None, np.zeros(_zyx(mshape), F32))
    assert not got.view(np.uint32).any() and c == 0 and s == 0.0


# ---- 5. the drivers against the restatement --------------------------------------------------------------------------
def _check_run(got, got_st, want, per, what):
    from sift3d_amd import hip as h
    import torch
    _bits(got, want, what)
    s, c = h.demons_stats(torch.from_numpy(got_st))
    assert len(s) == len(per)
    for k, (sd, ins) in enumerate(per):
        _check_stats(float(s[k]), int(c[k]), sd, ins, "%s, iteration %d" % (what, k))


@pytest.mark.parametrize("update", ["additive", "diffeomorphic"])
def test_driver_bit_exact_against_restatement(hip, oracle_mod, update):
    F, M, u = _pair(update, 3, 50)
    WF, WM = _mask(F.shape[1:], 7), _mask(M.shape[1:], 8)
    got, st = _run(hip, update, F, M, u, 3, [WF], [WM])
    want, per = dk.ref_demons(F, M, u, 3, 0.8, 1.0, 1.5, oracle_mod, WF, WM, update, 2)
    _check_run(got, st, want, per, update)
    unmasked, _ = _run(hip, update, F, M, u, 3)
    assert not np.array_equal(got, unmasked)


def test_two_levels_bit_exact_against_restatement(hip, oracle_mod):
    """per-level masks restricted from the float masks (never thresholded copies); the moving mask of level 1 NULL"""
    F, M, u = _pair("additive", 2, 51)
    WF, WM = _mask(F.shape[1:], 9, 0.7), _mask(M.shape[1:], 10, 0.7)
    Fs, Ms = mr.ref_pyramid(F, 2), mr.ref_pyramid(M, 2)
    WFs, WMs = dk.mask_pyramid(WF, 2), dk.mask_pyramid(WM, 2)
    assert ((WFs[1] > 0) & (WFs[1] < 1)).any()               # level 1's mask is the float restriction
    WMs[1] = None
    got, st = _run(hip, "additive", Fs, Ms, u, [2, 3], WFs, WMs)
    want, per = dk.ref_multires(Fs, Ms, u, [2, 3], 0.8, 1.0, 1.5, oracle_mod, WFs, WMs)
    _check_run(got, st, want, per, "two levels")


@pytest.mark.parametrize("update", ["logdomain", "symmetric"])
def test_logdemons_bit_exact_against_restatement(hip, oracle_mod, update):
    F, M, v = _pair(update, 2, 52)
    WF, WM = _mask(F.shape[1:], 11), _mask(M.shape[1:], 12)
    got, st = _run(hip, update, F, M, v, 3, [WF], [WM])
    want, per = dk.ref_logdemons(F, M, v, 3, 0.8, 1.0, 1.5, oracle_mod, WF, WM, symmetric=update == "symmetric",
                                 bch=1, squarings=2)
    _check_run(got, st, want, per, update)


# ---- 6. the symmetric swap -------------------------------------------------------------------------------------------
def test_symmetric_swap_negates_the_velocity(hip):
    F, M, v = _pair("symmetric", 2, 53)
    WF, WM = _mask(F.shape[1:], 13), _mask(M.shape[1:], 14)
    a, _ = _run(hip, "symmetric", F, M, v, 3, [WF], [WM])
    b, _ = _run(hip, "symmetric", M, F, -v, 3, [WM], [WF])
    assert not np.array_equal(a, v)
    _bits(lg.unsigned_zero(b), lg.unsigned_zero(-a), "swapped run")
    # and it is the masks' exchange that does it: with the masks left in place the runs differ
    c, _ = _run(hip, "symmetric", M, F, -v, 3, [WF], [WM])
    assert not np.array_equal(lg.unsigned_zero(c), lg.unsigned_zero(-a))


# ---- 7. content invariance -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("update", ["additive", "logdomain"])
def test_content_out_of_the_fixed_mask_never_reaches_the_result(hip, update):
    """F changed (finite) at the voxels whose whole 3 x 3 x 3 neighbourhood is out of the fixed mask: the stencil
    reaches one voxel and W does not depend on F, so the field and the statistics keep their bits"""
    F, M, u = _pair(update, 3, 54)
    nz, ny, nx = F.shape[1:]
    WF = _mask(F.shape[1:], 15, 0.8)
    WF[6:17, 8:20, 10:30] = 0.0                               # a lesion
    out = WF < 0.5
    pad = np.pad(out, 1, constant_values=True)                # off the grid counts as out: nothing is read there
    deep = np.ones_like(out)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                deep &= pad[dz:dz + nz, dy:dy + ny, dx:dx + nx]
    assert deep[7:16, 9:19, 11:29].all() and deep.sum() >= 9 * 10 * 18
    F2 = F.copy()
    F2[:, deep] = np.random.default_rng(3).normal(0, 50, (F.shape[0], int(deep.sum()))).astype(F32)
    a, sa = _run(hip, update, F, M, u, 4, [WF], None)
    b, sb = _run(hip, update, F2, M, u, 4, [WF], None)
    _bits(b, a, "%s, content invariance" % update)
    np.testing.assert_array_equal(sb, sa)
    # unmasked, the same change does reach the result
    c, _ = _run(hip, update, F, M, u, 4)
    d, _ = _run(hip, update, F2, M, u, 4)
    assert not np.array_equal(c, d)


# ---- 8. no smoothing -------------------------------------------------------------------------------------------------
def test_without_smoothing_an_uncounted_voxel_keeps_its_bits(hip):
    F, M, u = _pair("additive", 2, 55)
    WF = _mask(F.shape[1:], 16, 0.5)
    got, _ = _run(hip, "additive", F, M, u, 4, [WF], None, sigmas=(0.0, 0.0))
    out = WF < 0.5
    assert not (u == 0).any()                                 # (u + 0.0f keeps every bit but -0.0f's sign)
    _bits(got[:, out], u[:, out], "voxels out of the fixed mask")
    assert (got[:, ~out] != u[:, ~out]).any()


# ---- 9. the public interface -----------------------------------------------------------------------------------------
def _volumes(n=24):
    import torch
    from sift3d_amd import api
    vol = api.synth_survey(n + 4)
    fixed = np.ascontiguousarray(vol[2:n + 2, 2:n + 2, 2:n + 2], F32)
    moving = np.ascontiguousarray(vol[3:n + 3, 2:n + 2, 1:n + 1], F32)
    return torch.from_numpy(fixed).cuda(), torch.from_numpy(moving).cuda()


def test_refine_field_mask_kinds_agree(hip, oracle_mod):
    import torch
    from sift3d_amd import api
    fixed, moving = _volumes()
    region = np.zeros(fixed.shape, bool)
    region[4:20, 3:22, 5:19] = True
    kw = dict(iterations=3, features="intensity")
    runs = [api.refine_field(moving, fixed, mask_fixed=m, mask_moving=m, **kw)
            for m in (region, region.astype(np.uint8) * 7, region.astype(F32), torch.from_numpy(region).cuda(),
                      torch.from_numpy(np.where(region, 0.5, 0.25).astype(F32)).cuda())]
    assert isinstance(runs[0], api.DemonsRefinement)
    for r in runs[1:]:
        _bits(r.field.cpu().numpy(), runs[0].field.cpu().numpy(), "mask kinds")
        np.testing.assert_array_equal(r.msd, runs[0].msd)
    # msd is the mean over the counted voxels
    w = region.astype(F32)
    _, per = dk.ref_demons(fixed.cpu().numpy(), moving.cpu().numpy(), np.zeros((3,) + region.shape, F32), 3,
                           api.DEMONS_ALPHA, api.DEMONS_SIGMA_FLUID, api.DEMONS_SIGMA_DIFFUSION, oracle_mod, w, w)
    for k, (sd, ins) in enumerate(per):
        s, c = dm.ref_stats(sd, ins)
        assert 0 < c <= region.sum()
        assert abs(runs[0].msd[k] - s / c) <= (dm.gamma(c) + 2.0 ** -52) * (s / c)
    # with both masks None: today's call
    plain = api.refine_field(moving, fixed, **kw)
    u = torch.zeros((3,) + tuple(fixed.shape), device="cuda")
    st = hip.demons(fixed, moving, u, 3, api.DEMONS_ALPHA, api.DEMONS_SIGMA_FLUID, api.DEMONS_SIGMA_DIFFUSION)
    _bits(plain.field.cpu().numpy(), u.cpu().numpy(), "masks None")
    s, c = hip.demons_stats(st)
    np.testing.assert_array_equal(plain.msd, s / c.astype(np.float64))
    assert not np.array_equal(plain.field.cpu().numpy(), runs[0].field.cpu().numpy())


def test_refine_field_levels_and_symmetric_with_masks(hip, oracle_mod):
    from sift3d_amd import api
    fixed, moving = _volumes()
    region = np.zeros(fixed.shape, F32)
    region[4:20, 3:22, 5:19] = 1.0
    r = api.refine_field(moving, fixed, iterations=2, features="intensity", levels=2, mask_fixed=region,
                         mask_moving=region > 0)
    assert isinstance(r, api.MultiresRefinement) and len(r.msd) == 4
    F, M = fixed.cpu().numpy(), moving.cpu().numpy()
    want, _ = dk.ref_multires(mr.ref_pyramid(F, 2), mr.ref_pyramid(M, 2), np.zeros((3,) + F.shape, F32), [2, 2],
                              api.DEMONS_ALPHA, api.DEMONS_SIGMA_FLUID, api.DEMONS_SIGMA_DIFFUSION, oracle_mod,
                              dk.mask_pyramid(region, 2), dk.mask_pyramid(region, 2))
    _bits(r.field.cpu().numpy(), want, "levels=2: the masks are restricted, not thresholded")
    s = api.refine_field(moving, fixed, iterations=2, features="intensity", update="symmetric", levels=2,
                         mask_fixed=region, velocity_squarings=2)
    assert isinstance(s, api.MultiresLogDemonsRefinement) and len(s.msd) == 4
    assert np.isfinite(s.velocity.cpu().numpy()).all() and np.isfinite(s.msd).all()
    t = api.refine_field(moving, fixed, iterations=2, features="intensity", update="symmetric", levels=2,
                         velocity_squarings=2)
    assert not np.array_equal(s.velocity.cpu().numpy(), t.velocity.cpu().numpy())


def test_register_dense_hands_the_masks_to_refine_field(hip, monkeypatch):
    import torch
    from sift3d_amd import api
    fixed, moving = _volumes()
    seen = {}
    real = api.refine_field

    def spy(*a, **kw):
        seen.update(kw)
        return real(*a, **kw)

    Spline = type("Spline", (), dict(A=np.eye(3, 4), tps=None, inliers=0, num_matches=0))
    monkeypatch.setattr(api, "register_deformable", lambda m, f, **kw: seen.update(deformable=kw) or Spline())
    monkeypatch.setattr(api, "displacement_field",
                        lambda tps, shape, device=None: torch.zeros((3,) + tuple(shape), device="cuda"))
    monkeypatch.setattr(api, "refine_field", spy)
    wf = np.zeros(fixed.shape, bool)
    wf[2:20, 2:20, 2:20] = True
    wm = torch.ones(moving.shape, device="cuda")
    r = api.register_dense(moving, fixed, iterations=2, features="intensity", mask_fixed=wf, mask_moving=wm)
    assert seen["mask_fixed"] is wf and seen["mask_moving"] is wm
    assert seen["deformable"] == {}                           # the keypoint and spline stages see no mask
    want = real(moving, fixed, torch.zeros((3,) + tuple(fixed.shape), device="cuda"), iterations=2,
                features="intensity", mask_fixed=wf, mask_moving=wm)
    _bits(r.field.cpu().numpy(), want.field.cpu().numpy(), "register_dense")
    np.testing.assert_array_equal(r.msd, want.msd)
