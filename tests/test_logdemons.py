"""Log-domain demons on the device against the numpy restatement (include/sift3d_amd.h, "Log-domain demons"): the
Lie bracket kernel, the signed exponential, the driver and its pyramid bit for bit, the api layer, and the 176^3
lattice case end to end."""
import numpy as np
import pytest

from tests import logdemons_restatement as ld
from tests import multires_restatement as mr
from tests.test_demons import SHAPES, _bits, _check_stats, _known_deformation, composed_error
from tests.test_multires import _lattice_case, _report

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


def _pair(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 1, (3,) + shape).astype(F32), rng.normal(0, 1, (3,) + shape).astype(F32))


# ---- 1. the bracket kernel ---------------------------------------------------------------------------------------
# (nz, ny, nx).  The kernel's tile is 64 x 4 columns of 8 planes: (9, 5, 67) is tile + 1 on every axis (with rows of
# 67 a second tile along x holds 3 voxels), so every halo read crosses a tile.
GRIDS = [(37, 29, 23), (37, 2, 23), (1, 29, 2), (1, 1, 1), (9, 5, 67)]
MODES = ["bracket", "bch1"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("grid", GRIDS)
def test_bracket_bit_exact_against_restatement(hip, grid, mode):
    a, b = _pair(grid, 1 + grid[1])
    want = ld.ref_bracket(a, b, mode)
    _bits(hip.field_bracket(_t(a), _t(b), None, mode).cpu().numpy(), want, "%s %s" % (mode, grid))
    if grid != (1, 1, 1):
        assert want.any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("lead", [64, 65])                   # floats ahead of out: 16-byte aligned, and 4 bytes past
def test_bracket_writes_nothing_outside_its_output(hip, mode, lead):
    import torch
    grid = (9, 5, 67)
    a, b = _pair(grid, 9)
    n3 = 3 * grid[0] * grid[1] * grid[2]
    sentinel = np.array([0x7fc0beef], np.uint32).view(F32)[0]
    buf = torch.from_numpy(np.full(lead + n3 + 64, sentinel, F32)).cuda()
    out = buf[lead:lead + n3].view((3,) + grid)
    assert out.data_ptr() % 16 == (4 * lead) % 16
    hip.field_bracket(_t(a), _t(b), out, mode)
    got = buf.cpu().numpy()
    _bits(got[lead:lead + n3].reshape((3,) + grid), ld.ref_bracket(a, b, mode), "%s at +%d floats" % (mode, lead))
    for band in (got[:lead], got[lead + n3:]):
        assert (band.view(np.uint32) == 0x7fc0beef).all()


@pytest.mark.parametrize("mode", MODES)
def test_bracket_nan_and_inf_propagate_as_numpy(hip, mode):
    grid = (9, 5, 67)
    a, b = _pair(grid, 13)
    a[0, 4, 2, 30] = np.nan                                  # inside, at a face, and next to a tile's rim
    a[1, 0, 0, 0] = np.inf
    a[2, 8, 4, 66] = -np.inf
    a[1, 3, 3, 63] = np.inf
    b[2, 5, 1, 64] = np.nan
    want = ld.ref_bracket(a, b, mode)
    assert np.isnan(want).any() and np.isfinite(want).any()
    got = hip.field_bracket(_t(a), _t(b), None, mode).cpu().numpy()
    # a NaN's payload and sign are not part of IEEE arithmetic's contract: NaN where the restatement has NaN, bits
    # elsewhere (infinities included)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))


def test_bracket_of_a_field_with_itself(hip):
    a, _ = _pair((9, 5, 67), 17)
    da = _t(a)
    got = hip.field_bracket(da, da, None, "bracket").cpu().numpy()
    _bits(got, ld.ref_bracket(a, a), "[a, a]")
    assert not got.any()


# ---- 2. the signed exponential -----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 1, 3])
def test_signed_exp_bit_exact(hip, K):
    import torch
    nx, ny, nz = SHAPES[0][0]
    v = np.random.default_rng(K).normal(0, 2.0, (3, nz, ny, nx)).astype(F32)
    for negate in (True, False):
        out = torch.full(v.shape, 5.0, device="cuda")
        hip.field_exp(_t(v), out, K, negate=negate)
        _bits(out.cpu().numpy(), ld.ref_exp(v, K, negate), "exp K %d negate %s" % (K, negate))


# ---- 3. the driver -----------------------------------------------------------------------------------------------
def _case(shape, mshape, nc, seed):
    """F, M and a start velocity of about +-1 voxel; through exp(v) some voxels sample outside the moving grid.  On
    one shape (the symmetric cases) the velocity has no component along an axis of one voxel: any other value would
    send every voxel out of the grid, and the run would have no force to test."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    mx, my, mz = mshape
    F = rng.normal(0, 1, (nc, nz, ny, nx)).astype(F32)
    M = rng.normal(0, 1, (nc, mz, my, mx)).astype(F32)
    v = rng.normal(0, 1.0, (3, nz, ny, nx)).astype(F32)
    if shape == mshape:
        for d, n in enumerate(shape):
            if n == 1:
                v[d] = F32(0.0)
    return F, M, v


S0, S1, S2 = SHAPES
# (fixed, moving, nc, sigmas, bch, Kv, symmetric): LOG on test_demons.SHAPES (fixed and moving differ), SYMMETRIC on
# two of the fixed shapes; every value of nc, the sigmas, bch and Kv with LOG and with SYMMETRIC
DRIVER = [(S0[0], S0[1], 1, (0.0, 0.0), 0, 0, 0), (S0[0], S0[1], 3, (1.5, 2.0), 1, 3, 0),
          (S1[0], S1[1], 3, (0.0, 0.0), 1, 0, 0), (S1[0], S1[1], 1, (1.5, 2.0), 0, 3, 0),
          (S2[0], S2[1], 1, (1.5, 2.0), 1, 3, 0), (S2[0], S2[1], 3, (0.0, 0.0), 0, 3, 0),
          (S0[0], S0[0], 1, (1.5, 2.0), 1, 3, 1), (S0[0], S0[0], 3, (0.0, 0.0), 0, 0, 1),
          (S0[0], S0[0], 3, (1.5, 2.0), 0, 3, 1), (S2[0], S2[0], 3, (1.5, 2.0), 1, 0, 1),
          (S2[0], S2[0], 1, (0.0, 0.0), 1, 3, 1)]


@pytest.mark.parametrize("shape,mshape,nc,sigmas,bch,K,sym", DRIVER)
def test_driver_bit_exact_against_restatement(hip, oracle_mod, shape, mshape, nc, sigmas, bch, K, sym):
    F, M, v0 = _case(shape, mshape, nc, 3 + nc + shape[1] + K)
    sf, sdf = sigmas
    vel = _t(v0)
    stats = hip.logdemons([_t(F)], [_t(M)], vel, [3], 0.8, sf, sdf, bool(sym), bch, K)
    s, c = hip.demons_stats(stats)
    want, per = ld.ref_logdemons(F, M, v0, 3, 0.8, sf, sdf, oracle_mod, bool(sym), bch, K)
    _bits(vel.cpu().numpy(), want, "logdemons %s nc %d sigmas %s bch %d K %d sym %d" % (shape, nc, sigmas, bch, K, sym))
    assert len(s) == 3
    for k, (sd, ins) in enumerate(per):
        _check_stats(float(s[k]), int(c[k]), sd, ins, "iteration %d" % k)
        assert 0 < ins.sum()
    assert not np.array_equal(want, v0)


# ---- 4. the pyramid ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sym", [0, 1])
def test_two_levels_bit_exact_against_restatement(hip, oracle_mod, sym):
    shape = S0[0]
    mshape = shape if sym else S0[1]
    F, M, v0 = _case(shape, mshape, 3, 21 + sym)
    Fs, Ms = mr.ref_pyramid(F, 2), mr.ref_pyramid(M, 2)
    args = (0.8, 1.0, 1.5)
    vel = _t(v0)
    stats = hip.logdemons([_t(a) for a in Fs], [_t(a) for a in Ms], vel, [2, 1], *args, bool(sym), 1, 2)
    s, c = hip.demons_stats(stats)
    want, per = ld.ref_logdemons_multires(Fs, Ms, v0, [2, 1], *args, oracle_mod, bool(sym), 1, 2)
    _bits(vel.cpu().numpy(), want, "two levels, symmetric %d" % sym)
    assert len(s) == len(per) == 3
    for k, (sd, ins) in enumerate(per):
        _check_stats(float(s[k]), int(c[k]), sd, ins, "record %d" % k)
    # one level through the pyramid's restatement is the flat run
    one = _t(v0)
    hip.logdemons([_t(F)], [_t(M)], one, [2], *args, bool(sym), 1, 2)
    _bits(one.cpu().numpy(), ld.ref_logdemons_multires([F], [M], v0, [2], *args, oracle_mod, bool(sym), 1, 2)[0],
          "one level")
    _bits(one.cpu().numpy(), ld.ref_logdemons(F, M, v0, 2, *args, oracle_mod, bool(sym), 1, 2)[0], "flat")


# ---- 5. small cases ----------------------------------------------------------------------------------------------
def test_zero_iterations_leave_the_velocity(hip):
    import torch
    F, M, v0 = _case((9, 8, 7), (9, 8, 7), 2, 1)
    for sym in (False, True):
        vel = _t(v0)
        stats = hip.logdemons([_t(F)], [_t(M)], vel, [0], 1.0, 1.0, 1.0, sym, 1, 2)
        torch.cuda.synchronize()
        assert stats.numel() == 0
        _bits(vel.cpu().numpy(), v0, "iterations 0")


@pytest.mark.parametrize("sym", [False, True])
def test_identity_stays_zero(hip, sym):
    import torch
    F = _t(np.random.default_rng(2).normal(0, 1, (2, 11, 10, 9)).astype(F32))
    vel = torch.zeros((3, 11, 10, 9), device="cuda")
    hip.logdemons([F], [F.clone()], vel, [3], 1.0, 1.0, 1.5, sym, 1, 2)
    assert not vel.cpu().numpy().view(np.uint32).any()


def test_non_default_stream_and_repeat_calls(hip):
    import torch
    shape = S0[0]
    F, M, v0 = _case(shape, shape, 3, 5)
    dF, dM = _t(F), _t(M)
    need = hip.lib().sift3d_amd_logdemons_work_floats(shape[0], shape[1], shape[2], 3, 1, 1)
    work = torch.full((need,), float("nan"), device="cuda")              # reused, dirty, scratch
    runs = []
    for _ in range(2):
        vel = _t(v0)
        st = hip.logdemons([dF], [dM], vel, [3], 1.0, 1.5, 2.0, True, 1, 2, work=work)
        runs.append((vel.cpu().numpy(), st.cpu().numpy()))
    np.testing.assert_array_equal(runs[0][0].view(np.uint32), runs[1][0].view(np.uint32))
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(s):
            hip.current_stream(refresh=True)
            dF2, dM2 = dF.clone(), dM.clone()
            vel = _t(v0)
            st = hip.logdemons([dF2], [dM2], vel, [3], 1.0, 1.5, 2.0, True, 1, 2)
            got_v, got_s = vel.clone(), st.clone()
        hip.current_stream(refresh=True)
        torch.cuda.current_stream().wait_stream(s)
        np.testing.assert_array_equal(got_v.cpu().numpy().view(np.uint32), runs[0][0].view(np.uint32))
        np.testing.assert_array_equal(got_s.cpu().numpy(), runs[0][1])
    finally:
        hip.current_stream(refresh=True)


# ---- 6. the api layer --------------------------------------------------------------------------------------------
def _blobs(n, shift, seed):
    """a 40^3-style intensity volume: a dozen Gaussian blobs, their centres moved by `shift` voxels"""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    v = np.zeros((n, n, n))
    for _ in range(12):
        c = rng.uniform(0.2 * n, 0.8 * n, 3) + shift
        v += rng.uniform(50, 100) * np.exp(-((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) / (2 * 4.0 ** 2))
    return v.astype(F32)


@pytest.mark.parametrize("levels", [1, 2])
def test_api_symmetric_is_antisymmetric(hip, levels):
    """refine_field(update="symmetric") with (M, F) and with (F, M): the velocities are each other's negation and the
    field of one is the inverse of the other, bit for bit up to the sign of zeros (0.5f * (x - x) is +0 in both
    runs; tests/test_logdemons_host.py derives it)"""
    from sift3d_amd import api
    fixed, moving = _t(_blobs(40, 0.0, 6)), _t(_blobs(40, np.array([1.5, -1.0, 0.5]), 6))
    kw = dict(features="intensity", update="symmetric", levels=levels, alpha=1.0)
    a = api.refine_field(moving, fixed, None, 5, **kw)
    b = api.refine_field(fixed, moving, None, 5, **kw)
    assert type(a) is (api.LogDemonsRefinement if levels == 1 else api.MultiresLogDemonsRefinement)
    va, vb = a.velocity.cpu().numpy(), b.velocity.cpu().numpy()
    assert np.abs(va).max() > 0.1 and len(a.msd) == 5 * levels and a.msd[-1] < a.msd[0]
    _bits(ld.unsigned_zero(vb), ld.unsigned_zero(-va), "velocities")
    _bits(ld.unsigned_zero(b.field.cpu().numpy()), ld.unsigned_zero(a.inverse.cpu().numpy()), "field / inverse")
    _bits(ld.unsigned_zero(b.inverse.cpu().numpy()), ld.unsigned_zero(a.field.cpu().numpy()), "inverse / field")
    # the members are what they say
    K = api.field_squarings(16.0)
    _bits(a.field.cpu().numpy(), api.field_exp(a.velocity, K).cpu().numpy(), "field")
    _bits(a.inverse.cpu().numpy(), api.field_exp(a.velocity, K, negate=True).cpu().numpy(), "inverse")
    assert a.scaled_max == pytest.approx(float(np.sqrt((va.astype(np.float64) ** 2).sum(0)).max()) * 2.0 ** -K)
    _bits(api.lie_bracket(a.velocity, b.field).cpu().numpy(), ld.ref_bracket(va, b.field.cpu().numpy()), "lie_bracket")
    # the start velocity is honoured and left alone, and too few squarings are reported, not refused
    v0 = a.velocity.clone()
    with pytest.warns(UserWarning, match="exceeds 0.5"):
        c = api.refine_field(moving, fixed, None, 1, velocity=v0 * 8.0, velocity_squarings=0, bch=0, **kw)
    assert c.scaled_max > 0.5
    _bits(v0.cpu().numpy(), va, "the caller's velocity")


# ---- 7. end to end -----------------------------------------------------------------------------------------------
# forward error (median, p90) of the log-domain runs over the diffeomorphic run's, measured on an MI355X (the test's
# docstring); the test allows 1.25 x these for run-to-run and ordering slack, and never more than 2
MEASURED_RATIO = {"logdomain": (1.0087, 1.0006), "symmetric": (1.0086, 1.0081)}


def test_lattice_case_end_to_end():
    """tests/test_demons.py's 176^3 lattice case from zero on three levels, "diffeomorphic" against "logdomain" and
    "symmetric".  The log-domain runs optimise the same force under a stricter parameterisation: they are held to
    the diffeomorphic run's forward error times MEASURED_RATIO x 1.25, must not fold forwards or backwards in the
    inner region, and their exp(-v) must be an inverse as accurate as the forward map (median within 2 x: the factor
    covers the boundary band, where the two grids see different extrapolation).  invert_field's error on the same
    points and the residual of field o inverse are printed, not asserted.  Measured on an MI355X (35937 points,
    50 + 50 + 50 iterations, Kv = 5):
      diffeomorphic: median 0.1322, p90 0.2625 voxel; no folds; msd 0.07668 -> 0.02753
      logdomain:     median 0.1333 (x 1.0087), p90 0.2626 (x 1.0006); no folds in field or inverse; scaled_max 0.3107;
                     inverse error median 0.1639, p90 0.4197 (invert_field on the same field: 0.1618, 0.4193);
                     |field o inverse| mean 0.0139, max 0.0494 voxel; finest level's msd 0.03183 -> 0.02663
      symmetric:     median 0.1333 (x 1.0086), p90 0.2646 (x 1.0081); no folds in field or inverse; scaled_max 0.3104;
                     inverse error median 0.1629, p90 0.4221 (invert_field: 0.1616, 0.4225);
                     |field o inverse| mean 0.0138, max 0.0471 voxel; finest level's msd 0.03170 -> 0.02689"""
    import torch
    from sift3d_amd import api
    n, fixed, moving, known = _lattice_case()
    _, T = _known_deformation(n)
    lo, hi = n // 8, n - n // 8
    inner = (slice(lo, hi),) * 3
    idx = np.arange(lo, hi, 4)
    z, y, x = np.meshgrid(idx, idx, idx, indexing="ij")
    q = np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.float64)
    Tq = T(q)

    def inverse_error(w):
        w = w[:, lo:hi:4, lo:hi:4, lo:hi:4].cpu().numpy().astype(np.float64)
        return np.linalg.norm(Tq - (q + np.stack([w[0].ravel(), w[1].ravel(), w[2].ravel()], 1)), axis=1)

    rd = api.refine_field(moving, fixed, None, levels=3, update="diffeomorphic")
    md, pd, _ = _report("diffeomorphic", known, rd, lo, hi)
    del rd
    failures = []
    for upd in ("logdomain", "symmetric"):
        r = api.refine_field(moving, fixed, None, levels=3, update=upd)
        assert type(r) is api.MultiresLogDemonsRefinement and len(r.msd) == 150
        m, p, inner_fwd = _report(upd, known, r, lo, hi)
        inner_inv = int(np.count_nonzero(~(r.inverse_jacobian.det[inner] > 0).cpu().numpy()))
        err_fwd = composed_error(known, r.field, lo, hi)
        err_inv = inverse_error(r.inverse)
        fp = api.invert_field(r.field, tuple(moving.shape))
        err_fp = inverse_error(fp.field)
        res = torch.sqrt((api.compose_fields(r.field, r.inverse).double() ** 2).sum(0))[inner]
        fine = r.msd[r.level_slices[0]]
        print("%s: forward / diffeomorphic: median ratio %.4f, p90 ratio %.4f; scaled_max %.4f; inverse folded: %d "
              "whole grid, %d inner; inverse error median %.4f p90 %.4f (forward median %.4f); invert_field's: median "
              "%.4f p90 %.4f, residual max %.3g; |field o inverse| mean %.4g max %.4g; finest msd %.5f -> %.5f"
              % (upd, m / md, p / pd, r.scaled_max, r.inverse_jacobian.folded, inner_inv, np.median(err_inv),
                 np.percentile(err_inv, 90), np.median(err_fwd), np.median(err_fp), np.percentile(err_fp, 90),
                 fp.residual_max[-1], float(res.mean()), float(res.max()), fine[0], fine[-1]))
        assert fine[-1] < fine[0]
        assert r.scaled_max <= 0.5
        assert inner_fwd == 0 and inner_inv == 0
        assert np.median(err_inv) <= 2.0 * np.median(err_fwd)
        cap_m, cap_p = (min(2.0, 1.25 * k) for k in MEASURED_RATIO[upd])
        if m / md > cap_m or p / pd > cap_p:
            failures.append((upd, m / md, cap_m, p / pd, cap_p))
        del r, fp, res
    assert not failures, failures


# ---- 8. more than 2^31 elements ----------------------------------------------------------------------------------
def test_bracket_over_2_31_elements_sampled(hip):
    """3 n > 2^31: blocks of rows near the 2^31st element and at the grid's end against the restatement.  A block is
    cut with one more row and plane on every side that is not the grid's own face, and compared without them (the
    restatement's one-sided differences there are the block's, not the grid's)."""
    import torch
    ox, oy, oz = 1024, 1024, 700
    n = ox * oy * oz
    assert 3 * n > 2 ** 31
    g = torch.Generator(device="cuda")
    g.manual_seed(4)
    a = torch.randn((3, oz, oy, ox), device="cuda", generator=g)
    b = torch.randn((3, oz, oy, ox), device="cuda", generator=g)
    out = hip.field_bracket(a, b, None, "bch1")
    z_cross = (2 ** 31 - 2 * n) // (ox * oy)
    blocks = [(z_cross - 1, z_cross + 2, 0, 2), (oz - 2, oz, oy - 3, oy), (z_cross, z_cross + 1, 700, 702)]
    for z0, z1, y0, y1 in blocks:
        za, zb, ya, yb = max(z0 - 1, 0), min(z1 + 1, oz), max(y0 - 1, 0), min(y1 + 1, oy)
        want = ld.ref_bracket(a[:, za:zb, ya:yb, :].cpu().numpy(), b[:, za:zb, ya:yb, :].cpu().numpy(), "bch1")
        want = want[:, z0 - za:z1 - za, y0 - ya:y1 - ya, :]
        _bits(out[:, z0:z1, y0:y1, :].cpu().numpy(), want, "block z %d..%d y %d..%d" % (z0, z1, y0, y1))
