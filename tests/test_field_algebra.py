"""GPU: field composition (sift3d_hip_field_compose), the exponential and the inverse drivers, the diffeomorphic demons
driver and the api layer, against the numpy restatement (tests/field_algebra_restatement.py): fields bit for bit,
counts and max exactly, sums within the bound of any summation order; then end to end on tests/test_demons.py's
case."""
import numpy as np
import pytest

from tests import demons_restatement as dm
from tests import field_algebra_restatement as fa
from tests.test_demons import SHAPES, SIGMAS, _bits, _known_deformation, composed_error, dev_tps, _ncc

pytestmark = pytest.mark.gpu


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


def _check_stats(got, want, what):
    s, m, c, i = got
    ws, wm, wc, wi = want
    assert (int(c), int(i)) == (wc, wi), (what, int(c), int(i), wc, wi)
    assert float(m) == wm, (what, float(m), wm)
    assert abs(float(s) - ws) <= dm.gamma(wc) * ws, (what, float(s), ws)


def _fields(ushape, oshape, seed, nan=False):
    """u on (ux, uy, uz), v on (ox, oy, oz): v scaled so that samples leave u's grid on every side"""
    rng = np.random.default_rng(seed)
    ux, uy, uz = ushape
    ox, oy, oz = oshape
    u = rng.normal(0, 1.5, (3, uz, uy, ux)).astype(np.float32)
    v = rng.normal(0, 1, (3, oz, oy, ox)).astype(np.float32)
    for d, (n, o) in enumerate(zip(ushape, oshape)):
        v[d] = v[d] * np.float32(max(n, o) * 0.4) + np.float32((n - o) / 2.0)
    if nan:
        flat = v.reshape(3, -1)
        idx = rng.choice(flat.shape[1], max(1, flat.shape[1] // 50), replace=False)
        flat[rng.integers(0, 3, idx.size), idx] = np.nan
    return u, v


@pytest.mark.parametrize("mode", ["compose", "invert"])
@pytest.mark.parametrize("shape,mshape", SHAPES + [((31, 41, 19), (37, 29, 23)), ((2, 1, 5), (37, 2, 23))])
def test_compose_bit_exact_against_restatement(hip, shape, mshape, mode):
    import torch
    for nan in (False, True):
        u, v = _fields(mshape, shape, 3 + shape[1] + nan, nan)
        out = torch.full(v.shape, 7.0, device="cuda")
        st = hip.field_compose(_t(u), _t(v), out, mode, stats=True)
        got = hip.field_stats(st)
        want, wst = fa.ref_compose(u, v, mode)
        _bits(out.cpu().numpy(), want, "compose %s / %s %s nan %s" % (shape, mshape, mode, nan))
        _check_stats([g[0] for g in got], wst, "stats")
        assert 0 < wst[3] < wst[2]                              # the clamp path and the inside path
        # stats only, and no stats
        st2 = hip.field_compose(_t(u), _t(v), None, mode, stats=True)
        np.testing.assert_array_equal(st2.cpu().numpy(), st.cpu().numpy())
        out2 = torch.empty_like(out)
        assert hip.field_compose(_t(u), _t(v), out2, mode) is None
        _bits(out2.cpu().numpy(), want, "no stats")
        print("compose %s / %s %s nan %s: sum %.17g ref %.17g max %.9g count %d inside %d"
              % (shape, mshape, mode, nan, got[0][0], wst[0], wst[1], wst[2], wst[3]))


def test_clamp_on_every_side(hip):
    """samples past each of the six faces of u's grid read the nearest edge value"""
    u, v = _fields((9, 8, 7), (12, 11, 10), 5)
    ins_all = []
    for d in range(3):
        for sgn in (-1, 1):
            vv = v.copy()
            vv[d] += np.float32(sgn * 40.0)
            want, wst = fa.ref_compose(u, vv)
            import torch
            out = torch.empty(vv.shape, device="cuda")
            hip.field_compose(_t(u), _t(vv), out, "compose")
            _bits(out.cpu().numpy(), want, "side %d %+d" % (d, sgn))
            ins_all.append(wst[3])
    assert ins_all == [0] * 6


def test_compose_equals_parent_expression_inside(hip):
    """COMPOSE == v + api.warp_field(u, v) bit for bit where the sample is inside"""
    from sift3d_amd import api
    shape, mshape = SHAPES[0]
    u, v = _fields(mshape, shape, 11)
    du, dv = _t(u), _t(v)
    w = api.compose_fields(du, dv).cpu().numpy()
    old = (dv + api.warp_field(du, dv)).cpu().numpy()
    q = [np.arange(n)[idx] for n, idx in zip(v.shape[:0:-1], ((None, None, slice(None)), (None, slice(None), None),
                                                              (slice(None), None, None)))]
    ok = np.ones(v.shape[1:], bool)
    for d, n in enumerate(u.shape[:0:-1]):
        qd = q[d].astype(np.float64) + v[d].astype(np.float64)
        ok &= (qd >= 0) & (qd <= n - 1)
    assert 0 < ok.sum() < ok.size
    _bits(w[:, ok], old[:, ok], "compose vs v + warp_field")


def test_over_2_31_elements_sampled(hip):
    """3 n > 2^31 on the output grid (u small): blocks of rows near the 2^31st element and at the grid's end against
    the restatement (the composition of a voxel reads v at that voxel only), the counts and max of the whole grid"""
    import torch
    ox, oy, oz = 1024, 1024, 700
    n = ox * oy * oz
    assert 3 * n > 2 ** 31
    ushape = (40, 36, 30)
    g = torch.Generator(device="cuda")
    g.manual_seed(4)
    u = torch.randn((3,) + ushape[::-1], device="cuda", generator=g)
    v = (torch.rand((3, oz, oy, ox), device="cuda", generator=g) - 0.5) * 100.0
    out = torch.empty_like(v)
    st = hip.field_compose(u, v, out, "compose", stats=True)
    s, m, c, i = (a[0] for a in hip.field_stats(st))
    z_cross = (2 ** 31 - 2 * n) // (ox * oy)
    un = u.cpu().numpy()
    for z0, z1, y0, y1 in [(z_cross - 1, z_cross + 2, 0, 2), (oz - 2, oz, oy - 3, oy), (z_cross, z_cross + 1, 700, 702)]:
        vb = v[:, z0:z1, y0:y1, :].cpu().numpy()
        want, _ = fa.ref_compose(un, vb, origin=(0, y0, z0))
        _bits(out[:, z0:z1, y0:y1, :].cpu().numpy(), want, "block z %d..%d y %d..%d" % (z0, z1, y0, y1))
    assert int(c) == n
    # inside count and max over the whole grid in torch, float64
    zz, yy, xx = (torch.arange(k, device="cuda", dtype=torch.float64) for k in (oz, oy, ox))
    ok = torch.ones((oz, oy, ox), dtype=torch.bool, device="cuda")
    for d, (p, mm) in enumerate(((xx[None, None, :], ushape[0]), (yy[None, :, None], ushape[1]),
                                 (zz[:, None, None], ushape[2]))):
        q = p + v[d].double()
        ok &= (q >= 0) & (q <= mm - 1)
    assert int(i) == int(ok.sum())
    r = out.double()
    mag = torch.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
    assert float(m) == float(mag.max())
    print("over 2^31: sum %.17g count %d inside %d max %.9g" % (s, c, i, m))


@pytest.mark.parametrize("K", [0, 1, 3])
def test_exp_bit_exact(hip, K):
    import torch
    shape, _ = SHAPES[0]
    rng = np.random.default_rng(K)
    nx, ny, nz = shape
    v = (rng.normal(0, 2.0, (3, nz, ny, nx))).astype(np.float32)
    out = torch.full(v.shape, 5.0, device="cuda")
    hip.field_exp(_t(v), out, K)
    _bits(out.cpu().numpy(), fa.ref_exp(v, K), "exp K %d" % K)


@pytest.mark.parametrize("N", [0, 1, 5])
@pytest.mark.parametrize("init", ["zero", "random"])
def test_invert_bit_exact(hip, N, init):
    shape, mshape = SHAPES[0]
    u, _ = _fields(mshape, shape, 9)
    u = (u * np.float32(0.3)).astype(np.float32)
    rng = np.random.default_rng(N)
    w0 = np.zeros((3,) + mshape[::-1], np.float32) if init == "zero" else \
        rng.normal(0, 1, (3,) + mshape[::-1]).astype(np.float32)
    w = _t(w0)
    st = hip.field_invert(_t(u), w, N)
    got = hip.field_stats(st)
    want, recs = fa.ref_invert(u, w0, N)
    _bits(w.cpu().numpy(), want, "invert N %d %s" % (N, init))
    assert len(got[0]) == N + 1
    for k, r in enumerate(recs):
        _check_stats([g[k] for g in got], r, "record %d" % k)


def test_non_default_stream_and_repeat_calls(hip):
    import torch
    shape, mshape = SHAPES[0]
    u, v = _fields(mshape, shape, 21)
    du, dv = _t(u), _t(v)
    runs = []
    for _ in range(2):
        w = torch.zeros((3,) + mshape[::-1], device="cuda")
        st = hip.field_invert(du, w, 4)
        e = torch.empty_like(dv)
        hip.field_exp(dv, e, 3)
        runs.append((w.cpu().numpy(), st.cpu().numpy(), e.cpu().numpy()))
    for a, b in zip(runs[0], runs[1]):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    big = torch.ones((256, 512, 512), device="cuda")
    du2, dv2 = torch.zeros_like(du), torch.zeros_like(dv)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    try:
        with torch.cuda.stream(s):
            hip.current_stream(refresh=True)
            for _ in range(20):
                big.mul_(1.0001)
            du2.copy_(du)
            dv2.copy_(dv)
            w = torch.zeros((3,) + mshape[::-1], device="cuda")
            st = hip.field_invert(du2, w, 4)
            e = torch.empty_like(dv2)
            hip.field_exp(dv2, e, 3)
            got = (w.clone(), st.clone(), e.clone())
        hip.current_stream(refresh=True)
        torch.cuda.current_stream().wait_stream(s)
        for a, b in zip(got, runs[0]):
            np.testing.assert_array_equal(a.cpu().numpy().view(np.uint8), b.view(np.uint8))
    finally:
        hip.current_stream(refresh=True)


def _demons_case(shape, mshape, nc, seed):
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    mx, my, mz = mshape
    F = rng.normal(0, 1, (nc, nz, ny, nx)).astype(np.float32)
    M = rng.normal(0, 1, (nc, mz, my, mx)).astype(np.float32)
    u = rng.normal(0, 1.5, (3, nz, ny, nx)).astype(np.float32)
    u[0] += np.float32(2.0)
    u[1] += np.float32(3.0)
    return F, M, u


@pytest.mark.parametrize("K", [0, 2])
@pytest.mark.parametrize("sigmas", SIGMAS)
@pytest.mark.parametrize("nc", [1, 3, 12])
@pytest.mark.parametrize("shape,mshape", SHAPES)
def test_diffeomorphic_driver_bit_exact(hip, oracle_mod, shape, mshape, nc, sigmas, K):
    F, M, u = _demons_case(shape, mshape, nc, 7 + nc + shape[1])
    sf, sdf = sigmas
    field = _t(u)
    stats = hip.demons(_t(F), _t(M), field, 3, 0.8, sf, sdf, update="diffeomorphic", squarings=K)
    s, c = hip.demons_stats(stats)
    want, per = fa.ref_demons_diffeo(F, M, u, 3, 0.8, sf, sdf, K, oracle_mod)
    _bits(field.cpu().numpy(), want, "diffeomorphic %s nc %d sigmas %s K %d" % (shape, nc, sigmas, K))
    assert len(s) == 3
    for k, (sd, ins) in enumerate(per):
        ws, wc = dm.ref_stats(sd, ins)
        assert int(c[k]) == wc
        assert abs(float(s[k]) - ws) <= dm.gamma(wc) * ws


def test_ex_additive_equals_demons_device(hip):
    import torch
    shape, mshape = SHAPES[0]
    F, M, u = _demons_case(shape, mshape, 3, 2)
    dF, dM = _t(F), _t(M)
    L = hip.lib()
    nx, ny, nz = shape
    mx, my, mz = mshape
    need = L.sift3d_amd_demons_work_floats_ex(nx, ny, nz, 3, 0)
    res = []
    for ex in (False, True):
        field = _t(u)
        work = torch.empty(need, dtype=torch.float32, device="cuda")
        stats = torch.empty(4 * 2, dtype=torch.int64, device="cuda")
        args = [dF.data_ptr(), nx, ny, nz, dM.data_ptr(), mx, my, mz, 3, field.data_ptr(), 4, 0.8, 1.5, 2.0]
        if ex:
            rc = L.sift3d_amd_demons_device_ex(*args, 0, 0, work.data_ptr(), stats.data_ptr(), hip.current_stream())
        else:
            rc = L.sift3d_amd_demons_device(*args, work.data_ptr(), stats.data_ptr(), hip.current_stream())
        assert rc == 0
        res.append((field.cpu().numpy(), stats.cpu().numpy()))
    np.testing.assert_array_equal(res[0][0].view(np.uint32), res[1][0].view(np.uint32))
    np.testing.assert_array_equal(res[0][1], res[1][1])


def test_folding_case_pinned(hip):
    """the CPU test's case (tests/test_field_algebra_host.fold_case) on the device: both fields bit for bit against
    the restatements' and the pinned fold counts"""
    import torch
    from sift3d_amd import api
    from tests.test_field_algebra_host import FOLDS_ADDITIVE, FOLDS_DIFFEOMORPHIC, fold_case
    F, M, kw = fold_case()
    dF, dM = _t(F), _t(M)
    got = []
    for upd in ("additive", "diffeomorphic"):
        r = api.refine_field(dM, dF, None, kw["iterations"], kw["alpha"], kw["sigma_fluid"], kw["sigma_diffusion"],
                             "intensity", update=upd)
        got.append(r.jacobian.folded)
    torch.cuda.synchronize()
    print("folding case on the device: additive %d, diffeomorphic %d" % tuple(got))
    assert got == [FOLDS_ADDITIVE, FOLDS_DIFFEOMORPHIC]


# ---- end to end: tests/test_demons.py's case -----------------------------------------------------------------
def test_register_dense_diffeomorphic_and_inverse():
    import torch
    from sift3d_amd import api, hip
    n = 176
    fixed = torch.empty((n, n, n), device="cuda")
    hip.synth_lattice(fixed, 0, 21)
    known, T = _known_deformation(n)
    moving = dev_tps(fixed, known, fixed.shape)
    torch.cuda.synchronize()
    spl = api.register_deformable(moving, fixed)
    res = api.register_dense(moving, fixed, update="diffeomorphic")
    lo, hi = n // 8, n - n // 8
    u_s = api.displacement_field(spl.tps, fixed.shape)
    err_s = composed_error(known, u_s, lo, hi)
    err_d = composed_error(known, res.field, lo, hi)
    f = fixed.cpu().numpy()[lo:hi, lo:hi, lo:hi]
    ncc_s = _ncc(spl.warped.cpu().numpy()[lo:hi, lo:hi, lo:hi], f)
    ncc_d = _ncc(res.warped.cpu().numpy()[lo:hi, lo:hi, lo:hi], f)
    det = res.jacobian.det.cpu().numpy()
    inner_folded = int(np.count_nonzero(~(det[lo:hi, lo:hi, lo:hi] > 0)))
    print("register_dense diffeomorphic: spline median %.4f p90 %.4f NCC %.5f; refined median %.4f p90 %.4f NCC "
          "%.5f; folded %d whole grid, %d inner; msd %.5f -> %.5f"
          % (np.median(err_s), np.percentile(err_s, 90), ncc_s, np.median(err_d), np.percentile(err_d, 90), ncc_d,
             res.jacobian.folded, inner_folded, res.msd[0], res.msd[-1]))
    assert np.median(err_d) < np.median(err_s)
    assert np.percentile(err_d, 90) <= np.percentile(err_s, 90)
    assert ncc_d >= ncc_s
    assert inner_folded == 0
    assert res.msd[-1] < res.msd[0]
    # the inverse: moving -> fixed on the moving grid
    L = fa.lipschitz(res.field.cpu().numpy())
    print("Lipschitz constant of the field: %.4f" % L)
    assert L < 1
    inv = api.invert_field(res.field, tuple(moving.shape))
    U = float(torch.sqrt((res.field.double() ** 2).sum(0)).max())
    rho = 8 * 2.0 ** -24 * (U + 1)
    r0 = float(inv.residual_max[0])
    for k, rm in enumerate(inv.residual_max):
        bound = np.sqrt(3.0) * (L ** k * r0 + 2 * rho / (1 - L))
        assert rm <= bound, (k, rm, bound)
    idx = np.arange(lo, hi, 4)
    z, y, x = np.meshgrid(idx, idx, idx, indexing="ij")
    q = np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.float64)
    w = inv.field[:, lo:hi:4, lo:hi:4, lo:hi:4].cpu().numpy().astype(np.float64)
    qw = q + np.stack([w[0].ravel(), w[1].ravel(), w[2].ravel()], 1)
    Tq = T(q)
    err_inv = np.linalg.norm(Tq - qw, axis=1)
    Aq = q @ np.asarray(res.A)[:, :3].T + np.asarray(res.A)[:, 3]
    err_aff = np.linalg.norm(Tq - Aq, axis=1)
    print("inverse: median %.4f p90 %.4f (affine median %.4f p90 %.4f); forward median %.4f p90 %.4f; residual max "
          "%.3g mean %.3g; L %.4f"
          % (np.median(err_inv), np.percentile(err_inv, 90), np.median(err_aff), np.percentile(err_aff, 90),
             np.median(err_d), np.percentile(err_d, 90), inv.residual_max[-1], inv.residual_mean[-1], L))
    assert np.median(err_inv) < np.median(err_aff)
