"""CPU (not gpu): the host side of field composition, the exponential, the inverse and the diffeomorphic demons
driver -- every refusal of the new entries (checked before any device call), the exported symbols, the work
sizes -- and the numpy restatement (tests/field_algebra_restatement.py) against analysis: affine composition,
the exponential of constant and linear fields, the inverse of an affine field, and a case where additive demons
folds and the diffeomorphic update does not."""
import math

import numpy as np
import pytest

from tests import demons_restatement as dm
from tests import field_algebra_restatement as fa
from tests import field_restatement as fr
from tests.test_warp import ref_coords, rot

U24 = 2.0 ** -24                                  # float32's unit roundoff


@pytest.fixture(scope="module")
def api():
    from sift3d_amd import api as a
    a.lib()
    return a


@pytest.fixture(scope="module")
def bufs(api):
    """made-up addresses without a device; real allocations covering every range named below with one, so that a
    regressed check could not make a kernel touch unmapped memory"""
    from sift3d_amd import hip
    if api.device_available():
        b = [hip.lib().sift3d_hip_malloc(1 << 18) for _ in range(3)]
        assert all(b)
        yield b
        for p in b:
            hip.lib().sift3d_hip_free(p)
    else:
        yield [0x1000000, 0x2000000, 0x3000000]


EXPORTED = ["sift3d_hip_field_compose", "sift3d_amd_field_exp_work_floats", "sift3d_amd_field_exp_device",
            "sift3d_amd_field_invert_work_floats", "sift3d_amd_field_invert_device", "sift3d_amd_demons_work_floats_ex",
            "sift3d_amd_demons_device_ex"]


def test_symbols_exported(api):
    from sift3d_amd import _native, hip
    L = _native.load()
    for name in EXPORTED:
        assert hasattr(L, name), name
    hip.lib()
    for name in ("field_compose", "field_exp", "field_invert", "field_stats", "demons"):
        assert callable(getattr(hip, name))
    for name in ("compose_fields", "field_exp", "invert_field", "refine_field", "register_dense"):
        assert callable(getattr(api, name))
    assert api.FieldInverse._fields == ("field", "residual_max", "residual_mean", "inside")
    assert api.INVERT_ITERATIONS == 28 and 0.6 ** api.INVERT_ITERATIONS <= 1e-6


def test_work_floats(api):
    from sift3d_amd import hip
    L = hip.lib()
    part = 32768 // 4
    n = 37 * 29 * 23
    assert L.sift3d_amd_demons_work_floats_ex(37, 29, 23, 12, 0) == L.sift3d_amd_demons_work_floats(37, 29, 23, 12)
    assert L.sift3d_amd_demons_work_floats_ex(37, 29, 23, 12, 0) == part + 17 * n
    assert L.sift3d_amd_demons_work_floats_ex(37, 29, 23, 12, 1) == part + 23 * n
    assert L.sift3d_amd_demons_work_floats_ex(8, 8, 8, 1, 1) == part + 12 * 512
    assert L.sift3d_amd_demons_work_floats_ex(8, 8, 8, 1, 2) == 0
    assert L.sift3d_amd_demons_work_floats_ex(8, 8, 8, 1, -1) == 0
    assert L.sift3d_amd_demons_work_floats_ex(0, 8, 8, 1, 1) == 0
    assert L.sift3d_amd_field_exp_work_floats(37, 29, 23) == 3 * n
    assert L.sift3d_amd_field_invert_work_floats(37, 29, 23) == 65536 // 4 + 3 * n
    for a in ((0, 8, 8), (8, -1, 8), (8, 8, 0)):
        assert L.sift3d_amd_field_exp_work_floats(*a) == 0
        assert L.sift3d_amd_field_invert_work_floats(*a) == 0


# 8^3 fields: 6144 bytes each
FB = 3 * 512 * 4


def _cmp(L, a):
    return L.sift3d_hip_field_compose(a["u"], a["ux"], a["uy"], a["uz"], a["v"], a["ox"], a["oy"], a["oz"], a["out"],
                                      a["mode"], a["stats"], a["work"], None)


def test_compose_refusals(bufs):
    from sift3d_amd import hip
    L = hip.lib()
    A, B, W = bufs
    base = dict(u=A, ux=8, uy=8, uz=8, v=A + 8192, ox=8, oy=8, oz=8, out=B, mode=0, stats=B + 8192, work=W)
    changes = [
        dict(u=None), dict(v=None), dict(out=None, stats=None), dict(work=None),
        dict(ux=0), dict(uy=-1), dict(uz=0), dict(ox=0), dict(oy=-2), dict(oz=0),
        dict(mode=2), dict(mode=-1),
        dict(stats=B + 8196), dict(work=W + 4),                            # 8-byte alignment
        dict(u=A + 2), dict(v=A + 8193), dict(out=B + 1),
        dict(out=A + 8192),                                                # in place: out == v
        dict(out=A + 8192 + 4 * 100),                                      # out inside v
        dict(out=A + 4 * 1000),                                            # out runs into u ... and v
        dict(out=A),                                                       # out == u
        dict(stats=A + 64),                                                # stats inside u
        dict(stats=B + FB - 8),                                            # stats inside out
        dict(work=B + 4 * 100),                                            # the partials over out
        dict(work=A + 8192),                                               # the partials over v
        dict(stats=W + 65536 - 8),                                         # stats inside the partials
        dict(ox=16, out=B, stats=B + 2 * FB - 16),                         # stats inside a larger out
    ]
    for ch in changes:
        a = dict(base)
        a.update(ch)
        assert _cmp(L, a) == -1, ch
    # out NULL (stats only) and stats NULL (then work may be NULL too) are allowed; bad arguments are still refused
    for ch in (dict(out=None, mode=3), dict(stats=None, work=None, ux=0), dict(stats=None, work=None, out=A)):
        a = dict(base)
        a.update(ch)
        assert _cmp(L, a) == -1, ch


def test_exp_refusals(bufs):
    from sift3d_amd import hip
    L = hip.lib()
    A, B, W = bufs

    def run(**ch):
        a = dict(v=A, ox=8, oy=8, oz=8, K=2, out=B, work=W)
        a.update(ch)
        return L.sift3d_amd_field_exp_device(a["v"], a["ox"], a["oy"], a["oz"], a["K"], a["out"], a["work"], None)

    for ch in (dict(v=None), dict(out=None), dict(work=None), dict(ox=0), dict(oy=-1), dict(oz=0),
               dict(K=-1), dict(K=21), dict(K=1 << 30), dict(v=A + 2), dict(out=B + 1), dict(work=W + 4),
               dict(out=A), dict(out=A + 4 * 1535), dict(work=A + 4 * 100), dict(work=B + 4 * 1000),
               dict(work=B - 4 * 1000)):
        assert run(**ch) == -1, ch


def test_invert_refusals(bufs):
    from sift3d_amd import hip
    L = hip.lib()
    A, B, W = bufs

    def run(**ch):
        a = dict(u=A, ux=8, uy=8, uz=8, w=B, ox=8, oy=8, oz=8, N=3, work=W, stats=B + 8192)
        a.update(ch)
        return L.sift3d_amd_field_invert_device(a["u"], a["ux"], a["uy"], a["uz"], a["w"], a["ox"], a["oy"], a["oz"],
                                                a["N"], a["work"], a["stats"], None)

    for ch in (dict(u=None), dict(w=None), dict(work=None), dict(stats=None), dict(ux=0), dict(uy=-1), dict(uz=0),
               dict(ox=0), dict(oy=-3), dict(oz=0), dict(N=-1), dict(u=A + 2), dict(w=B + 1), dict(work=W + 4),
               dict(stats=B + 8196),
               dict(w=A + 4 * 100),                                         # w inside u
               dict(work=A + 4 * 1000),                                     # the work buffer over u
               dict(work=B - 4 * 100),                                      # the work buffer runs into w
               dict(stats=B + FB - 8),                                      # stats inside w
               dict(stats=W + 65536 + 4 * 100),                             # stats inside the second iterate
               dict(N=40, stats=A - 40 * 32)):                              # the 41 records run into u
        assert run(**ch) == -1, ch


def _drv_args(bufs):
    """F and M in buffer 0, u and stats in 1, the work buffer in 2 (8^3, nc = 1: 17408 floats diffeomorphic)"""
    A, B, W = bufs
    return dict(F=A, nx=8, ny=8, nz=8, M=A + 8192, mx=8, my=8, mz=8, nc=1, u=B, it=3, alpha=1.0, sf=1.0, sd=1.0,
                upd=1, K=2, work=W, stats=B + 8192)


def _drv(L, a):
    return L.sift3d_amd_demons_device_ex(a["F"], a["nx"], a["ny"], a["nz"], a["M"], a["mx"], a["my"], a["mz"],
                                         a["nc"], a["u"], a["it"], a["alpha"], a["sf"], a["sd"], a["upd"], a["K"],
                                         a["work"], a["stats"], None)


@pytest.mark.parametrize("upd", [0, 1])
def test_demons_ex_refusals(bufs, upd):
    from sift3d_amd import hip
    L = hip.lib()
    base = _drv_args(bufs)
    base["upd"] = upd
    A, B, W = bufs
    work = 4 * L.sift3d_amd_demons_work_floats_ex(8, 8, 8, 1, upd)
    changes = [
        dict(upd=2), dict(upd=-1), dict(K=-1), dict(K=21),
        dict(F=None), dict(M=None), dict(u=None), dict(work=None), dict(stats=None),
        dict(nx=0), dict(ny=-2), dict(nz=0), dict(mx=-1), dict(my=0), dict(mz=0),
        dict(nc=0), dict(it=-1),
        dict(alpha=0.0), dict(alpha=float("nan")), dict(sf=-0.1), dict(sd=float("inf")),
        dict(stats=B + 8196), dict(work=W + 4), dict(F=A + 2), dict(M=A + 8193), dict(u=B + 2),
        dict(u=A + 4 * 300), dict(u=W + 4 * 9000), dict(stats=B + 4 * 1000), dict(work=B),
        dict(stats=W + work - 16),                                         # stats inside the work buffer's end
    ]
    for ch in changes:
        a = dict(base)
        a.update(ch)
        assert _drv(L, a) == -1, ch


def test_python_refusals(api):
    vol = np.zeros((3, 5, 6, 7), np.float32)
    for call in (lambda: api.compose_fields(vol, vol), lambda: api.field_exp(vol),
                 lambda: api.invert_field(vol, (5, 6, 7))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        api.refine_field(vol[0], vol[0], update="diffeomorphic")
    assert api.demons_squarings(2.0) == 0 and api.demons_squarings(1.0) == 0
    assert api.demons_squarings(0.25) == 2 and api.demons_squarings(0.3) == 2 and api.demons_squarings(0.5) == 1
    assert api.field_squarings(0.5) == 0 and api.field_squarings(0.51) == 1 and api.field_squarings(4.0) == 3


# ---- the restatement against analysis -------------------------------------------------------------------------
def _affine(M, t):
    A = np.zeros((3, 4))
    A[:, :3] = M
    A[:, 3] = t
    return A


def _apply(A, x, y, z):
    return ref_coords(A, x, y, z)


def test_compose_of_affine_fields():
    """u = the field of A on u's grid, v = the field of B on the output grid: on voxels whose sample is inside, w =
    COMPOSE(u, v) is the field of A o B but for rounding.  Trilinear interpolation reproduces an affine function
    exactly, so the error is rounding alone.  With U = max|u|, V = max|v|, D = the largest difference of u across
    a grid edge, L = u's Lipschitz constant:
      - u and v are rounded once to float: 2^-24 U in the corner values, 2^-24 V in the sample point, which moves
        the sample by at most L 2^-24 V;
      - each of the 3 lerp levels a + f (b - a): b - a, f (b - a) and the sum round (2^-24 D, 2^-24 D, 2^-24 (U +
        D)), the fraction f = (float)(q - floor q) rounds (2^-24 D); the weights 1 - f, f sum to 1, so corner
        errors do not grow: 3 levels give 2^-24 (3 U + 12 D);
      - w = v + s rounds once: 2^-24 (V + U).
    So |w - w_true| <= 2^-24 (5 U + 12 D + (2 + L) V) per component."""
    ushape, oshape = (23, 19, 17), (21, 25, 15)
    A = _affine(rot((1, 2, 3), 7.0) * 1.03, (1.5, -2.0, 0.7))
    B = _affine(rot((-1, 0.5, 2), 5.0) * 0.98, (-1.0, 1.2, 0.3))
    u = fr.ref_affine_field(A, ushape)
    v = fr.ref_affine_field(B, oshape)
    w, (_, _, cnt, ins_n) = fa.ref_compose(u, v)
    x, y, z = fr.grid(oshape)
    q = _apply(B, x, y, z)
    ins = np.ones(q[0].shape, bool)
    for qd, n in zip(q, ushape[::-1]):
        ins &= (qd >= 1e-9) & (qd <= n - 1 - 1e-9)
    r = _apply(A, *q)
    want = [rd - pd.astype(np.float64) for rd, pd in zip(r, (x, y, z))]
    U, V = float(np.abs(u).max()), float(np.abs(v).max())
    L = fa.lipschitz(u)
    D = L
    bound = U24 * (5 * U + 12 * D + (2 + L) * V)
    err = max(float(np.abs(w[d].astype(np.float64) - want[d])[ins].max()) for d in range(3))
    print("compose affine: err %.3g bound %.3g (U %.3g V %.3g L %.3g) on %d voxels" % (err, bound, U, V, L, ins.sum()))
    assert ins.sum() > 1000 and cnt == w[0].size and 0 < ins_n < cnt
    assert err <= bound


@pytest.mark.parametrize("K", [0, 1, 3, 6])
def test_exp_of_constant_field_is_exact(K):
    """v = c constant: w_0 = c 2^-K is exact (a power of two), trilinear interpolation of a constant is the
    constant (a + f (a - a) = a, also where the sample is clamped), and w_k + w_k = 2 w_k is exact: exp(v) = c"""
    c = np.array([3.25, -11.5, 0.7], np.float32)
    v = np.broadcast_to(c[:, None, None, None], (3, 9, 7, 11)).astype(np.float32)
    got = fa.ref_exp(v, K)
    assert np.array_equal(got.view(np.uint32), v.view(np.uint32))


@pytest.mark.parametrize("K", [1, 3, 5])
def test_exp_of_linear_field(K):
    """v(p) = B (p - c), c the grid's centre, I + B a contraction of the infinity norm: every exact iterate maps
    the grid's box into itself, so every sample point of the exact chain is inside, and the clamp (1-Lipschitz
    toward a point inside) cannot increase an error.  Exactly, w_k(p) = ((I + B 2^-K)^(2^k) - I)(p - c).  The error
    recursion per squaring, e_k = max |w_k - exact| per component:
      e_{k+1} <= e_k (the v term) + L_k e_k (the sample point moves) + e_k (the corner values; weights sum to 1)
                 + rho_k = (2 + L_k) e_k + rho_k,
    with L_k the Lipschitz constant of the exact w_k and rho_k one composition's rounding bound (test above, U =
    V = max|w_k|, D = L_k): rho_k = 2^-24 (5 U + 12 L_k + (2 + L_k) U).  e_0 = 2^-24 max|v| 2^-K (v rounded once,
    the scaling exact)."""
    shape = (15, 13, 17)
    B = np.array([[-0.12, 0.03, -0.02], [-0.04, -0.15, 0.02], [0.01, -0.03, -0.10]])
    Mk = np.eye(3) + B / 2.0 ** K
    assert np.abs(Mk).sum(1).max() <= 1.0
    x, y, z = fr.grid(shape)
    cen = (np.array(shape[::-1], np.float64) - 1) / 2
    P = np.stack([x - cen[0], y - cen[1], z - cen[2]]).reshape(3, -1).astype(np.float64)
    v = (B @ P).reshape((3,) + shape).astype(np.float32)
    got = fa.ref_exp(v, K).astype(np.float64)
    e = U24 * float(np.abs(v).max()) * 2.0 ** -K
    for k in range(K):
        Wk = np.linalg.matrix_power(Mk, 2 ** k) - np.eye(3)
        Lk = float(np.abs(Wk).sum(1).max())
        Uk = float(np.abs(Wk @ P).max())
        rho = U24 * (5 * Uk + 12 * Lk + (2 + Lk) * Uk)
        e = (2 + Lk) * e + rho
    want = ((np.linalg.matrix_power(Mk, 2 ** K) - np.eye(3)) @ P).reshape((3,) + shape)
    err = float(np.abs(got - want).max())
    print("exp linear K %d: err %.3g bound %.3g" % (K, err, e))
    assert err <= e


def test_inverse_of_affine_field():
    """u = the field of A (fixed -> moving) on the fixed grid; the inverse w on the moving grid should be the field
    of A^-1 (api.affine_invert) on moving voxels whose true preimage is inside the fixed grid.  The step T(w)(q) =
    -u(q + w(q)) is a contraction of the infinity norm with factor L (u's Lipschitz constant; the clamp is
    1-Lipschitz), and w* = T(w*) where the preimage is inside.  From w_0 = 0, |w_0 - w*| = |w*| <= max|u|, so
      |w_N - w*| <= L^N max|u| / (1 - L) + rho / (1 - L),
    rho one INVERT step's rounding: by the composition bound 2^-24 (5 U + 12 L + (1 + L) |w|) with |w| <= U / (1 -
    L) <= 1.43 U at L <= 0.3: at most 2^-24 (7 U + 4) <= c 2^-24 (U + 1) with c = 7; c = 8 here, one more for the
    float64 reference and the double sample point."""
    from sift3d_amd import api
    fshape, mshape = (21, 19, 23), (19, 22, 20)
    A = _affine(np.eye(3) + np.array([[0.06, -0.05, 0.03], [0.04, 0.05, -0.02], [-0.03, 0.02, -0.06]]),
                (2.0, -1.5, 1.0))
    u = fr.ref_affine_field(A, fshape)
    L = fa.lipschitz(u)
    assert L <= 0.3, L
    U = float(np.abs(u).max())
    N = 12
    w, recs = fa.ref_invert(u, np.zeros((3,) + mshape, np.float32), N)
    Ai = api.affine_invert(A)
    x, y, z = fr.grid(mshape)
    pre = _apply(Ai, x, y, z)
    ok = np.ones(x.shape, bool)
    for qd, n in zip(pre, fshape[::-1]):
        ok &= (qd >= 0) & (qd <= n - 1)
    want = [pd - qd.astype(np.float64) for pd, qd in zip(pre, (x, y, z))]
    err = max(float(np.abs(w[d].astype(np.float64) - want[d])[ok].max()) for d in range(3))
    c = 8
    bound = L ** N * U / (1 - L) + c * U24 * (U + 1) / (1 - L)
    print("invert affine: L %.3f err %.3g bound %.3g, residual max %s" % (L, err, bound, [r[1] for r in recs]))
    assert ok.sum() > 1000 and err <= bound
    assert len(recs) == N + 1


# ---- a case where additive demons folds and the diffeomorphic update does not ----------------------------------
def fold_case():
    """24^3 intensity volumes: fixed = Gaussian-blurred noise (sigma 1.5, peak 100), moving = fixed pulled through a
    smooth random displacement (sigma 4, peak 5 voxels); alpha 0.25 (K = 2), sigma_fluid 1, no diffusion blur, 5
    iterations from zero"""
    from oracle import sift3d_oracle as so
    n = 24
    rng = np.random.default_rng(2)
    noise = rng.normal(0, 1, (n, n, n)).astype(np.float32)
    F = so.blur(noise, so.gauss_taps(1.5), (1, 1, 1), unit=1.0).astype(np.float32)
    F = (F / np.abs(F).max() * 100).astype(np.float32)
    d = np.stack([so.blur(rng.normal(0, 1, (n, n, n)).astype(np.float32), so.gauss_taps(4.0), (1, 1, 1), unit=1.0)
                  for _ in range(3)])
    d = (d / np.abs(d).max() * 5.0).astype(np.float32)
    M = fr.ref_warp_field(F, d, "linear", 0.0)
    return F, M, dict(iterations=5, alpha=0.25, sigma_fluid=1.0, sigma_diffusion=0.0, squarings=2)


# Found by a search over seeds 1-2, displacement peaks 3 / 5, noise sigma 1.5 / 2.5 and sigma_fluid 0 / 1 / 2 (5
# iterations, alpha 0.25, K = 2): without the fluid blur both fold (the raw force is rough, so exp(delta) is not
# invertible either); with sigma_fluid 2 neither does; with sigma_fluid 1 additive folds in all 8 cases (7 .. 551
# voxels) and diffeomorphic in one (3 voxels).  This is the case with the most additive folds and none diffeomorphic.
FOLDS_ADDITIVE = 551
FOLDS_DIFFEOMORPHIC = 0


def test_folding_case(oracle_mod):
    F, M, kw = fold_case()
    u0 = np.zeros((3,) + F.shape, np.float32)
    ua, _ = dm.ref_demons(F, M, u0, kw["iterations"], kw["alpha"], kw["sigma_fluid"], kw["sigma_diffusion"], oracle_mod)
    ud, _ = fa.ref_demons_diffeo(F, M, u0, kw["iterations"], kw["alpha"], kw["sigma_fluid"], kw["sigma_diffusion"],
                                 kw["squarings"], oracle_mod)
    fa_ = fr.ref_stats(fr.ref_jacobian_det(ua))[0]
    fd = fr.ref_stats(fr.ref_jacobian_det(ud))[0]
    print("folding case: additive %d, diffeomorphic %d" % (fa_, fd))
    assert math.ceil(math.log2(1 / kw["alpha"])) == kw["squarings"]
    assert (fa_, fd) == (FOLDS_ADDITIVE, FOLDS_DIFFEOMORPHIC)
