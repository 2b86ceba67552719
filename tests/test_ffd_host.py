"""The free-form deformation contract without a device (include/sift3d_amd.h, "B-spline free-form deformation"): the
restatement (tests/ffd_restatement.py) against analysis, the host entries, every refusal of every device entry before
any device call, the exported symbols and layouts, and the restatement's driver on the pair the device test uses."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import ffd_restatement as fr
from tests.demons_restatement import gamma
from tests.field_restatement import ref_warp_field
from tests.test_affine_refine_host import gaussians

U = 2.0 ** -53
U32 = 2.0 ** -24


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


# ---- the restatement against analysis ----------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [1, 2, 3, 7, 8, 50, 256])
def test_weight_table(hip, delta):
    w = fr.weights(delta)
    assert np.array_equal(w, hip.ffd_weights(delta))                     # the host entry, bit for bit
    assert np.array_equal(w[0], np.array([1 / 6, 4 / 6, 1 / 6, 0], np.float64).astype(np.float32))
    s = w.astype(np.float64).sum(axis=1)
    assert np.all(np.abs(s - 1.0) <= 2 * U32)                            # 2 ulp of 1 in float32
    assert np.all(w >= 0) and np.array_equal(w[1:, 0], w[1:, 3][::-1]) and np.array_equal(w[1:, 1], w[1:, 2][::-1])


def affine_lattice(out_shape, spacing, L, t):
    """the lattice sampled from the affine function c_d(pos) = L[d] . pos + t[d] at the controls' positions"""
    shape = fr.lattice_shape(out_shape, spacing)
    d = fr.spacing3(spacing)
    pos = [(np.arange(g) - 1.0) * dd for g, dd in zip(shape[:0:-1], d)]  # x, y, z
    z, y, x = np.meshgrid(pos[2], pos[1], pos[0], indexing="ij")
    return np.stack([L[k][0] * x + L[k][1] * y + L[k][2] * z + t[k] for k in range(3)])


def test_affine_lattice_reproduces_the_affine_function():
    """Cubic B-splines reproduce polynomials of degree <= 3 sampled at the knots, so the exact spline of an affine
    lattice is the affine function.  The float32 sum has 64 terms of three multiplications each: every term carries
    3 roundings and the running sum 63 more, so |s - exact| <= gamma32_(66) * sum |terms| <= 67 u32 * max |c| (the
    weights are non-negative and sum to 1 within 2 u32 per axis), plus the rounding of the lattice itself to float32
    (u32 max |c|) and of the weights (u32 each, three per term): 72 u32 max |c| in all."""
    out_shape, spacing = (9, 14, 21), (4, 3, 2)
    L = [[0.01, -0.02, 0.005], [0.0, 0.03, -0.01], [-0.015, 0.0, 0.02]]
    t = [0.5, -1.25, 2.0]
    c = affine_lattice(out_shape, spacing, L, t)
    s = fr.spline(c.astype(np.float32), spacing, out_shape).astype(np.float64)
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in out_shape), indexing="ij")
    want = np.stack([L[k][0] * x + L[k][1] * y + L[k][2] * z + t[k] for k in range(3)])
    assert np.abs(s - want).max() <= 72 * U32 * np.abs(c).max()


def test_adjoint_identity():
    """<Phi c, v> = <c, Phi^T v> in float64: both sides are sums of the same products W c v up to rounding; each
    side's error is within gamma_(64 + n) of sum |W c v| <= sum |c| . Phi^T |v|"""
    rng = np.random.default_rng(5)
    out_shape, spacing = (7, 10, 19), (3, 4, 5)
    shape = fr.lattice_shape(out_shape, spacing)[1:]
    c = rng.standard_normal(shape)
    v = rng.standard_normal(out_shape)
    (ix, wx), (iy, wy), (iz, wz) = fr._axes(out_shape, spacing)
    phi_c = np.zeros(out_shape)
    for cc in range(4):
        for b in range(4):
            for a in range(4):
                W = (wx[:, a].astype(np.float64)[None, None, :] * wy[:, b].astype(np.float64)[None, :, None]) * \
                    wz[:, cc].astype(np.float64)[:, None, None]
                phi_c += W * c[(iz + cc)[:, None, None], (iy + b)[None, :, None], (ix + a)[None, None, :]]
    adj, _, sup = fr.adjoint(v, spacing)
    mag, _, _ = fr.adjoint(np.abs(v), spacing)
    lhs, rhs = float((phi_c * v).sum()), float((c * adj).sum())
    assert abs(lhs - rhs) <= 2 * gamma(64 + v.size) * float((np.abs(c) * mag).sum())
    assert sup.sum() == 64 * v.size


def test_gradient_is_the_finite_difference_of_the_cost():
    """(2 / n) Gc against the central difference of S_ee / n over single control points, with A = [I | 0.5] and a zero
    lattice: every sample has the fractions 0.5, a control moved by h = 0.05 moves a sample by at most 4/6 h, so no
    sample changes its cell (asserted) and the trilinear interpolant is linear in the displacement: no truncation
    error, as in tests/test_affine_refine_host.py.  What is left is float32 rounding: eps = 16 u32 max |M| bounds a
    sample's error and 2 eps a gradient component's; the field value 0.5 + W h is rounded to float32 (2^-25 absolute),
    which moves e by |g| 2^-25.  Each e^2 is off by at most 2 |e| (eps + |g| 2^-25) + (eps + |g| 2^-25)^2; the
    analytic side by 2 sum W (|e| 2 eps + |g| eps + 2 eps^2)."""
    fshape, mshape, spacing, h = (9, 10, 11), (10, 11, 12), (4, 3, 5), 0.05
    F, M = gaussians(fshape, 3), gaussians(mshape, 4)
    A = np.eye(3, 4)
    A[:, 3] = 0.5
    shape = fr.lattice_shape(fshape, spacing)
    c0 = np.zeros(shape, np.float32)
    base, u0 = fr.evaluate(F, M, c0, spacing, A)
    assert base.n == F.size
    eps = 16 * U32 * float(np.abs(M).max())
    m, gx, gy, gz, _ = fr.sample_grad(M, u0)
    e = np.abs((m - F).astype(np.float64))
    G = [np.abs(v.astype(np.float64)) for v in (gx, gy, gz)]
    rng = np.random.default_rng(0)
    picks = [(d,) + tuple(rng.integers(0, n) for n in shape[1:]) for d in range(3) for _ in range(4)]
    picks += [(0, 0, 0, 0), (2,) + tuple(n - 1 for n in shape[1:])]
    for pick in picks:
        d = pick[0]
        side = []
        for sgn in (1.0, -1.0):
            c = c0.copy()
            c[pick] = sgn * h
            rec, u = fr.evaluate(F, M, c, spacing, A)
            assert np.array_equal(np.floor(u.astype(np.float64)), np.floor(u0.astype(np.float64)))
            assert rec.n == base.n
            side.append(rec)
        fd = (side[0].see - side[1].see) / (2 * h) / base.n
        ind = np.zeros(shape[1:])
        ind[pick[1:]] = 1.0
        W = np.zeros(fshape)                                             # the control's weight at every voxel
        (ix, wx), (iy, wy), (iz, wz) = fr._axes(fshape, spacing)
        for cc in range(4):
            for b in range(4):
                for a in range(4):
                    hit = ind[(iz + cc)[:, None, None], (iy + b)[None, :, None], (ix + a)[None, None, :]]
                    W += hit * (wx[:, a][None, None, :] * wy[:, b][None, :, None] * wz[:, cc][:, None, None])
        de = eps + G[d] * 2.0 ** -25
        e_side = e + h * G[d] * W
        bound = (2 * float(((2 * e_side * de + de * de) * (W > 0)).sum()) / (2 * h)
                 + 2 * float((W * (e * 2 * eps + G[d] * eps + 2 * eps * eps)).sum())) / base.n
        got = 2.0 / base.n * base.Gc[pick]
        print("control %s: gradient %.9g difference %.9g off %.3g bound %.3g" % (pick, got, fd, abs(fd - got), bound))
        assert abs(fd - got) <= bound
    assert np.abs(base.Gc).max() > 0


def test_bending_energy_of_an_affine_lattice_is_zero():
    """exactly 0 in exact arithmetic; in float64 each derivative is a sum of 27 products with cancellation, within
    gamma_30 of sum |coef| |c| <= (4 / delta_min^2) max |c| (the float32 lattice is itself affine only to u32 max |c|,
    which the second-difference stencils amplify by the same 4 / delta^2)"""
    out_shape, spacing = (9, 14, 21), (4, 3, 2)
    c = affine_lattice(out_shape, spacing, [[0.01, -0.02, 0.005], [0.0, 0.03, -0.01], [-0.015, 0.0, 0.02]],
                       [0.5, -1.25, 2.0]).astype(np.float32)
    R, dR, _, _ = fr.bending(c, spacing)
    tol = 2 * U32 * 4 / min(spacing) ** 2 * float(np.abs(c).max())       # per derivative
    assert 0 <= R <= 12 * 3 * tol * tol
    assert np.abs(dR).max() <= 2 * 9 * 27 * (4 / min(spacing) ** 2) * tol


def test_bending_gradient_is_the_finite_difference():
    """R is a quadratic form, so its central difference is exact up to rounding: R's sum is correctly rounded and
    each derivative carries at most 40 roundings, so a value of R is within 100 u R and the quotient within
    100 u R / h of dR/dc; dR itself within gamma_200 of its sum |term|.  The lattice holds multiples of 1/64, so that
    both sides of the difference are exactly h from the centre"""
    rng = np.random.default_rng(8)
    spacing, h = (4, 3, 2), 0.125
    c = (rng.integers(-128, 129, (3, 5, 6, 7)) / 64.0).astype(np.float32)   # c + h and c - h are exact in float32
    R, dR, _, dRt = fr.bending(c, spacing)
    assert R > 0
    for pick in [(0, 0, 0, 0), (1, 2, 3, 3), (2, 4, 5, 6), (0, 1, 1, 1), (2, 3, 0, 6), (1, 2, 2, 0)]:
        up, dn = c.copy(), c.copy()
        up[pick] += np.float32(h)
        dn[pick] -= np.float32(h)
        step = float(up[pick].astype(np.float64) - dn[pick].astype(np.float64))
        Ru, Rd = fr.bending(up, spacing)[0], fr.bending(dn, spacing)[0]
        assert abs((Ru - Rd) / step - dR[pick]) <= 100 * U * (Ru + Rd) / step + gamma(200) * dRt[pick], pick


@pytest.mark.parametrize("out_shape,spacing", [((9, 10, 21), (4, 3, 2)), ((5, 8, 8), 8), ((3, 4, 5), 8),
                                               ((6, 7, 33), 1), ((48, 48, 48), 8)])
def test_refine2_doubles_the_coarse_field(out_shape, spacing):
    """Subdivision leaves the spline unchanged: the refined lattice's field at the fine voxel 2 i is 2 x the coarse
    field at i.  Each is a float32 sum of 64 terms (bound 67 u32 sum-of-weights max |c|, as above); the subdivision
    adds at most 3 roundings per axis (9 u32 max |c|), and the weights of the two tables are rounded separately
    (3 u32 per term on each side): (2 * 70 + 9 + 6) u32 * 2 max |c| covers both sides."""
    rng = np.random.default_rng(2)
    cshape = tuple((o + 1) // 2 for o in out_shape)
    coarse = rng.uniform(-1.5, 1.5, fr.lattice_shape(cshape, spacing)).astype(np.float32)
    fine = fr.refine2(coarse, out_shape, spacing)
    assert fine.shape == fr.lattice_shape(out_shape, spacing)
    uc = fr.spline(coarse, spacing, cshape).astype(np.float64)
    uf = fr.spline(fine, spacing, out_shape).astype(np.float64)
    assert np.abs(uf[:, ::2, ::2, ::2] - 2 * uc).max() <= 155 * U32 * 2 * 1.5
    for o, d in zip(out_shape, fr.spacing3(spacing)[::-1]):                 # the index ranges close
        assert ((o - 1) // d) // 2 + 3 == fr.lattice_dim((o + 1) // 2, d) - 1


# ---- the library without a device --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bufs():
    """made-up addresses without a device; real allocations covering every range named below with one"""
    from sift3d_amd import api, hip
    if api.device_available():
        b = [hip.lib().sift3d_hip_malloc(1 << 22) for _ in range(7)]
        assert all(b)
        yield b
        for p in b:
            hip.lib().sift3d_hip_free(p)
    else:
        yield [0x10000000 * (k + 1) for k in range(7)]


def test_symbols_layouts_and_sizes(hip):
    from sift3d_amd import _native, api
    L = _native.load()
    for name in ("sift3d_amd_ffd_lattice_dim", "sift3d_amd_ffd_weights", "sift3d_amd_ffd_field_work_bytes",
                 "sift3d_amd_ffd_record_bytes", "sift3d_amd_ffd_evaluate_work_bytes",
                 "sift3d_amd_ffd_bending_work_bytes", "sift3d_amd_ffd_refine_work_bytes", "sift3d_hip_ffd_field",
                 "sift3d_hip_ffd_evaluate", "sift3d_hip_ffd_bending", "sift3d_hip_ffd_refine2",
                 "sift3d_amd_ffd_refine_default_params", "sift3d_amd_ffd_refine_struct_bytes",
                 "sift3d_amd_ffd_refine_device"):
        assert hasattr(L, name), name
    for f in ("ffd_field", "refine_ffd", "register_ffd", "ffd_bending_energy"):
        assert callable(getattr(api, f)), f
    L = hip.lib()
    S = L.sift3d_amd_ffd_refine_struct_bytes
    assert [S(k) for k in range(8)] == [C.sizeof(hip.FFDRefineParams), C.sizeof(hip.FFDEvaluation),
                                        C.sizeof(hip.FFDRefineResult), 32, 128, 6, 256, 0]
    assert C.sizeof(hip.FFDEvaluation) == 48 and C.sizeof(hip.FFDRefineParams) == 64
    G = L.sift3d_amd_ffd_lattice_dim
    assert [G(o, d) for o, d in ((1, 8), (8, 8), (9, 8), (17, 4), (5, 1))] == [4, 4, 5, 8, 8]
    assert G(0, 8) == 0 and G(8, 0) == 0 and G(-1, 2) == 0
    assert hip.ffd_lattice_shape((5, 9, 17), (4, 3, 2)) == fr.lattice_shape((5, 9, 17), (4, 3, 2)) == (3, 6, 6, 8)
    assert L.sift3d_amd_ffd_field_work_bytes(4, 3, 2) == 9 * 16 and L.sift3d_amd_ffd_field_work_bytes(0, 3, 2) == 0
    assert L.sift3d_amd_ffd_field_work_bytes(4, 257, 2) == 0
    assert L.sift3d_amd_ffd_record_bytes(4, 5, 6) == 32 + 2 * 3 * 120 * 8 and L.sift3d_amd_ffd_record_bytes(3, 5, 6) == 0
    E = L.sift3d_amd_ffd_evaluate_work_bytes
    assert E(8, 8, 8, 8, 8, 8) == 384 + 8 * (2 * hip.SIMILARITY_GRID + 3 * 512 + 3 * 256 + 3 * 128 + 18 * 8)
    assert E(0, 8, 8, 8, 8, 8) == 0 and E(8, 8, 8, 8, 0, 8) == 0
    assert L.sift3d_amd_ffd_bending_work_bytes(4, 4, 4) == 8 * (2 * hip.SIMILARITY_GRID + 18 * 8)
    W = L.sift3d_amd_ffd_refine_work_bytes
    assert W(8, 8, 8, 8, 8, 8, 8, 8, 8, 2) == W(8, 8, 8, 8, 8, 8, 8, 8, 8, 1) + 2 * 4 * 64
    assert W(8, 8, 8, 8, 8, 8, 8, 8, 8, 0) == 0 and W(8, 8, 8, 8, 8, 8, 8, 8, 8, 7) == 0
    assert W(8, 8, 8, 8, 0, 8, 8, 8, 8, 1) == 0 and W(8, 8, 8, 8, 8, 8, 8, 300, 8, 1) == 0
    p = hip.ffd_refine_params()
    assert (tuple(p.spacing), p.levels, p.max_evaluations) == ((8, 8, 8), 3, 60)
    assert (p.bending, p.step0, p.step_max, p.tol, p.min_overlap) == (0.005, 1.0, 4.0, 0.01, 0.5)
    assert L.sift3d_amd_ffd_weights(0, np.zeros(4, np.float32).ctypes.data) == -1
    assert L.sift3d_amd_ffd_weights(257, np.zeros(4, np.float32).ctypes.data) == -1
    assert L.sift3d_amd_ffd_weights(4, None) == -1


def _a(A):
    a = np.ascontiguousarray(A, np.float64).reshape(12)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


BAD_A = np.eye(3, 4)
BAD_A[2, 1] = np.inf


def test_field_refusals(hip, bufs):
    L = hip.lib()
    c, U_, W = bufs[:3]

    def call(c=c, g=(5, 5, 5), d=(8, 8, 8), A=None, o=(8, 8, 8), U=U_, W=W):
        keep, ptr = _a(A) if A is not None else (None, None)
        return L.sift3d_hip_ffd_field(c, *g, *d, ptr, *o, U, W, None)
    cases = [dict(c=None), dict(U=None), dict(W=None), dict(o=(0, 8, 8)), dict(o=(8, 8, -1)), dict(d=(0, 8, 8)),
             dict(d=(8, 8, 257)), dict(g=(4, 5, 5)), dict(g=(5, 5, 6)), dict(o=(9, 8, 8)), dict(A=BAD_A),
             dict(c=c + 2), dict(U=U_ + 1), dict(W=W + 4), dict(W=W + 8),
             dict(U=c), dict(U=c + 4 * 374), dict(W=c), dict(W=U_ + 16 * 383), dict(U=W + 16)]
    for kw in cases:
        assert call(**kw) == -1, kw


def test_evaluate_bending_and_refine2_refusals(hip, bufs):
    L = hip.lib()
    F, M, c, U_, R, G, W = bufs

    def call(F=F, o=(8, 8, 8), M=M, n=(8, 8, 8), c=c, g=(5, 5, 5), d=(8, 8, 8), A=None, lam=0.0, U=U_, R=R, G=G, W=W):
        keep, ptr = _a(A) if A is not None else (None, None)
        return L.sift3d_hip_ffd_evaluate(F, *o, M, *n, c, *g, *d, ptr, lam, U, R, G, W, None)
    nan = float("nan")
    cases = [dict(F=None), dict(M=None), dict(c=None), dict(U=None), dict(R=None), dict(G=None), dict(W=None),
             dict(o=(0, 8, 8)), dict(n=(8, 0, 8)), dict(d=(8, -1, 8)), dict(d=(300, 8, 8)), dict(g=(5, 4, 5)),
             dict(A=BAD_A), dict(lam=-1.0), dict(lam=nan), dict(lam=float("inf")),
             dict(F=F + 2), dict(M=M + 1), dict(c=c + 3), dict(U=U_ + 2), dict(R=R + 4), dict(G=G + 2), dict(W=W + 8),
             dict(U=F), dict(R=M + 4 * 511), dict(G=c + 4 * 374), dict(W=F), dict(R=U_), dict(G=R + 32), dict(W=G),
             dict(U=W + 64)]
    for kw in cases:
        assert call(**kw) == -1, kw

    def bend(c=c, g=(5, 5, 5), d=(8, 8, 8), R=R, W=W):
        return L.sift3d_hip_ffd_bending(c, *g, *d, R, W, None)
    for kw in [dict(c=None), dict(R=None), dict(W=None), dict(g=(3, 5, 5)), dict(g=(5, 5, 0)), dict(d=(0, 8, 8)),
               dict(d=(8, 8, 1000)), dict(c=c + 1), dict(R=R + 4), dict(W=W + 4), dict(R=c), dict(W=c + 4 * 374),
               dict(R=W + 8)]:
        assert bend(**kw) == -1, kw

    def sub(c=c, o=(16, 16, 16), d=(8, 8, 8), f=G):
        return L.sift3d_hip_ffd_refine2(c, *o, *d, f, None)
    for kw in [dict(c=None), dict(f=None), dict(o=(0, 16, 16)), dict(d=(8, 0, 8)), dict(d=(8, 8, 257)), dict(c=c + 2),
               dict(f=G + 1), dict(f=c), dict(f=c + 4 * 191), dict(f=c - 4 * 374)]:      # 3 * 64 coarse, 3 * 125 fine
        assert sub(**kw) == -1, kw


def test_refine_device_refusals(hip, bufs):
    L = hip.lib()
    F, M, c, U_, _, _, W = bufs
    res = hip.FFDRefineResult()

    def call(F=F, o=(8, 8, 8), M=M, n=(8, 8, 8), A=None, res=C.byref(res), c=c, U=U_, W=W, null_params=False, **kw):
        keep, ptr = _a(A) if A is not None else (None, None)
        p = None if null_params else C.byref(hip.ffd_refine_params(**kw))
        return L.sift3d_amd_ffd_refine_device(F, *o, M, *n, ptr, p, res, c, U, W, None)
    nan, inf = float("nan"), float("inf")
    cases = [dict(F=None), dict(M=None), dict(res=None), dict(c=None), dict(U=None), dict(W=None),
             dict(o=(0, 8, 8)), dict(n=(8, 8, -1)), dict(A=BAD_A), dict(levels=0), dict(levels=7),
             dict(max_evaluations=0), dict(max_evaluations=129), dict(bending=-1.0), dict(bending=nan),
             dict(step0=0.0), dict(step0=nan), dict(step_max=0.5), dict(step_max=inf), dict(tol=0.0), dict(tol=nan),
             dict(min_overlap=-0.1), dict(min_overlap=1.5), dict(min_overlap=nan),
             dict(F=F + 2), dict(M=M + 1), dict(c=c + 2), dict(U=U_ + 1), dict(W=W + 8),
             dict(W=F), dict(W=M + 4 * 511), dict(c=F), dict(U=M), dict(c=U_ + 4 * 3 * 511), dict(U=W + 1024)]
    for kw in cases:
        assert call(**kw) == -1, kw
    p = hip.ffd_refine_params()
    p.spacing[1] = 0
    assert L.sift3d_amd_ffd_refine_device(F, 8, 8, 8, M, 8, 8, 8, None, C.byref(p), C.byref(res), c, U_, W, None) == -1


def test_python_value_errors():
    from sift3d_amd import api, hip
    v = np.zeros((5, 7, 9), np.float32)
    for kw in (dict(spacing=0), dict(spacing=257), dict(spacing=(8, 8)), dict(spacing=1.5), dict(levels=0),
               dict(levels=7), dict(bending=-1.0), dict(bending=float("nan")), dict(A=np.eye(3)),
               dict(max_evaluations=0), dict(bogus=1)):
        with pytest.raises(ValueError):
            api.refine_ffd(v, v, **kw)
    with pytest.raises(ValueError):
        api.ffd_field(np.zeros((3, 4, 4, 4), np.float32), 8, (8, 8, 9))      # the lattice is not g
    with pytest.raises(ValueError):
        api.ffd_field(np.zeros((2, 4, 4, 4), np.float32), 8, (8, 8, 8))
    with pytest.raises(ValueError):
        hip.ffd_weights(0)
    if not api.device_available():
        with pytest.raises(RuntimeError):
            api.refine_ffd(v, v)


# ---- the driver ---------------------------------------------------------------------------------------------------
DRIVER = dict(spacing=8, levels=2, bending=0.005, max_evaluations=20)


def known_displacement(shape, amplitude=2.0):
    """w [3, z, y, x] float64: one sinusoid period per axis, w_x from y, w_y from z, w_z from x"""
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    return amplitude * np.stack([np.sin(2 * np.pi * y / shape[1]), np.sin(2 * np.pi * z / shape[0]),
                                 np.sin(2 * np.pi * x / shape[2])])


@functools.lru_cache(maxsize=None)
def driver_pair():
    """(fixed, moving, truth): a 48^3 crop of a 64^3 synth_survey volume and of the same volume resampled through the
    known smooth field w (warp_field's restatement; the crop keeps 8 voxels from every face, w moves at most 2, so no
    fill inside), and the field the registration should find: moving(p) = base(p + w(p)), so fixed(p) =
    moving(p + u(p)) with u + w(p + u) = 0, solved by fixed-point iteration on the analytic w"""
    from sift3d_amd import api
    n, lo, m = 64, 8, 48
    base = np.ascontiguousarray(api.synth_survey(n), np.float32)
    big = np.zeros((3, n, n, n))
    big[:, lo:lo + m, lo:lo + m, lo:lo + m] = known_displacement((m, m, m))
    ext = known_displacement((m, m, m))

    def w_at(q):                                                         # analytic, crop coordinates (x, y, z)
        return 2.0 * np.stack([np.sin(2 * np.pi * q[1] / m), np.sin(2 * np.pi * q[2] / m),
                               np.sin(2 * np.pi * q[0] / m)])
    z, y, x = np.meshgrid(*(np.arange(-lo, n - lo, dtype=np.float64),) * 3, indexing="ij")
    wfull = w_at(np.stack([x, y, z])).astype(np.float32)
    moved = ref_warp_field(base, wfull)
    F = np.ascontiguousarray(base[lo:lo + m, lo:lo + m, lo:lo + m])
    M = np.ascontiguousarray(moved[lo:lo + m, lo:lo + m, lo:lo + m])
    z, y, x = np.meshgrid(*(np.arange(m, dtype=np.float64),) * 3, indexing="ij")
    p = np.stack([x, y, z])
    u = np.zeros_like(p)
    for _ in range(60):
        u = -w_at(p + u)
    assert np.abs(u + w_at(p + u)).max() < 1e-9 and ext.shape == u.shape
    return F, M, u


def summarize(trail, fld, truth):
    """(msd ratio last accepted / first, rms field error over the voxels 4 away from every face)"""
    first = [e for e in trail if e[6] == 0][0]
    last = [e for e in trail if e[6] == 0 and e[5]][-1]
    inner = (slice(None),) + (slice(4, -4),) * 3
    rms = float(np.sqrt(((np.asarray(fld, np.float64) - truth)[inner] ** 2).sum(axis=0).mean()))
    return last[1] / first[1], rms


@functools.lru_cache(maxsize=None)
def restatement_driver():
    F, M, truth = driver_pair()
    r = fr.refine(F, M, None, DRIVER["spacing"], DRIVER["levels"], DRIVER["bending"], DRIVER["max_evaluations"])
    return r, summarize(r.trail, r.field, truth)


def check_trail(trail, levels, max_evaluations):
    """the trail's conventions: levels coarse to fine, the first entry of a level accepted at step0, E falls strictly
    over the accepted entries of a level, E = msd + bending R, the step doubles after an accept (up to step_max) and
    halves after a reject"""
    lv = [e[6] for e in trail]
    assert lv == sorted(lv, reverse=True) and set(lv) == set(range(levels))
    for l in range(levels):
        es = [e for e in trail if e[6] == l]
        assert 1 <= len(es) <= max_evaluations and es[0][5] and es[0][4] == 1.0
        acc = [e[0] for e in es if e[5]]
        assert all(b < a for a, b in zip(acc, acc[1:]))
        for a, b in zip(es[1:], es[2:]):
            assert b[4] == (min(2 * a[4], 4.0) if a[5] else a[4] / 2)
        for e in es:
            assert abs(e[0] - (e[1] + DRIVER["bending"] * e[2])) <= 1e-12 * abs(e[0]) and e[3] > 0


def test_restatement_driver_recovers_the_known_field():
    """the figures DESIGN.md 3.4.9 records; the field is recovered to a fraction of its 2-voxel amplitude"""
    r, (ratio, rms) = restatement_driver()
    print("restatement driver: stop %s, %d evaluations, MSD ratio %.4g, RMS field error %.4g voxels"
          % (r.stop, len(r.trail), ratio, rms))
    check_trail(r.trail, DRIVER["levels"], DRIVER["max_evaluations"])
    assert r.stop in fr.STOPS
    assert ratio < 0.5 and rms < 1.0                                     # RMS of the truth itself: 2.45
