"""The Jacobian penalty without a device (include/sift3d_amd.h, "Jacobian penalty"): the restatement
(tests/jacobian_penalty_restatement.py) against calculus, phi's two properties, every refusal of the two entries before
any device call, the exported symbols and work sizes, and the layouts that must not have changed."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import ffd_restatement as fr
from tests import jacobian_penalty_restatement as jp
from tests.demons_restatement import gamma
from tests.test_ffd_host import BAD_A, _a

U = 2.0 ** -53
REF = 1.3
H = 2.0 ** -23


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


# ---- phi ---------------------------------------------------------------------------------------------------------
def test_phi_is_c1_at_one_quarter():
    """value and slope of the two branches at r = 1/4, each evaluated by its own formula: equal, exactly"""
    r = 0.25
    hi, dhi = (r + 1.0 / r) - 2.0, 1.0 - 1.0 / (r * r)
    t = r - 0.25
    lo, dlo = (2.25 - 15.0 * t) + 64.0 * (t * t), -15.0 + 128.0 * t
    assert hi == lo == 2.25 and dhi == dlo == -15.0
    assert 2.0 / r ** 3 == 128.0                                          # and the curvature: the Taylor polynomial's
    below = np.nextafter(0.25, 0.0)
    assert jp.phi_of(0.25) == (2.25, -15.0) and abs(jp.phi_of(below)[0] - 2.25) <= 16 * U


def test_phi_is_symmetric_on_dyadic_r():
    """phi(r) = phi(1 / r): for r = 2^k, 1/4 <= r <= 4, r and 1 / r are exact and r + 1 / r is the same sum of the same
    two numbers; bit for bit"""
    for k in (-2, -1, 0, 1, 2):
        r = 2.0 ** k
        assert jp.phi_of(r)[0] == jp.phi_of(1.0 / r)[0], k
    assert jp.phi_of(1.0) == (0.0, 0.0)
    # other dyadic r above 1/4 whose reciprocal is not dyadic: equal within the roundings of 1 / r and the sums
    for r in (0.375, 0.75, 1.5, 2.5, 3.0):
        a, b = float(jp.phi_of(r)[0]), float(jp.phi_of(1.0 / r)[0])
        assert abs(a - b) <= 4 * U * (r + 1.0 / r + 2.0), r


def test_phi_is_finite_and_hands_a_nan_on():
    p, d = jp.phi_of(np.array([-1e3, -1.0, 0.0, 1e-300, 0.2, np.nan]))
    assert np.isfinite(p[:5]).all() and np.isfinite(d[:5]).all() and np.isnan(p[5])
    assert np.all(d[:5] < 0)                                             # below 1/4 the slope points back towards 1


# ---- calculus on the float64 restatement -------------------------------------------------------------------------
def sample_field():
    """(5, 4, 6) random float64 field whose r covers the three branches"""
    rng = np.random.default_rng(0)
    return rng.uniform(-1.0, 1.0, (3, 5, 4, 6))


def fd_against(analytic_over_n, up, dn, base, umax, n):
    """The central difference of P between the penalties `up` and `dn` (the variable moved by +H and -H) against the
    analytic derivative, and the bound it must meet.

    Moving one field value (or one control of channel d) moves only row d of every j(p), and det is linear in a row: so
    r_p(s) = r_p + s k_p exactly, and k_p = (r+_p - r-_p) / 2H up to rounding.  For phi with |phi''| <= B_p between r-_p
    and r+_p, |(phi(r+) - phi(r-)) / 2H - phi'(r) k| <= (H / 2) B_p k_p^2 (Taylor with the remainder in phi''; phi is
    C^2 with phi'' = 2 / r^3 <= 128 from 1/4 up and 128 below, so B_p is phi'' at the smaller end, capped at 128).
    Rounding: a computed r is within dr = gamma_16 6 J^3 / |ref| of the exact one (J = 1 + 2 max |u| bounds every |j|
    with its own two roundings; six products of three in the det), a phi within L_p dr + 4 u m_p (L_p the larger
    |phi'| of the two ends plus 128 dr, m_p the sum of |terms| of the branch's formula), and the difference is summed
    over the voxels that moved only (the others cancel exactly, term by term).  The analytic side carries
    (128 dr / |ref| + 8 u |a_p|) 2 J^2 per term, seven terms per voxel at most."""
    J = 1.0 + 2.0 * umax
    dr = gamma(16) * 6.0 * J ** 3 / abs(REF)
    moved = up.r != dn.r
    k = (up.r - dn.r) / (2 * H)
    lo = np.minimum(up.r, dn.r)
    B = np.where(lo >= 0.25, 2.0 / np.maximum(lo, 0.25) ** 3, 128.0)
    trunc = float((0.5 * H * B * k * k)[moved].sum())
    L = np.maximum(np.abs(jp.phi_of(up.r)[1]), np.abs(jp.phi_of(dn.r)[1])) + 128.0 * dr
    mag = []
    for q in (up.r, dn.r):
        t = q - 0.25
        mag.append(np.where(q >= 0.25, np.abs(q) + 1.0 / np.maximum(np.abs(q), 0.25) + 2.0,
                            2.25 + 15.0 * np.abs(t) + 64.0 * t * t))
    dphi = L * dr + 4 * U * np.maximum(*mag)
    rounding = float((2.0 * dphi)[moved].sum()) / (2 * H)
    a = np.abs(jp.phi_of(base.r)[1] / REF)
    analytic = float((7.0 * (128.0 * dr / abs(REF) + 8 * U * a) * 2.0 * J * J)[moved].sum())
    fd = math.fsum((up.phi - dn.phi).reshape(-1).tolist()) / (2 * H) / n
    bound = (trunc + rounding + analytic) / n
    return fd, abs(fd - analytic_over_n), bound


def test_sum_form_is_the_gradient_of_the_penalty():
    u = sample_field()
    base = jp.penalty(u, REF, np.float64)
    r = base.r
    assert (r >= 0.25).any() and ((r > 0) & (r < 0.25)).any() and (r <= 0).any()
    n = r.size
    worst = 0.0
    for idx in np.ndindex(u.shape):
        a, b = u.copy(), u.copy()
        a[idx] += H
        b[idx] -= H
        assert a[idx] - u[idx] == H and u[idx] - b[idx] == H             # the step is exact (|u| <= 1, H = 2^-23)
        fd, off, bound = fd_against(base.S[idx] / n, jp.penalty(a, REF, np.float64), jp.penalty(b, REF, np.float64),
                                    base, 1.0 + H, n)
        worst = max(worst, off / bound)
        assert off <= bound, (idx, fd, base.S[idx] / n, off, bound)
    print("S / N against central differences: worst off / bound %.3g" % worst)
    assert np.abs(base.S).max() > 0


def spline64(c, spacing, out_shape):
    """the spline of a float64 lattice channel-wise, float64 (the float32 weights widened): linear in c"""
    (ix, wx), (iy, wy), (iz, wz) = fr._axes(out_shape, spacing)
    s = np.zeros((3,) + tuple(out_shape))
    for cc in range(4):
        for b in range(4):
            for a in range(4):
                W = (wx[:, a].astype(np.float64)[None, None, :] * wy[:, b].astype(np.float64)[None, :, None]) * \
                    wz[:, cc].astype(np.float64)[:, None, None]
                s += W * c[:, (iz + cc)[:, None, None], (iy + b)[None, :, None], (ix + a)[None, None, :]]
    return s


def test_adjoint_of_the_sum_form_is_the_gradient_over_the_lattice():
    """d P / d c = Phi^T S / N: the same check through the spline, on every control of a lattice over (5, 4, 6)"""
    out_shape, spacing = (5, 4, 6), (3, 2, 2)
    rng = np.random.default_rng(1)
    c = rng.integers(-5 * 1024, 5 * 1024 + 1, fr.lattice_shape(out_shape, spacing)) / 1024.0   # c + H, c - H exact
    u = spline64(c, spacing, out_shape)
    base = jp.penalty(u, REF, np.float64)
    r = base.r
    assert (r >= 0.25).any() and ((r > 0) & (r < 0.25)).any() and (r <= 0).any()
    n = r.size
    GJ = jp.lattice_gradient(base.S, spacing, exact=True)
    # the adjoint's own sums are correctly rounded; its terms carry S's error, which fd_against allows for per voxel
    worst = 0.0
    for idx in np.ndindex(c.shape):
        a, b = c.copy(), c.copy()
        a[idx] += H
        b[idx] -= H
        ua, ub = spline64(a, spacing, out_shape), spline64(b, spacing, out_shape)
        umax = float(max(np.abs(ua).max(), np.abs(ub).max()))
        fd, off, bound = fd_against(GJ[idx] / n, jp.penalty(ua, REF, np.float64), jp.penalty(ub, REF, np.float64),
                                    base, umax, n)
        # the field's own rounding (64 terms, gamma_66 of at most max |c|) moves every r by at most 3 J^2 of it
        J = 1.0 + 2.0 * umax
        slack = gamma(66) * 2.0 * 3.0 * J * J / abs(REF) * float(np.abs(jp.phi_of(base.r)[1]).max() + 128.0) * \
            np.count_nonzero(ua != ub) / (2 * H) / n
        worst = max(worst, off / (bound + slack)) if bound + slack > 0 else worst
        assert off <= bound + slack, (idx, fd, GJ[idx] / n, off, bound, slack)
    print("Phi^T S / N against central differences over the lattice: worst off / bound %.3g" % worst)
    assert np.abs(GJ).max() > 0


def test_float32_mode_is_the_determinant_the_library_reports():
    """the restatement's float32 j and double det are "Displacement fields" steps 1 - 3: rounded to float they are
    numpy.gradient's determinant as tests/field_restatement.py states it"""
    from tests.field_restatement import ref_jacobian_det
    rng = np.random.default_rng(4)
    u = rng.uniform(-1.5, 1.5, (3, 5, 4, 6)).astype(np.float32)
    p = jp.penalty(u, 1.0)
    assert np.array_equal(p.r.astype(np.float32), ref_jacobian_det(u))
    assert p.nonpos == int((~(p.r > 0)).sum()) and p.rmin == p.r.min() and p.rmax == p.r.max()
    assert p.P == p.sum / u[0].size


def test_reference_determinant_order():
    A = np.array([[1.1, 0.2, -0.1, 3.0], [0.05, 0.9, 0.3, -2.0], [-0.2, 0.1, 1.2, 0.5]])
    assert abs(jp.ref_of(A) - np.linalg.det(A[:, :3])) <= 16 * U * 3.0
    assert jp.ref_of(None) == 1.0 and jp.ref_of(np.eye(3, 4)) == 1.0


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


def test_symbols_sizes_and_unchanged_layouts(hip):
    from sift3d_amd import _native, api
    L = _native.load()
    for name in ("sift3d_amd_jacobian_penalty_work_bytes", "sift3d_hip_jacobian_penalty",
                 "sift3d_amd_ffd_refine_jacobian_work_bytes", "sift3d_amd_ffd_refine_jacobian_device"):
        assert hasattr(L, name), name
    for f in ("jacobian_penalty", "refine_ffd"):
        assert callable(getattr(api, f)), f
    assert callable(hip.jacobian_penalty_record) and callable(hip.jacobian_penalty)
    assert callable(hip.ffd_refine_jacobian)
    L = hip.lib()
    W = L.sift3d_amd_jacobian_penalty_work_bytes
    assert W(6, 4, 5) == 8 * (4 * hip.SIMILARITY_GRID + 120) and W(1, 1, 1) == 8 * (4 * hip.SIMILARITY_GRID + 1)
    assert W(0, 4, 5) == 0 and W(6, -1, 5) == 0 and W(6, 4, 0) == 0
    assert hip.JACOBIAN_PENALTY_RECORD_BYTES == 32 and C.sizeof(hip.FFDPenalty) == 24
    D = L.sift3d_amd_ffd_refine_jacobian_work_bytes
    M = L.sift3d_amd_ffd_mi_refine_work_bytes
    for levels in (1, 2):
        assert D(9, 8, 7, 8, 8, 8, 4, 3, 2, levels) == M(9, 8, 7, 8, 8, 8, 4, 3, 2, levels) + 32 + \
            8 * 3 * 6 * 6 * 7 + W(9, 8, 7)                               # the lattice of (9, 8, 7) at (4, 3, 2): 6 x 6 x 7
    assert D(8, 8, 8, 8, 8, 8, 8, 8, 8, 0) == 0 and D(8, 8, 8, 8, 8, 8, 8, 8, 8, 7) == 0
    assert D(0, 8, 8, 8, 8, 8, 8, 8, 8, 1) == 0 and D(8, 8, 8, 8, 8, 8, 8, 300, 8, 1) == 0
    # additions only: every layout and size of the existing FFD entries is what it was
    S = L.sift3d_amd_ffd_refine_struct_bytes
    assert [S(k) for k in range(8)] == [64, 48, 8 + 48 * 6 * 128, 32, 128, 6, 256, 0]
    assert C.sizeof(hip.FFDRefineParams) == 64 and C.sizeof(hip.FFDEvaluation) == 48
    assert L.sift3d_amd_ffd_record_bytes(4, 5, 6) == 32 + 2 * 3 * 120 * 8
    assert L.sift3d_amd_ffd_evaluate_work_bytes(8, 8, 8, 8, 8, 8) == \
        384 + 8 * (2 * hip.SIMILARITY_GRID + 3 * 512 + 3 * 256 + 3 * 128 + 18 * 8)
    R = L.sift3d_amd_ffd_refine_work_bytes
    assert R(8, 8, 8, 8, 8, 8, 8, 8, 8, 2) == R(8, 8, 8, 8, 8, 8, 8, 8, 8, 1) + 2 * 4 * 64


def test_jacobian_penalty_refusals(hip, bufs):
    L = hip.lib()
    fld, rec, grad, work = bufs[:4]
    nan, inf = float("nan"), float("inf")
    field_bytes, n = 4 * 3 * 8 * 8 * 8, 512

    def call(fld=fld, o=(8, 8, 8), ref=1.0, rec=rec, grad=grad, work=work):
        return L.sift3d_hip_jacobian_penalty(fld, *o, ref, rec, grad, work, None)
    cases = [dict(fld=None), dict(rec=None), dict(work=None), dict(o=(0, 8, 8)), dict(o=(8, -1, 8)), dict(o=(8, 8, 0)),
             dict(ref=0.0), dict(ref=-0.0), dict(ref=nan), dict(ref=inf), dict(ref=-inf),
             dict(fld=fld + 2), dict(rec=rec + 4), dict(grad=grad + 4), dict(work=work + 4),
             dict(rec=fld), dict(rec=fld + field_bytes - 8), dict(grad=fld + field_bytes - 8), dict(work=fld),
             dict(grad=rec), dict(work=rec + 24), dict(grad=work + 8 * (4 * hip.SIMILARITY_GRID + n) - 8),
             dict(work=grad + 8 * 3 * n - 8), dict(rec=grad + 8 * 3 * n - 8)]
    for kw in cases:
        assert call(**kw) == -1, kw


def test_refine_jacobian_device_refusals(hip, bufs):
    L = hip.lib()
    F, M, c, U_, _, _, W = bufs
    res = hip.FFDRefineResult()
    sim = hip.Similarity()
    pen = (hip.FFDPenalty * (hip.AFFINE_MAX_LEVELS * hip.FFD_MAX_EVALUATIONS))()
    singular = np.eye(3, 4)
    singular[2, :3] = singular[1, :3]

    def call(F=F, o=(8, 8, 8), M=M, n=(8, 8, 8), A=None, res=C.byref(res), c=c, U=U_, W=W, WF=None, WM=None, bins=0,
             rf=(0.0, 1.0), rm=(0.0, 1.0), sim=C.byref(sim), jac=1.0, pen=pen, **kw):
        keep, ptr = _a(A) if A is not None else (None, None)
        p = C.byref(hip.ffd_refine_params(**kw))
        return L.sift3d_amd_ffd_refine_jacobian_device(F, *o, M, *n, ptr, p, res, c, U, W, None, WF, WM, bins, *rf, *rm,
                                                       sim, jac, pen)
    nan, inf = float("nan"), float("inf")
    cases = [dict(F=None), dict(M=None), dict(res=None), dict(c=None), dict(U=None), dict(W=None), dict(pen=None),
             dict(bins=32, sim=None), dict(jac=-1.0), dict(jac=nan), dict(jac=inf), dict(A=BAD_A), dict(A=singular),
             dict(A=np.zeros((3, 4))), dict(o=(0, 8, 8)), dict(n=(8, 8, -1)), dict(levels=0), dict(levels=7),
             dict(max_evaluations=0), dict(max_evaluations=129), dict(bending=-1.0), dict(bending=nan),
             dict(step0=0.0), dict(step_max=0.5), dict(tol=0.0), dict(min_overlap=1.5),
             dict(bins=3), dict(bins=65), dict(bins=32, rf=(1.0, 1.0)), dict(bins=32, rm=(0.0, nan)),
             dict(F=F + 2), dict(M=M + 1), dict(c=c + 2), dict(U=U_ + 1), dict(W=W + 8), dict(WF=F + 2), dict(WM=M + 1),
             dict(W=F), dict(W=M + 4 * 511), dict(c=F), dict(U=M), dict(c=U_ + 4 * 3 * 511), dict(U=W + 1024),
             # the penalty's share of the work buffer is checked too: a lattice that starts inside its last bytes
             dict(c=W + L.sift3d_amd_ffd_refine_jacobian_work_bytes(8, 8, 8, 8, 8, 8, 8, 8, 8, 3) - 4)]
    for kw in cases:
        assert call(**kw) == -1, kw


def test_python_value_errors():
    from sift3d_amd import api
    v = np.zeros((5, 7, 9), np.float32)
    singular = np.eye(3, 4)
    singular[0, :3] = 0.0
    for kw in (dict(jacobian=-1.0), dict(jacobian=float("nan")), dict(jacobian=float("inf")),
               dict(jacobian=1.0, A=singular)):
        with pytest.raises(ValueError):
            api.refine_ffd(v, v, **kw)
    f = np.zeros((3, 4, 4, 4), np.float32)
    for ref in (0.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            api.jacobian_penalty(f, ref)
    if not api.device_available():
        with pytest.raises(RuntimeError):
            api.jacobian_penalty(f)
