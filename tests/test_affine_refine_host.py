"""CPU (not gpu): the affine refinement contract (include/sift3d_amd.h, "Intensity-driven affine refinement") without a
device.  The numpy restatement (tests/affine_refine_restatement.py) against analysis, the host entries
sift3d_amd_affine_lm_step and sift3d_amd_affine_apply_delta against the restatement, every argument refusal of the
device entries (which check their arguments before any device call), and the restatement's driver on the cases that
tests/test_affine_refine.py runs on the device."""
import ctypes as C

import numpy as np
import pytest

from tests import affine_refine_restatement as ar
from tests.test_similarity_host import end_to_end_case
from tests.test_warp import about_center, ref_warp, rot

U = 2.0 ** -53
U32 = 2.0 ** -24
TOL = 1e-3                                                  # the driver's default, voxels


def gaussians(shape, seed, k=4):
    """a smooth volume: the sum of k Gaussians of width about a third of the grid"""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    v = np.zeros(shape)
    for _ in range(k):
        c = rng.uniform(0.2, 0.8, 3) * (np.array(shape) - 1)
        s = rng.uniform(0.25, 0.4) * min(shape)
        v += rng.uniform(0.5, 1.5) * np.exp(-((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) / (2 * s * s))
    return v.astype(np.float32)


def inverse(T):
    R = np.linalg.inv(T[:, :3])
    return np.hstack([R, (-R @ T[:, 3])[:, None]])


# ---- the restatement against analysis ----------------------------------------------------------------------------
def _fd_maps():
    """name -> A for the finite-difference check on the 10 x 11 x 12 grid.  "half": [I | 0.5], every fraction 0.5.
    "general": a rotation of 1 degree about (1, 2, 3) through the centre plus an irrational shift, which puts the
    centre's fractions at (sqrt 2 - 1, sqrt 3 - 1, (sqrt 5 - 1) / 2 - 0.3) = (0.414, 0.732, 0.318); the rotation
    moves a voxel at most 6.5 * sin(1 degree) * sqrt 2 = 0.16 from that on an axis, so fx, fy and fz differ from one
    another (by 0.05 and more on average, asserted) and from a half, vary over the grid, and stay at least 0.1 from a
    lattice plane."""
    half = np.eye(3, 4)
    half[:, 3] = 0.5
    shape = (10, 11, 12)
    frac = (np.sqrt(2.0) - 1, np.sqrt(3.0) - 1, (np.sqrt(5.0) - 1) / 2 - 0.3)
    return {"half": half, "general": about_center(rot((1, 2, 3), 1.0), shape, shape, shift=frac)}


@pytest.mark.parametrize("which", ["half", "general"])
def test_b_is_the_finite_difference_of_the_sum_of_squares(which):
    """2 b_r = d S_ee / d theta_r, by the central difference (S(theta + h) - S(theta - h)) / 2h over each of the 12
    centred parameters, F and M sums of Gaussians (10 x 11 x 12 and one voxel more per axis), at the two maps of
    _fd_maps: the second tells the three fractions apart, which the first cannot.

    Parameter (d, j) moves q_d only, by h |P_j| <= 5.5 h = 0.055 with h = 1e-2, and every sample is at least 0.1
    from a lattice plane: no sample changes its cell (asserted), and along one axis the trilinear
    interpolant is linear within a cell.  So the central difference has no truncation error whatever the volume's
    second derivative (which would enter through the samples that change cells): e(theta +- h) = e +- h g P_j, and
    the difference of the squares is 4 h e g P_j exactly.  What is left is rounding.  eps = 16 u32 max |M| bounds
    the float32 error of a sample (the rounding of f and three levels of lerp, three operations each) and 2 eps that
    of a gradient component (a difference of two such values).  Each e^2 of S is off by at most 2 |e| eps + eps^2, so
    the difference quotient by sum over both sides of that / 2h; 2 b_r by 2 sum |P_j| (|e| 2 eps + |g| eps + 2 eps^2).
    The tolerance is the sum of the two (float64 roundings are 2^29 times smaller)."""
    fshape, mshape, h = (10, 11, 12), (11, 12, 13), 1e-2
    F, M = gaussians(fshape, 1), gaussians(mshape, 2)
    A = _fd_maps()[which]
    base = ar.normal_equations(F, M, A)
    assert base.n == F.size
    fr = [v - np.floor(v) for v in ar.ref_coords(A, *np.meshgrid(*(np.arange(n) for n in fshape), indexing="ij")[::-1])]
    assert all(v.min() >= 0.1 and v.max() <= 0.9 for v in fr)
    if which == "general":                                       # the fractions differ: a swap of two would show
        assert min(np.abs(fr[0] - fr[1]).mean(), np.abs(fr[1] - fr[2]).mean(), np.abs(fr[0] - fr[2]).mean()) > 0.05
        assert all(np.ptp(v) > 0.1 for v in fr)
    eps = 16 * U32 * float(np.abs(M).max())
    m, gx, gy, gz, ins = ar.sample_grad(M, A, fshape)
    e = np.abs((m - F).astype(np.float64))
    c = ar.centre(fshape)
    z, y, x = np.meshgrid(*(np.arange(n) for n in fshape), indexing="ij")
    P = [np.abs(x - c[0]), np.abs(y - c[1]), np.abs(z - c[2]), np.ones(fshape)]
    G = [np.abs(v.astype(np.float64)) for v in (gx, gy, gz)]
    for r in range(12):
        d, j = divmod(r, 4)
        delta = np.zeros(12)
        delta[r] = h
        side = []
        for sgn in (1.0, -1.0):
            At = ar.apply_delta(A, sgn * delta, fshape)
            q = ar.ref_coords(At, x, y, z)
            assert all(np.array_equal(np.floor(v), np.floor(w)) for v, w in zip(q, ar.ref_coords(A, x, y, z)))
            side.append(ar.normal_equations(F, M, At))
        fd = (side[0].see - side[1].see) / (2 * h)
        e_side = e + h * G[d] * P[j]
        bound = 2 * float((2 * e_side * eps + eps * eps).sum()) / (2 * h) \
            + 2 * float((P[j] * (e * 2 * eps + G[d] * eps + 2 * eps * eps)).sum())
        print("%s parameter %2d: 2 b %.9g difference %.9g off %.3g bound %.3g"
              % (which, r, 2 * base.b[r], fd, abs(fd - 2 * base.b[r]), bound))
        assert abs(fd - 2 * base.b[r]) <= bound
        assert bound < 0.05 * np.abs(2 * base.b).max()               # the bound says something


def test_h_is_symmetric_and_positive_semidefinite():
    """H = sum J J^T.  Its computed eigenvalues are off by at most ||H - H_exact|| <= 12 * 2 u * max sum |term| (each
    entry a correctly rounded sum of products rounded once) plus the eigensolver's own backward error, a small
    multiple of 12 u ||H||; 100 u ||H||_F covers both."""
    F, M = gaussians((9, 10, 11), 3), gaussians((10, 9, 12), 4)
    A = about_center(rot((1, 2, 3), 7.0), M.shape, F.shape, shift=(0.3, -0.2, 0.4))
    rec = ar.normal_equations(F, M, A)
    assert 0 < rec.n < F.size
    assert np.array_equal(rec.H, rec.H.T)
    w = np.linalg.eigvalsh(rec.H)
    assert w.min() >= -100 * U * np.linalg.norm(rec.H), w
    assert rec.see > 0 and np.all(np.diag(rec.H) > 0)


def test_constant_moving_volume_gives_zero_b_and_h():
    F = gaussians((6, 7, 8), 5)
    M = np.full((7, 8, 9), 0.75, np.float32)
    A = about_center(rot((0, 0, 1), 10.0), M.shape, F.shape)
    rec = ar.normal_equations(F, M, A)
    assert rec.n > 0 and rec.see > 0
    assert not rec.b.any() and not rec.H.any()
    assert ar.lm_step(rec.n, rec.b, rec.H) is None                 # H_ii == 0: not positive definite


# ---- the host entries against the restatement ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


def spd_record(seed, scale=1.0):
    """a record as 200 voxels would make it: H = J^T J, b = J^T e, with the columns of J on the scales of the centred
    parameters (positions up to `scale` * 30)"""
    rng = np.random.default_rng(seed)
    J = rng.normal(0, 1, (200, 12)) * np.tile([30.0 * scale, 20.0 * scale, 10.0 * scale, 1.0], 3)
    e = rng.normal(0, 0.1, 200)
    return 200, float(e @ e), J.T @ e, J.T @ J


@pytest.mark.parametrize("mask", [0xFFF, 0x888, 0x001, 0x400, 0x5A5])
@pytest.mark.parametrize("lam", [0.0, 1e-3, 10.0])
def test_lm_step_against_numpy(hip, mask, lam):
    """delta solves K delta = -b on the free set (m parameters) by Cholesky.  Higham (Accuracy and Stability of
    Numerical Algorithms, theorem 10.4) gives (K + dK) delta = -b with |dK| <= gamma_(3m+1) |C| |C^T|, so the residual
    is at most gamma_(3m+1) || |C| |C^T| || ||delta||, and || |C| |C^T| ||_2 <= m ||K||_2; the issue's simpler form,
    8 m (m + 1) u (||K|| ||delta|| + ||b||), is larger than that for every m and is the bound asserted.  The same
    bound holds for numpy's solution, so the two differ by at most twice the bound in the residual."""
    n, see, b, H = spd_record(mask + int(lam * 7))
    got = hip.affine_lm_step(n, see, b, H, mask, lam)
    want = ar.lm_step(n, b, H, mask, lam)
    idx = ar.free_indices(mask)
    m = len(idx)
    assert got is not None and want is not None
    fixed = [i for i in range(12) if i not in idx]
    assert not got[fixed].any()
    Hf = H[np.ix_(idx, idx)]
    K = Hf + lam * np.diag(np.diag(Hf))
    bound = 8 * m * (m + 1) * U * (np.linalg.norm(K, 2) * np.linalg.norm(got[idx]) + np.linalg.norm(b[idx]))
    res = np.linalg.norm(K @ got[idx] + b[idx])
    print("mask %03x lambda %g: residual %.3g bound %.3g" % (mask, lam, res, bound))
    assert res <= bound
    assert np.linalg.norm(K @ (got[idx] - want[idx])) <= 2 * bound


def test_lm_step_refusals(hip):
    n, see, b, H = spd_record(9)
    assert hip.affine_lm_step(n, see, b, H, 0, 1e-3) is None                  # empty mask
    assert hip.affine_lm_step(n, see, b, H, 0x1000, 1e-3) is None             # a bit past the 12 parameters
    assert hip.affine_lm_step(0, see, b, H, 0xFFF, 1e-3) is None              # n == 0
    assert hip.affine_lm_step(n, see, b, H, 0xFFF, -1.0) is None
    assert hip.affine_lm_step(n, see, b, H, 0xFFF, float("nan")) is None
    Hz = H.copy()
    Hz[5, :] = Hz[:, 5] = 0.0                                                 # a zero diagonal entry
    assert hip.affine_lm_step(n, see, b, Hz, 0xFFF, 1e-3) is None
    assert hip.affine_lm_step(n, see, b, Hz, 0xFFF & ~(1 << 5), 1e-3) is not None     # unless it is not free
    assert hip.affine_lm_step(n, see, b, -H, 0xFFF, 1e-3) is None             # not positive definite
    L = hip.lib()
    d = (C.c_double * 12)()
    assert L.sift3d_amd_affine_lm_step(None, 0xFFF, 0.0, d) == -1
    rec = np.zeros(1, hip.AFFINE_RECORD_DTYPE)
    assert L.sift3d_amd_affine_lm_step(rec.ctypes.data, 0xFFF, 0.0, None) == -1


def test_apply_delta_equals_restatement_bit_for_bit(hip):
    rng = np.random.default_rng(12)
    for shape in ((48, 48, 48), (9, 20, 133), (1, 1, 1), (2, 3, 4)):
        A = about_center(rot((1, 2, 3), 11.0) * 1.05, shape, shape, shift=(1.5, -2.25, 0.3))
        delta = rng.normal(0, 0.01, 12)
        got = hip.affine_apply_delta(A, delta, shape)
        np.testing.assert_array_equal(got, ar.apply_delta(A, delta, shape))
        np.testing.assert_array_equal(hip.affine_apply_delta(A, np.zeros(12), shape)[:, :3], A[:, :3])
    with pytest.raises(ValueError):
        hip.affine_apply_delta(np.eye(3), np.zeros(12), (4, 4, 4))
    with pytest.raises(ValueError):
        hip.affine_apply_delta(np.eye(3, 4), np.zeros(12), (4, 0, 4))
    # a translation step moves every point by delta, whatever the centre
    got = hip.affine_apply_delta(np.eye(3, 4), [0, 0, 0, 1, 0, 0, 0, 2, 0, 0, 0, 3], (5, 6, 7))
    np.testing.assert_array_equal(got[:, 3], [1, 2, 3])


# ---- the device entries refuse bad arguments before any device call --------------------------------------------
@pytest.fixture(scope="module")
def bufs():
    """made-up addresses without a device; real allocations covering every range named below with one"""
    from sift3d_amd import api, hip
    if api.device_available():
        b = [hip.lib().sift3d_hip_malloc(1 << 21) for _ in range(4)]
        assert all(b)
        yield b
        for p in b:
            hip.lib().sift3d_hip_free(p)
    else:
        yield [0x10000000 * (k + 1) for k in range(4)]


def _a(A):
    a = np.ascontiguousarray(A, np.float64).reshape(12)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def test_symbols_exported(hip):
    from sift3d_amd import _native, api
    L = _native.load()
    for name in ("sift3d_hip_affine_normal_eqs", "sift3d_amd_affine_normal_work_bytes", "sift3d_amd_affine_lm_step",
                 "sift3d_amd_affine_apply_delta", "sift3d_amd_affine_refine_device",
                 "sift3d_amd_affine_refine_work_bytes", "sift3d_amd_affine_refine_default_params"):
        assert hasattr(L, name), name
    assert callable(hip.affine_normal_equations) and callable(api.refine_affine)
    W = hip.lib().sift3d_amd_affine_normal_work_bytes
    assert W(5, 6, 7) == hip.SIMILARITY_GRID * 74 * 8 == W(512, 512, 512)
    assert W(0, 6, 7) == 0 and W(5, -1, 7) == 0 and W(5, 6, 0) == 0
    R = hip.lib().sift3d_amd_affine_refine_work_bytes
    assert R(8, 8, 8, 8, 8, 8, 1) == W(8, 8, 8) + 1264
    assert R(8, 8, 8, 6, 6, 6, 2) == R(8, 8, 8, 6, 6, 6, 1) + 4 * 64 + 4 * 28
    assert R(8, 8, 8, 8, 8, 8, 0) == 0 and R(8, 8, 8, 8, 8, 8, 7) == 0 and R(8, 0, 8, 8, 8, 8, 1) == 0
    S = hip.lib().sift3d_amd_affine_refine_struct_bytes
    assert [S(k) for k in range(7)] == [C.sizeof(hip.AffineRefineParams), C.sizeof(hip.AffineEvaluation),
                                        C.sizeof(hip.AffineRefineResult), hip.AFFINE_NORMAL_BYTES,
                                        hip.AFFINE_MAX_EVALUATIONS, hip.AFFINE_MAX_LEVELS, 0]
    assert hip.AFFINE_RECORD_DTYPE.itemsize == S(3) and hip.affine_normal_work_bytes((7, 6, 5)) == W(5, 6, 7)
    p = hip.affine_refine_params()
    assert (p.free_mask, p.levels, p.max_evaluations) == (0xFFF, 1, 30)
    assert (p.lambda0, p.lambda_factor, p.lambda_min, p.lambda_max, p.tol, p.min_overlap) == \
        (1e-3, 10.0, 1e-9, 1e7, 1e-3, 0.5)


def test_normal_equations_refusals(hip, bufs):
    L = hip.lib()
    F, M, R, W = bufs
    keep, ident = _a(np.eye(3, 4))

    def call(F=F, o=(8, 8, 8), M=M, n=(8, 8, 8), A=ident, R=R, W=W):
        return L.sift3d_hip_affine_normal_eqs(F, *o, M, *n, A, R, W, None)
    work = hip.affine_normal_work_bytes()
    cases = [dict(F=None), dict(M=None), dict(A=None), dict(R=None), dict(W=None),
             dict(o=(0, 8, 8)), dict(o=(8, -1, 8)), dict(o=(8, 8, 0)), dict(n=(0, 8, 8)), dict(n=(8, 8, -2)),
             dict(F=F + 2), dict(M=M + 1), dict(R=R + 4), dict(W=W + 4),                              # misaligned
             dict(R=F), dict(R=M + 4 * 500), dict(W=M), dict(W=F + 4 * 510), dict(R=F + 4 * 511 - 1256),     # on inputs
             dict(R=W), dict(R=W + work - 8), dict(W=R + 1256), dict(W=R - work + 8),                 # on each other
             dict(o=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), F=F)]                                    # too many tiles
    for kw in cases:
        assert call(**kw) == -1, kw
    for v in (np.nan, np.inf, -np.inf):
        for k in (0, 7, 11):
            A = np.eye(3, 4).reshape(12)
            A[k] = v
            kept, bad = _a(A)
            assert call(A=bad) == -1, (v, k)


def test_refine_device_refusals(hip, bufs):
    L = hip.lib()
    F, M, R, W = bufs
    res = hip.AffineRefineResult()

    def call(F=F, o=(8, 8, 8), M=M, n=(8, 8, 8), A=np.eye(3, 4), res=C.byref(res), W=W, null_params=False, **kw):
        a, ptr = _a(A) if A is not None else (None, None)
        p = None if null_params else C.byref(hip.affine_refine_params(**kw))
        return L.sift3d_amd_affine_refine_device(F, *o, M, *n, ptr, p, res, W, None)
    nan, inf = float("nan"), float("inf")
    bad_A = np.eye(3, 4)
    bad_A[1, 2] = nan
    cases = [dict(F=None), dict(M=None), dict(A=None), dict(res=None), dict(W=None),
             dict(o=(0, 8, 8)), dict(n=(8, 8, -1)), dict(A=bad_A),
             dict(free_mask=0), dict(free_mask=0x1000), dict(levels=0), dict(levels=7),
             dict(max_evaluations=0), dict(max_evaluations=129),
             dict(lambda0=0.0), dict(lambda0=nan), dict(lambda_factor=1.0), dict(lambda_factor=inf),
             dict(lambda_min=0.0), dict(lambda_max=1e-4), dict(lambda_max=inf), dict(tol=-1.0), dict(tol=nan),
             dict(min_overlap=-0.1), dict(min_overlap=1.5), dict(min_overlap=nan),
             dict(F=F + 2), dict(M=M + 1), dict(W=W + 4), dict(W=F), dict(W=M + 4 * 511),
             dict(W=F - hip.affine_normal_work_bytes() - hip.AFFINE_NORMAL_BYTES)]
    for kw in cases:
        assert call(**kw) == -1, kw


def test_python_value_errors():
    from sift3d_amd import api
    v = np.zeros((5, 7, 9), np.float32)
    for kw in (dict(free="rigid"), dict(free=0), dict(free=0x1000), dict(free=1.5), dict(levels=0), dict(levels=7),
               dict(interp="nearest"), dict(A=np.eye(3)), dict(max_evaluations=0), dict(bogus=1)):
        with pytest.raises(ValueError):
            api.refine_affine(v, v, **kw)
    with pytest.raises(ValueError):
        api.refine_affine(v, np.zeros((7, 9), np.float32))
    if not api.device_available():
        with pytest.raises(RuntimeError):
            api.refine_affine(v, v)


# ---- the restatement's driver: the cases of the device test ---------------------------------------------------------
def biased_case(api, deg=3.0, shift=(1.5, -1.0, 0.5)):
    """fixed = synth_survey(48); T the true pull map (a rotation about (1, 2, 3) through the centre plus a shift);
    moving = fixed through T's inverse: the zero fill lies inside the moving grid, which biases the minimum"""
    if deg == 3.0:
        fixed, T, Tinv = end_to_end_case(api)
    else:
        fixed = np.ascontiguousarray(api.synth_survey(48), np.float32)
        T = about_center(rot((1, 2, 3), deg), fixed.shape, fixed.shape, shift=shift)
        Tinv = inverse(T)
    moving = ref_warp(fixed, Tinv, fixed.shape, "linear", 0.0)[0].astype(np.float32)
    return fixed, moving, T


def bias_free_case(api, t=(2.0, -1.0, 1.0)):
    """fixed = synth_survey(64)[8:56]^3; moving = the same crop of the survey pulled through the inverse of the integer
    translation t: no zero fill inside the moving grid, and the MSD at the truth is exactly 0"""
    S = np.ascontiguousarray(api.synth_survey(64), np.float32)
    T = np.eye(3, 4)
    T[:, 3] = t
    pulled = ref_warp(S, inverse(T), S.shape, "linear", 0.0)[0].astype(np.float32)
    crop = (slice(8, 56),) * 3
    return np.ascontiguousarray(S[crop]), np.ascontiguousarray(pulled[crop]), T


def check_descent(r, start_error, end_error):
    """the conditions of the biased case on a driver's result"""
    for l in set(r.levels.tolist()):
        acc = r.msd[(r.levels == l) & r.accepted]
        assert np.all(np.diff(acc) < 0), acc                       # accepted MSD values strictly decrease
    first, last = r.msd[0], r.msd[r.accepted][-1]
    print("msd %.6f -> %.6f (%.1fx), corner error %.3f -> %.3f (%.1fx), %d evaluations, stop %s"
          % (first, last, first / last, start_error, end_error, start_error / end_error, r.evaluations, r.stop))
    assert last <= first / 10
    assert end_error <= start_error / 3


@pytest.fixture(scope="module")
def api():
    from sift3d_amd import api as a
    a.lib()
    return a


def test_driver_biased_case(api):
    """3 degrees + (1.5, -1, 0.5) from the identity.  Measured on the restatement: msd 0.016109 -> 0.000582 (27.7x),
    corner error 3.991 -> 0.911 (4.4x), 7 evaluations, converged."""
    fixed, moving, T = biased_case(api)
    r = ar.refine(fixed, moving)
    check_descent(r, ar.corner_distance(np.eye(3, 4), T, fixed.shape), ar.corner_distance(r.A, T, fixed.shape))
    assert r.stop == "converged"


def test_driver_bias_free_translation(api):
    """An integer translation, translation only: the MSD at the truth is exactly 0 and the driver, which stops on a
    step below tol and converges quadratically there, ends within 10 tol of it (measured: 3.6e-8 voxel after 5
    evaluations)."""
    fixed, moving, T = bias_free_case(api)
    assert ar.normal_equations(fixed, moving, T, exact=False).see == 0.0
    r = ar.refine(fixed, moving, free_mask=0x888)
    err = ar.corner_distance(r.A, T, fixed.shape)
    print("corner error %.3g after %d evaluations, stop %s" % (err, r.evaluations, r.stop))
    assert err <= 10 * TOL
    np.testing.assert_array_equal(r.A[:, :3], np.eye(3))


def test_driver_levels(api):
    """10 degrees + (8, -6, 4): three levels end where one level does, with fewer evaluations at level 0 (measured:
    18 against 30, the two final maps 0.0024 voxel apart at the corners)."""
    fixed, moving, T = biased_case(api, 10.0, (8.0, -6.0, 4.0))
    one = ar.refine(fixed, moving)
    three = ar.refine(fixed, moving, levels=3)
    apart = ar.corner_distance(one.A, three.A, fixed.shape)
    n1, n3 = int((one.levels == 0).sum()), int((three.levels == 0).sum())
    print("level-0 evaluations %d against %d, final maps %.3g apart" % (n3, n1, apart))
    assert apart <= 10 * TOL
    assert n3 < n1
    assert three.levels.tolist() == sorted(three.levels.tolist(), reverse=True)      # coarsest first
