"""The landmark contract without a device (include/sift3d_amd.h, "FFD landmarks"): the restatement
(tests/ffd_landmarks_restatement.py) against analysis, the inside rule at its edges, the exported symbols and layouts,
every refusal of the three entries before any device call, the Python ValueErrors, and the restatement's driver with the
term on the pair the device test uses."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import ffd_landmarks_restatement as lr
from tests import ffd_restatement as fr
from tests.demons_restatement import gamma
from tests.test_ffd_host import DRIVER, affine_lattice, driver_pair, restatement_driver

U = 2.0 ** -53
U32 = 2.0 ** -24


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


# ---- the restatement against analysis ----------------------------------------------------------------------------
def test_affine_lattice_reproduces_the_affine_function_at_points():
    """Cubic B-splines reproduce an affine function sampled at the knots at every point of the support.  In double the
    64 terms carry 3 roundings each and the sum 63 more (gamma_66 sum |term| <= 67 u max |c|: the weights are not
    negative and sum to 1); each weight's polynomial is evaluated with at most 8 roundings of quantities <= 4, so it is
    within 40 u of its exact value and the 64 products of three of them within 64 * 3 * 40 u in all; the lattice itself
    is rounded to float32 (u32 max |c|, weighted by weights that sum to 1).  (u32 + 8000 u) max |c| covers it."""
    out_shape, spacing = (9, 14, 21), (4, 3, 2)
    Lm = [[0.01, -0.02, 0.005], [0.0, 0.03, -0.01], [-0.015, 0.0, 0.02]]
    t = [0.5, -1.25, 2.0]
    c = affine_lattice(out_shape, spacing, Lm, t)
    rng = np.random.default_rng(3)
    P = rng.uniform(0, 1, (500, 3)) * (np.array(out_shape[::-1]) - 1.0)
    s, inside = lr.spline(c.astype(np.float32), spacing, P)
    assert inside.all()
    want = np.stack([Lm[k][0] * P[:, 0] + Lm[k][1] * P[:, 1] + Lm[k][2] * P[:, 2] + t[k] for k in range(3)], axis=1)
    off = np.abs(s - want).max()
    print("affine lattice at 500 points: off %.3g, bound %.3g" % (off, (U32 + 8000 * U) * np.abs(c).max()))
    assert off <= (U32 + 8000 * U) * np.abs(c).max()


@pytest.mark.parametrize("out_shape,spacing", [((5, 9, 17), (4, 3, 2)), ((3, 4, 5), (8, 8, 8)), ((5, 6, 33), (1, 1, 1))])
def test_whole_voxel_points_agree_with_the_voxel_spline(out_shape, spacing):
    """the voxel table is the same weights rounded to float32 and the voxel sum is float32: 64 * 2^-24 max |c|"""
    rng = np.random.default_rng(4)
    c = rng.uniform(-1.5, 1.5, fr.lattice_shape(out_shape, spacing)).astype(np.float32)
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in out_shape), indexing="ij")
    P = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    s, inside = lr.spline(c, spacing, P)
    assert inside.all()
    want = fr.spline(c, spacing, out_shape).astype(np.float64).reshape(3, -1).T
    assert np.abs(s - want).max() <= 64 * U32 * np.abs(c).max()


def case(seed=0, m=40, out_shape=(7, 10, 19), spacing=(3, 4, 5), integer=False):
    rng = np.random.default_rng(seed)
    shape = fr.lattice_shape(out_shape, spacing)
    c = (rng.integers(-128, 129, shape) / 64.0).astype(np.float32) if integer else \
        rng.uniform(-1.5, 1.5, shape).astype(np.float32)
    P = rng.uniform(0, 1, (m, 3)) * (np.array(out_shape[::-1]) - 1.0)
    Q = P + rng.uniform(-2, 2, (m, 3))
    w = rng.uniform(0, 2, m)
    return c, spacing, P, Q, w


def test_adjoint_identity():
    """<GL, c'> = sum_i w_i r_i . s'(P_i) for any lattice c': both sides sum the same products (w W r) c' up to
    rounding, each within gamma_(64 + m + 8) of sum |GL term| |c'|"""
    c, spacing, P, Q, w = case(1)
    rec = lr.landmarks(c, spacing, P, Q, w)
    rng = np.random.default_rng(2)
    c2 = rng.standard_normal(c.shape).astype(np.float32)
    s2, _ = lr.spline(c2, spacing, P)
    lhs = float((rec.GL * c2.astype(np.float64)).sum())
    rhs = float((w[:, None] * rec.r * s2).sum())
    bound = 2 * gamma(64 + len(P) + 8) * float((rec.GL_terms * np.abs(c2)).sum())
    print("adjoint identity: %.17g against %.17g, bound %.3g" % (lhs, rhs, bound))
    assert abs(lhs - rhs) <= bound and rec.support.sum() == 64 * len(P)


def test_gradient_is_the_central_difference_of_the_value():
    """lambda L = lambda S / Omega is a quadratic form of the lattice, so its central difference is exact up to
    rounding.  The lattice holds multiples of 1/64, so c + h and c - h are exact in float32.  S's sum is correctly
    rounded and each term carries at most 80 roundings (the spline's 64 terms of 4, the pull, the squares), so a value
    is within gamma_100 of itself and the quotient within gamma_100 (V+ + V-) / (2 h); the analytic side is within
    gamma_100 of its sum |term|."""
    lam, h = 0.37, 0.125
    c, spacing, P, Q, w = case(5, integer=True)
    base = lr.landmarks(c, spacing, P, Q, w)
    assert base.counted == len(P)
    rng = np.random.default_rng(6)
    picks = [(d,) + tuple(rng.integers(0, n) for n in c.shape[1:]) for d in range(3) for _ in range(4)]
    picks += [(0, 1, 1, 1), (2,) + tuple(n - 2 for n in c.shape[1:])]
    hit = 0
    for pick in picks:
        V = []
        for sgn in (1.0, -1.0):
            cc = c.copy()
            cc[pick] += np.float32(sgn * h)
            rec = lr.landmarks(cc, spacing, P, Q, w)
            V.append(lam * rec.S / rec.Omega)
        fd = (V[0] - V[1]) / (2 * h)
        got = lam * 2.0 / base.Omega * base.GL[pick]
        bound = gamma(100) * (V[0] + V[1]) / (2 * h) + gamma(100) * lam * 2.0 / base.Omega * base.GL_terms[pick]
        assert abs(fd - got) <= bound, (pick, fd, got, bound)
        hit += got != 0.0
    assert hit >= 6


def test_inside_rule_at_its_edges():
    """0 <= x < (g - 3) delta: x = 0 (and -0.0), x = o - 1, just below and exactly at (g - 3) delta, negative, NaN and
    both infinities"""
    o, delta = 17, 4
    g = fr.lattice_dim(o, delta)
    top = float((g - 3) * delta)
    xs = np.array([0.0, -0.0, o - 1.0, np.nextafter(top, 0.0), top, -1e-300, -0.5, -1e300, np.nan,
                   np.inf, -np.inf, 1e300])
    i0, w, inside = lr.point_axis(xs, delta, g)
    assert inside.tolist() == [True, True, True, True, False, False, False, False, False, False, False, False]
    assert i0[:4].tolist() == [0, 0, 4, g - 4] and top >= o
    assert np.all(np.abs(w.sum(axis=1) - 1.0) <= 8 * U) and np.all(w >= 0)
    c = np.ones(fr.lattice_shape((5, 9, o), (delta, 3, 2)), np.float32)
    P = np.stack([xs, np.full(len(xs), 2.5), np.full(len(xs), 1.25)], axis=1)
    T, ins = lr.points(c, (delta, 3, 2), P)
    assert ins.tolist() == inside.tolist() and np.isnan(T[~ins]).all() and not np.isnan(T[ins]).any()
    rec = lr.landmarks(c, (delta, 3, 2), P, np.zeros_like(P))
    assert rec.counted == 4 and not rec.r[~ins].any() and np.isfinite(rec.S) and np.isfinite(rec.GL).all()
    none = lr.landmarks(c, (delta, 3, 2), P[4:], np.zeros_like(P[4:]))
    assert (none.counted, none.S, none.Omega, none.rmax) == (0, 0.0, 0.0, 0.0) and not none.GL.any()
    assert lr.term(none) == (0.0, 0.0)


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
    for name in ("sift3d_hip_ffd_points", "sift3d_hip_ffd_landmarks", "sift3d_amd_ffd_landmarks_work_bytes",
                 "sift3d_amd_ffd_landmarks_struct_bytes", "sift3d_amd_ffd_refine_landmarks_work_bytes",
                 "sift3d_amd_ffd_evaluate_landmarks_bytes", "sift3d_hip_ffd_evaluate_landmarks",
                 "sift3d_amd_ffd_refine_landmarks_device"):
        assert hasattr(L, name), name
    for f in ("ffd_transform_points", "FFDLandmarkTerm"):
        assert hasattr(api, f), f
    for f in ("ffd_points", "ffd_landmarks", "ffd_refine_landmarks"):
        assert callable(getattr(hip, f)), f
    L = hip.lib()
    S = L.sift3d_amd_ffd_landmarks_struct_bytes
    assert [S(k) for k in range(5)] == [C.sizeof(hip.FFDLandmarkTerm), 32, 65536, 6 * 128, 0]
    assert C.sizeof(hip.FFDLandmarkTerm) == 24 and hip.FFD_MAX_LANDMARKS == lr.MAX_LANDMARKS
    W = L.sift3d_amd_ffd_landmarks_work_bytes
    assert W(1, 4, 4, 4) > 0 and W(300, 9, 9, 9) % 16 == 0 and W(65536, 35, 35, 35) > W(65535, 35, 35, 35)
    assert W(0, 4, 4, 4) == 0 and W(65537, 4, 4, 4) == 0 and W(1, 3, 4, 4) == 0 and W(1, 4, 4, 0) == 0
    D = L.sift3d_amd_ffd_refine_landmarks_work_bytes
    J = L.sift3d_amd_ffd_refine_jacobian_work_bytes
    full = D(48, 48, 48, 48, 48, 48, 8, 8, 8, 2, 300)
    assert full >= J(48, 48, 48, 48, 48, 48, 8, 8, 8, 2) + 32 + 3 * 9 ** 3 * 8 + W(300, 9, 9, 9)
    assert D(48, 48, 48, 48, 48, 48, 8, 8, 8, 2, 0) == 0 and D(48, 48, 48, 48, 48, 48, 8, 8, 8, 7, 300) == 0
    assert D(48, 48, 48, 48, 48, 48, 8, 0, 8, 2, 300) == 0 and D(0, 48, 48, 48, 48, 48, 8, 8, 8, 2, 300) == 0


def _a(A):
    a = np.ascontiguousarray(A, np.float64).reshape(12)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


BAD_A = np.eye(3, 4)
BAD_A[2, 1] = np.inf


def test_points_refusals(hip, bufs):
    L = hip.lib()
    c, P_, T_ = bufs[:3]

    def call(c=c, g=(5, 5, 5), d=(8, 8, 8), A=None, P=P_, m=10, T=T_):
        keep, ptr = _a(A) if A is not None else (None, None)
        return L.sift3d_hip_ffd_points(c, *g, *d, ptr, P, m, T, None)
    cases = [dict(c=None), dict(P=None), dict(T=None), dict(g=(3, 5, 5)), dict(g=(5, 5, 0)), dict(d=(0, 8, 8)),
             dict(d=(8, 8, 257)), dict(m=0), dict(m=-1), dict(A=BAD_A), dict(c=c + 2), dict(P=P_ + 4), dict(T=T_ + 4),
             dict(T=c), dict(T=c + 4 * 374), dict(T=P_), dict(T=P_ + 8 * 29), dict(T=P_ - 8 * 29)]
    for kw in cases:
        assert call(**kw) == -1, kw


def _pts(m=10, bad=None):
    P = np.arange(3.0 * m).reshape(m, 3) % 7
    Q = P + 0.5
    w = np.ones(m)
    if bad == "Q":
        Q[m // 2, 1] = np.nan
    if bad == "Qinf":
        Q[0, 0] = np.inf
    if bad == "wneg":
        w[m - 1] = -1e-300
    if bad == "wnan":
        w[0] = np.nan
    if bad == "winf":
        w[1] = np.inf
    return P, Q, w


def test_landmarks_refusals(hip, bufs):
    L = hip.lib()
    c, W_, R_, r_, G_ = bufs[:5]

    def call(c=c, g=(5, 5, 5), d=(8, 8, 8), A=None, m=10, bad=None, P=True, Q=True, w=True, W=W_, R=R_, r=r_, G=G_):
        keep, ptr = _a(A) if A is not None else (None, None)
        Pa, Qa, wa = _pts(max(m, 1), bad)
        return L.sift3d_hip_ffd_landmarks(c, *g, *d, ptr, Pa.ctypes.data if P else None, Qa.ctypes.data if Q else None,
                                          wa.ctypes.data if w else None, m, W, R, r, G, None)
    cases = [dict(c=None), dict(P=False), dict(Q=False), dict(W=None), dict(R=None), dict(g=(3, 5, 5)),
             dict(g=(5, 0, 5)), dict(d=(8, 0, 8)), dict(d=(300, 8, 8)), dict(A=BAD_A), dict(m=0), dict(m=-3),
             dict(bad="Q"), dict(bad="Qinf"), dict(bad="wneg"), dict(bad="wnan"), dict(bad="winf"),
             dict(c=c + 2), dict(R=R_ + 4), dict(r=r_ + 4), dict(G=G_ + 4), dict(W=W_ + 8),
             dict(R=c), dict(W=c), dict(r=c + 4 * 374), dict(G=c), dict(r=R_), dict(G=R_ + 24), dict(R=W_ + 64),
             dict(G=r_ + 8 * 29)]
    for kw in cases:
        assert call(**kw) == -1, kw
    big = np.zeros((65537, 3))
    assert L.sift3d_hip_ffd_landmarks(c, 5, 5, 5, 8, 8, 8, None, big.ctypes.data, big.ctypes.data, None, 65537, W_, R_,
                                      None, None, None) == -1


def test_evaluate_landmarks_refusals(hip, bufs):
    L = hip.lib()
    F, M, c, U_, R, G, W = bufs
    B = L.sift3d_amd_ffd_evaluate_landmarks_bytes
    assert B(0, 10, 9, 9, 9, 8, 8, 8) == 32 + 3 * 125 * 8 + L.sift3d_amd_ffd_landmarks_work_bytes(10, 5, 5, 5)
    assert B(1, 10, 9, 9, 9, 8, 8, 8) == 32 + 3 * 125 * 8 + L.sift3d_amd_jacobian_penalty_work_bytes(9, 9, 9)
    assert B(0, 0, 8, 8, 8, 8, 8, 8) == 0 and B(2, 10, 8, 8, 8, 8, 8, 8) == 0 and B(1, 10, 8, 0, 8, 8, 8, 8) == 0
    lm_, jac_ = G + (1 << 21), W + (1 << 21)                             # the second halves of two of the buffers

    def call(F=F, o=(9, 9, 9), M=M, n=(9, 9, 9), c=c, g=(5, 5, 5), d=(8, 8, 8), A=None, bend=0.0, U=U_, R=R, G=G, W=W,
             jw=0.0, jac=jac_, m=10, bad=None, P=True, lam=0.5, lm=lm_):
        keep, ptr = _a(A) if A is not None else (None, None)
        Pa, Qa, wa = _pts(max(m, 1), bad)
        return L.sift3d_hip_ffd_evaluate_landmarks(F, *o, M, *n, c, *g, *d, ptr, bend, U, R, G, W, None, None, None, jw,
                                                   jac, Pa.ctypes.data if P else None, Qa.ctypes.data, wa.ctypes.data,
                                                   m, lam, lm)
    nan = float("nan")
    cases = [dict(F=None), dict(c=None), dict(U=None), dict(R=None), dict(G=None), dict(W=None), dict(lm=None),
             dict(o=(0, 8, 8)), dict(n=(8, 0, 8)), dict(d=(300, 8, 8)), dict(g=(5, 4, 5)), dict(A=BAD_A), dict(bend=-1.0),
             dict(jw=-1.0), dict(jw=nan), dict(jw=0.5, jac=None), dict(jw=0.5, A=np.zeros((3, 4))), dict(lam=-1.0),
             dict(lam=nan), dict(m=0), dict(m=65537), dict(P=False), dict(bad="Q"), dict(bad="wneg"), dict(F=F + 2),
             dict(lm=lm_ + 4), dict(jac=jac_ + 4), dict(W=W + 8), dict(lm=F), dict(lm=c), dict(lm=U_), dict(lm=R),
             dict(lm=G), dict(lm=W), dict(jac=M), dict(jac=lm_ + 64), dict(U=F)]
    for kw in cases:
        assert call(**kw) == -1, kw


def test_refine_landmarks_refusals(hip, bufs):
    L = hip.lib()
    F, M, c, U_, _, _, W = bufs
    res = hip.FFDRefineResult()
    pen = (hip.FFDPenalty * (6 * 128))()
    terms = (hip.FFDLandmarkTerm * (6 * 128))()
    sim = hip.Similarity()

    def call(F=F, o=(8, 8, 8), M=M, n=(8, 8, 8), A=None, res=C.byref(res), c=c, U=U_, W=W, WF=None, WM=None, bins=0,
             ranges=(0.0, 1.0, 0.0, 1.0), sim=C.byref(sim), jac=0.0, pen=pen, m=10, bad=None, P=True, Q=True, lam=0.01,
             terms=terms, null_params=False, **kw):
        keep, ptr = _a(A) if A is not None else (None, None)
        p = None if null_params else C.byref(hip.ffd_refine_params(**kw))
        Pa, Qa, wa = _pts(max(m, 1), bad)
        return L.sift3d_amd_ffd_refine_landmarks_device(F, *o, M, *n, ptr, p, res, c, U, W, None, WF, WM, bins, *ranges,
                                                        sim, jac, pen, Pa.ctypes.data if P else None,
                                                        Qa.ctypes.data if Q else None, wa.ctypes.data, m, lam, terms)
    nan, inf = float("nan"), float("inf")
    singular = np.zeros((3, 4))
    cases = [dict(F=None), dict(M=None), dict(res=None), dict(c=None), dict(U=None), dict(W=None),
             dict(o=(0, 8, 8)), dict(n=(8, 8, -1)), dict(A=BAD_A), dict(levels=0), dict(levels=7),
             dict(max_evaluations=0), dict(max_evaluations=129), dict(bending=-1.0), dict(step0=0.0), dict(tol=nan),
             dict(spacing=(8, 8, 8), F=F + 2), dict(W=W + 8), dict(W=F), dict(c=F), dict(U=M),
             dict(terms=None), dict(P=False), dict(Q=False), dict(m=0), dict(m=65537), dict(bad="Q"), dict(bad="wneg"),
             dict(bad="wnan"), dict(lam=-0.5), dict(lam=nan), dict(lam=inf), dict(jac=-1.0), dict(jac=nan),
             dict(jac=0.5, pen=None), dict(A=singular), dict(bins=32, sim=None), dict(bins=3),
             dict(bins=32, ranges=(1.0, 1.0, 0.0, 1.0))]
    for kw in cases:
        assert call(**kw) == -1, kw


def test_python_value_errors():
    from sift3d_amd import api
    v = np.zeros((5, 7, 9), np.float32)
    P = np.ones((4, 3))
    for lm, kw in ((P, {}), ((P,), {}), ((P, P[:3]), {}), ((P[:, :2], P[:, :2]), {}), ((P[:0], P[:0]), {}),
                   ((np.ones((65537, 3)), np.ones((65537, 3))), {}), ((P, P * np.nan), {}), ((P, P, np.ones(3)), {}),
                   ((P, P, -np.ones(4)), {}), ((P, P, np.full(4, np.inf)), {}), ((P, P), dict(landmark_weight=-1.0)),
                   ((P, P), dict(landmark_weight=float("nan"))), ((P, P), dict(features="descriptors"))):
        with pytest.raises(ValueError):
            api.refine_ffd(v, v, landmarks=lm, **kw)
    with pytest.raises(ValueError):
        api.refine_ffd(np.zeros((2, 5, 7, 9), np.float32), np.zeros((2, 5, 7, 9), np.float32), landmarks=(P, P))
    lat = np.zeros((3, 4, 4, 4), np.float32)
    for args in ((lat, 0, P), (lat, 8, P[:, :2]), (lat[:2], 8, P), (lat, 8, P, np.eye(3))):
        with pytest.raises(ValueError):
            api.ffd_transform_points(*args)
    T, inside = api.ffd_transform_points(lat, 8, np.zeros((0, 3)))
    assert T.shape == (0, 3) and inside.shape == (0,)
    if not api.device_available():
        with pytest.raises(RuntimeError):
            api.ffd_transform_points(lat, 8, P)
        with pytest.raises(RuntimeError):
            api.refine_ffd(v, v, landmarks=(P, P))


# ---- the driver ---------------------------------------------------------------------------------------------------
LANDMARKS = 300
WEIGHT = 0.01


@functools.lru_cache(maxsize=None)
def driver_landmarks():
    """300 exact correspondences of driver_pair(): P ~ U[0, 47]^3, Q = P + truth(P) from the analytic field (the
    fixed-point iteration of driver_pair on the points themselves)"""
    F, _, _ = driver_pair()
    m = F.shape[0]
    P = np.random.default_rng(0).uniform(0.0, 47.0, (LANDMARKS, 3))

    def w_at(q):
        return 2.0 * np.stack([np.sin(2 * np.pi * q[:, 1] / m), np.sin(2 * np.pi * q[:, 2] / m),
                               np.sin(2 * np.pi * q[:, 0] / m)], axis=1)
    u = np.zeros_like(P)
    for _ in range(60):
        u = -w_at(P + u)
    assert np.abs(u + w_at(P + u)).max() < 1e-9
    return P, P + u


def landmark_rms(lattice, spacing, A=None):
    """RMS distance between the mapped fixed landmarks and the moving ones (the restatement's points)"""
    P, Q = driver_landmarks()
    T, inside = lr.points(lattice, spacing, P, A)
    assert inside.all()
    return float(np.sqrt(((T - Q) ** 2).sum(axis=1).mean()))


def field_rms(fld, truth):
    inner = (slice(None),) + (slice(4, -4),) * 3
    return float(np.sqrt(((np.asarray(fld, np.float64) - truth)[inner] ** 2).sum(axis=0).mean()))


@functools.lru_cache(maxsize=None)
def restatement_landmarks_only():
    F, _, truth = driver_pair()
    P, Q = driver_landmarks()
    flat = np.full(F.shape, 0.5, np.float32)
    return lr.refine(flat, flat, P, Q, None, 1.0, None, DRIVER["spacing"], DRIVER["levels"], DRIVER["bending"], None,
                     DRIVER["max_evaluations"])


@functools.lru_cache(maxsize=None)
def restatement_with_landmarks():
    F, M, truth = driver_pair()
    P, Q = driver_landmarks()
    return lr.refine(F, M, P, Q, None, WEIGHT, None, DRIVER["spacing"], DRIVER["levels"], DRIVER["bending"], None,
                     DRIVER["max_evaluations"])


def test_restatement_driver_landmarks_only():
    """constant volumes: the image term is 0 and the landmarks alone pull the lattice.  The float64 prototype reached
    L_last / L_first = 0.0013 and an RMS field error of 0.109 voxels (the truth's own RMS is 2.45)."""
    _, _, truth = driver_pair()
    r = restatement_landmarks_only()
    lv0 = [(e, t) for e, t in zip(r.trail, r.landmarks) if e[6] == 0 and e[5]]
    first = [t for e, t in zip(r.trail, r.landmarks) if e[6] == DRIVER["levels"] - 1][0]
    ratio, rms = lv0[-1][1][0] / first[0], field_rms(r.field, truth)
    print("landmarks only: stop %s, %d evaluations, L %.4g -> %.4g (ratio %.4g), RMS field error %.4g voxels"
          % (r.stop, len(r.trail), first[0], lv0[-1][1][0], ratio, rms))
    assert all(t[2] == LANDMARKS for t in r.landmarks) and all(e[1] == 0.0 for e in r.trail)
    assert ratio < 0.01 and rms < 0.25


def test_restatement_driver_with_landmarks_halves_both_errors():
    """image and landmarks at lambda = 0.01 against the image-only restatement driver: the RMS field error and the RMS
    landmark residual are both at most half of the image-only run's (the prototype's ratios were 0.32 and 0.18)."""
    _, _, truth = driver_pair()
    ref, (_, rms_ref) = restatement_driver()
    r = restatement_with_landmarks()
    rms = field_rms(r.field, truth)
    res, res_ref = landmark_rms(r.lattice, DRIVER["spacing"]), landmark_rms(ref.lattice, DRIVER["spacing"])
    print("image + landmarks (lambda %g): RMS field error %.4g against %.4g (ratio %.3g), RMS landmark residual %.4g "
          "against %.4g (ratio %.3g)" % (WEIGHT, rms, rms_ref, rms / rms_ref, res, res_ref, res / res_ref))
    for e, t in zip(r.trail, r.landmarks):
        assert t[2] == LANDMARKS and abs(e[0] - ((e[1] + DRIVER["bending"] * e[2]) + WEIGHT * t[0])) <= 1e-12 * abs(e[0])
    assert rms <= 0.5 * rms_ref and res <= 0.5 * res_ref
