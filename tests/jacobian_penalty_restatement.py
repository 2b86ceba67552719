"""numpy restatement of "Jacobian penalty" (include/sift3d_amd.h).

penalty(u, ref, dtype): dtype float32 is the header's arithmetic, the float j of "Displacement fields" widened to
float64 and everything after it float64 in the stated order, so that nonpos, rmin, rmax, every phi and every entry of S
carry the device's bits; `sum` is correctly rounded (math.fsum), so that a bound on the device's sum need not allow for
the reference's own error.  dtype float64 is the same formulas on a float64 j: the smooth function whose calculus the
host tests check.  refine(...) is tests/ffd_restatement.py's (tests/ffd_mi_restatement.py's) driver with the third term,
built from those modules' functions."""
import collections
import math

import numpy as np

from tests import ffd_mi_restatement as fm
from tests import ffd_restatement as fr
from tests import mask_restatement as mr
from tests import affine_mi_restatement as am

F32 = np.float32
Penalty = collections.namedtuple("Penalty", "P sum sum_abs nonpos rmin rmax r phi S")
Refinement = collections.namedtuple("Refinement", "lattice field trail stop penalty")


def phi_of(r):
    """(phi, phi') of float64 r, elementwise, the header's two branches"""
    r = np.asarray(r, np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        hi = (r + 1.0 / r) - 2.0
        dhi = 1.0 - 1.0 / (r * r)
        t = r - 0.25
        lo = (2.25 - 15.0 * t) + 64.0 * (t * t)
        dlo = -15.0 + 128.0 * t
    up = r >= 0.25
    return np.where(up, hi, lo), np.where(up, dhi, dlo)


def _gradient(u, ax, dtype):
    """numpy.gradient's rule along array axis ax in `dtype`: (u[i+1] - u[i-1]) * 0.5 inside, one-sided ends, 0 on an
    axis of length 1"""
    n = u.shape[ax]
    g = np.zeros(u.shape, dtype)
    if n == 1:
        return g
    v, w = np.moveaxis(u, ax, 0), np.moveaxis(g, ax, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        w[1:-1] = ((v[2:] - v[:-2]).astype(dtype) * dtype(0.5)).astype(dtype)
        w[0] = (v[1] - v[0]).astype(dtype)
        w[-1] = (v[-1] - v[-2]).astype(dtype)
    return g


def jacobian(u, dtype=F32):
    """j[d][e] float64 [oz, oy, ox], e = 0, 1, 2 the x, y, z axes: (d == e) + g_de formed in `dtype`"""
    u = np.ascontiguousarray(u, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        return [[((dtype(1.0) if d == e else dtype(0.0)) + _gradient(u[d], 2 - e, dtype)).astype(dtype)
                 .astype(np.float64) for e in range(3)] for d in range(3)]


def det_of(j):
    with np.errstate(invalid="ignore", over="ignore"):
        return j[0][0] * (j[1][1] * j[2][2] - j[1][2] * j[2][1]) - j[0][1] * (j[1][0] * j[2][2] - j[1][2] * j[2][0]) + \
            j[0][2] * (j[1][0] * j[2][1] - j[1][1] * j[2][0])


def cofactor(j, d, e):
    d1, d2 = [k for k in range(3) if k != d]
    e1, e2 = [k for k in range(3) if k != e]
    with np.errstate(invalid="ignore", over="ignore"):
        if (d + e) % 2 == 0:
            return j[d1][e1] * j[d2][e2] - j[d2][e1] * j[d1][e2]
        return j[d2][e1] * j[d1][e2] - j[d1][e1] * j[d2][e2]


def sum_form(a, j):
    """S [3, oz, oy, ox] float64: the header's terms in its order (axis e ascending, then p ascending)"""
    S = np.zeros((3,) + a.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        for e in range(3):
            ax = 2 - e
            n = a.shape[ax]
            if n == 1:
                continue
            for d in range(3):
                K = np.moveaxis(a * cofactor(j, d, e), ax, 0)                # K_de(p), p along the leading axis
                s = np.moveaxis(S[d], ax, 0)                                 # a view: S_d(q)
                # p = q - 1: coefficient 1/2, 1 when p == 0
                s[1:2] = s[1:2] + K[0:1] * 1.0
                s[2:] = s[2:] + K[1:-1] * 0.5
                # p = q at the two ends
                s[0] = s[0] + K[0] * -1.0
                s[-1] = s[-1] + K[-1] * 1.0
                # p = q + 1: coefficient -1/2, -1 when p == n - 1
                s[:-2] = s[:-2] + K[1:-1] * -0.5
                s[-2:-1] = s[-2:-1] + K[-1:] * -1.0
    return S


def penalty(u, ref=1.0, dtype=F32):
    """Penalty(P, sum, sum |phi|, nonpos, rmin, rmax, r, phi, S) of a field u [3, oz, oy, ox]"""
    ref = np.float64(ref)
    j = jacobian(u, dtype)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        r = det_of(j) / ref
        phi, dphi = phi_of(r)
        a = dphi / ref
    S = sum_form(a, j)
    ok = ~np.isnan(r)
    total = math.fsum(phi.reshape(-1).tolist())
    return Penalty(total / r.size, total, float(np.abs(phi).sum()), int((~(r > 0)).sum()),
                   float(r[ok].min()) if ok.any() else float("inf"), float(r[ok].max()) if ok.any() else float("-inf"),
                   r, phi, S)


def ref_of(A):
    """the determinant of A's linear part in the header's order; 1.0 without A"""
    if A is None:
        return 1.0
    A = np.asarray(A, np.float64).reshape(-1)
    return float(A[0] * (A[5] * A[10] - A[6] * A[9]) - A[1] * (A[4] * A[10] - A[6] * A[8]) +
                 A[2] * (A[4] * A[9] - A[5] * A[8]))


def lattice_gradient(S, spacing, exact=False):
    """GJ [3, gz, gy, gx]: S through the adjoint of the spline"""
    return np.stack([fr.adjoint(Sd, spacing, exact)[0] for Sd in S])


def refine(F, M, A=None, spacing=8, levels=3, bending_weight=0.005, jacobian_weight=0.0, max_evaluations=60,
           metric="msd", bins=32, range_f=None, range_m=None, WF=None, WM=None, step0=1.0, step_max=4.0, tol=0.01,
           min_overlap=0.5):
    """the header's driver with E = (image + bending R) + jacobian P and the third term of the gradient; trail entries
    as ffd_restatement.refine's (metric "mi": ffd_mi_restatement.refine's), penalty one (P, rmin, nonpos) per entry.
    With metric "msd" the masks are not restated (None only)."""
    A = None if A is None else np.array(A, np.float64).reshape(3, 4)
    ref = ref_of(A)
    mi = metric == "mi"
    assert mi or (WF is None and WM is None)
    ranges = (fm.own_range(F) if range_f is None else range_f, fm.own_range(M) if range_m is None else range_m)
    Fs, Ms, WFs, WMs = (mr.pyramid(v, levels) for v in (F, M, WF, WM))
    for _ in range(1, levels):
        if A is not None:
            A[:, 3] = A[:, 3] * 0.5
    trail, pens, stop, c = [], [], 1, None

    def cost(image, R, pen):
        two = image + bending_weight * R
        return two + jacobian_weight * pen.P if jacobian_weight > 0 else two

    def ev(l, lat):
        """(n, image, R, penalty, what the gradient needs)"""
        u = fr.field(lat, spacing, Fs[l].shape, A)
        pen = penalty(u, ref)
        if mi:
            hist, n = fm.histogram_field(Fs[l], Ms[l], u, bins, ranges[0], ranges[1], WFs[l], WMs[l])
            m = am.measures(hist)
            return n, m.cost, fr.bending(lat, spacing)[0], pen, m
        rec, _ = fr.evaluate(Fs[l], Ms[l], lat, spacing, A, exact=False)
        return rec.n, (rec.see / rec.n if rec.n else float("nan")), fr.bending(lat, spacing)[0], pen, rec

    def grad_at(l, lat, pen, aux):
        dR = fr.bending(lat, spacing)[1]
        if mi:
            rec, _ = fm.evaluate(Fs[l], Ms[l], lat, spacing, A, aux.W, bins, ranges, WFs[l], WMs[l], exact=False)
            scale = 1.0
        else:
            rec, scale = aux, 2.0
        with np.errstate(divide="ignore", invalid="ignore"):
            g = (scale / np.float64(rec.n)) * rec.Gc + bending_weight * dR
            if jacobian_weight > 0:
                g = g + (jacobian_weight / np.float64(pen.r.size)) * lattice_gradient(pen.S, spacing)
        g = g.astype(F32)
        return g, float(np.abs(g).max())

    for l in range(levels - 1, -1, -1):
        shape = Fs[l].shape
        c = np.zeros(fr.lattice_shape(shape, spacing), F32) if c is None else fr.refine2(c, shape, spacing)
        s = step0
        n, image, R, pen, aux = ev(l, c)
        E = cost(image, R, pen)
        trail.append((E, image, R, n, s, True, l))
        pens.append((pen.P, pen.rmin, pen.nonpos))
        n_first, evals, g = n, 1, None
        if not np.isfinite(E):
            stop = 3
        else:
            while True:
                if evals >= max_evaluations:
                    stop = 1
                    break
                if g is None:
                    g, gmax = grad_at(l, c, pen, aux)
                if gmax == 0.0:
                    stop = 2
                    break
                ct = (c - F32(s / gmax) * g).astype(F32)
                nt, it, Rt, pt, at = ev(l, ct)
                evals += 1
                Et = cost(it, Rt, pt)
                accept = bool(np.isfinite(Et) and nt >= min_overlap * n_first and Et < E)
                trail.append((Et, it, Rt, nt, s, accept, l))
                pens.append((pt.P, pt.rmin, pt.nonpos))
                if not np.isfinite(Et) and not (mi and nt == 0):
                    stop = 3
                    break
                if accept:
                    c, n, image, R, pen, aux, E, g = ct, nt, it, Rt, pt, at, Et, None
                    s = min(2.0 * s, step_max)
                else:
                    s = s * 0.5
                if s < tol:
                    stop = 0
                    break
        if l > 0 and A is not None:
            A[:, 3] = A[:, 3] * 2.0
    return Refinement(c, fr.field(c, spacing, Fs[0].shape, A), trail, fr.STOPS[stop], pens)
