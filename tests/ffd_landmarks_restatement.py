"""numpy restatement of the landmark contract (include/sift3d_amd.h, "FFD landmarks"): the point weights, the 64-term
spline at a point and the map T in float64 in the header's order; the residuals, the record and GL with their sums
correctly rounded (math.fsum) and the sum of |term| beside each, so that a bound on the device's sums need not allow for
the reference's own error; the driver is the header's loop (tests/ffd_restatement.py, tests/jacobian_penalty_restatement
.py) with the term added to the cost and the gradient."""
import collections
import math

import numpy as np

from tests import ffd_restatement as fr
from tests import jacobian_penalty_restatement as jr
from tests import mask_restatement as mr

F32 = np.float32
MAX_LANDMARKS = 65536
Record = collections.namedtuple("Record", "counted S Omega rmax r inside GL S_terms Omega_terms GL_terms support")
Refinement = collections.namedtuple("Refinement", "lattice field trail stop penalty landmarks")


def point_axis(x, delta, g):
    """(i0 int64 [n], w float64 [n, 4], inside bool [n]) of the coordinates x along an axis of spacing delta and lattice
    size g; where not inside i0 = 0 and the weights are those of t = 0"""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        v = x / np.float64(delta)
        f = np.floor(v)
        inside = (f >= 0.0) & (f <= np.float64(g - 4))
    i0 = np.where(inside, f, 0.0).astype(np.int64)
    t = np.where(inside, v - i0.astype(np.float64), 0.0)
    u = 1.0 - t
    t2 = t * t
    t3 = t2 * t
    w = np.stack([((u * u) * u) / 6.0, ((3.0 * t3 - 6.0 * t2) + 4.0) / 6.0,
                  (((-3.0 * t3 + 3.0 * t2) + 3.0 * t) + 1.0) / 6.0, t3 / 6.0], axis=1)
    return i0, w, inside


def _axes(lattice_shape, spacing, P):
    _, gz, gy, gx = lattice_shape
    dx, dy, dz = fr.spacing3(spacing)
    P = np.asarray(P, np.float64).reshape(-1, 3)
    ax = [point_axis(P[:, k], d, g) for k, (d, g) in enumerate(((dx, gx), (dy, gy), (dz, gz)))]
    return ax, ax[0][2] & ax[1][2] & ax[2][2]


def spline(lattice, spacing, P):
    """(s float64 [n, 3], inside): the 64 terms of every point in the header's order; rows that are not inside hold the
    spline of cell 0 at t = 0 and mean nothing"""
    c = np.ascontiguousarray(lattice, F32).astype(np.float64)
    ((ix, wx, _), (iy, wy, _), (iz, wz, _)), inside = _axes(c.shape, spacing, P)
    s = np.zeros((len(ix), 3))
    for cc in range(4):
        for b in range(4):
            for a in range(4):
                v = c[:, iz + cc, iy + b, ix + a].T                      # [n, 3]
                s = s + wz[:, cc, None] * (wy[:, b, None] * (wx[:, a, None] * v))
    return s, inside


def pull(P, A):
    """q [n, 3]: the header's pull map, or P itself without A"""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    if A is None:
        return P.copy()
    A = np.asarray(A, np.float64).reshape(3, 4)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([A[d][0] * x + ((A[d][1] * y + A[d][2] * z) + A[d][3]) for d in range(3)], axis=1)


def points(lattice, spacing, P, A=None):
    """(T float64 [n, 3], inside): sift3d_hip_ffd_points, NaN rows where not inside"""
    s, inside = spline(lattice, spacing, P)
    with np.errstate(invalid="ignore", over="ignore"):
        T = pull(P, A) + s
    T[~inside] = np.nan
    return T, inside


def _fsum(a):
    return math.fsum(np.asarray(a, np.float64).reshape(-1).tolist())


def landmarks(lattice, spacing, P, Q, w=None, A=None, exact=True):
    """Record of sift3d_hip_ffd_landmarks.  exact=False sums GL with numpy (the driver's use)"""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    Q = np.asarray(Q, np.float64).reshape(-1, 3)
    w = np.ones(len(P)) if w is None else np.asarray(w, np.float64)
    shape = np.shape(lattice)
    T, inside = points(lattice, spacing, P, A)
    r = np.where(inside[:, None], T - Q, 0.0)
    ss = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
    om = np.where(inside, w, 0.0)
    terms = om * ss
    rmax = float(np.fmax.reduce(np.sqrt(ss[inside]), initial=0.0))
    ((ix, wx, _), (iy, wy, _), (iz, wz, _)), _ = _axes(shape, spacing, P)
    _, gz, gy, gx = shape
    idx, gt = [], []
    sel = np.nonzero(inside)[0]
    for cc in range(4):
        for b in range(4):
            for a in range(4):
                coef = om[sel] * ((wz[sel, cc] * wy[sel, b]) * wx[sel, a])
                idx.append(((iz[sel] + cc) * gy + (iy[sel] + b)) * gx + (ix[sel] + a))
                gt.append(coef[:, None] * r[sel])
    idx = np.concatenate(idx) if len(sel) else np.zeros(0, np.int64)
    gt = np.concatenate(gt) if len(sel) else np.zeros((0, 3))
    n = gz * gy * gx
    sup = np.bincount(idx, minlength=n)
    tot = np.stack([np.bincount(idx, np.abs(gt[:, d]), n) for d in range(3)])
    if exact:
        order = np.argsort(idx, kind="stable")
        cuts = np.cumsum(sup)[:-1]
        GL = np.stack([np.array([math.fsum(g.tolist()) for g in np.split(gt[order, d], cuts)]) for d in range(3)])
        S, Om = _fsum(terms), _fsum(om)
    else:
        GL = np.stack([np.bincount(idx, gt[:, d], n) for d in range(3)])
        S, Om = float(terms.sum()), float(om.sum())
    return Record(int(inside.sum()), S, Om, rmax, r, inside, GL.reshape(3, gz, gy, gx), float(np.abs(terms).sum()),
                  float(np.abs(om).sum()), tot.reshape(3, gz, gy, gx), sup.reshape(gz, gy, gx))


def term(rec, level=0):
    """(L, rmax) in level-0 units"""
    return ((4.0 ** level * rec.S) / rec.Omega if rec.Omega != 0.0 else 0.0), rec.rmax * 2.0 ** level


def refine(F, M, P, Q, w=None, landmark_weight=0.0, A=None, spacing=8, levels=3, bending_weight=0.005,
           jacobian_weight=None, max_evaluations=60, step0=1.0, step_max=4.0, tol=0.01, min_overlap=0.5):
    """the header's driver for the MSD with E = base_E + lambda L and the term of the gradient; jacobian_weight None
    runs without the penalty.  trail entries as ffd_restatement.refine's, landmarks one (L, rmax, counted) per entry"""
    A = None if A is None else np.array(A, np.float64).reshape(3, 4)
    ref = jr.ref_of(A)
    P = np.asarray(P, np.float64).reshape(-1, 3)
    Q = np.asarray(Q, np.float64).reshape(-1, 3)
    Fs, Ms = mr.pyramid(F, levels), mr.pyramid(M, levels)
    for _ in range(1, levels):
        if A is not None:
            A[:, 3] = A[:, 3] * 0.5
    jw = 0.0 if jacobian_weight is None else jacobian_weight
    trail, pens, lms, stop, c = [], [], [], 1, None

    def ev(l, lat):
        rec, u = fr.evaluate(Fs[l], Ms[l], lat, spacing, A, exact=False)
        R, dR, _, _ = fr.bending(lat, spacing)
        pen = None if jacobian_weight is None else jr.penalty(u, ref)
        lm = landmarks(lat, spacing, P * 0.5 ** l, Q * 0.5 ** l, w, A, exact=False)
        L, rmax = term(lm, l)
        image = rec.see / rec.n if rec.n else float("nan")
        E = image + bending_weight * R
        if jw > 0:
            E = E + jw * pen.P
        if landmark_weight > 0:
            E = E + landmark_weight * L
        with np.errstate(divide="ignore", invalid="ignore"):
            g = (2.0 / np.float64(rec.n)) * rec.Gc + bending_weight * dR
            if jw > 0:
                g = g + (jw / np.float64(pen.r.size)) * jr.lattice_gradient(pen.S, spacing)
            if landmark_weight > 0 and lm.Omega != 0.0:
                g = g + ((landmark_weight * (2.0 * 4.0 ** l)) / lm.Omega) * lm.GL
        g = g.astype(F32)
        return dict(n=rec.n, image=image, R=R, pen=pen, L=L, rmax=rmax, counted=lm.counted, E=E, g=g,
                    gmax=float(np.abs(g).max()))

    def record(e, s, acc, l):
        trail.append((e["E"], e["image"], e["R"], e["n"], s, acc, l))
        if e["pen"] is not None:
            pens.append((e["pen"].P, e["pen"].rmin, e["pen"].nonpos))
        lms.append((e["L"], e["rmax"], e["counted"]))

    for l in range(levels - 1, -1, -1):
        shape = Fs[l].shape
        c = np.zeros(fr.lattice_shape(shape, spacing), F32) if c is None else fr.refine2(c, shape, spacing)
        s = step0
        cur = ev(l, c)
        record(cur, s, True, l)
        n_first, evals = cur["n"], 1
        if not np.isfinite(cur["E"]):
            stop = 3
        else:
            while True:
                if evals >= max_evaluations:
                    stop = 1
                    break
                if cur["gmax"] == 0.0:
                    stop = 2
                    break
                ct = (c - F32(s / cur["gmax"]) * cur["g"]).astype(F32)
                tr = ev(l, ct)
                evals += 1
                accept = bool(np.isfinite(tr["E"]) and tr["n"] >= min_overlap * n_first and tr["E"] < cur["E"])
                record(tr, s, accept, l)
                if not np.isfinite(tr["E"]):
                    stop = 3
                    break
                if accept:
                    c, cur = ct, tr
                    s = min(2.0 * s, step_max)
                else:
                    s = s * 0.5
                if s < tol:
                    stop = 0
                    break
        if l > 0 and A is not None:
            A[:, 3] = A[:, 3] * 2.0
    return Refinement(c, fr.field(c, spacing, Fs[0].shape, A), trail, fr.STOPS[stop], pens or None, lms)
