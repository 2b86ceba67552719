"""numpy restatement of the mask contract (include/sift3d_amd.h, "Masks"), built on the unmasked restatements.

The sample, its gradient, the field and the inside test are tests/similarity_restatement.sample,
tests/affine_refine_restatement.sample_grad and tests/ffd_restatement.sample_grad / field, unchanged; their inside array
is and-ed with the two mask tests (a float32 compare w >= 0.5 on the fixed mask at p and on the moving mask at the
voxel floor(q + 0.5), q in float64), and the reductions are redone the same way: bincount for the histogram, math.fsum
for every sum, with sum |term| beside it for the bounds.  With masks None the functions are the unmasked restatements'
arithmetic on the unmasked inside array.  The drivers are the headers' loops with level l's masks
tests.multires_restatement.ref_restrict of level l - 1's float masks."""
import math

import numpy as np

from tests import affine_refine_restatement as ar
from tests import ffd_restatement as fr
from tests import similarity_restatement as sr
from tests.multires_restatement import ref_restrict
from tests.test_warp import ref_coords, ref_inside

F32 = np.float32


def mask_in(w):
    """w >= 0.5f, one float32 compare: a NaN is out"""
    with np.errstate(invalid="ignore"):
        return np.asarray(w, F32) >= F32(0.5)


def coords(transform, out_shape):
    """q (x, y, z; float64 [oz, oy, ox]) of a 3 x 4 affine, a field [3, oz, oy, ox] or None (the identity)"""
    oz, oy, ox = out_shape
    z, y, x = np.meshgrid(np.arange(oz), np.arange(oy), np.arange(ox), indexing="ij")
    T = np.eye(3, 4) if transform is None else np.asarray(transform)
    if T.ndim == 4:
        return [p.astype(np.float64) + u.astype(F32).astype(np.float64) for p, u in zip((x, y, z), T)]
    return ref_coords(T.reshape(3, 4), x, y, z)


def counted(q, moving_shape, WF=None, WM=None):
    """inside(q) and W_F(p) in and W_M(floor(q + 0.5)) in"""
    ins = ref_inside(q, moving_shape)
    if WF is not None:
        assert tuple(np.shape(WF)) == tuple(q[0].shape)
        ins = ins & mask_in(WF)
    if WM is not None:
        assert tuple(np.shape(WM)) == tuple(moving_shape)
        ix, iy, iz = (np.floor(np.where(ins, v, 0.0) + 0.5).astype(np.int64) for v in q)
        ins = ins & mask_in(np.asarray(WM, F32)[iz, iy, ix])
    return ins


def _fsum(a):
    return math.fsum(np.asarray(a, np.float64).reshape(-1).tolist())


# ---- similarity ------------------------------------------------------------------------------------------------------
def joint(F, M, transform, bins, range_f, range_m, interp="linear", WF=None, WM=None):
    """similarity_restatement.joint over the counted voxels: (hist uint64 [B, B], Stats)"""
    F = np.ascontiguousarray(F, F32)
    m, ins = sr.sample(M, transform, F.shape, interp)
    ins = ins & counted(coords(transform, F.shape), np.shape(M), WF, WM)
    f, m = F[ins], m.astype(F32)[ins]
    idx = sr.bin_of(f, bins, *range_f) * bins + sr.bin_of(m, bins, *range_m)
    hist = np.bincount(idx, minlength=bins * bins).astype(np.uint64).reshape(bins, bins)
    fd, md, dd = f.astype(np.float64), m.astype(np.float64), (f - m).astype(np.float64)
    terms = [fd, md, fd * fd, md * md, fd * md, dd * dd]
    return hist, sr.Stats(int(f.size), np.array([_fsum(t) for t in terms]), np.array([np.abs(t).sum() for t in terms]))


# ---- the normal equations --------------------------------------------------------------------------------------------
def normal_equations(F, M, A, WF=None, WM=None, exact=True):
    """affine_refine_restatement.normal_equations over the counted voxels"""
    fsum = _fsum if exact else (lambda a: float(np.sum(a)))
    F = np.ascontiguousarray(F, F32)
    m, gx, gy, gz, ins = ar.sample_grad(M, A, F.shape)
    ins = ins & counted(coords(A, F.shape), np.shape(M), WF, WM)
    oz, oy, ox = F.shape
    c = ar.centre(F.shape)
    z, y, x = np.meshgrid(np.arange(oz), np.arange(oy), np.arange(ox), indexing="ij")
    E = (m - F).astype(F32)[ins].astype(np.float64)
    G = [v[ins].astype(np.float64) for v in (gx, gy, gz)]
    P = [x[ins] - c[0], y[ins] - c[1], z[ins] - c[2], np.ones(E.size)]
    J = [G[d] * P[j] for d in range(3) for j in range(4)]
    b, bt = np.zeros(12), np.zeros(12)
    H, Ht = np.zeros((12, 12)), np.zeros((12, 12))
    for r in range(12):
        t = J[r] * E
        b[r], bt[r] = fsum(t), float(np.abs(t).sum())
        for s in range(r, 12):
            t = J[r] * J[s]
            H[r, s] = H[s, r] = fsum(t)
            Ht[r, s] = Ht[s, r] = float(np.abs(t).sum())
    return ar.Normal(int(E.size), fsum(E * E), b, H, float((E * E).sum()), bt, Ht)


def pyramid(v, levels):
    """[v, restrict(v), ...] as float32, or [None] * levels"""
    if v is None:
        return [None] * levels
    out = [np.ascontiguousarray(v, F32)]
    for _ in range(1, levels):
        out.append(ref_restrict(out[-1]))
    return out


def refine_affine(F, M, A=None, WF=None, WM=None, levels=1, free_mask=0xFFF, max_evaluations=30, lambda0=1e-3,
                  lambda_factor=10.0, lambda_min=1e-9, lambda_max=1e7, tol=1e-3, min_overlap=0.5):
    """affine_refine_restatement.refine with the masked normal equations and the mask pyramid"""
    A = np.eye(3, 4) if A is None else np.array(A, np.float64).reshape(3, 4)
    Fs, Ms, WFs, WMs = (pyramid(v, levels) for v in (F, M, WF, WM))
    for _ in range(1, levels):
        A[:, 3] = A[:, 3] * 0.5
    trail = []
    stop = 2
    for l in range(levels - 1, -1, -1):
        def ev(At, l=l):
            return normal_equations(Fs[l], Ms[l], At, WFs[l], WMs[l], exact=False)
        lam = lambda0
        rec = ev(A)
        trail.append((rec.see / rec.n if rec.n else float("nan"), rec.n, lam, True, l))
        n_first, evals = rec.n, 1
        while True:
            if evals >= max_evaluations:
                stop = 2
                break
            delta = ar.lm_step(rec.n, rec.b, rec.H, free_mask, lam)
            At = ar.apply_delta(A, delta, Fs[l].shape) if delta is not None else None
            if At is None or not np.isfinite(At).all():
                stop = 3
                break
            trial = ev(At)
            evals += 1
            accept = trial.n > 0 and trial.n >= min_overlap * n_first and trial.see / trial.n < rec.see / rec.n
            trail.append((trial.see / trial.n if trial.n else float("nan"), trial.n, lam, accept, l))
            if accept:
                move = ar.corner_distance(A, At, Fs[l].shape)
                A, rec = At, trial
                lam = max(lam / lambda_factor, lambda_min)
                if move < tol:
                    stop = 0
                    break
            else:
                lam = lam * lambda_factor
                if lam > lambda_max:
                    stop = 1
                    break
        if l > 0:
            A[:, 3] = A[:, 3] * 2.0
    t = list(zip(*trail))
    return ar.Refinement(A, np.array(t[0]), np.array(t[1], np.int64), np.array(t[3]), np.array(t[2]),
                         np.array(t[4], np.int64), len(trail), ar.STOPS[stop])


# ---- free-form deformation -------------------------------------------------------------------------------------------
def evaluate(F, M, lattice, spacing, A=None, WF=None, WM=None, exact=True):
    """ffd_restatement.evaluate over the counted voxels: (Record, field, force float64 [3, oz, oy, ox])"""
    F = np.ascontiguousarray(F, F32)
    u = fr.field(lattice, spacing, F.shape, A)
    m, gx, gy, gz, ins = fr.sample_grad(M, u)
    ins = ins & counted(coords(u, F.shape), np.shape(M), WF, WM)
    E = np.where(ins, (m - F).astype(F32).astype(np.float64), 0.0)
    G = [np.where(ins, v.astype(np.float64), 0.0) for v in (gx, gy, gz)]
    fsum = _fsum if exact else (lambda a: float(np.sum(a)))
    force = np.stack([E * Gd for Gd in G])
    parts = [fr.adjoint(f, spacing, exact) for f in force]
    rec = fr.Record(int(ins.sum()), fsum(E * E), np.stack([p[0] for p in parts]), float((E * E).sum()),
                    np.stack([p[1] for p in parts]), parts[0][2])
    return rec, u, force


def refine_ffd(F, M, A=None, WF=None, WM=None, spacing=8, levels=3, bending_weight=0.005, max_evaluations=60,
               step0=1.0, step_max=4.0, tol=0.01, min_overlap=0.5):
    """ffd_restatement.refine with the masked evaluation and the mask pyramid"""
    A = None if A is None else np.array(A, np.float64).reshape(3, 4)
    Fs, Ms, WFs, WMs = (pyramid(v, levels) for v in (F, M, WF, WM))
    for _ in range(1, levels):
        if A is not None:
            A[:, 3] = A[:, 3] * 0.5
    trail, stop, c = [], 1, None

    def ev(l, lat):
        rec, _, _ = evaluate(Fs[l], Ms[l], lat, spacing, A, WFs[l], WMs[l], exact=False)
        R, dR, _, _ = fr.bending(lat, spacing)
        g, gmax = fr.gradient(rec, dR, bending_weight)
        return rec, R, g, gmax, fr.cost(rec, R, bending_weight)

    def entry(rec, R, E, s, acc, l):
        return (E, rec.see / rec.n if rec.n else float("nan"), R, rec.n, s, acc, l)

    for l in range(levels - 1, -1, -1):
        shape = Fs[l].shape
        c = np.zeros(fr.lattice_shape(shape, spacing), F32) if c is None else fr.refine2(c, shape, spacing)
        s = step0
        rec, R, g, gmax, E = ev(l, c)
        trail.append(entry(rec, R, E, s, True, l))
        n_first, evals = rec.n, 1
        if not np.isfinite(E):
            stop = 3
        else:
            while True:
                if evals >= max_evaluations:
                    stop = 1
                    break
                if gmax == 0.0:
                    stop = 2
                    break
                ct = (c - F32(s / gmax) * g).astype(F32)
                rt, Rt, gt, gmt, Et = ev(l, ct)
                evals += 1
                accept = bool(np.isfinite(Et) and rt.n >= min_overlap * n_first and Et < E)
                trail.append(entry(rt, Rt, Et, s, accept, l))
                if not np.isfinite(Et):
                    stop = 3
                    break
                if accept:
                    c, rec, R, g, gmax, E = ct, rt, Rt, gt, gmt, Et
                    s = min(2.0 * s, step_max)
                else:
                    s = s * 0.5
                if s < tol:
                    stop = 0
                    break
        if l > 0 and A is not None:
            A[:, 3] = A[:, 3] * 2.0
    return fr.Refinement(c, fr.field(c, spacing, Fs[0].shape, A), trail, fr.STOPS[stop])
