"""numpy restatement of "Affine refinement under a linear intensity map (NCC)" (include/sift3d_amd.h), built on
tests/affine_refine_restatement.py (sample_grad, centre, apply_delta, corner_distance) and tests/mask_restatement.py
(the counted voxels, the mask pyramid).

The sample and its gradient are float32 in the stated order; f, m and G are widened to float64 and every term is
formed there; every sum of the record is correctly rounded (math.fsum) and comes with sum |term|, so that a bound on
the device's sum need not allow for the reference's own error.  The fit follows the header's order of operations; the
step builds the 14 x 14 system and solves it on the free set by the header's Cholesky (K = C C^T row by row, then the
two triangular solves) in Python floats, operation for operation; the driver is the header's loop."""
import collections
import math

import numpy as np

from tests import affine_refine_restatement as ar
from tests import mask_restatement as mr

F32 = np.float32
SUMS = ("S_m", "S_f", "S_mm", "S_fm", "S_ff", "u", "v", "w", "H")
Record = collections.namedtuple("Record", ("n",) + SUMS + ("terms",))      # terms: {name: sum |term|, shaped alike}
Fit = collections.namedtuple("Fit", "alpha beta cost ncc")
Refinement = collections.namedtuple("Refinement", "A cost count accepted lambdas levels evaluations stop fit")


def _fsum(a):
    return math.fsum(np.asarray(a, np.float64).reshape(-1).tolist())


def record(F, M, A, WF=None, WM=None, exact=True):
    """the record over the counted voxels.  exact=False adds with numpy's pairwise sum instead of math.fsum (the
    driver: many evaluations, no bit compared)"""
    fsum = _fsum if exact else (lambda a: float(np.sum(a)))
    F = np.ascontiguousarray(F, F32)
    m, gx, gy, gz, ins = ar.sample_grad(M, A, F.shape)
    ins = ins & mr.counted(mr.coords(A, F.shape), np.shape(M), WF, WM)
    oz, oy, ox = F.shape
    c = ar.centre(F.shape)
    z, y, x = np.meshgrid(np.arange(oz), np.arange(oy), np.arange(ox), indexing="ij")
    f, m = F[ins].astype(np.float64), m[ins].astype(np.float64)
    G = [v[ins].astype(np.float64) for v in (gx, gy, gz)]
    P = [x[ins] - c[0], y[ins] - c[1], z[ins] - c[2], np.ones(f.size)]
    J = [G[d] * P[j] for d in range(3) for j in range(4)]

    def both(t):
        return fsum(t), float(np.abs(t).sum())

    val, mag = {}, {}
    for name, t in (("S_m", m), ("S_f", f), ("S_mm", m * m), ("S_fm", f * m), ("S_ff", f * f)):
        val[name], mag[name] = both(t)
    for name, q in (("u", None), ("v", m), ("w", f)):
        pairs = [both(J[r] if q is None else J[r] * q) for r in range(12)]
        val[name], mag[name] = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    H, Ht = np.zeros((12, 12)), np.zeros((12, 12))
    for r in range(12):
        for s in range(r, 12):
            H[r, s], Ht[r, s] = both(J[r] * J[s])
            H[s, r], Ht[s, r] = H[r, s], Ht[r, s]
    val["H"], mag["H"] = H, Ht
    return Record(int(f.size), *(val[k] for k in SUMS), mag)


def fit(rec):
    """Fit(alpha, beta, cost, ncc) in the header's order of operations; None where the fit is undefined"""
    if rec.n < 2:
        return None
    nd = float(rec.n)
    vm = rec.S_mm - rec.S_m * rec.S_m / nd
    vf = rec.S_ff - rec.S_f * rec.S_f / nd
    c = rec.S_fm - rec.S_f * rec.S_m / nd
    if not vm > 0:
        return None
    alpha = c / vm
    beta = (rec.S_f - alpha * rec.S_m) / nd
    cost = max((vf - alpha * c) / nd, 0.0)
    return Fit(alpha, beta, cost, 0.0 if vf <= 0 else c / math.sqrt(vf * vm))


def system14(rec, ft):
    """(H14 [14, 14], b14 [14]) at the fit's (alpha, beta)"""
    a, b, nd = ft.alpha, ft.beta, float(rec.n)
    H = np.zeros((14, 14))
    H[:12, :12] = (a * a) * np.asarray(rec.H)
    H[:12, 12] = H[12, :12] = a * np.asarray(rec.v)
    H[:12, 13] = H[13, :12] = a * np.asarray(rec.u)
    H[12, 12], H[12, 13], H[13, 12], H[13, 13] = rec.S_mm, rec.S_m, rec.S_m, nd
    g = np.zeros(14)
    g[:12] = a * ((a * np.asarray(rec.v) + b * np.asarray(rec.u)) - np.asarray(rec.w))
    g[12] = (a * rec.S_mm + b * rec.S_m) - rec.S_fm
    g[13] = (a * rec.S_m + b * nd) - rec.S_f
    return H, g


def cholesky_solve(K, rhs):
    """x of K x = rhs from K's lower triangle: K = C C^T row by row (s = K_ij - C_i0 C_j0 - C_i1 C_j1 ... in that
    order, C_ii = sqrt(s), C_ij = s / C_jj), C z = rhs forwards, C^T x = z backwards; None when K is not positive
    definite or x is not finite"""
    m = len(rhs)
    C = [[float(K[i][j]) for j in range(m)] for i in range(m)]
    for i in range(m):
        for j in range(i + 1):
            s = C[i][j]
            for k in range(j):
                s -= C[i][k] * C[j][k]
            if i == j:
                if not s > 0.0 or not math.isfinite(s):
                    return None
                C[i][i] = math.sqrt(s)
            else:
                C[i][j] = s / C[j][j]
    y = [0.0] * m
    for i in range(m):
        s = float(rhs[i])
        for k in range(i):
            s -= C[i][k] * y[k]
        y[i] = s / C[i][i]
    for i in range(m - 1, -1, -1):
        s = y[i]
        for k in range(i + 1, m):
            s -= C[k][i] * y[k]
        y[i] = s / C[i][i]
        if not math.isfinite(y[i]):
            return None
    return np.array(y)


def lm_step(rec, free_mask=0xFFF, lam=0.0):
    """delta [12]: the first 12 entries of (H14 + lam diag H14) delta14 = -b14 on the free set (the mask's bits, and
    12 and 13 always), 0 elsewhere; None where the contract refuses"""
    idx = ar.free_indices(free_mask)
    ft = fit(rec)
    if not idx or int(free_mask) & ~0xFFF or ft is None or not (np.isfinite(lam) and lam >= 0):
        return None
    H, g = system14(rec, ft)
    all14 = idx + [12, 13]
    Hf = H[np.ix_(all14, all14)]
    y = cholesky_solve(Hf + lam * np.diag(np.diag(Hf)), -g[all14])
    if y is None:
        return None
    delta = np.zeros(12)
    delta[idx] = y[:len(idx)]
    return delta


def refine(F, M, A=None, WF=None, WM=None, levels=1, free_mask=0xFFF, max_evaluations=30, lambda0=1e-3,
           lambda_factor=10.0, lambda_min=1e-9, lambda_max=1e7, tol=1e-3, min_overlap=0.5):
    """the header's driver: affine_refine_restatement.refine's loop with the fit's cost in the place of S_ee / n"""
    A = np.eye(3, 4) if A is None else np.array(A, np.float64).reshape(3, 4)
    Fs, Ms, WFs, WMs = (mr.pyramid(v, levels) for v in (F, M, WF, WM))
    for _ in range(1, levels):
        A[:, 3] = A[:, 3] * 0.5
    nan = float("nan")

    def cost_of(r):
        ft = fit(r)
        return nan if ft is None else ft.cost

    trail = []
    stop = 2
    for l in range(levels - 1, -1, -1):
        def ev(At, l=l):
            return record(Fs[l], Ms[l], At, WFs[l], WMs[l], exact=False)
        lam = lambda0
        rec = ev(A)
        cost = cost_of(rec)
        trail.append((cost, rec.n, lam, True, l))
        n_first, evals = rec.n, 1
        while True:
            if evals >= max_evaluations:
                stop = 2
                break
            delta = lm_step(rec, free_mask, lam)
            At = ar.apply_delta(A, delta, Fs[l].shape) if delta is not None else None
            if At is None or not np.isfinite(At).all():
                stop = 3
                break
            trial = ev(At)
            evals += 1
            cost_t = cost_of(trial)
            accept = trial.n > 0 and trial.n >= min_overlap * n_first and cost_t < cost
            trail.append((cost_t, trial.n, lam, accept, l))
            if accept:
                move = ar.corner_distance(A, At, Fs[l].shape)
                A, rec, cost = At, trial, cost_t
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
    return Refinement(A, np.array(t[0]), np.array(t[1], np.int64), np.array(t[3]), np.array(t[2]),
                      np.array(t[4], np.int64), len(trail), ar.STOPS[stop], fit(rec))
