"""numpy restatement of the affine refinement contract (include/sift3d_amd.h, "Intensity-driven affine refinement").

The sample and its gradient are float32 in the stated order (the value is tests.test_warp.ref_warp's, bit for bit);
the terms E E, J E and J J^T are float64; every sum is correctly rounded (math.fsum), so that a bound on the device's
sum need not allow for the reference's own error, and comes with sum |term| for that bound.  The LM step solves on the
free set with numpy.linalg.solve; apply_delta follows the header's order of operations; the driver is the header's
loop, with coarser levels from tests.multires_restatement.ref_restrict."""
import collections
import math

import numpy as np

from tests.multires_restatement import ref_restrict
from tests.test_warp import ref_coords, ref_inside

F32 = np.float32
Normal = collections.namedtuple("Normal", "n see b H see_terms b_terms H_terms")
Refinement = collections.namedtuple("Refinement", "A msd count accepted lambdas levels evaluations stop")
STOPS = ("converged", "lambda", "evaluations", "lm_failed")


def centre(fshape):
    """c = ((ox - 1) / 2, (oy - 1) / 2, (oz - 1) / 2) of the fixed grid [oz, oy, ox]"""
    oz, oy, ox = fshape
    return np.array([(ox - 1) / 2.0, (oy - 1) / 2.0, (oz - 1) / 2.0])


def sample_grad(M, A, out_shape):
    """(m, gx, gy, gz float32 [oz, oy, ox], inside) of M through the pull map A: gather_grad of the contract"""
    M = np.ascontiguousarray(M, F32)
    nz, ny, nx = M.shape
    oz, oy, ox = out_shape
    z, y, x = np.meshgrid(np.arange(oz), np.arange(oy), np.arange(ox), indexing="ij")
    q = ref_coords(A, x, y, z)
    ins = ref_inside(q, M.shape)
    q = [np.where(ins, v, 0.0) for v in q]
    i = [np.floor(v) for v in q]
    f = [(v - iv).astype(F32) for v, iv in zip(q, i)]
    i = [iv.astype(np.int64) for iv in i]
    j = [np.minimum(iv + 1, n - 1) for iv, n in zip(i, (nx, ny, nz))]
    flat = M.reshape(-1)

    def g(ix, iy, iz):
        return flat[(iz * ny + iy) * nx + ix]

    def lerp(a, b, t):
        return (a + t * (b - a)).astype(F32)

    a00, b00 = g(i[0], i[1], i[2]), g(j[0], i[1], i[2])
    a10, b10 = g(i[0], j[1], i[2]), g(j[0], j[1], i[2])
    a01, b01 = g(i[0], i[1], j[2]), g(j[0], i[1], j[2])
    a11, b11 = g(i[0], j[1], j[2]), g(j[0], j[1], j[2])
    fx, fy, fz = f
    c00, c10, c01, c11 = lerp(a00, b00, fx), lerp(a10, b10, fx), lerp(a01, b01, fx), lerp(a11, b11, fx)
    c0, c1 = lerp(c00, c10, fy), lerp(c01, c11, fy)
    m = lerp(c0, c1, fz)
    gx = lerp(lerp(b00 - a00, b10 - a10, fy), lerp(b01 - a01, b11 - a11, fy), fz)
    gy = lerp(c10 - c00, c11 - c01, fz)
    gz = (c1 - c0).astype(F32)
    return m, gx, gy, gz, ins


def _fsum(a):
    return math.fsum(np.asarray(a, np.float64).reshape(-1).tolist())


def normal_equations(F, M, A, exact=True):
    """Normal(n, S_ee, b [12], H [12, 12], and sum |term| of each) over the fixed voxels that sample inside M.
    exact=False adds with numpy's pairwise sum instead of math.fsum (the driver: many evaluations, no bit compared)"""
    fsum = _fsum if exact else (lambda a: float(np.sum(a)))
    F = np.ascontiguousarray(F, F32)
    m, gx, gy, gz, ins = sample_grad(M, A, F.shape)
    oz, oy, ox = F.shape
    c = centre(F.shape)
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
    return Normal(int(E.size), fsum(E * E), b, H, float((E * E).sum()), bt, Ht)


def free_indices(mask):
    return [i for i in range(12) if int(mask) >> i & 1]


def lm_step(n, b, H, free_mask=0xFFF, lam=0.0):
    """delta [12]: (H + lam diag H) delta = -b on the free set, 0 elsewhere; None where the contract refuses"""
    idx = free_indices(free_mask)
    if n == 0 or not idx or int(free_mask) & ~0xFFF:
        return None
    Hf = np.asarray(H, np.float64)[np.ix_(idx, idx)]
    K = Hf + lam * np.diag(np.diag(Hf))
    if np.any(np.diag(K) <= 0):
        return None
    try:
        np.linalg.cholesky(K)
        d = np.linalg.solve(K, -np.asarray(b, np.float64)[idx])
    except np.linalg.LinAlgError:
        return None
    delta = np.zeros(12)
    delta[idx] = d
    return delta if np.isfinite(delta).all() else None


def apply_delta(A, delta, fshape):
    """the header's update, operation for operation (float64)"""
    A = np.asarray(A, np.float64).reshape(3, 4)
    d = np.asarray(delta, np.float64).reshape(3, 4)
    c = centre(fshape)
    out = np.zeros((3, 4))
    for r in range(3):
        a = A[r]
        t = a[3] + ((a[0] * c[0] + a[1] * c[1]) + a[2] * c[2])
        o = [a[j] + d[r, j] for j in range(3)]
        out[r, :3] = o
        out[r, 3] = (t + d[r, 3]) - ((o[0] * c[0] + o[1] * c[1]) + o[2] * c[2])
    return out


def corners(fshape):
    oz, oy, ox = fshape
    return np.array([[x, y, z, 1.0] for z in (0, oz - 1) for y in (0, oy - 1) for x in (0, ox - 1)], np.float64)


def corner_distance(A, B, fshape):
    """the largest distance between A p and B p over the 8 corners p of the fixed grid"""
    D = np.asarray(B, np.float64).reshape(3, 4) - np.asarray(A, np.float64).reshape(3, 4)
    return float(np.sqrt(((corners(fshape) @ D.T) ** 2).sum(axis=1)).max())


def refine(F, M, A=None, levels=1, free_mask=0xFFF, max_evaluations=30, lambda0=1e-3, lambda_factor=10.0,
           lambda_min=1e-9, lambda_max=1e7, tol=1e-3, min_overlap=0.5):
    """the header's driver"""
    A = np.eye(3, 4) if A is None else np.array(A, np.float64).reshape(3, 4)
    Fs, Ms = [np.ascontiguousarray(F, F32)], [np.ascontiguousarray(M, F32)]
    for _ in range(1, levels):
        Fs.append(ref_restrict(Fs[-1]))
        Ms.append(ref_restrict(Ms[-1]))
        A[:, 3] = A[:, 3] * 0.5
    trail = []
    stop = 2
    for l in range(levels - 1, -1, -1):
        Fl, Ml = Fs[l], Ms[l]
        lam = lambda0
        rec = normal_equations(Fl, Ml, A, exact=False)
        trail.append((rec.see / rec.n if rec.n else float("nan"), rec.n, lam, True, l))
        n_first, evals = rec.n, 1
        while True:
            if evals >= max_evaluations:
                stop = 2
                break
            delta = lm_step(rec.n, rec.b, rec.H, free_mask, lam)
            At = apply_delta(A, delta, Fl.shape) if delta is not None else None
            if At is None or not np.isfinite(At).all():
                stop = 3
                break
            trial = normal_equations(Fl, Ml, At, exact=False)
            evals += 1
            accept = trial.n > 0 and trial.n >= min_overlap * n_first and trial.see / trial.n < rec.see / rec.n
            trail.append((trial.see / trial.n if trial.n else float("nan"), trial.n, lam, accept, l))
            if accept:
                move = corner_distance(A, At, Fl.shape)
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
    return Refinement(A, np.array(t[0]), np.array(t[1], np.int64), np.array(t[3]), np.array(t[2]),
                      np.array(t[4], np.int64), len(trail), STOPS[stop])
