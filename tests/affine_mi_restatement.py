"""numpy restatement of "Mutual-information affine refinement (Mattes)" (include/sift3d_amd.h), built on
tests/affine_refine_restatement.py (sample_grad, centre, lm_step, apply_delta, corner_distance), on
tests/mask_restatement.py (the counted voxels, the mask pyramid) and on tests/similarity_restatement.py (the fixed bin,
the entropies).

The window is float64 in the header's order with np.rint (round to nearest even) for the fixed point; the histogram is
np.add.at on int64 (exact integers); the measures and the table W follow the header's order of operations; every sum of
the record is correctly rounded (math.fsum) and comes with sum |term|, so that a bound on the device's sum need not
allow for the reference's own error; the driver is the header's loop."""
import collections
import math

import numpy as np

from tests import affine_refine_restatement as ar
from tests import mask_restatement as mr
from tests import similarity_restatement as sr

F32 = np.float32
Q = 65536.0
Window = collections.namedtuple("Window", "k0 q dw out")
Measures = collections.namedtuple("Measures", "n mi nmi entropy_fixed entropy_moving entropy_joint cost W r c")
Record = collections.namedtuple("Record", "n see b H see_terms b_terms H_terms")
Refinement = collections.namedtuple("Refinement", "A cost count accepted lambdas levels evaluations stop measures")


def scale(lo, hi, bins):
    """s_m = (double)(B - 3) / ((double) hi - (double) lo)"""
    return float(bins - 3) / (float(F32(hi)) - float(F32(lo)))


def window(m, lo, hi, bins):
    """Window(k0 int64, q int64 [..., 4], dw float64 [..., 4], out bool) of the moving values m (float32)"""
    m = np.asarray(m, F32).astype(np.float64)
    top = float(bins - 2)
    t = 1.0 + (m - float(F32(lo))) * scale(lo, hi, bins)
    out = (t < 1.0) | (t > top)
    t = np.minimum(np.maximum(t, 1.0), top)
    k0 = np.minimum(np.floor(t).astype(np.int64) - 1, bins - 4)
    r = t - (k0 + 1).astype(np.float64)
    u, t2 = 1.0 - r, r * r
    t3 = t2 * r
    w = np.stack([((u * u) * u) / 6.0, ((3.0 * t3 - 6.0 * t2) + 4.0) / 6.0,
                  (((-3.0 * t3 + 3.0 * t2) + 3.0 * r) + 1.0) / 6.0, t3 / 6.0], axis=-1)
    dw = np.stack([-(u * u) / 2.0, (3.0 * t2 - 4.0 * r) / 2.0, ((-3.0 * t2 + 2.0 * r) + 1.0) / 2.0, t2 / 2.0], axis=-1)
    return Window(k0, np.rint(w * Q).astype(np.int64), dw, out)


def _counted(F, M, A, WF, WM):
    """(f, m, gx, gy, gz float32 and x, y, z of the counted voxels)"""
    F = np.ascontiguousarray(F, F32)
    m, gx, gy, gz, ins = ar.sample_grad(M, A, F.shape)
    ins = ins & mr.counted(mr.coords(A, F.shape), np.shape(M), WF, WM)
    oz, oy, ox = F.shape
    z, y, x = np.meshgrid(np.arange(oz), np.arange(oy), np.arange(ox), indexing="ij")
    return F[ins], m[ins], gx[ins], gy[ins], gz[ins], x[ins], y[ins], z[ins]


def histogram(F, M, A, bins, range_f, range_m, WF=None, WM=None):
    """(hist int64 [B, B] indexed [b_f, b_m], count, per-voxel sum of q over the counted voxels)"""
    f, m = _counted(F, M, A, WF, WM)[:2]
    bf = sr.bin_of(f, bins, *range_f)
    win = window(m, range_m[0], range_m[1], bins)
    hist = np.zeros((bins, bins), np.int64)
    for k in range(4):
        np.add.at(hist, (bf, win.k0 + k), win.q[:, k])
    return hist, int(f.size), int(win.q.sum())


def measures(hist):
    """Measures of sift3d_amd_parzen_mi: n = N, the entropies, mi, nmi, cost = -mi, W, and the marginals"""
    h = np.asarray(hist).astype(np.uint64)
    bins = h.shape[0]
    r, c = h.sum(axis=1, dtype=np.uint64), h.sum(axis=0, dtype=np.uint64)
    total = int(r.sum(dtype=np.uint64))
    W = np.zeros((bins, bins))
    nz = h != 0
    cd = np.broadcast_to(c.astype(np.float64), h.shape)
    W[nz] = np.log(h.astype(np.float64)[nz] / cd[nz])
    if total == 0:
        nan = float("nan")
        return Measures(0, nan, nan, nan, nan, nan, nan, W, r, c)
    hf, hm, hfm = sr.entropy(r, total), sr.entropy(c, total), sr.entropy(h, total)
    mi = (hf + hm) - hfm
    return Measures(total, mi, 0.0 if hfm == 0 else (hf + hm) / hfm, hf, hm, hfm, -mi, W, r, c)


def _fsum(a):
    return math.fsum(np.asarray(a, np.float64).reshape(-1).tolist())


def psi_of(f, m, W, bins, range_f, range_m):
    """psi float64 of the voxels with fixed values f and samples m"""
    bf = sr.bin_of(f, bins, *range_f)
    win = window(m, range_m[0], range_m[1], bins)
    W = np.asarray(W, np.float64)
    Wk = [W[bf, win.k0 + k] for k in range(4)]
    dw = win.dw
    v = scale(range_m[0], range_m[1], bins) * (((dw[:, 0] * Wk[0] + dw[:, 1] * Wk[1]) + dw[:, 2] * Wk[2])
                                               + dw[:, 3] * Wk[3])
    return np.where(win.out, 0.0, v)


def record(F, M, A, W, bins, range_f, range_m, WF=None, WM=None, exact=True):
    """Record(n, S_pp, b [12], H [12, 12], and sum |term| of each) with the table W.  exact=False adds with numpy's
    pairwise sum instead of math.fsum (the driver: many evaluations, no bit compared)"""
    fsum = _fsum if exact else (lambda a: float(np.sum(a)))
    f, m, gx, gy, gz, x, y, z = _counted(F, M, A, WF, WM)
    c = ar.centre(np.shape(F))
    psi = psi_of(f, m, W, bins, range_f, range_m)
    G = [psi * v.astype(np.float64) for v in (gx, gy, gz)]
    P = [x - c[0], y - c[1], z - c[2], np.ones(f.size)]
    J = [G[d] * P[j] for d in range(3) for j in range(4)]
    b, bt = np.zeros(12), np.zeros(12)
    H, Ht = np.zeros((12, 12)), np.zeros((12, 12))
    for r in range(12):
        t = -J[r]
        b[r], bt[r] = fsum(t), float(np.abs(t).sum())
        for s in range(r, 12):
            t = J[r] * J[s]
            H[r, s] = H[s, r] = fsum(t)
            Ht[r, s] = Ht[s, r] = float(np.abs(t).sum())
    return Record(int(f.size), fsum(psi * psi), b, H, float((psi * psi).sum()), bt, Ht)


def refine(F, M, A=None, bins=32, range_f=None, range_m=None, WF=None, WM=None, levels=1, free_mask=0xFFF,
           max_evaluations=30, lambda0=1e-3, lambda_factor=10.0, lambda_min=1e-9, lambda_max=1e7, tol=1e-3,
           min_overlap=0.5):
    """the header's driver: affine_refine_restatement.refine's loop; an evaluation is the histogram and its measures,
    and the record is made only at the map the next step starts from.  A range left None is the volume's min and max."""
    A = np.eye(3, 4) if A is None else np.array(A, np.float64).reshape(3, 4)
    range_f = (float(np.min(F)), float(np.max(F))) if range_f is None else range_f
    range_m = (float(np.min(M)), float(np.max(M))) if range_m is None else range_m
    Fs, Ms, WFs, WMs = (mr.pyramid(v, levels) for v in (F, M, WF, WM))
    for _ in range(1, levels):
        A[:, 3] = A[:, 3] * 0.5
    trail = []
    stop = 2
    ms = None
    for l in range(levels - 1, -1, -1):
        def ev(At, l=l):
            hist, n, _ = histogram(Fs[l], Ms[l], At, bins, range_f, range_m, WFs[l], WMs[l])
            return n, measures(hist)

        def rec_at(At, me, l=l):
            return record(Fs[l], Ms[l], At, me.W, bins, range_f, range_m, WFs[l], WMs[l], exact=False)
        lam = lambda0
        n, ms = ev(A)
        cost = ms.cost
        rec = None
        trail.append((cost, n, lam, True, l))
        n_first, evals = n, 1
        while True:
            if evals >= max_evaluations:
                stop = 2
                break
            if rec is None and n:
                rec = rec_at(A, ms)
            delta = ar.lm_step(rec.n, rec.b, rec.H, free_mask, lam) if rec is not None else None
            At = ar.apply_delta(A, delta, Fs[l].shape) if delta is not None else None
            if At is None or not np.isfinite(At).all():
                stop = 3
                break
            n_t, ms_t = ev(At)
            evals += 1
            accept = n_t > 0 and n_t >= min_overlap * n_first and ms_t.cost < cost
            trail.append((ms_t.cost, n_t, lam, accept, l))
            if accept:
                move = ar.corner_distance(A, At, Fs[l].shape)
                A, n, ms, cost, rec = At, n_t, ms_t, ms_t.cost, None
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
                      np.array(t[4], np.int64), len(trail), ar.STOPS[stop], ms)
