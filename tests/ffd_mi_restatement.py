"""numpy restatement of "Mutual-information free-form deformation (Mattes)" (include/sift3d_amd.h), composed from the
restatements it is the product of: tests/ffd_restatement.py (field, sample_grad, adjoint, bending, refine2),
tests/affine_mi_restatement.py (window, measures, psi_of), tests/mask_restatement.py (the counted voxels, the mask
pyramid) and tests/similarity_restatement.py (the fixed bin).

The histogram is np.add.at on int64 (exact integers); psi is affine_mi_restatement's arithmetic; the force -(psi * g_d)
is float64, one rounding; Gc's sums are correctly rounded (math.fsum) and come with sum |term| and the support, so that a
bound on the device's sum need not allow for the reference's own error; the driver is the header's loop."""
import collections
import math

import numpy as np

from tests import affine_mi_restatement as am
from tests import ffd_restatement as fr
from tests import mask_restatement as mr
from tests import similarity_restatement as sr

F32 = np.float32
Record = collections.namedtuple("Record", "n spp Gc spp_terms Gc_terms support")
Refinement = collections.namedtuple("Refinement", "lattice field trail stop measures")


def own_range(v):
    return float(np.min(v)), float(np.max(v))


def _sampled(F, M, u, WF, WM):
    """(m, gx, gy, gz float32 [oz, oy, ox], counted) of M through the field u"""
    m, gx, gy, gz, ins = fr.sample_grad(M, u)
    return m, gx, gy, gz, ins & mr.counted(mr.coords(u, np.shape(F)), np.shape(M), WF, WM)


def histogram_field(F, M, field, bins, range_f, range_m, WF=None, WM=None):
    """(hist int64 [B, B] indexed [b_f, b_m], count) of sift3d_hip_parzen_hist_field"""
    F = np.ascontiguousarray(F, F32)
    u = np.ascontiguousarray(field, F32)
    with np.errstate(invalid="ignore"):
        m, _, _, _, ins = _sampled(F, M, u, WF, WM)
    f, mm = F[ins], m[ins]
    bf = sr.bin_of(f, bins, *range_f)
    win = am.window(mm, range_m[0], range_m[1], bins)
    hist = np.zeros((bins, bins), np.int64)
    for k in range(4):
        np.add.at(hist, (bf, win.k0 + k), win.q[:, k])
    return hist, int(ins.sum())


def force(F, M, u, W, bins, ranges, WF=None, WM=None):
    """(n, psi float64 [oz, oy, ox], E G'_d = -(psi g_d) float64 [3, oz, oy, ox]): zero at the voxels not counted"""
    F = np.ascontiguousarray(F, F32)
    m, gx, gy, gz, ins = _sampled(F, M, u, WF, WM)
    psi = np.zeros(F.shape)
    psi[ins] = am.psi_of(F[ins], m[ins], W, bins, ranges[0], ranges[1])
    G = np.stack([-(psi * np.where(ins, v.astype(np.float64), 0.0)) for v in (gx, gy, gz)])
    return int(ins.sum()), psi, G + 0.0                                  # + 0.0: no negative zeros


def evaluate(F, M, lattice, spacing, A, W, bins, ranges, WF=None, WM=None, exact=True):
    """(Record, field): n, S_pp, Gc [3, gz, gy, gx], sum |term| of each and the support, with the table W"""
    F = np.ascontiguousarray(F, F32)
    u = fr.field(lattice, spacing, F.shape, A)
    n, psi, G = force(F, M, u, W, bins, ranges, WF, WM)
    fsum = (lambda a: math.fsum(np.asarray(a).reshape(-1).tolist())) if exact else (lambda a: float(np.sum(a)))
    parts = [fr.adjoint(Gd, spacing, exact) for Gd in G]
    return Record(n, fsum(psi * psi), np.stack([p[0] for p in parts]), float((psi * psi).sum()),
                  np.stack([p[1] for p in parts]), parts[0][2]), u


def gradient(rec, dR, bend):
    """(grad float32, gmax): the factor is 1 / n"""
    with np.errstate(divide="ignore", invalid="ignore"):
        g = ((1.0 / np.float64(rec.n)) * rec.Gc + bend * dR).astype(F32)
    return g, float(np.abs(g).max())


def cost_at(F, M, lattice, spacing, A, bins, ranges, bend=0.0, WF=None, WM=None):
    """(-mi + bend * R, n, Measures) at a lattice"""
    u = fr.field(lattice, spacing, np.shape(F), A)
    hist, n = histogram_field(F, M, u, bins, ranges[0], ranges[1], WF, WM)
    me = am.measures(hist)
    R = fr.bending(lattice, spacing)[0] if bend else 0.0
    return me.cost + bend * R, n, me


def refine(F, M, A=None, spacing=8, levels=3, bending_weight=0.005, max_evaluations=60, bins=32, range_f=None,
           range_m=None, WF=None, WM=None, step0=1.0, step_max=4.0, tol=0.01, min_overlap=0.5):
    """the header's driver: ffd_restatement.refine's loop with the cost -mi + bending R; an evaluation is the field,
    the histogram and R, and the gradient is made only at the lattice the next step starts from.  Trail entries
    (E, -mi, R, n, step, accepted, level).  A range left None is the volume's min and max."""
    A = None if A is None else np.array(A, np.float64).reshape(3, 4)
    ranges = (own_range(F) if range_f is None else range_f, own_range(M) if range_m is None else range_m)
    Fs, Ms, WFs, WMs = (mr.pyramid(v, levels) for v in (F, M, WF, WM))
    for _ in range(1, levels):
        if A is not None:
            A[:, 3] = A[:, 3] * 0.5
    trail, stop, c, me = [], 1, None, None

    def ev(l, lat):
        u = fr.field(lat, spacing, Fs[l].shape, A)
        hist, n = histogram_field(Fs[l], Ms[l], u, bins, ranges[0], ranges[1], WFs[l], WMs[l])
        m = am.measures(hist)
        R = fr.bending(lat, spacing)[0]
        return n, m, R, m.cost + bending_weight * R

    def grad_at(l, lat, m):
        rec, _ = evaluate(Fs[l], Ms[l], lat, spacing, A, m.W, bins, ranges, WFs[l], WMs[l], exact=False)
        return gradient(rec, fr.bending(lat, spacing)[1], bending_weight)

    for l in range(levels - 1, -1, -1):
        shape = Fs[l].shape
        c = np.zeros(fr.lattice_shape(shape, spacing), F32) if c is None else fr.refine2(c, shape, spacing)
        s = step0
        n, me, R, E = ev(l, c)
        trail.append((E, me.cost, R, n, s, True, l))
        n_first, evals, g = n, 1, None
        if not np.isfinite(E):
            stop = 3
        else:
            while True:
                if evals >= max_evaluations:
                    stop = 1
                    break
                if g is None:
                    g, gmax = grad_at(l, c, me)
                if gmax == 0.0:
                    stop = 2
                    break
                ct = (c - F32(s / gmax) * g).astype(F32)
                nt, mt, Rt, Et = ev(l, ct)
                evals += 1
                accept = bool(np.isfinite(Et) and nt >= min_overlap * n_first and Et < E)
                trail.append((Et, mt.cost, Rt, nt, s, accept, l))
                if not np.isfinite(Et) and nt != 0:
                    stop = 3
                    break
                if accept:
                    c, n, me, R, E, g = ct, nt, mt, Rt, Et, None
                    s = min(2.0 * s, step_max)
                else:
                    s = s * 0.5
                if s < tol:
                    stop = 0
                    break
        if l > 0 and A is not None:
            A[:, 3] = A[:, 3] * 2.0
    return Refinement(c, fr.field(c, spacing, Fs[0].shape, A), trail, fr.STOPS[stop], me)
