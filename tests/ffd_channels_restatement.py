"""numpy restatement of the multi-channel free-form deformation contract (include/sift3d_amd.h, "Multi-channel
free-form deformation"), on top of tests/ffd_restatement.py and tests/mask_restatement.py.

One field, one inside test and one pair of masks for all channels; per channel the sample and its gradient are
ffd_restatement.sample_grad's on that channel; e_c = m_c - f_c in float32; the force S_d = ((E_0 g_0d + E_1 g_1d) + ...)
in float64 in ascending c, starting from channel 0's product (every product of two widened floats is exact, so S_d is
defined bit for bit); n counts voxels; S_ee is the correctly rounded sum of all E_c E_c; Gc is ffd_restatement.adjoint
of S, its sum |term| taken over the channels' own terms |W E_c g_cd|, which is what the header's bound is stated on.
With nc == 1 every number is ffd_restatement.evaluate's.  The driver is ffd_restatement.refine's loop over the
caller's levels."""
import collections

import numpy as np

from tests import ffd_restatement as fr
from tests import mask_restatement as mk
from tests.multires_restatement import ref_restrict

F32 = np.float32
Record = collections.namedtuple("Record", fr.Record._fields + ("S",))


def evaluate(F, M, lattice, spacing, A=None, WF=None, WM=None, exact=True):
    """(Record, field) for stacks F [nc, oz, oy, ox], M [nc, nz, ny, nx]; Record.S is the force [3, oz, oy, ox]"""
    F = np.ascontiguousarray(F, F32)
    M = np.ascontiguousarray(M, F32)
    assert F.ndim == 4 and M.ndim == 4 and F.shape[0] == M.shape[0] >= 1
    shape = F.shape[1:]
    u = fr.field(lattice, spacing, shape, A)
    ins = None
    S, mag, see_terms = None, None, []
    for c in range(F.shape[0]):
        m, gx, gy, gz, inside = fr.sample_grad(M[c], u)
        if ins is None:
            ins = inside & mk.counted(mk.coords(u, shape), M.shape[1:], WF, WM)
        E = np.where(ins, (m - F[c]).astype(F32).astype(np.float64), 0.0)
        P = np.stack([E * np.where(ins, v.astype(np.float64), 0.0) for v in (gx, gy, gz)])     # exact products
        S = P if S is None else S + P
        mag = np.abs(P) if mag is None else mag + np.abs(P)
        see_terms.append(E * E)
    S = np.where(ins, S, 0.0)                                            # a voxel that is not counted stores +0.0
    see_terms = np.stack(see_terms)
    fsum = fr._fsum if exact else (lambda a: float(np.sum(a)))
    parts = [fr.adjoint(Sd, spacing, exact) for Sd in S]
    terms = [fr.adjoint(a, spacing, False)[0] for a in mag]              # sum_p sum_c |W E_c g_cd|
    rec = Record(int(ins.sum()), fsum(see_terms), np.stack([p[0] for p in parts]), float(see_terms.sum()),
                 np.stack(terms), parts[0][2], S)
    return rec, u


def pyramid(v, levels):
    """[v, restrict(v), ...] of a volume, a stack (channel by channel) or None"""
    if v is None:
        return [None] * levels
    out = [np.ascontiguousarray(v, F32)]
    for _ in range(1, levels):
        a = out[-1]
        out.append(ref_restrict(a) if a.ndim == 3 else np.stack([ref_restrict(ch) for ch in a]))
    return out


def refine(Fs, Ms, A=None, WFs=None, WMs=None, spacing=8, bending_weight=0.005, max_evaluations=60, step0=1.0,
           step_max=4.0, tol=0.01, min_overlap=0.5):
    """the header's driver over the caller's levels (stacks per level, level 0 the finest; masks per level or None);
    trail entries (E, msd = S_ee / n, R, n, step, accepted, level)"""
    levels = len(Fs)
    A = None if A is None else np.array(A, np.float64).reshape(3, 4)
    WFs = [None] * levels if WFs is None else WFs
    WMs = [None] * levels if WMs is None else WMs
    for _ in range(1, levels):
        if A is not None:
            A[:, 3] = A[:, 3] * 0.5
    trail, stop, c = [], 1, None

    def ev(l, lat):
        rec, _ = evaluate(Fs[l], Ms[l], lat, spacing, A, WFs[l], WMs[l], exact=False)
        R, dR, _, _ = fr.bending(lat, spacing)
        g, gmax = fr.gradient(rec, dR, bending_weight)
        return rec, R, g, gmax, fr.cost(rec, R, bending_weight)

    def entry(rec, R, E, s, acc, l):
        return (E, rec.see / rec.n if rec.n else float("nan"), R, rec.n, s, acc, l)

    for l in range(levels - 1, -1, -1):
        shape = Fs[l].shape[1:]
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
    return fr.Refinement(c, fr.field(c, spacing, Fs[0].shape[1:], A), trail, fr.STOPS[stop])


def descriptor_levels(v, levels, sigma, so):
    """the descriptor stacks of a volume per level: tests/dense_restatement.py on every level's restricted volume"""
    from tests import dense_restatement as dr
    return [dr.dense_descriptors(a, so, sigma) for a in pyramid(v, levels)]
