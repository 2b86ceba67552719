"""numpy restatement of the local cross-correlation contract (include/sift3d_amd.h, "Local cross-correlation").

float64 / float32 numpy, word for word after the header: validity is the masked demons force's rule
(demons_mask_restatement.counted); box() is 3 (2r + 1) shifted adds of zero-padded arrays, x then y then z, each
ascending from +0.0; the per-voxel arithmetic is written in the header's order.  The driver is built from the helpers
of the other restatements: field_restatement.ref_warp_field and ref_gradient, demons_restatement.blur3 (the oracle's
blur), field_algebra_restatement.ref_exp and ref_compose, multires_restatement.ref_restrict and ref_prolong.  Nothing
here imports the library under test."""
import numpy as np

from tests import demons_mask_restatement as dk
from tests import demons_restatement as dm
from tests import field_algebra_restatement as fa
from tests import field_restatement as fr
from tests import multires_restatement as mr

F32 = np.float32
F64 = np.float64
TAU = 2.0 ** -30
MAX_RADIUS = 4


def box(t, r):
    """box(t): the separable window sums of a float64 volume [nz, ny, nx] in the contract's order"""
    t = np.asarray(t, F64)
    w = 2 * r + 1
    for ax in (2, 1, 0):                                     # x, y, z
        n = t.shape[ax]
        pad = [(0, 0)] * 3
        pad[ax] = (r, r)
        p = np.pad(t, pad)                                   # off-grid positions hold +0.0
        s = np.zeros_like(t)                                 # every sum from +0.0
        for j in range(w):                                   # offsets -r .. r ascending
            sl = [slice(None)] * 3
            sl[ax] = slice(j, j + n)
            s = s + p[tuple(sl)]
        t = s
    return t


def valid(u, moving_shape, WF=None, WM=None):
    """v(p) as a bool array: k_demons_force<true>'s rule"""
    return dk.counted(u, moving_shape, WF, WM)


def sums(F, W, v, r):
    """(n, sf, sw, sff, sww, sfw): the six window sums; an invalid voxel contributes +0.0 (a select)"""
    f = np.where(v, np.asarray(F, F32).astype(F64), 0.0)
    w = np.where(v, np.asarray(W, F32).astype(F64), 0.0)
    return (box(v.astype(F64), r), box(f, r), box(w, r), box(f * f, r), box(w * w, r), box(f * w, r))


def stats(F, W, v, r):
    """(cc float64, coef float64 [4], counted bool): the statistics pass per voxel"""
    n, sf, sw, sff, sww, sfw = sums(F, W, v, r)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        A = sfw - (sf * sw) / n
        B = sff - (sf * sf) / n
        C = sww - (sw * sw) / n
        counted = v & (n >= 2.0) & (B > TAU * sff) & (C > TAU * sww)
        cc = (A * A) / (B * C)
        a = (2.0 * A) / (B * C)
        b = (2.0 * cc) / C
        am = a * (sf / n)
        bm = b * (sw / n)
    z = np.zeros_like(n)
    cc, a, am, b, bm = (np.where(counted, t, z) for t in (cc, a, am, b, bm))
    return cc, np.stack([a, am, b, bm]), counted


def ref_lncc(F, W, u, moving_shape, r, WF=None, WM=None):
    """(cc map float32, coef float64 [4, nz, ny, nx], sum float, count int, cc float64) of one statistics pass"""
    v = valid(u, moving_shape, WF, WM)
    cc, coef, counted = stats(F, W, v, r)
    return cc.astype(F32), coef, float(np.sum(cc[counted], dtype=F64)), int(np.count_nonzero(counted)), cc


def gradient(F, W, v, coef, r):
    """g(q) float64: the exact derivative of sum_p cc(p) with respect to W(q), validity held fixed (0 where invalid)"""
    ba, bam, bb, bbm = (box(c, r) for c in coef)
    f = np.asarray(F, F32).astype(F64)
    w = np.asarray(W, F32).astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        g = (f * ba - bam) - (w * bb - bbm)
    return np.where(v, g, 0.0)


def ref_force(F, W, u, moving_shape, r, coef, WF=None, WM=None):
    """phi [3, nz, ny, nx] float32: (float)(g * (double) d_e W) where valid, +0.0f elsewhere"""
    v = valid(u, moving_shape, WF, WM)
    g = gradient(F, W, v, coef, r)
    W = np.asarray(W, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        phi = [np.where(v, (g * fr.ref_gradient(W, ax).astype(F64)).astype(F32), F32(0.0)) for ax in (2, 1, 0)]
    return np.stack(phi).astype(F32)


def ref_normalize(phi, step):
    """the field scaled so that its longest vector is `step` voxels; m2 == 0 leaves it"""
    phi = np.asarray(phi, F32)
    p = phi.astype(F64)
    m2 = float(np.max((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2])) if phi[0].size else 0.0
    if not m2 > 0.0:
        return phi.copy()
    s = F32(float(step) / np.sqrt(m2))
    return (s * phi).astype(F32)


def ref_demons_lncc(F, M, field, iterations, r, step, sigma_fluid, sigma_diffusion, so, WF=None, WM=None,
                    update="additive", squarings=0):
    """(field after `iterations` iterations, [(sum cc, count) per iteration]); F [nz, ny, nx], M [mz, my, mx]"""
    F = np.asarray(F, F32)
    M = np.asarray(M, F32)
    u = np.array(field, F32, copy=True)
    per = []
    for _ in range(int(iterations)):
        W = fr.ref_warp_field(M, u, "linear", 0.0)
        _, coef, s, c, _ = ref_lncc(F, W, u, M.shape, r, WF, WM)
        per.append((s, c))
        phi = ref_force(F, W, u, M.shape, r, coef, WF, WM)
        if sigma_fluid > 0:
            phi = dm.blur3(phi, so, sigma_fluid)
        phi = ref_normalize(phi, step)
        if update == "additive":
            u = (u + phi).astype(F32)
        else:
            u = fa.ref_compose(u, fa.ref_exp(phi, squarings))[0]
        if sigma_diffusion > 0:
            u = dm.blur3(u, so, sigma_diffusion)
    return u, per


def ref_multires_lncc(Fs, Ms, field, iterations, r, step, sigma_fluid, sigma_diffusion, so, WFs=None, WMs=None,
                      update="additive", squarings=0):
    """"Multi-resolution demons" around ref_demons_lncc: (the finest field, [(sum, count)] in the order run)"""
    levels = len(Fs)
    WFs = [None] * levels if WFs is None else list(WFs)
    WMs = [None] * levels if WMs is None else list(WMs)
    us = [np.array(field, F32, copy=True)]
    for _ in range(1, levels):
        us.append(mr.ref_restrict(us[-1], 0.5))
    per = []
    for l in range(levels - 1, -1, -1):
        us[l], p = ref_demons_lncc(Fs[l], Ms[l], us[l], iterations[l], r, step, sigma_fluid, sigma_diffusion, so,
                                   WFs[l], WMs[l], update, squarings)
        per.extend(p)
        if l > 0:
            us[l - 1] = mr.ref_prolong(us[l], us[l - 1].shape[1:])
    return us[0], per


def gamma(n):
    """gamma_n = n u / (1 - n u), u = 2^-53 (demons_restatement.gamma)"""
    return dm.gamma(n)
