"""numpy restatement of the masked demons contract (include/sift3d_amd.h, "Masks in demons"), built on the unmasked
restatements.

The force terms are demons_restatement.force_terms, unchanged; their inside array is and-ed with the two mask tests
(mask_restatement.mask_in: a float32 compare w >= 0.5, on the fixed mask at p and on the moving mask at the voxel
floor(q + 0.5), q = (double) p + (double) u(p) per axis), and delta, s_d and the sums are redone over it.  With masks
None the functions are the unmasked restatements' arithmetic on the unmasked inside array.  The iterations are the
unmasked restatements' loops with that force; the blurs, the warp, the exponentials, the bracket and the two grid
transfers are theirs.  The symmetric update's backward force exchanges the masks with the volumes."""
import numpy as np

from tests import demons_restatement as dm
from tests import field_algebra_restatement as fa
from tests import field_restatement as fr
from tests import logdemons_restatement as lg
from tests import multires_restatement as mr
from tests.mask_restatement import mask_in

F32 = np.float32


def counted(field, moving_shape, WF=None, WM=None):
    """inside(p) and W_F(p) in and W_M[floor(q + 0.5)] in; field [3, nz, ny, nx], moving_shape (mz, my, mx)"""
    field = np.asarray(field, F32)
    ins = dm.inside(field, moving_shape)
    if WF is not None:
        assert tuple(np.shape(WF)) == tuple(field.shape[1:])
        ins = ins & mask_in(WF)
    if WM is not None:
        assert tuple(np.shape(WM)) == tuple(moving_shape)
        x, y, z = fr.grid(field.shape[1:])
        idx = []
        for p, ud in zip((x, y, z), field):
            q = p.astype(np.float64) + ud.astype(np.float64)
            with np.errstate(invalid="ignore"):
                idx.append(np.floor(np.where(ins, q, 0.0) + 0.5).astype(np.int64))
        ins = ins & mask_in(np.asarray(WM, F32)[idx[2], idx[1], idx[0]])
    return ins


def ref_force(F, W, field, moving_shape, alpha, WF=None, WM=None):
    """demons_restatement.ref_force over the counted voxels: (delta, s_d (0 where not counted), counted)"""
    num, sg, sd, _ = dm.force_terms(F, W, field, moving_shape)
    ins = counted(field, moving_shape, WF, WM)
    a2 = float(alpha) * float(alpha)
    den = sg + a2 * sd
    live = ins & (den > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        delta = np.stack([np.where(live, (n / den).astype(F32), F32(0.0)) for n in num]).astype(F32)
    return delta, np.where(ins, sd, 0.0), ins


def ref_demons(F, M, field, iterations, alpha, sigma_fluid, sigma_diffusion, so, WF=None, WM=None, update="additive",
               squarings=0):
    """demons_restatement.ref_demons / field_algebra_restatement.ref_demons_diffeo with the masked force"""
    F = np.asarray(F, F32)
    M = np.asarray(M, F32)
    u = np.array(field, F32, copy=True)
    per = []
    for _ in range(int(iterations)):
        W = fr.ref_warp_field(M, u, "linear", 0.0)
        delta, sd, ins = ref_force(F, W, u, M.shape[-3:], alpha, WF, WM)
        per.append((sd, ins))
        if sigma_fluid > 0:
            delta = dm.blur3(delta, so, sigma_fluid)
        if update == "additive":
            u = (u + delta).astype(F32)
        else:
            u = fa.ref_compose(u, fa.ref_exp(delta, squarings))[0]
        if sigma_diffusion > 0:
            u = dm.blur3(u, so, sigma_diffusion)
    return u, per


def _delta(F, M, e, alpha, sigma_fluid, so, WF, WM):
    """logdemons_restatement._delta with the masked force: WF on F's grid (tested at p), WM on M's (at q)"""
    W = fr.ref_warp_field(M, e, "linear", 0.0)
    delta, sd, ins = ref_force(F, W, e, M.shape[-3:], alpha, WF, WM)
    if sigma_fluid > 0:
        delta = dm.blur3(delta, so, sigma_fluid)
    return delta, sd, ins


def ref_logdemons(F, M, velocity, iterations, alpha, sigma_fluid, sigma_diffusion, so, WF=None, WM=None,
                  symmetric=False, bch=1, squarings=0):
    """logdemons_restatement.ref_logdemons with the masked force; the backward force exchanges the masks"""
    F = np.asarray(F, F32)
    M = np.asarray(M, F32)
    v = np.array(velocity, F32, copy=True)
    per = []
    for _ in range(int(iterations)):
        df, sd, ins = _delta(F, M, lg.ref_exp(v, squarings), alpha, sigma_fluid, so, WF, WM)
        per.append((sd, ins))
        zf = lg.ref_bracket(v, df, "bch1") if bch else (v + df).astype(F32)
        if symmetric:
            db = _delta(M, F, lg.ref_exp(v, squarings, True), alpha, sigma_fluid, so, WM, WF)[0]
            n = (v * F32(-1.0)).astype(F32)
            zb = lg.ref_bracket(n, db, "bch1") if bch else (n + db).astype(F32)
            v = (F32(0.5) * (zf - zb)).astype(F32)
        else:
            v = zf
        if sigma_diffusion > 0:
            v = dm.blur3(v, so, sigma_diffusion)
    return v, per


def mask_pyramid(w, levels):
    """[w, R(w), R(R(w)), ...] of the float mask (restrict2, scale 1), or [None] * levels"""
    if w is None:
        return [None] * levels
    return mr.ref_pyramid(np.ascontiguousarray(w, F32), levels)


def ref_multires(Fs, Ms, field, iterations, alpha, sigma_fluid, sigma_diffusion, so, WFs=None, WMs=None,
                 update="additive", squarings=0, log=None):
    """multires_restatement.ref_multires / logdemons_restatement.ref_logdemons_multires with per-level masks (lists
    with None allowed, or None).  log: None for the displacement updates, else dict(symmetric=, bch=, squarings=)"""
    levels = len(Fs)
    assert len(Ms) == levels and len(iterations) == levels
    WFs = [None] * levels if WFs is None else list(WFs)
    WMs = [None] * levels if WMs is None else list(WMs)
    assert len(WFs) == levels and len(WMs) == levels
    us = [np.array(field, F32, copy=True)]
    for _ in range(1, levels):
        us.append(mr.ref_restrict(us[-1], 0.5))
    per = []
    for l in range(levels - 1, -1, -1):
        if log is None:
            us[l], p = ref_demons(Fs[l], Ms[l], us[l], iterations[l], alpha, sigma_fluid, sigma_diffusion, so, WFs[l],
                                  WMs[l], update, squarings)
        else:
            us[l], p = ref_logdemons(Fs[l], Ms[l], us[l], iterations[l], alpha, sigma_fluid, sigma_diffusion, so,
                                     WFs[l], WMs[l], **log)
        per.extend(p)
        if l > 0:
            us[l - 1] = mr.ref_prolong(us[l], us[l - 1].shape[1:])
    return us[0], per
