"""numpy restatement of field composition, the exponential, the inverse and the diffeomorphic demons update
(include/sift3d_amd.h, "Field composition, exponential and inverse").

The composition sample is warp_field's LINEAR sample (field_restatement.ref_field_points, i.e. the affine warp's
restatement with the identity map) taken at the sample point clamped onto u's grid; the residual statistics follow
the header in float64.  The exponential and the inverse chain it as the drivers do, and the diffeomorphic demons
driver reuses demons_restatement's force and blur."""
import numpy as np

from tests import demons_restatement as dm
from tests import field_restatement as fr
from tests.test_warp import ref_warp_points
from tests.tps_restatement import IDENT

F32 = np.float32
QNAN = np.float32(np.nan)


def ref_compose(u, v, mode="compose", origin=(0, 0, 0)):
    """(out [3, oz, oy, ox] float32, (sum, max, count, inside)) of one composition sample pass: u [3, uz, uy, ux],
    v [3, oz, oy, ox] float32; mode "compose" (out = v + s) or "invert" (out = -s).  v may be a block of a larger
    output grid whose voxel (0, 0, 0) is voxel origin = (x0, y0, z0) of the grid (a voxel reads v at itself only)."""
    u = np.asarray(u, np.float32)
    v = np.asarray(v, np.float32)
    ushape = u.shape[1:]
    uz, uy, ux = ushape
    x, y, z = fr.grid(v.shape[1:])
    x, y, z = x + origin[0], y + origin[1], z + origin[2]
    q = [p.astype(np.float64) + vd.astype(np.float64) for p, vd in zip((x, y, z), v)]
    nan = np.isnan(q[0]) | np.isnan(q[1]) | np.isnan(q[2])
    ins = np.ones(q[0].shape, bool)
    for qd, n in zip(q, (ux, uy, uz)):
        ins &= (qd >= 0.0) & (qd <= float(n - 1))
    qc = []
    for qd, n in zip(q, (ux, uy, uz)):
        c = np.where(ins, qd, np.minimum(np.maximum(qd, 0.0), float(n - 1)))
        qc.append(np.where(nan, 0.0, c))
    s = []
    for c in range(3):
        flat = np.ascontiguousarray(u[c]).reshape(-1)
        val, _ = ref_warp_points(lambda k: flat[k], ushape, IDENT, qc[0], qc[1], qc[2], "linear", 0.0)
        s.append(val.astype(np.float32))
    r = [(vd + sd).astype(np.float32) for vd, sd in zip(v, s)]
    out = np.stack(r if mode == "compose" else [-sd for sd in s]).astype(np.float32)
    out[:, nan] = QNAN
    r64 = [rd.astype(np.float64) for rd in r]
    m = np.sqrt((r64[0] * r64[0] + r64[1] * r64[1]) + r64[2] * r64[2])
    ok = ~nan
    mm = m[ok]
    stats = (float(np.sum(mm, dtype=np.float64)), float(mm.max()) if mm.size else 0.0, int(ok.sum()),
             int(ins.sum()))
    return out, stats


def ref_exp(v, squarings):
    """exp(v) by scaling and squaring: w_0 = v * 2^-K (float), w_{k+1} = COMPOSE(w_k, w_k); K == 0 copies v"""
    v = np.asarray(v, np.float32)
    if squarings == 0:
        return v.copy()
    w = (v * np.float32(2.0 ** -squarings)).astype(np.float32)
    for _ in range(squarings):
        w = ref_compose(w, w)[0]
    return w


def ref_invert(u, w0, iterations):
    """(w_N, [stats of w_0 .. w_N]): w_{k+1} = INVERT(u, w_k), then a statistics-only pass on w_N"""
    w = np.asarray(w0, np.float32).copy()
    recs = []
    for _ in range(int(iterations)):
        w, st = ref_compose(u, w, "invert")
        recs.append(st)
    recs.append(ref_compose(u, w, "invert")[1])
    return w, recs


def ref_demons_diffeo(F, M, field, iterations, alpha, sigma_fluid, sigma_diffusion, squarings, so):
    """(field after `iterations` diffeomorphic iterations, [(s_d, inside) per iteration]): demons_restatement's
    steps 1-3 and 5, step 4 replaced by u <- COMPOSE(u, exp(delta))"""
    F = np.asarray(F, np.float32)
    M = np.asarray(M, np.float32)
    u = np.array(field, np.float32, copy=True)
    per = []
    for _ in range(int(iterations)):
        W = fr.ref_warp_field(M, u, "linear", 0.0)
        delta, sd, ins = dm.ref_force(F, W, u, M.shape[-3:], alpha)
        per.append((sd, ins))
        if sigma_fluid > 0:
            delta = dm.blur3(delta, so, sigma_fluid)
        e = ref_exp(delta, squarings)
        u = ref_compose(u, e)[0]
        if sigma_diffusion > 0:
            u = dm.blur3(u, so, sigma_diffusion)
    return u, per


def lipschitz(u):
    """L = max_d sum_e max |Delta_e u_d| over grid edges: the infinity-norm Lipschitz constant of u's trilinear
    interpolant (float64)"""
    u = np.asarray(u, np.float64)
    best = 0.0
    for d in range(3):
        tot = 0.0
        for ax in (3, 2, 1):                                    # x, y, z of a [3, z, y, x] field
            if u.shape[ax] > 1:
                tot += float(np.abs(np.diff(u[d:d + 1], axis=ax)).max())
        best = max(best, tot)
    return best
