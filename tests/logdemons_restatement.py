"""numpy restatement of the log-domain demons contract (include/sift3d_amd.h, "Log-domain demons").

The Lie bracket is written out in float32 numpy in the header's order with field_restatement.ref_gradient
(numpy.gradient's rules); the signed exponential scales by -2^-K and squares with
field_algebra_restatement.ref_compose; the iteration reuses demons_restatement's force and blur and
field_restatement's warp, and the pyramid multires_restatement's two transfers."""
import numpy as np

from tests import demons_restatement as dm
from tests import field_algebra_restatement as fa
from tests import field_restatement as fr
from tests import multires_restatement as mr

F32 = np.float32
AXES = (2, 1, 0)                                             # x, y, z of a [nz, ny, nx] channel


def ref_bracket(a, b, mode="bracket"):
    """[a, b] = J_a b - J_b a ("bracket") or (a + b) + 0.5f * [a, b] ("bch1"); a, b [3, nz, ny, nx] float32"""
    a = np.asarray(a, F32)
    b = np.asarray(b, F32)
    out = np.empty_like(a)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(3):
            ga = [fr.ref_gradient(a[d], ax) for ax in AXES]
            gb = [fr.ref_gradient(b[d], ax) for ax in AXES]
            t = (ga[0] * b[0] + ga[1] * b[1]) + ga[2] * b[2]
            s = (gb[0] * a[0] + gb[1] * a[1]) + gb[2] * a[2]
            br = t - s
            out[d] = br if mode == "bracket" else (a[d] + b[d]) + F32(0.5) * br
    return out.astype(F32)


def ref_exp(v, squarings, negate=False):
    """exp(v) (field_algebra_restatement.ref_exp) or, with negate, exp(-v): w_0 = v * (-2^-K), then K squarings"""
    if not negate:
        return fa.ref_exp(v, squarings)
    w = (np.asarray(v, F32) * F32(-(2.0 ** -squarings))).astype(F32)
    for _ in range(squarings):
        w = fa.ref_compose(w, w)[0]
    return w


def _delta(F, M, e, alpha, sigma_fluid, so):
    """steps 2-4: the force of F against M read through e, blurred; (delta, s_d, inside)"""
    W = fr.ref_warp_field(M, e, "linear", 0.0)
    delta, sd, ins = dm.ref_force(F, W, e, M.shape[-3:], alpha)
    if sigma_fluid > 0:
        delta = dm.blur3(delta, so, sigma_fluid)
    return delta, sd, ins


def ref_logdemons(F, M, velocity, iterations, alpha, sigma_fluid, sigma_diffusion, so, symmetric=False, bch=1,
                  squarings=0):
    """(velocity after `iterations` iterations, [(s_d, inside) of the forward force per iteration])"""
    F = np.asarray(F, F32)
    M = np.asarray(M, F32)
    v = np.array(velocity, F32, copy=True)
    per = []
    for _ in range(int(iterations)):
        df, sd, ins = _delta(F, M, ref_exp(v, squarings), alpha, sigma_fluid, so)
        per.append((sd, ins))
        zf = ref_bracket(v, df, "bch1") if bch else (v + df).astype(F32)
        if symmetric:
            db = _delta(M, F, ref_exp(v, squarings, True), alpha, sigma_fluid, so)[0]
            n = (v * F32(-1.0)).astype(F32)
            zb = ref_bracket(n, db, "bch1") if bch else (n + db).astype(F32)
            v = (F32(0.5) * (zf - zb)).astype(F32)
        else:
            v = zf
        if sigma_diffusion > 0:
            v = dm.blur3(v, so, sigma_diffusion)
    return v, per


def ref_logdemons_multires(Fs, Ms, velocity, iterations, alpha, sigma_fluid, sigma_diffusion, so, symmetric=False,
                           bch=1, squarings=0):
    """the pyramid of multires_restatement.ref_multires with ref_logdemons on every level"""
    levels = len(Fs)
    assert len(Ms) == levels and len(iterations) == levels
    vs = [np.array(velocity, F32, copy=True)]
    for _ in range(1, levels):
        vs.append(mr.ref_restrict(vs[-1], 0.5))
    per = []
    for l in range(levels - 1, -1, -1):
        vs[l], p = ref_logdemons(Fs[l], Ms[l], vs[l], iterations[l], alpha, sigma_fluid, sigma_diffusion, so,
                                 symmetric, bch, squarings)
        per.extend(p)
        if l > 0:
            vs[l - 1] = mr.ref_prolong(vs[l], vs[l - 1].shape[1:])
    return vs[0], per


def work_floats(nx, ny, nz, nc, symmetric, levels):
    """the header's scratch formula"""
    def pad4(x):
        return (x + 3) // 4 * 4
    s = 1 if symmetric else 0
    total = pad4(8192 + 4 * s + (nc + 14 + 6 * s) * nx * ny * nz)
    for _ in range(1, levels):
        nx, ny, nz = (nx + 1) // 2, (ny + 1) // 2, (nz + 1) // 2
        total += pad4(3 * nx * ny * nz)
    return total


def unsigned_zero(a):
    """the array with -0.0 replaced by +0.0 (x + 0.0f), for comparisons of bits up to the sign of zero"""
    return (np.asarray(a, F32) + F32(0.0)).astype(F32)
