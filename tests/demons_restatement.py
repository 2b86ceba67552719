"""numpy restatement of the dense demons contract (include/sift3d_amd.h, "Dense demons refinement").

The force is written out here in float32 / float64 numpy in the header's order: the inside test of warp_field,
d_c = F_c - W_c, the symmetric gradient g_ce = 0.5f * (d_e F_c + d_e W_c) with numpy.gradient's rules
(field_restatement.ref_gradient), the three double sums over c in channel order, and delta_e = (float)(num_e / den).
The iteration reuses field_restatement.ref_warp_field for the warp and the oracle's blur / gauss_taps (the
detector's blur, pinned to the reference) for the two smoothings, as dense_restatement.py does for its window."""
import numpy as np

from tests import field_restatement as fr

F32 = np.float32


def inside(field, moving_shape, origin=(0, 0, 0)):
    """warp_field's inside test of q_d = (double) p_d + (double) u_d against the moving grid (mz, my, mx); the
    field may be a block of a larger grid whose voxel (0, 0, 0) is voxel origin = (x0, y0, z0) of the grid"""
    mz, my, mx = moving_shape
    x, y, z = fr.grid(field.shape[1:])
    x, y, z = x + origin[0], y + origin[1], z + origin[2]
    ok = np.ones(field.shape[1:], bool)
    for p, ud, m in zip((x, y, z), field, (mx, my, mz)):
        q = p.astype(np.float64) + np.asarray(ud, np.float32).astype(np.float64)
        ok &= (q >= 0.0) & (q <= float(m - 1))
    return ok


def force_terms(F, W, field, moving_shape, origin=(0, 0, 0)):
    """(num [3], s_g, s_d, inside) per voxel, float64 sums over the channels in order; F, W [nc, nz, ny, nx]"""
    F = np.asarray(F, np.float32)
    W = np.asarray(W, np.float32)
    if F.ndim == 3:
        F, W = F[None], W[None]
    shape = F.shape[1:]
    num = [np.zeros(shape, np.float64) for _ in range(3)]
    sg = np.zeros(shape, np.float64)
    sd = np.zeros(shape, np.float64)
    axes = (2, 1, 0)                                         # x, y, z of a [nz, ny, nx] channel
    for c in range(F.shape[0]):
        d = F[c] - W[c]
        g = [F32(0.5) * (fr.ref_gradient(F[c], a) + fr.ref_gradient(W[c], a)) for a in axes]
        dd = d.astype(np.float64)
        for e in range(3):
            num[e] = num[e] + dd * g[e].astype(np.float64)
        g64 = [ge.astype(np.float64) for ge in g]
        sg = sg + ((g64[0] * g64[0] + g64[1] * g64[1]) + g64[2] * g64[2])
        sd = sd + dd * dd
    return num, sg, sd, inside(field, moving_shape, origin)


def ref_force(F, W, field, moving_shape, alpha, origin=(0, 0, 0)):
    """(delta [3, nz, ny, nx] float32, s_d [nz, ny, nx] float64 (0 outside), inside mask).  For a block of a larger
    grid (origin as in inside()) the derivatives on the block's faces are one-sided: only voxels one inside a
    face that is not the grid's own are the grid's values."""
    num, sg, sd, ins = force_terms(F, W, field, moving_shape, origin)
    a2 = float(alpha) * float(alpha)
    den = sg + a2 * sd
    live = ins & (den > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        delta = np.stack([np.where(live, (n / den).astype(np.float32), F32(0.0)) for n in num]).astype(np.float32)
    return delta, np.where(ins, sd, 0.0), ins


def ref_stats(sd, ins):
    """(sum, count): the float64 numpy sum of the inside s_d and the inside count"""
    return float(np.sum(sd[ins], dtype=np.float64)), int(np.count_nonzero(ins))


def blur3(v, so, sigma):
    """each of 3 channels through the oracle's blur (units 1, unit 1.0) with the taps of sigma"""
    taps = so.gauss_taps(sigma)
    return np.stack([so.blur(v[c], taps, (1, 1, 1), unit=1.0) for c in range(3)]).astype(np.float32)


def ref_demons(F, M, field, iterations, alpha, sigma_fluid, sigma_diffusion, so):
    """(field after `iterations` iterations, [(s_d, inside) per iteration]); F [nc, nz, ny, nx] (or 3-D),
    M [nc, mz, my, mx] (or 3-D)"""
    F = np.asarray(F, np.float32)
    M = np.asarray(M, np.float32)
    u = np.array(field, np.float32, copy=True)
    per = []
    for _ in range(int(iterations)):
        W = fr.ref_warp_field(M, u, "linear", 0.0)
        delta, sd, ins = ref_force(F, W, u, M.shape[-3:], alpha)
        per.append((sd, ins))
        if sigma_fluid > 0:
            delta = blur3(delta, so, sigma_fluid)
        u = (u + delta).astype(np.float32)
        if sigma_diffusion > 0:
            u = blur3(u, so, sigma_diffusion)
    return u, per


def gamma(n):
    """gamma_n = n u / (1 - n u), u = 2^-53: the bound on the relative error of any order of summing n
    non-negative doubles"""
    nu = float(n) * 2.0 ** -53
    return nu / (1.0 - nu)
