"""numpy restatement of the displacement-field contract (include/sift3d_amd.h, "Displacement fields").

A field is float32 u[3][oz][oy][ox] (x, y, z; source voxels), a pull map: output voxel p reads the source at
p + u(p).  The export follows the contract in IEEE float64 (the affine part, warp_affine's order) and float32
(the TPS radial sum, restated once in tests/tps_restatement.py); sampling is the affine warp's, restated in
tests/test_warp.py and reused here with the identity map (1*q + ((0*y + 0*z) + 0) is q for finite q, and a NaN
stays a NaN, i.e. outside).  The Jacobian follows numpy.gradient's rules in float32 and the cofactor expansion
in float64."""
import numpy as np

from tests.test_warp import ref_coords, ref_warp_points
from tests.tps_restatement import IDENT, ref_radial


def grid(out_shape):
    """integer x, y, z arrays of an output grid (oz, oy, ox)"""
    oz, oy, ox = out_shape
    z, y, x = np.meshgrid(np.arange(oz), np.arange(oy), np.arange(ox), indexing="ij")
    return x, y, z


def ref_affine_field_points(A, x, y, z):
    """u_d = (float)(q_d - (double) p_d) at integer points (x, y, z): a list of three float32 arrays"""
    q = ref_coords(A, x, y, z)
    return [(qd - np.asarray(pd).astype(np.float64)).astype(np.float32) for qd, pd in zip(q, (x, y, z))]


def ref_affine_field(A, out_shape):
    return np.stack(ref_affine_field_points(A, *grid(out_shape)))


def ref_tps_field_points(tps, x, y, z):
    """u_d = (float)((affine_d(p) + (double) s_d(p)) - (double) p_d)"""
    aff = ref_coords(tps.A, x, y, z)
    s = ref_radial(tps.ctrl, tps.weights, x, y, z)
    return [((a + sd.astype(np.float64)) - np.asarray(pd).astype(np.float64)).astype(np.float32)
            for a, sd, pd in zip(aff, s, (x, y, z))]


def ref_tps_field(tps, out_shape):
    return np.stack(ref_tps_field_points(tps, *grid(out_shape)))


def ref_field_points(gather, shape, u, x, y, z, interp="linear", fill=0.0):
    """One channel at output voxels (x, y, z), with u = (ux, uy, uz) float32 at those voxels: the source
    at q_d = (double) p_d + (double) u_d.  Returns (values, inside)."""
    q = [np.asarray(p).astype(np.float64) + np.asarray(ud, np.float32).astype(np.float64)
         for p, ud in zip((x, y, z), u)]
    return ref_warp_points(gather, shape, IDENT, q[0], q[1], q[2], interp, fill)


def ref_warp_field(src, field, interp="linear", fill=0.0):
    """src [nz, ny, nx] or [nc, nz, ny, nx] float32, field [3, oz, oy, ox] float32 -> [(nc,) oz, oy, ox]"""
    src = np.asarray(src, np.float32)
    x, y, z = grid(field.shape[1:])
    chans = src[None] if src.ndim == 3 else src
    out = []
    for c in chans:
        flat = np.ascontiguousarray(c).reshape(-1)
        out.append(ref_field_points(lambda k: flat[k], c.shape, field, x, y, z, interp, fill)[0])
    out = np.stack(out).astype(np.float32)
    return out[0] if src.ndim == 3 else out


def ref_gradient(u, axis):
    """d u / d x_axis in float32 by numpy.gradient's rules: (u[i+1] - u[i-1]) * 0.5f inside, u[1] - u[0] and
    u[n-1] - u[n-2] at the ends, 0 on an axis of length 1"""
    u = np.asarray(u, np.float32)
    n = u.shape[axis]
    g = np.zeros_like(u)
    if n == 1:
        return g

    def sl(a, b):
        s = [slice(None)] * u.ndim
        s[axis] = slice(a, b)
        return tuple(s)

    g[sl(0, 1)] = u[sl(1, 2)] - u[sl(0, 1)]
    g[sl(n - 1, n)] = u[sl(n - 1, n)] - u[sl(n - 2, n - 1)]
    if n > 2:
        g[sl(1, n - 1)] = (u[sl(2, n)] - u[sl(0, n - 2)]) * np.float32(0.5)
    return g


def ref_jacobian_det(field):
    """det [oz, oy, ox] float32 of p -> p + u(p): j_de = (d == e) + g_de in float32, the cofactor expansion along
    row 0 in float64 (this order, unfused), rounded to float32"""
    f = np.asarray(field, np.float32)
    axes = (2, 1, 0)                                    # x, y, z of a [oz, oy, ox] channel
    j = [[(np.float32(1.0 if d == e else 0.0) + ref_gradient(f[d], axes[e])).astype(np.float64)
          for e in range(3)] for d in range(3)]
    det = (j[0][0] * (j[1][1] * j[2][2] - j[1][2] * j[2][1]) - j[0][1] * (j[1][0] * j[2][2] - j[1][2] * j[2][0])
           + j[0][2] * (j[1][0] * j[2][1] - j[1][1] * j[2][0]))
    return det.astype(np.float32)


def ref_stats(det):
    """(folded, min, max): folded counts !(det > 0), NaN included; min / max of the non-NaN dets, +inf / -inf
    when there is none"""
    det = np.asarray(det, np.float32)
    folded = int(np.count_nonzero(~(det > 0)))
    ok = det[~np.isnan(det)]
    if ok.size == 0:
        return folded, float("inf"), float("-inf")
    return folded, float(ok.min()), float(ok.max())
