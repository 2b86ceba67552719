"""numpy restatement of the thin-plate spline contract (include/sift3d_amd.h, "Thin-plate spline").

The coordinates q(p) follow the contract in IEEE float64 (the affine part, warp_affine's order) and
float32 (the radial sum, in point order, no contraction, np.sqrt correctly rounded).  Sampling at q
is the affine warp's, restated once in tests/test_warp.py: ref_warp_points with the identity map
reads the source at exactly q (1*q + ((0*y + 0*z) + 0) is q for finite q), so it is reused here
rather than copied.  The selection rules of sift3d_amd_tps_fit (duplicates, farthest-point thinning)
are restated too."""
import numpy as np

from tests.test_warp import ref_coords, ref_warp_points

IDENT = np.hstack([np.eye(3), np.zeros((3, 1))])


def ref_radial(ctrl, weights, x, y, z):
    """s_d = s_d + w_i,d * (-r_i) over i in order, from 0.0f, in float32; c_i and w_i are the float32
    values of the device layout.  x, y, z: integer arrays (broadcast together)."""
    c = np.asarray(ctrl, np.float64).reshape(-1, 3).astype(np.float32)
    w = np.asarray(weights, np.float64).reshape(-1, 3).astype(np.float32)
    xf, yf, zf = (np.asarray(v).astype(np.float32) for v in np.broadcast_arrays(x, y, z))
    s = [np.zeros(xf.shape, np.float32) for _ in range(3)]
    for i in range(len(c)):
        dx, dy, dz = xf - c[i, 0], yf - c[i, 1], zf - c[i, 2]
        r = np.sqrt((dx * dx + dy * dy) + dz * dz)
        nr = -r
        for d in range(3):
            s[d] = s[d] + w[i, d] * nr
    return s


def ref_tps_coords(tps, x, y, z):
    """q_d = affine_d(p) + (double) s_d(p)"""
    aff = ref_coords(tps.A, x, y, z)
    s = ref_radial(tps.ctrl, tps.weights, x, y, z)
    return [a + sd.astype(np.float64) for a, sd in zip(aff, s)]


def ref_tps_points(gather, shape, tps, x, y, z, interp="linear", fill=0.0):
    """The restatement at output voxels (x, y, z); gather(flat int64 indices) -> float32 source values."""
    q = ref_tps_coords(tps, x, y, z)
    return ref_warp_points(gather, shape, IDENT, q[0], q[1], q[2], interp, fill)


def ref_tps_warp(src, tps, out_shape, interp="linear", fill=0.0):
    oz, oy, ox = out_shape
    z, y, x = np.meshgrid(np.arange(oz), np.arange(oy), np.arange(ox), indexing="ij")
    flat = np.ascontiguousarray(src).reshape(-1)
    return ref_tps_points(lambda k: flat[k], src.shape, tps, x, y, z, interp, fill)


# ---- the fit's selection rules ---------------------------------------------------------------------
def ref_distinct(src):
    """indices of the distinct src points, ascending; of equal points the lowest index"""
    src = np.asarray(src, np.float64)
    keep, seen = [], set()
    for i, p in enumerate(src):
        key = tuple(float(v) + 0.0 for v in p)         # -0.0 and 0.0 are the same point
        if key not in seen:
            seen.add(key)
            keep.append(i)
    return np.array(keep, np.int64)


def ref_thin(src, cand, mmax):
    """greedy farthest-point sampling of mmax of the points src[cand]: start at cand[0]; add the point
    with the largest squared distance (dx dx + dy dy) + dz dz to its nearest chosen point, the lowest
    position on ties.  Returns the chosen indices, ascending."""
    p = np.asarray(src, np.float64)[cand]
    d = np.full(len(p), np.inf)
    taken = np.zeros(len(p), bool)
    cur = 0
    for s in range(mmax):
        taken[cur] = True
        if s == mmax - 1:
            break
        dx, dy, dz = (p[:, k] - p[cur, k] for k in range(3))
        d = np.minimum(d, (dx * dx + dy * dy) + dz * dz)
        dm = np.where(taken, -1.0, d)
        cur = int(np.argmax(dm))                       # the first maximum: the lowest position
    return np.asarray(cand)[taken]
