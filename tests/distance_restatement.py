"""Numpy restatement of the distance contract (include/sift3d_amd.h, "Distance transforms and surface distances"), word
for word: the squared distance as a float32 brute force over ALL feature voxels in the definition's operation order
(no separable passes, so it shares nothing with the kernels but the definition), the root, the signed distance, the
six-neighbour surface of a label, the two sorted lists and the host measures in double."""
import collections

import numpy as np

SurfaceMeasures = collections.namedtuple("SurfaceMeasures",
                                         "hausdorff hd95 assd mean_fm mean_mf max_fm max_mf n_fixed n_moving")
INF = np.float32(np.inf)


def weights(spacing):
    """(w_x, w_y, w_z), w_a = (float) (s_a * s_a) with the product in double"""
    s = np.ones(3) if spacing is None else np.asarray(spacing, np.float64).reshape(3)
    return (s * s).astype(np.float32)


def mask_in(mask):
    """w >= 0.5f: one float compare, so a NaN is out"""
    with np.errstate(invalid="ignore"):
        return np.asarray(mask, np.float32) >= np.float32(0.5)


def distance_sq(mask, spacing=None, invert=False):
    """D2(p) = min over every feature voxel q of ((w_x * (float) dx dx) + (w_y * (float) dy dy)) + (w_z * (float) dz dz)
    in float32, +inf without a feature"""
    feat = mask_in(mask)
    if invert:
        feat = ~feat
    wx, wy, wz = weights(spacing)
    nz, ny, nx = feat.shape
    out = np.full(feat.shape, INF, np.float32)
    q = np.argwhere(feat)                                                        # rows (z, y, x)
    if not len(q):
        return out
    qz, qy, qx = (q[:, a].astype(np.int64)[None, :] for a in range(3))
    yy, xx = (v.reshape(-1, 1).astype(np.int64) for v in np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij"))
    for z in range(nz):
        dx, dy, dz = xx - qx, yy - qy, z - qz
        c = (wx * (dx * dx).astype(np.float32) + wy * (dy * dy).astype(np.float32)) + wz * (dz * dz).astype(np.float32)
        assert c.dtype == np.float32
        out[z] = c.min(axis=1).reshape(ny, nx)
    return out


def distance(mask, spacing=None, invert=False):
    return np.sqrt(distance_sq(mask, spacing, invert))                           # float32, correctly rounded


def distance_signed(mask, spacing=None):
    """+sqrtf(D2 to the set) outside the set, -sqrtf(D2 to its complement) inside it"""
    inside = mask_in(mask)
    return np.where(inside, -np.sqrt(distance_sq(mask, spacing, True)), np.sqrt(distance_sq(mask, spacing, False)))


def label_surface(L, k):
    """p is on the surface when L(p) == (float) k and one of its six face neighbours (one beyond the grid included) is
    not in the label: (surface as float32 0 / 1, count)"""
    S = np.asarray(L, np.float32) == np.float32(k)
    P = np.pad(S, 1, constant_values=False)
    core = (P[:-2, 1:-1, 1:-1] & P[2:, 1:-1, 1:-1] & P[1:-1, :-2, 1:-1] & P[1:-1, 2:, 1:-1] & P[1:-1, 1:-1, :-2]
            & P[1:-1, 1:-1, 2:])
    surf = S & ~core
    return surf.astype(np.float32), int(surf.sum())


def surface_lists(LF, LM, k, spacing=None):
    """(d_fm, d_mf) sorted ascending, float32: D to the moving surface at the fixed surface's voxels, and the other way"""
    sf, _ = label_surface(LF, k)
    sm, _ = label_surface(LM, k)
    d_fm = np.sort(distance(sm, spacing)[sf >= 0.5])
    d_mf = np.sort(distance(sf, spacing)[sm >= 0.5])
    return d_fm.astype(np.float32), d_mf.astype(np.float32)


def ascending_sum(d):
    acc = 0.0
    for v in np.asarray(d, np.float64):
        acc = acc + float(v)
    return acc


def measures(d_fm, d_mf):
    """the host measures from the two sorted lists, in double, in the header's order"""
    n_f, n_m = len(d_fm), len(d_mf)
    if n_f == 0 or n_m == 0:
        nan = float("nan")
        return SurfaceMeasures(nan, nan, nan, nan, nan, nan, nan, n_f, n_m)
    a, b = np.asarray(d_fm, np.float64), np.asarray(d_mf, np.float64)
    sum_fm, sum_mf = ascending_sum(a), ascending_sum(b)
    max_fm, max_mf = float(a[-1]), float(b[-1])
    n = n_f + n_m
    d = np.sort(np.concatenate([a, b]))
    pos = 0.95 * float(n - 1)
    i = int(np.floor(pos))
    hd95 = float(d[i]) + (pos - float(i)) * (float(d[min(i + 1, n - 1)]) - float(d[i]))
    return SurfaceMeasures(max(max_fm, max_mf), hd95, (sum_fm + sum_mf) / float(n), sum_fm / float(n_f),
                           sum_mf / float(n_m), max_fm, max_mf, n_f, n_m)


def surface_distances(LF, LM, labels, spacing=None):
    return [measures(*surface_lists(LF, LM, k, spacing)) for k in labels]
