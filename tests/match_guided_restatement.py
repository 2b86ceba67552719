"""numpy restatement of transform-guided (spatially gated) matching: sift3d_hip_nn2_gated, sift3d_amd_spatial_order
and sift3d_amd_matcher_match_guided (sift3d_match.hip, sift3d_register.c; the contract is in include/sift3d_amd.h).

  gate        float32: dx = pa.x - pb.x, dy, dz; d2 = (dx dx + dy dy) + dz dz, each operation rounded once (the unit
              is built without contraction); d2 <= r2f, r2f = (float)(radius * radius) with the product in double;
              a NaN anywhere makes it false;
  top-2       tests/match_restatement.py's e = |b|^2 - 2 a.b with the candidates outside the gate removed, its
              lexicographic top-2 and max(|a|^2 + e, 0);
  boxes       per 128-row block in the walked order: min / max over the points without a NaN coordinate
              (+inf / -inf for none), gap2 in the gate's association, visited = pairs with not gap2 > r2f;
  order       (Morton key of floor(p / cell) - its minimum, clamped to 21 bits; index), non-finite points last;
  decision    the blind matcher's on the gated searches, and d1 <= (float)(max_distance^2) when one is given.
"""
import numpy as np

from tests import match_restatement as mr

F = np.float32
BLOCK = 128


def pos4(xyz):
    """n x 3 (any float type) -> the device layout: float32 n x 4, rounded to nearest, the fourth float 0."""
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    out = np.zeros((len(p), 4), F)
    with np.errstate(over="ignore"):
        out[:, :3] = p.astype(F)
    return out


def r2f(radius):
    with np.errstate(over="ignore"):
        return F(float(radius) * float(radius))


def gate_d2(pa, pb):
    """d2 of every pair (nA x nB float32) in the stated association"""
    pa, pb = np.asarray(pa, F), np.asarray(pb, F)
    with np.errstate(over="ignore", invalid="ignore"):
        dx = pa[:, None, 0] - pb[None, :, 0]
        dy = pa[:, None, 1] - pb[None, :, 1]
        dz = pa[:, None, 2] - pb[None, :, 2]
        return (dx * dx + dy * dy) + dz * dz


def gate(pa, pb, radius):
    with np.errstate(invalid="ignore"):
        return gate_d2(pa, pb) <= r2f(radius)                # (a NaN compares false)


def nn2_gated(a, b, pa, pb, radius):
    """sift3d_hip_nn2_gated: (j int32, d1, d2 float32); independent of the row orders"""
    a = np.ascontiguousarray(a, F)
    b = np.ascontiguousarray(b, F)
    na = mr.row_norms(a)
    if len(b) == 0:
        return mr.top2(np.zeros((len(a), 0), F))
    e = mr.row_norms(b)[None, :] - F(2.0) * mr.dots(a, b)
    return top2_of(e, na, gate(pa, pb, radius))


def top2_of(e, na, ok):
    """the gated top-2 of given e = |b|^2 - 2 a.b (nA x nB float32) and |a|^2: candidates outside ok removed"""
    e = np.where(ok, e, F(np.inf)).astype(F)
    j, e1, e2 = mr.top2(e)
    j = np.where(ok.any(axis=1), j, -1).astype(np.int32)
    with np.errstate(invalid="ignore"):
        d1 = np.maximum(na + e1, F(0.0)).astype(F)
        d2 = np.maximum(na + e2, F(0.0)).astype(F)
    return j, d1, d2


def block_boxes(pos, perm=None):
    """(lo, hi), each nblk x 3 float32: the box of every 128-row block of pos[perm]"""
    p = np.asarray(pos, F)[:, :3]
    if perm is not None:
        p = p[np.asarray(perm)]
    nblk = -(-len(p) // BLOCK)
    lo = np.full((nblk, 3), np.inf, F)
    hi = np.full((nblk, 3), -np.inf, F)
    for k in range(nblk):
        q = p[k * BLOCK:(k + 1) * BLOCK]
        q = q[~np.isnan(q).any(axis=1)]
        if len(q):
            lo[k], hi[k] = q.min(axis=0), q.max(axis=0)
    return lo, hi


def gap2(loA, hiA, loB, hiB):
    """gap2 of every block pair (nblkA x nblkB float32); fmax drops a NaN, as fmaxf does"""
    with np.errstate(over="ignore", invalid="ignore"):
        g = np.fmax(F(0.0), np.fmax(loA[:, None, :] - hiB[None, :, :], loB[None, :, :] - hiA[:, None, :])).astype(F)
        return (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]


def visited(pa, pb, radius, perm_a=None, perm_b=None):
    """(block pairs visited, block pairs in all) of one search"""
    if len(pa) == 0:
        return 0, 0
    loA, hiA = block_boxes(pa, perm_a)
    loB, hiB = block_boxes(pb, perm_b)
    with np.errstate(invalid="ignore"):
        skip = gap2(loA, hiA, loB, hiB) > r2f(radius)
    return int((~skip).sum()), int(skip.size)


def spatial_order(xyz, cell):
    """sift3d_amd_spatial_order: int32 permutation"""
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    n = len(p)
    fin = np.isfinite(p).all(axis=1)
    keys = [None] * n
    if fin.any():
        with np.errstate(invalid="ignore", over="ignore"):
            c = np.floor(p / float(cell))
        off = c - c[fin].min(axis=0)
        for i in np.nonzero(fin)[0]:
            key = 0
            for k in range(3):
                v = int(off[i, k]) if off[i, k] < 2097151.0 else 2097151
                for b in range(21):
                    key |= ((v >> b) & 1) << (3 * b + k)
            keys[i] = key
    order = sorted(range(n), key=lambda i: (keys[i] if keys[i] is not None else 1 << 64, i))
    return np.array(order, np.int32).reshape(n)


def match_guided(fwd, bwd, nn_thresh, max_distance=None):
    """sift3d_amd_matcher_match_guided over the gated searches of both directions"""
    out = mr.match(fwd, bwd, nn_thresh)
    if max_distance is not None and max_distance > 0:
        cap2 = F(float(max_distance) * float(max_distance))
        f1 = np.asarray(fwd[1], F)
        with np.errstate(invalid="ignore"):
            out = np.where(f1 <= cap2, out, -1).astype(np.int32)
    return out
