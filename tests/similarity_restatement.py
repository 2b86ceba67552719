"""numpy restatement of the similarity contract (include/sift3d_amd.h, "Similarity measures").

The sample is the warps' own: tests.test_warp.ref_warp (an affine pull map) and tests.field_restatement's
ref_field_points (a displacement field), which give the value and the inside test.  Binning is float32, unfused,
exactly as stated; the histogram is a bincount over b_f * B + b_m (exact integers); the moments are sums of products
formed in float64 from the float32 values (d = f - m a float32 subtraction first), each sum correctly rounded
(math.fsum), so that a bound on the device's sum need not allow for the reference's own error.  The measures follow the
header's order of operations."""
import collections
import math

import numpy as np

from tests import field_restatement as fr
from tests.test_warp import ref_warp

Stats = collections.namedtuple("Stats", "count sums terms")     # sums: float64 [6]; terms: sum |term| per sum
Measures = collections.namedtuple("Measures", "n msd ncc mi nmi entropy_fixed entropy_moving entropy_joint")
SUMS = ("f", "m", "ff", "mm", "fm", "dd")


def bin_scale(bins, lo, hi):
    """s = (float) B / (hi - lo), float32"""
    return np.float32(bins) / (np.float32(hi) - np.float32(lo))


def bin_of(v, bins, lo, hi):
    """t = (v - lo) * s; b = t < 0 ? 0 : t >= B ? B - 1 : (int) t, float32"""
    v = np.asarray(v, np.float32)
    t = (v - np.float32(lo)) * bin_scale(bins, lo, hi)
    with np.errstate(invalid="ignore"):
        mid = np.where((t >= 0) & (t < np.float32(bins)), t, np.float32(0)).astype(np.int64)
    return np.where(t < 0, 0, np.where(t >= np.float32(bins), bins - 1, mid))


def sample(M, transform, out_shape, interp="linear"):
    """(m float32 [oz, oy, ox], inside) of the moving volume through a 3 x 4 affine, a field [3, oz, oy, ox] or None"""
    M = np.ascontiguousarray(M, np.float32)
    if transform is None:
        assert tuple(M.shape) == tuple(out_shape)
        transform = np.eye(3, 4)
    T = np.asarray(transform)
    if T.ndim == 4:
        assert tuple(T.shape[1:]) == tuple(out_shape)
        flat = M.reshape(-1)
        x, y, z = fr.grid(out_shape)
        return fr.ref_field_points(lambda k: flat[k], M.shape, T.astype(np.float32), x, y, z, interp, 0.0)
    return ref_warp(M, T.reshape(3, 4), out_shape, interp, 0.0)


def joint(F, M, transform, bins, range_f, range_m, interp="linear"):
    """(hist uint64 [B, B] indexed [b_f, b_m], Stats) over the fixed voxels that sample inside M"""
    F = np.ascontiguousarray(F, np.float32)
    m, ins = sample(M, transform, F.shape, interp)
    f, m = F[ins], m.astype(np.float32)[ins]
    idx = bin_of(f, bins, *range_f) * bins + bin_of(m, bins, *range_m)
    hist = np.bincount(idx, minlength=bins * bins).astype(np.uint64).reshape(bins, bins)
    fd, md, dd = f.astype(np.float64), m.astype(np.float64), (f - m).astype(np.float64)
    terms = [fd, md, fd * fd, md * md, fd * md, dd * dd]
    return hist, Stats(int(f.size), np.array([math.fsum(t.tolist()) for t in terms]),
                       np.array([np.abs(t).sum() for t in terms]))


def entropy(counts, total):
    """acc = acc - p log p over the non-zero counts in order, p = (double) k / (double) total"""
    acc = 0.0
    t = float(total)
    for k in np.asarray(counts).reshape(-1).tolist():
        if k:
            p = float(k) / t
            acc = acc - p * float(np.log(p))
    return acc


def measures(hist, count, sums):
    """the header's measures from a histogram and a moments record, in its order of operations (float64)"""
    h = np.asarray(hist).astype(np.uint64)
    r, c = h.sum(axis=1, dtype=np.uint64), h.sum(axis=0, dtype=np.uint64)
    total = int(r.sum(dtype=np.uint64))
    n = int(count)
    if n == 0 or total == 0:
        return Measures(n, *([float("nan")] * 7))
    s = [float(v) for v in sums]
    nd = float(n)
    vf = s[2] - s[0] * s[0] / nd
    vm = s[3] - s[1] * s[1] / nd
    ncc = 0.0 if vf <= 0 or vm <= 0 else (s[4] - s[0] * s[1] / nd) / float(np.sqrt(vf * vm))
    hf, hm, hfm = entropy(r, total), entropy(c, total), entropy(h, total)
    return Measures(n, s[5] / nd, ncc, (hf + hm) - hfm, 0.0 if hfm == 0 else (hf + hm) / hfm, hf, hm, hfm)


def similarity(F, M, transform=None, bins=64, interp="linear", range_f=None, range_m=None):
    """api.similarity's restatement: own ranges (hi = lo + 1 for a constant volume) where none is given"""
    def own(v, given):
        if given is not None:
            return given
        lo, hi = float(np.min(v)), float(np.max(v))
        return (lo, hi) if hi > lo else (lo, lo + 1.0)
    hist, st = joint(F, M, transform, bins, own(F, range_f), own(M, range_m), interp)
    return measures(hist, st.count, st.sums), hist


def label_overlap(confusion):
    """(dice, jaccard, vol_f, vol_m) of a confusion matrix [L, L]: the integers exactly, one division each"""
    h = np.asarray(confusion).astype(np.uint64)
    r, c = h.sum(axis=1, dtype=np.uint64), h.sum(axis=0, dtype=np.uint64)
    L = h.shape[0]
    dice, jac = np.full(L, np.nan), np.full(L, np.nan)
    for k in range(L):
        hkk, both = int(h[k, k]), int(r[k]) + int(c[k])
        if both:
            dice[k] = float(2 * hkk) / float(both)
            jac[k] = float(hkk) / float(both - hkk)
    return dice, jac, r.astype(np.int64), c.astype(np.int64)
