"""numpy restatement of the MIND-SSC contract (include/sift3d_amd.h, "MIND self-similarity descriptors").

float64 numpy, word for word after the header: the six clamped shifts, the twelve squared differences in double, box()
in the order of tests/lncc_restatement.py ("Window sums"), S ascending, V = S / 12, the clamp, Dmin, t_k and cexp with
the header's coefficients.  Nothing here imports the library under test."""
import numpy as np

from tests import ffd_channels_restatement as fc
from tests.lncc_restatement import box, gamma  # noqa: F401  (gamma: for the tests)

F32 = np.float32
F64 = np.float64
CHANNELS = 12
MAX_RADIUS = 2
MAX_DILATION = 4
# (i, j) per channel; the neighbours n0 .. n5 are +x, -x, +y, -y, +z, -z times the dilation
PAIRS = ((0, 2), (0, 3), (0, 4), (0, 5), (1, 2), (1, 3), (1, 4), (1, 5), (2, 4), (2, 5), (3, 4), (3, 5))
LOG2E = float.fromhex("0x1.71547652b82fep+0")
COEF = tuple(float.fromhex(h) for h in (
    "0x1.0000000000000p+0", "-0x1.62e42fefa39efp-1", "0x1.ebfbdff82c58fp-3", "-0x1.c6b08d704a0c0p-5",
    "0x1.3b2ab6fba4e77p-7", "-0x1.5d87fe78a6731p-10", "0x1.430912f86c787p-13", "-0x1.ffcbfc588b0c7p-17",
    "0x1.62c0223a5c824p-20", "-0x1.b5253d395e7c4p-24", "0x1.e4cf5158b8ecap-28"))
CUTOFF = 104.0


def cexp(t):
    """the contract's exponential of -t, float64 in and out, one multiply and one add per Horner step"""
    t = np.asarray(t, F64)
    zero = t >= CUTOFF
    y = np.where(zero, 0.0, t) * LOG2E
    n = np.floor(y)
    f = y - n
    p = np.full_like(f, COEF[10])
    for c in COEF[9::-1]:
        p = p * f
        p = p + c
    r = p * np.ldexp(1.0, -n.astype(np.int64))
    return np.where(zero, 0.0, r)


def shifts(I, d):
    """s_i(q) = I(clamp(q + n_i)): six float64 volumes"""
    I = np.asarray(I, F32).astype(F64)
    out = []
    for ax in (2, 1, 0):                                     # x, y, z
        n = I.shape[ax]
        for sgn in (1, -1):
            idx = np.clip(np.arange(n) + sgn * d, 0, n - 1)
            out.append(np.take(I, idx, axis=ax))
    return out


def distances(I, r, d):
    """D [12, nz, ny, nx] float64"""
    s = shifts(I, d)
    D = []
    for i, j in PAIRS:
        e = s[i] - s[j]
        D.append(box(e * e, r))
    return np.stack(D)


def variance(D):
    """the unclamped V: S ascending from +0.0, then / 12.0"""
    S = np.zeros_like(D[0])
    for k in range(CHANNELS):
        S = S + D[k]
    return S / 12.0


def descriptor(D, V, vlo=0.0, vhi=np.inf):
    """out [12, nz, ny, nx] float32 from the distances and the unclamped V"""
    Vc = np.minimum(np.maximum(V, vlo), vhi)
    Dmin = D[0]
    for k in range(1, CHANNELS):
        Dmin = np.minimum(Dmin, D[k])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = np.where(Vc == 0.0, 0.0, (D - Dmin) / Vc)
    return cexp(t).astype(F32)


def ref_mind(I, r=1, d=2, vlo=0.0, vhi=np.inf):
    """(out float32 [12, ...], D float64 [12, ...], V float64 [...], sum of V, voxel count)"""
    D = distances(I, r, d)
    V = variance(D)
    return descriptor(D, V, vlo, vhi), D, V, float(np.sum(V, dtype=F64)), int(V.size)


def mind_ssc(I, r=1, d=2, floor=1e-3, ceiling=1e3, mean=None):
    """api.mind_ssc: the clamps are floor and ceiling times the mean of V (`mean`: the caller's, for a comparison
    that must not depend on the order of that one sum; None: numpy's)"""
    D = distances(I, r, d)
    V = variance(D)
    if floor is None and ceiling is None:
        return descriptor(D, V)
    if mean is None:
        mean = float(np.sum(V, dtype=F64)) / V.size
    return descriptor(D, V, 0.0 if floor is None else floor * mean, np.inf if ceiling is None else ceiling * mean)


def mind_levels(v, levels, **kw):
    """the MIND stacks of a volume per level: mind_ssc of every level's restricted volume"""
    return [mind_ssc(a, **kw) for a in fc.pyramid(np.asarray(v, F32), levels)]
