"""numpy restatement of "Discrete displacement search" (include/sift3d_amd.h), operation for operation: the cost
volume, the coupled selection, the block-field smoothing and expansion, and one level of the driver.  float64 where the
contract says double, float32 where it says float; every sum that the contract orders is added in that order, one term
at a time (numpy's own sums are pairwise and are not used for them)."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
MAX_RADIUS, MAX_CHANNELS, MAX_PASSES, MAX_THETAS = 6, 16, 16, 16
DEFAULT_THETAS = (0.00009, 0.0003, 0.0009, 0.003, 0.009, 0.03)


def gamma(n):
    """the bound n u / (1 - n u) of a double sum of n non-negative terms in any order, relative to the exact sum"""
    u = 2.0 ** -53
    return n * u / (1 - n * u)


def labels(R):
    """(dx, dy, dz, |d|^2) of every label k, int arrays of K = (2R + 1)^3"""
    D = 2 * R + 1
    k = np.arange(D ** 3)
    dx, dy, dz = k % D - R, (k // D) % D - R, k // (D * D) - R
    return dx, dy, dz, dx * dx + dy * dy + dz * dz


def _stack(a):
    a = np.asarray(a)
    assert a.dtype == F32 and a.ndim in (3, 4)
    return a if a.ndim == 4 else a[None]


def _windows(P, R, nb, z, y, x):
    """A[bz, by, bx, dz', dy', dx'] = P[4 bz + z + dz', 4 by + y + dy', 4 bx + x + dx'] for the volume P padded by R on
    every side: voxel (x, y, z) of every block under every label, label index order (dz, dy, dx)"""
    D = 2 * R + 1
    sz, sy, sx = P.strides
    return np.lib.stride_tricks.as_strided(P[z:, y:, x:], shape=nb + (D, D, D),
                                           strides=(4 * sz, 4 * sy, 4 * sx, sz, sy, sx), writeable=False)


def cost_volume(F, W, R, VF=None, VW=None):
    """cost float32 [nbz, nby, nbx, K]"""
    F, W = _stack(F), _stack(W)
    assert F.shape == W.shape and 1 <= R <= MAX_RADIUS and 1 <= F.shape[0] <= MAX_CHANNELS
    nc, nz, ny, nx = F.shape
    nb = (nz // 4, ny // 4, nx // 4)
    assert min(nb) >= 1
    K = (2 * R + 1) ** 3
    inside = np.ones((nz, ny, nx), bool) if VW is None else np.asarray(VW, F32) >= F32(0.5)
    inW = np.pad(inside, R, constant_values=False)
    inF = np.ones((nz, ny, nx), bool) if VF is None else np.asarray(VF, F32) >= F32(0.5)
    acc = np.zeros(nb + (2 * R + 1,) * 3, F64)
    label_ok = np.ones(acc.shape, bool)
    block_ok = np.ones(nb, bool)
    crop = (slice(0, 4 * nb[0], 4), slice(0, 4 * nb[1], 4), slice(0, 4 * nb[2], 4))
    for z in range(4):
        for y in range(4):
            for x in range(4):
                label_ok &= _windows(inW, R, nb, z, y, x)
                block_ok &= inF[z:, y:, x:][crop]
    for c in range(nc):
        Wp = np.pad(W[c], R)
        for z in range(4):
            for y in range(4):
                for x in range(4):
                    f = F[c][z:, y:, x:][crop].astype(F64)[..., None, None, None]
                    e = f - _windows(Wp, R, nb, z, y, x).astype(F64)
                    s = e * e
                    acc = acc + s
    with np.errstate(over="ignore"):
        cost = (acc / (64.0 * nc)).astype(F32)
    cost[~(label_ok & block_ok[..., None, None, None])] = np.inf
    return np.ascontiguousarray(cost.reshape(nb + (K,)))


def cost_select(cost, u, theta):
    """(v float32 [3, nb...], data float32 [nb...], (exactly rounded sum of data over the non-empty blocks, their
    count))"""
    cost = np.asarray(cost)
    u = np.asarray(u)
    assert cost.dtype == F32 and u.dtype == F32 and cost.ndim == 4 and u.shape == (3,) + cost.shape[:3]
    assert math.isfinite(theta) and theta >= 0
    K = cost.shape[3]
    R = (round(K ** (1 / 3)) - 1) // 2
    assert (2 * R + 1) ** 3 == K
    dx, dy, dz, d2 = labels(R)
    ex = dx.astype(F64) - u[0].astype(F64)[..., None]
    ey = dy.astype(F64) - u[1].astype(F64)[..., None]
    ez = dz.astype(F64) - u[2].astype(F64)[..., None]
    q = (ex * ex + ey * ey) + ez * ez
    val = cost.astype(F64) + F64(theta) * q
    lo = val.min(-1)
    cand = val == lo[..., None]
    d2c = np.where(cand, d2, np.iinfo(np.int64).max)
    cand &= d2c == d2c.min(-1)[..., None]
    k = cand.argmax(-1)                                       # the first True: the smallest k
    empty = lo == np.inf
    v = np.stack([dx[k], dy[k], dz[k]]).astype(F32)
    v[:, empty] = u[:, empty]
    data = np.take_along_axis(cost, k[..., None], -1)[..., 0].copy()
    data[empty] = np.inf
    return v, data, (math.fsum(data[~empty].astype(F64).ravel()), int((~empty).sum()))


def _binomial(a, axis):
    n = a.shape[axis]
    i = np.arange(n)
    lo, hi = np.take(a, np.maximum(i - 1, 0), axis), np.take(a, np.minimum(i + 1, n - 1), axis)
    return (F32(0.25) * lo + F32(0.5) * a) + F32(0.25) * hi


def smooth(a, passes):
    """the block field [3, nbz, nby, nbx] after `passes` passes of B_z B_y B_x"""
    a = np.asarray(a)
    assert a.dtype == F32 and a.ndim == 4 and a.shape[0] == 3 and 0 <= passes <= MAX_PASSES
    a = a.copy()
    for _ in range(passes):
        a = _binomial(_binomial(_binomial(a, 3), 2), 1)
        assert a.dtype == F32
    return a


def _lerp_axis(a, axis, n):
    nb = a.shape[axis]
    t = (np.arange(n).astype(F32) - F32(1.5)) * F32(0.25)
    t = np.minimum(np.maximum(t, F32(0)), F32(nb - 1))
    i0 = np.floor(t).astype(np.int64)
    i1 = np.minimum(i0 + 1, nb - 1)
    f = t - i0.astype(F32)
    shape = [1] * a.ndim
    shape[axis] = n
    f = f.reshape(shape)
    out = (F32(1) - f) * np.take(a, i0, axis) + f * np.take(a, i1, axis)
    assert out.dtype == F32
    return out


def expand(b, shape):
    """the voxel field [3, nz, ny, nx] of the block field b [3, nbz, nby, nbx], nb = n // 4"""
    b = np.asarray(b)
    nz, ny, nx = shape
    assert b.dtype == F32 and b.shape == (3, nz // 4, ny // 4, nx // 4)
    return np.ascontiguousarray(_lerp_axis(_lerp_axis(_lerp_axis(b, 3, nx), 2, ny), 1, nz))


def level(F, M, u, R, thetas, passes, VF, VM, warp, compose):
    """One level of the driver (steps 1 to 9 without the prolongation) from the start field u.  warp(src, u, interp)
    and compose(u, w) are the caller's: the device's own entries in the GPU tests, whose bits are pinned elsewhere.
    Returns (u_new, [the (sum, count) record of every theta], the intermediates W, V_W, C, b, w)."""
    F, M = _stack(F), _stack(M)
    W = np.stack([warp(m, u, "linear") for m in M])
    VW = warp(np.ones(M.shape[1:], F32) if VM is None else VM, u, "nearest")
    C = cost_volume(F, W, R, VF, VW)
    b = np.zeros((3,) + C.shape[:3], F32)
    records = []
    for theta in thetas:
        v, _, rec = cost_select(C, b, theta)
        records.append(rec)
        b = smooth(v, passes)
    w = expand(b, F.shape[1:])
    return compose(u, w), records, (W, VW, C, b, w)
