"""numpy restatement of the block-matching contract (include/sift3d_amd.h, "Block matching").

The matcher: the 64 terms of every sum are added one at a time in the contract's order i = x + 4 y + 16 z, vectorised
over blocks and candidates only, in float64 from the float32 voxels (every product of two floats is exact there, so
numpy's unfused arithmetic is the contract's).  Validity is restated as such: a candidate is valid when every voxel of
the shifted block is on the grid and in V_W and vW > sWW 2^-40.  The choice is a lexsort on (-cc, |d|^2, k).  The
sub-voxel step can be switched off (subvoxel=False) to show why it is there.

The trimmed fit: Kabsch by numpy's SVD (rigid), lstsq (affine), the difference of centroids (translation), on the
scaled points; the LTS loop with a stable argsort, so ties go to the lower index.  It differs from the C fit (Horn's
quaternion, normal equations) by rounding only.

The driver: warp_affine and restrict2 are the existing restatements (tests.test_warp.ref_warp,
tests.multires_restatement.ref_restrict)."""
import collections
import math

import numpy as np

from tests.multires_restatement import ref_restrict
from tests.test_warp import ref_warp

NMIN = {"translation": 1, "rigid": 3, "affine": 4}
TAU = 2.0 ** -40
Iteration = collections.namedtuple(
    "Iteration", "level A_in A_out n_valid n_selected n_used selected used mean_cc rms move failed")


def _in(mask, shape):
    return np.ones(shape, bool) if mask is None else np.asarray(mask, np.float32) >= np.float32(0.5)


def block_match(F, W, radius, VF=None, VW=None, subvoxel=True, chunk=512):
    """(disp float32 [3, nbz, nby, nbx], cc float32 [nbz, nby, nbx], var float64 [nbz, nby, nbx])"""
    F = np.ascontiguousarray(F, np.float32)
    W = np.ascontiguousarray(W, np.float32)
    R = int(radius)
    D = 2 * R + 1
    nz, ny, nx = F.shape
    nbz, nby, nbx = nz // 4, ny // 4, nx // 4
    assert min(nbz, nby, nbx) > 0
    nb = nbz * nby * nbx
    inF, inW = _in(VF, F.shape), _in(VW, F.shape)
    Wp = np.zeros((nz + 2 * R, ny + 2 * R, nx + 2 * R), np.float32)
    Ip = np.zeros(Wp.shape, bool)
    Wp[R:R + nz, R:R + ny, R:R + nx] = W
    Ip[R:R + nz, R:R + ny, R:R + nx] = inW
    k = np.arange(D ** 3)
    dx, dy, dz = k % D - R, k // D % D - R, k // (D * D) - R
    d2 = dx * dx + dy * dy + dz * dz
    disp = np.zeros((3, nb), np.float32)
    cc_out = np.full(nb, -1.0, np.float32)
    var = np.zeros(nb, np.float64)
    for lo in range(0, nb, chunk):
        b = np.arange(lo, min(lo + chunk, nb))
        bx, by, bz = b % nbx, b // nbx % nby, b // (nbx * nby)
        sF = np.zeros(b.size)
        sFF = np.zeros(b.size)
        sW = np.zeros((k.size, b.size))
        sWW = np.zeros_like(sW)
        sFW = np.zeros_like(sW)
        okF = np.ones(b.size, bool)
        okW = np.ones(sW.shape, bool)
        with np.errstate(all="ignore"):
            for i in range(64):
                x, y, z = i & 3, (i >> 2) & 3, i >> 4
                f = F[4 * bz + z, 4 * by + y, 4 * bx + x].astype(np.float64)
                okF &= inF[4 * bz + z, 4 * by + y, 4 * bx + x]
                sF = sF + f
                sFF = sFF + f * f
                iz = (4 * bz + z + R)[None, :] + dz[:, None]
                iy = (4 * by + y + R)[None, :] + dy[:, None]
                ix = (4 * bx + x + R)[None, :] + dx[:, None]
                w = Wp[iz, iy, ix].astype(np.float64)
                okW &= Ip[iz, iy, ix]
                sW = sW + w
                sWW = sWW + w * w
                sFW = sFW + f[None, :] * w
            vF = sFF - (sF * sF) / 64.0
            vW = sWW - (sW * sW) / 64.0
            c = sFW - (sF[None, :] * sW) / 64.0
            cc = (c * c) / (vF[None, :] * vW)
        okF &= vF > sFF * TAU
        okW &= vW > sWW * TAU
        key = np.where(okW, cc, -np.inf)
        order = np.lexsort((np.broadcast_to(k[:, None], key.shape), np.broadcast_to(d2[:, None], key.shape), -key),
                           axis=0)
        win = order[0]
        cols = np.arange(b.size)
        valid = okF & okW[win, cols]
        c0 = cc[win, cols]
        d = np.stack([dx[win], dy[win], dz[win]]).astype(np.float64)
        for a, stride in enumerate((1, D, D * D)):
            if not subvoxel:
                break
            inside = (d[a] > -R) & (d[a] < R)
            km, kp = np.where(inside, win - stride, win), np.where(inside, win + stride, win)
            cm, cp = cc[km, cols], cc[kp, cols]
            with np.errstate(all="ignore"):
                den = (cm - 2.0 * c0) + cp
                o = np.clip(0.5 * (cm - cp) / den, -0.5, 0.5)
            use = inside & okW[km, cols] & okW[kp, cols] & (den < 0)
            d[a] = d[a] + np.where(use, o, 0.0)
        disp[:, b] = np.where(valid, d, 0.0).astype(np.float32)
        cc_out[b] = np.where(valid, c0, -1.0).astype(np.float32)
        var[b] = np.where(valid, vF, 0.0)
    shape = (nbz, nby, nbx)
    return disp.reshape((3,) + shape), cc_out.reshape(shape), var.reshape(shape)


def subvoxel_offset(cm, c0, cp):
    """the contract's offset from three valid scores along one axis"""
    den = (cm - 2.0 * c0) + cp
    return float(np.clip(0.5 * (cm - cp) / den, -0.5, 0.5)) if den < 0 else 0.0


# ---- the trimmed fit -------------------------------------------------------------------------------------------------
def fit(x, y, model):
    """(L, t) of y ~ L x + t, or None for a degenerate set (the contract's test on the scatter's eigenvalues)"""
    cx, cy = x.mean(0), y.mean(0)
    xc, yc = x - cx, y - cy
    if model == "translation":
        L = np.eye(3)
    else:
        for pts, need in ((xc, 2 if model == "rigid" else 3),) + (((yc, 2),) if model == "rigid" else ()):
            lam = np.sort(np.linalg.eigvalsh(pts.T @ pts))[::-1]
            if not lam[0] > 0 or not lam[need - 1] > 1e-10 * lam[0]:
                return None
        if model == "rigid":
            U, _, Vt = np.linalg.svd(yc.T @ xc)
            L = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt
        else:
            L = np.linalg.lstsq(xc, yc, rcond=None)[0].T
    return L, cy - L @ cx


def fit_trimmed(src, dst, model="rigid", keep=0.5, max_iter=20, scale_src=None, scale_dst=None):
    """(T [3, 4], used bool [n], refits) or None where the contract refuses"""
    src, dst = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(dst, np.float64).reshape(-1, 3)
    ss = np.ones(3) if scale_src is None else np.asarray(scale_src, np.float64)
    sd = np.ones(3) if scale_dst is None else np.asarray(scale_dst, np.float64)
    n = len(src)
    if n < NMIN[model] or not 0 < keep <= 1 or not (np.isfinite(src).all() and np.isfinite(dst).all()):
        return None
    x, y = src * ss, dst * sd
    k = min(max(math.ceil(keep * n), NMIN[model]), n)
    cur = np.ones(n, bool)
    got = fit(x, y, model)
    refits = 0
    while got is not None:
        L, t = got
        r = ((x @ L.T + t - y) ** 2).sum(1)
        nxt = np.zeros(n, bool)
        nxt[np.argsort(r, kind="stable")[:k]] = True
        if (nxt == cur).all() or refits >= max_iter:
            break
        cur = nxt
        got = fit(x[cur], y[cur], model)
        refits += 1
    if got is None:
        return None
    return np.concatenate([L * ss[None, :] / sd[:, None], (t / sd)[:, None]], 1), cur, refits


# ---- the driver ------------------------------------------------------------------------------------------------------
def apply(A, p):
    """A p in warp_affine's order of operations, p [n, 3]"""
    A = np.asarray(A, np.float64).reshape(3, 4)
    return np.stack([A[d, 0] * p[:, 0] + ((A[d, 1] * p[:, 1] + A[d, 2] * p[:, 2]) + A[d, 3]) for d in range(3)], 1)


def corner_move(A, B, shape):
    oz, oy, ox = shape
    c = np.array([[x, y, z] for z in (0, oz - 1) for y in (0, oy - 1) for x in (0, ox - 1)], np.float64)
    return float(np.sqrt(((apply(B, c) - apply(A, c)) ** 2).sum(1)).max())


def iteration(F, M, A, level=0, model="rigid", radius=3, keep_blocks=0.5, keep_inliers=0.5, WF=None, WM=None,
              spacing_fixed=None, spacing_moving=None, subvoxel=True):
    """one iteration of the driver on one level's volumes, from the pull map A"""
    F, M = np.asarray(F, np.float32), np.asarray(M, np.float32)
    A = np.asarray(A, np.float64).reshape(3, 4)
    W = ref_warp(M, A, F.shape, "linear", 0.0)[0].astype(np.float32)
    ones = np.ones(M.shape, np.float32) if WM is None else np.asarray(WM, np.float32)
    VW = ref_warp(ones, A, F.shape, "nearest", 0.0)[0].astype(np.float32)
    disp, cc, var = block_match(F, W, radius, WF, VW, subvoxel)
    nbz, nby, nbx = cc.shape
    cc, var, disp = cc.reshape(-1), var.reshape(-1), disp.reshape(3, -1)
    valid = np.nonzero(cc >= 0)[0]
    nan = float("nan")
    failed = Iteration(level, A, A, valid.size, 0, 0, None, None, nan, nan, nan, True)
    if valid.size < NMIN[model]:
        return failed
    nsel = min(math.ceil(keep_blocks * valid.size), valid.size)
    sel = np.sort(valid[np.argsort(-var[valid], kind="stable")[:nsel]])
    failed = failed._replace(n_selected=nsel, selected=sel)
    src = np.stack([4.0 * (sel % nbx) + 1.5, 4.0 * (sel // nbx % nby) + 1.5, 4.0 * (sel // (nbx * nby)) + 1.5], 1)
    dst = apply(A, src + disp[:, sel].T.astype(np.float64))
    got = fit_trimmed(src, dst, model, keep_inliers, 20, spacing_fixed, spacing_moving)
    if got is None:
        return failed
    T, used, _ = got
    sd = np.ones(3) if spacing_moving is None else np.asarray(spacing_moving, np.float64)
    r = (((apply(T, src) - dst) * sd) ** 2).sum(1)[used]
    return Iteration(level, A, T, valid.size, nsel, int(used.sum()), sel, used,
                     float(cc[sel][used].astype(np.float64).mean()), float(np.sqrt(r.mean())),
                     corner_move(A, T, F.shape), False)


def pyramid(v, levels):
    out = [None if v is None else np.asarray(v, np.float32)]
    for _ in range(1, levels):
        out.append(None if v is None else ref_restrict(out[-1], 1.0))
    return out


def register(F, M, A=None, model="rigid", levels=3, iterations=5, radius=3, keep_blocks=0.5, keep_inliers=0.5,
             tol=0.01, WF=None, WM=None, spacing_fixed=None, spacing_moving=None, subvoxel=True):
    """(A, trail, stop of level 0)"""
    Fs, Ms, WFs, WMs = (pyramid(v, levels) for v in (F, M, WF, WM))
    A = np.eye(3, 4) if A is None else np.array(A, np.float64).reshape(3, 4)
    A[:, 3] *= 0.5 ** (levels - 1)
    trail = []
    stop = "iterations"
    for l in range(levels - 1, -1, -1):
        stop = "iterations"
        for _ in range(iterations):
            e = iteration(Fs[l], Ms[l], A, l, model, radius, keep_blocks, keep_inliers, WFs[l], WMs[l], spacing_fixed,
                          spacing_moving, subvoxel)
            trail.append(e)
            if e.failed:
                stop = "failed"
                break
            A = e.A_out.copy()
            if e.move < tol:
                stop = "converged"
                break
        if l > 0:
            A[:, 3] *= 2.0
    return A, trail, stop
