"""numpy restatement of the multi-resolution demons contract (include/sift3d_amd.h, "Multi-resolution demons").

Restriction and prolongation are written out in float32 numpy in the header's order: per axis x, y, z in turn,
(0.25f a + 0.5f b) + 0.25f c on the clamped taps 2 i - 1, 2 i, 2 i + 1 and then the scale; 0.5f (a[i0] + a[i1]) with
i0 = p / 2, i1 = min(i0 + (p & 1), c - 1) and then the factor 2.  The weights are powers of two, so only the adds
round and numpy's float32 arithmetic is the kernels'.  The pyramid chains them with demons_restatement.ref_demons /
field_algebra_restatement.ref_demons_diffeo as the driver chains the transfers with sift3d_amd_demons_device_ex."""
import numpy as np

from tests import demons_restatement as dm

F32 = np.float32


def half_shape(shape):
    return tuple((int(n) + 1) // 2 for n in shape)


def _restrict_axis(a, ax):
    n = a.shape[ax]
    i = 2 * np.arange((n + 1) // 2)

    def tap(k):
        return np.take(a, np.clip(i + k, 0, n - 1), axis=ax)

    with np.errstate(invalid="ignore", over="ignore"):
        return ((F32(0.25) * tap(-1) + F32(0.5) * tap(0)) + F32(0.25) * tap(1)).astype(F32)


def ref_restrict(a, scale=1.0):
    """a [..., nz, ny, nx] float32 -> [..., cz, cy, cx]: the passes along x, y, z in turn, then * scale"""
    a = np.asarray(a, F32)
    for ax in (-1, -2, -3):
        a = _restrict_axis(a, ax)
    with np.errstate(invalid="ignore", over="ignore"):
        return (a * F32(scale)).astype(F32)


def _prolong_axis(a, ax, n):
    c = a.shape[ax]
    assert c == (n + 1) // 2
    p = np.arange(n)
    i0 = p // 2
    i1 = np.minimum(i0 + (p & 1), c - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        return (F32(0.5) * (np.take(a, i0, axis=ax) + np.take(a, i1, axis=ax))).astype(F32)


def ref_prolong(u, shape):
    """u [3, cz, cy, cx] float32 -> [3, nz, ny, nx], shape = (nz, ny, nx): the passes along x, y, z in turn, then
    * 2"""
    u = np.asarray(u, F32)
    for ax, n in zip((-1, -2, -3), tuple(shape)[::-1]):
        u = _prolong_axis(u, ax, n)
    with np.errstate(invalid="ignore", over="ignore"):
        return (F32(2.0) * u).astype(F32)


def ref_pyramid(v, levels):
    """[v, R(v), R(R(v)), ...]: `levels` entries"""
    out = [np.asarray(v, F32)]
    for _ in range(1, levels):
        out.append(ref_restrict(out[-1]))
    return out


def ref_multires(Fs, Ms, field, iterations, alpha, sigma_fluid, sigma_diffusion, so, update="additive", squarings=0):
    """(the finest field, [(s_d, inside) per iteration in the order run: the coarsest level's first]); Fs, Ms the
    per-level feature stacks (level 0 the finest), iterations one count per level"""
    levels = len(Fs)
    assert len(Ms) == levels and len(iterations) == levels
    us = [np.array(field, F32, copy=True)]
    for _ in range(1, levels):
        us.append(ref_restrict(us[-1], 0.5))
    per = []
    for l in range(levels - 1, -1, -1):
        if update == "additive":
            us[l], p = dm.ref_demons(Fs[l], Ms[l], us[l], iterations[l], alpha, sigma_fluid, sigma_diffusion, so)
        else:
            from tests import field_algebra_restatement as fa
            us[l], p = fa.ref_demons_diffeo(Fs[l], Ms[l], us[l], iterations[l], alpha, sigma_fluid, sigma_diffusion,
                                            squarings, so)
        per.extend(p)
        if l > 0:
            us[l - 1] = ref_prolong(us[l], us[l - 1].shape[1:])
    return us[0], per


def capture_case(so):
    """48^3 intensity volumes: M0 = Gaussian-blurred noise (sigma 1.5, peak 100), d = three noise volumes blurred with
    sigma 8 and scaled together to peak 12 voxels (drawn after M0); fixed = M0 pulled through d, moving = M0, so the
    true pull field fixed -> moving is d.  Returns (fixed, moving, d, demons keywords)."""
    from tests import field_restatement as fr
    n = 48
    rng = np.random.default_rng(2)
    M0 = so.blur(rng.normal(0, 1, (n, n, n)).astype(F32), so.gauss_taps(1.5), (1, 1, 1), unit=1.0).astype(F32)
    M0 = (M0 / np.abs(M0).max() * 100).astype(F32)
    d = np.stack([so.blur(rng.normal(0, 1, (n, n, n)).astype(F32), so.gauss_taps(8.0), (1, 1, 1), unit=1.0)
                  for _ in range(3)])
    d = (d / np.abs(d).max() * 12.0).astype(F32)
    fixed = fr.ref_warp_field(M0, d, "linear", 0.0)
    return fixed, M0, d, dict(alpha=1.0, sigma_fluid=1.0, sigma_diffusion=1.0)


def capture_error(u, d, lo=6, hi=42):
    """(median, p90) of |u - d| over [lo, hi)^3"""
    e = np.sqrt(((np.asarray(u, np.float64) - np.asarray(d, np.float64)) ** 2).sum(0))[lo:hi, lo:hi, lo:hi]
    return float(np.median(e)), float(np.percentile(e, 90))


def last_msd(per):
    sd, ins = per[-1]
    s, c = dm.ref_stats(sd, ins)
    return s / c
