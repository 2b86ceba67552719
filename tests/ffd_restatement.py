"""numpy restatement of the free-form deformation contract (include/sift3d_amd.h, "B-spline free-form deformation").

The weight table is float64 in the header's order, rounded to float32; the spline value is float32 in the stated order
of its 64 terms; the field adds the affine part as tests/field_restatement.py states it; the sample and its gradient are
tests/affine_refine_restatement.py's arithmetic at q = p + u; the terms of the record are float64 and its sums
correctly rounded (math.fsum), so that a bound on the device's sum need not allow for the reference's own error; the
bending energy follows the header's stencils in float64; the subdivision is float32 in the stated order; the driver is
the header's loop with coarser levels from tests.multires_restatement.ref_restrict."""
import collections
import math

import numpy as np

from tests.field_restatement import ref_affine_field
from tests.multires_restatement import ref_restrict
from tests.test_warp import ref_inside

F32 = np.float32
Record = collections.namedtuple("Record", "n see Gc see_terms Gc_terms support")
Refinement = collections.namedtuple("Refinement", "lattice field trail stop")
STOPS = ("converged", "evaluations", "flat", "failed")


def spacing3(spacing):
    return (spacing,) * 3 if np.isscalar(spacing) else tuple(int(v) for v in spacing)


def lattice_dim(o, delta):
    return (o - 1) // delta + 4


def lattice_shape(out_shape, spacing):
    """[3, gz, gy, gx] for a grid (oz, oy, ox) and spacing (dx, dy, dz)"""
    oz, oy, ox = out_shape
    dx, dy, dz = spacing3(spacing)
    return (3, lattice_dim(oz, dz), lattice_dim(oy, dy), lattice_dim(ox, dx))


def weights(delta):
    """w [delta, 4] float32, the header's expressions in float64"""
    t = np.arange(delta, dtype=np.float64) / np.float64(delta)
    u = 1.0 - t
    t2 = t * t
    t3 = t2 * t
    w = np.stack([((u * u) * u) / 6.0, ((3.0 * t3 - 6.0 * t2) + 4.0) / 6.0,
                  (((-3.0 * t3 + 3.0 * t2) + 3.0 * t) + 1.0) / 6.0, t3 / 6.0], axis=1)
    return w.astype(F32)


def _axes(out_shape, spacing):
    """per axis (x, y, z): (i0 [o], w [o, 4] float32)"""
    oz, oy, ox = out_shape
    out = []
    for o, d in zip((ox, oy, oz), spacing3(spacing)):
        p = np.arange(o)
        out.append((p // d, weights(d)[p % d]))
    return out


def spline(lattice, spacing, out_shape):
    """s [3, oz, oy, ox] float32: the 64 terms in the header's order"""
    c = np.ascontiguousarray(lattice, F32)
    (ix, wx), (iy, wy), (iz, wz) = _axes(out_shape, spacing)
    oz, oy, ox = out_shape
    s = np.zeros((3, oz, oy, ox), F32)
    for cc in range(4):
        for b in range(4):
            for a in range(4):
                v = c[:, (iz + cc)[:, None, None], (iy + b)[None, :, None], (ix + a)[None, None, :]]
                t = wz[:, cc][:, None, None] * (wy[:, b][None, :, None] * (wx[:, a][None, None, :] * v))
                s = (s + t.astype(F32)).astype(F32)
    return s


def field(lattice, spacing, out_shape, A=None):
    s = spline(lattice, spacing, out_shape)
    if A is None:
        return s
    return (ref_affine_field(A, out_shape) + s).astype(F32)


def sample_grad(M, u):
    """(m, gx, gy, gz float32 [oz, oy, ox], inside) of M at q = p + u(p): warp_field's sample and gather_grad"""
    M = np.ascontiguousarray(M, F32)
    nz, ny, nx = M.shape
    _, oz, oy, ox = u.shape
    z, y, x = np.meshgrid(np.arange(oz), np.arange(oy), np.arange(ox), indexing="ij")
    q = [p.astype(np.float64) + ud.astype(np.float64) for p, ud in zip((x, y, z), u)]
    ins = ref_inside(q, M.shape)
    q = [np.where(ins, v, 0.0) for v in q]
    i = [np.floor(v) for v in q]
    f = [(v - iv).astype(F32) for v, iv in zip(q, i)]
    i = [iv.astype(np.int64) for iv in i]
    j = [np.minimum(iv + 1, n - 1) for iv, n in zip(i, (nx, ny, nz))]
    flat = M.reshape(-1)

    def g(ix, iy, iz):
        return flat[(iz * ny + iy) * nx + ix]

    def lerp(a, b, t):
        return (a + t * (b - a)).astype(F32)

    a00, b00 = g(i[0], i[1], i[2]), g(j[0], i[1], i[2])
    a10, b10 = g(i[0], j[1], i[2]), g(j[0], j[1], i[2])
    a01, b01 = g(i[0], i[1], j[2]), g(j[0], i[1], j[2])
    a11, b11 = g(i[0], j[1], j[2]), g(j[0], j[1], j[2])
    fx, fy, fz = f
    c00, c10, c01, c11 = lerp(a00, b00, fx), lerp(a10, b10, fx), lerp(a01, b01, fx), lerp(a11, b11, fx)
    c0, c1 = lerp(c00, c10, fy), lerp(c01, c11, fy)
    m = lerp(c0, c1, fz)
    gx = lerp(lerp(b00 - a00, b10 - a10, fy), lerp(b01 - a01, b11 - a11, fy), fz)
    gy = lerp(c10 - c00, c11 - c01, fz)
    gz = (c1 - c0).astype(F32)
    return m, gx, gy, gz, ins


def _fsum(a):
    return math.fsum(np.asarray(a, np.float64).reshape(-1).tolist())


def adjoint(v, spacing, exact=True):
    """(Phi^T v, sum |term|, support) for v float64 [oz, oy, ox]: out[k, j, i] = sum_p W(p; k, j, i) v(p) with
    W = ((double) wx * (double) wy) * (double) wz, [gz, gy, gx]; support counts the voxels under each control"""
    oz, oy, ox = v.shape
    _, gz, gy, gx = lattice_shape(v.shape, spacing)
    (ix, wx), (iy, wy), (iz, wz) = _axes(v.shape, spacing)
    idx, terms = [], []
    for cc in range(4):
        for b in range(4):
            for a in range(4):
                W = (wx[:, a].astype(np.float64)[None, None, :] * wy[:, b].astype(np.float64)[None, :, None]) * \
                    wz[:, cc].astype(np.float64)[:, None, None]
                k = (((iz + cc)[:, None, None] * gy + (iy + b)[None, :, None]) * gx + (ix + a)[None, None, :])
                idx.append(np.broadcast_to(k, v.shape).reshape(-1))
                terms.append((W * v).reshape(-1))
    idx, terms = np.concatenate(idx), np.concatenate(terms)
    m = gz * gy * gx
    tot = np.bincount(idx, np.abs(terms), m)
    sup = np.bincount(idx, minlength=m)
    if exact:
        order = np.argsort(idx, kind="stable")
        st, cuts = terms[order], np.cumsum(sup)[:-1]
        out = np.array([math.fsum(g.tolist()) for g in np.split(st, cuts)])
    else:
        out = np.bincount(idx, terms, m)
    return out.reshape(gz, gy, gx), tot.reshape(gz, gy, gx), sup.reshape(gz, gy, gx)


def evaluate(F, M, lattice, spacing, A=None, exact=True):
    """(Record, field): n, S_ee, Gc [3, gz, gy, gx] and sum |term| of each over the fixed voxels that sample inside M"""
    F = np.ascontiguousarray(F, F32)
    u = field(lattice, spacing, F.shape, A)
    m, gx, gy, gz, ins = sample_grad(M, u)
    E = np.where(ins, (m - F).astype(F32).astype(np.float64), 0.0)
    G = [np.where(ins, v.astype(np.float64), 0.0) for v in (gx, gy, gz)]
    fsum = _fsum if exact else (lambda a: float(np.sum(a)))
    parts = [adjoint(E * Gd, spacing, exact) for Gd in G]
    return Record(int(ins.sum()), fsum(E * E), np.stack([p[0] for p in parts]), float((E * E).sum()),
                  np.stack([p[1] for p in parts]), parts[0][2]), u


def stencils(delta):
    d = float(delta)
    return np.array([[1.0 / 6.0, 4.0 / 6.0, 1.0 / 6.0], [-0.5 / d, 0.0, 0.5 / d],
                     [1.0 / (d * d), -2.0 / (d * d), 1.0 / (d * d)]])


ORDERS = ((2, 0, 0), (0, 2, 0), (0, 0, 2), (1, 1, 0), (1, 0, 1), (0, 1, 1))      # (x, y, z) orders of xx .. yz
WEIGHTS = (1.0, 1.0, 1.0, 2.0, 2.0, 2.0)


def bending(lattice, spacing):
    """(R, dR [3, gz, gy, gx], sum |term| of R's sum, sum |term| of dR's): the header's stencils in float64"""
    c = np.asarray(lattice, F32).astype(np.float64)
    _, gz, gy, gx = c.shape
    sx, sy, sz = (stencils(d) for d in spacing3(spacing))
    N = (gx - 2) * (gy - 2) * (gz - 2)
    dR, dRt = np.zeros_like(c), np.zeros_like(c)
    terms = []

    def sl(n, o):
        return slice(o, n - 2 + o)

    for t, (ox_, oy_, oz_) in enumerate(ORDERS):
        D = np.zeros((3, gz - 2, gy - 2, gx - 2))
        for cc in range(3):
            ry = np.zeros_like(D)
            for b in range(3):
                rx = np.zeros_like(D)
                for a in range(3):
                    rx = rx + sx[ox_][a] * c[:, sl(gz, cc), sl(gy, b), sl(gx, a)]
                ry = ry + sy[oy_][b] * rx
            D = D + sz[oz_][cc] * ry
        terms.append(WEIGHTS[t] * (D * D))
        for cc in range(3):
            for b in range(3):
                for a in range(3):
                    coef = (sz[oz_][cc] * sy[oy_][b]) * sx[ox_][a]
                    v = WEIGHTS[t] * (coef * D)
                    dR[:, sl(gz, cc), sl(gy, b), sl(gx, a)] += v
                    dRt[:, sl(gz, cc), sl(gy, b), sl(gx, a)] += np.abs(v)
    terms = np.stack(terms)
    return _fsum(terms) / N, (2.0 / N) * dR, float(terms.sum()) / N, (2.0 / N) * dRt


def gradient(rec, dR, bend):
    """(grad float32, gmax)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        g = ((2.0 / np.float64(rec.n)) * rec.Gc + bend * dR).astype(F32)
    return g, float(np.abs(g).max())


def _sub_axis(c, ax, g_fine):
    c = np.moveaxis(c, ax, -1)
    out = np.zeros(c.shape[:-1] + (g_fine,), F32)
    for j in range(g_fine):
        if j & 1:
            i = (j + 1) // 2
            out[..., j] = ((c[..., i - 1] + F32(6.0) * c[..., i]) + c[..., i + 1]) * F32(0.125)
        else:
            i = j // 2
            out[..., j] = (c[..., i] + c[..., i + 1]) * F32(0.5)
    return np.moveaxis(out, -1, ax)


def refine2(coarse, out_shape, spacing):
    """the lattice over the grid out_shape from the lattice over ((o + 1) / 2): x, y, z in turn, then * 2, float32"""
    c = np.ascontiguousarray(coarse, F32)
    assert c.shape == lattice_shape(tuple((o + 1) // 2 for o in out_shape), spacing)
    shape = lattice_shape(out_shape, spacing)
    for ax in (3, 2, 1):
        c = _sub_axis(c, ax, shape[ax])
    return (c * F32(2.0)).astype(F32)


def cost(rec, R, bend):
    return (rec.see / rec.n if rec.n else float("nan")) + bend * R


def refine(F, M, A=None, spacing=8, levels=3, bending_weight=0.005, max_evaluations=60, step0=1.0, step_max=4.0,
           tol=0.01, min_overlap=0.5):
    """the header's driver; trail entries (E, msd, R, n, step, accepted, level)"""
    A = None if A is None else np.array(A, np.float64).reshape(3, 4)
    Fs, Ms = [np.ascontiguousarray(F, F32)], [np.ascontiguousarray(M, F32)]
    for _ in range(1, levels):
        Fs.append(ref_restrict(Fs[-1]))
        Ms.append(ref_restrict(Ms[-1]))
        if A is not None:
            A[:, 3] = A[:, 3] * 0.5
    trail, stop, c = [], 1, None

    def ev(Fl, Ml, lat):
        rec, _ = evaluate(Fl, Ml, lat, spacing, A, exact=False)
        R, dR, _, _ = bending(lat, spacing)
        g, gmax = gradient(rec, dR, bending_weight)
        return rec, R, g, gmax, cost(rec, R, bending_weight)

    def entry(rec, R, E, s, acc, l):
        return (E, rec.see / rec.n if rec.n else float("nan"), R, rec.n, s, acc, l)

    for l in range(levels - 1, -1, -1):
        Fl, Ml = Fs[l], Ms[l]
        c = np.zeros(lattice_shape(Fl.shape, spacing), F32) if c is None else refine2(c, Fl.shape, spacing)
        s = step0
        rec, R, g, gmax, E = ev(Fl, Ml, c)
        trail.append(entry(rec, R, E, s, True, l))
        n_first, evals = rec.n, 1
        if not np.isfinite(E):
            stop = 3
        else:
            while True:
                if evals >= max_evaluations:
                    stop = 1
                    break
                if gmax == 0.0:
                    stop = 2
                    break
                ct = (c - F32(s / gmax) * g).astype(F32)
                rt, Rt, gt, gmt, Et = ev(Fl, Ml, ct)
                evals += 1
                accept = bool(np.isfinite(Et) and rt.n >= min_overlap * n_first and Et < E)
                trail.append(entry(rt, Rt, Et, s, accept, l))
                if not np.isfinite(Et):
                    stop = 3
                    break
                if accept:
                    c, rec, R, g, gmax, E = ct, rt, Rt, gt, gmt, Et
                    s = min(2.0 * s, step_max)
                else:
                    s = s * 0.5
                if s < tol:
                    stop = 0
                    break
        if l > 0 and A is not None:
            A[:, 3] = A[:, 3] * 2.0
    return Refinement(c, field(c, spacing, Fs[0].shape, A), trail, STOPS[stop])
