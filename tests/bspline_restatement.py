"""numpy restatement of the cubic B-spline contract (include/sift3d_amd.h, "Cubic B-spline resampling"), in its exact
arithmetic: float32 products and sums, one rounding per operation, in the header's order.

Prefilter: per axis c[i] = acc after acc = +0; for k = H .. 1: acc = acc + h[k] * (s[m(i - k)] + s[m(i + k)]);
acc = acc + h[0] * s[i], on the whole-sample mirror extension m; axes x, y, z in turn; an axis of 1 is skipped.
Sample: inside test and coordinates as the linear warps'; taps i - 1 .. i + 2 mirrored; the four weights from
f = (float)(q - i); dot(w, a) = ((w0 a0 + w1 a1) + w2 a2) + w3 a3 along x, then y, then z."""
import numpy as np

from tests.test_warp import ref_coords, ref_inside

H = 16
F = np.float32
# SIFT3D_AMD_BSPLINE_TAPS: (float)(sqrt(3) * (sqrt(3) - 2)^k), k = 0 .. H
TAPS = np.array([float.fromhex(v) for v in (
    "0x1.bb67aep+0", "-0x1.db3d74p-2", "0x1.fd5c5ap-4", "-0x1.10f732p-5", "0x1.24904cp-7", "-0x1.39919cp-9",
    "0x1.5014fep-11", "-0x1.68362cp-13", "0x1.8212dap-15", "-0x1.9dcaep-17", "0x1.bb805ep-19", "-0x1.db57eap-21",
    "0x1.fd78b6p-23", "-0x1.110664p-24", "0x1.24a096p-26", "-0x1.39a31p-28", "0x1.5027b4p-30")], np.float32)
C6 = F(float.fromhex("0x1.555556p-3"))
C23 = F(float.fromhex("0x1.555556p-1"))


def mirror(j, n):
    """whole-sample mirror of integer array j into [0, n): period 2n - 2, reflecting as often as needed"""
    j = np.asarray(j, np.int64)
    if n == 1:
        return np.zeros_like(j)
    P = 2 * n - 2
    j = np.mod(j, P)                                    # mathematical modulus: in [0, P)
    return np.where(j >= n, P - j, j)


def prefilter_axis(s, axis):
    """one pass along `axis` of a float32 array; the lines are independent"""
    s = np.asarray(s, np.float32)
    n = s.shape[axis]
    if n == 1:
        return s.copy()
    i = np.arange(n)
    acc = np.zeros_like(s)
    for k in range(H, 0, -1):
        lo = np.take(s, mirror(i - k, n), axis=axis)
        hi = np.take(s, mirror(i + k, n), axis=axis)
        acc = acc + TAPS[k] * (lo + hi)
    out = acc + TAPS[0] * s
    assert out.dtype == np.float32
    return out


def prefilter(vol):
    """[nz, ny, nx] or [nc, nz, ny, nx] float32 -> coefficients: x, then y, then z"""
    c = np.asarray(vol, np.float32)
    for axis in (-1, -2, -3):
        c = prefilter_axis(c, c.ndim + axis)
    return c


def prefilter_line(vol, axis, fixed):
    """The coefficients along one line of a [nz, ny, nx] volume without filtering all of it: the line along `axis`
    (0 = z, 1 = y, 2 = x) through the voxel fixed = (z, y, x) (its `axis` entry is ignored).  On the other two axes
    only the mirrored window fixed - H .. fixed + H is kept and the pass is evaluated at its centre: the same
    expressions as prefilter(), for the voxels of the line."""
    sub = np.asarray(vol, np.float32)
    full = sub.shape
    for a in range(3):
        if a != axis and full[a] > 1:
            sub = np.take(sub, mirror(fixed[a] + np.arange(-H, H + 1), full[a]), axis=a)
    for a in (2, 1, 0):
        if a == axis:
            sub = prefilter_axis(sub, a)
        elif full[a] > 1:
            acc = np.zeros_like(np.take(sub, [H], axis=a))
            for k in range(H, 0, -1):
                acc = acc + TAPS[k] * (np.take(sub, [H - k], axis=a) + np.take(sub, [H + k], axis=a))
            sub = acc + TAPS[0] * np.take(sub, [H], axis=a)
    assert sub.dtype == np.float32
    return sub.reshape(-1)


def weights(f):
    """the four cubic B-spline weights of float32 fractions f, in the header's expressions"""
    f = np.asarray(f, np.float32)
    g = F(1.0) - f
    w0 = ((g * g) * g) * C6
    w1 = C23 - (F(0.5) * (f * f)) * (F(2.0) - f)
    w2 = C23 - (F(0.5) * (g * g)) * (F(2.0) - g)
    w3 = ((f * f) * f) * C6
    return [w0, w1, w2, w3]


def dot4(w, a):
    return ((w[0] * a[0] + w[1] * a[1]) + w[2] * a[2]) + w[3] * a[3]


def sample_points(gather, shape, q, fill=0.0):
    """The cubic sample at points q = (qx, qy, qz), float64 arrays.  gather(flat int64 indices) -> float32
    coefficients of a [nz, ny, nx] volume.  Returns (values float32, inside)."""
    nz, ny, nx = shape
    ins = ref_inside(q, shape)
    q = [np.where(ins, v, 0.0) for v in q]
    i = [np.floor(v) for v in q]
    w = [weights((v - iv).astype(np.float32)) for v, iv in zip(q, i)]
    i = [iv.astype(np.int64) for iv in i]
    tx = [mirror(i[0] - 1 + j, nx) for j in range(4)]
    ty = [mirror(i[1] - 1 + j, ny) for j in range(4)]
    tz = [mirror(i[2] - 1 + j, nz) for j in range(4)]
    sz = []
    for jz in range(4):
        r = []
        for jy in range(4):
            row = (tz[jz] * ny + ty[jy]) * nx
            r.append(dot4(w[0], [gather(row + tx[j]).astype(np.float32) for j in range(4)]))
        sz.append(dot4(w[1], r))
    val = dot4(w[2], sz)
    assert val.dtype == np.float32
    return np.where(ins, val, np.float32(fill)), ins


def _grid(out_shape):
    oz, oy, ox = out_shape
    z, y, x = np.meshgrid(np.arange(oz), np.arange(oy), np.arange(ox), indexing="ij")
    return x, y, z


def warp_affine(coef, A, out_shape, fill=0.0):
    """coef [nz, ny, nx] float32 coefficients -> [oz, oy, ox] through the pull map A"""
    coef = np.asarray(coef, np.float32)
    flat = np.ascontiguousarray(coef).reshape(-1)
    return sample_points(lambda k: flat[k], coef.shape, ref_coords(A, *_grid(out_shape)), fill)[0]


def field_coords(field, x, y, z):
    """q_d = (double) p_d + (double) u_d at output voxels (x, y, z) with u = (ux, uy, uz) float32 there"""
    return [np.asarray(p).astype(np.float64) + np.asarray(u, np.float32).astype(np.float64)
            for p, u in zip((x, y, z), field)]


def warp_field(coef, field, fill=0.0):
    """coef [nz, ny, nx] or [nc, nz, ny, nx] coefficients, field [3, oz, oy, ox] -> [(nc,) oz, oy, ox]"""
    coef = np.asarray(coef, np.float32)
    field = np.asarray(field, np.float32)
    q = field_coords(field, *_grid(field.shape[1:]))
    chans = coef[None] if coef.ndim == 3 else coef
    out = []
    for c in chans:
        flat = np.ascontiguousarray(c).reshape(-1)
        out.append(sample_points(lambda k: flat[k], c.shape, q, fill)[0])
    out = np.stack(out)
    return out[0] if coef.ndim == 3 else out
