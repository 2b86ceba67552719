"""numpy restatement of the dense descriptor contract (include/sift3d_amd.h, "Dense descriptors").

Steps 1, 2 and 4 are written out here in float32 / float64 numpy with the contract's expression
order; step 3 is the oracle's apply_Sep_FIR_filter (oracle.blur / oracle.fir_axis).  The face
table is the oracle's init_geometry (orc_mesh).
"""
import numpy as np

F = np.float32
EPS = F(1.1920928955078125e-06)    # bary_eps (sift.c:42)


def mesh(so):
    """(v, ids): cart2bary's vertices of each face (20 x 3 x 3) and the vertex id of each of them
    (20 x 3) -- the geometric ids, not init_geometry's idx[], which every face keeps unswapped while
    it swaps v[0] and v[1] (quirk Q1; the sparse descriptor's bins follow idx[])."""
    v, _ = so.Oracle().mesh()
    V = vertices(so)
    ids = np.array([[int(np.argmin(np.abs(V - v[f, j]).sum(1))) for j in range(3)] for f in range(20)], np.int32)
    assert all(np.array_equal(V[ids[f, j]], v[f, j]) for f in range(20) for j in range(3))
    return v, ids


def vertices(so):
    """Coordinates of vertex c (12 x 3): the one vertex common to the five faces that carry id c."""
    v, idx = so.Oracle().mesh()
    out = np.zeros((12, 3), np.float32)
    for c in range(12):
        faces = [f for f in range(20) if c in idx[f]]
        common = [p for p in v[faces[0]] if all(any(np.array_equal(p, q) for q in v[f]) for f in faces)]
        assert len(common) == 1, (c, common)
        out[c] = common[0]
    return out


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cart2bary(g, tri):
    """cart2bary (sift.c:268-297) of gradients g = (gx, gy, gz) (float32 arrays) against one face
    (3 x 3 float32 vertices); returns (ok, bx, by, bz) with the acceptance test of icos_hist_bin
    (sift.c:1277-1279) folded into ok."""
    v0, v1, v2 = [tuple(F(c) for c in row) for row in tri]
    e1 = tuple(F(v1[k] - v0[k]) for k in range(3))
    e2 = tuple(F(v2[k] - v0[k]) for k in range(3))
    p = _cross(g, e2)
    det = _dot(e1, p)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        di = F(1.0) / det
        t = tuple(F(v0[k] * F(-1.0)) for k in range(3))
        q = _cross(t, e1)
        by = di * _dot(t, p)
        bz = di * _dot(g, q)
        bx = F(1.0) - by - bz
        k = _dot(e2, q) * di
        ok = ~(np.abs(det) < EPS) & ~((bx < -EPS) | (by < -EPS) | (bz < -EPS) | (k < 0))
    return ok, bx, by, bz


def face_of(g, so_mesh):
    """icos_hist_bin (sift.c:1253-1290): index of the first accepted face (-1: none) and the
    barycentrics there; also the number of faces that accept each direction."""
    v, _ = so_mesh
    shape = np.shape(g[0])
    face = np.full(shape, -1, np.int32)
    bary = [np.zeros(shape, np.float32) for _ in range(3)]
    nacc = np.zeros(shape, np.int32)
    for f in range(20):
        ok, bx, by, bz = cart2bary(g, v[f])
        nacc += ok
        new = ok & (face < 0)
        face[new] = f
        for b, val in zip(bary, (bx, by, bz)):
            b[new] = val[new]
    return face, bary, nacc


def gradient(vol, units=(1, 1, 1)):
    """Step 1: IM_GET_GRAD_ISO with neighbours clamped into the volume."""
    vol = np.ascontiguousarray(vol, np.float32)
    out = []
    for ax, u in zip((2, 1, 0), units):         # x, y, z = numpy axes 2, 1, 0
        n = vol.shape[ax]
        hi = np.take(vol, np.minimum(np.arange(n) + 1, n - 1), axis=ax)
        lo = np.take(vol, np.maximum(np.arange(n) - 1, 0), axis=ax)
        g = F(0.5) * (hi - lo)
        out.append(g * (F(1.0) / F(u)))
    return tuple(out)


def dense_bin(vol, so_mesh, units=(1, 1, 1)):
    """Steps 1-2: [12, nz, ny, nx] float32."""
    g = gradient(vol, units)
    m2 = g[0] * g[0] + g[1] * g[1] + g[2] * g[2]
    live = ~(m2 < EPS)
    face, bary, _ = face_of(g, so_mesh)
    assert np.all(face[live] >= 0)
    mag = np.sqrt(m2)                            # correctly rounded, as IEEE float32 sqrt
    _, idx = so_mesh
    out = np.zeros((12,) + vol.shape, np.float32)
    for j in range(3):
        w = mag * bary[j]
        ch = idx[np.maximum(face, 0), j]
        for c in range(12):
            sel = live & (ch == c)
            out[c][sel] = w[sel]
    return out


def blur_channels(h, so, sigma, units=(1, 1, 1)):
    """Step 3: every channel through oracle.blur (x, y, z; unit 1.0)."""
    taps = so.gauss_taps(sigma)
    return np.stack([so.blur(h[c], taps, units, unit=1.0) for c in range(12)])


def normalize(h):
    """Step 4: normalize_desc without truncation, per voxel."""
    s = np.zeros(h.shape[1:], np.float64)
    for c in range(12):
        hc = h[c].astype(np.float64)
        s = s + hc * hc
    norm = np.sqrt(s) + np.finfo(np.float64).eps
    inv = (1.0 / norm).astype(np.float32)
    return h * inv


def dense_descriptors(vol, so, sigma, units=(1, 1, 1)):
    m = mesh(so)
    return normalize(blur_channels(dense_bin(vol, m, units), so, sigma, units))
