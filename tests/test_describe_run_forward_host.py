"""CPU: the keypoint list and the volumes of tests/test_describe_run_forward.py, and the runs of repeated bins
in them (the round mask of register forwarding, restated in numpy).

The fast kernel commits a batch of 64 window voxels in two passes of 16 rounds; round u of pass p adds voxel
32 p + u (half-wave 0) and voxel 32 p + 16 + u (half-wave 1).  A voxel REPEATS when its three bin addresses --
equivalently its face and its (clamped) base cell -- are those of its predecessor in its half-wave's sequence:
voxel v - 1, voxel 15 for voxel 32, voxel 31 for voxel 48; voxels 0 and 16 never repeat.  Bit 16 p + u of the
round mask m is set when both voxels of the round repeat: every commit lane then addresses the bin it addressed
the round before.  Forwarding the bin in a register through such rounds (no carry across batches) was built,
measured and not kept; the restatement stays as the description of what the pinned rows cover --
a commit that treats repeated bins specially meets every kind of run here -- and as the place where the share of
such rounds is counted.

`round_masks` restates the mask per work item (one of the DPARTS = 4 ranges of a window's planes), in float32
with the kernel's expressions: the window test and the split as `work_items` of
tests/test_describe_quad_commit.py restates them (the voxel counts are held to it below), the gradient, the face
(octant guess, the 20-face scan where a live voxel's guess is not accepted by margin), the stale lanes of a last
batch (a lane beyond the count keeps the voxel it held one batch before, the window box's first voxel if there
was none).

Three 40^3 volumes: a linear ramp (one face everywhere, bins change at cell borders only: long runs), the
lattice of the other describe tests, uniform noise (blurred by the pyramid; it repeats least).  The Gaussian
weight is numpy's exp here and a table of expf on the device, which could move a face decision only for a
direction within an ulp of an icosahedron edge.
"""
import numpy as np
import pytest

from tests.test_describe_quad_commit import work_items

F = np.float32
N, SEED = 40, 11
EPS = F(1.1920928955078125e-06)
I3 = np.eye(3, dtype=F)
X_ONLY = np.diag([1.0, 0.0, 0.0]).astype(F)   # the rotated gradient = (gx, 0, 0): on an icosahedron edge


def rotation(axis, deg):
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return (np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K).astype(F)


OBLIQUE = rotation((1.0, 2.0, 3.0), 25.0)      # window rows cross the cell borders obliquely

# (what, s, centre, sd or None = the level's own, R); the six sizes are those tests/test_describe_quad_commit.py
# found for the fast kernel's parts (R = I: work_items depends on the window alone, not on the volume)
ROWS = [
    ("axis wide", 2, (20.0, 19.0, 21.0), None, I3),           # level 2, every part holds full batches
    ("oblique", 1, (20.0, 20.0, 20.0), None, OBLIQUE),
    ("oblique subvoxel", 0, (19.25, 20.5, 20.75), None, OBLIQUE),
    ("edge", 0, (20.0, 20.0, 20.0), None, X_ONLY),            # the 20-face fallback
    ("corner", 0, (0.0, 0.0, 0.0), 0.25, I3),                 # clipped box, empty parts
    ("corner wide", 0, (39.0, 39.0, 39.0), None, OBLIQUE),
    ("tail", 0, (20.0, 20.0, 20.0), 0.525, I3),               # parts 323, 363, 242, 323: a last batch of 3
    ("b32", 0, (20.25, 20.0, 20.0), 0.3675, I3),              # parts 96, 98, 49, 96: a last batch of 32
    ("b33", 0, (20.25, 20.0, 20.0), 0.5725, I3),              # parts 353, ...: a last batch of 33
]
VOLUMES = ("ramp", "lattice", "noise")


def volume(name, oracle_mod):
    if name == "ramp":
        z, y, x = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
        return (F(0.011) * x.astype(F) + F(0.007) * y.astype(F) + F(0.017) * z.astype(F)).astype(F)
    if name == "lattice":
        return oracle_mod.synth_lattice(N, seed=SEED)
    return np.random.Generator(np.random.PCG64(2024)).random((N, N, N), dtype=F)


def keypoints(oracle, dtype):
    """([what], records) of ROWS; `oracle` holds the pyramid of the volume (sd of its levels)."""
    out = np.zeros(len(ROWS), dtype)
    for k, (_, s, c, sd, R) in zip(out, ROWS):
        k["o"], k["s"], k["R"] = 0, s, R
        k["sd"] = oracle.level(0, 0, s)[2] if sd is None else sd
        k["xd"], k["yd"], k["zd"] = c
    return [r[0] for r in ROWS], out


# ---- the icosahedron as the library builds it (upload_mesh, sift3d_hip_set_mesh) ----
def face_table():
    g = F((1.0 + np.sqrt(5.0)) / 2.0)
    o, z = F(1), F(0)
    vert = np.array([[z, o, g], [z, -o, g], [z, o, -g], [z, -o, -g], [o, g, z], [-o, g, z], [o, -g, z], [-o, -g, z],
                     [g, z, o], [-g, z, o], [g, z, -o], [-g, z, -o]], F)
    faces = [(0, 1, 8), (0, 8, 4), (0, 4, 5), (0, 5, 9), (0, 9, 1), (1, 6, 8), (8, 6, 10), (8, 10, 4), (4, 10, 2),
             (4, 2, 5), (5, 2, 11), (5, 11, 9), (9, 11, 7), (9, 7, 1), (1, 7, 6), (3, 6, 7), (3, 7, 11), (3, 11, 2),
             (3, 2, 10), (3, 10, 6)]
    tab = np.zeros((20, 13), F)       # e1, e2, t, q, e2.q
    for i, f in enumerate(faces):
        v = vert[list(f)].copy()
        for j in range(3):
            mag = np.sqrt(v[j, 0] * v[j, 0] + v[j, 1] * v[j, 1] + v[j, 2] * v[j, 2])
            v[j] = v[j] * F(1.0) / mag
        a, b = v[2] - v[1], v[1] - v[0]
        n = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)
        if n[0] * v[0, 0] + n[1] * v[0, 1] + n[2] * v[0, 2] < 0:
            v[[0, 1]] = v[[1, 0]]
        e1, e2, t = v[1] - v[0], v[2] - v[0], v[0] * F(-1.0)
        q = np.array([t[1] * e1[2] - t[2] * e1[1], t[2] * e1[0] - t[0] * e1[2], t[0] * e1[1] - t[1] * e1[0]], F)
        tab[i] = np.concatenate([e1, e2, t, q, [e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2]]])
    return tab


def face_eval(tab, rx, ry, rz):
    """cart2bary + the acceptance test for every face: (pass, min barycentric), shape (20, n)."""
    with np.errstate(all="ignore"):
        T = tab[:, :, None]
        e1, e2, t, q, e2q = T[:, 0:3], T[:, 3:6], T[:, 6:9], T[:, 9:12], T[:, 12]
        px = ry * e2[:, 2] - rz * e2[:, 1]
        py = rz * e2[:, 0] - rx * e2[:, 2]
        pz = rx * e2[:, 1] - ry * e2[:, 0]
        det = e1[:, 0] * px + e1[:, 1] * py + e1[:, 2] * pz
        di = F(1.0) / det
        yb = di * (t[:, 0] * px + t[:, 1] * py + t[:, 2] * pz)
        zb = di * (rx * q[:, 0] + ry * q[:, 1] + rz * q[:, 2])
        xb = F(1.0) - yb - zb
        kk = e2q * di
        ok = ~(np.abs(det) < EPS) & ~((xb < -EPS) | (yb < -EPS) | (zb < -EPS) | (kk < 0))
        return ok, np.minimum(xb, np.minimum(yb, zb))


def octant_table(tab):
    g = F(1.6180339887)
    rep = np.array([[1.0, 1.0, 1.0], [g / F(3), 0.05, (F(2) * g + F(1)) / F(3)],
                    [(F(2) * g + F(1)) / F(3), g / F(3), 0.05], [0.05, (F(2) * g + F(1)) / F(3), g / F(3)]], F)
    oct_ = np.zeros(32, int)
    for c in range(4):
        for o in range(8):
            r = rep[c] * np.array([-1 if o & 1 else 1, -1 if o & 2 else 1, -1 if o & 4 else 1], F)
            ok, _ = face_eval(tab, r[0:1], r[1:2], r[2:3])
            oct_[c * 8 + o] = int(np.argmax(ok[:, 0]))
    return oct_


def faces_of(tab, oct_, rx, ry, rz, live):
    """The face whose bin offsets a lane carries: the guess where it is accepted by margin or the lane is not
    live, else the first face in table order that passes."""
    g, g2 = F(1.6180339887), F(2.6180339887)
    ax, ay, az = np.abs(rx), np.abs(ry), np.abs(rz)
    n1 = (ax + g2 * ay - g * az) < 0
    n2 = (ay + g2 * az - g * ax) < 0
    n3 = (az + g2 * ax - g * ay) < 0
    cls = np.where(n1, 1, np.where(n2, 2, np.where(n3, 3, 0)))
    guess = oct_[cls * 8 + (rx < 0) + 2 * (ry < 0) + 4 * (rz < 0)]
    ok, mn = face_eval(tab, rx, ry, rz)
    idx = np.arange(len(rx))
    found = ok[guess, idx] & (mn[guess, idx] > F(2e-5))
    scan = np.argmax(ok, axis=0)
    use_scan = live & ~found & ok.any(axis=0)
    return np.where(use_scan, scan, guess)


def voxel_keys(G, k, tab, oct_):
    """Per work item (part) of keypoint k on level image G: the (face, base cell) key of its window voxels in
    scan order, and the key of the window box's first voxel (what a lane holds before its first voxel)."""
    n = G.shape[0]
    R = np.asarray(k["R"], F).reshape(9)
    cx, cy, cz = F(k["xd"]), F(k["yd"]), F(k["zd"])
    sigma = F(k["sd"] * 7.071067812)
    rad = F(2.0 * float(sigma))
    half_w = F(float(rad) / 1.4142135623730951)
    bin_f = F(1.0) / ((F(2.0) * half_w) / F(4.0))
    rad2, sig2 = rad * rad, sigma * sigma

    def bounds(c):
        return int(max(np.floor(c - rad), F(1.0))), int(min(np.ceil(c + rad), F(n - 2)))

    (xs, xe), (ys, ye), (bzs, bze) = bounds(cx), bounds(cy), bounds(cz)
    ortho = max(abs(R[a] * R[b] + R[3 + a] * R[3 + b] + R[6 + a] * R[6 + b] - F(a == b))
                for a in range(3) for b in range(a, 3))
    cube_z = half_w * (abs(R[6]) + abs(R[7]) + abs(R[8])) * F(1.001) if ortho <= F(1e-4) else rad * F(1.001)
    zs = max(bzs, int(np.floor(cz - cube_z - F(1.0))))
    ze = min(bze, int(np.ceil(cz + cube_z + F(1.0))))

    def keys(x, y, z, inside):
        dx, dy, dz = x.astype(F) - cx, y.astype(F) - cy, z.astype(F) - cz
        sq = dx * dx + dy * dy + dz * dz
        vb = [((R[i] * dx + R[3 + i] * dy + R[6 + i] * dz) + half_w) * bin_f for i in range(3)]
        lo, hi = np.minimum(np.minimum(vb[0], vb[1]), vb[2]), np.maximum(np.maximum(vb[0], vb[1]), vb[2])
        win = ~(sq > rad2) & ~(lo < 0) & ~(hi >= 4)
        w = np.exp(F(-0.5) * sq / sig2).astype(F)
        gx = F(0.5) * (G[z, y, x + 1] - G[z, y, x - 1]) * w
        gy = F(0.5) * (G[z, y + 1, x] - G[z, y - 1, x]) * w
        gz = F(0.5) * (G[z + 1, y, x] - G[z - 1, y, x]) * w
        rx = R[0] * gx + R[3] * gy + R[6] * gz
        ry = R[1] * gx + R[4] * gy + R[7] * gz
        rz = R[2] * gx + R[5] * gy + R[8] * gz
        live = inside & ~((rx * rx + ry * ry + rz * rz) < EPS)
        face = faces_of(tab, oct_, rx, ry, rz, live)
        cell = [np.clip(np.trunc(v).astype(int), 0, 2) for v in vb]
        return win, face * 64 + cell[0] + 4 * cell[1] + 16 * cell[2]

    npl = max(ze - zs + 1, 0)
    cuts = [0, (33 * npl + 50) // 100, (npl + 1) // 2, (67 * npl + 50) // 100, npl]
    one = np.array([0])
    _, first = keys(xs + one, ys + one, bzs + one, np.array([False]))
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b <= a or xe < xs or ye < ys:
            parts.append(np.zeros(0, int))
            continue
        z, y, x = [v.ravel() for v in np.meshgrid(np.arange(zs + a, zs + b), np.arange(ys, ye + 1),
                                                  np.arange(xs, xe + 1), indexing="ij")]
        win, key = keys(x, y, z, np.ones(len(x), bool))
        parts.append(key[win])
    return parts, int(first[0])


PRED = np.array([v - 1 for v in range(64)])
PRED[32], PRED[48] = 15, 31


def round_masks(keys, first):
    """One work item: [(m, count, lane keys)] per batch of 64, as the kernel forms them."""
    out, lanes = [], np.full(64, first)
    for b in range(0, len(keys), 64):
        cnt = min(64, len(keys) - b)
        lanes = lanes.copy()
        lanes[:cnt] = keys[b:b + cnt]          # lanes beyond cnt keep what they held
        rep = lanes == lanes[PRED]
        rep[0] = rep[16] = False
        m = 0
        for p in range(2):
            for u in range(16):
                if rep[32 * p + u] and rep[32 * p + 16 + u]:
                    m |= 1 << (16 * p + u)
        out.append((m, cnt, lanes, rep))
    return out


@pytest.fixture(scope="module")
def masks(oracle_mod):
    """{(volume, what): [round_masks of each of the four parts]}"""
    tab = face_table()
    oct_ = octant_table(tab)
    out, sizes = {}, {}
    for name in VOLUMES:
        o = oracle_mod.Oracle()
        assert o.detect(volume(name, oracle_mod)) == 0
        what, recs = keypoints(o, oracle_mod.KP_DTYPE)
        for w, k in zip(what, recs):
            parts, first = voxel_keys(o.level(0, 0, int(k["s"]))[0], k, tab, oct_)
            out[name, w] = [round_masks(p, first) for p in parts]
            sizes[name, w] = ([len(p) for p in parts], work_items(k["xd"], k["yd"], k["zd"], k["sd"], k["R"])[1])
    return out, sizes


def test_windows_are_the_kernels(masks):
    """The voxel count of every part equals work_items' (the restatement the quad-commit test uses), and the
    list holds the windows the GPU file's docstring names."""
    _, sizes = masks
    assert len(ROWS) <= 16
    for key, (mine, theirs) in sizes.items():
        assert mine == theirs, (key, mine, theirs)
    for v in VOLUMES:
        assert any(1 <= p % 64 <= 3 for p in sizes[v, "tail"][0])
        assert any(p % 64 == 32 for p in sizes[v, "b32"][0]) and any(p % 64 == 33 for p in sizes[v, "b33"][0])
        assert 0 in sizes[v, "corner"][0] and sum(sizes[v, "corner"][0]) > 0
        assert all(p >= 4 * 64 for p in sizes[v, "axis wide"][0])
        assert all(sum(sizes[v, w][0]) > 64 for w in ("oblique", "oblique subvoxel", "edge", "corner wide"))


def test_mask_invariants(masks):
    """Bit 0 is never set; a set bit means both voxels of the round carry their predecessors' keys."""
    out, _ = masks
    for item in out.values():
        for part in item:
            for m, cnt, lanes, rep in part:
                assert not m & 1
                for p in range(2):
                    for u in range(16):
                        if m >> (16 * p + u) & 1:
                            for v in (32 * p + u, 32 * p + 16 + u):
                                assert lanes[v] == lanes[PRED[v]] and v not in (0, 16)


def test_list_meets_every_kind(masks):
    out, _ = masks
    kinds = {k: [] for k in "abcdef"}
    for key, item in out.items():
        for pi, part in enumerate(item):
            where = key + (pi,)
            for bi, (m, cnt, lanes, rep) in enumerate(part):
                bit = [bool(m >> i & 1) for i in range(32)]
                if bit[16]:
                    kinds["a"].append(where)        # a run carried across the pass boundary inside a batch
                if bit[31] and bi + 1 < len(part):
                    nxt = part[bi + 1][2]
                    if nxt[0] == lanes[47] and nxt[16] == lanes[63]:
                        kinds["b"].append(where)    # a run that reaches round 15 of pass 1, cut by the batch rule
                for p in range(2):
                    for u in range(16):
                        r0, r1 = rep[32 * p + u], rep[32 * p + 16 + u]
                        if r0 != r1:
                            kinds["c"].append(where)    # exactly one half-wave repeats: both read
                        i = 16 * p + u
                        if i and bit[i - 1] and r0 and not r1:
                            kinds["d"].append(where)    # a run ended by a change in half-wave 1 only
                        if bit[i] and bi == len(part) - 1 and cnt < 64 and 32 * p + 16 + u >= cnt:
                            kinds["e"].append(where)    # a run in the final, partial batch, stale lanes included
            if len(part) >= 2 and not any(m for m, _, _, _ in part):
                kinds["f"].append(where)                # a work item without a skipped round
    print({k: len(set(v)) for k, v in kinds.items()})
    missing = [k for k, v in kinds.items() if not v]
    assert not missing, "kinds %s do not occur in the list" % missing


def test_share_of_skipped_rounds(masks):
    """The three volumes span the mechanism's range: on the ramp a run ends only at a cell border or a row's end,
    the noise (blurred by the pyramid, so not without runs) repeats least."""
    out, _ = masks

    def share(vol):
        ms = [m for (v, _), item in out.items() if v == vol for part in item for m, cnt, _, _ in part if cnt == 64]
        return sum(bin(m).count("1") for m in ms) / (32.0 * len(ms))

    s = {v: share(v) for v in VOLUMES}
    print(s)
    assert s["ramp"] > s["lattice"] > s["noise"], s
