"""Caller-made candidate lists for the orientation stage (sift3d_orient.hip) -- TEST INFRASTRUCTURE ONLY.

Shared by tests/test_oracle_golden.py (the oracle against the g8 fixtures of the reference), tests/
test_orient_candidates_host.py (restatements, no GPU) and tests/test_orient_candidates.py (the stage entries
sift3d_hip_orient / sift3d_hip_orient_tab against the oracle's orc_orient_conf).

A LIST is (levels, cands): `levels` are the dicts tests/cpu_backend.py and hip.level_table consume (data: a numpy
array [nz_loc, ny, nx] here, off, nz_glob, units, octave, sd), `cands` hip.CAND_DTYPE records (idx: the voxel's
index in the LOCAL array, tag: the level).  Every list is GROUPED BY LEVEL, TAG ASCENDING -- the order of the
extrema stage, and what k_orient_groups assumes: it takes a level's candidates to be the one run between the first
and the last record that carry its tag.  Inside a level the order is free (the kernels treat every candidate on its
own), and the tests shuffle it on purpose.  Every candidate has 1 <= x <= nx - 2 (y, z alike): what the extrema
stage guarantees.
"""
import json
import math

import numpy as np

from tests import util

F = np.float32
CAND_DTYPE = np.dtype([("idx", "u4"), ("tag", "i4"), ("val", "f4")])      # = hip.CAND_DTYPE

G8 = ["g8_survey", "g8_aniso", "g8_scales", "g8_noise", "g8_noise_blur", "g8_faint"]
RTOL = 1e-5                  # the project's bar on R against the reference (BASELINE.json north_star)
THRESHOLDS = (0.0, 0.2, 0.4, 0.6)


# ---- g8 fixtures -----------------------------------------------------------------------------------------------

def g8_cases(g):
    return json.loads(str(g["cases"]))


def g8_case(g, case):
    return {k: g["%s_%s" % (case, k)] for k in ("os", "xyz", "sd", "scale", "status", "conf", "R")}


def g8_list(c, level_fn):
    """One g8 case as a list: one level descriptor per distinct (o, s, sd), in the case's own order (the fixtures
    are grouped), over level_fn(o, s) -> (array, units) multiplied by the case's level scale.  Returns levels, cands
    and `order`, the case's entries in list order (cands[i] is entry order[i])."""
    keys = []
    for o, s, sd in zip(c["os"][:, 0].tolist(), c["os"][:, 1].tolist(), c["sd"].tolist()):
        if (o, s, sd) not in keys:
            keys.append((o, s, sd))
    levels, picks, order = [], [], []
    for o, s, sd in keys:
        a, u = level_fn(o, s)
        m = np.nonzero((c["os"][:, 0] == o) & (c["os"][:, 1] == s) & (c["sd"] == sd))[0]
        levels.append(dict(data=np.ascontiguousarray(a * F(c["scale"])), off=0, nz_glob=a.shape[0],
                           units=tuple(float(v) for v in u), octave=o, sd=sd))
        picks.append(c["xyz"][m])
        order.append(m)
    return levels, make_cands(levels, picks), np.concatenate(order)


# ---- lists -----------------------------------------------------------------------------------------------------

def level(data, sd, units=(1.0, 1.0, 1.0), off=0, nz_glob=None, octave=0):
    data = np.ascontiguousarray(data, F)
    return dict(data=data, off=int(off), nz_glob=int(data.shape[0] if nz_glob is None else nz_glob),
                units=tuple(float(v) for v in units), octave=octave, sd=float(sd))


def make_cands(levels, picks):
    """picks[t]: (m, 3) voxels (x, y, z GLOBAL) of level t, in the order given -> records grouped by tag."""
    out = []
    for tag, (L, p) in enumerate(zip(levels, picks)):
        p = np.asarray(p, np.int64).reshape(-1, 3)
        nzl, ny, nx = L["data"].shape
        zl = p[:, 2] - L["off"]
        assert ((p[:, 0] >= 1) & (p[:, 0] <= nx - 2) & (p[:, 1] >= 1) & (p[:, 1] <= ny - 2)).all()
        assert ((p[:, 2] >= 1) & (p[:, 2] <= L["nz_glob"] - 2) & (zl >= 1) & (zl <= nzl - 2)).all()
        c = np.zeros(len(p), CAND_DTYPE)
        c["idx"], c["tag"], c["val"] = p[:, 0] + nx * (p[:, 1] + ny * zl), tag, 1.0
        out.append(c)
    return np.concatenate(out) if out else np.zeros(0, CAND_DTYPE)


def voxels(levels, cands):
    """(n, 3) x, y, z GLOBAL of every record."""
    out = np.zeros((len(cands), 3), np.int64)
    for i, c in enumerate(cands):
        L = levels[int(c["tag"])]
        nzl, ny, nx = L["data"].shape
        idx = int(c["idx"])
        out[i] = idx % nx, (idx // nx) % ny, idx // (nx * ny) + L["off"]
    return out


def random_voxels(rng, shape, n, margin=1):
    nz, ny, nx = shape
    return np.stack([rng.integers(margin, d - margin, n) for d in (nx, ny, nz)], 1)


def oracle(so, levels, cands, whole=None):
    """orc_orient_conf on every record: R (n, 9), conf, status.  The keep flags at a threshold are keep_at().
    whole[t]: the level's whole volume (the oracle does not clamp a window to a slab's planes)."""
    n = len(cands)
    R, conf, status = np.zeros((n, 9), F), np.zeros(n), np.zeros(n, np.int32)
    xyz = voxels(levels, cands)
    for tag, L in enumerate(levels):
        m = np.nonzero(cands["tag"] == tag)[0]
        if not len(m):
            continue
        if whole is not None and whole.get(tag) is not None:
            _, R[m], conf[m], status[m] = so.orient_conf(whole[tag], L["units"], L["sd"], xyz[m])
        else:
            _, R[m], conf[m], status[m] = so.orient_conf(L["data"], L["units"], L["sd"], xyz[m], off=L["off"],
                                                         nz_glob=L["nz_glob"])
    return R, conf, status


def keep_at(conf, status, thresh):
    """assign_orientation_thresh (sift.c:1100-1101): kept unless REJECT or conf < thresh."""
    return ((status == 0) & ~(conf < thresh)).astype(np.int32)


# ---- restatements of the kernels' level-only decisions ------------------------------------------------------------

TAB_CAP, TAB_ROWS = 8192, 4096         # ORI_TAB_CAP (quads), ORI_TAB_ROWS


def table_count(sd, units):
    """k_orient_table's counting for a level: the rows (j, l) of its search box, first / len of the in-sphere
    interval of every row, quads = sum ceil(len / 4), and whether the level gets a table."""
    ux, uy, uz = (F(v) for v in units)
    rad = 1.5 * sd * 3.0
    rad2 = rad * rad
    e = [rad / float(u) + 2.0 for u in (ux, uy, uz)]
    if not all(0.0 < v < 500.0 for v in e):
        return dict(rows=0, quads=0, voxels=0, table=False, first=None, len=None)
    mx, my, mz = (int(v) for v in e)
    wy, wz = 2 * my + 1, 2 * mz + 1
    i = np.arange(-mx, mx + 1).astype(F)[None, None, :] * ux
    j = np.arange(-my, my + 1).astype(F)[None, :, None] * uy
    l = np.arange(-mz, mz + 1).astype(F)[:, None, None] * uz
    sq = (i * i + j * j) + l * l                                        # float32, the reference's order
    assert sq.dtype == F
    inside = ~(sq.astype(np.float64) > rad2)
    ln = inside.sum(axis=2)
    first = np.where(ln > 0, inside.argmax(axis=2) - mx, 0)
    quads = int(((ln + 3) // 4).sum())
    rows = wy * wz
    return dict(rows=rows, quads=quads, voxels=int(ln.sum()), first=first, len=ln,
                table=rows <= TAB_ROWS and quads <= TAB_CAP)


def lut_used(sd, units):
    """orient_serial's weight table: isotropic power-of-two units u with rad^2 / u^2 < 191 (and u^2 * 192 < 2^24)."""
    ux, uy, uz = (F(v) for v in units)
    if not (ux == uy == uz) or ux <= 0:
        return False
    mant, _ = math.frexp(float(ux))
    rad = 1.5 * sd * 3.0
    u2 = ux * ux
    return mant == 0.5 and rad * rad / float(u2) < 191.0 and float(u2 * F(192)) < 16777216.0


# sd pairs on either side of a limit, per units: (units, sd below, sd above, what)
LIMIT_PAIRS = [
    ((1.0, 1.0, 1.0), 4.2, 4.3, "quads"),
    ((4.0, 1.0, 1.0), 6.4, 6.6, "quads"),
    ((8.0, 1.0, 1.0), 6.6, 6.8, "rows"),
    ((1.0, 1.0, 1.0), 3.0, 3.2, "lut"),
    ((2.0, 2.0, 2.0), 6.0, 6.4, "lut"),
    ((0.5, 0.5, 0.5), 1.5, 1.6, "lut"),
]
NO_LUT = ((1.5, 1.5, 1.5), 2.0)         # isotropic, not a power of two: never the table of weights


def window_fits(nx, ny, ux, uy, sd):
    """sift3d_hip_orient_window_fits restated: min(n - 2, 2 ceil(4.5 sd / u) + 1) <= 1023 on x and y."""
    for n, u in ((nx, ux), (ny, uy)):
        w = n - 2.0
        if u > 0.0 and sd > 0.0:
            w = min(w, 2.0 * math.ceil(1.5 * sd * 3.0 / u) + 1.0)
        if w > 1023.0:
            return 0
    return 1


def window_planes(sd, uz):
    """Planes each way of a candidate's window box: ceil(4.5 sd / uz) + 1."""
    return int(math.ceil(1.5 * sd * 3.0 / float(F(uz)))) + 1
