"""detect_extrema (sift.c:735-871) on caller-made levels, restated in plain numpy: float32 data, no device.

Levels are [nz, ny, nx] float32 arrays (x fastest).  What is restated:

  from_gauss      D[k] = G[k] - G[k+1] in float32 (im_subtract, imutil.c:719-739): for the Gaussian-level entries of the
                  device library the truth is always this difference of the arrays handed to the device;
  dogmax          max |D| over a whole level, starting from 0.0f (sift.c:822-826);
  threshold       (float)(double peak_thresh * float dogmax) (sift.c:739, 829);
  extremum8       strictly above or strictly below the eight samples of sift.c:798-810 (six in the level, one in the
                  previous and one in the next DoG level);
  extremum_cuboid the CUBOID_EXTREMA build's 27 + 26 + 27 samples (sift.c:761-796);
  records         (idx = x + nx*(y + ny*z), tag, val = |D|) in (level, z, y, x) order over the planes [z_lo, z_hi) of
                  each level, both thresholds strict (sift.c:842); the caller supplies the maxima, as it does for the
                  device entries, so that a slab can use those of the whole volume;
  sub_lattice_max the maxima sift3d_hip_dogmax_sub documents (include/sift3d_amd.h): planes z = 1, 6, 11, ... (plane 0
                  of a one-plane level), rows y = 0, 3, 6, ..., every x.

For the host twin (tests/test_extrema_levels_host.py) only, the launch geometry that decides which code of
sift3d_amd/csrc/sift3d_extrema.hip a shape reaches: txq / TY from nx, sweep_segments and its z seams, the tile count,
wpr / nwords / nblk, the alignment of the block-count array and the number of scan chunks, and the route
sift3d_hip_extrema_mode takes.
"""
import numpy as np

F = np.float32
CAND_DTYPE = np.dtype([("idx", "u4"), ("tag", "i4"), ("val", "f4")])     # sift3d_hip_cand

EX_WPB = 128          # 64-voxel mask words per block of the count / scan / emit kernels
SCAN_CHUNK = 8192     # entries ex_scan_range scans between two carries
SUB_Z, SUB_Y = 5, 3   # strides of the sub-lattice
MAX_OCT = 12          # SIFT3D_HIP_EXTREMA_MAX_OCT


def from_gauss(G):
    with np.errstate(over="ignore"):
        return [np.asarray(G[k], F) - np.asarray(G[k + 1], F) for k in range(len(G) - 1)]


def dogmax(D):
    m = F(0.0)
    a = np.abs(np.asarray(D, F))
    return F(max(m, a.max())) if a.size else m


def threshold(peak, dmax):
    with np.errstate(over="ignore"):
        return F(np.float64(peak) * np.float64(F(dmax)))


def _interior(shape):
    m = np.zeros(shape, bool)
    m[1:-1, 1:-1, 1:-1] = True
    return m


def _shift(a, dz, dy, dx):
    """a[z + dz, y + dy, x + dx] on the interior voxels (a view of shape (nz - 2, ny - 2, nx - 2))."""
    nz, ny, nx = a.shape
    return a[1 + dz:nz - 1 + dz, 1 + dy:ny - 1 + dy, 1 + dx:nx - 1 + dx]


def _strict(cur, others):
    c = _shift(cur, 0, 0, 0)
    gt = np.ones(c.shape, bool)
    lt = np.ones(c.shape, bool)
    for o in others:
        gt &= c > o
        lt &= c < o
    out = np.zeros(cur.shape, bool)
    out[1:-1, 1:-1, 1:-1] = gt | lt
    return out


def extremum8(prev, cur, nxt):
    """sift.c:798-810, 844-849: a bool per voxel, False on the six faces (sift.c:832-835)."""
    if min(cur.shape) < 3:
        return np.zeros(cur.shape, bool)
    others = [_shift(prev, 0, 0, 0), _shift(nxt, 0, 0, 0)]
    for d in ((0, 0, 1), (0, 0, -1), (0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0)):
        others.append(_shift(cur, *d))
    return _strict(cur, others)


def extremum_cuboid(prev, cur, nxt):
    """sift.c:761-796: all 27 samples of the previous and of the next level, the 26 neighbours in the level."""
    if min(cur.shape) < 3:
        return np.zeros(cur.shape, bool)
    others = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                others.append(_shift(prev, dz, dy, dx))
                others.append(_shift(nxt, dz, dy, dx))
                if dz or dy or dx:
                    others.append(_shift(cur, dz, dy, dx))
    return _strict(cur, others)


def level_mask(prev, cur, nxt, thr, z_lo=None, z_hi=None, cuboid=False):
    """The voxels of one level detect_extrema keeps, restricted to the planes [z_lo, z_hi)."""
    cur = np.asarray(cur, F)
    nz = cur.shape[0]
    z_lo = 1 if z_lo is None else z_lo
    z_hi = nz - 1 if z_hi is None else z_hi
    m = (extremum_cuboid if cuboid else extremum8)(np.asarray(prev, F), cur, np.asarray(nxt, F))
    m &= (cur > F(thr)) | (cur < -F(thr))                                  # sift.c:842, both strict
    zz = np.arange(nz)
    m &= ((zz >= z_lo) & (zz < z_hi))[:, None, None]
    return m


def records(levels, peak, cuboid=False):
    """levels: dicts(prev, cur, next, absmax, tag[, z_lo, z_hi]) in output order -> CAND_DTYPE records."""
    out = []
    for L in levels:
        cur = np.asarray(L["cur"], F)
        m = level_mask(L["prev"], cur, L["next"], threshold(peak, L["absmax"]), L.get("z_lo"), L.get("z_hi"), cuboid)
        idx = np.flatnonzero(m)                                            # C order of [nz, ny, nx]: z, y, x
        r = np.zeros(len(idx), CAND_DTYPE)
        r["idx"], r["tag"], r["val"] = idx, L["tag"], np.abs(cur.reshape(-1)[idx])
        out.append(r)
    return np.concatenate(out) if out else np.zeros(0, CAND_DTYPE)


def octave_levels(D, absmax=None, tag0=0, z_lo=None, z_hi=None):
    """The keypoint levels 1 .. len(D) - 2 of an octave's DoG levels, as records() takes them."""
    absmax = [dogmax(d) for d in D] if absmax is None else absmax
    return [dict(prev=D[k - 1], cur=D[k], next=D[k + 1], absmax=absmax[k], tag=tag0 + k - 1, z_lo=z_lo, z_hi=z_hi)
            for k in range(1, len(D) - 1)]


def octave_records(D, peak, absmax=None, tag0=0, z_lo=None, z_hi=None, cuboid=False):
    return records(octave_levels(D, absmax, tag0, z_lo, z_hi), peak, cuboid)


def sub_lattice_planes(nz):
    return list(range(1, nz, SUB_Z)) if nz >= 2 else [0]


def sub_lattice_max(D):
    D = np.asarray(D, F)
    sub = np.abs(D[sub_lattice_planes(D.shape[0])][:, ::SUB_Y, :])
    return F(max(F(0.0), sub.max()))


# ---- launch geometry (host twin only) ---------------------------------------------------------------------------

def txq(nx):
    return 64 if nx >= 256 else 32 if nx >= 128 else 16


def tile_rows(nx):
    return 256 // txq(nx)


def sweep_segments(n_out, bxy):
    """Planes per z segment: about 2048 workgroups in all, in segments of 16 planes or more."""
    nseg = min(-(-2048 // bxy), max(n_out // 16, 1))
    return -(-n_out // nseg)


def gauss6_geometry(nx, ny, nz, z_lo=1, z_hi=None):
    """What sift3d_hip_extrema_gauss6* launch for a level of these dims."""
    z_hi = nz - 1 if z_hi is None else z_hi
    q, ty = txq(nx), tile_rows(nx)
    gx, gy = -(-nx // (4 * q)), -(-ny // ty)
    n_out = z_hi - z_lo
    ts = sweep_segments(n_out, gx * gy) if n_out > 0 else 0
    gz = -(-n_out // ts) if n_out > 0 else 0
    wpr = -(-nx // 64)
    nwords = nz * ny * wpr
    nblk = -(-nwords // EX_WPB)
    return dict(txq=q, ty=ty, gx=gx, gy=gy, gz=gz, ts=ts, tiles=gx * gy * gz,
                seams=[z_lo + k * ts for k in range(1, gz)],               # first plane of every segment but the first
                wpr=wpr, nwords=nwords, nblk=nblk,
                blk_aligned16=(3 * nwords * 8) % 16 == 0,                  # blk = masks + 3 * nwords (d_work: 16 B aligned)
                scan_chunks=-(-3 * nblk // SCAN_CHUNK))


def xcd_remap(T):
    """The tile each workgroup of k_extrema_sweep3g sweeps, by launch order: XCD k (workgroups k, k + 8, ...) takes
    the k-th eighth of the T tiles, the first T % 8 XCDs one tile more."""
    q, r = T >> 3, T & 7
    return [(L & 7) * q + min(L & 7, r) + (L >> 3) for L in range(T)]


def mode_route(nx, nz, nlevels, cuboid=False, chained=True, aligned=True, same_z=True, z_lo=1, z_hi=None):
    """The mask kernel sift3d_hip_extrema_mode picks: 'sweep3', 'mask' or 'mask_cuboid'.  chained: the levels share
    their DoG arrays (next of level i is cur of level i + 1); aligned: every level 16-byte aligned; same_z: one z
    range for all levels."""
    z_hi = nz - 1 if z_hi is None else z_hi
    if cuboid:
        return "mask_cuboid"
    if (nlevels == 3 and nx % 4 == 0 and nz >= 3 and chained and aligned and same_z and z_lo >= 1 and z_hi <= nz - 1):
        return "sweep3"
    return "mask"


def gauss6_covered(nx, nz, z_lo=1, z_hi=None, aligned=True):
    z_hi = nz - 1 if z_hi is None else z_hi
    return nx % 4 == 0 and nz >= 3 and z_lo >= 1 and z_hi <= nz - 1 and aligned
