"""Caller-made levels for the extrema stage (tests/test_extrema_levels.py, its host twin, oracle/make_golden.py g9_*).

Data only: recipes and the arrays they describe, no device and no library.  A recipe is JSON: seed, shape [nz, ny, nx],
range R, a list of plants and an optional scale.  build(recipe, state) gives the five DoG levels D and the six
Gaussian levels G of one octave:

  base     D[0..4] and G[5] are integer-valued PCG64 draws in [-R, R]; G[k] = G[k + 1] + D[k] in float32 is exact (small
           integers), so the stored-DoG entry (given D) and the Gaussian-level entries (given G) see the same DoG bits:
           G[k] - G[k + 1] == D[k] bit for bit.  R = 3 gives many natural ties, R = 50 about 20 % candidates;
  plants   [k, z, y, x, before, after, col0] assignments to D on top of the base (state 0: `before`, 1: `after`);
           col0 zeroes the voxel's whole column (all D and G[5]) first, so that ONE value that is no integer (a
           threshold voxel) keeps the sums exact;
  scale    "subnormal": every array times 2^-140 (integers times a power of two: differences stay exact);
           "inf": finite Gaussian levels near 2^127 whose signs alternate on a random half of the voxels, so that the
           differences overflow to +-inf there and stay finite elsewhere.

Tie sites: an isolated strict maximum V = R + 10 (minimum -V) whose one chosen neighbour holds V - 1 before and V after.
Both values lie above every base value, so no other voxel's verdict depends on the state (the host twin checks that
the two states differ in exactly the planted centres).
"""
import numpy as np

from tests import extrema_restatement as xr

F = np.float32
PEAK = 0.1

# (dk, dz, dy, dx) of the eight samples of sift.c:798-810
DIRS8 = {"prev": (-1, 0, 0, 0), "next": (1, 0, 0, 0), "x+": (0, 0, 0, 1), "x-": (0, 0, 0, -1),
         "y+": (0, 0, 1, 0), "y-": (0, 0, -1, 0), "z-": (0, -1, 0, 0), "z+": (0, 1, 0, 0)}
CROSS8 = list(DIRS8.values())
CUBE80 = [(dk, dz, dy, dx) for dk in (-1, 0, 1) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
          if (dk, dz, dy, dx) != (0, 0, 0, 0)]
# a face, an edge and a corner neighbour of each of the three levels (sift.c:761-789)
CUBOID_TIES = [(dk,) + o for dk, offs in ((-1, ((0, 0, 1), (0, 1, 1), (1, 1, 1))),
                                          (0, ((0, -1, 0), (1, 0, -1), (-1, 1, -1))),
                                          (1, ((1, 0, 0), (-1, 1, 0), (1, -1, -1)))) for o in offs]


def base(seed, shape, R):
    rng = np.random.Generator(np.random.PCG64(seed))
    draws = rng.integers(-R, R + 1, size=(6,) + tuple(shape))
    return [np.ascontiguousarray(draws[k], F) for k in range(5)], np.ascontiguousarray(draws[5], F)


def gauss_of(D, g5):
    G = [None] * 5 + [np.asarray(g5, F)]
    for k in range(4, -1, -1):
        G[k] = G[k + 1] + D[k]
    return G


def build(recipe, state=1):
    """-> (D, G): five DoG and six Gaussian levels, float32 [nz, ny, nx]."""
    shape = tuple(recipe["shape"])
    if recipe.get("scale") == "inf":
        return _build_inf(recipe)
    if recipe.get("constant") is not None:
        G = [np.full(shape, recipe["constant"], F) for _ in range(6)]
        return xr.from_gauss(G), G
    D, g5 = base(recipe["seed"], shape, recipe["range"])
    for k, z, y, x, before, after, col0 in recipe.get("plants", ()):
        if col0:
            for d in D:
                d[z, y, x] = 0.0
            g5[z, y, x] = 0.0
        D[k][z, y, x] = F(after if state else before)
    G = gauss_of(D, g5)
    if recipe.get("scale") == "subnormal":
        s = F(2.0 ** -140)
        D, G = [d * s for d in D], [g * s for g in G]
    return D, G


def _build_inf(recipe):
    shape = tuple(recipe["shape"])
    rng = np.random.Generator(np.random.PCG64(recipe["seed"]))
    B = rng.integers(0, 101, size=(6,) + shape)
    flip = rng.integers(0, 2, size=shape).astype(bool)
    G = []
    for k in range(6):
        g = (F(2.0 ** 127) * (F(1.0) + B[k].astype(F) / F(128.0))).astype(F)
        G.append(np.where(flip & (k % 2 == 1), -g, g).astype(F))
    return xr.from_gauss(G), G


def maxima(D):
    return np.array([xr.dogmax(d) for d in D], F)


# ---- placing plants ---------------------------------------------------------------------------------------------

class Placer:
    """Puts sites (a centre and some planted neighbours) where they do not disturb each other: a planted cell is never
    one of the compared samples of another site's centre."""

    def __init__(self, shape, cube=False):
        self.shape = tuple(shape)
        self.cross = CUBE80 if cube else CROSS8
        self.cells, self.guard, self.plants, self.sites = set(), set(), [], []

    def _inside(self, c):
        k, z, y, x = c
        return 0 <= k < 5 and 0 <= z < self.shape[0] and 0 <= y < self.shape[1] and 0 <= x < self.shape[2]

    def put(self, label, value, neighbours=(), ks=(1, 2, 3), zs=None, ys=None, xs=None, col0=False, interior=True):
        """value: the centre's; neighbours: [(offset, before, after)]; zs / ys / xs: allowed centre coordinates."""
        nz, ny, nx = self.shape
        lo = 1 if interior else 0
        zs = range(lo, nz - lo) if zs is None else zs
        ys = range(lo, ny - lo) if ys is None else ys
        xs = range(lo, nx - lo) if xs is None else xs
        for z in zs:
            for y in ys:
                for x in xs:
                    for k in ks:
                        c = (k, z, y, x)
                        add = lambda o: (k + o[0], z + o[1], y + o[2], x + o[3])
                        mine = [c] + [add(o) for o, _, _ in neighbours]
                        cross = [q for q in map(add, self.cross) if self._inside(q)]
                        if col0:                   # the rest of a zeroed column belongs to the site
                            cross += [(kk, z, y, x) for kk in range(5) if abs(kk - k) > 1]
                        if not all(self._inside(q) for q in mine):
                            continue
                        if any(q in self.cells or q in self.guard for q in mine) or any(q in self.cells for q in cross):
                            continue
                        self.cells.update(mine)
                        self.guard.update(cross)
                        self.plants.append([k, z, y, x, float(value), float(value), bool(col0)])
                        for q, (_, before, after) in zip(mine[1:], neighbours):
                            self.plants.append(list(q) + [float(before), float(after), False])
                        self.sites.append(dict(label=label, k=k, z=z, y=y, x=x))
                        return c
        raise AssertionError("no room for %s in %s" % (label, self.shape))


def _in(vals, lo, hi):
    return [v for v in vals if lo <= v <= hi]


def tie_recipe(name, seed, shape, R=50):
    """One site per neighbour position and route the shape has, as a maximum and as a minimum."""
    nz, ny, nx = shape
    g = xr.gauss6_geometry(nx, ny, nz)
    V = R + 10
    seg = 4 * g["txq"]
    seams = g["seams"]
    want = []
    # x: same quad; adjacent lane; across the 16-lane row (x = 63 | 64); across the segment end (ed[])
    want += [("x-", "x", v) for v in _in(sorted({2, 8, 64, seg, 2 * seg}), 2, nx - 2)]
    want += [("x+", "x", v) for v in _in(sorted({1, 7, 63, seg - 1, 2 * seg - 1}), 1, nx - 3)]
    # y: inside the tile; across its top and bottom halo rows
    want += [("y-", "y", v) for v in _in(sorted({2, g["ty"], 2 * g["ty"]}), 2, ny - 2)]
    want += [("y+", "y", v) for v in _in(sorted({1, g["ty"] - 1, 2 * g["ty"] - 1}), 1, ny - 3)]
    # z: the register rotation, and the seam between two z segments
    want += [("z-", "z", v) for v in _in(sorted({1, 2} | set(seams)), 1, nz - 2)]
    want += [("z+", "z", v) for v in _in(sorted({nz - 2, nz - 3} | {s - 1 for s in seams}), 1, nz - 2)]
    want += [("prev", None, None), ("next", None, None)]
    P = Placer(shape)
    for i, (d, axis, v) in enumerate(want):
        for sign in (1, -1):
            kw = {axis + "s": [v]} if axis else {}
            ks = [(1, 2, 3)[(i + j) % 3] for j in range(3)]
            P.put("%s@%s=%s %s" % (d, axis, v, "max" if sign > 0 else "min"), sign * V,
                  [(DIRS8[d], sign * (V - 1), sign * V)], ks=ks, **kw)
    return dict(name=name, seed=seed, shape=list(shape), range=R, plants=P.plants, sites=P.sites)


def cuboid_tie_recipe(name, seed, shape, R=50):
    V = R + 10
    P = Placer(shape, cube=True)
    for off in CUBOID_TIES:
        for sign in (1, -1):
            P.put("%s %s" % (off, "max" if sign > 0 else "min"), sign * V, [(off, sign * (V - 1), sign * V)])
    return dict(name=name, seed=seed, shape=list(shape), range=R, plants=P.plants, sites=P.sites, cuboid=True)


THR_DOGMAX = 9.0


def threshold_recipe(name="threshold", seed=31, shape=(5, 9, 16), R=3):
    """dogmax = 9 on every keypoint level and peak = 0.1: (float)(0.1 * 9.0) = 0.9f but 0.1f * 9.0f = 0.90000004f.
    Per keypoint level a voxel exactly at thr, one an ulp above, the mirror pair at -thr (all with zero
    neighbours, in a zero column), and a POSITIVE strict minimum above thr."""
    T = xr.threshold(PEAK, THR_DOGMAX)
    up = np.nextafter(T, F(1.0))
    P = Placer(shape)
    zero6 = [(o, 0.0, 0.0) for o in CROSS8 if o[0] == 0]
    for k in (1, 2, 3):
        # the level's maximum: on a face, where nothing is a candidate
        P.put("dogmax k%d" % k, THR_DOGMAX, ks=(k,), zs=[0], interior=False)
        P.put("at +thr k%d" % k, T, zero6, ks=(k,), col0=True)
        P.put("above +thr k%d" % k, up, zero6, ks=(k,), col0=True)
        P.put("at -thr k%d" % k, -T, zero6, ks=(k,), col0=True)
        P.put("below -thr k%d" % k, -up, zero6, ks=(k,), col0=True)
        P.put("positive minimum k%d" % k, 2.0, [(o, 3.0, 3.0) for o in CROSS8], ks=(k,))
    return dict(name=name, seed=seed, shape=list(shape), range=R, plants=P.plants, sites=P.sites)


def border_recipe(name, seed, shape, R=50):
    """Strict maxima and minima ON the six faces (never candidates, sift.c:832-835) and on the first and last interior
    line of every axis; mask bits 0 and 63 (x = 64, x = 63) where the row is long enough."""
    nz, ny, nx = shape
    V = R + 10
    P = Placer(shape)
    for i, (axis, n) in enumerate((("x", nx), ("y", ny), ("z", nz))):
        for v in (0, n - 1):
            for sign in (1, -1):                  # (inside the face: only this axis' bound rejects the voxel)
                kw = dict(zs=range(1, nz - 1), ys=range(1, ny - 1), xs=range(1, nx - 1))
                kw[axis + "s"] = [v]
                P.put("face %s=%d" % (axis, v), sign * (V + 7), interior=False, **kw)
        for v in sorted({1, n - 2}):
            for sign in (1, -1):
                P.put("%s=%d %s" % (axis, v, "max" if sign > 0 else "min"), sign * V, **{axis + "s": [v]})
    for v in (63, 64, 127, 128):
        if 1 <= v <= nx - 2:
            for sign in (1, -1):
                P.put("x=%d (bit %d) %s" % (v, v % 64, "max" if sign > 0 else "min"), sign * V, xs=[v])
    return dict(name=name, seed=seed, shape=list(shape), range=R, plants=P.plants, sites=P.sites)


def est_recipes():
    """The unique maximum of a level on plane 0 only, on plane nz - 1 only, at the last row and column, off the
    sub-lattice; and a volume that is zero on the whole sub-lattice."""
    out = []
    shape, R = (7, 8, 16), 50
    nz, ny, nx = shape
    for name, (z, y, x) in (("est_plane0", (0, 4, 5)), ("est_plane_last", (nz - 1, 4, 6)),
                            ("est_last_row_col", (2, ny - 1, nx - 1)), ("est_off_lattice", (3, 4, 7))):
        plants = [[k, z, y, x, 200.0 + k, 200.0 + k, False] for k in range(5)]
        out.append(dict(name=name, seed=41, shape=list(shape), range=R, plants=plants))
    plants = []
    for z in xr.sub_lattice_planes(nz):
        for y in range(0, ny, xr.SUB_Y):
            for x in range(nx):
                plants.append([0, z, y, x, 0.0, 0.0, True])
    out.append(dict(name="est_zero_lattice", seed=42, shape=list(shape), range=R, plants=plants))
    return out


def plain(name, seed, shape, R=50, plants=(), **kw):
    return dict(name=name, seed=seed, shape=list(shape), range=R, plants=[list(p) for p in plants], **kw)


def _one_max(shape, R=50):
    """A strict maximum at the first interior voxel of keypoint level 2 (a shape with almost no interior)."""
    return [[2, 1, 1, 1, R + 10.0, R + 10.0, False]]


# a. every instantiation and route.  [nz, ny, nx]; TXQ 16: nx < 128, TXQ 32: nx < 256, TXQ 64 above.
SHAPES = [
    plain("3x3x4", 1, (3, 3, 4), plants=_one_max((3, 3, 4))),
    plain("5x16x8", 2, (5, 16, 8)),
    plain("5x17x64", 3, (5, 17, 64)),
    plain("5x7x68", 4, (5, 7, 68)),
    plain("3x19x68", 5, (3, 19, 68)),
    plain("5x8x128", 6, (5, 8, 128)),
    plain("3x11x132", 7, (3, 11, 132)),
    plain("6x9x132 +-3", 8, (6, 9, 132), R=3),
    plain("5x4x256", 9, (5, 4, 256)),
    plain("3x7x260", 10, (3, 7, 260)),
    plain("35x7x8 z seam", 11, (35, 7, 8)),
    plain("5x7x68 +-3", 12, (5, 7, 68), R=3),
    # (G9 below refers to entries 3 and 7 by index: append only)  a z seam under the two wider instantiations, and
    # nine tiles whose last one has interior rows
    plain("35x8x128 z seam", 13, (35, 8, 128)),
    plain("35x4x256 z seam", 14, (35, 4, 256)),
    plain("3x131x64", 15, (3, 131, 64)),
]
# tile counts of the XCD remap: nx = 64 (one tile across), 16-row tiles, one z segment
TILE_COUNTS = {1: 16, 7: 97, 8: 113, 9: 129, 15: 225, 17: 257}          # tiles -> ny
TILES = [plain("%d tiles" % t, 20 + t, (3, ny, 64)) for t, ny in TILE_COUNTS.items()]
# g. more than one scan chunk (3 * nblk > 8192) with the block counts at both alignments; a small odd word count
SCAN = [plain("scan nwords odd", 51, (585, 599, 4)), plain("scan nwords even", 52, (585, 600, 4))]

TIES = [tie_recipe("ties txq16", 61, (5, 35, 68)), tie_recipe("ties txq32", 62, (5, 19, 132)),
        tie_recipe("ties txq64", 63, (5, 11, 260)), tie_recipe("ties z seam", 64, (35, 7, 8)),
        tie_recipe("ties nx4", 65, (7, 40, 4))]
CUBOID_TIE = cuboid_tie_recipe("ties cuboid", 66, (7, 12, 23))
THRESHOLD = threshold_recipe()
BORDERS = [border_recipe("borders 5x9x68", 71, (5, 9, 68)), border_recipe("borders nx4", 72, (5, 40, 4)),
           border_recipe("borders nz3", 73, (3, 12, 132))]
SUBNORMAL = plain("subnormal", 4, (5, 7, 68), scale="subnormal")
SUBNORMAL_BASE = plain("5x7x68", 4, (5, 7, 68))
INF = dict(name="inf", seed=81, shape=[5, 7, 68], range=0, plants=[], scale="inf")
CONSTANT = dict(name="constant", seed=0, shape=[5, 7, 68], range=0, plants=[], constant=7.0)
EST = est_recipes()
# h. octave lists of differing dims ([nz, ny, nx])
FINISH_DIMS = [(9, 19, 68), (5, 11, 36), (5, 7, 20), (3, 5, 8), (3, 3, 4)]



def stack(seed, shape, R, n):
    """n unrelated integer-valued levels (the stored-DoG entry takes any triples)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return [np.ascontiguousarray(a, F) for a in rng.integers(-R, R + 1, size=(n,) + tuple(shape))]


# e. sift3d_hip_extrema_mode: which mask kernel a configuration reaches (xr.mode_route).  Level i of a case is the
# triple (S[i], S[i + 1], S[i + 2]) of stack(seed, shape, 50, nlevels + 2); z: one (z_lo, z_hi) or one per level;
# off4: the levels lie 4 bytes past a 16-byte boundary.
MODE_CASES = [
    dict(name="3 levels", seed=91, shape=(6, 9, 12), nlevels=3, route="sweep3"),
    dict(name="3 levels, slab", seed=91, shape=(9, 9, 12), nlevels=3, z=(3, 6), route="sweep3"),
    dict(name="3 levels, empty slab", seed=91, shape=(6, 9, 12), nlevels=3, z=(4, 4), route="sweep3"),
    dict(name="3 levels, z ranges differ", seed=92, shape=(9, 9, 12), nlevels=3, z=[(1, 8), (2, 5), (4, 8)],
         route="mask"),
    dict(name="3 levels, 4 bytes off", seed=93, shape=(6, 9, 12), nlevels=3, off4=True, route="mask"),
    dict(name="3 levels, cuboid", seed=94, shape=(6, 9, 12), nlevels=3, cuboid=True, route="mask_cuboid"),
    dict(name="1 level", seed=95, shape=(5, 7, 8), nlevels=1, route="mask"),
    dict(name="2 levels", seed=96, shape=(5, 7, 8), nlevels=2, route="mask"),
    dict(name="4 levels", seed=97, shape=(5, 7, 8), nlevels=4, route="mask"),
    dict(name="8 levels", seed=98, shape=(5, 7, 8), nlevels=8, route="mask"),
    dict(name="8 levels, cuboid", seed=98, shape=(5, 7, 8), nlevels=8, cuboid=True, route="mask_cuboid"),
] + [dict(name="nx %d" % nx, seed=100 + nx, shape=(5, 6, nx), nlevels=3, route="mask") for nx in (5, 63, 65, 66)]


def mode_levels(case):
    """-> (stack, level dicts for xr.records with the maxima of the whole levels)."""
    S = stack(case["seed"], case["shape"], 50, case["nlevels"] + 2)
    nz = case["shape"][0]
    z = case.get("z", (1, nz - 1))
    zr = [z] * case["nlevels"] if isinstance(z, tuple) else z
    return S, [dict(prev=S[i], cur=S[i + 1], next=S[i + 2], absmax=xr.dogmax(S[i + 1]), tag=10 + i, z_lo=zr[i][0],
                    z_hi=zr[i][1]) for i in range(case["nlevels"])]


# the g9 fixtures of the reference (oracle/make_golden.py): (fixture, recipe, state, peak, cuboid)
G9 = ([("g9_ties_%d" % i, r, s, PEAK, False) for i, r in enumerate(TIES[:4]) for s in (0, 1)]
      + [("g9_threshold", THRESHOLD, 1, PEAK, False), ("g9_threshold_peak1", THRESHOLD, 1, 1.0, False)]
      + [("g9_borders_%d" % i, r, 1, PEAK, False) for i, r in enumerate(BORDERS)]
      + [("g9_subnormal", SUBNORMAL, 1, PEAK, False), ("g9_inf", INF, 1, PEAK, False),
         ("g9_pm3", SHAPES[7], 1, PEAK, False),
         ("g9_cuboid_ties", CUBOID_TIE, 0, PEAK, True), ("g9_cuboid_ties", CUBOID_TIE, 1, PEAK, True),
         ("g9_cuboid", SHAPES[3], 1, PEAK, True)])


def g9_key(recipe, state, peak, cuboid):
    return "%s|state%d|peak%r|%s" % (recipe["name"], state, peak, "cuboid" if cuboid else "8")


def truth(recipe, state=1, peak=PEAK, cuboid=False, z_lo=None, z_hi=None, tag0=0):
    """The restatement's records for a recipe, with the maxima of the whole levels."""
    D, _ = build(recipe, state)
    return xr.octave_records(D, peak, maxima(D), tag0, z_lo, z_hi, cuboid)
