"""The cases of tests/test_sampling_matrix.py and tests/test_sampling_fuzz.py (no device here).

Every registration kernel is built on one sampling core (sift3d_amd/csrc/sift3d_resample.h), and each launcher picks a
template instantiation per call.  selection_key restates those choices in Python, ALL_KEYS lists every choice a
launcher can make, MATRIX holds one smallest case per key and fuzz_cases draws seeded cases stratified by key, so that
an instantiation that arrives without a case fails tests/test_sampling_matrix_host.py.

A case is data only: shapes, interpolation, which masks exist, bins, the output's alignment, the compose variant and a
seed.  build(case) makes its arrays, the same on the host and in the device tests.

A moving axis of length 1 is inside only at coordinate 0 exactly, so build() makes that coordinate exact: the affine's
row is zero (its shift too), a field's channel is -p (integers: the sum p + u is exact), a lattice channel and the
spline weights of that axis are zero."""
import collections
import types

import numpy as np

from tests import ffd_restatement as ffr
from tests import field_restatement as fr
from tests import mask_restatement as mr
from tests.test_similarity import volumes
from tests.test_warp import about_center, rot
from tests.tps_restatement import ref_tps_coords

F32 = np.float32
RANGE = (-1.0, 1.5)                                         # volumes() puts values at, and beyond, both ends
FILL = -1.5

Case = collections.namedtuple("Case", "family fshape mshape interp field wf wm bins align mode stats spacing seed "
                                      "nonfinite")
TPS = collections.namedtuple("TPS", "ctrl weights A")       # the fields of api.TPS that hip.warp_tps reads

# family -> (kernel, the names of the key's entries after the family).  One line per family: a new metric adds a line.
KERNELS = (
    ("warp_affine", "k_warp_affine", ("linear", "vec")),
    ("warp_tps", "k_warp_tps", ("linear",)),
    ("warp_field", "k_warp_field", ("linear", "vec")),
    ("compose", "k_field_compose", ("mode", "linear", "stats", "vec")),
    ("similarity", "k_similarity", ("linear", "field", "masked")),
    ("msd", "k_affine_normal", ("linear", "masked")),
    ("ncc", "k_affine_ncc_normal", ("linear", "masked")),   # both of its passes (PART 1 and 2) run in every call
    ("parzen", "k_parzen_hist", ("linear", "masked")),
    ("mi", "k_affine_mi_normal", ("linear", "masked")),
    ("ffd", "k_ffd_force", ("linear", "masked")),
)
FAMILIES = tuple(k[0] for k in KERNELS)
KEY_FIELDS = {k[0]: k[2] for k in KERNELS}
MASKED_FAMILIES = ("similarity", "msd", "ncc", "parzen", "mi", "ffd")
STORE_FAMILIES = ("warp_affine", "warp_tps", "warp_field", "compose")     # their output sits between guard bands


def case(family, fshape, mshape, interp="linear", field=False, wf=False, wm=False, bins=19, align=0, mode="compose",
         stats=False, spacing=(4, 3, 2), seed=1, nonfinite=False):
    return Case(family, tuple(fshape), tuple(mshape), interp, bool(field), bool(wf), bool(wm), int(bins), int(align),
                mode, bool(stats), tuple(spacing), int(seed), bool(nonfinite))


# ---- the launchers' choices ------------------------------------------------------------------------------------------
def linear_of(interp, nx):
    """LINEAR: 0 nearest, 2 a moving grid with nx >= 2, 1 nx == 1 (the ternaries of every launcher below)"""
    return 0 if interp == "nearest" else 2 if nx >= 2 else 1


def vec_of(c):
    """grid_args (sift3d_resample.h): vec = ox % 4 == 0 and dst 16-byte aligned; align is dst's offset in floats"""
    return int(c.fshape[2] % 4 == 0 and c.align % 4 == 0)


def selection_key(family, c):
    assert family == c.family
    nx = c.mshape[2]
    masked = c.wf or c.wm
    if family == "warp_affine":                             # sift3d_warp.hip 522
        return (family, linear_of(c.interp, nx), vec_of(c))
    if family == "warp_tps":                                # sift3d_warp.hip 565 (plane stores: no exchange, no vec)
        return (family, linear_of(c.interp, nx))
    if family == "warp_field":                              # sift3d_warp.hip 641
        return (family, linear_of(c.interp, nx), vec_of(c))
    if family == "compose":                                 # sift3d_warp.hip 712 (linear only: ux >= 2 ? 2 : 1)
        return (family, c.mode, linear_of("linear", nx), c.stats, vec_of(c))
    if family == "similarity":                              # sift3d_similarity.hip run(); FIELD, MASKED: its launcher
        return (family, linear_of(c.interp, nx), c.field, masked)
    if family == "msd":                                     # sift3d_affine_normal_launch
        return (family, linear_of("linear", nx), masked)
    if family == "ncc":                                     # sift3d_affine_refine.hip ncc_pass()
        return (family, linear_of("linear", nx), masked)
    if family == "parzen":                                  # sift3d_parzen_hist_launch
        return (family, linear_of("linear", nx), masked)
    if family == "mi":                                      # sift3d_affine_mi_normal_launch
        return (family, linear_of("linear", nx), masked)
    if family == "ffd":                                     # sift3d_ffd.hip sift3d_ffd_evaluate_launch()
        return (family, linear_of("linear", nx), masked)
    raise KeyError(family)


_VALUES = {"linear": (0, 1, 2), "vec": (0, 1), "mode": ("compose", "invert"), "stats": (False, True),
           "field": (False, True), "masked": (False, True)}


def _keys_of(family):
    keys = [(family,)]
    for name in KEY_FIELDS[family]:
        vals = _VALUES[name]
        if name == "linear" and family not in ("warp_affine", "warp_tps", "warp_field", "similarity"):
            vals = (1, 2)                                   # no nearest instantiation of the gradient kernels, of compose
        keys = [k + (v,) for k in keys for v in vals]
    return keys


# 49 kernel instantiations (3 + 3 + 3 + 8 + 12 + 5 * 4; the NCC's two passes count as one choice), and the run-time
# store path vec 0 / 1 of the three kernels that store through exchange_store: 63 keys
ALL_KEYS = frozenset(k for f in FAMILIES for k in _keys_of(f))
INSTANTIATIONS = frozenset(k[:len(k) - ("vec" in KEY_FIELDS[k[0]])] for k in ALL_KEYS)
assert len(INSTANTIATIONS) == 49 and len(ALL_KEYS) == 63


def key_dict(key):
    return dict(zip(KEY_FIELDS[key[0]], key[1:]))


# ---- one smallest case per key ---------------------------------------------------------------------------------------
# x extents of 1, 5, 64 and 70: the one-voxel axis, a partial tile, exactly one tile, a tile and a tail.
def _matrix():
    out = []
    n = 0
    for key in sorted(ALL_KEYS, key=repr):
        f, k = key[0], key_dict(key)
        n += 1
        L = k["linear"]
        kw = dict(seed=100 + n, interp="nearest" if L == 0 else "linear")
        if f in STORE_FAMILIES:
            if k.get("vec", 1):
                ox = 64
            elif L == 2:
                ox, kw["align"] = 64, 1                     # ox % 4 == 0, dst 4 bytes past a 16-byte boundary
            else:
                ox = 70 if L == 0 else 5                    # the row tail
            if f == "warp_tps":
                ox = (70, 5, 64)[L]
            nx = 1 if L == 1 else {64: 60, 70: 70, 5: 5}[ox]
            fshape, mshape = (3, 5, ox), (4, 6, nx)
            if f == "compose":
                kw.update(mode=k["mode"], stats=k["stats"])
        elif f == "similarity":
            fshape, mshape = {0: ((4, 6, 70), (5, 6, 64)), 1: ((3, 5, 70), (4, 6, 1)), 2: ((4, 5, 64), (3, 6, 70))}[L]
            if L == 0 and k["field"]:
                fshape, mshape = (3, 5, 5), (4, 6, 1)       # nearest on a moving grid with nx == 1
            kw.update(field=k["field"], bins=(7, 64)[n % 2])
        elif f == "ffd":
            fshape, mshape = ((5, 6, 70), (6, 5, 64)) if L == 2 else ((4, 6, 64), (5, 6, 1))
            kw.update(spacing=(7, 3, 2) if L == 2 else (5, 2, 3))
        else:
            fshape, mshape = ((5, 6, 70), (6, 5, 64)) if L == 2 else ((4, 6, 70), (5, 6, 1))
            kw.update(bins=(19, 4, 64)[n % 3])
        if k.get("masked"):
            kw.update(wf=True, wm=True)
        c = case(f, fshape, mshape, **kw)
        assert selection_key(f, c) == key, (key, c)
        out.append(c)
    return tuple(out)


MATRIX = _matrix()

# section 5: non-finite coordinates, which only a field can carry
NONFINITE = tuple(c._replace(nonfinite=True) for c in MATRIX
                  if c.family in ("warp_field", "compose") or (c.family == "similarity" and c.field))

# ---- seeded cases, stratified by key -----------------------------------------------------------------------------------
XS = (1, 2, 3, 4, 5, 7, 8, 9, 16, 60, 63, 64, 65, 68, 70, 127, 128, 129, 133)


def _draw(family, key, rng, seed):
    k = key_dict(key)
    L = k["linear"]
    xs = np.array(XS)
    if "vec" in k:
        quad = xs[xs % 4 == 0]
        if k["vec"]:
            ox, align = int(rng.choice(quad)), 0
        elif rng.random() < 0.5:
            ox, align = int(rng.choice(quad)), 1            # the scalar stores of a row that is a multiple of 4 long
        else:
            ox, align = int(rng.choice(xs[xs % 4 != 0])), int(rng.integers(0, 2))
    else:
        ox, align = int(rng.choice(xs)), int(rng.integers(0, 2))
    oy, oz = int(rng.integers(1, 10)), int(rng.integers(1, 7))
    if L == 1 or (L == 0 and rng.random() < 0.25):
        nx = 1
    else:
        nx = int(np.clip(ox + rng.integers(-3, 4), 2, 133))
    ny = int(np.clip(oy + rng.integers(-2, 3), 1, 9))
    nz = int(np.clip(oz + rng.integers(-2, 3), 1, 6))
    wf, wm = ((True, False), (False, True), (True, True))[int(rng.integers(0, 3))] if k.get("masked") else (False, False)
    bins = int(rng.choice((2, 7, 50, 64, 128) if family == "similarity" else (4, 19, 64)))
    field = k.get("field", bool(rng.integers(0, 2)))
    c = case(family, (oz, oy, ox), (nz, ny, nx), "nearest" if L == 0 else "linear", field, wf, wm, bins, align,
             k.get("mode", "compose"), k.get("stats", False), tuple(int(v) for v in rng.integers(1, 9, 3)), seed)
    assert selection_key(family, c) == key, (key, c)
    return c


def fuzz_cases(family, seed, n):
    """n cases of a family: the keys in turn, seed s starting where seed s - 1 stopped (so two seeds of 24 give each of
    compose's 16 keys 3 cases), the rest drawn"""
    rng = np.random.default_rng([int(seed), FAMILIES.index(family), 77])
    keys = sorted((k for k in ALL_KEYS if k[0] == family), key=repr)
    return [_draw(family, keys[(int(seed) * n + i) % len(keys)], rng, int(seed) * 1000 + i) for i in range(n)]


# ---- a case's arrays -------------------------------------------------------------------------------------------------
def _grid(shape):
    z, y, x = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    return x, y, z


def build(c, content=None):
    """The arrays of a case (numpy): F, M, A, WF, WM (None where absent) and, by family, field, u / v, lattice, tps.
    content: a generator (shape, seed) -> float32 volume (tests/registration_content.py) whose output replaces F, M and
    the src made from M; everything else is drawn as without it, from the same seeded stream."""
    rng = np.random.default_rng([c.seed, FAMILIES.index(c.family), 5])
    d = types.SimpleNamespace()
    d.F, d.M = volumes(c.fshape, c.mshape, c.seed)
    if content is not None:
        d.F, d.M = (np.ascontiguousarray(content(s, c.seed + k), F32) for k, s in enumerate((c.fshape, c.mshape)))
        assert d.F.shape == c.fshape and d.M.shape == c.mshape
    one = [n == 1 for n in c.mshape[::-1]]                  # moving axes (x, y, z) of length 1
    axis = rng.standard_normal(3)
    lin = rot(axis, float(rng.uniform(-8.0, 8.0))) * rng.uniform(0.9, 1.1, 3)[None, :]
    shift = [float(rng.uniform(-1.0, 1.0)) * min(1.5, 0.3 * (n - 1)) for n in c.mshape[::-1]]
    d.A = about_center(lin, c.mshape, c.fshape, shift)
    for ax in range(3):
        if one[ax]:
            d.A[ax, :] = 0.0
    d.WF = (rng.random(c.fshape) < 0.75).astype(F32) if c.wf else None
    d.WM = (rng.random(c.mshape) < 0.75).astype(F32) if c.wm else None
    x, y, z = _grid(c.fshape)
    needs_field = c.family in ("warp_field", "compose") or (c.family == "similarity" and c.field)
    if needs_field:
        fld = (fr.ref_affine_field(d.A, c.fshape) + rng.normal(0, 0.3, (3,) + c.fshape)).astype(F32)
        for ax, p in enumerate((x, y, z)):
            if one[ax]:
                fld[ax] = -p.astype(F32)
        if c.nonfinite:
            flat = fld.reshape(3, -1)
            at = rng.choice(flat.shape[1], min(10, flat.shape[1]), replace=False)
            bad = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], F32)
            flat[rng.integers(0, 3, at.size), at] = bad[np.arange(at.size) % 5]
        d.field = fld
    if c.family == "compose":
        d.u = rng.normal(0, 1.5, (3,) + c.mshape).astype(F32)
        d.v = d.field
    if c.family == "warp_field":
        d.src = np.stack([d.M, (d.M * F32(-0.5)).astype(F32)]) if c.seed % 2 else d.M
    if c.family == "warp_tps":
        m = 5
        ctrl = rng.uniform(0, 1, (m, 3)) * (np.array(c.fshape[::-1]) - 1)
        w = rng.normal(0, 0.01, (m, 3))
        w[:, one] = 0.0
        d.tps = TPS(ctrl, w, d.A)
    if c.family == "ffd":
        d.lattice = rng.uniform(-1.0, 1.0, ffr.lattice_shape(c.fshape, c.spacing)).astype(F32)
        for ax in range(3):
            if one[ax]:
                d.lattice[ax] = 0.0
    return d


def counted(c, d=None):
    """(n, voxels): how many output voxels the restatements count in (inside the moving grid and in both masks)"""
    d = build(c) if d is None else d
    x, y, z = _grid(c.fshape)
    if c.family == "warp_tps":
        q = ref_tps_coords(d.tps, x, y, z)
    elif c.family == "ffd":
        q = mr.coords(ffr.field(d.lattice, c.spacing, c.fshape, d.A), c.fshape)
    elif hasattr(d, "field"):
        q = mr.coords(d.field, c.fshape)
    else:
        q = mr.coords(d.A, c.fshape)
    return int(mr.counted(q, c.mshape, d.WF, d.WM).sum()), int(np.prod(c.fshape))
