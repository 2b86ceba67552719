"""Hostile content for the registration stack: what tests/test_registration_content*.py feed the sampling core, the
B-spline prefilter, the demons force and update, the grid transfers, the Lie bracket, the histograms and the moments
instead of noise of order 1.  Seeded, numpy only, no device.

The classes are tests/pyramid_content.py's, as they are: subnormal, fade, faint_spikes, huge, integer, constant.  The
volumes must be finite: every one of these entries says so in its contract (include/sift3d_amd.h), so non-finite
intensities are not a class here and nothing is pinned on them.  (Non-finite *coordinates* are tests/sampling_cases.py's
NONFINITE cases.)

The module holds what the GPU file and its CPU twin must agree on: the content of a (shape, class, seed), the range of
the histogram entries per class, the arrays of every case of sampling_cases.MATRIX on a class, the cases of the kernels
outside that matrix with their references (the existing restatements, called with or without a modelled flush), and the
helpers for the flush share and the NaN-tolerant word compare.

Ranges (range_of): the histogram entries bin t = (v - lo) * s with s = (float) B / (hi - lo) in float.
  subnormal, faint_spikes, fade   (-(B // 2) * 2**-126, (B - B // 2) * 2**-126), a function of the bin count B: bins of
                                  2**-126, the narrowest whose scale s = 2**126 is exact and finite, with 0.0 on the edge
                                  between bin B // 2 - 1 and bin B // 2 for odd counts as for even ones.  A negative
                                  subnormal (of 2**-144 or more: v - lo is a float sum) falls in bin B // 2 - 1, a
                                  positive one and both zeros in bin B // 2, so a flush moves the negative samples into
                                  the other bin; fade's normal part clamps into the end bins.  A sample of 2**-140 is
                                  2**-14 of a bin, four units of the Parzen window's fixed point (2**-16), so a flush
                                  also changes the window's weights of most moving samples, and the table W is not 0.
                                  (The range first proposed for these classes, (-2**-120, 2**-120) for every B, has 0.0
                                  inside the middle bin of an odd count, where a flush moves nothing, and bins 2**20
                                  times the content, where every moving sample has the same Parzen weights, the table W
                                  is 0 and mi's sums with it: it could not fail in those cases, so it was replaced.)
  huge                            (-2**102, 2**102)
  integer                         (-300, 300)
  constant                        (0, 1)
The range that is natural for `subnormal`, its own min and max, is about 1e-41 wide: B / (hi - lo) overflows float and
the entries must refuse it (natural_range)."""
import types

import numpy as np

from tests import affine_init_restatement as ai
from tests import bspline_restatement as br
from tests import demons_mask_restatement as dk
from tests import field_algebra_restatement as fa
from tests import field_restatement as fr
from tests import logdemons_restatement as lg
from tests import multires_restatement as mu
from tests import pyramid_content as pc
from tests import sampling_cases as sc
from tests.test_warp import about_center, ref_warp, rot
from tests.tps_restatement import ref_tps_warp

F = np.float32
CLASSES = tuple(pc.CLASSES)
UNDERFLOW_CLASSES = pc.UNDERFLOW_CLASSES
is_subnormal, ftz, bits = pc.is_subnormal, pc.ftz, pc.bits

RANGE = dict(huge=(-2.0 ** 102, 2.0 ** 102), integer=(-300.0, 300.0), constant=(0.0, 1.0))
BIN = 2.0 ** -126                          # the underflow classes' bin width: s = B / (B * 2**-126) = 2**126 exactly


def range_of(cls, bins):
    """(lo, hi) of the histogram entries for a class and a bin count (the module docstring's table)"""
    if cls in UNDERFLOW_CLASSES:
        return -(bins // 2) * BIN, (bins - bins // 2) * BIN
    return RANGE[cls]


def content(shape, cls, seed):
    """The class's volume of a 3-D shape.  pyramid_content.fade starts at 2**-110 in the corner of the origin and is
    subnormal from x + y + z = 16 on, which a volume with a one-voxel axis ((4, 6, 1): x + y + z <= 8) never reaches:
    such a volume is the far corner of fade on a grid 5 longer on every axis (x + y + z from 15: one normal corner)."""
    shape = tuple(int(n) for n in shape)
    if cls == "fade" and sum(n - 1 for n in shape) < 24:
        v = pc.fade(tuple(n + 5 for n in shape), seed)[5:, 5:, 5:]
    else:
        v = pc.CLASSES[cls](shape, seed)
    v = np.ascontiguousarray(v, F)
    assert v.shape == shape and np.isfinite(v).all()
    return v


def stack(shape, cls, seed):
    """[n, nz, ny, nx] of the class: one volume per channel, seeds seed, seed + 1, ..."""
    return np.stack([content(shape[1:], cls, seed + k) for k in range(shape[0])])


def generator(cls):
    return lambda shape, seed: content(shape, cls, seed)


def natural_range(v):
    return float(v.min()), float(v.max())


def share(mask, of=None):
    """the share of `mask` among all words, or among the words `of`"""
    mask = np.asarray(mask, bool)
    if of is None:
        return float(np.count_nonzero(mask)) / max(mask.size, 1)
    return float(np.count_nonzero(mask & of)) / max(int(np.count_nonzero(of)), 1)


def underflow_shares(want, flushed):
    """(share of the nonzero reference words that are subnormal, share of them that the flushed run changes)"""
    want, flushed = np.asarray(want, F), np.asarray(flushed, F)
    of = want != 0
    return share(is_subnormal(want), of), share(bits(want) != bits(flushed), of)


def same_words(got, want):
    """None where got and want agree word for word (-0.0 is not +0.0), a NaN of any payload matching a NaN; else a
    description of the first difference"""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    if got.shape != want.shape:
        return "shape %r, not %r" % (got.shape, want.shape)
    bad = (bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))
    if not bad.any():
        return None
    i = tuple(int(v[0]) for v in np.nonzero(bad))
    return "%d of %d words differ, first at %r: got %r (0x%08x), want %r (0x%08x)" \
        % (int(bad.sum()), bad.size, i, got[i], bits(got)[i], want[i], bits(want)[i])


# ----------------------------------------------------------------------------------------------------------------------
# a. the sampling core: every case of sampling_cases.MATRIX on every class
# ----------------------------------------------------------------------------------------------------------------------
def matrix_data(c, cls):
    """build(c) with F, M (and the src made from M) of the class.  compose: the class goes into u, the field that is
    sampled (one volume per channel), and v is built so that the sum does not swallow it: its x channel is
    0.5 + ((x % 3) - 1), its y and z channels are zero, so that the output's y and z channels are the interpolated u;
    on a moving axis of length 1 the channel stays build()'s -p (the coordinate is exactly 0)."""
    d = sc.build(c, generator(cls))
    if c.family == "compose":
        d.u = stack((3,) + c.mshape, cls, c.seed + 10)
        x, y, z = sc._grid(c.fshape)
        v = np.zeros((3,) + c.fshape, F)
        v[0] = (0.5 + ((x % 3) - 1)).astype(F)
        for ax, p in enumerate((x, y, z)):
            if c.mshape[2 - ax] == 1:
                v[ax] = -p.astype(F)
        d.v = d.field = v
    return d


def flushed_data(d):
    """d with every intensity flushed (the coordinates, masks and lattice as they are)"""
    e = types.SimpleNamespace(**vars(d))
    for name in ("F", "M", "src", "u"):
        if hasattr(d, name):
            setattr(e, name, ftz(getattr(d, name)))
    return e


def store_reference(c, d):
    """what run_store compares a store family's output with"""
    if c.family == "warp_affine":
        return ref_warp(d.M, d.A, c.fshape, c.interp, sc.FILL)[0]
    if c.family == "warp_tps":
        return ref_tps_warp(d.M, d.tps, c.fshape, c.interp, sc.FILL)[0]
    if c.family == "warp_field":
        return fr.ref_warp_field(d.src, d.field, c.interp, sc.FILL)
    return fa.ref_compose(d.u, d.v, c.mode)[0]


def unfilled(c, d, want):
    """the words of a store reference that are samples (not the fill of a voxel that samples outside; for the
    composition its y and z channels, which are the interpolated u)"""
    want = np.asarray(want, F)
    if c.family == "compose":
        keep = np.zeros(want.shape, bool)
        keep[1:] = True
        for ax in (1, 2):
            if c.mshape[2 - ax] == 1:
                keep[ax] = False
        return keep
    return bits(want) != bits(F(sc.FILL))


# ----------------------------------------------------------------------------------------------------------------------
# b. the kernels outside that matrix
# ----------------------------------------------------------------------------------------------------------------------
PREFILTER_SHAPE = (35, 34, 70)            # x pass: tiles of 64; y / z pass: 32 outputs; halo 16 mirrored samples: one
BSPLINE_OUT = (5, 6, 70)                  # tile and a tail on every axis
FIXED, MOVING = (5, 6, 70), (6, 5, 64)    # the demons force and iteration
FIXED_ODD = (5, 7, 67)                    # 3 * 5 * 7 * 67 % 4 == 3: the scalar tail of k_field_add behind its quads
TRANSFER_SHAPES = ((5, 6, 70), (4, 6, 64))                                  # odd and even extents
SEED = 20261021


def _seed(cls, k=0):
    return SEED % 100000 + 100 * k + CLASSES.index(cls)


def bspline_case(cls):
    """(volume, A, field): a rotation about the centre onto BSPLINE_OUT, and its field with normal(0, 0.3) noise"""
    rng = np.random.default_rng([SEED, 1])
    vol = content(PREFILTER_SHAPE, cls, _seed(cls, 1))
    A = about_center(rot(np.array([0.3, -0.5, 0.8]), 9.0), PREFILTER_SHAPE, BSPLINE_OUT, (0.4, -0.3, 0.2))
    field = (fr.ref_affine_field(A, BSPLINE_OUT) + rng.normal(0, 0.3, (3,) + BSPLINE_OUT)).astype(F)
    return vol, A, field


def bspline_reference(vol, A, field, flush=False):
    """(coefficients, affine warp, field warp) by bspline_restatement; flush: every input and output flushed"""
    f = ftz if flush else (lambda a: a)
    coef = f(br.prefilter(f(vol)))
    return coef, f(br.warp_affine(coef, A, BSPLINE_OUT, 0.0)), f(br.warp_field(coef, field, 0.0))


def force_case(cls, nc, masked, fixed=FIXED):
    """(F [nc, fixed], M [nc, MOVING], u, W = the reference warp of M through u, WF, WM)"""
    rng = np.random.default_rng([SEED, 2, nc, int(masked)])
    Fv = stack((nc,) + fixed, cls, _seed(cls, 2))
    M = stack((nc,) + MOVING, cls, _seed(cls, 3))
    u = rng.normal(0, 0.7, (3,) + fixed).astype(F)
    WF = (rng.random(fixed) < 0.75).astype(F) if masked else None
    WM = (rng.random(MOVING) < 0.75).astype(F) if masked else None
    return Fv, M, u, fr.ref_warp_field(M, u, "linear", 0.0), WF, WM


def force_reference(Fv, W, u, WF, WM, flush=False):
    """(delta, s_d, counted) of demons_mask_restatement.ref_force (with no masks: demons_restatement's arithmetic), alpha
    1.0; flush: F and W flushed"""
    f = ftz if flush else (lambda a: a)
    return dk.ref_force(f(Fv), f(W), u, MOVING, 1.0, WF, WM)


def to_subnormal(a):
    """a times the power of two that puts max |a| into [2**-131, 2**-130) (exact but for the bits that fall off the
    subnormal grid)"""
    a = np.asarray(a, np.float64)
    e = -130 - int(np.floor(np.log2(np.abs(a).max()))) - 1
    return np.ldexp(a, e).astype(F)


def demons_start(cls, fixed):
    """the iteration's starting field: class content scaled into the subnormal range in its x and y channels, normal(0,
    0.3) in z"""
    rng = np.random.default_rng([SEED, 3])
    u = np.empty((3,) + fixed, F)
    u[0] = to_subnormal(content(fixed, cls, _seed(cls, 4)))
    u[1] = to_subnormal(content(fixed, cls, _seed(cls, 5)))
    u[2] = rng.normal(0, 0.3, fixed).astype(F)
    return u


def demons_reference(Fv, M, u0, WF=None, WM=None):
    """one iteration, both sigmas 0, alpha 1.0: the field after it and [(s_d, counted)]"""
    return dk.ref_demons(Fv, M, u0, 1, 1.0, 0.0, 0.0, None, WF, WM)


def transfer_reference(cls, shape, flush=False):
    """dict of the grid transfers of the class at a shape: restrict (scale 1.0), restrict_half (scale 0.5, of a 3-channel
    stack) and prolong (a coarse field of the class onto the shape), with their inputs"""
    f = ftz if flush else (lambda a: a)
    vol = content(shape, cls, _seed(cls, 6))
    fld = stack((3,) + shape, cls, _seed(cls, 7))
    coarse = stack((3,) + mu.half_shape(shape), cls, _seed(cls, 8))
    return dict(vol=vol, fld=fld, coarse=coarse, restrict=f(mu.ref_restrict(f(vol), 1.0)),
                restrict_half=f(mu.ref_restrict(f(fld), 0.5)), prolong=f(mu.ref_prolong(f(coarse), shape)))


def bracket_case(cls):
    """(a of the class, b normal noise), 3 x FIXED"""
    rng = np.random.default_rng([SEED, 4])
    return stack((3,) + FIXED, cls, _seed(cls, 9)), rng.normal(0, 1, (3,) + FIXED).astype(F)


def bracket_reference(a, b, mode, flush=False):
    f = ftz if flush else (lambda v: v)
    return f(lg.ref_bracket(f(a), b, mode))


MOMENT_FLOORS = (0.0, 2.0 ** -126)


def moments_case(cls, floor):
    """(V, mask): V = floor + class (a float32 sum; the class itself for floor 0), FIXED"""
    rng = np.random.default_rng([SEED, 5])
    v = content(FIXED, cls, _seed(cls, 10))
    if floor:
        v = (F(floor) + v).astype(F)
    return v, (rng.random(FIXED) < 0.7).astype(F)


def moments_reference(V, floor, weight, mask, flush=False):
    """affine_init_restatement.moments; flush: V flushed and the float32 difference V - floor flushed (a flushed
    difference counts where the exact one does unless it is a subnormal)"""
    if not flush:
        return ai.moments(V, floor, weight, mask)
    w = ftz(ftz(V) - F(floor))                              # (both floors are normal or zero)
    return ai.moments(w, 0.0, weight, mask)


# ----------------------------------------------------------------------------------------------------------------------
# section 5: the volumes of api._own_range
# ----------------------------------------------------------------------------------------------------------------------
OWN_RANGE_SHAPE = (5, 6, 70)


def own_range_volumes():
    """name -> volume: what api.similarity must accept with its own ranges"""
    rng = np.random.default_rng([SEED, 6])
    k = rng.integers(0, 4, OWN_RANGE_SHAPE)
    return dict(constant_2p25=content(OWN_RANGE_SHAPE, "constant", 0) * F(2.0 ** 25),
                subnormal=content(OWN_RANGE_SHAPE, "subnormal", 1),
                one_plus_ulps=(F(1.0) + k.astype(F) * F(2.0 ** -23)).astype(F),
                tiny_span=(F(2e-38) + k.astype(F) * F(1e-38)).astype(F),      # normal values 1e-38 apart
                constant_big=np.full(OWN_RANGE_SHAPE, F(2.0 ** 25), F),        # lo + 1 rounds to lo
                constant=content(OWN_RANGE_SHAPE, "constant", 0))
