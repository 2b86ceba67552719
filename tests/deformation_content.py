"""Hostile content for the deformation stack: what tests/test_deformation_content*.py feed the FFD lattice kernels, the
sampling-core kernels that arrived after tests/sampling_cases.py's matrix, and the field kernels, instead of noise of
order 1.  Seeded, numpy only, no device.

tests/registration_content.py flushes "every intensity ... (the coordinates, masks and lattice as they are)"; here the
class goes into what that file left alone: the control lattice (section A), the displacement field (section C), and
into the intensities of the kernels that its families do not reach (section B).  The classes are
tests/pyramid_content.py's as they are (through registration_content.content, which gives a small `fade` its
subnormal corner), plus two purpose-built inputs:

  root_tiny   base * 2**-60, formed as `fade` forms its values: a product of two samples (e g_d, the FFD force)
              underflows float but not double, so that the gradient's double sums are of order 2**-120 and its
              (float) cast rounds into the subnormal range
  collapsed   a field whose x channel is exactly -x and whose y and z channels are integers that depend on y and z
              only: j_00 = 1 + (-1) = +0 and j_01 = j_02 = j_10 = j_20 = +0, so that every term of the cofactor
              expansion is a zero whose sign is that of its other factor, and every determinant is +0.0 or -0.0

The module holds what the GPU file and its CPU twin must agree on: the arrays of every case, the references (the
existing restatements, each callable with flush=True: every float input and every float output of a kernel flushed, as
pyramid_content.ftz models it) and, where a contract says "unfused", a model of the fused form."""
import types

import numpy as np

from tests import ffd_restatement as fr
from tests import field_algebra_restatement as fa
from tests import pyramid_content as pc
from tests import registration_content as rc
from tests import sampling_cases as sc
from tests.test_ffd_landmarks import point_pool

F = np.float32
CLASSES = rc.CLASSES
UNDERFLOW_CLASSES = rc.UNDERFLOW_CLASSES
FUSED_CLASSES = ("huge", "integer", "constant")       # where a fused multiply-add shows (the sums are off the grid)
FIELD_CLASSES = CLASSES + ("collapsed",)
ftz = pc.ftz

FIXED, MOVING, SPACING = rc.FIXED, rc.MOVING, (7, 3, 2)
FIXED_ODD, SPACING_ODD = rc.FIXED_ODD, (8, 3, 2)
MOVING_NX1 = (6, 5, 1)                                # LINEAR == 1
GRIDS = ((FIXED, SPACING), (FIXED_ODD, SPACING_ODD))
SEED = 20261021
QUIET = dict(invalid="ignore", over="ignore", under="ignore", divide="ignore")


def _seed(cls, k=0):
    return SEED % 100000 + 1000 * k + FIELD_CLASSES.index(cls)


def _f(flush):
    return ftz if flush else (lambda a: a)


# ----------------------------------------------------------------------------------------------------------------------
# A. the lattice as content
# ----------------------------------------------------------------------------------------------------------------------
def lattice(cls, shape, spacing, k=0):
    """the control lattice [3, gz, gy, gx] over a grid, one volume of the class per channel"""
    return rc.stack(fr.lattice_shape(shape, spacing), cls, _seed(cls, k))


def order1_lattice(shape, spacing, k=0, amplitude=1.0):
    rng = np.random.default_rng([SEED, 11, k])
    return rng.uniform(-amplitude, amplitude, fr.lattice_shape(shape, spacing)).astype(F)


def identity_x_affine(shape):
    """a pull map whose x row is the exact identity row, so that (float)(q_x - x) is +0.0 and the x channel of the field
    is the spline alone (the class survives); the y and z rows are a rotation of 3 degrees about the x axis through the
    grid's centre, with a shift"""
    oz, oy, _ = shape
    a = np.deg2rad(3.0)
    cy, cz = 0.5 * (oy - 1), 0.5 * (oz - 1)
    A = np.zeros((3, 4))
    A[0] = [1.0, 0.0, 0.0, 0.0]
    A[1] = [0.0, np.cos(a), -np.sin(a), cy - (np.cos(a) * cy - np.sin(a) * cz) + 0.25]
    A[2] = [0.0, np.sin(a), np.cos(a), cz - (np.sin(a) * cy + np.cos(a) * cz) - 0.125]
    return A


def field_reference(lat, spacing, shape, A=None, flush=False):
    f = _f(flush)
    return f(fr.field(f(lat), spacing, shape, A))


def _fma(a, b, c):
    """float32 a * b + c with one rounding, modelled through float64: the product of two floats is exact there, the sum
    is rounded to double and then to float"""
    return (np.asarray(a, F).astype(np.float64) * np.asarray(b, F).astype(np.float64)
            + np.asarray(c, F).astype(np.float64)).astype(F)


def spline_fused(lat, spacing, shape):
    """ffd_restatement.spline with s = fma(wz, wy * (wx * c), s) in the place of s + wz * (wy * (wx * c))"""
    c = np.ascontiguousarray(lat, F)
    (ix, wx), (iy, wy), (iz, wz) = fr._axes(shape, spacing)
    s = np.zeros((3,) + tuple(shape), F)
    for cc in range(4):
        for b in range(4):
            for a in range(4):
                v = c[:, (iz + cc)[:, None, None], (iy + b)[None, :, None], (ix + a)[None, None, :]]
                t = (wy[:, b][None, :, None] * (wx[:, a][None, None, :] * v)).astype(F)
                s = _fma(np.broadcast_to(wz[:, cc][:, None, None], t.shape), t, s)
    return s


def _sub_axis_fused(c, ax, g_fine):
    c = np.moveaxis(c, ax, -1)
    out = np.zeros(c.shape[:-1] + (g_fine,), F)
    for j in range(g_fine):
        if j & 1:
            i = (j + 1) // 2
            out[..., j] = (_fma(np.full(c.shape[:-1], 6.0, F), c[..., i], c[..., i - 1]) + c[..., i + 1]) * F(0.125)
        else:
            i = j // 2
            out[..., j] = (c[..., i] + c[..., i + 1]) * F(0.5)
    return np.moveaxis(out, -1, ax)


def refine2_fused(coarse, shape, spacing):
    """ffd_restatement.refine2 with fma(6, v1, v0) + v2 in the place of (v0 + 6 v1) + v2"""
    c = np.ascontiguousarray(coarse, F)
    fine = fr.lattice_shape(shape, spacing)
    for ax in (3, 2, 1):
        c = _sub_axis_fused(c, ax, fine[ax])
    return (c * F(2.0)).astype(F)


def coarse_lattice(cls, shape, spacing):
    """the lattice over the grid half as fine as `shape`: what ffd_refine2 subdivides"""
    return lattice(cls, tuple((o + 1) // 2 for o in shape), spacing, 1)


def refine2_reference(coarse, shape, spacing, flush=False):
    f = _f(flush)
    return f(fr.refine2(f(coarse), shape, spacing))


def bending_reference(lat, spacing, flush=False):
    """(R, dR, sum |term| of R, of dR) of ffd_restatement.bending; flush: the lattice flushed (the sums are double)"""
    return fr.bending(_f(flush)(lat), spacing)


LANDMARKS = 300


def landmark_case(cls, shape, spacing):
    """(lattice of the class, P, Q, w): 300 points of tests/test_ffd_landmarks.py's pool (whole voxels, sub-voxel
    points, points beyond the support and the edge coordinates), Q = P + uniform(-3, 3), weights with zeros"""
    rng = np.random.default_rng([SEED, 12, FIELD_CLASSES.index(cls)])
    pool = point_pool(shape, spacing, 3)
    P = pool[rng.permutation(len(pool))[:LANDMARKS]]
    Q = rng.uniform(-3.0, 3.0, (LANDMARKS, 3)) + np.nan_to_num(P, nan=0.0, posinf=0.0, neginf=0.0)
    w = rng.uniform(0.0, 2.0, LANDMARKS)
    w[rng.integers(0, LANDMARKS, LANDMARKS // 5)] = 0.0
    return lattice(cls, shape, spacing, 2), P, Q, w


def root_tiny(shape, seed):
    """base * 2**-60, exact (a power of two), as pyramid_content.fade forms its values"""
    return (pc._base(shape, seed).astype(np.float64) * np.ldexp(1.0, -60)).astype(F)


BEND_TINY = 2.0 ** -125                               # weights that keep the terms beside (2 / n) Gc in its range
LANDMARK_TINY = 2.0 ** -124


def cast_case():
    """A5: root_tiny intensities on (FIXED, MOVING), a lattice of order 1 (no pull map) and 40 landmarks inside the
    grid.  (2 / n) Gc is of order 2**-120 / 2**-7: around the smallest normal float"""
    d = types.SimpleNamespace()
    d.F, d.M = root_tiny(FIXED, SEED % 1000 + 1), root_tiny(MOVING, SEED % 1000 + 2)
    d.lattice = order1_lattice(FIXED, SPACING, 5, 0.75)
    d.spacing = SPACING
    rng = np.random.default_rng([SEED, 13])
    d.P = rng.uniform(0.0, 1.0, (40, 3)) * (np.array(FIXED[::-1]) - 1.0)
    d.Q = d.P + rng.uniform(-2.0, 2.0, (40, 3))
    return d


def cast_reference(d):
    """(Record, dR, grad float32, gmax) of the restatement at bending BEND_TINY without landmarks or penalty"""
    rec, _ = fr.evaluate(d.F, d.M, d.lattice, d.spacing, None)
    dR = fr.bending(d.lattice, d.spacing)[1]
    g, gmax = fr.gradient(rec, dR, BEND_TINY)
    return rec, dR, g, gmax


# ----------------------------------------------------------------------------------------------------------------------
# B. the sampling-core kernels that arrived after the matrix: intensities of every class
# ----------------------------------------------------------------------------------------------------------------------
BINS = 19


def hist_field_case(cls, nx1, masked):
    """B1: sampling_cases' similarity-through-a-field construction (nx == 1: the field's x channel is -p)"""
    c = sc.case("similarity", FIXED, MOVING_NX1 if nx1 else MOVING, field=True, wf=masked, wm=masked, bins=BINS,
                seed=40 + 2 * nx1 + masked)
    assert sc.selection_key("similarity", c)[1:] == (1 if nx1 else 2, True, masked)
    return c, rc.matrix_data(c, cls)


def mi_case(cls, nx1, masked):
    """B2: sampling_cases' ffd construction (nx == 1: the lattice's x channel and A's x row are zero), intensities of
    the class, the lattice of order 1"""
    fshape, mshape, spacing = ((4, 6, 64), (5, 6, 1), (5, 2, 3)) if nx1 else (FIXED, MOVING, SPACING)
    c = sc.case("ffd", fshape, mshape, wf=masked, wm=masked, spacing=spacing, bins=BINS, seed=60 + 2 * nx1 + masked)
    assert sc.selection_key("ffd", c) == ("ffd", 1 if nx1 else 2, masked)
    return c, rc.matrix_data(c, cls)


def channels_case(cls, linear, masked, nc=2):
    """B3: tests/test_ffd_channels.py's test_every_instantiation with stacks of the class"""
    from tests.test_ffd_channels import masks
    mshape = MOVING_NX1 if linear == 1 else MOVING
    d = types.SimpleNamespace(spacing=SPACING)
    d.F = rc.stack((nc,) + FIXED, cls, _seed(cls, 3))
    d.M = rc.stack((nc,) + mshape, cls, _seed(cls, 4))
    d.lattice = order1_lattice(FIXED, SPACING, 6 + linear)
    d.A = np.eye(3, 4)
    d.A[:, 3] = [0.4, -0.3, 0.6]
    if linear == 1:
        d.A[0] = 0.0
        d.lattice[0] = 0.0
    d.WF, d.WM = masks(FIXED, mshape, 7 + linear) if masked else (None, None)
    return d


def batch_maps(fshape, mshape):
    """B4: K = 3 pull maps: the identity, a rotation about the centres, one wholly outside (on a moving grid with
    nx == 1 the x row of each is zero: the coordinate is exactly 0)"""
    from tests.test_warp import about_center, rot
    out = np.eye(3, 4)
    out[1, 3] = mshape[1] + 5.0
    A = [np.eye(3, 4), about_center(rot((1, 2, 3), 7.0), mshape, fshape, shift=(0.3, -0.2, 0.1)), out]
    if mshape[2] == 1:
        for a in A:
            a[0] = 0.0
    return np.array(A)


def batch_case(cls, nx1, masked):
    mshape = MOVING_NX1 if nx1 else MOVING
    rng = np.random.default_rng([SEED, 14, int(nx1)])
    d = types.SimpleNamespace()
    d.F, d.M = rc.content(FIXED, cls, _seed(cls, 5)), rc.content(mshape, cls, _seed(cls, 6))
    d.A = batch_maps(FIXED, mshape)
    d.WF = (rng.random(FIXED) < 0.75).astype(F) if masked else None
    d.WM = (rng.random(mshape) < 0.75).astype(F) if masked else None
    return d


# ----------------------------------------------------------------------------------------------------------------------
# C. fields as content
# ----------------------------------------------------------------------------------------------------------------------
def collapsed(shape, seed):
    oz, oy, ox = shape
    u = np.empty((3,) + tuple(shape), F)
    u[0] = -np.arange(ox, dtype=F)[None, None, :]
    u[1] = rc.content((oz, oy, 1), "integer", seed)
    u[2] = rc.content((oz, oy, 1), "integer", seed + 1)
    return u


def field_of(cls, shape, k=0):
    """a displacement field [3, oz, oy, ox] whose three channels are of the class (or `collapsed`)"""
    if cls == "collapsed":
        return collapsed(shape, _seed(cls, 7 + k))
    return rc.stack((3,) + tuple(shape), cls, _seed(cls, 7 + k))


def exp_reference(v, K, flush=False):
    """field_algebra_restatement.ref_exp; flush: v, the scaled field and every composition's output flushed"""
    if not flush:
        return fa.ref_exp(v, K)
    v = ftz(v)
    if K == 0:
        return v.copy()
    w = ftz((v * F(2.0 ** -K)).astype(F))
    for _ in range(K):
        w = ftz(fa.ref_compose(w, w)[0])
    return w


INVERT_STEPS = 2


def invert_reference(u, flush=False):
    """w_N of field_algebra_restatement.ref_invert from a zero start; flush: u and every iterate flushed"""
    w = np.zeros_like(u)
    if not flush:
        return fa.ref_invert(u, w, INVERT_STEPS)[0]
    u = ftz(u)
    for _ in range(INVERT_STEPS):
        w = ftz(fa.ref_compose(u, w, "invert")[0])
    return w
