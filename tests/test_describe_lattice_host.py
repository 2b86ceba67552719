"""Host: the gradient fold considered for k_describe's lattice variant, restated in numpy float32.

(The fold was built, measured no gain on the MI355X and was taken out again -- DESIGN.md 3.3; this restatement
stays as the record of where the two forms agree, should a later design want it.)

The kernel scales a sample difference d three times, g = fl(fl(fl(0.5 * d) * iu) * w) (IM_GET_GRAD_ISO, the
level's inverse unit, the Gaussian weight); the lattice variant, whose iu is a power of two, could form s = fl(fl(0.5
* iu) * w) once per voxel and g = fl(d * s) per component.  The two are the same float wherever every scaling by a
power of two is exact, i.e. everywhere but where an intermediate is subnormal -- and there the weighted squared
magnitude m2 is far below the 1.1920928955078125e-06 threshold of sift.c:1264, so the voxel contributes nothing
in either form.  Asserted over 10^6 random sample pairs per octave unit 1, 2, 4, 8 and over a sweep of
differences down through the subnormal range.
"""
import numpy as np
import pytest

F = np.float32
THRESH = F(1.1920928955078125e-06)
UNITS = (1.0, 2.0, 4.0, 8.0)


def three_step(d, iu, w):
    g = F(0.5) * d
    g = g * iu
    return g * w


def folded(d, iu, w):
    s = (F(0.5) * iu) * w
    return d * s


def m2_of(g):
    return g[0] * g[0] + g[1] * g[1] + g[2] * g[2]


def check(d, w, unit):
    """d: (3, n) float32 sample differences, w: (n,) weights.  Returns the number of voxels whose forms differ."""
    iu = F(1.0) / F(unit)
    with np.errstate(under="ignore"):
        a, b = three_step(d, iu, w), folded(d, iu, w)
        differ = (a != b).any(axis=0)
        ma, mb = m2_of(a), m2_of(b)
    assert a.dtype == F and b.dtype == F
    assert (ma[differ] < THRESH).all() and (mb[differ] < THRESH).all(), \
        (unit, float(ma[differ].max()), float(mb[differ].max()))
    # (and nothing else about such a voxel depends on the gradient: the magnitude is forced to 0)
    return int(differ.sum())


@pytest.mark.parametrize("unit", UNITS)
def test_random_sample_pairs_fold_exactly(unit):
    rng = np.random.default_rng(int(unit))
    n = 1000000
    # samples of a pyramid of an image scaled to [0, 1]; weights of window voxels, exp(-2) <= w <= 1
    p, q = rng.random((3, n), dtype=F), rng.random((3, n), dtype=F)
    w = np.exp(-2.0 * rng.random(n)).astype(F)
    assert check(p - q, w, unit) == 0


@pytest.mark.parametrize("unit", UNITS)
def test_differences_down_through_the_subnormal_range(unit):
    rng = np.random.default_rng(100 + int(unit))
    differing = 0
    for e in range(-90, -150, -1):
        n = 4096
        mant = (1.0 + rng.random((3, n))) * rng.choice([-1.0, 1.0], (3, n))
        with np.errstate(under="ignore"):
            d = np.ldexp(mant, e).astype(F)
        w = np.exp(-2.0 * rng.random(n)).astype(F)
        k = check(d, w, unit)
        if e > -118:                    # |g| >= 2^-118 * 0.5 / 8 * exp(-2) > 2^-126
            assert k == 0, (e, k)       # every intermediate is a normal number: the forms agree
        differing += k
    assert differing > 0                # the sweep does reach the inputs on which they differ
