"""Affine refinement on the device (sift3d_hip_affine_normal_eqs, sift3d_amd_affine_refine_device; include/
sift3d_amd.h, "Intensity-driven affine refinement") against the numpy restatement (tests/affine_refine_restatement.py):
the count bit for bit; every sum exactly where every term is an integer multiple of 1/4, and otherwise to
gamma_(n + 8) sum |terms|: gamma_n bounds any order of summing n doubles (tests/demons_restatement.gamma; the
restatement's own sums are correctly rounded) and a term carries at most 8 roundings in whichever way it is factored
(header).  The driver against the restatement's driver on the cases of tests/test_affine_refine_host.py."""
import numpy as np
import pytest

from tests import affine_refine_restatement as ar
from tests.demons_restatement import gamma
from tests.test_affine_refine_host import TOL, bias_free_case, biased_case, check_descent
from tests.test_similarity import SHAPES, TILE, dev, transforms, volumes
from tests.test_similarity_host import end_to_end_case
from tests.test_warp import about_center, rot

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


def check(hip, F, M, A, what, exact=False):
    """one call against the restatement.  Returns (n, S_ee, b, H)."""
    n, see, b, H = hip.affine_normal_equations(dev(F), dev(M), A)
    want = ar.normal_equations(F, M, A)
    assert n == want.n, (what, n, want.n)
    assert np.array_equal(H, H.T), what                                      # symmetric bit for bit
    g = 0.0 if exact else gamma(n + 8)
    assert abs(see - want.see) <= g * want.see_terms, (what, "S_ee", see, want.see)
    db, dH = np.abs(b - want.b), np.abs(H - want.H)
    assert np.all(db <= g * want.b_terms), (what, "b", db.max(), (db - g * want.b_terms).max())
    assert np.all(dH <= g * want.H_terms), (what, "H", dH.max(), (dH - g * want.H_terms).max())
    return n, see, b, H


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_normal_equations_shapes_and_transforms(hip, k):
    fshape, mshape = SHAPES[k]
    F, M = volumes(fshape, mshape, 10 + k)
    for name, A in transforms(fshape, mshape).items():
        what = "%s -> %s %s" % (fshape, mshape, name)
        n, see, b, H = check(hip, F, M, A, what)
        if name == "outside":
            assert n == 0 and see == 0.0 and not b.any() and not H.any(), what
            raw = hip.affine_normal_equations(dev(F), dev(M), A, raw=True)
            assert not raw.cpu().numpy().any(), what                         # an all-zero record


def test_integer_content_gives_exact_sums(hip):
    """integer-valued volumes under an integer shift: m, the gradients and e are integers, the centred positions of
    an odd grid are integers (of an even one, halves), so every term is an integer multiple of 1/4 far below 2^53 and
    so is every partial sum and every factor of a term: any order and any factoring is exact"""
    rng = np.random.default_rng(4)
    for fshape, mshape in (((9, 21, 133), (11, 19, 140)), ((4, 6, 70), (5, 6, 72))):
        F = rng.integers(-30, 30, fshape).astype(np.float32)
        M = rng.integers(-30, 30, mshape).astype(np.float32)
        A = np.eye(3, 4)
        A[:, 3] = [5, -2, 1]
        n, see, b, H = check(hip, F, M, A, "integers %s" % (fshape,), exact=True)
        assert 0 < n < F.size and b.any() and np.all(np.diag(H) > 0)


def test_more_tiles_than_workgroups_and_calls_repeat(hip):
    """tests/test_similarity.test_more_tiles_than_workgroups' grid: a second, partial pass over the tiles.  Two calls
    return identical record bytes."""
    G = hip.SIMILARITY_GRID
    ty = int(np.ceil(np.sqrt(G + 1)))
    tz = -(-(G + 1) // ty)
    fshape = (TILE[0] * (tz - 1) + 1, TILE[1] * (ty - 1) + 1, 2)
    assert G < ty * tz < 2 * G
    F, M = volumes(fshape, (fshape[0] - 3, fshape[1] + 2, 3), 3)
    A = about_center(rot((1, 0, 0), 10.0), M.shape, fshape, shift=(0.2, 0, 0))
    check(hip, F, M, A, "grid cap")
    Fd, Md = dev(F), dev(M)
    r0 = hip.affine_normal_equations(Fd, Md, A, raw=True).cpu().numpy()
    r1 = hip.affine_normal_equations(Fd, Md, A, raw=True).cpu().numpy()
    assert np.array_equal(r0, r1)


def test_value_path_is_the_warp(hip):
    """S_ee of the record against the similarity record's sum d d on the same inputs: both square the float
    difference of f and the warp's m, so they agree to the bound on two orders of summing, and exactly on integers"""
    fshape, mshape = (9, 20, 133), (8, 21, 130)
    F, M = volumes(fshape, mshape, 16)
    A = transforms(fshape, mshape)["rotation"]
    n, see, _, _ = hip.affine_normal_equations(dev(F), dev(M), A)
    count, sums = hip.similarity_stats(hip.similarity(dev(F), dev(M), A, 64, (-1.0, 1.5), (-1.0, 1.5))[1])
    assert n == count > 0
    assert abs(see - sums[5]) <= 2 * gamma(n) * max(see, sums[5])
    rng = np.random.default_rng(5)
    Fi = rng.integers(-300, 300, fshape).astype(np.float32)
    Mi = rng.integers(-300, 300, mshape).astype(np.float32)
    S = np.eye(3, 4)
    S[:, 3] = [3, -2, 1]
    n, see, _, _ = hip.affine_normal_equations(dev(Fi), dev(Mi), S)
    count, sums = hip.similarity_stats(hip.similarity(dev(Fi), dev(Mi), S, 64, (-300.0, 300.0), (-300.0, 300.0))[1])
    assert n == count > 0 and see == sums[5]


def test_caller_buffers_and_value_errors(hip):
    import torch
    F, M = (dev(v) for v in volumes((5, 7, 9), (6, 5, 8), 8))
    rec = torch.full((158,), 7, dtype=torch.int64, device="cuda")
    work = torch.empty(hip.affine_normal_work_bytes(), dtype=torch.uint8, device="cuda")
    got = hip.affine_normal_equations(F, M, np.eye(3, 4), record=rec, work=work)
    want = hip.affine_normal_equations(F, M, np.eye(3, 4))
    assert got[0] == want[0] and got[1] == want[1] and np.array_equal(got[3], want[3])
    for bad in (lambda: hip.affine_normal_equations(F, M, np.eye(3)),
                lambda: hip.affine_normal_equations(F.cpu(), M, np.eye(3, 4)),
                lambda: hip.affine_normal_equations(F, M, np.eye(3, 4), record=rec[:100]),
                lambda: hip.affine_normal_equations(F, M, np.eye(3, 4), work=work[:100])):
        with pytest.raises(ValueError):
            bad()


# ---- the driver ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api():
    from sift3d_amd import api as a
    a.lib()
    return a


def test_driver_biased_case(api):
    """tests/test_affine_refine_host.test_driver_biased_case on the device: the same conditions, and the final map
    within 10 tol of the restatement driver's at the corners (both stop inside tol of the same minimum; the bits of
    the sums are the only difference)."""
    fixed, moving, T = biased_case(api)
    r = api.refine_affine(dev(moving), dev(fixed))
    ref = ar.refine(fixed, moving)
    check_descent(r, ar.corner_distance(np.eye(3, 4), T, fixed.shape), ar.corner_distance(r.A, T, fixed.shape))
    apart = ar.corner_distance(r.A, ref.A, fixed.shape)
    print("device\n", r.A, "\nrestatement\n", ref.A, "\n%.3g apart; evaluations %d and %d, stop %s and %s"
          % (apart, r.evaluations, ref.evaluations, r.stop, ref.stop))
    assert apart <= 10 * TOL
    assert r.level_slices == {0: slice(0, r.evaluations)} and len(r.msd) == r.evaluations
    from sift3d_amd import hip
    want = dev(np.zeros_like(fixed))
    hip.warp_affine(dev(moving), want, r.A, "linear")
    assert np.array_equal(r.warped.cpu().numpy(), want.cpu().numpy())
    last, sim = r.msd[r.accepted][-1], api.similarity(fixed, moving, r.A).msd     # two orders of one sum
    assert abs(last - sim) <= 2 * gamma(fixed.size) * max(last, sim)


def test_driver_bias_free_translation(api):
    fixed, moving, T = bias_free_case(api)
    r = api.refine_affine(dev(moving), dev(fixed), free="translation")
    ref = ar.refine(fixed, moving, free_mask=0x888)
    err, apart = ar.corner_distance(r.A, T, fixed.shape), ar.corner_distance(r.A, ref.A, fixed.shape)
    print("corner error %.3g after %d evaluations, stop %s; %.3g from the restatement's"
          % (err, r.evaluations, r.stop, apart))
    assert err <= 10 * TOL and apart <= 10 * TOL
    assert np.array_equal(r.A[:, :3], np.eye(3))                             # the linear part: bit-identical
    A0 = about_center(rot((1, 2, 3), 2.0), moving.shape, fixed.shape)
    r2 = api.refine_affine(dev(moving), dev(fixed), A0, free=0x888, max_evaluations=5)
    assert np.array_equal(r2.A[:, :3], A0[:, :3])


def test_driver_levels(api):
    fixed, moving, T = biased_case(api, 10.0, (8.0, -6.0, 4.0))
    one = api.refine_affine(dev(moving), dev(fixed))
    three = api.refine_affine(dev(moving), dev(fixed), levels=3)
    ref = ar.refine(fixed, moving, levels=3)
    apart = ar.corner_distance(one.A, three.A, fixed.shape)
    n1, n3 = int((one.levels == 0).sum()), int((three.levels == 0).sum())
    to_ref = ar.corner_distance(three.A, ref.A, fixed.shape)
    print("level-0 evaluations %d against %d, final maps %.3g apart; levels=3 %.3g from the restatement's"
          % (n3, n1, apart, to_ref))
    assert apart <= 10 * TOL and to_ref <= 10 * TOL
    assert n3 < n1
    assert list(three.level_slices) == [2, 1, 0]
    check_descent(three, ar.corner_distance(np.eye(3, 4), T, fixed.shape),
                  ar.corner_distance(three.A, T, fixed.shape))


def test_inputs_agree_and_value_errors(api):
    fixed, moving, T = biased_case(api)
    a = api.refine_affine(dev(moving), dev(fixed), max_evaluations=4)
    b = api.refine_affine(moving, api.Image.from_array(fixed), max_evaluations=4)
    c = api.refine_affine(api.Image.from_array(moving), fixed, np.eye(3, 4), max_evaluations=4)
    for other in (b, c):
        assert np.array_equal(a.A, other.A) and np.array_equal(a.msd, other.msd)
        assert np.array_equal(a.count, other.count) and a.stop == other.stop == "evaluations"
    small = api.refine_affine(moving[:40, :44], fixed, max_evaluations=3)       # A = None needs no equal shapes
    assert small.evaluations == 3 and small.warped.shape == fixed.shape
    for kw in (dict(free="rigid"), dict(free=0), dict(free=0x1000), dict(levels=0), dict(levels=7),
               dict(interp="nearest"), dict(A=np.eye(3)), dict(bogus=1)):
        with pytest.raises(ValueError):
            api.refine_affine(dev(moving), dev(fixed), **kw)
    with pytest.raises(RuntimeError):
        api.refine_affine(dev(moving), dev(fixed), lambda0=-1.0)              # the entry refuses


def test_register_refine(api):
    """refine=False is today's register, bit for bit (the same calls in the same order); refine=True ends at an MSD no
    larger than the RANSAC affine's, as api.similarity measures both."""
    import torch
    from sift3d_amd import hip
    fixed, T, Tinv = end_to_end_case(api)
    Fd = dev(fixed)
    Md = torch.empty_like(Fd)
    hip.warp_affine(Fd, Md, Tinv, "linear", 0.0)
    plain = api.register(Md, Fd)
    again = api.register(Md, Fd, refine=False)
    assert type(plain).__name__ == "Registration" and plain._fields == ("A", "inliers", "num_matches", "warped")
    assert np.array_equal(plain.A, again.A) and np.array_equal(plain.inliers, again.inliers)
    assert plain.num_matches == again.num_matches
    assert np.array_equal(plain.warped.cpu().numpy(), again.warped.cpu().numpy())
    want = torch.empty_like(Fd)
    hip.warp_affine(Md, want, api.affine_invert(plain.A), "linear")
    assert np.array_equal(plain.warped.cpu().numpy(), want.cpu().numpy())
    fine = api.register(Md, Fd, refine=True)
    assert np.array_equal(fine.A_ransac, plain.A) and np.array_equal(fine.inliers, plain.inliers)
    before = api.similarity(Fd, Md, api.affine_invert(plain.A)).msd
    after = api.similarity(Fd, Md, fine.refinement.A).msd
    print("msd: RANSAC %.6g, refined %.6g after %d evaluations (%s)"
          % (before, after, fine.refinement.evaluations, fine.refinement.stop))
    assert after <= before
    np.testing.assert_allclose(api.affine_invert(fine.A), fine.refinement.A, rtol=0, atol=1e-9)
