"""Affine refinement under a linear intensity map on the device (sift3d_hip_affine_ncc_normal_eqs,
sift3d_amd_affine_ncc_refine_device; include/sift3d_amd.h, "Affine refinement under a linear intensity map (NCC)")
against the numpy restatement (tests/affine_ncc_restatement.py): the count bit for bit; every one of the 101 sums
exactly where every term is an integer multiple of 1/4, and otherwise to gamma_(n + 8) sum |terms|, as
tests/test_affine_refine.py bounds the MSD record (gamma_n bounds any order of summing n doubles, the restatement's own
sums are correctly rounded, and a term carries at most 8 roundings in whichever way it is factored).  The driver against
the restatement's driver on the mapped pairs of tests/test_affine_ncc_host.py."""
import numpy as np
import pytest

from tests import affine_ncc_restatement as an
from tests import affine_refine_restatement as ar
from tests.demons_restatement import gamma
from tests.test_affine_ncc_host import mapped_case
from tests.test_affine_refine_host import TOL
from tests.test_similarity import SHAPES, TILE, dev, transforms, volumes
from tests.test_similarity_host import end_to_end_case
from tests.test_warp import about_center, rot

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


def check(hip, F, M, A, what, exact=False, WF=None, WM=None):
    """one call against the restatement.  Returns the device's record."""
    got = hip.affine_ncc_normal_equations(dev(F), dev(M), A, mask_fixed=None if WF is None else dev(WF),
                                          mask_moving=None if WM is None else dev(WM))
    want = an.record(F, M, A, WF, WM)
    assert int(got["n"]) == want.n, (what, int(got["n"]), want.n)
    assert np.array_equal(got["H"], got["H"].T), what                        # symmetric bit for bit
    g = 0.0 if exact else gamma(want.n + 8)
    for name in an.SUMS:
        d = np.abs(np.asarray(got[name]) - np.asarray(getattr(want, name)))
        bound = g * np.asarray(want.terms[name])
        assert np.all(d <= bound), (what, name, float(np.max(d)), float(np.max(d - bound)))
    return got


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_record_shapes_and_transforms(hip, k):
    fshape, mshape = SHAPES[k]
    F, M = volumes(fshape, mshape, 10 + k)
    for name, A in transforms(fshape, mshape).items():
        what = "%s -> %s %s" % (fshape, mshape, name)
        got = check(hip, F, M, A, what)
        if name == "outside":
            raw = hip.affine_ncc_normal_equations(dev(F), dev(M), A, raw=True)
            assert int(got["n"]) == 0 and not raw.cpu().numpy().any(), what     # an all-zero record


def test_integer_content_gives_exact_sums(hip):
    """tests/test_affine_refine.test_integer_content_gives_exact_sums' two pairs: integer volumes under an integer
    shift, so f, m and the gradients are integers, the centred positions integers or halves, and every term, every
    partial sum and every factor of a term an integer multiple of 1/4 far below 2^53: any order and factoring is exact"""
    rng = np.random.default_rng(4)
    for fshape, mshape in (((9, 21, 133), (11, 19, 140)), ((4, 6, 70), (5, 6, 72))):
        F = rng.integers(-30, 30, fshape).astype(np.float32)
        M = rng.integers(-30, 30, mshape).astype(np.float32)
        A = np.eye(3, 4)
        A[:, 3] = [5, -2, 1]
        got = check(hip, F, M, A, "integers %s" % (fshape,), exact=True)
        assert 0 < int(got["n"]) < F.size and got["v"].any() and got["w"].any() and np.all(np.diag(got["H"]) > 0)


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
    r0 = hip.affine_ncc_normal_equations(Fd, Md, A, raw=True).cpu().numpy()
    r1 = hip.affine_ncc_normal_equations(Fd, Md, A, raw=True).cpu().numpy()
    assert np.array_equal(r0, r1)


def test_cross_checks_against_similarity_and_the_msd_record(hip):
    """The five moments are the similarity record's sums of the same f and m, so they agree to the bound on two orders
    of summing, and exactly on integers.  H: k_affine_ncc_normal keeps k_affine_normal's factoring and order of the 60
    sums of H operation for operation, so H equals sift3d_hip_affine_normal_eqs' H bit for bit."""
    fshape, mshape = (9, 20, 133), (8, 21, 130)
    F, M = volumes(fshape, mshape, 16)
    A = transforms(fshape, mshape)["rotation"]
    rng = np.random.default_rng(5)
    Fi = rng.integers(-300, 300, fshape).astype(np.float32)
    Mi = rng.integers(-300, 300, mshape).astype(np.float32)
    S = np.eye(3, 4)
    S[:, 3] = [3, -2, 1]
    for Fv, Mv, T, rng_, exact in ((F, M, A, (-1.0, 1.5), False), (Fi, Mi, S, (-300.0, 300.0), True)):
        got = hip.affine_ncc_normal_equations(dev(Fv), dev(Mv), T)
        count, sums = hip.similarity_stats(hip.similarity(dev(Fv), dev(Mv), T, 64, rng_, rng_)[1])
        n = int(got["n"])
        assert n == count > 0
        for name, k in (("S_f", 0), ("S_m", 1), ("S_ff", 2), ("S_mm", 3), ("S_fm", 4)):
            a, b = float(got[name]), float(sums[k])
            if exact:
                assert a == b, name
            else:
                # sum |term| of S_f, S_m and S_fm is at most sqrt(n S_ff), sqrt(n S_mm) and sqrt(S_ff S_mm)
                mag = {"S_f": np.sqrt(n * sums[2]), "S_m": np.sqrt(n * sums[3]), "S_ff": sums[2], "S_mm": sums[3],
                       "S_fm": np.sqrt(sums[2] * sums[3])}[name]
                assert abs(a - b) <= 2 * gamma(n) * mag, (name, a, b)
        _, _, _, H = hip.affine_normal_equations(dev(Fv), dev(Mv), T)
        assert np.array_equal(got["H"], H)


def test_masks(hip):
    """both masks, a float fixed mask with values at 0.5 (in) and nextafter(0.5, 0) (out), against the masked
    restatement; both masks all in give the unmasked record's bytes"""
    fshape, mshape = (5, 6, 70), (5, 6, 70)
    F, M = volumes(fshape, mshape, 15)
    A = about_center(rot((0, 0, 1), 3.0), mshape, fshape, shift=(0.4, -0.3, 0.2))
    rng = np.random.default_rng(8)
    edge = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(0)), 1.0, 0.0, 2.0, np.nan, -1.0, np.inf], np.float32)
    WF = edge[rng.integers(0, len(edge), fshape)]
    WM = (rng.uniform(0, 1, mshape) < 0.7).astype(np.float32)
    got = check(hip, F, M, A, "both masks", WF=WF, WM=WM)
    plain = check(hip, F, M, A, "no masks")
    assert 0 < int(got["n"]) < int(plain["n"])
    half = np.full(fshape, np.nextafter(np.float32(0.5), np.float32(0)), np.float32)
    assert int(hip.affine_ncc_normal_equations(dev(F), dev(M), A, mask_fixed=dev(half))["n"]) == 0
    Fd, Md = dev(F), dev(M)
    r0 = hip.affine_ncc_normal_equations(Fd, Md, A, raw=True).cpu().numpy()
    r1 = hip.affine_ncc_normal_equations(Fd, Md, A, raw=True, mask_fixed=dev(np.full(fshape, 0.5, np.float32)),
                                         mask_moving=dev(np.ones(mshape, np.float32))).cpu().numpy()
    assert np.array_equal(r0, r1) and r0[0] > 0


def test_caller_buffers_and_value_errors(hip):
    import torch
    F, M = (dev(v) for v in volumes((5, 7, 9), (6, 5, 8), 8))
    rec = torch.full((186,), 7, dtype=torch.int64, device="cuda")
    work = torch.empty(hip.affine_ncc_normal_work_bytes(), dtype=torch.uint8, device="cuda")
    got = hip.affine_ncc_normal_equations(F, M, np.eye(3, 4), record=rec, work=work)
    want = hip.affine_ncc_normal_equations(F, M, np.eye(3, 4))
    assert got.tobytes() == want.tobytes() and int(got["n"]) > 0
    for bad in (lambda: hip.affine_ncc_normal_equations(F, M, np.eye(3)),
                lambda: hip.affine_ncc_normal_equations(F.cpu(), M, np.eye(3, 4)),
                lambda: hip.affine_ncc_normal_equations(F, M, np.eye(3, 4), record=rec[:100]),
                lambda: hip.affine_ncc_normal_equations(F, M, np.eye(3, 4), work=work[:100]),
                lambda: hip.affine_ncc_normal_equations(F, M, np.eye(3, 4), mask_fixed=M)):
        with pytest.raises(ValueError):
            bad()


# ---- the driver ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api():
    from sift3d_amd import api as a
    a.lib()
    return a


def cost_from_moments(hip, fixed, moving, A):
    """(cost, bound): the fit's cost from the similarity pass's moments at A, and a bound on the difference between
    two such costs whose five sums were each added in another order.  n cost = S_ff + alpha^2 S_mm + n beta^2
    + 2 alpha beta S_m - 2 alpha S_fm - 2 beta S_f at the fit, and its derivatives by the sums at the optimum of alpha
    and beta are those coefficients; a sum moves by at most 2 gamma_n sum |term| between two orders, and sum |term| of
    S_f, S_m, S_fm is at most sqrt(n S_ff), sqrt(n S_mm), sqrt(S_ff S_mm).  The fit's own dozen operations add 16 u of
    the same magnitudes (second-order terms, gamma^2, are left out)."""
    lo, hi = float(min(fixed.min(), moving.min())), float(max(fixed.max(), moving.max()))
    n, s = hip.similarity_stats(hip.similarity(dev(fixed), dev(moving), A, 64, (lo, hi), (lo, hi))[1])
    rec = an.Record(n, s[1], s[0], s[3], s[4], s[2], None, None, None, None, None)
    ft = an.fit(rec)
    a, b = abs(ft.alpha), abs(ft.beta)
    mag = s[2] + a * a * s[3] + n * b * b + 2 * a * b * np.sqrt(n * s[3]) + 2 * a * np.sqrt(s[2] * s[3]) \
        + 2 * b * np.sqrt(n * s[2])
    return ft.cost, (2 * gamma(n) + 16 * U) * mag / n


@pytest.mark.parametrize("free,mask", [("translation", 0x888), ("affine", 0xFFF)])
@pytest.mark.parametrize("gain,offset", [(-0.5, 0.0), (0.5, 32.0)])
def test_driver_mapped_pairs(api, hip, gain, offset, free, mask):
    fixed, moving, T = mapped_case(gain, offset)
    r = api.refine_affine(dev(moving), dev(fixed), free=free, metric="ncc")
    ref = an.refine(fixed, moving, free_mask=mask)
    assert type(r).__name__ == "NccAffineRefinement"
    err, apart = ar.corner_distance(r.A, T, fixed.shape), ar.corner_distance(r.A, ref.A, fixed.shape)
    print("gain %g offset %g %s: corner error %.3g after %d evaluations, stop %s; %.3g from the restatement's; "
          "gain %.6g offset %.6g ncc %.9f" % (gain, offset, free, err, r.evaluations, r.stop, apart, r.gain, r.offset,
                                              r.ncc))
    assert err <= 10 * TOL and apart <= 10 * TOL
    assert r.stop == "converged"
    assert abs(r.gain * gain - 1) <= 1e-3 and abs(r.offset + offset / gain) <= 1e-2
    assert r.level_slices == {0: slice(0, r.evaluations)} and len(r.cost) == r.evaluations
    want = dev(np.zeros_like(fixed))
    hip.warp_affine(dev(moving), want, r.A, "linear")
    assert np.array_equal(r.warped.cpu().numpy(), want.cpu().numpy())        # intensities are not remapped
    last = r.cost[r.accepted][-1]
    sim, bound = cost_from_moments(hip, fixed, moving, r.A)
    print("final cost %.6g, from the similarity pass's moments %.6g, bound %.3g" % (last, sim, bound))
    assert abs(last - sim) <= bound
    if free == "translation":
        assert np.array_equal(r.A[:, :3], np.eye(3))


def test_driver_levels(api):
    fixed, moving, T = mapped_case(0.5, 32.0)
    one = api.refine_affine(dev(moving), dev(fixed), metric="ncc")
    two = api.refine_affine(dev(moving), dev(fixed), levels=2, metric="ncc")
    apart = ar.corner_distance(one.A, two.A, fixed.shape)
    print("levels=2 ends %.3g from levels=1, %.3g from T, stop %s" % (apart, ar.corner_distance(two.A, T, fixed.shape),
                                                                      two.stop))
    assert apart <= 10 * TOL
    assert list(two.level_slices) == [1, 0]


def test_driver_masks_and_inputs_agree(api):
    """numpy input and tensor input give one result; all-in masks give the unmasked trail"""
    fixed, moving, T = mapped_case(-0.5, 0.0)
    a = api.refine_affine(dev(moving), dev(fixed), metric="ncc", max_evaluations=4)
    b = api.refine_affine(moving, fixed, np.eye(3, 4), metric="ncc", max_evaluations=4)
    c = api.refine_affine(moving, fixed, metric="ncc", max_evaluations=4, mask_fixed=np.ones(fixed.shape, bool),
                          mask_moving=np.ones(moving.shape, np.float32), levels=1)
    for other in (b, c):
        assert np.array_equal(a.A, other.A) and np.array_equal(a.cost, other.cost)
        assert np.array_equal(a.count, other.count) and a.stop == other.stop
        assert (a.ncc, a.gain, a.offset) == (other.ncc, other.gain, other.offset)


def test_register_with_the_ncc_metric(api):
    """end to end: register() hands refine=dict(metric="ncc") to refine_affine.  The moving volume carries a gain of 2
    and an offset of 1/8 (the keypoint stages see the same structure).  An accepted step lowers V_f (1 - ncc^2) / n, so
    |ncc| at the refined map is at least |ncc| at the RANSAC map it started from, as api.similarity measures both (two
    orders of the same sums: 1e-9)."""
    import torch
    from sift3d_amd import hip
    fixed, T, Tinv = end_to_end_case(api)
    Fd = dev(fixed)
    Md = torch.empty_like(Fd)
    hip.warp_affine(Fd, Md, Tinv, "linear", 0.0)
    mapped = (2.0 * Md + 0.125).contiguous()
    fine = api.register(mapped, Fd, refine=dict(metric="ncc"))
    assert type(fine).__name__ == "RefinedRegistration"
    assert type(fine.refinement).__name__ == "NccAffineRefinement"
    print("ncc %.6f gain %.4f offset %.4f after %d evaluations (%s)" % (
        fine.refinement.ncc, fine.refinement.gain, fine.refinement.offset, fine.refinement.evaluations,
        fine.refinement.stop))
    before = api.similarity(Fd, mapped, api.affine_invert(fine.A_ransac)).ncc
    after = api.similarity(Fd, mapped, fine.refinement.A).ncc
    print("ncc: RANSAC %.9f, refined %.9f" % (before, after))
    assert abs(after) >= abs(before) - 1e-9 and abs(after - fine.refinement.ncc) <= 1e-9
    np.testing.assert_allclose(api.affine_invert(fine.A), fine.refinement.A, rtol=0, atol=1e-9)
