"""Mutual-information affine refinement on the device (sift3d_hip_parzen_hist_affine, sift3d_hip_affine_mi_normal_eqs,
sift3d_amd_affine_mi_refine_device; include/sift3d_amd.h, "Mutual-information affine refinement (Mattes)") against the
numpy restatement (tests/affine_mi_restatement.py): the fixed-point histogram and the count bit for bit; the record's
count bit for bit and every one of its 73 sums exactly where every term is a small dyadic rational, and otherwise to
gamma_(n + 11) sum |terms|.  Both sides of a record comparison take the restatement's table W, so no logarithm enters a
device comparison.  The driver against the restatement's driver on the pairs of tests/test_affine_mi_host.py."""
import numpy as np
import pytest

from tests import affine_mi_restatement as am
from tests import affine_ncc_restatement as an
from tests import affine_refine_restatement as ar
from tests.demons_restatement import gamma
from tests.test_affine_mi_host import BINS, DRIVER_BOUND, driven, driver_case, own_range
from tests.test_affine_refine_host import TOL
from tests.test_similarity import SHAPES, TILE, dev, transforms, volumes
from tests.test_similarity_host import end_to_end_case
from tests.test_warp import about_center, rot

pytestmark = pytest.mark.gpu
RF, RM = (-1.0, 1.5), (-1.0, 1.5)                          # volumes() puts values at, and beyond, both ends
SOME_BINS = [4, 19, 64]


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


def opt(v):
    return None if v is None else dev(v)


# ---- the histogram ---------------------------------------------------------------------------------------------------
def check_hist(hip, F, M, A, bins, what, rf=RF, rm=RM, WF=None, WM=None):
    """one call against the restatement, bit for bit.  Returns (hist, count)."""
    hist, count = hip.parzen_histogram(dev(F), dev(M), A, bins, rf, rm, mask_fixed=opt(WF), mask_moving=opt(WM))
    hist, count = hist.cpu().numpy(), int(count.cpu().numpy()[0])
    want, n, qsum = am.histogram(F, M, A, bins, rf, rm, WF, WM)
    np.testing.assert_array_equal(hist, want, err_msg=what)
    assert count == n, (what, count, n)
    assert int(hist.sum()) == qsum and abs(qsum - 65536 * n) <= 2 * n, what          # N = the voxels' sums of q
    return hist, count


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_histogram_shapes_transforms_bins(hip, k):
    fshape, mshape = SHAPES[k]
    F, M = volumes(fshape, mshape, 10 + k)
    for name, A in transforms(fshape, mshape).items():
        for bins in SOME_BINS:
            hist, count = check_hist(hip, F, M, A, bins, "%s -> %s %s B=%d" % (fshape, mshape, name, bins))
            if name == "outside":
                assert count == 0 and not hist.any()


def grid_cap_shape(hip):
    """tests/test_similarity.test_more_tiles_than_workgroups' grid: a second, partial pass over the tiles"""
    G = hip.SIMILARITY_GRID
    ty = int(np.ceil(np.sqrt(G + 1)))
    tz = -(-(G + 1) // ty)
    assert G < ty * tz < 2 * G
    return (TILE[0] * (tz - 1) + 1, TILE[1] * (ty - 1) + 1, 2)


def test_histogram_more_tiles_than_workgroups_and_calls_repeat(hip):
    fshape = grid_cap_shape(hip)
    F, M = volumes(fshape, (fshape[0] - 3, fshape[1] + 2, 3), 3)
    A = about_center(rot((1, 0, 0), 10.0), M.shape, fshape, shift=(0.2, 0, 0))
    check_hist(hip, F, M, A, 19, "grid cap")
    Fd, Md = dev(F), dev(M)
    h0, c0 = hip.parzen_histogram(Fd, Md, A, 19, RF, RM)
    h1, c1 = hip.parzen_histogram(Fd, Md, A, 19, RF, RM)
    assert np.array_equal(h0.cpu().numpy(), h1.cpu().numpy()) and int(c0[0]) == int(c1[0]) > 0


def mask_pair(fshape, mshape):
    """tests/test_affine_ncc.test_masks' masks: a float fixed mask with values at 0.5 (in) and just below (out)"""
    rng = np.random.default_rng(8)
    edge = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(0)), 1.0, 0.0, 2.0, np.nan, -1.0, np.inf], np.float32)
    return edge[rng.integers(0, len(edge), fshape)], (rng.uniform(0, 1, mshape) < 0.7).astype(np.float32)


def test_histogram_masks(hip):
    fshape, mshape = (5, 6, 70), (5, 6, 70)
    F, M = volumes(fshape, mshape, 15)
    A = about_center(rot((0, 0, 1), 3.0), mshape, fshape, shift=(0.4, -0.3, 0.2))
    WF, WM = mask_pair(fshape, mshape)
    plain = check_hist(hip, F, M, A, 19, "no masks")
    both = check_hist(hip, F, M, A, 19, "both masks", WF=WF, WM=WM)
    one_f = check_hist(hip, F, M, A, 19, "fixed mask", WF=WF)
    one_m = check_hist(hip, F, M, A, 19, "moving mask", WM=WM)
    assert 0 < both[1] < min(one_f[1], one_m[1]) and max(one_f[1], one_m[1]) < plain[1]
    Fd, Md = dev(F), dev(M)
    h0, c0 = hip.parzen_histogram(Fd, Md, A, 19, RF, RM)
    h1, c1 = hip.parzen_histogram(Fd, Md, A, 19, RF, RM, mask_fixed=dev(np.full(fshape, 0.5, np.float32)),
                                  mask_moving=dev(np.ones(mshape, np.float32)))
    assert h0.cpu().numpy().tobytes() == h1.cpu().numpy().tobytes() and int(c0[0]) == int(c1[0]) > 0


# ---- the record ------------------------------------------------------------------------------------------------------
def check_record(hip, F, M, A, bins, what, W=None, rf=RF, rm=RM, WF=None, WM=None, exact=False):
    """One call against the restatement, both with the restatement's table (W=None: the table of the histogram at A).

    The bound: the restatement's sums are correctly rounded, and gamma_k sum |term| bounds the sum of n terms that each
    carry k - n roundings, in any order.  A term of the MSD record carries at most 8 roundings however it is factored
    (header); here G'_d = psi * g_d is rounded where G_d was an exact widening (one rounding for each of the two
    gradient factors of a term of H, one for the single factor of a term of b), and the product G'_d G'_e, exact for
    two widened floats, is rounded too: 11.  psi itself enters both sides bit for bit: one function, one W."""
    if W is None:
        W = am.measures(am.histogram(F, M, A, bins, rf, rm, WF, WM)[0]).W
    n, spp, b, H = hip.affine_mi_normal_equations(dev(F), dev(M), A, W, rf, rm, mask_fixed=opt(WF), mask_moving=opt(WM))
    want = am.record(F, M, A, W, bins, rf, rm, WF, WM)
    assert n == want.n, (what, n, want.n)
    assert np.array_equal(H, H.T), what                                      # symmetric bit for bit
    g = 0.0 if exact else gamma(want.n + 11)
    for name, got, ref, terms in (("S_pp", spp, want.see, want.see_terms), ("b", b, want.b, want.b_terms),
                                  ("H", H, want.H, want.H_terms)):
        d = np.abs(np.asarray(got) - np.asarray(ref))
        bound = g * np.asarray(terms)
        assert np.all(d <= bound), (what, name, float(np.max(d)), float(np.max(d - bound)))
    return n, spp, b, H


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_record_shapes_and_transforms(hip, k):
    fshape, mshape = SHAPES[k]
    F, M = volumes(fshape, mshape, 10 + k)
    for i, (name, A) in enumerate(transforms(fshape, mshape).items()):
        bins = SOME_BINS[(i + k) % 3]
        what = "%s -> %s %s B=%d" % (fshape, mshape, name, bins)
        n, spp, b, H = check_record(hip, F, M, A, bins, what)
        if name == "outside":
            raw = hip.affine_mi_normal_equations(dev(F), dev(M), A, np.ones((bins, bins)), RF, RM, raw=True)
            assert n == 0 and not raw.cpu().numpy().any(), what             # an all-zero record


def test_record_more_tiles_than_workgroups_and_calls_repeat(hip):
    fshape = grid_cap_shape(hip)
    F, M = volumes(fshape, (fshape[0] - 3, fshape[1] + 2, 3), 3)
    A = about_center(rot((1, 0, 0), 10.0), M.shape, fshape, shift=(0.2, 0, 0))
    W = am.measures(am.histogram(F, M, A, 19, RF, RM)[0]).W
    check_record(hip, F, M, A, 19, "grid cap", W=W)
    Fd, Md, Wd = dev(F), dev(M), dev(W)
    r0 = hip.affine_mi_normal_equations(Fd, Md, A, Wd, RF, RM, raw=True).cpu().numpy()
    r1 = hip.affine_mi_normal_equations(Fd, Md, A, Wd, RF, RM, raw=True).cpu().numpy()
    assert np.array_equal(r0, r1) and r0[0] > 0


def test_record_masks(hip):
    fshape, mshape = (5, 6, 70), (5, 6, 70)
    F, M = volumes(fshape, mshape, 15)
    A = about_center(rot((0, 0, 1), 3.0), mshape, fshape, shift=(0.4, -0.3, 0.2))
    WF, WM = mask_pair(fshape, mshape)
    W = am.measures(am.histogram(F, M, A, 19, RF, RM)[0]).W
    plain = check_record(hip, F, M, A, 19, "no masks", W=W)
    both = check_record(hip, F, M, A, 19, "both masks", W=W, WF=WF, WM=WM)
    check_record(hip, F, M, A, 19, "fixed mask", W=W, WF=WF)
    check_record(hip, F, M, A, 19, "moving mask", W=W, WM=WM)
    assert 0 < both[0] < plain[0]
    Fd, Md, Wd = dev(F), dev(M), dev(W)
    r0 = hip.affine_mi_normal_equations(Fd, Md, A, Wd, RF, RM, raw=True).cpu().numpy()
    r1 = hip.affine_mi_normal_equations(Fd, Md, A, Wd, RF, RM, raw=True,
                                        mask_fixed=dev(np.full(fshape, 0.5, np.float32)),
                                        mask_moving=dev(np.ones(mshape, np.float32))).cpu().numpy()
    assert np.array_equal(r0, r1) and r0[0] > 0


def test_record_of_voxels_outside_the_moving_range(hip):
    """a voxel whose sample lies outside [lo_m, hi_m] is counted and adds nothing else: with every sample outside, the
    record is n and zeros, whatever W holds"""
    fshape, mshape = (5, 6, 70), (5, 6, 70)
    F, M = volumes(fshape, mshape, 15)
    A = about_center(rot((0, 0, 1), 3.0), mshape, fshape, shift=(0.4, -0.3, 0.2))
    W = np.random.default_rng(2).normal(0, 1, (19, 19))
    n, spp, b, H = check_record(hip, F, M, A, 19, "all out", W=W, rm=(100.0, 200.0), exact=True)
    assert n > 0 and spp == 0 and not b.any() and not H.any()
    n2, spp2, b2, H2 = check_record(hip, F, M, A, 19, "some out", W=W)
    assert n2 == n and spp2 > 0 and b2.any()


def test_dyadic_content_gives_exact_sums(hip):
    """tests/test_affine_refine.test_integer_content_gives_exact_sums' two pairs under an integer shift, B = 19 and
    hi_m - lo_m = 16, so s_m = 1 exactly, and an integer-valued W.  Integer moving values: r is 0 (1 at hi_m) and dw is
    in {-1/2, 0, 1/2}; moving values at the halves: r = 1/2 and dw = (-1/8, -5/8, 5/8, 1/8).  The gradients are
    integers, the centred positions integers or halves, so psi, G', every term and every partial sum is an integer
    multiple of 2^-10 far below 2^53: any order and factoring is exact.  Values beyond the range (|m| up to 10 against
    8) are `out`."""
    rng = np.random.default_rng(4)
    W = rng.integers(-4, 5, (19, 19)).astype(np.float64)
    for fshape, mshape in (((9, 21, 133), (11, 19, 140)), ((4, 6, 70), (5, 6, 72))):
        F = rng.integers(-30, 30, fshape).astype(np.float32)
        Mi = rng.integers(-10, 11, mshape).astype(np.float32)
        A = np.eye(3, 4)
        A[:, 3] = [5, -2, 1]
        for M, what in ((Mi, "integers"), (Mi + np.float32(0.5), "halves")):
            win = am.window(M, -8.0, 8.0, 19)
            assert set(np.unique(np.abs(win.dw[~win.out]))) <= ({0.0, 0.5} if what == "integers" else {0.125, 0.625})
            n, spp, b, H = check_record(hip, F, M, A, 19, "%s %s" % (what, fshape), W=W, rf=(-30.0, 30.0),
                                        rm=(-8.0, 8.0), exact=True)
            assert 0 < n < F.size and win.out.any() and spp > 0 and b.any() and np.all(np.diag(H) > 0)
            check_hist(hip, F, M, A, 19, "%s %s" % (what, fshape), rf=(-30.0, 30.0), rm=(-8.0, 8.0))


def test_cross_checks_against_the_ncc_and_msd_records(hip):
    """W == 0: the record is all zero but for n.  W[i][j] = j, linear in the bin: psi = s_m sum_k dw[k] (k0 + k) = s_m
    wherever the sample is in range, by the partition of unity of the weights (sum dw = 0, sum k dw[k] = 1).  Then
    b = -s_m u of the NCC record and H = s_m^2 H of the MSD record, within gamma_(n + 11) sum |term| against the NCC
    restatement's correctly rounded sums.  The sum over k cancels (terms up to B / 2 against a result of 1) and costs
    up to about 4 B roundings of psi, twice that in a term of H, beside the n - 1 additions that gamma_n allows for and
    that no order of this kernel comes near (a term passes through at most 4 additions per pass over the tiles, 6 of
    the butterfly, 3 of the waves and 16 of the finish): at B = 4 (k0 == 0, three exact products) any n fits, at
    B = 19 n > 300 does."""
    for fshape, mshape, all_bins in (((9, 20, 133), (8, 21, 130), (4, 19)),):
        F, M = volumes(fshape, mshape, 16)
        A = transforms(fshape, mshape)["rotation"]
        ref = an.record(F, M, A)
        for bins in all_bins:
            rm = (-10.0, 10.0)                                               # every value is inside
            s_m = am.scale(rm[0], rm[1], bins)
            Fd, Md = dev(F), dev(M)
            n, spp, b, H = hip.affine_mi_normal_equations(Fd, Md, A, np.zeros((bins, bins)), RF, rm)
            assert n == ref.n > 300 and spp == 0 and not b.any() and not H.any()
            W = np.tile(np.arange(bins, dtype=np.float64), (bins, 1))
            n, spp, b, H = hip.affine_mi_normal_equations(Fd, Md, A, W, RF, rm)
            g = gamma(n + 11)
            assert n == ref.n and abs(spp - s_m * s_m * n) <= g * s_m * s_m * n
            assert np.all(np.abs(b + s_m * ref.u) <= g * s_m * ref.terms["u"]), bins
            assert np.all(np.abs(H - s_m * s_m * ref.H) <= g * s_m * s_m * ref.terms["H"]), bins
            Hm = hip.affine_normal_equations(Fd, Md, A)[3]
            assert np.all(np.abs(H - s_m * s_m * Hm) <= 2 * g * s_m * s_m * ref.terms["H"]), bins


def test_caller_buffers_and_value_errors(hip):
    import torch
    F, M = (dev(v) for v in volumes((5, 7, 9), (6, 5, 8), 8))
    W = dev(np.random.default_rng(1).normal(0, 1, (19, 19)))
    rec = torch.full((158,), 7, dtype=torch.int64, device="cuda")
    work = torch.empty(hip.affine_normal_work_bytes(), dtype=torch.uint8, device="cuda")
    got = hip.affine_mi_normal_equations(F, M, np.eye(3, 4), W, RF, RM, record=rec, work=work)
    want = hip.affine_mi_normal_equations(F, M, np.eye(3, 4), W, RF, RM)
    assert got[0] == want[0] > 0 and all(np.array_equal(a, b) for a, b in zip(got[1:], want[1:]))
    hist = torch.full((19, 19), 7, dtype=torch.int64, device="cuda")
    hwork = torch.empty(hip.SIMILARITY_GRID * 8, dtype=torch.uint8, device="cuda")
    h0, c0 = hip.parzen_histogram(F, M, np.eye(3, 4), 19, RF, RM, hist=hist, work=hwork)
    h1, c1 = hip.parzen_histogram(F, M, np.eye(3, 4), 19, RF, RM)
    assert h0 is hist and torch.equal(h0, h1) and torch.equal(c0, c1)
    for bad in (lambda: hip.affine_mi_normal_equations(F, M, np.eye(3), W, RF, RM),
                lambda: hip.affine_mi_normal_equations(F.cpu(), M, np.eye(3, 4), W, RF, RM),
                lambda: hip.affine_mi_normal_equations(F, M, np.eye(3, 4), W[:, :5], RF, RM),
                lambda: hip.affine_mi_normal_equations(F, M, np.eye(3, 4), W.float(), RF, RM),
                lambda: hip.affine_mi_normal_equations(F, M, np.eye(3, 4), W, RF, RM, record=rec[:100]),
                lambda: hip.affine_mi_normal_equations(F, M, np.eye(3, 4), W, RF, RM, work=work[:100]),
                lambda: hip.affine_mi_normal_equations(F, M, np.eye(3, 4), W, RF, RM, mask_fixed=M),
                lambda: hip.parzen_histogram(F, M, np.eye(3, 4), 3, RF, RM),
                lambda: hip.parzen_histogram(F, M, np.eye(3, 4), 19, RF, RM, hist=hist[:5]),
                lambda: hip.parzen_histogram(F, M, np.eye(3, 4), 19, RF, RM, work=hwork[:100])):
        with pytest.raises(ValueError):
            bad()


# ---- the driver ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api():
    from sift3d_amd import api as a
    a.lib()
    return a


def device_mi(hip, fixed, moving, A, bins=BINS):
    hist, _ = hip.parzen_histogram(dev(fixed), dev(moving), A, bins, own_range(fixed), own_range(moving))
    return hip.parzen_mi(hist)


@pytest.mark.parametrize("translation", [False, True])
@pytest.mark.parametrize("kind", ["hump", "linear"])
def test_driver_rich_pairs(api, hip, kind, translation):
    """The device's driver ends where the restatement's does (10 TOL: the accept decisions come from exact integers, and
    relative noise of 1e-12 on b and H moved a float64 prototype's result by 1e-9 voxel), converged and within the
    restatement's own bound of Tc; its last accepted cost is the host routine's value on the device's histogram at the
    final map, the same integers through the same routine: equal."""
    fixed, moving, Tc = driver_case(kind, translation)
    r = api.refine_affine(dev(moving), dev(fixed), free="translation" if translation else "affine", metric="mi",
                          bins=BINS, max_evaluations=60)
    ref = driven(kind, translation)
    assert type(r).__name__ == "MiAffineRefinement" and r.bins == BINS
    err, apart = ar.corner_distance(r.A, Tc, fixed.shape), ar.corner_distance(r.A, ref.A, fixed.shape)
    print("%s %s: corner error %.3g after %d evaluations, stop %s; %.3g from the restatement's (%d evaluations); mi %.6f"
          % (kind, "translation" if translation else "affine", err, r.evaluations, r.stop, apart, ref.evaluations, r.mi))
    assert apart <= 10 * TOL
    assert r.stop == "converged" and err <= DRIVER_BOUND
    assert r.level_slices == {0: slice(0, r.evaluations)} and len(r.cost) == r.evaluations
    at_A = device_mi(hip, fixed, moving, r.A)
    assert r.cost[r.accepted][-1] == -at_A.mi and r.mi == at_A.mi and r.nmi == at_A.nmi
    assert np.all(np.diff(r.cost[r.accepted]) < 0)
    want = dev(np.zeros_like(fixed))
    hip.warp_affine(dev(moving), want, r.A, "linear")
    assert np.array_equal(r.warped.cpu().numpy(), want.cpu().numpy())        # intensities are not remapped
    if translation:
        assert np.array_equal(r.A[:, :3], np.eye(3))


def test_driver_levels(api):
    fixed, moving, Tc = driver_case("hump")
    two = api.refine_affine(dev(moving), dev(fixed), levels=2, metric="mi", bins=BINS, max_evaluations=60)
    err = ar.corner_distance(two.A, Tc, fixed.shape)
    print("levels=2 ends %.3g from Tc after %d evaluations, stop %s" % (err, two.evaluations, two.stop))
    assert err <= DRIVER_BOUND
    assert list(two.level_slices) == [1, 0]


def test_driver_masks_and_inputs_agree(api):
    """numpy input and tensor input give one result; all-in masks give the unmasked trail"""
    fixed, moving, Tc = driver_case("linear")
    a = api.refine_affine(dev(moving), dev(fixed), metric="mi", max_evaluations=4)
    b = api.refine_affine(moving, fixed, np.eye(3, 4), metric="mi", bins=32, max_evaluations=4,
                          range_fixed=own_range(fixed), range_moving=own_range(moving))
    c = api.refine_affine(moving, fixed, metric="mi", max_evaluations=4, mask_fixed=np.ones(fixed.shape, bool),
                          mask_moving=np.ones(moving.shape, np.float32), levels=1)
    assert a.evaluations == 4 and a.bins == 32
    for other in (b, c):
        assert np.array_equal(a.A, other.A) and np.array_equal(a.cost, other.cost)
        assert np.array_equal(a.count, other.count) and a.stop == other.stop
        assert (a.mi, a.nmi) == (other.mi, other.nmi)


def register_case(api, hip, remap):
    """(fixed, moving on the device, fixed on the host): end_to_end_case's pair, the moving volume remapped"""
    import torch
    fixed, T, Tinv = end_to_end_case(api)
    Fd = dev(fixed)
    Md = torch.empty_like(Fd)
    hip.warp_affine(Fd, Md, Tinv, "linear", 0.0)
    return Fd, remap(Md).contiguous(), fixed


def check_register(api, hip, Fd, mapped, fixed):
    fine = api.register(mapped, Fd, refine=dict(metric="mi"))
    assert type(fine).__name__ == "RefinedRegistration"
    assert type(fine.refinement).__name__ == "MiAffineRefinement"
    mv = mapped.cpu().numpy()
    before = device_mi(hip, fixed, mv, api.affine_invert(fine.A_ransac)).mi
    after = device_mi(hip, fixed, mv, fine.refinement.A).mi
    print("mi: RANSAC %.9f, refined %.9f after %d evaluations (%s)" % (before, after, fine.refinement.evaluations,
                                                                       fine.refinement.stop))
    assert after >= before and after == fine.refinement.mi
    np.testing.assert_allclose(api.affine_invert(fine.A), fine.refinement.A, rtol=0, atol=1e-9)
    return fine


def test_register_with_the_mi_metric(api, hip):
    """end to end: register() hands refine=dict(metric="mi") to refine_affine.  The moving volume is the fixed one
    through the true map, mapped by the hump (m - 50)^2 / 25 of the driver case.  An accepted step raises the MI, so the
    MI at the refined map is at least the MI at the RANSAC map it started from, both measured by parzen_histogram and
    parzen_mi: exact integers through one routine.

    The volume's values lie in [-1.31, 1.10], where the hump is a decreasing map (about 100 - 4 m): the contrast is
    inverted, and SIFT3D's descriptors do not survive that (on the CPU oracle the plain pair gives 12 ratio-test
    matches of 25 and 21 keypoints, this pair 1; the device matched none), so RANSAC has no model.  With metric="mi"
    register() then starts the refinement from the identity, 4.0 voxels from the truth at the corners (the restatement's driver ends 0.59 away after its 30
    evaluations, the MI up from 0.73 to 1.48), and reports the
    identity as A_ransac with no inliers; with any other refinement, or none, it raises as it did."""
    Fd, mapped, fixed = register_case(api, hip, lambda m: (m - 50.0) ** 2 / 25.0)
    fine = check_register(api, hip, Fd, mapped, fixed)
    assert np.array_equal(fine.A_ransac, np.eye(3, 4)) and not fine.inliers.any()
    T = end_to_end_case(api)[1]
    start, end = (ar.corner_distance(A, T, fixed.shape) for A in (np.eye(3, 4), fine.refinement.A))
    print("from the identity: %.3g voxels from the truth at the corners, refined %.3g" % (start, end))
    for other in (True, dict(metric="ncc"), False):
        with pytest.raises(RuntimeError):
            api.register(mapped, Fd, refine=other)


def test_register_with_the_mi_metric_under_a_gain(api, hip):
    """the same end-to-end call on tests/test_affine_ncc.test_register_with_the_ncc_metric's pair (a gain of 2 and an
    offset of 1/8, which the keypoint stages see through): the refinement starts from RANSAC's model"""
    Fd, mapped, fixed = register_case(api, hip, lambda m: 2.0 * m + 0.125)
    fine = check_register(api, hip, Fd, mapped, fixed)
    assert fine.inliers.sum() >= 4 and not np.array_equal(fine.A_ransac, np.eye(3, 4))
