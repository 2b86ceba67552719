"""Mutual-information free-form deformation on the device (sift3d_hip_parzen_hist_field, sift3d_hip_ffd_mi_evaluate,
sift3d_amd_ffd_mi_refine_device; include/sift3d_amd.h, "Mutual-information free-form deformation (Mattes)") against the
numpy restatement (tests/ffd_mi_restatement.py): the fixed-point histogram through a field and its count bit for bit;
the evaluation's field and count bit for bit, S_pp to gamma_(n + 11) sum |terms| and every entry of Gc to
gamma_(k + 9) sum |terms| (k the voxels under the control: the FFD record's bound with one more rounding per term, the
product psi * g_d), the gradient bit for bit from the device's own Gc with the factor 1 / n.  Both sides of an
evaluation take the restatement's table W, so no logarithm enters a device comparison.  The driver against the
restatement's driver on the pair of tests/test_ffd_mi_host.py.  Every instantiation of the two new kernel families
(k_parzen_hist<., ., FIELD>, k_ffd_mi_force: LINEAR 1 or 2, times MASKED) has a case here."""
import numpy as np
import pytest

from tests import affine_mi_restatement as am
from tests import ffd_mi_restatement as fm
from tests import ffd_restatement as fr
from tests import sampling_cases as sc
from tests.demons_restatement import gamma
from tests.test_ffd import GRIDS, random_lattice, rotating
from tests.test_ffd_host import driver_pair as msd_driver_pair
from tests.test_ffd_mi_host import DRIVER, check_trail, driver_pair, level0_gain, restatement_driver, rms_error
from tests.test_similarity import TILE, dev, volumes

pytestmark = pytest.mark.gpu
RF, RM = (-1.0, 1.5), (-1.0, 1.5)                          # volumes() puts values at, and beyond, both ends
NARROW = (-0.5, 0.5)                                       # narrower than the moving values: some are `out`
SOME_BINS = [4, 19, 64]


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


@pytest.fixture(scope="module")
def api():
    from sift3d_amd import api as a
    a.lib()
    return a


def opt(v):
    return None if v is None else dev(v)


def moving_shape(shape):
    return (shape[0] + 1, shape[1] + 2, shape[2] - 1)      # tests/test_ffd.test_record's


def transforms(shape):
    """tests/test_ffd.test_record's four: (name, lattice kind, A)"""
    partly = np.eye(3, 4)
    partly[:, 3] = [shape[2] * 0.4, -0.3, 0.2]
    outside = np.eye(3, 4)
    outside[:, 3] = [1000.0, 0.0, 0.0]
    return [("zero", "zero", None), ("random", "random", rotating(shape)), ("partly outside", "random", partly),
            ("outside", "zero", outside)]


def lattice_of(kind, shape, spacing, seed):
    return np.zeros(fr.lattice_shape(shape, spacing), np.float32) if kind == "zero" else \
        random_lattice(shape, spacing, seed)


# ---- the histogram through a field -----------------------------------------------------------------------------------
def check_hist(hip, F, M, field, bins, what, rf=RF, rm=RM, WF=None, WM=None):
    """one call against the restatement, bit for bit.  Returns (hist, count)."""
    hist, count = hip.parzen_histogram_field(dev(F), dev(M), dev(field), bins, rf, rm, mask_fixed=opt(WF),
                                             mask_moving=opt(WM))
    hist, count = hist.cpu().numpy(), int(count.cpu().numpy()[0])
    want, n = fm.histogram_field(F, M, field, bins, rf, rm, WF, WM)
    np.testing.assert_array_equal(hist, want, err_msg=what)
    assert count == n, (what, count, n)
    assert abs(int(hist.sum()) - 65536 * n) <= 2 * n, what
    return hist, count


@pytest.mark.parametrize("k", range(len(GRIDS)))
def test_histogram_field_grids_transforms_bins(hip, k):
    shape, spacing = GRIDS[k]
    F, M = volumes(shape, moving_shape(shape), 20 + k)
    seen_out = False
    for name, kind, A in transforms(shape):
        field = fr.field(lattice_of(kind, shape, spacing, 30 + k), spacing, shape, A)
        for bins in SOME_BINS:
            hist, count = check_hist(hip, F, M, field, bins, "%s %s B=%d" % (shape, name, bins))
            if name == "outside":
                assert count == 0 and not hist.any()
            if name == "partly outside":
                assert 0 < count < F.size
        if name == "random":
            narrow = check_hist(hip, F, M, field, 19, "%s narrow range" % (shape,), rm=NARROW)
            m = fr.sample_grad(M, field)[0]
            seen_out = bool(am.window(m, NARROW[0], NARROW[1], 19).out.any()) and narrow[1] > 0
    assert seen_out


@pytest.mark.parametrize("nx", [70, 1])
@pytest.mark.parametrize("masked", [False, True])
def test_histogram_field_every_instantiation(hip, nx, masked):
    """k_parzen_hist<LINEAR, MASKED, true>: LINEAR 2 (nx >= 2) and 1 (a moving volume one voxel wide, the field's x
    channel -p so that the coordinate is exactly 0: tests/sampling_cases.py's construction), with masks and without"""
    c = sc.case("similarity", (4, 6, 70), (5, 6, nx), field=True, wf=masked, wm=masked, seed=40 + nx + masked)
    assert sc.selection_key("similarity", c) == ("similarity", 2 if nx >= 2 else 1, True, masked)
    d = sc.build(c)
    for bins in SOME_BINS:
        _, count = check_hist(hip, d.F, d.M, d.field, bins, "nx %d masked %s B=%d" % (nx, masked, bins), WF=d.WF,
                              WM=d.WM)
        assert 0 < count and (not masked or count < d.F.size)


@pytest.mark.parametrize("masked", [False, True])
def test_histogram_field_with_non_finite_entries(hip, masked):
    """a non-finite field entry is outside (tests/sampling_cases.NONFINITE's construction: NaN, +-inf, +-1e30)"""
    c = sc.case("similarity", (4, 5, 64), (3, 6, 70), field=True, wf=masked, wm=masked, seed=7, nonfinite=True)
    d = sc.build(c)
    assert not np.isfinite(d.field).all()
    clean = np.where(np.isfinite(d.field) & (np.abs(d.field) < 1e29), d.field, np.float32(1e6))
    _, count = check_hist(hip, d.F, d.M, d.field, 19, "non-finite", WF=d.WF, WM=d.WM)
    _, count_clean = check_hist(hip, d.F, d.M, clean, 19, "far outside instead", WF=d.WF, WM=d.WM)
    assert 0 < count == count_clean


def test_histogram_field_of_a_zero_lattice_is_the_affine_histogram(hip):
    """the field of ffd_field(zero lattice, A) with integer offsets is exact, so the bytes are parzen_histogram's at A"""
    import torch
    shape, spacing = GRIDS[0]
    F, M = volumes(shape, moving_shape(shape), 5)
    A = np.eye(3, 4)
    A[:, 3] = [1.0, 2.0, -1.0]
    field = torch.empty((3,) + shape, dtype=torch.float32, device="cuda")
    hip.ffd_field(dev(np.zeros(fr.lattice_shape(shape, spacing), np.float32)), spacing, field, A)
    for masks in (dict(), dict(mask_fixed=dev((np.arange(F.size).reshape(shape) % 3 > 0).astype(np.float32)))):
        h0, c0 = hip.parzen_histogram_field(dev(F), dev(M), field, 19, RF, RM, **masks)
        h1, c1 = hip.parzen_histogram(dev(F), dev(M), A, 19, RF, RM, **masks)
        assert h0.cpu().numpy().tobytes() == h1.cpu().numpy().tobytes() and int(c0[0]) == int(c1[0]) > 0


# ---- the MI evaluation -----------------------------------------------------------------------------------------------
def check_record(hip, F, M, c, spacing, A, bins, what, rf=RF, rm=RM, WF=None, WM=None):
    """One evaluation against the restatement, both with the restatement's table W (of the histogram at the lattice)."""
    u = fr.field(c, spacing, F.shape, A)
    hist, cnt = fm.histogram_field(F, M, u, bins, rf, rm, WF, WM)
    W = am.measures(hist).W
    rec, grad, fld = hip.ffd_mi_evaluate(dev(F), dev(M), dev(c), spacing, W, rf, rm, A, bending=0.01,
                                         mask_fixed=opt(WF), mask_moving=opt(WM))
    n, spp, R, gmax, Gc, dR = hip.ffd_record(rec, c.shape)
    want, u2 = fm.evaluate(F, M, c, spacing, A, W, bins, (rf, rm), WF, WM)
    assert np.array_equal(fld.cpu().numpy(), u) and np.array_equal(u, u2), what
    _, dcount = hip.parzen_histogram_field(dev(F), dev(M), fld, bins, rf, rm, mask_fixed=opt(WF),
                                           mask_moving=opt(WM))
    assert n == want.n == cnt == int(dcount[0]), (what, n, want.n, cnt)
    print("%s: n %d S_pp %.9g (off %.3g)" % (what, n, spp, abs(spp - want.spp)))
    assert abs(spp - want.spp) <= gamma(n + 11) * want.spp_terms, (what, spp, want.spp)
    bound = np.array([gamma(int(k) + 9) for k in want.support.reshape(-1)]).reshape(want.support.shape)
    bound = bound * want.Gc_terms
    off = np.abs(Gc - want.Gc)
    assert np.all(off <= bound), (what, off.max(), (off - bound).max())
    Rw, dRw, Rt, dRt = fr.bending(c, spacing)
    assert abs(R - Rw) <= gamma(6 * 40 + c.size) * Rt, (what, R, Rw)
    assert np.all(np.abs(dR - dRw) <= gamma(200) * dRt), what
    if n:
        g, gm = fm.gradient(want._replace(Gc=Gc), dR, 0.01)              # from the device's own sums: bit for bit
        assert np.array_equal(grad.cpu().numpy(), g) and gmax == gm, what
    return rec, n, spp, Gc


@pytest.mark.parametrize("k", range(len(GRIDS)))
def test_record(hip, k):
    shape, spacing = GRIDS[k]
    bins = SOME_BINS[k % 3]
    F, M = volumes(shape, moving_shape(shape), 20 + k)
    some = False
    for name, kind, A in transforms(shape):
        c = lattice_of(kind, shape, spacing, 30 + k)
        rec, n, spp, Gc = check_record(hip, F, M, c, spacing, A, bins, "%s %s" % (shape, name))
        some = some or Gc.any()
        if name == "partly outside":
            assert 0 < n < F.size
        if name == "outside":
            assert n == 0 and spp == 0.0 and not Gc.any()
            raw = rec.cpu().numpy()
            assert not raw[:2].any() and not raw[4:4 + Gc.size].any()    # n, S_pp and Gc: all-zero bytes
    assert some
    c = lattice_of("random", shape, spacing, 30 + k)
    check_record(hip, F, M, c, spacing, rotating(shape), 19, "%s narrow range" % (shape,), rm=NARROW)


@pytest.mark.parametrize("nx", [64, 1])
@pytest.mark.parametrize("masked", [False, True])
def test_record_every_instantiation(hip, nx, masked):
    """k_ffd_mi_force<LINEAR, MASKED>: tests/sampling_cases.py's ffd construction (nx == 1: the lattice's x channel and
    A's x row are zero, so the coordinate is exactly 0), with masks and without"""
    fshape, mshape, spacing = ((5, 6, 70), (6, 5, 64), (7, 3, 2)) if nx >= 2 else ((4, 6, 64), (5, 6, 1), (5, 2, 3))
    c = sc.case("ffd", fshape, mshape, wf=masked, wm=masked, spacing=spacing, seed=60 + nx + masked)
    assert sc.selection_key("ffd", c) == ("ffd", 2 if nx >= 2 else 1, masked)
    d = sc.build(c)
    _, n, spp, Gc = check_record(hip, d.F, d.M, d.lattice, spacing, d.A, 19, "nx %d masked %s" % (nx, masked),
                                 WF=d.WF, WM=d.WM)
    assert 0 < n and (not masked or n < d.F.size) and spp > 0 and Gc.any()


def test_more_tiles_than_workgroups_and_calls_repeat(hip):
    """tests/test_ffd.py's grid-cap shape: a second, partial pass over the tiles, for the histogram and the evaluation"""
    G = hip.SIMILARITY_GRID
    ty = int(np.ceil(np.sqrt(G + 1)))
    tz = -(-(G + 1) // ty)
    shape = (TILE[0] * (tz - 1) + 1, TILE[1] * (ty - 1) + 1, 2)
    assert G < ty * tz < 2 * G
    spacing = (2, 16, 16)
    F, M = volumes(shape, (shape[0] - 3, shape[1] + 2, 3), 3)
    c = random_lattice(shape, spacing, 7, 0.5)
    field = fr.field(c, spacing, shape, None)
    hist, count = check_hist(hip, F, M, field, 19, "grid cap")
    assert count > 0
    check_record(hip, F, M, c, spacing, None, 19, "grid cap")
    W = am.measures(hist).W
    Fd, Md, cd, ud = dev(F), dev(M), dev(c), dev(field)
    h0, c0 = hip.parzen_histogram_field(Fd, Md, ud, 19, RF, RM)
    h1, c1 = hip.parzen_histogram_field(Fd, Md, ud, 19, RF, RM)
    assert h0.cpu().numpy().tobytes() == h1.cpu().numpy().tobytes() and int(c0[0]) == int(c1[0]) == count
    r0, g0, _ = hip.ffd_mi_evaluate(Fd, Md, cd, spacing, W, RF, RM, None, 0.01)
    r1, g1, _ = hip.ffd_mi_evaluate(Fd, Md, cd, spacing, W, RF, RM, None, 0.01)
    assert np.array_equal(r0.cpu().numpy(), r1.cpu().numpy()) and np.array_equal(g0.cpu().numpy(), g1.cpu().numpy())


# ---- the driver ------------------------------------------------------------------------------------------------------
def run_driver(api, moving, fixed, **kw):
    return api.refine_ffd(moving, fixed, None, DRIVER["spacing"], DRIVER["levels"], DRIVER["bending"], metric="mi",
                          bins=DRIVER["bins"], max_evaluations=DRIVER["max_evaluations"], **kw)


@pytest.fixture(scope="module")
def device_driver(api):
    fixed, moving, _, _ = driver_pair()
    return run_driver(api, dev(moving), dev(fixed))


def test_driver_against_the_restatement(api, hip, device_driver):
    """The device's summation order may flip one accept / reject (tests/test_ffd.py's margins, for the same reason):
    the RMS field error is at most 1.5 x the restatement's and the mutual information gained on level 0 at least half
    of what the restatement gained.  The last accepted cost is the host routine's value on the device's own histogram
    through the final field: the same integers through the same routine, so equal."""
    fixed, moving, _, truth = driver_pair()
    ref, rms_ref = restatement_driver()
    r = device_driver
    assert type(r).__name__ == "MiFFDRefinement" and r.bins == DRIVER["bins"]
    trail = [tuple(e) for e in r.trail]
    rms, gain, gain_ref = rms_error(r.field.cpu().numpy(), truth), level0_gain(trail), level0_gain(ref.trail)
    print("device mi driver: stop %s, %d evaluations, RMS %.4g (restatement %.4g), mi gain on level 0 %.4g "
          "(restatement %.4g)" % (r.stop, len(trail), rms, rms_ref, gain, gain_ref))
    check_trail(trail, DRIVER["levels"], DRIVER["max_evaluations"], DRIVER["bending"])
    assert r.stop in ("converged", "evaluations", "flat", "failed")
    assert rms <= 1.5 * rms_ref
    assert gain >= 0.5 * gain_ref
    assert r.jacobian.folded == 0
    last = [e for e in trail if e[6] == 0 and e[5]][-1]
    hist, count = hip.parzen_histogram_field(dev(fixed), dev(moving), r.field, DRIVER["bins"], fm.own_range(fixed),
                                             fm.own_range(moving))
    at_end = hip.parzen_mi(hist)
    assert last[1] == at_end.cost and r.mi == at_end.mi and r.nmi == at_end.nmi and last[3] == int(count[0])
    assert tuple(r.lattice.shape) == fr.lattice_shape(fixed.shape, DRIVER["spacing"]) and r.spacing == (8, 8, 8)
    assert np.array_equal(r.field.cpu().numpy(), fr.field(r.lattice.cpu().numpy(), 8, fixed.shape))
    assert tuple(r.warped.shape) == fixed.shape


def test_driver_masks_and_inputs_agree(api, device_driver):
    """numpy input with the ranges spelt out equals tensor input; all-in masks give the unmasked trail"""
    fixed, moving, _, _ = driver_pair()
    a = device_driver
    b = run_driver(api, moving, fixed, range_fixed=fm.own_range(fixed), range_moving=fm.own_range(moving))
    c = run_driver(api, moving, fixed, mask_fixed=np.ones(fixed.shape, bool),
                   mask_moving=np.ones(moving.shape, np.float32))
    for other in (b, c):
        assert [tuple(e) for e in other.trail] == [tuple(e) for e in a.trail] and other.stop == a.stop
        assert np.array_equal(other.lattice.cpu().numpy(), a.lattice.cpu().numpy())
        assert (other.mi, other.nmi, other.bins) == (a.mi, a.nmi, a.bins)


def test_register_ffd_end_to_end(api):
    """register_ffd hands ffd_params=dict(metric="mi") to refine_ffd: tests/test_ffd_host.py's pair with the moving
    volume through the hump map of tests/test_affine_mi.py's end-to-end test (on this volume's values a decreasing
    map: the contrast is inverted), both stages driven by the mutual information"""
    F, M, _ = msd_driver_pair()
    mapped = ((M - np.float32(50.0)) ** 2 / np.float32(25.0)).astype(np.float32)
    r = api.register_ffd(mapped, F, levels=2, refine=dict(metric="mi"),
                         ffd_params=dict(metric="mi", max_evaluations=10))
    assert type(r.refinement).__name__ == "MiFFDRefinement"
    assert type(r.registration.refinement).__name__ == "MiAffineRefinement"
    assert r.refinement.stop in ("converged", "evaluations", "flat", "failed")
    assert r.refinement.trail[-1].level == 0 and tuple(r.refinement.field.shape) == (3,) + F.shape
    acc = [e.E for e in r.refinement.trail if e.level == 0 and e.accepted]
    assert all(b < a for a, b in zip(acc, acc[1:]))
    assert np.isfinite(r.refinement.mi) and r.refinement.mi == -[e for e in r.refinement.trail
                                                                 if e.level == 0 and e.accepted][-1].msd
