"""The FFD lattice kernels, the later sampling-core kernels and the field kernels on subnormal, flat and huge content
(-m gpu), against their existing restatements.

tests/test_registration_content.py stops where tests/registration_content.py says: it flushes "every intensity ... (the
coordinates, masks and lattice as they are)".  Here the class (pyramid_content.CLASSES, as they are) goes into the
control lattice (A), into the intensities of the sampling-core kernels that arrived after sampling_cases.MATRIX (B) and
into the displacement field (C).  The cases, the references and the fused models are in tests/deformation_content.py;
tests/test_deformation_content_host.py proves on the CPU that the cases can fail.  Measured there, as the smallest share
over both grids of the nonzero reference words that are subnormal / that a modelled flush changes:

    family                     subnormal       fade            faint_spikes
    ffd_field                  1.000 / 1.000   1.000 / 1.000   1.000 / 1.000
    ffd_field affine, x        1.000 / 1.000   1.000 / 1.000   1.000 / 1.000
    ffd_refine2                1.000 / 1.000   0.999 / 1.000   1.000 / 1.000
    field_exp, K = 3           1.000 / 1.000   0.840 / 0.883   1.000 / 1.000
    field_invert, N = 2        1.000 / 1.000   0.841 / 0.841   1.000 / 1.000

the share of the nonzero words that a modelled fused multiply-add changes (ffd_value: s = fma(wz, wy * (wx * c), s);
sub_mix: fma(6, v1, v0)), which is 0 in every underflow class (the running sum lies on the subnormal grid), so that
the two defect models need different classes:

    model, grid                huge    integer  constant
    ffd_value  (5, 6, 70)      0.559   0.570    0.581
    ffd_value  (5, 7, 67)      0.573   0.549    0.415
    sub_mix    (5, 6, 70)      0.289   0.000    0.838
    sub_mix    (5, 7, 67)      0.307   0.000    0.875

and for the other families: A5 (root_tiny): 1278 of 2100 voxels counted, every gradient word nonzero, 0.995 of them
subnormal and changed by a flushed cast, gmax 1.49e-38; parzen_histogram_field: a flush moves at least 0.879 of the
counted voxels of `subnormal` and 0.827 of `fade` to another cell (the fixed bin and the moving sample's fixed-point
window weights); similarity_batch: 0.736 and 0.573; ffd_bending, ffd_mi_evaluate and ffd_evaluate_channels: a flush of
the inputs moves a sum beyond its gamma bound in every case of every underflow class; `collapsed`: 140 of 2100 and 67
of 2345 determinants are -0.0, the others +0.0.

Purpose-built inputs: `root_tiny` (base * 2**-60: the products of two samples underflow float, not double, so that
k_ffd_combine's (float) of a double rounds into the subnormal range) and `collapsed` (x channel exactly -x, y and z
channels integers of y and z only: every determinant is +0.0 or -0.0, both occur).

Shapes: fixed (5, 6, 70) and moving (6, 5, 64) at spacing (7, 3, 2); the odd pair is fixed (5, 7, 67) at spacing
(8, 3, 2), not the (4, 3, 2) first proposed: at (4, 3, 2) the lattice is [3, 6, 6, 20], long enough for
registration_content.content to give `fade` its normal corner, and only 0.454 of the field's words are subnormal; at
(8, 3, 2) it is [3, 6, 6, 12] and the share is 1.000.  The spacing was changed, the condition was not.  A moving grid
with nx = 1 wherever a kernel has a LINEAR == 1 instantiation.

Left out on purpose: k_ffd_step (c - a * grad, unfused) is reachable only through the refinement drivers, which start
from a zero lattice, and no entry point is added for it.  The landmark term (A4) is double arithmetic on the widened
lattice and cannot underflow; it is pinned word for word all the same.  The Jacobian penalty (C4) cannot tell a flushed
field from the field: 1 + g is exactly 1 for a subnormal g, so what is asserted there is the expected values (phi and S
all zero; `collapsed` on the polynomial branch at r = +-0; `huge` finite in double)."""
import numpy as np
import pytest

from tests import deformation_content as dc
from tests import ffd_landmarks_restatement as lr
from tests import ffd_restatement as fr
from tests import field_restatement as fld
from tests import registration_content as rc
from tests import test_sampling_matrix as tm
from tests.demons_restatement import gamma

pytestmark = pytest.mark.gpu
F = np.float32
QUIET = dc.QUIET
dev = tm.dev


@pytest.fixture(scope="module")
def hip():
    import torch
    from sift3d_amd import api, hip as h
    if not torch.cuda.is_available() or not api.device_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    h.lib()
    return h


def carved(shape, align=0):
    return tm.Carved(shape, align)


def check_words(wrong, what, got, want):
    msg = rc.same_words(got, want)
    if msg:
        wrong.append("%s: %s" % (what, msg))


def collect(wrong, what, fn, *args):
    """run a comparison of another test file, keeping its failure beside the others'"""
    try:
        with np.errstate(**QUIET):
            return fn(*args)
    except AssertionError as e:
        wrong.append("%s: %s" % (what, str(e)[:600]))
    return None


def done(wrong):
    assert not wrong, "%d comparisons fail\n  %s" % (len(wrong), "\n  ".join(wrong))


# ----------------------------------------------------------------------------------------------------------------------
# A. the lattice as content
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [False, True], ids=["spline", "affine"])
def test_ffd_field(hip, affine):
    """k_ffd_field<AFFINE>: ffd_value is "float, unfused, x innermost, from +0".  With the affine the x row is the exact
    identity row, so that the x channel is (float)(+0.0) + the spline"""
    wrong = []
    for shape, spacing in dc.GRIDS:
        A = dc.identity_x_affine(shape) if affine else None
        for cls in dc.CLASSES:
            lat = dc.lattice(cls, shape, spacing)
            with np.errstate(**QUIET):
                want = dc.field_reference(lat, spacing, shape, A)
            out = carved((3,) + shape)
            hip.ffd_field(dev(lat), spacing, out.view, A)
            check_words(wrong, "k_ffd_field %s %s" % (cls, shape), out.numpy(), want)
            assert out.intact(), (cls, shape)
    done(wrong)


def test_ffd_refine2(hip):
    """k_ffd_refine2: sub_mix is ((v0 + 6 v1) + v2) * 0.125f in float, unfused"""
    wrong = []
    for shape, spacing in dc.GRIDS:
        for cls in dc.CLASSES:
            coarse = dc.coarse_lattice(cls, shape, spacing)
            with np.errstate(**QUIET):
                want = dc.refine2_reference(coarse, shape, spacing)
            got = hip.ffd_refine2(dev(coarse), shape, spacing).cpu().numpy()
            check_words(wrong, "k_ffd_refine2 %s %s" % (cls, shape), got, want)
    done(wrong)


def test_ffd_bending(hip):
    """tests/test_ffd.py's comparisons of R and dR; `constant` has no second derivative: R is 0.0 and dR has no nonzero
    word"""
    wrong = []
    for shape, spacing in dc.GRIDS:
        for cls in dc.CLASSES:
            lat = dc.lattice(cls, shape, spacing)
            R, dR = hip.ffd_bending(dev(lat), spacing)
            Rw, dRw, Rt, dRt = dc.bending_reference(lat, spacing)
            what = "ffd_bending %s %s" % (cls, shape)
            print("%s: R %.9g (off %.3g)" % (what, R, abs(R - Rw)))
            if not abs(R - Rw) <= gamma(6 * 40 + lat.size) * Rt:
                wrong.append("%s: R %r, want %r" % (what, R, Rw))
            if not np.all(np.abs(dR - dRw) <= gamma(200) * dRt):
                wrong.append("%s: dR off by %r" % (what, float(np.abs(dR - dRw).max())))
            if cls == "constant":
                assert R == 0.0 and not np.ascontiguousarray(dR).view(np.uint64).any(), what
            else:
                assert R > 0 and dR.any(), what
    done(wrong)


@pytest.mark.parametrize("affine", [False, True], ids=["spline", "affine"])
def test_ffd_points_and_landmarks(hip, affine):
    """mapped points and residuals word for word, S, Omega and GL to tests/test_ffd_landmarks.py's gamma bounds"""
    from tests.test_ffd_landmarks import check_landmarks, same_bits
    wrong = []
    for shape, spacing in dc.GRIDS:
        A = dc.identity_x_affine(shape) if affine else None
        for cls in dc.CLASSES:
            lat, P, Q, w = dc.landmark_case(cls, shape, spacing)
            what = "ffd_points %s %s" % (cls, shape)
            with np.errstate(**QUIET):
                want, inside = lr.points(lat, spacing, P, A)
            got = hip.ffd_points(dev(lat), spacing, P, A).cpu().numpy()
            if not same_bits(got, want):
                bad = np.argwhere((got.view(np.int64) != want.view(np.int64)) & ~(np.isnan(got) & np.isnan(want)))
                wrong.append("%s: %d words differ, first at %r" % (what, len(bad), bad[:1].tolist()))
            assert inside.any() and not inside.all(), what
            rec = collect(wrong, "ffd_landmarks %s %s" % (cls, shape), check_landmarks, hip, lat, spacing, P, Q, w, A,
                          "%s %s" % (cls, shape))
            assert rec is None or 20 <= rec[0].counted < len(P), what
    done(wrong)


@pytest.mark.parametrize("jacobian", [None, 0.3], ids=["plain", "jacobian"])
@pytest.mark.parametrize("lam", [0.0, dc.LANDMARK_TINY], ids=["no_landmarks", "landmarks"])
def test_gradient_cast_rounds_into_the_subnormal_range(hip, lam, jacobian):
    """k_ffd_combine<JAC, LM> ends in (float) b of a double: on `root_tiny` intensities (2 / n) Gc is of order 1e-38 and
    the cast rounds onto the subnormal grid.  d_grad from the device's own Gc, dR, GJ, GL and Omega
    (tests/test_ffd_landmarks.py's test_gradient_bit_for_bit_from_the_device_sums), word for word (-0.0 is not +0.0),
    and gmax equal; Gc against the restatement to tests/test_ffd.py's bound.  The bending and landmark weights are
    2**-125 and 2**-124, so that their terms stay beside (2 / n) Gc; the penalty's weight 0.3 makes its term of order 1,
    which swallows the rest: that instantiation's cast is an ordinary one"""
    d = dc.cast_case()
    c, cvox = d.lattice, int(np.prod(d.lattice.shape[1:]))
    want, _, _, _ = dc.cast_reference(d)
    runs = [hip.ffd_evaluate_landmarks(dev(d.F), dev(d.M), dev(c), d.spacing, d.P, d.Q, None, lam, None, dc.BEND_TINY,
                                       jacobian)]
    if jacobian is None and lam == 0.0:
        runs.append(hip.ffd_evaluate(dev(d.F), dev(d.M), dev(c), d.spacing, None, dc.BEND_TINY) + (None, None))
    for rec, grad, _, lm, jac in runs:
        n, see, R, gmax, Gc, dR = hip.ffd_record(rec, c.shape)
        assert n == want.n, (n, want.n)
        bound = np.array([gamma(int(k) + 8) for k in want.support.reshape(-1)]).reshape(want.support.shape)
        off = np.abs(Gc - want.Gc)
        assert np.all(off <= bound * want.Gc_terms), (off.max(), (off - bound * want.Gc_terms).max())
        assert abs(see - want.see) <= gamma(d.F.size + 8) * want.see_terms, (see, want.see)
        g = (2.0 / np.float64(n)) * Gc + dc.BEND_TINY * dR
        if jacobian:
            g = g + (jacobian / np.float64(d.F.size)) * jac.cpu().numpy()[4:4 + 3 * cvox].reshape(c.shape)
        if lam > 0:
            counted, S, Om, rmax = hip.ffd_landmarks_record(lm)
            GL = lm.cpu().numpy()[4:4 + 3 * cvox].reshape(c.shape)
            assert counted == len(d.P) and Om > 0 and GL.any()
            g = g + ((lam * 2.0) / Om) * GL
        g = g.astype(F)
        got = grad.cpu().numpy()
        sub = rc.share(rc.is_subnormal(got), got != 0)
        print("k_ffd_combine<%s, %s>: n %d gmax %.9g, subnormal share of the nonzero gradient words %.3f"
              % (bool(jacobian), lam > 0, n, gmax, sub))
        msg = rc.same_words(got, g)
        assert msg is None, "k_ffd_combine<%s, %s>: %s" % (bool(jacobian), lam > 0, msg)
        assert gmax == float(np.abs(g).max()), (gmax, float(np.abs(g).max()))
        if not jacobian:
            assert sub >= 0.5, sub


# ----------------------------------------------------------------------------------------------------------------------
# B. the sampling-core kernels that arrived after the matrix
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("nx1", [False, True], ids=["linear", "nx1"])
def test_parzen_histogram_field(hip, nx1, masked):
    """k_parzen_hist<LINEAR, MASKED, FIELD = true>: histogram and count bit for bit"""
    from tests.test_ffd_mi import check_hist
    wrong = []
    for cls in dc.CLASSES:
        c, d = dc.hist_field_case(cls, nx1, masked)
        rng = rc.range_of(cls, c.bins)
        got = collect(wrong, "k_parzen_hist field %s" % cls, check_hist, hip, d.F, d.M, d.field, c.bins, cls, rng, rng,
                      d.WF, d.WM)
        assert got is None or got[1] >= 8, cls
    done(wrong)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("nx1", [False, True], ids=["linear", "nx1"])
def test_ffd_mi_evaluate(hip, nx1, masked):
    """k_ffd_mi_force<LINEAR, MASKED> with the table W of the restatement's histogram: tests/test_ffd_mi.py's
    check_record (the count exact, S_pp and Gc to their gamma bounds, the gradient from the device's own sums)"""
    from tests.test_ffd_mi import check_record
    wrong = []
    for cls in dc.CLASSES:
        c, d = dc.mi_case(cls, nx1, masked)
        rng = rc.range_of(cls, c.bins)
        got = collect(wrong, "k_ffd_mi_force %s" % cls, check_record, hip, d.F, d.M, d.lattice, c.spacing, d.A, c.bins,
                      cls, rng, rng, d.WF, d.WM)
        assert got is None or got[1] >= 8, cls
    done(wrong)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("linear", [2, 1], ids=["linear", "nx1"])
def test_ffd_evaluate_channels(hip, linear, masked):
    """k_ffd_force_channels<LINEAR, MASKED> at nc = 2: tests/test_ffd_channels.py's check_channels (the field, the count
    and the force S bit for bit, S_ee and Gc to their gamma bounds)"""
    from tests.test_ffd_channels import check_channels
    wrong = []
    for cls in dc.CLASSES:
        d = dc.channels_case(cls, linear, masked)
        got = collect(wrong, "k_ffd_force_channels %s" % cls, check_channels, hip, d.F, d.M, d.lattice, d.spacing, d.A,
                      d.WF, d.WM, cls)
        assert got is None or got[2] >= 8, cls
        if cls == "constant" and got is not None:
            assert got[3] == 0.0 and not got[4].any()                    # no residual: S_ee and Gc are 0.0
    done(wrong)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("nx1", [False, True], ids=["linear", "nx1"])
def test_similarity_batch(hip, nx1, masked):
    """k_similarity_batch on K = 3 maps (the identity, a rotation, one wholly outside): byte for byte three
    hip.similarity calls, which tests/test_registration_content.py pins on these classes.  `constant` puts every counted
    voxel into one cell: every wave takes the branch of commit() in which all its counted lanes hold one bin and adds
    popcount(live) once, which noise with 5 or more bins essentially never takes"""
    wrong = []
    for cls in dc.CLASSES:
        d = dc.batch_case(cls, nx1, masked)
        rng = rc.range_of(cls, dc.BINS)
        Fd, Md = dev(d.F), dev(d.M)
        masks = dict(mask_fixed=dev(d.WF), mask_moving=dev(d.WM)) if masked else {}
        for interp in ("linear", "nearest"):
            single = [hip.similarity(Fd, Md, a, dc.BINS, rng, rng, interp, **masks) for a in d.A]
            wh = np.array([h.cpu().numpy() for h, s in single])
            ws = np.array([s.cpu().numpy() for h, s in single])
            counts = [hip.similarity_stats(s)[0] for h, s in single]
            assert counts[0] >= 64 and counts[1] >= 64 and counts[2] == 0, (cls, interp, counts)
            for bins in (0, dc.BINS):
                hist, stats = hip.similarity_batch(Fd, Md, d.A, bins, rng, rng, interp, **masks)
                what = "k_similarity_batch %s %s bins %d" % (cls, interp, bins)
                if stats.cpu().numpy().tobytes() != ws.tobytes():
                    wrong.append("%s: the records differ from similarity's" % what)
                if bins:
                    got = hist.cpu().numpy()
                    if got.tobytes() != wh.tobytes():
                        k = np.argwhere(got != wh)[0].tolist()
                        wrong.append("%s: the histograms differ, first at %r: got %d, want %d"
                                     % (what, k, got[tuple(k)], wh[tuple(k)]))
                    if cls == "constant":
                        for k in range(2):
                            assert np.count_nonzero(got[k]) == 1 and int(got[k].max()) == counts[k], (what, k, counts)
                        assert not got[2].any(), what
                else:
                    assert hist is None
    done(wrong)


# ----------------------------------------------------------------------------------------------------------------------
# C. fields as content
# ----------------------------------------------------------------------------------------------------------------------
def test_jacobian_det(hip):
    """the determinant map word for word and the statistics; underflow classes: 1 + g is exactly 1, det is 1.0f; `huge`:
    +-inf, none NaN; `collapsed`: every det +-0.0, every voxel folded, min / max -0.0 / +0.0 bit for bit (fkey puts -0
    just below +0)"""
    wrong = []
    for shape, _ in dc.GRIDS:
        n = int(np.prod(shape))
        for cls in dc.FIELD_CLASSES:
            u = dc.field_of(cls, shape)
            with np.errstate(**QUIET):
                want = fld.ref_jacobian_det(u)
            wf, wmn, wmx = fld.ref_stats(want)
            det = carved(shape)
            _, folded, mn, mx = hip.jacobian_det(dev(u), det.view)
            what = "k_jacobian_det %s %s" % (cls, shape)
            check_words(wrong, what, det.numpy(), want)
            assert det.intact(), what
            assert (folded, mn, mx) == (wf, wmn, wmx), (what, (folded, mn, mx), (wf, wmn, wmx))
            assert hip.jacobian_det(dev(u))[1:] == (folded, mn, mx), what          # det not written: the same stats
            if cls in dc.UNDERFLOW_CLASSES:
                assert folded == 0 and mn == mx == 1.0, (what, folded, mn, mx)
            elif cls == "huge":
                assert mn == -np.inf and mx == np.inf and 0 < folded < n, (what, folded, mn, mx)
            elif cls == "collapsed":
                assert folded == n and mn == 0.0 and mx == 0.0, (what, folded, mn, mx)
                assert np.signbit(mn) and not np.signbit(mx), (what, mn, mx)
    done(wrong)


@pytest.mark.parametrize("K", [0, 3])
def test_field_exp(hip, K):
    """k_field_scale halves a subnormal K times (ties to even on the subnormal grid), then K compositions"""
    wrong = []
    for shape, _ in dc.GRIDS:
        for cls in dc.CLASSES:
            v = dc.field_of(cls, shape, 1)
            with np.errstate(**QUIET):
                want = dc.exp_reference(v, K)
            out = carved((3,) + shape)
            hip.field_exp(dev(v), out.view, K)
            check_words(wrong, "field_exp K = %d %s %s" % (K, cls, shape), out.numpy(), want)
            assert out.intact(), (cls, shape)
    done(wrong)


def test_field_invert(hip):
    wrong = []
    for shape, _ in dc.GRIDS:
        for cls in dc.CLASSES:
            u = dc.field_of(cls, shape, 1)
            with np.errstate(**QUIET):
                want = dc.invert_reference(u)
            w = carved((3,) + shape)
            w.view.zero_()
            hip.field_invert(dev(u), w.view, dc.INVERT_STEPS)
            check_words(wrong, "field_invert %s %s" % (cls, shape), w.numpy(), want)
            assert w.intact(), (cls, shape)
    done(wrong)


def test_jacobian_penalty_and_its_lattice_gradient(hip):
    """tests/test_jacobian_penalty.py's check (nonpos, rmin, rmax and S bit for bit, the sum to gamma(n + 8) sum |phi|)
    and its bound for GJ, on the fields of test_jacobian_det"""
    from tests import jacobian_penalty_restatement as jp
    from tests.test_jacobian_penalty import check
    wrong = []
    for shape, spacing in dc.GRIDS:
        n = int(np.prod(shape))
        for cls in dc.FIELD_CLASSES:
            u = dc.field_of(cls, shape)
            what = "k_jp_value %s %s" % (cls, shape)
            want = collect(wrong, what, check, hip, u, 1.0, what)
            if want is None:
                with np.errstate(**QUIET):
                    want = jp.penalty(u, 1.0)
            if cls in dc.UNDERFLOW_CLASSES:
                assert not want.phi.any() and not want.S.view(np.uint64).any() and want.nonpos == 0, what
            elif cls == "collapsed":
                assert want.nonpos == n and not want.r.any() and (want.phi == want.phi.flat[0]).all(), what
            elif cls == "huge":
                assert np.isfinite(want.sum) and np.isfinite(want.S).all(), what
            rec, GJ = hip.ffd_jacobian_gradient(dev(u), spacing, 1.0)
            nonpos, total, rmin, rmax = hip.jacobian_penalty_record(rec)
            assert (nonpos, rmin, rmax) == (want.nonpos, want.rmin, want.rmax), what
            GJ = GJ.cpu().numpy()
            for k in range(3):
                with np.errstate(**QUIET):
                    exact, terms, support = fr.adjoint(want.S[k], spacing)
                bound = np.array([gamma(int(s) + 8) for s in support.reshape(-1)]).reshape(support.shape) * terms
                if not np.all(np.abs(GJ[k] - exact) <= bound):
                    wrong.append("k_ffd_adjoint of S %s %s channel %d: off by %r" % (cls, shape, k,
                                                                                  float(np.abs(GJ[k] - exact).max())))
            if cls in dc.UNDERFLOW_CLASSES:
                assert not GJ.any(), what
    done(wrong)
