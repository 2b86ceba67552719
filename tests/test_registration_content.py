"""The registration kernels on subnormal, flat and huge content (-m gpu), against their existing restatements.

Every other test of this stack draws its intensities from noise of order 1, which cannot show a kernel that flushes
subnormals, a fused or reciprocal form that is not IEEE on tiny or huge operands, or an exact-zero path.  The classes
(pyramid_content.CLASSES), the range of the histogram entries per class, the arrays of every case and the references
are in tests/registration_content.py; tests/test_registration_content_host.py proves on the CPU that the cases can fail.
Measured there, as the smallest share of the nonzero reference words that are subnormal / that a modelled flush changes:

    family                  fade            subnormal, faint_spikes
    warp_affine             0.751 / 0.769   1.0 / 1.0
    warp_tps                0.744 / 0.744   1.0 / 1.0
    warp_field              0.746 / 0.746   1.0 / 1.0
    compose, y and z        0.800 / 0.800   1.0 / 1.0
    prefilter               0.985 / 0.999   0.995 / 1.0
    B-spline warps          1.0 / 1.0       1.0 / 1.0
    restrict (scale 1)      0.807 / 0.891   1.0 / 1.0
    restrict (scale 0.5)    0.829 / 0.875   1.0 / 1.0
    prolong                 0.559 / 0.617   1.0 / 1.0
    bracket                 0.827 / 0.886   1.0 / 1.0
    demons_force            - / 0.894       - / 1.0

and for the reducing families, with the ranges of registration_content.range_of (bins of 2**-126 with 0.0 on a bin
edge, for odd bin counts too): in every case a flush moves at least 0.601 of the counted voxels of `subnormal` and 0.551
of `fade` to another cell of similarity's histogram (0.841 and 0.873 of parzen's, where the cell is the fixed bin and
the moving sample's fixed-point window weights), it changes the histogram of every case of `faint_spikes` that counts a
spike, it changes the count of the moments, and it moves a sum of msd, ncc, mi and ffd beyond its gamma bound.

a. The sampling core: every case of sampling_cases.MATRIX (one per launcher choice) on every class, with the
   comparisons of tests/test_sampling_matrix.py: the stores word for word between intact guard bands, histograms and
   counts bit for bit with the class's range, sums to their gamma bounds.
b. The kernels outside that matrix: the B-spline prefilter and warps, the demons force and one iteration (the u += delta
   kernel on a field with subnormal channels, by its quads, its tail and its scalar path), restrict, prolong, the Lie
   bracket and the moments.
c. api.similarity with its own ranges on volumes whose min and max the entries refuse as they are (api._own_range)."""
import numpy as np
import pytest

from tests import affine_init_restatement as ai
from tests import registration_content as rc
from tests import sampling_cases as sc
from tests import test_sampling_matrix as tm
from tests.demons_restatement import gamma, ref_stats

pytestmark = pytest.mark.gpu
F = np.float32
QUIET = dict(invalid="ignore", over="ignore", under="ignore", divide="ignore")


@pytest.fixture(scope="module")
def hip():
    import torch
    from sift3d_amd import api, hip as h
    if not torch.cuda.is_available() or not api.device_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    h.lib()
    return h


dev = tm.dev


def carved(shape, align=0):
    return tm.Carved(shape, align)


def check_words(wrong, cls, what, got, want):
    msg = rc.same_words(got, want)
    if msg:
        wrong.append("%s %s: %s" % (cls, what, msg))


# ----------------------------------------------------------------------------------------------------------------------
# a. the sampling core
# ----------------------------------------------------------------------------------------------------------------------
def constant_extras(hip, c, d):
    """what `constant` gives exactly: no residual and no gradient, so S_ee (mi: S_pp, with a table W that is log 1), b
    and H are 0.0; no variance in m, so the NCC fit is the header's rule on the record's own V_m, which is 0 but for the
    rounding of the sums (of either sign); no force"""
    what = tm.ident(c)
    if c.family == "msd":
        n, see, b, H = hip.affine_normal_equations(dev(d.F), dev(d.M), d.A, mask_fixed=dev(d.WF), mask_moving=dev(d.WM))
        assert n >= 8 and see == 0.0 and not b.any() and not H.any(), (what, n, see)
    elif c.family == "mi":
        from tests import affine_mi_restatement as am
        rng = rc.range_of("constant", c.bins)
        W = am.measures(am.histogram(d.F, d.M, d.A, c.bins, rng, rng, d.WF, d.WM)[0]).W
        assert not W.any(), what
        n, spp, b, H = hip.affine_mi_normal_equations(dev(d.F), dev(d.M), d.A, W, rng, rng, mask_fixed=dev(d.WF),
                                                      mask_moving=dev(d.WM))
        assert n >= 8 and spp == 0.0 and not b.any() and not H.any(), (what, n, spp)
    elif c.family == "ncc":
        rec = hip.affine_ncc_normal_equations(dev(d.F), dev(d.M), d.A, mask_fixed=dev(d.WF), mask_moving=dev(d.WM))
        n = float(rec["n"])
        vm = float(rec["S_mm"]) - float(rec["S_m"]) * float(rec["S_m"]) / n
        assert n >= 8 and abs(vm) <= 2 * gamma(n + 8) * float(rec["S_mm"]), (what, vm)
        fit = hip.affine_ncc_fit(rec)
        print("%s constant: V_m %.3g, fit %r" % (what, vm, fit))
        assert (fit is None) == (not vm > 0), (what, vm, fit)
        assert not rec["u"].any() and not rec["v"].any() and not rec["w"].any() and not rec["H"].any(), what
    elif c.family == "ffd":
        from tests.test_masks import ffd_eval
        force = ffd_eval(hip, d.F, d.M, d.lattice, c.spacing, d.A, 0.01, d.WF, d.WM)[3]
        assert not np.asarray(force).any(), what


def run_matrix(hip, family):
    wrong = []
    for c in (c for c in sc.MATRIX if c.family == family):
        for cls in rc.CLASSES:
            d = rc.matrix_data(c, cls)
            try:
                with np.errstate(**QUIET):
                    tm.run_case(hip, c, identity=True, d=d, rng=rc.range_of(cls, c.bins))
                    if cls == "constant":
                        constant_extras(hip, c, d)
            except AssertionError as e:
                wrong.append("%s %s: %s" % (cls, tm.ident(c), str(e)[:600]))
    assert not wrong, "%d of the family's (case, class) pairs fail\n  %s" % (len(wrong), "\n  ".join(wrong))


@pytest.mark.parametrize("family", sc.FAMILIES)
def test_matrix_on_every_class(hip, family):
    run_matrix(hip, family)


@pytest.mark.parametrize("entry", ["similarity", "parzen_histogram"])
def test_natural_range_of_subnormal_content_is_refused(hip, entry):
    """its own min and max are about 1e-41 apart: bins / (hi - lo) overflows float (the contract's "so narrow that s
    overflows")"""
    c = [c for c in sc.MATRIX if c.family == "parzen" and c.mshape[2] > 1][0]
    d = rc.matrix_data(c, "subnormal")
    rng = rc.natural_range(d.F)
    assert rng[0] < 0 < rng[1] and rng[1] - rng[0] < 1e-40
    with pytest.raises(RuntimeError):
        if entry == "similarity":
            hip.similarity(dev(d.F), dev(d.M), d.A, 64, rng, rng)
        else:
            hip.parzen_histogram(dev(d.F), dev(d.M), d.A, 64, rng, rng)


# ----------------------------------------------------------------------------------------------------------------------
# b. the kernels outside that matrix
# ----------------------------------------------------------------------------------------------------------------------
def test_bspline_prefilter_and_warps(hip):
    wrong = []
    for cls in rc.CLASSES:
        vol, A, field = rc.bspline_case(cls)
        with np.errstate(**QUIET):
            want_coef, want_affine, want_field = rc.bspline_reference(vol, A, field)
        coef = carved(rc.PREFILTER_SHAPE)
        hip.bspline_prefilter(dev(vol), coef.view)
        check_words(wrong, cls, "prefilter", coef.numpy(), want_coef)
        # the warps from the reference's coefficients, so that each kernel answers for itself
        for name, want in (("bspline_warp_affine", want_affine), ("bspline_warp_field", want_field)):
            out = carved(rc.BSPLINE_OUT)
            if name == "bspline_warp_affine":
                hip.bspline_warp_affine(dev(want_coef), out.view, A, 0.0)
            else:
                hip.bspline_warp_field(dev(want_coef), out.view, dev(field), 0.0)
            check_words(wrong, cls, name, out.numpy(), want)
            assert out.intact(), (cls, name)
        assert coef.intact(), cls
    assert not wrong, "\n  ".join(wrong)


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("nc", [1, 2])
def test_demons_force(hip, nc, masked):
    wrong = []
    for cls in rc.CLASSES:
        Fv, M, u, W, WF, WM = rc.force_case(cls, nc, masked)
        with np.errstate(**QUIET):
            want, sd, ins = rc.force_reference(Fv, W, u, WF, WM)
        step = carved((3,) + rc.FIXED)
        stats = hip.demons_force(dev(Fv), dev(W), dev(u), step.view, 1.0, rc.MOVING, mask_fixed=dev(WF),
                                 mask_moving=dev(WM))
        s, n = hip.demons_stats(stats)
        got = step.numpy()
        check_words(wrong, cls, "delta", got, want)
        assert step.intact(), cls
        want_s, want_n = ref_stats(sd, ins)
        assert int(n[0]) == want_n, (cls, int(n[0]), want_n)
        assert abs(float(s[0]) - want_s) <= gamma(max(want_n, 1)) * want_s, (cls, float(s[0]), want_s)
        if cls == "constant":
            assert not rc.bits(got).any(), "constant: delta must be +0.0 everywhere, word for word"
    assert not wrong, "\n  ".join(wrong)


@pytest.mark.parametrize("fixed", [rc.FIXED, rc.FIXED_ODD], ids=["quads", "quads_and_tail"])
@pytest.mark.parametrize("align", [0, 1], ids=["aligned", "one_float_past"])
def test_demons_iteration_adds_subnormals(hip, fixed, align):
    """one iteration with both sigmas 0: warp, force, u += delta.  The field starts with subnormal x and y channels; it
    lies on a 16-byte boundary (k_field_add's quads, and the n % 4 floats behind them for the odd shape) or one float past
    one (its scalar path)"""
    wrong = []
    for cls in rc.CLASSES:
        Fv, M, _, _, _, _ = rc.force_case(cls, 1, False, fixed)
        u0 = rc.demons_start(cls, fixed)
        with np.errstate(**QUIET):
            want, per = rc.demons_reference(Fv, M, u0)
        field = carved((3,) + fixed, align)
        field.view.copy_(dev(u0))
        stats = hip.demons(dev(Fv), dev(M), field.view, 1, 1.0, 0.0, 0.0)
        s, n = hip.demons_stats(stats)
        check_words(wrong, cls, "field", field.numpy(), want)
        assert field.intact(), cls
        want_s, want_n = ref_stats(*per[0])
        assert int(n[0]) == want_n and abs(float(s[0]) - want_s) <= gamma(max(want_n, 1)) * want_s, (cls, s, n)
    assert not wrong, "\n  ".join(wrong)


@pytest.mark.parametrize("shape", rc.TRANSFER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restrict_and_prolong(hip, shape):
    from tests.multires_restatement import half_shape
    wrong = []
    for cls in rc.CLASSES:
        with np.errstate(**QUIET):
            ref = rc.transfer_reference(cls, shape)
        half = half_shape(shape)
        out = carved(half)
        hip.restrict2(dev(ref["vol"]), out.view, 1.0)
        check_words(wrong, cls, "restrict", out.numpy(), ref["restrict"])
        out3 = carved((3,) + half)
        hip.restrict2(dev(ref["fld"]), out3.view, 0.5)
        check_words(wrong, cls, "restrict 0.5", out3.numpy(), ref["restrict_half"])
        fine = carved((3,) + shape)
        hip.field_prolong2(dev(ref["coarse"]), fine.view)
        check_words(wrong, cls, "prolong", fine.numpy(), ref["prolong"])
        assert out.intact() and out3.intact() and fine.intact(), cls
    assert not wrong, "\n  ".join(wrong)


@pytest.mark.parametrize("mode", ["bracket", "bch1"])
def test_field_bracket(hip, mode):
    wrong = []
    for cls in rc.CLASSES:
        a, b = rc.bracket_case(cls)
        with np.errstate(**QUIET):
            want = rc.bracket_reference(a, b, mode)
        out = carved((3,) + rc.FIXED)
        hip.field_bracket(dev(a), dev(b), out.view, mode)
        check_words(wrong, cls, mode, out.numpy(), want)
        assert out.intact(), cls
    assert not wrong, "\n  ".join(wrong)


@pytest.mark.parametrize("weight", ["binary", "intensity"])
def test_moments(hip, weight):
    for cls in rc.CLASSES:
        for floor in rc.MOMENT_FLOORS:
            V, mask = rc.moments_case(cls, floor)
            for m in (None, mask):
                rec = hip.moments(dev(V), weight, floor, dev(m))
                want = ai.moments(V, floor, weight, m)
                what = (cls, floor, weight, m is not None)
                assert int(rec["n"]) == want.n, (what, int(rec["n"]), want.n)
                got = np.concatenate([[rec["S0"]], rec["S1"], rec["S2"]])
                bound = gamma(V.size + 8) * want.terms
                assert (np.abs(got - want.sums) <= bound).all(), (what, got - want.sums, bound)


# ----------------------------------------------------------------------------------------------------------------------
# c. api.similarity with its own ranges
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rc.own_range_volumes()))
def test_api_similarity_accepts_its_own_range(hip, name):
    from sift3d_amd import api
    v = rc.own_range_volumes()[name]
    for bins in (2, 64):
        r = api.similarity(v, v, bins=bins)
        assert r.count == v.size and int(r.joint.sum()) == v.size, (name, bins, r.count)
        assert r.msd == 0.0
        if name.startswith("constant"):
            assert int(r.joint[0, 0]) == r.count and r.mi == 0.0, (name, bins, r.mi)
            # the variance of a constant is exactly 0 where its sums are exact in double (a power of two: constant_big);
            # for float32(0.1) it is the rounding of S_ff - S_f^2 / n in whatever order the device adds, and the header
            # defines ncc from its sign, so nothing is asked of ncc there
            if name == "constant_big":
                assert r.ncc == 0.0, (name, bins, r.ncc)
        else:
            # both volumes fall into the same bins: the joint histogram is diagonal
            assert int(np.trace(r.joint)) == r.count, (name, bins)
    wide = np.array([-3e38, 3e38], F).reshape(1, 1, 2)
    with pytest.raises(ValueError, match="wider than the largest float"):
        api.similarity(wide, wide)
