"""CPU twin of tests/test_deformation_content.py: proves on the references alone, with no device, that its cases can
fail, so that a pass on the device cannot be vacuous.  The conditions are conditions on the content, not measurements:
a seed or shape that misses one gets another seed or shape in tests/deformation_content.py, never a lower threshold.
The measured figures are printed (pytest -s) and recorded in the device file's docstring; MEASURED below is that table.

A1, A2, C2, C3 (float stores): in each underflow class at least half of the nonzero reference words are subnormal, and a
    modelled flush (every float input and output of a kernel) changes at least half of them.
A1, A2 (contracts that say "unfused"): a modelled fused multiply-add changes at least a quarter of the nonzero words for
    at least two of huge, integer, constant.  In the underflow classes it changes none (the running sum lies on the
    subnormal grid, where fused equals unfused): the two defect models need different classes.
A5: at least half of the nonzero words of the restated gradient of `root_tiny` are subnormal, and a flushed cast changes
    a word.
A3, B2, B3: the restatement on flushed inputs moves a sum beyond the device test's own gamma bound.
B1, B4: a flush moves at least half of the counted voxels of `subnormal` and of `fade` to another histogram cell.
C1: `collapsed` holds determinants of both zero signs and nothing else; `huge` holds both infinities and no NaN.
C4: j = (d == e) + g is exactly the identity for a subnormal field, flushed or not, so no flush of a field can move the
    penalty: there the twin proves what the device test asserts instead (phi and S all zero; `collapsed` on the
    polynomial branch at r = +-0 with every voxel non-positive).

MEASURED (share of the nonzero reference words that are subnormal / that a modelled flush changes; smallest over the
cases of the family):
    see tests/test_deformation_content.py's docstring"""
import collections

import numpy as np
import pytest

from tests import affine_mi_restatement as am
from tests import deformation_content as dc
from tests import ffd_channels_restatement as fc
from tests import ffd_landmarks_restatement as lr
from tests import ffd_mi_restatement as fm
from tests import ffd_restatement as fr
from tests import field_restatement as fld
from tests import jacobian_penalty_restatement as jp
from tests import mask_restatement as mr
from tests import registration_content as rc
from tests import similarity_restatement as sr
from tests.demons_restatement import gamma

F = np.float32
QUIET = dc.QUIET


class Shares:
    """the smallest (subnormal share, changed share) per (family, class), asserted at least one half"""

    def __init__(self):
        self.lo = collections.defaultdict(lambda: [1.0, 1.0])

    def add(self, family, cls, want, flushed, what):
        assert np.count_nonzero(want) >= 20, (what, cls)
        sub, dif = rc.underflow_shares(want, flushed)
        a = self.lo[family, cls]
        a[0], a[1] = min(a[0], sub), min(a[1], dif)
        assert sub >= 0.5, (what, cls, "subnormal share", sub)
        assert dif >= 0.5, (what, cls, "share a flush changes", dif)

    def show(self):
        for (family, cls), (sub, dif) in sorted(self.lo.items()):
            print("%-22s %-13s smallest share of subnormal words %.3f, of words a flush changes %.3f"
                  % (family, cls, sub, dif))


def changed(a, b):
    """the share of a's nonzero words that differ in b"""
    return rc.share(rc.bits(a) != rc.bits(b), np.asarray(a) != 0)


def beyond(got, want, terms, g):
    return bool(np.any(np.abs(np.asarray(got) - np.asarray(want)) > g * np.asarray(terms)))


# ----------------------------------------------------------------------------------------------------------------------
# A. the lattice as content
# ----------------------------------------------------------------------------------------------------------------------
def test_field_and_refine2_reach_gradual_underflow_and_show_a_fused_form():
    lo, fused = Shares(), collections.defaultdict(dict)
    for shape, spacing in dc.GRIDS:
        for cls in dc.CLASSES:
            lat, coarse = dc.lattice(cls, shape, spacing), dc.coarse_lattice(cls, shape, spacing)
            with np.errstate(**QUIET):
                plain = dc.field_reference(lat, spacing, shape)
                affine = dc.field_reference(lat, spacing, shape, dc.identity_x_affine(shape))
                fine = dc.refine2_reference(coarse, shape, spacing)
                f_plain = dc.spline_fused(lat, spacing, shape)
                f_fine = dc.refine2_fused(coarse, shape, spacing)
            assert np.isfinite(plain).all() and np.isfinite(affine).all() and np.isfinite(fine).all(), cls
            # the identity row: the x channel of the affine field is the spline's, word for word
            assert rc.same_words(affine[0], plain[0]) is None, cls
            assert cls == "huge" or not np.array_equal(affine[1:], plain[1:])       # (huge swallows the rotation)
            fused["ffd_value", shape][cls] = changed(plain, f_plain)
            fused["sub_mix", shape][cls] = changed(fine, f_fine)
            if cls in dc.UNDERFLOW_CLASSES:
                with np.errstate(**QUIET):
                    lo.add("ffd_field", cls, plain, dc.field_reference(lat, spacing, shape, flush=True), shape)
                    x = dc.field_reference(lat, spacing, shape, dc.identity_x_affine(shape), flush=True)
                    lo.add("ffd_field affine, x", cls, affine[0], x[0], shape)
                    lo.add("ffd_refine2", cls, fine, dc.refine2_reference(coarse, shape, spacing, flush=True), shape)
    lo.show()
    for (what, shape), per in sorted(fused.items()):
        print("%-10s %-12s share of nonzero words a fused multiply-add changes: %s"
              % (what, shape, "  ".join("%s %.3f" % (c, per[c]) for c in dc.CLASSES)))
        assert sum(per[c] >= 0.25 for c in dc.FUSED_CLASSES) >= 2, (what, shape, per)


def test_bending_a_flush_moves_the_sums():
    for shape, spacing in dc.GRIDS:
        for cls in dc.CLASSES:
            lat = dc.lattice(cls, shape, spacing)
            R, dR, Rt, dRt = dc.bending_reference(lat, spacing)
            assert np.isfinite(R) and np.isfinite(dR).all(), cls
            if cls == "constant":
                assert R == 0.0 and Rt == 0.0 and not dR.view(np.uint64).any() and not dRt.any()
            else:
                assert R > 0 and dR.any(), cls
            if cls in dc.UNDERFLOW_CLASSES:
                Rx, dRx, _, _ = dc.bending_reference(lat, spacing, flush=True)
                assert abs(Rx - R) > gamma(6 * 40 + lat.size) * Rt, (cls, R, Rx)
                assert beyond(dRx, dR, dRt, gamma(200)), cls


def test_landmarks_count_and_stay_finite():
    """the landmark term is double arithmetic on the widened lattice: nothing of it can underflow (2**-149 is far inside
    the double range), so its cases are pinned by the word-for-word comparison of the mapped points and residuals; here:
    every class counts points, leaves some out, and gives finite sums and a gradient"""
    for shape, spacing in dc.GRIDS:
        for cls in dc.CLASSES:
            lat, P, Q, w = dc.landmark_case(cls, shape, spacing)
            with np.errstate(**QUIET):
                want = lr.landmarks(lat, spacing, P, Q, w, dc.identity_x_affine(shape))
            assert 20 <= want.counted < len(P), (cls, want.counted)
            assert np.isfinite(want.S) and np.isfinite(want.GL).all() and want.GL.any() and want.Omega > 0, cls


def test_the_gradient_cast_rounds_into_the_subnormal_range():
    d = dc.cast_case()
    rec, dR, g, gmax = dc.cast_reference(d)
    of = g != 0
    sub = rc.share(rc.is_subnormal(g), of)
    flushed = rc.ftz(g)
    print("A5 root_tiny: n %d of %d, nonzero gradient words %.3f, subnormal among them %.3f, gmax %.3g (flushed %.3g), "
          "words a flushed cast changes %.3f" % (rec.n, d.F.size, of.mean(), sub, gmax, float(np.abs(flushed).max()),
                                                 changed(g, flushed)))
    assert rec.n >= 0.4 * d.F.size and of.mean() >= 0.5
    assert sub >= 0.5
    assert rc.same_words(flushed, g) is not None


# ----------------------------------------------------------------------------------------------------------------------
# B. the sampling-core kernels that arrived after the matrix
# ----------------------------------------------------------------------------------------------------------------------
def parzen_cells(d, bins, rng):
    """what every counted voxel adds to the histogram: its fixed bin, k0 and the four fixed-point weights"""
    m, _, _, _, ins = fm._sampled(d.F, d.M, d.field, d.WF, d.WM)
    win = am.window(m[ins], rng[0], rng[1], bins)
    return np.column_stack([sr.bin_of(np.ascontiguousarray(d.F, F)[ins], bins, *rng), win.k0, win.q])


def test_histogram_field_a_flush_moves_half_the_voxels():
    least = {}
    for nx1 in (False, True):
        for masked in (False, True):
            for cls in dc.CLASSES:
                c, d = dc.hist_field_case(cls, nx1, masked)
                rng = rc.range_of(cls, c.bins)
                with np.errstate(**QUIET):
                    h0, n = fm.histogram_field(d.F, d.M, d.field, c.bins, rng, rng, d.WF, d.WM)
                assert n >= 8 and (not masked or n < d.F.size), (cls, nx1, masked, n)
                if cls in ("subnormal", "fade"):
                    e = rc.flushed_data(d)
                    a, b = parzen_cells(d, c.bins, rng), parzen_cells(e, c.bins, rng)
                    moved = float(np.count_nonzero((a != b).any(axis=1))) / n
                    least[cls] = min(least.get(cls, 1.0), moved)
                    assert moved >= 0.5, (cls, nx1, masked, moved)
                    assert not np.array_equal(h0, fm.histogram_field(e.F, e.M, d.field, c.bins, rng, rng, d.WF, d.WM)[0])
    for cls, v in sorted(least.items()):
        print("%-22s %-13s smallest share of counted voxels that a flush moves to another cell %.3f"
              % ("parzen_histogram_field", cls, v))


def test_mi_force_a_flush_moves_a_sum():
    for nx1 in (False, True):
        for masked in (False, True):
            for cls in dc.CLASSES:
                c, d = dc.mi_case(cls, nx1, masked)
                rng = rc.range_of(cls, c.bins)
                with np.errstate(**QUIET):
                    u = fr.field(d.lattice, c.spacing, c.fshape, d.A)
                    W = am.measures(fm.histogram_field(d.F, d.M, u, c.bins, rng, rng, d.WF, d.WM)[0]).W
                    w, _ = fm.evaluate(d.F, d.M, d.lattice, c.spacing, d.A, W, c.bins, (rng, rng), d.WF, d.WM)
                assert w.n >= 8 and np.isfinite(w.spp) and np.isfinite(w.Gc).all(), (cls, nx1, masked)
                if cls in dc.UNDERFLOW_CLASSES:
                    e = rc.flushed_data(d)
                    x, _ = fm.evaluate(e.F, e.M, d.lattice, c.spacing, d.A, W, c.bins, (rng, rng), d.WF, d.WM)
                    bound = np.array([gamma(int(k) + 9) for k in w.support.reshape(-1)]).reshape(w.support.shape)
                    moved = x.n != w.n or beyond(x.spp, w.spp, w.spp_terms, gamma(w.n + 11)) or \
                        bool(np.any(np.abs(x.Gc - w.Gc) > bound * w.Gc_terms))
                    assert moved, (cls, nx1, masked)


def test_channels_force_a_flush_moves_a_sum():
    for linear in (1, 2):
        for masked in (False, True):
            for cls in dc.CLASSES:
                d = dc.channels_case(cls, linear, masked)
                with np.errstate(**QUIET):
                    w, _ = fc.evaluate(d.F, d.M, d.lattice, d.spacing, d.A, d.WF, d.WM)
                assert w.n >= 8 and np.isfinite(w.see) and np.isfinite(w.S).all(), (cls, linear, masked)
                if cls == "constant":
                    assert w.see == 0.0 and not w.S.any()
                if cls in dc.UNDERFLOW_CLASSES:
                    with np.errstate(**QUIET):
                        x, _ = fc.evaluate(rc.ftz(d.F), rc.ftz(d.M), d.lattice, d.spacing, d.A, d.WF, d.WM)
                    assert x.n == w.n
                    assert beyond(x.see, w.see, w.see_terms, gamma(d.F.size + 8)), (cls, linear, masked)
                    # (the 30 voxels of a one-voxel-wide M hold no spike: no force, flushed or not)
                    assert not np.array_equal(x.S.view(np.uint64), w.S.view(np.uint64)) or \
                        (cls == "faint_spikes" and not w.S.any()), (cls, linear, masked)


def similarity_cells(d, A, interp, bins, rng):
    Fv = np.ascontiguousarray(d.F, F)
    m, ins = sr.sample(d.M, A, Fv.shape, interp)
    ins = ins & mr.counted(mr.coords(A, Fv.shape), np.shape(d.M), d.WF, d.WM)
    return np.column_stack([sr.bin_of(Fv[ins], bins, *rng), sr.bin_of(m.astype(F)[ins], bins, *rng)])


def test_similarity_batch_a_flush_moves_half_the_voxels_and_constant_fills_one_cell():
    least = {}
    for nx1 in (False, True):
        for masked in (False, True):
            for interp in ("linear", "nearest"):
                for cls in dc.CLASSES:
                    d = dc.batch_case(cls, nx1, masked)
                    rng = rc.range_of(cls, dc.BINS)
                    counts = []
                    for A in d.A:
                        hist, st = mr.joint(d.F, d.M, A, dc.BINS, rng, rng, interp, d.WF, d.WM)
                        counts.append(st.count)
                        if cls == "constant" and st.count:
                            assert np.count_nonzero(hist) == 1 and int(hist.max()) == st.count
                        if cls in ("subnormal", "fade") and st.count:
                            e = rc.flushed_data(d)
                            a, b = (similarity_cells(v, A, interp, dc.BINS, rng) for v in (d, e))
                            moved = float(np.count_nonzero((a != b).any(axis=1))) / st.count
                            least[cls] = min(least.get(cls, 1.0), moved)
                            assert moved >= 0.5, (cls, nx1, masked, interp, moved)
                    # the identity and the rotation count more than a wave's worth of voxels, the third map none
                    assert counts[0] >= 64 and counts[1] >= 64 and counts[2] == 0, (cls, nx1, masked, counts)
    for cls, v in sorted(least.items()):
        print("%-22s %-13s smallest share of counted voxels that a flush moves to another cell %.3f"
              % ("similarity_batch", cls, v))


# ----------------------------------------------------------------------------------------------------------------------
# C. fields as content
# ----------------------------------------------------------------------------------------------------------------------
def test_jacobian_fields_hold_what_the_device_test_expects():
    for shape, _ in dc.GRIDS:
        n = int(np.prod(shape))
        for cls in dc.FIELD_CLASSES:
            u = dc.field_of(cls, shape)
            with np.errstate(**QUIET):
                det = fld.ref_jacobian_det(u)
                pen = jp.penalty(u, 1.0)
            folded = fld.ref_stats(det)[0]
            if cls in dc.UNDERFLOW_CLASSES:
                assert (rc.bits(det) == rc.bits(F(1.0))).all() and folded == 0, cls
                # 1 + g is exactly 1: a flushed field gives the same Jacobian, the penalty cannot tell them apart
                assert not pen.phi.any() and not pen.S.view(np.uint64).any() and pen.nonpos == 0, cls
                assert rc.same_words(fld.ref_jacobian_det(rc.ftz(u)), det) is None
            elif cls == "huge":
                assert np.isposinf(det).any() and np.isneginf(det).any() and not np.isnan(det).any(), cls
                assert np.isinf(det).mean() > 0.9 and 0 < folded < n
                assert np.isfinite(pen.sum) and np.isfinite(pen.S).all() and 0 < pen.nonpos < n
            elif cls == "collapsed":
                neg = int(np.signbit(det).sum())
                print("collapsed %s: %d determinants are -0.0, %d are +0.0" % (shape, neg, n - neg))
                assert not det.any() and 20 <= neg <= n - 20 and folded == n
                assert not pen.r.any() and pen.nonpos == n
                t = -0.25                                       # the polynomial branch at r = +-0
                assert (pen.phi == (2.25 - 15.0 * t) + 64.0 * (t * t)).all() and pen.S.any()
            else:
                assert np.isfinite(det).all() and (cls == "constant" or 0 < folded < n), cls
                if cls == "constant":
                    assert (det == 1.0).all()


def test_exp_and_invert_reach_gradual_underflow():
    lo = Shares()
    for shape, _ in dc.GRIDS:
        for cls in dc.CLASSES:
            v = dc.field_of(cls, shape, 1)
            with np.errstate(**QUIET):
                e0, e3, w = dc.exp_reference(v, 0), dc.exp_reference(v, 3), dc.invert_reference(v)
            assert rc.same_words(e0, v) is None
            assert np.isfinite(e3).all() and np.isfinite(w).all(), cls
            if cls in dc.UNDERFLOW_CLASSES:
                with np.errstate(**QUIET):
                    lo.add("field_exp K = 3", cls, e3, dc.exp_reference(v, 3, flush=True), shape)
                    lo.add("field_invert N = 2", cls, w, dc.invert_reference(v, flush=True), shape)
    lo.show()
