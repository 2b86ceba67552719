"""CPU twin of tests/test_registration_content.py: proves on the references alone, with no device, that its cases can
fail, so that a pass on the device cannot be vacuous.

Float-storing families (the warps, both composition modes, the prefilter, the B-spline warps, restrict, prolong, the
bracket), in each underflow class (subnormal, fade, faint_spikes): at least half of the nonzero reference words are
subnormal, and a modelled flush (pyramid_content.ftz on the inputs and on the output: what a kernel built to flush would
read and store) changes at least half of them.  The demons force is of order 0.5 whatever the scale of its inputs, so
only the second condition applies to it.  Reducing families: the reference on flushed inputs violates the device test's
own acceptance: at least half of the counted voxels change their histogram cell (similarity, parzen), n differs
(moments), a sum moves by more than its gamma bound (msd, ncc, mi, ffd).  `huge`: every reference output is finite.
The halves are conditions on the content, not measurements: a shape that misses them gets another shape or another
class parameter in tests/registration_content.py, never a lower threshold.  The measured minima are printed (pytest -s)
and recorded in the device file's docstring.

Also here: sampling_cases.build(c) is byte for byte what it was before it took `content`, and api._own_range's rule
against similarity_restatement.bin_scale."""
import collections

import numpy as np
import pytest

from tests import affine_mi_restatement as am
from tests import affine_ncc_restatement as an
from tests import mask_restatement as mr
from tests import registration_content as rc
from tests import sampling_cases as sc
from tests import similarity_restatement as sr
from tests.demons_restatement import gamma
from tests.test_similarity import volumes

F = np.float32
QUIET = dict(invalid="ignore", over="ignore", under="ignore", divide="ignore")


class Minima:
    """the smallest (subnormal share, changed share) per (family, class), printed at the end of a test"""

    def __init__(self):
        self.lo = collections.defaultdict(lambda: [1.0, 1.0])

    def add(self, family, cls, sub, dif, what):
        a = self.lo[family, cls]
        a[0], a[1] = min(a[0], sub), min(a[1], dif)
        assert sub >= 0.5, (what, cls, "subnormal share", sub)
        assert dif >= 0.5, (what, cls, "share a flush changes", dif)

    def show(self):
        for (family, cls), (sub, dif) in sorted(self.lo.items()):
            print("%-22s %-13s smallest share of subnormal words %.3f, of words a flush changes %.3f"
                  % (family, cls, sub, dif))


def cases_of(family):
    return [c for c in sc.MATRIX if c.family == family]


# ----------------------------------------------------------------------------------------------------------------------
# a. the sampling core
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sc.STORE_FAMILIES)
def test_store_families_reach_gradual_underflow(family):
    lo, words = Minima(), collections.Counter()
    for c in cases_of(family):
        for cls in rc.CLASSES:
            d = rc.matrix_data(c, cls)
            with np.errstate(**QUIET):
                want = rc.store_reference(c, d)
            assert np.isfinite(want).all(), (c, cls)                            # `huge` included
            if cls not in rc.UNDERFLOW_CLASSES:
                continue
            with np.errstate(**QUIET):
                flushed = rc.ftz(rc.store_reference(c, rc.flushed_data(d)))
            of = rc.unfilled(c, d, want) & (want != 0)
            # (faint_spikes is sparse: about 1 % of a few hundred voxels; the family's cases together have enough)
            if cls == "faint_spikes" and not (d.u if c.family == "compose" else d.M).any():
                continue                                    # 24 voxels hold no spike: signed zeros only
            assert np.count_nonzero(of) >= 1, (c, cls)
            words[cls] += int(np.count_nonzero(of))
            lo.add(family + ("" if family != "compose" else ", y and z channels"), cls,
                   rc.share(rc.is_subnormal(want), of), rc.share(rc.bits(want) != rc.bits(flushed), of), c)
    assert min(words[cls] for cls in rc.UNDERFLOW_CLASSES) >= 20, words
    lo.show()


def _cells(family, c, d, rng):
    """the histogram cell of every counted voxel, one row each: (b_f, b_m) of similarity; of parzen (b_f, k0 and the four
    fixed-point weights of the moving sample's window), which is what the voxel adds to its row of the histogram"""
    if family == "similarity":
        T = d.field if c.field else d.A
        Fv = np.ascontiguousarray(d.F, F)
        m, ins = sr.sample(d.M, T, Fv.shape, c.interp)
        ins = ins & mr.counted(mr.coords(T, Fv.shape), np.shape(d.M), d.WF, d.WM)
        return np.column_stack([sr.bin_of(Fv[ins], c.bins, *rng), sr.bin_of(m.astype(F)[ins], c.bins, *rng)])
    f, m = am._counted(d.F, d.M, d.A, d.WF, d.WM)[:2]
    win = am.window(m, rng[0], rng[1], c.bins)
    return np.column_stack([sr.bin_of(f, c.bins, *rng), win.k0, win.q])


@pytest.mark.parametrize("family", ["similarity", "parzen"])
def test_histogram_families_a_flush_moves_half_the_voxels(family):
    """every case, odd bin counts included: at least half of the counted voxels of `subnormal` and of `fade` add to
    another cell once F and M are flushed (the same voxels are counted: the coordinates do not change), and the
    histograms differ.  faint_spikes is sparse: 99 in 100 voxels are zeros of either sign, which a flush leaves where
    they are, so its condition is that the histogram changes in every case that has a spike among its counted samples"""
    least = {}
    for c in cases_of(family):
        for cls in rc.CLASSES:
            d, rng = rc.matrix_data(c, cls), rc.range_of(cls, c.bins)
            s = sr.bin_scale(c.bins, *rng)
            assert np.isfinite(s) and s > 0 and F(rng[0]) == rng[0] and F(rng[1]) == rng[1]
            e = rc.flushed_data(d)
            if family == "similarity":
                T = d.field if c.field else d.A
                h0, st = mr.joint(d.F, d.M, T, c.bins, rng, rng, c.interp, d.WF, d.WM)
                h1 = mr.joint(e.F, e.M, T, c.bins, rng, rng, c.interp, d.WF, d.WM)[0]
                n = st.count
                assert np.isfinite(st.sums).all(), (c, cls)
            else:
                h0, n, _ = am.histogram(d.F, d.M, d.A, c.bins, rng, rng, d.WF, d.WM)
                h1 = am.histogram(e.F, e.M, d.A, c.bins, rng, rng, d.WF, d.WM)[0]
            assert n == sc.counted(c, d)[0] and n >= 8, (c, cls, n)
            if cls in rc.UNDERFLOW_CLASSES:
                a, b = _cells(family, c, d, rng), _cells(family, c, e, rng)
                assert len(a) == len(b) == n
                moved = float(np.count_nonzero((a != b).any(axis=1))) / n
                if cls == "faint_spikes":
                    spike = (d.F != 0).any() and (d.M != 0).any() and c.mshape[2] > 1
                    assert moved or not spike, (c, cls)          # (the 24 voxels of a one-voxel-wide M hold no spike)
                    assert not moved or not np.array_equal(h0, h1), (c, cls)
                    key = "faint_spikes (voxels, all cases)"
                    least[key] = least.get(key, 0.0) + moved * n
                    continue
                least[cls] = min(least.get(cls, 1.0), moved)
                assert moved >= 0.5, (c, cls, moved)
                assert not np.array_equal(h0, h1), (c, cls)
    assert least["faint_spikes (voxels, all cases)"] >= 20, least
    for cls, v in sorted(least.items()):
        print("%-22s %-32s smallest share of counted voxels that a flush moves to another cell %.3f" % (family, cls, v))


def _beyond(got, want, terms, g):
    return bool(np.any(np.abs(np.asarray(got) - np.asarray(want)) > g * np.asarray(terms)))


@pytest.mark.parametrize("family", ["msd", "ncc", "mi", "ffd"])
def test_sum_families_a_flush_moves_a_sum_beyond_its_bound(family):
    hit = collections.defaultdict(list)
    for c in cases_of(family):
        for cls in rc.CLASSES:
            flush = cls in rc.UNDERFLOW_CLASSES
            if not flush and cls != "huge" and not (cls == "constant" and family in ("msd", "ncc", "mi")):
                continue
            d, rng = rc.matrix_data(c, cls), rc.range_of(cls, c.bins)
            e = rc.flushed_data(d)
            with np.errstate(**QUIET):
                if family == "msd":
                    w = mr.normal_equations(d.F, d.M, d.A, d.WF, d.WM)
                    finite = [w.see, w.b, w.H]
                    if cls == "constant":
                        assert w.n >= 8 and w.see == 0.0 and not w.b.any() and not w.H.any(), c
                    if flush:
                        x = mr.normal_equations(e.F, e.M, d.A, d.WF, d.WM)
                        g = gamma(w.n + 8)
                        moved = x.n != w.n or _beyond(x.see, w.see, w.see_terms, g) or \
                            _beyond(x.b, w.b, w.b_terms, g) or _beyond(x.H, w.H, w.H_terms, g)
                elif family == "ncc":
                    w = an.record(d.F, d.M, d.A, d.WF, d.WM)
                    finite = [getattr(w, k) for k in an.SUMS]
                    if cls == "constant":
                        # no variance in m: V_m = S_mm - S_m^2 / n is 0 but for the rounding of its three operations
                        # (the sums of float32(0.1) and of its square are not exact in double), of either sign
                        vm = w.S_mm - w.S_m * w.S_m / float(w.n)
                        assert w.n >= 8 and abs(vm) <= 4 * 2.0 ** -53 * w.S_mm, (c, vm)
                        assert an.fit(w) is None or vm > 0, c
                    if flush:
                        x = an.record(e.F, e.M, d.A, d.WF, d.WM)
                        g = gamma(w.n + 8)
                        moved = x.n != w.n or any(_beyond(getattr(x, k), getattr(w, k), w.terms[k], g) for k in an.SUMS)
                elif family == "mi":
                    W = am.measures(am.histogram(d.F, d.M, d.A, c.bins, rng, rng, d.WF, d.WM)[0]).W
                    w = am.record(d.F, d.M, d.A, W, c.bins, rng, rng, d.WF, d.WM)
                    finite = [w.see, w.b, w.H]
                    if cls == "constant":
                        # one fixed bin, one window: the table W is log 1, psi is 0 and M has no gradient
                        assert w.n >= 8 and not W.any() and w.see == 0.0 and not w.b.any() and not w.H.any(), c
                    if flush:
                        x = am.record(e.F, e.M, d.A, W, c.bins, rng, rng, d.WF, d.WM)
                        g = gamma(w.n + 11)
                        moved = x.n != w.n or _beyond(x.see, w.see, w.see_terms, g) or \
                            _beyond(x.b, w.b, w.b_terms, g) or _beyond(x.H, w.H, w.H_terms, g)
                else:
                    w, u, force = mr.evaluate(d.F, d.M, d.lattice, c.spacing, d.A, d.WF, d.WM)
                    finite = [w.see, w.Gc, force]
                    if flush:
                        x = mr.evaluate(e.F, e.M, d.lattice, c.spacing, d.A, d.WF, d.WM)[0]
                        moved = x.n != w.n or _beyond(x.see, w.see, w.see_terms, gamma(d.F.size + 8))
            assert w.n >= 8, (c, cls)
            assert all(np.isfinite(v).all() for v in finite), (c, cls)          # `huge` included
            if flush:
                hit[cls].append(bool(moved))
                if not moved:
                    print("%s %s>%s %s: a flush moves no sum beyond its bound" % (family, c.fshape, c.mshape, cls))
    # every underflow class moves a sum in every case of the family
    for cls in rc.UNDERFLOW_CLASSES:
        assert hit[cls] and all(hit[cls]), (family, cls, hit[cls])


def test_build_without_content_is_what_it_was():
    """three cases of the matrix: build(c) byte for byte the arrays it drew before it took `content` (the volumes of
    test_similarity.volumes, and the same stream for everything else), and `content` changes F, M and src alone"""
    picks = [cases_of("warp_field")[0], cases_of("compose")[-1], cases_of("ffd")[-1]]
    seen = 0
    for c in picks:
        d, e = sc.build(c), sc.build(c, rc.generator("huge"))
        Fv, M = volumes(c.fshape, c.mshape, c.seed)
        assert d.F.tobytes() == Fv.tobytes() and d.M.tobytes() == M.tobytes()
        if c.family == "warp_field":
            src = np.stack([M, (M * F(-0.5)).astype(F)]) if c.seed % 2 else M
            assert d.src.tobytes() == src.tobytes()
            assert e.src.shape == d.src.shape and e.src.reshape((-1,) + c.mshape)[0].tobytes() == e.M.tobytes()
        assert e.F.tobytes() == rc.content(c.fshape, "huge", c.seed).tobytes()
        assert e.M.tobytes() == rc.content(c.mshape, "huge", c.seed + 1).tobytes()
        for name, a in vars(d).items():
            b = getattr(e, name)
            if name in ("F", "M", "src"):
                continue
            seen += 1
            if a is None or isinstance(a, sc.TPS):
                assert (a is None and b is None) or all(np.array_equal(p, q) for p, q in zip(a, b)), name
            else:
                assert a.tobytes() == b.tobytes(), (c, name)
    assert seen >= 12


def test_small_fade_crosses_into_the_subnormal_range():
    for shape in ((4, 6, 1), (5, 6, 1)):
        v = rc.content(shape, "fade", 3)
        assert not rc.is_subnormal(v[0, 0, 0]) and v[0, 0, 0] != 0 and rc.is_subnormal(v).mean() > 0.5
    assert rc.content((4, 6, 60), "fade", 3).tobytes() == rc.pc.fade((4, 6, 60), 3).tobytes()


# ----------------------------------------------------------------------------------------------------------------------
# b. the kernels outside the matrix
# ----------------------------------------------------------------------------------------------------------------------
def test_bspline_reaches_gradual_underflow():
    lo = Minima()
    for cls in rc.CLASSES:
        vol, A, field = rc.bspline_case(cls)
        with np.errstate(**QUIET):
            want = rc.bspline_reference(vol, A, field)
        assert all(np.isfinite(w).all() for w in want), cls
        assert min(np.count_nonzero(w) for w in want[1:]) > 0.5 * want[1].size, cls     # the warps sample inside
        if cls in rc.UNDERFLOW_CLASSES:
            with np.errstate(**QUIET):
                flushed = rc.bspline_reference(vol, A, field, flush=True)
            for name, w, x in zip(("prefilter", "bspline_warp_affine", "bspline_warp_field"), want, flushed):
                lo.add(name, cls, *rc.underflow_shares(w, x), name)
    lo.show()


def test_demons_force_a_flush_changes_half_the_words():
    least = {}
    for cls in rc.CLASSES:
        for nc in (1, 2):
            for masked in (False, True):
                Fv, M, u, W, WF, WM = rc.force_case(cls, nc, masked)
                with np.errstate(**QUIET):
                    want, sd, ins = rc.force_reference(Fv, W, u, WF, WM)
                assert np.isfinite(want).all() and np.isfinite(sd).all(), cls
                assert 0 < ins.sum() < ins.size
                if cls == "constant":
                    assert not rc.bits(want).any()
                if cls in rc.UNDERFLOW_CLASSES:
                    with np.errstate(**QUIET):
                        x = rc.force_reference(Fv, W, u, WF, WM, flush=True)[0]
                    of = want != 0
                    assert np.count_nonzero(of) >= 20
                    dif = rc.share(rc.bits(want) != rc.bits(x), of)
                    least[cls] = min(least.get(cls, 1.0), dif)
                    assert dif >= 0.5, (cls, nc, masked, dif)
    for cls, v in sorted(least.items()):
        print("%-22s %-13s smallest share of nonzero delta words that a flush changes %.3f" % ("demons_force", cls, v))


def test_demons_iteration_adds_subnormals_in_quads_and_tail():
    for fixed in (rc.FIXED, rc.FIXED_ODD):
        n = 3 * int(np.prod(fixed))
        assert (n % 4 == 0) == (fixed == rc.FIXED)
        for cls in rc.CLASSES:
            Fv, M, _, _, _, _ = rc.force_case(cls, 1, False, fixed)
            u0 = rc.demons_start(cls, fixed)
            # (fade spans 30 octaves, the subnormal range 23: its faint end falls off the grid to zeros)
            assert rc.is_subnormal(u0[:2]).mean() > dict(faint_spikes=0.005, fade=0.15).get(cls, 0.9), cls
            with np.errstate(**QUIET):
                want, per = rc.demons_reference(Fv, M, u0)
            assert np.isfinite(want).all()
            sub = rc.is_subnormal(want).reshape(-1)
            # the sums u + delta that keep a subnormal: in the quads and (the odd shape) among the last n % 4 floats
            assert np.count_nonzero(sub) >= (8 if cls == "faint_spikes" else 100), (cls, int(sub.sum()))
            if cls == "constant":
                # delta is +0.0 everywhere: every word of the two channels is a kept subnormal, the last floats too
                assert rc.is_subnormal(want[:2]).all()


def test_transfers_and_bracket_reach_gradual_underflow():
    lo = Minima()
    for cls in rc.CLASSES:
        for shape in rc.TRANSFER_SHAPES:
            with np.errstate(**QUIET):
                want = rc.transfer_reference(cls, shape)
            for name in ("restrict", "restrict_half", "prolong"):
                assert np.isfinite(want[name]).all(), (cls, name)
            if cls in rc.UNDERFLOW_CLASSES:
                with np.errstate(**QUIET):
                    x = rc.transfer_reference(cls, shape, flush=True)
                for name in ("restrict", "restrict_half", "prolong"):
                    lo.add(name, cls, *rc.underflow_shares(want[name], x[name]), (name, shape))
        a, b = rc.bracket_case(cls)
        for mode in ("bracket", "bch1"):
            with np.errstate(**QUIET):
                want = rc.bracket_reference(a, b, mode)
            assert np.isfinite(want).all(), (cls, mode)
            if cls in rc.UNDERFLOW_CLASSES and mode == "bracket":
                # (bch1 adds b, of order 1, which swallows the bracket: it is run on the device, its share is not asked)
                lo.add("bracket", cls, *rc.underflow_shares(want, rc.bracket_reference(a, b, mode, flush=True)), mode)
    lo.show()


def test_moments_a_flush_changes_the_count():
    for cls in rc.CLASSES:
        for floor in rc.MOMENT_FLOORS:
            V, mask = rc.moments_case(cls, floor)
            for weight in ("binary", "intensity"):
                for m in (None, mask):
                    want = rc.moments_reference(V, floor, weight, m)
                    assert np.isfinite(want.sums).all(), (cls, floor, weight)
                    if cls in rc.UNDERFLOW_CLASSES:
                        # (faint_spikes: its positive spikes count, about 1 in 200 voxels, and a flush removes them)
                        x = rc.moments_reference(V, floor, weight, m, flush=True)
                        least = 5 if cls == "faint_spikes" else 100
                        assert x.n != want.n and want.n >= least, (cls, floor, weight, want.n, x.n)
                    if cls == "subnormal":
                        assert 0.4 < want.n / (V.size if m is None else mask.sum()) < 0.6
                        assert rc.moments_reference(V, floor, weight, m, flush=True).n == 0


# ----------------------------------------------------------------------------------------------------------------------
# the ranges
# ----------------------------------------------------------------------------------------------------------------------
def test_ranges_bin_the_classes_as_the_table_says():
    shape = (5, 6, 70)
    for B in (4, 7, 19, 64, 128):
        for cls in ("subnormal", "faint_spikes"):
            lo, hi = rc.range_of(cls, B)
            assert sr.bin_scale(B, lo, hi) == F(2.0 ** 126) and F(lo) == lo and F(hi) == hi
            v = rc.content(shape, cls, 1)
            b = sr.bin_of(v, B, lo, hi)
            # v - lo is a float sum: a negative sample fainter than half an ulp of lo (2**-145 for 128 bins) rounds away
            neg = v <= -F(2.0 ** -144)
            assert set(np.unique(b[neg])) == {B // 2 - 1} and set(np.unique(b[v >= 0])) == {B // 2}
            assert set(np.unique(b[v < 0])) <= {B // 2 - 1, B // 2} and neg.sum() > 0.9 * (v < 0).sum()
            assert set(np.unique(sr.bin_of(rc.ftz(v), B, lo, hi))) == {B // 2}
        for cls in rc.CLASSES:
            s = sr.bin_scale(B, *rc.range_of(cls, B))
            assert np.isfinite(s) and s > 0
    with np.errstate(over="ignore"):
        assert np.isinf(sr.bin_scale(64, *rc.natural_range(rc.content(shape, "subnormal", 1))))


def test_own_range_rule():
    """api._own_range: a range that the entries accept (bin_scale finite and positive, lo < hi as floats) and that
    contains [min, max]; today's pair wherever the entries accept today's pair; ValueError where max - min overflows"""
    import torch
    from sift3d_amd import api
    for bins in (2, 64, 128):
        for name, v in rc.own_range_volumes().items():
            lo, hi = api._own_range(torch.from_numpy(v), None, bins)
            flo, fhi = F(lo), F(hi)
            assert np.isfinite(flo) and np.isfinite(fhi) and flo < fhi, (name, lo, hi)
            with np.errstate(over="ignore"):
                s = sr.bin_scale(bins, lo, hi)
            assert np.isfinite(s) and s > 0, (name, bins, lo, hi, s)
            assert flo <= v.min() and v.max() <= fhi, (name, lo, hi)
            vlo, vhi = float(v.min()), float(v.max())
            old = (vlo, vhi) if vhi > vlo else (vlo, vlo + 1.0)
            with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
                s_old = sr.bin_scale(bins, *old)
            if F(old[0]) < F(old[1]) and np.isfinite(s_old) and s_old > 0:
                assert (lo, hi) == old, (name, bins)
            else:
                assert name in ("constant_big", "subnormal", "tiny_span"), name
            if name.startswith("constant"):
                assert flo == v.min()                                           # the constant falls into bin 0
    # ordinary volumes: today's pairs
    v = np.random.default_rng(1).normal(0, 1, (3, 4, 5)).astype(F)
    assert api._own_range(torch.from_numpy(v), None, 64) == (float(v.min()), float(v.max()))
    assert api._own_range(torch.from_numpy(np.full((2, 2, 2), 2.0, F)), None) == (2.0, 3.0)
    assert api._own_range(torch.from_numpy(v), (0, 1), 64) == (0.0, 1.0)
    # a constant at the top of the float range is widened downwards
    top = np.finfo(F).max
    lo, hi = api._own_range(torch.from_numpy(np.full((2, 2, 2), top, F)), None, 64)
    assert F(lo) < F(hi) == top and np.isfinite(sr.bin_scale(64, lo, hi))
    # a span above FLT_MAX, and a volume that is not finite
    wide = np.array([-3e38, 3e38], F).reshape(1, 1, 2)
    with pytest.raises(ValueError, match="wider than the largest float"):
        api._own_range(torch.from_numpy(wide), None, 64)
    with pytest.raises(ValueError, match="finite"):
        api._own_range(torch.from_numpy(np.array([0.0, np.inf], F).reshape(1, 1, 2)), None, 64)
