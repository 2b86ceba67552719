"""GPU: every instantiation of the sampling core's kernels against its restatement, one hand-picked case per launcher
choice (tests/sampling_cases.py: MATRIX), with the comparisons of each family's own tests: histograms, counts, fields,
forces and warped volumes byte for byte, sums to gamma bounds (tests/test_similarity.py, tests/test_affine_refine.py,
tests/test_affine_ncc.py, tests/test_affine_mi.py, tests/test_ffd.py, tests/test_field_algebra.py).  The outputs of
the warps and of the composition sit between guard bands.  A masked instantiation is also run with all-ones masks,
whose bytes are the unmasked instantiation's.  Non-finite coordinates reach the kernels through fields only."""
import numpy as np
import pytest

from tests import affine_mi_restatement as am
from tests import affine_ncc_restatement as an
from tests import ffd_restatement as ffr
from tests import field_algebra_restatement as fa
from tests import field_restatement as fr
from tests import mask_restatement as mr
from tests import sampling_cases as sc
from tests.demons_restatement import gamma
from tests.test_masks import ffd_eval
from tests.test_warp import ref_warp
from tests.tps_restatement import ref_tps_warp

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL = 0x7FC0DEAD                                       # a quiet NaN with a payload
GUARD = 64                                                  # words before and after an output (a multiple of 4)


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ident(c):
    return "%s %s>%s" % ("-".join(str(v) for v in sc.selection_key(c.family, c)[1:]),
                         "x".join(map(str, c.fshape)), "x".join(map(str, c.mshape)))


def bits(got, want, what):
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


class Carved:
    """A float32 output of `shape` carved out of a larger buffer of sentinel words, `align` floats past a 16-byte
    boundary; intact() is whether every word before and after it still holds the sentinel"""

    def __init__(self, shape, align):
        import torch
        self.n = int(np.prod(shape))
        self.off = GUARD + int(align)
        self.buf = torch.full((self.off + self.n + GUARD + 4,), SENTINEL, dtype=torch.int32, device="cuda")
        self.view = self.buf[self.off:self.off + self.n].view(torch.float32).view(tuple(shape))
        assert self.view.data_ptr() % 16 == 4 * (int(align) % 4) and self.view.is_contiguous()

    def numpy(self):
        return self.view.cpu().numpy()

    def intact(self):
        b = self.buf.cpu().numpy()
        return bool(np.all(b[:self.off] == SENTINEL) and np.all(b[self.off + self.n:] == SENTINEL))


def masks_of(d, ones, c):
    if ones:
        return np.ones(c.fshape, F32), np.ones(c.mshape, F32)
    return d.WF, d.WM


# ---- one device run per family: returns the bytes that an all-ones run must repeat -----------------------------------
def run_store(hip, c, d):
    """the warps and the composition: the output byte for byte between intact guard bands"""
    what = ident(c)
    if c.family == "warp_affine":
        out = Carved(c.fshape, c.align)
        hip.warp_affine(dev(d.M), out.view, d.A, c.interp, sc.FILL)
        want = ref_warp(d.M, d.A, c.fshape, c.interp, sc.FILL)[0]
    elif c.family == "warp_tps":
        out = Carved(c.fshape, c.align)
        hip.warp_tps(dev(d.M), out.view, d.tps, c.interp, sc.FILL)
        want = ref_tps_warp(d.M, d.tps, c.fshape, c.interp, sc.FILL)[0]
    elif c.family == "warp_field":
        out = Carved(d.src.shape[:-3] + c.fshape, c.align)
        hip.warp_field(dev(d.src), out.view, dev(d.field), c.interp, sc.FILL)
        want = fr.ref_warp_field(d.src, d.field, c.interp, sc.FILL)
    else:
        out = Carved((3,) + c.fshape, c.align)
        st = hip.field_compose(dev(d.u), dev(d.v), out.view, c.mode, stats=True if c.stats else None)
        want, wst = fa.ref_compose(d.u, d.v, c.mode)
        if c.stats:
            s, m, n, i = (float(a[0]) if k < 2 else int(a[0]) for k, a in enumerate(hip.field_stats(st)))
            ws, wm, wn, wi = wst
            assert (n, i) == (wn, wi), (what, n, i, wn, wi)
            assert m == wm, (what, m, wm)
            assert s == ws or abs(s - ws) <= gamma(wn) * ws, (what, s, ws)    # == : an infinite sum (section 5)
        else:
            assert st is None
    bits(out.numpy(), want, what)
    assert out.intact(), what
    return None


def run_similarity(hip, c, d, ones=False, plain=False, rng=sc.RANGE):
    WF, WM = (None, None) if plain else masks_of(d, ones, c)
    T = d.field if c.field else d.A
    hist, stats = hip.similarity(dev(d.F), dev(d.M), dev(T) if c.field else T, c.bins, rng, rng, c.interp,
                                 mask_fixed=dev(WF), mask_moving=dev(WM))
    count, sums = hip.similarity_stats(stats)
    hist = hist.cpu().numpy()
    if not (ones or plain):
        what = ident(c)
        want_hist, want = mr.joint(d.F, d.M, T, c.bins, rng, rng, c.interp, WF, WM)
        np.testing.assert_array_equal(hist, want_hist.astype(np.int64), err_msg=what)
        assert count == want.count == int(want_hist.sum()), (what, count, want.count)
        for k, name in enumerate(("f", "m", "ff", "mm", "fm", "dd")):
            bound = gamma(max(count, 1)) * want.terms[k]
            assert abs(sums[k] - want.sums[k]) <= bound, (what, name, sums[k], want.sums[k], bound)
    return hist.tobytes(), stats.cpu().numpy().tobytes()


def run_msd(hip, c, d, ones=False, plain=False):
    WF, WM = (None, None) if plain else masks_of(d, ones, c)
    raw = hip.affine_normal_equations(dev(d.F), dev(d.M), d.A, raw=True, mask_fixed=dev(WF), mask_moving=dev(WM))
    if not (ones or plain):
        what = ident(c)
        n, see, b, H = hip.affine_normal_record(raw)
        want = mr.normal_equations(d.F, d.M, d.A, WF, WM)
        assert n == want.n, (what, n, want.n)
        assert np.array_equal(H, H.T), what
        g = gamma(n + 8)
        assert abs(see - want.see) <= g * want.see_terms, (what, "S_ee", see, want.see)
        assert np.all(np.abs(b - want.b) <= g * want.b_terms), (what, "b")
        assert np.all(np.abs(H - want.H) <= g * want.H_terms), (what, "H")
    return (raw.cpu().numpy().tobytes(),)


def run_ncc(hip, c, d, ones=False, plain=False):
    WF, WM = (None, None) if plain else masks_of(d, ones, c)
    raw = hip.affine_ncc_normal_equations(dev(d.F), dev(d.M), d.A, raw=True, mask_fixed=dev(WF), mask_moving=dev(WM))
    if not (ones or plain):
        what = ident(c)
        got = hip.affine_ncc_record(raw)
        want = an.record(d.F, d.M, d.A, WF, WM)
        assert int(got["n"]) == want.n, (what, int(got["n"]), want.n)
        assert np.array_equal(got["H"], got["H"].T), what
        g = gamma(want.n + 8)
        for name in an.SUMS:
            off = np.abs(np.asarray(got[name]) - np.asarray(getattr(want, name)))
            assert np.all(off <= g * np.asarray(want.terms[name])), (what, name, float(np.max(off)))
    return (raw.cpu().numpy().tobytes(),)


def run_parzen(hip, c, d, ones=False, plain=False, rng=sc.RANGE):
    WF, WM = (None, None) if plain else masks_of(d, ones, c)
    hist, count = hip.parzen_histogram(dev(d.F), dev(d.M), d.A, c.bins, rng, rng, mask_fixed=dev(WF),
                                       mask_moving=dev(WM))
    hist, count = hist.cpu().numpy(), int(count.cpu().numpy()[0])
    if not (ones or plain):
        what = ident(c)
        want, n, qsum = am.histogram(d.F, d.M, d.A, c.bins, rng, rng, WF, WM)
        np.testing.assert_array_equal(hist, want, err_msg=what)
        assert count == n, (what, count, n)
        assert int(hist.sum()) == qsum and abs(qsum - 65536 * n) <= 2 * n, what
    return hist.tobytes(), count


def run_mi(hip, c, d, ones=False, plain=False, rng=sc.RANGE):
    WF, WM = (None, None) if plain else masks_of(d, ones, c)
    W = am.measures(am.histogram(d.F, d.M, d.A, c.bins, rng, rng, d.WF, d.WM)[0]).W               # one table for all runs
    raw = hip.affine_mi_normal_equations(dev(d.F), dev(d.M), d.A, W, rng, rng, raw=True, mask_fixed=dev(WF),
                                         mask_moving=dev(WM))
    if not (ones or plain):
        what = ident(c)
        n, spp, b, H = hip.affine_normal_record(raw)
        want = am.record(d.F, d.M, d.A, W, c.bins, rng, rng, WF, WM)
        assert n == want.n, (what, n, want.n)
        assert np.array_equal(H, H.T), what
        g = gamma(want.n + 11)
        for name, got, ref, terms in (("S_pp", spp, want.see, want.see_terms), ("b", b, want.b, want.b_terms),
                                      ("H", H, want.H, want.H_terms)):
            off = np.abs(np.asarray(got) - np.asarray(ref))
            assert np.all(off <= g * np.asarray(terms)), (what, name, float(np.max(off)))
    return (raw.cpu().numpy().tobytes(),)


def run_ffd(hip, c, d, ones=False, plain=False):
    import torch
    WF, WM = (None, None) if plain else masks_of(d, ones, c)
    rec, grad, fld, force = ffd_eval(hip, d.F, d.M, d.lattice, c.spacing, d.A, 0.01, WF, WM)
    if not (ones or plain):
        what = ident(c)
        n, see, R, gmax, Gc, dR = hip.ffd_record(torch.from_numpy(rec), d.lattice.shape)
        want, u, wforce = mr.evaluate(d.F, d.M, d.lattice, c.spacing, d.A, WF, WM)
        assert np.array_equal(fld, u), what
        assert n == want.n, (what, n, want.n)
        assert np.array_equal(force, wforce), what
        assert abs(see - want.see) <= gamma(d.F.size + 8) * want.see_terms, (what, see, want.see)
        bound = np.array([gamma(int(k) + 8) for k in want.support.reshape(-1)]).reshape(want.support.shape)
        assert np.all(np.abs(Gc - want.Gc) <= bound * want.Gc_terms), what
        g, gm = ffr.gradient(want._replace(Gc=Gc), dR, 0.01)             # from the device's own sums: bit for bit
        assert np.array_equal(grad, g) and gmax == gm, what
    return tuple(a.tobytes() for a in (rec, grad, fld, force))


RUN = {"similarity": run_similarity, "msd": run_msd, "ncc": run_ncc, "parzen": run_parzen, "mi": run_mi, "ffd": run_ffd}


RANGED = ("similarity", "parzen", "mi")                      # the families whose run takes the bins' range


def run_case(hip, c, identity=False, d=None, rng=sc.RANGE):
    """One case on the device against its restatement.  identity: a masked case also with all-ones masks and with no
    masks, whose bytes must agree.  d: the case's arrays where they are not build(c)'s; rng: the range of the bins."""
    d = sc.build(c) if d is None else d
    # the restatements reach q through the identity map 1 * q + ((0 * y + 0 * z) + 0): with an infinite entry numpy
    # reports the 0 * inf (a NaN: outside, as the infinity is)
    with np.errstate(invalid="ignore" if c.nonfinite else "warn"):
        if c.family in sc.STORE_FAMILIES:
            return run_store(hip, c, d)
        kw = dict(rng=rng) if c.family in RANGED else {}
        RUN[c.family](hip, c, d, **kw)
        if identity and (c.wf or c.wm):
            ones, plain = RUN[c.family](hip, c, d, ones=True, **kw), RUN[c.family](hip, c, d, plain=True, **kw)
            assert ones == plain, ident(c)


def cases_of(cases, family):
    return [pytest.param(c, id=ident(c)) for c in cases if c.family == family]


# ---- the matrix: one parametrized test per family ----------------------------------------------------------------------
@pytest.mark.parametrize("c", cases_of(sc.MATRIX, "warp_affine"))
def test_warp_affine(hip, c):
    run_case(hip, c)


@pytest.mark.parametrize("c", cases_of(sc.MATRIX, "warp_tps"))
def test_warp_tps(hip, c):
    run_case(hip, c)


@pytest.mark.parametrize("c", cases_of(sc.MATRIX, "warp_field"))
def test_warp_field(hip, c):
    run_case(hip, c)


@pytest.mark.parametrize("c", cases_of(sc.MATRIX, "compose"))
def test_compose(hip, c):
    run_case(hip, c)


@pytest.mark.parametrize("c", cases_of(sc.MATRIX, "similarity"))
def test_similarity(hip, c):
    run_case(hip, c, identity=True)


@pytest.mark.parametrize("c", cases_of(sc.MATRIX, "msd"))
def test_msd_record(hip, c):
    run_case(hip, c, identity=True)


@pytest.mark.parametrize("c", cases_of(sc.MATRIX, "ncc"))
def test_ncc_record(hip, c):
    run_case(hip, c, identity=True)


@pytest.mark.parametrize("c", cases_of(sc.MATRIX, "parzen"))
def test_parzen_histogram(hip, c):
    run_case(hip, c, identity=True)


@pytest.mark.parametrize("c", cases_of(sc.MATRIX, "mi"))
def test_mi_record(hip, c):
    run_case(hip, c, identity=True)


@pytest.mark.parametrize("c", cases_of(sc.MATRIX, "ffd"))
def test_ffd_force(hip, c):
    run_case(hip, c, identity=True)


# ---- non-finite coordinates (NaN, +-inf, +-1e30 in a handful of field entries): such a voxel is outside; the
# composition gives NaN for a NaN and the clamped edge sample otherwise.  Every coordinate of these kernels passes
# taps_at's clamp (sift3d_resample.h) before an address is formed from it, mask_offset's included.
@pytest.mark.parametrize("c", [pytest.param(c, id=ident(c)) for c in sc.NONFINITE])
def test_non_finite_field_entries(hip, c):
    d = sc.build(c)
    fld = d.field
    assert np.isnan(fld).any() and np.isposinf(fld).any() and np.isneginf(fld).any() and (np.abs(fld) == F32(1e30)).any()
    run_case(hip, c, identity=True)
