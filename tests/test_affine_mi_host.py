"""CPU (not gpu): "Mutual-information affine refinement (Mattes)" (include/sift3d_amd.h) without a device.  The host
entries sift3d_amd_parzen_window and sift3d_amd_parzen_mi against the numpy restatement
(tests/affine_mi_restatement.py), every argument refusal of the device entries (which check their arguments before any
device call), the restatement's gradient against a finite difference of its cost, and the restatement's driver on the
pairs that tests/test_affine_mi.py runs on the device: it finds the true map under a non-monotone intensity map, where
the NCC driver has no optimum."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import affine_mi_restatement as am
from tests import affine_ncc_restatement as an
from tests import affine_refine_restatement as ar
from tests.test_affine_refine_host import TOL, _a, bufs, inverse  # noqa: F401  (bufs: a fixture)
from tests.test_warp import about_center, ref_warp, rot

U = 2.0 ** -53
BINS = 32
DRIVER_BOUND = 0.25                                         # voxels at the corners: see driver_case


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


# ---- the driver case -------------------------------------------------------------------------------------------------
_SOURCE = []


def source():
    """S: a 56^3 float32 sum of 40 Gaussians, scaled to a maximum of 100 (made once)"""
    if not _SOURCE:
        rng = np.random.default_rng(11)
        z, y, x = np.meshgrid(*(np.arange(56, dtype=np.float64),) * 3, indexing="ij")
        v = np.zeros((56, 56, 56))
        for _ in range(40):
            c = rng.uniform(0.05, 0.95, 3) * 55
            s = rng.uniform(0.06, 0.15) * 56
            a = rng.uniform(0.5, 1.5)
            v += a * np.exp(-((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) / (2 * s * s))
        _SOURCE.append((v * (100.0 / v.max())).astype(np.float32))
    return _SOURCE[0]


MAPS = {"hump": lambda m: (m - np.float32(50)) ** 2 / np.float32(25),          # not monotone on [0, 100]
        "linear": lambda m: np.float32(-0.5) * m + np.float32(10)}
_CASES = {}


def driver_case(kind, translation=False):
    """(fixed, moving, Tc): fixed = S[8:48]^3; moving = MAPS[kind] of the same crop of S pulled through the inverse of
    T = 1.03 rot((1, 2, 3), 3 degrees) about the volume's centre plus the shift (2, -1, 1) (translation=True: the shift
    alone); Tc is T in the crop's coordinates, the pull map fixed -> moving that the drivers should find.  The start,
    the identity, is 4.3 voxels from Tc at the corners (2.4 for the shift alone).  A 32-bin MI has its optimum a few
    hundredths of a voxel from Tc (the binning biases it), so a driver is held to DRIVER_BOUND = 0.25 voxel of Tc,
    about 3.5 times what a float64 prototype of this contract measured (0.067, 0.070, 0.023, 0.019), not to 10 TOL."""
    key = (kind, translation)
    if key not in _CASES:
        S = source()
        if translation:
            T = np.eye(3, 4)
            T[:, 3] = (2.0, -1.0, 1.0)
        else:
            T = about_center(1.03 * rot((1, 2, 3), 3.0), S.shape, S.shape, shift=(2.0, -1.0, 1.0))
        pulled = ref_warp(S, inverse(T), S.shape, "linear", 0.0)[0].astype(np.float32)
        crop = (slice(8, 48),) * 3
        moving = MAPS[kind](pulled[crop]).astype(np.float32)
        Tc = T.copy()
        Tc[:, 3] = T[:, :3] @ np.full(3, 8.0) + T[:, 3] - 8.0
        _CASES[key] = (np.ascontiguousarray(S[crop], np.float32), np.ascontiguousarray(moving), Tc)
    return _CASES[key]


def own_range(v):
    return float(v.min()), float(v.max())


_DRIVEN = {}


def driven(kind, translation):
    """the restatement driver's result on a driver case (made once; tests/test_affine_mi.py compares the device's)"""
    key = (kind, translation)
    if key not in _DRIVEN:
        fixed, moving, _ = driver_case(kind, translation)
        _DRIVEN[key] = am.refine(fixed, moving, bins=BINS, free_mask=0x888 if translation else 0xFFF,
                                 max_evaluations=60)
    return _DRIVEN[key]


# ---- symbols, sizes --------------------------------------------------------------------------------------------------
def test_symbols_exported_and_sizes_agree(hip):
    from sift3d_amd import _native, api
    L = _native.load()
    for name in ("sift3d_amd_parzen_window", "sift3d_amd_parzen_hist_work_bytes", "sift3d_hip_parzen_hist_affine",
                 "sift3d_amd_parzen_mi", "sift3d_hip_affine_mi_normal_eqs", "sift3d_amd_affine_mi_refine_work_bytes",
                 "sift3d_amd_affine_mi_refine_device"):
        assert hasattr(L, name), name
    for name in ("parzen_window", "parzen_histogram", "parzen_mi", "affine_mi_normal_equations", "affine_mi_refine"):
        assert callable(getattr(hip, name)), name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "sift3d_amd.h")).read()
    assert int(re.search(r"#define SIFT3D_AMD_PARZEN_MAX_BINS (\d+)", header).group(1)) == 64 == hip.PARZEN_MAX_BINS
    assert C.sizeof(hip.Similarity) == 64
    W = hip.lib().sift3d_amd_parzen_hist_work_bytes
    assert W(5, 6, 7) == hip.SIMILARITY_GRID * 8 == W(512, 512, 512)
    assert W(0, 6, 7) == 0 and W(5, -1, 7) == 0 and W(5, 6, 0) == 0
    R = hip.lib().sift3d_amd_affine_mi_refine_work_bytes
    slots = hip.lib().sift3d_amd_affine_normal_work_bytes(8, 8, 8)
    assert R(8, 8, 8, 8, 8, 8, 1) == slots + 1264 + 2 * 64 * 64 * 8 + 16        # record, hist + count, W
    assert R(8, 8, 8, 6, 6, 6, 2) == R(8, 8, 8, 6, 6, 6, 1) + 2 * (4 * 64 + 4 * 28)     # volumes, and room for masks
    assert R(8, 8, 8, 8, 8, 8, 0) == 0 and R(8, 8, 8, 8, 8, 8, 7) == 0 and R(8, 0, 8, 8, 8, 8, 1) == 0
    S = hip.lib().sift3d_amd_affine_refine_struct_bytes                        # nothing that existed changed its size
    assert [S(k) for k in range(7)] == [C.sizeof(hip.AffineRefineParams), C.sizeof(hip.AffineEvaluation),
                                        C.sizeof(hip.AffineRefineResult), 1264, 128, 6, 0]
    assert api.MiAffineRefinement._fields == ("A", "cost", "count", "accepted", "lambdas", "levels", "level_slices",
                                              "evaluations", "stop", "warped", "mi", "nmi", "bins")


# ---- the device entries refuse bad arguments before any device call --------------------------------------------------
BAD_BINS_AND_RANGES = [dict(bins=3), dict(bins=65), dict(bins=0), dict(rf=(1.0, 1.0)), dict(rf=(2.0, 1.0)),
                       dict(rm=(0.0, 0.0)), dict(rm=(1.0, -1.0)), dict(rf=(float("nan"), 1.0)),
                       dict(rf=(0.0, float("inf"))), dict(rm=(float("-inf"), 0.0)), dict(rm=(0.0, float("nan"))),
                       dict(rf=(-3e38, 3e38))]


def test_histogram_refusals(hip, bufs):  # noqa: F811
    L = hip.lib()
    F, M, R, W = bufs
    keep, ident = _a(np.eye(3, 4))
    hb, work = 64 * 64 * 8, hip.SIMILARITY_GRID * 8

    def call(F=F, o=(8, 8, 8), M=M, n=(8, 8, 8), A=ident, bins=64, rf=(0.0, 1.0), rm=(0.0, 1.0), H=R, Cn=R + 65536,
             W=W, WF=None, WM=None):
        return L.sift3d_hip_parzen_hist_affine(F, *o, M, *n, A, bins, *rf, *rm, H, Cn, W, None, WF, WM)
    cases = [dict(F=None), dict(M=None), dict(A=None), dict(H=None), dict(Cn=None), dict(W=None),
             dict(o=(0, 8, 8)), dict(o=(8, -1, 8)), dict(n=(8, 8, 0)),
             dict(F=F + 2), dict(M=M + 1), dict(H=R + 4), dict(Cn=R + 65536 + 4), dict(W=W + 4),
             dict(WF=F + 4096 + 2), dict(WM=M + 4096 + 1),
             dict(H=F), dict(H=M + 4 * 500), dict(Cn=F + 8), dict(W=M), dict(H=F + 4 * 512 - hb),           # on inputs
             dict(Cn=R + 8), dict(Cn=R + hb - 8), dict(H=W), dict(W=R + hb - 8), dict(W=R + 65536 - work + 8),
             dict(WF=R), dict(WM=R + 65536), dict(WF=W + work - 4),                                      # on the masks
             dict(o=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), F=F)] + BAD_BINS_AND_RANGES
    for kw in cases:
        assert call(**kw) == -1, kw
    for v in (np.nan, np.inf):
        A = np.eye(3, 4).reshape(12)
        A[7] = v
        kept, bad = _a(A)
        assert call(A=bad) == -1, v


def test_record_refusals(hip, bufs):  # noqa: F811
    L = hip.lib()
    F, M, R, W = bufs
    keep, ident = _a(np.eye(3, 4))
    tb, rb, work = 64 * 64 * 8, hip.AFFINE_NORMAL_BYTES, hip.affine_normal_work_bytes()

    def call(F=F, o=(8, 8, 8), M=M, n=(8, 8, 8), A=ident, bins=64, rf=(0.0, 1.0), rm=(0.0, 1.0), T=R + 131072,
             rec=R, W=W, WF=None, WM=None):
        return L.sift3d_hip_affine_mi_normal_eqs(F, *o, M, *n, A, bins, *rf, *rm, T, rec, W, None, WF, WM)
    cases = [dict(F=None), dict(M=None), dict(A=None), dict(T=None), dict(rec=None), dict(W=None),
             dict(o=(0, 8, 8)), dict(n=(8, 8, -2)),
             dict(F=F + 2), dict(M=M + 1), dict(T=R + 131072 + 4), dict(rec=R + 4), dict(W=W + 4), dict(WF=F + 4096 + 2),
             dict(rec=F), dict(rec=M + 4 * 500), dict(W=M), dict(rec=R + 131072), dict(rec=R + 131072 + tb - 8),
             dict(W=R + 131072 + tb - 8), dict(rec=W), dict(W=R + rb - 8), dict(WF=R), dict(WM=W + work - 4),
             dict(o=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), F=F)] + BAD_BINS_AND_RANGES
    for kw in cases:
        assert call(**kw) == -1, kw
    A = np.eye(3, 4).reshape(12)
    A[0] = np.nan
    kept, bad = _a(A)
    assert call(A=bad) == -1


def test_refine_device_refusals(hip, bufs):  # noqa: F811
    L = hip.lib()
    F, M, R, W = bufs
    res = hip.AffineRefineResult()
    sim = hip.Similarity()

    def call(F=F, o=(8, 8, 8), M=M, n=(8, 8, 8), A=np.eye(3, 4), bins=32, rf=(0.0, 1.0), rm=(0.0, 1.0),
             res=C.byref(res), sim=C.byref(sim), W=W, WF=None, WM=None, **kw):
        a, ptr = _a(A) if A is not None else (None, None)
        p = C.byref(hip.affine_refine_params(**kw))
        return L.sift3d_amd_affine_mi_refine_device(F, *o, M, *n, ptr, bins, *rf, *rm, p, res, sim, W, None, WF, WM)
    nan, inf = float("nan"), float("inf")
    bad_A = np.eye(3, 4)
    bad_A[1, 2] = nan
    need = L.sift3d_amd_affine_mi_refine_work_bytes(8, 8, 8, 8, 8, 8, 1)
    assert need <= 1 << 21
    cases = [dict(F=None), dict(M=None), dict(A=None), dict(res=None), dict(sim=None), dict(W=None),
             dict(o=(0, 8, 8)), dict(n=(8, 8, -1)), dict(A=bad_A),
             dict(free_mask=0), dict(free_mask=0x1000), dict(levels=0), dict(levels=7),
             dict(max_evaluations=0), dict(max_evaluations=129),
             dict(lambda0=0.0), dict(lambda0=nan), dict(lambda_factor=1.0), dict(lambda_factor=inf),
             dict(lambda_min=0.0), dict(lambda_max=1e-4), dict(lambda_max=inf), dict(tol=-1.0), dict(tol=nan),
             dict(min_overlap=-0.1), dict(min_overlap=1.5), dict(min_overlap=nan),
             dict(F=F + 2), dict(M=M + 1), dict(W=W + 4), dict(WF=R + 2), dict(W=F), dict(W=M + 4 * 511),
             dict(W=F - need + 8), dict(WF=W + need - 4), dict(WM=W)] + BAD_BINS_AND_RANGES
    for kw in cases:
        assert call(**kw) == -1, kw


def test_window_and_mi_refusals(hip):
    L = hip.lib()
    k0, out = C.c_int(), C.c_int()
    q, dw = (C.c_uint32 * 4)(), (C.c_double * 4)()
    ok = (0.5, 0.0, 1.0, 8, C.byref(k0), q, dw, C.byref(out))
    assert L.sift3d_amd_parzen_window(*ok) == 0
    for i in (4, 5, 6, 7):
        assert L.sift3d_amd_parzen_window(*(ok[:i] + (None,) + ok[i + 1:])) == -1, i
    for bins in (3, 65, -1):
        assert hip.parzen_window(0.5, 0.0, 1.0, bins) is None
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (np.nan, 1.0), (0.0, np.inf), (-3e38, 3e38)):
        assert hip.parzen_window(0.5, lo, hi, 8) is None
    h = np.ones((8, 8), np.uint64)
    sim = hip.Similarity()
    assert L.sift3d_amd_parzen_mi(h.ctypes.data, 8, C.byref(sim), None) == 0 and sim.n == 64     # W may be NULL
    assert L.sift3d_amd_parzen_mi(None, 8, C.byref(sim), None) == -1
    assert L.sift3d_amd_parzen_mi(h.ctypes.data, 8, None, None) == -1
    assert L.sift3d_amd_parzen_mi(h.ctypes.data, 3, C.byref(sim), None) == -1
    assert L.sift3d_amd_parzen_mi(h.ctypes.data, 65, C.byref(sim), None) == -1
    for bad in (np.ones((3, 3)), np.ones((65, 65)), np.ones((8, 9)), np.ones(8)):
        with pytest.raises(ValueError):
            hip.parzen_mi(bad)


# ---- the window: the library's one function against the restatement, bit for bit --------------------------------------
@pytest.mark.parametrize("bins", [4, 5, 32, 64])
@pytest.mark.parametrize("lo,hi", [(0.0, 100.0), (-3.25, 7.5), (10.0, 10.25)])
def test_window_against_restatement(hip, bins, lo, hi):
    """k0, q, dw and out on a thousand values: lo, hi, their neighbours in float32 on both sides, values outside the
    range, the bin edges and their neighbours, and random values.  The four weights are a partition of unity, so the
    sum of q is 65536 up to the four roundings to the grid (each at most 1/2): within 2."""
    lo, hi = np.float32(lo), np.float32(hi)
    rng = np.random.default_rng(bins)
    span = float(hi) - float(lo)
    edges = (float(lo) + span * np.arange(0, bins - 2) / (bins - 3)).astype(np.float32)
    vals = [lo, hi, np.nextafter(lo, np.float32(-np.inf)), np.nextafter(lo, np.float32(np.inf)),
            np.nextafter(hi, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf)),
            np.float32(float(lo) - span), np.float32(float(hi) + span), np.float32(-3e38), np.float32(3e38)]
    vals += list(edges) + list(np.nextafter(edges, np.float32(-np.inf))) + list(np.nextafter(edges, np.float32(np.inf)))
    vals += list(rng.uniform(float(lo) - 0.1 * span, float(hi) + 0.1 * span, 1000).astype(np.float32))
    vals = np.array(vals, np.float32)
    want = am.window(vals, lo, hi, bins)
    assert want.out.any() and not want.out.all() and set(np.unique(want.k0)) == set(range(bins - 3))
    for i, v in enumerate(vals):
        k0, q, dw, out = hip.parzen_window(v, lo, hi, bins)
        assert (k0, out) == (int(want.k0[i]), bool(want.out[i])), (v, k0, out)
        assert np.array_equal(q.astype(np.int64), want.q[i]), (v, q, want.q[i])
        assert dw.tobytes() == want.dw[i].tobytes(), (v, dw, want.dw[i])
        assert abs(int(q.sum()) - 65536) <= 2 and 0 <= k0 <= bins - 4 and q.max() <= 43691
    # in range the derivatives of the weights sum to 0 up to rounding: the partition of unity
    assert np.abs(want.dw.sum(axis=1)).max() <= 8 * U


# ---- the cost and the table ---------------------------------------------------------------------------------------------
def close(got, want, what):
    """within 8 u (1 + |value|): two logarithms that are each within 1 ulp and one division differ by that.  (The
    entropies are sums of up to B^2 such terms p log p with sum p = 1, each term below 1 / e in size.)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    ratio = np.abs(got - want) / (8 * U * (1 + np.abs(want)))
    assert np.all(ratio <= 1), (what, float(ratio.max()))


@pytest.mark.parametrize("kind,bins", [("hump", 32), ("linear", 19), ("hump", 64), ("linear", 4)])
def test_parzen_mi_against_restatement(hip, kind, bins):
    """On a histogram the restatement made: the total exactly, each entropy and each entry of W within 8 u (1 + |value|).
    If that bound on an entropy fails, the worst ratio is printed by `close`; tests/test_similarity_host.py allows the same
    formulas 1e-12 relative."""
    fixed, moving, Tc = driver_case(kind)
    hist, n, qsum = am.histogram(fixed, moving, np.eye(3, 4), bins, own_range(fixed), own_range(moving))
    assert n == fixed.size and int(hist.sum()) == qsum and hist.min() >= 0
    want = am.measures(hist)
    got = hip.parzen_mi(hist)
    assert got.n == want.n == qsum
    assert got.W.shape == (bins, bins) and np.array_equal(got.W == 0, want.W == 0)
    assert np.array_equal(want.W != 0, hist != 0) or np.all(want.W[(hist != 0) & (want.W == 0)] == 0)
    close(got.W, want.W, "W")
    for name in ("entropy_fixed", "entropy_moving", "entropy_joint", "mi", "nmi"):
        close(getattr(got, name), getattr(want, name), name)
    assert got.cost == -got.mi and 0 < got.mi <= min(got.entropy_fixed, got.entropy_moving) + 1e-12
    empty = hip.parzen_mi(np.zeros((bins, bins), np.int64))
    assert empty.n == 0 and np.isnan(empty.mi) and np.isnan(empty.nmi) and not empty.W.any()


# ---- the restatement against analysis ---------------------------------------------------------------------------------
def test_b_is_the_finite_difference_of_the_cost():
    """b / n = d cost / d theta at A = [I | (sqrt 2 - 1, sqrt 3 - 1, (sqrt 5 - 1) / 2 - 0.3)] on the hump pair, B = 32,
    by the central difference of cost = -mi through apply_delta with h = 1e-4 on the linear part and 1e-3 on the shift.
    Every fixed voxel but the last plane of each axis samples inside at A and at every perturbed map (39^3 voxels,
    asserted): a map that changes the overlap changes N, and the difference quotient of -mi is then wrong by tens of
    percent while the gradient is right.  -mi differs from the mean negative log-likelihood, whose gradient b / n is, by
    the entropy of the fixed marginal, which is constant while the counted set is.  Every component agrees within 1e-3
    of the largest (a float64 prototype measured 3e-5 of the largest)."""
    fixed, moving, _ = driver_case("hump")
    A = np.eye(3, 4)
    A[:, 3] = (np.sqrt(2.0) - 1, np.sqrt(3.0) - 1, (np.sqrt(5.0) - 1) / 2 - 0.3)
    rf, rm = own_range(fixed), own_range(moving)

    def cost(At):
        hist, n, _ = am.histogram(fixed, moving, At, BINS, rf, rm)
        assert n == 39 ** 3
        return am.measures(hist).cost
    hist, n, _ = am.histogram(fixed, moving, A, BINS, rf, rm)
    assert n == 39 ** 3
    rec = am.record(fixed, moving, A, am.measures(hist).W, BINS, rf, rm)
    assert rec.n == n
    grad = rec.b / n
    fd = np.zeros(12)
    for r in range(12):
        h = 1e-3 if r % 4 == 3 else 1e-4
        delta = np.zeros(12)
        delta[r] = h
        fd[r] = (cost(ar.apply_delta(A, delta, fixed.shape)) - cost(ar.apply_delta(A, -delta, fixed.shape))) / (2 * h)
    worst = np.abs(grad - fd).max()
    print("gradient", grad, "\ndifference", fd, "\nworst %.3g = %.3g of the largest" % (worst, worst / np.abs(fd).max()))
    assert worst <= 1e-3 * np.abs(fd).max()
    assert np.array_equal(rec.H, rec.H.T) and np.linalg.eigvalsh(rec.H).min() >= -100 * U * np.linalg.norm(rec.H)


# ---- the restatement's driver: the property the metric exists for --------------------------------------------------
@pytest.mark.parametrize("translation", [False, True])
@pytest.mark.parametrize("kind", ["hump", "linear"])
def test_driver_finds_the_map_under_an_unknown_intensity_map(kind, translation):
    """Measured on the restatement: full affine 0.067 (hump, 22 evaluations) and 0.070 (linear, 29) voxel from Tc,
    translation 0.023 and 0.019 (21 and 24 evaluations), all converged."""
    fixed, moving, Tc = driver_case(kind, translation)
    r = driven(kind, translation)
    err = ar.corner_distance(r.A, Tc, fixed.shape)
    hist = am.histogram(fixed, moving, Tc, BINS, own_range(fixed), own_range(moving))[0]
    print("%s %s: corner error %.3g after %d evaluations, stop %s; mi %.6f, at Tc %.6f"
          % (kind, "translation" if translation else "affine", err, r.evaluations, r.stop, r.measures.mi,
             am.measures(hist).mi))
    assert r.stop == "converged" and err <= DRIVER_BOUND
    acc = r.cost[r.accepted]
    assert np.all(np.diff(acc) < 0) and acc[-1] == -r.measures.mi
    if translation:
        np.testing.assert_array_equal(r.A[:, :3], np.eye(3))


def test_ncc_driver_on_the_hump_pair_for_information():
    """Where metric="ncc" ends on the hump pair: printed, nothing asserted about it (the map is not monotone, so the
    linear fit has no optimum at Tc)."""
    fixed, moving, Tc = driver_case("hump")
    r = an.refine(fixed, moving)
    print("ncc on the hump pair: %.3g voxels from Tc after %d evaluations, stop %s"
          % (ar.corner_distance(r.A, Tc, fixed.shape), r.evaluations, r.stop))


# ---- the Python interface ------------------------------------------------------------------------------------------------
def test_python_value_errors():
    from sift3d_amd import api
    v = np.zeros((5, 7, 9), np.float32)
    for kw in (dict(metric="bogus"), dict(metric=None), dict(metric="msd", bins=32), dict(metric="ncc", bins=32),
               dict(bins=16), dict(metric="ncc", range_fixed=(0.0, 1.0)), dict(range_moving=(0.0, 1.0)),
               dict(metric="mi", bins=3), dict(metric="mi", bins=65), dict(metric="mi", bins=8.5),
               dict(metric="mi", range_fixed=(1.0, 1.0)), dict(metric="mi", range_moving=(0.0, float("nan"))),
               dict(metric="mi", free="rigid"), dict(metric="mi", levels=0), dict(metric="mi", interp="nearest"),
               dict(metric="mi", bogus=1)):
        with pytest.raises(ValueError):
            api.refine_affine(v, v, **kw)
    if not api.device_available():
        with pytest.raises(RuntimeError):
            api.refine_affine(v, v, metric="mi")
