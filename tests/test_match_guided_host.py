"""CPU (not gpu): the host side of guided matching -- sift3d_hip_nn2_gated's refusals (before any device call) and
scratch size, sift3d_amd_spatial_order against its restatement, and two claims of the contract checked on the
restatement (tests/match_guided_restatement.py) alone: gap2 <= d2 for every pair of two blocks, in float32, and the
superset property of the guided decision."""
import ctypes as C

import numpy as np
import pytest

from tests import match_guided_restatement as gr
from tests import match_restatement as mr

F = np.float32


@pytest.fixture(scope="module")
def api():
    from sift3d_amd import api as a
    a.lib()
    return a


@pytest.fixture(scope="module")
def L(api):
    from sift3d_amd import hip
    return hip.lib()


# ---- sift3d_hip_nn2_gated: refusals and scratch size ------------------------------------------------------
BASE = 0x10000000                     # made-up, 256-byte aligned addresses: never dereferenced
GOOD = dict(A=BASE, nA=5, B=BASE + 0x100000, nB=7, dim=64, posA=BASE + 0x600000, posB=BASE + 0x700000, r2=4.0,
            permA=None, permB=None, j=BASE + 0x200000, d1=BASE + 0x300000, d2=BASE + 0x400000, vis=None,
            work=BASE + 0x500000)
ORDER = ("A", "nA", "B", "nB", "dim", "posA", "posB", "r2", "permA", "permB", "j", "d1", "d2", "vis", "work")


def _gated(L, **kw):
    a = dict(GOOD, **kw)
    return L.sift3d_hip_nn2_gated(*[a[k] for k in ORDER], None)


@pytest.mark.parametrize("bad", [
    # what sift3d_hip_nn2 refuses
    {"A": None}, {"B": None}, {"j": None}, {"d1": None}, {"d2": None}, {"work": None},
    {"nA": -1}, {"nB": -1}, {"nA": -5, "nB": -5},
    {"dim": 0}, {"dim": 16}, {"dim": 48}, {"dim": -32},
    {"A": BASE + 4}, {"B": BASE + 0x100000 + 4}, {"A": BASE + 8, "B": BASE + 0x100000 + 12},
    # and the gate's own
    {"posA": None}, {"posB": None}, {"posA": BASE + 0x600000 + 4}, {"posB": BASE + 0x700000 + 8},
    {"r2": -1.0}, {"r2": -1e-30}, {"r2": float("nan")}, {"r2": float("-inf")},
])
def test_nn2_gated_refuses_before_any_device_call(L, bad):
    assert _gated(L, nA=0, nB=0) == 0                # (the call itself is fine: nothing to compute)
    assert _gated(L, **bad) != 0
    assert L.sift3d_hip_last_error().decode() == "sift3d_hip_nn2_gated: invalid arguments"


def test_nn2_gated_empty_a_is_success_without_device(L):
    # nA = 0 without counters: nothing to compute, nothing written (every address is made up)
    for r2 in (0.0, 4.0, float("inf")):
        assert _gated(L, nA=0, r2=r2) == 0
    assert _gated(L, nA=0, nB=0, dim=1024, permA=BASE + 0x800000, permB=BASE + 0x900000) == 0


@pytest.mark.parametrize("na,nb", [(1, 1), (5, 1), (127, 129), (128, 128), (129, 257), (257, 130), (130, 2200),
                                   (128, 2049), (42501, 40000), (3, 0), (0, 9)])
def test_nn2_gated_work_floats(L, na, nb):
    """sift3d_hip_nn2's scratch, then 8 floats per 128-row block of either set"""
    want = na + nb + 8 + 3 * na * mr.runs(na, nb)[0] + 8 * (-(-na // 128) + -(-nb // 128))
    assert L.sift3d_hip_nn2_gated_work_floats(na, nb) == want
    assert L.sift3d_hip_nn2_gated_work_floats(na, nb) == L.sift3d_hip_nn2_work_floats(na, nb) \
        + 8 * (-(-na // 128) + -(-nb // 128))
    assert L.sift3d_hip_nn2_gated_work_floats(-4, -4) == 8


# ---- sift3d_amd_spatial_order -----------------------------------------------------------------------------
def _check_order(api, xyz, cell):
    got = api.spatial_order(xyz, cell)
    want = gr.spatial_order(xyz, cell)
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, want)
    assert sorted(got.tolist()) == list(range(len(np.asarray(xyz).reshape(-1, 3))))
    return got


def test_spatial_order_random_points(api):
    rng = np.random.default_rng(1)
    for n, cell in ((1000, 8.0), (777, 0.37), (300, 1e3), (64, np.inf)):
        p = rng.uniform(0, 200, (n, 3))
        got = _check_order(api, p, cell)
        if cell == np.inf or cell == 1e3:
            np.testing.assert_array_equal(got, np.arange(n))         # one cell: ties by index


def test_spatial_order_duplicates_and_negative_coordinates(api):
    rng = np.random.default_rng(2)
    p = rng.uniform(-300, 100, (500, 3))
    p[100:200] = p[:100]                              # exact duplicates: equal keys, by index
    p[250] = p[249] = [-0.0, 0.0, -1e-300]
    got = _check_order(api, p, 16.0)
    pos = np.empty(500, int)
    pos[got] = np.arange(500)
    assert (pos[100:200] > pos[:100]).all()
    # floor, not truncation: -0.5 and +0.5 lie in different cells, -0.5 and -0.9 in the same
    got = _check_order(api, np.array([[0.5, 0, 0], [-0.5, 0, 0], [-0.9, 0, 0], [0.9, 0, 0]]), 1.0)
    np.testing.assert_array_equal(got, [1, 2, 0, 3])


def test_spatial_order_morton_key(api):
    # the cells (x, y, z) of a 2 x 2 x 2 cube in Morton order: x is the lowest bit, then y, then z
    cells = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], float)
    rng = np.random.default_rng(3)
    shuffle = rng.permutation(8)
    got = _check_order(api, cells[shuffle] * 4.0 + 1.0, 4.0)
    np.testing.assert_array_equal(shuffle[got], np.arange(8))
    # clamped to 21 bits: cells beyond 2^21 - 1 share the last key and keep their index order
    far = np.array([[3e6, 0, 0], [2.5e6, 0, 0], [0.0, 0, 0], [2097151.0, 0, 0], [2097150.0, 0, 0]])
    np.testing.assert_array_equal(_check_order(api, far, 1.0), [2, 4, 0, 1, 3])


def test_spatial_order_non_finite_points_go_last(api):
    rng = np.random.default_rng(4)
    p = rng.uniform(-50, 50, (40, 3))
    p[7, 1] = np.nan
    p[3, 0] = np.inf
    p[30, 2] = -np.inf
    got = _check_order(api, p, 5.0)
    np.testing.assert_array_equal(got[-3:], [3, 7, 30])
    np.testing.assert_array_equal(_check_order(api, np.full((3, 3), np.nan), 5.0), [0, 1, 2])


def test_spatial_order_edges_and_refusals(api):
    assert len(_check_order(api, np.zeros((0, 3)), 2.0)) == 0
    np.testing.assert_array_equal(_check_order(api, [[5.0, -3.0, 1e9]], 2.0), [0])
    for cell in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError):
            api.spatial_order(np.zeros((4, 3)), cell)
    L = api.lib()
    perm = np.zeros(4, np.int32)
    assert L.sift3d_amd_spatial_order(np.zeros(12), -1, 1.0, perm) != 0


def test_matcher_guided_refusals_without_device(api):
    L = api.lib()
    L.sift3d_amd_matcher_match_guided.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p,
                                                  np.ctypeslib.ndpointer(np.float64), C.c_double, C.c_double,
                                                  C.c_double, np.ctypeslib.ndpointer(np.int32)]
    L.sift3d_amd_matcher_match_guided.restype = C.c_int
    a, b = api.DescriptorStore(), api.DescriptorStore()
    rng = np.random.default_rng(1)
    assert a.set(np.zeros((3, 4)), rng.random((3, 768), np.float32)) == 0
    assert b.set(np.zeros((4, 4)), rng.random((4, 768), np.float32)) == 0
    pred = np.zeros(9)
    # a made-up matcher: the arguments are refused before it is touched
    for radius, thr in ((0.0, 0.8), (-1.0, 0.8), (np.nan, 0.8), (4.0, 0.0), (4.0, -0.8)):
        out = np.full(3, 77, np.int32)
        assert L.sift3d_amd_matcher_match_guided(0x1000, a.h, b.h, pred, radius, thr, 0.0, out) != 0
        assert (out == 77).all()
    out = np.full(3, 77, np.int32)
    assert L.sift3d_amd_matcher_match_guided(None, a.h, b.h, pred, 4.0, 0.8, 0.0, out) != 0
    assert (out == 77).all()


# ---- the monotonicity claim of the block skip, in float32 ---------------------------------------------------
def test_gap2_never_exceeds_a_pair_distance():
    """2 000 random block pairs: for every pair of rows of the two blocks the gate's d2 >= the boxes' gap2, so
    gap2 > r2 implies d2 > r2 -- no epsilon.  Coordinates with all 24 mantissa bits in use, boxes that overlap on
    some axes, touch on others and lie far apart on the rest."""
    rng = np.random.default_rng(5)
    worst = np.inf
    for t in range(2000):
        scale = F(10.0) ** rng.integers(-2, 5)
        ca = rng.uniform(-1, 1, 3) * scale
        cb = ca + rng.uniform(-1, 1, 3) * scale * rng.choice([0.0, 0.01, 1.0, 30.0], 3)
        ea, eb = rng.uniform(0, 1, 3) * scale * 0.5, rng.uniform(0, 1, 3) * scale * 0.5
        pa = gr.pos4(ca + rng.uniform(-1, 1, (16, 3)) * ea)
        pb = gr.pos4(cb + rng.uniform(-1, 1, (16, 3)) * eb)
        if t % 7 == 0:
            pb[3, 1] = np.nan                          # stays out of the box; its pairs gate false anyway
        loA, hiA = gr.block_boxes(pa)
        loB, hiB = gr.block_boxes(pb)
        g2 = gr.gap2(loA, hiA, loB, hiB)[0, 0]
        d2 = gr.gate_d2(pa, pb)
        d2 = d2[~np.isnan(d2)]
        assert g2.dtype == np.float32 and d2.dtype == np.float32
        assert (d2 >= g2).all(), (t, g2, d2.min())
        if g2 > 0:
            worst = min(worst, float(d2.min() / g2))
    assert worst < 1.5                                 # (the bound is approached: the boxes are tight)


def test_gap2_of_empty_and_unbounded_boxes():
    inf = np.inf
    lo = np.array([[inf, inf, inf]], F)
    hi = np.array([[-inf, -inf, -inf]], F)
    box = (np.array([[0, 0, 0]], F), np.array([[1, 1, 1]], F))
    assert gr.gap2(lo, hi, *box)[0, 0] == inf                       # a block without a finite point: skipped
    assert gr.gap2(lo, hi, lo, hi)[0, 0] == inf
    assert gr.visited(gr.pos4([[np.nan, 0, 0]]), gr.pos4([[0, 0, 0]]), 5.0) == (0, 1)
    assert gr.visited(gr.pos4([[np.nan, 0, 0]]), gr.pos4([[0, 0, 0]]), np.inf) == (1, 1)     # inf > inf is false
    # a box reaching +inf against itself: inf - inf is dropped by fmax, the pair is visited
    assert gr.gap2(box[0], np.array([[inf, 1, 1]], F), box[0], np.array([[inf, 1, 1]], F))[0, 0] == 0


# ---- the superset property, on the restatement alone --------------------------------------------------------
def _descriptors(rng, na, nb, dim=64):
    """Random unit rows in clusters of look-alikes: the blind ratio test fails on many true partners"""
    base = np.abs(rng.standard_normal((na // 4 + 1, dim)))
    a = base[rng.integers(0, len(base), na)] + 0.05 * rng.standard_normal((na, dim))
    b = np.concatenate([a[:nb // 2] + 0.02 * rng.standard_normal((nb // 2, dim)),
                        base[rng.integers(0, len(base), nb - nb // 2)] + 0.05 * rng.standard_normal((nb - nb // 2, dim))])
    a, b = np.abs(a).astype(F), np.abs(b).astype(F)
    return a / np.linalg.norm(a, axis=1, keepdims=True), b / np.linalg.norm(b, axis=1, keepdims=True)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_superset_property_on_the_restatement(seed):
    rng = np.random.default_rng(seed)
    na, nb = 150, 170
    a, b = _descriptors(rng, na, nb)
    pa = rng.uniform(0, 40, (na, 3))
    pb = rng.uniform(0, 40, (nb, 3))
    pb[:nb // 2] = pa[:nb // 2] + rng.normal(0, 1.5, (nb // 2, 3))        # true partners lie near
    pa4, pb4 = gr.pos4(pa), gr.pos4(pb)
    blind = mr.match(mr.nn2(a, b), mr.nn2(b, a), 0.8)
    counts = []
    for radius in (3.0, 8.0, np.inf):
        fwd, bwd = gr.nn2_gated(a, b, pa4, pb4, radius), gr.nn2_gated(b, a, pb4, pa4, radius)
        guided = gr.match_guided(fwd, bwd, 0.8)
        ok = gr.gate(pa4, pb4, radius)
        np.testing.assert_array_equal(ok, gr.gate(pb4, pa4, radius).T)    # the gate is symmetric, bit for bit
        kept = [i for i in range(na) if blind[i] >= 0 and ok[i, blind[i]]]
        assert len(kept) > 5
        for i in kept:
            assert guided[i] == blind[i]
        assert all(ok[i, guided[i]] for i in range(na) if guided[i] >= 0)
        counts.append((len(kept), int((guided >= 0).sum())))
        # the cap removes exactly the matches beyond it
        d1 = fwd[1]
        cap = float(np.sqrt(np.median(d1[guided >= 0])))
        capped = gr.match_guided(fwd, bwd, 0.8, cap)
        want = np.where(d1 <= F(cap * cap), guided, -1)
        np.testing.assert_array_equal(capped, want)
        assert 0 < (capped >= 0).sum() < (guided >= 0).sum()
    assert counts[0][1] > counts[0][0]                 # the gate recovers matches the blind ratio test threw away
    np.testing.assert_array_equal(gr.match_guided(gr.nn2_gated(a, b, pa4, pb4, np.inf),
                                                  gr.nn2_gated(b, a, pb4, pa4, np.inf), 0.8), blind)
