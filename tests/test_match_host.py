"""CPU (not gpu): the host side of matching and RANSAC -- sift3d_hip_nn2's argument checks and scratch size,
the nn_thresh refusals of the matcher (all before any device call), RANSAC bit for bit against its
restatement (tests/match_restatement.py), and the restatement's own arithmetic."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from tests import match_restatement as mr


@pytest.fixture(scope="module")
def api():
    from sift3d_amd import api as a
    a.lib()
    return a


@pytest.fixture(scope="module")
def L(api):
    from sift3d_amd import hip
    return hip.lib()


# ---- sift3d_hip_nn2: refusals and scratch size ----------------------------------------------------------
BASE = 0x10000000                     # made-up, 256-byte aligned addresses: never dereferenced


def _nn2(L, A=BASE, nA=5, B=BASE + 0x100000, nB=7, dim=64, j=BASE + 0x200000, d1=BASE + 0x300000,
         d2=BASE + 0x400000, work=BASE + 0x500000):
    return L.sift3d_hip_nn2(A, nA, B, nB, dim, j, d1, d2, work, None)


@pytest.mark.parametrize("bad", [
    {"A": None}, {"B": None}, {"j": None}, {"d1": None}, {"d2": None}, {"work": None},
    {"nA": -1}, {"nB": -1}, {"nA": -5, "nB": -5},
    {"dim": 0}, {"dim": 16}, {"dim": 48}, {"dim": -32},
    {"A": BASE + 4}, {"B": BASE + 0x100000 + 4}, {"A": BASE + 8, "B": BASE + 0x100000 + 12},
])
def test_nn2_refuses_before_any_device_call(L, bad):
    assert _nn2(L, nA=0, nB=0) == 0                  # (clears nothing, but proves the call itself is fine)
    assert _nn2(L, **bad) != 0
    assert L.sift3d_hip_last_error().decode() == "sift3d_hip_nn2: invalid arguments"


def test_nn2_empty_a_is_success_without_device(L):
    # nA = 0: nothing to compute, nothing written (the outputs are fake addresses)
    assert _nn2(L, nA=0) == 0
    assert _nn2(L, nA=0, nB=0, dim=1024) == 0


@pytest.mark.parametrize("na,nb,ns,empty", [
    (1, 1, 1, 0), (5, 1, 1, 0), (33, 129, 2, 0),
    (128, 2049, 16, 7), (129, 2176, 16, 7), (16385, 4000, 16, 0),
    (42501, 40000, 7, 0), (40000, 42501, 7, 0), (262145, 200, 1, 0), (262016, 200, 2, 0),
    (3, 0, 1, 1), (0, 9, 1, 0),
])
def test_nn2_runs_and_work_floats(L, na, nb, ns, empty):
    """The run count of nn2_splits (restated by mr.runs) and the advertised scratch size: the norms of
    both sets, 8 floats of padding, and three ns x nA slices of per-run top-2."""
    got_ns, got_empty = mr.runs(na, nb)
    assert (got_ns, got_empty) == (ns, empty)
    assert L.sift3d_hip_nn2_work_floats(na, nb) == na + nb + 8 + 3 * na * ns
    assert L.sift3d_hip_nn2_work_floats(-4, -4) == 8 + 0


# ---- matcher refusals -----------------------------------------------------------------------------------
def test_matcher_refuses_nonpositive_threshold_without_device(api):
    L = api.lib()
    L.sift3d_amd_matcher_match.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                           np.ctypeslib.ndpointer(np.int32)]
    L.sift3d_amd_matcher_match.restype = C.c_int
    a, b = api.DescriptorStore(), api.DescriptorStore()
    rng = np.random.default_rng(1)
    assert a.set(np.zeros((3, 4)), rng.random((3, 768), np.float32)) == 0
    assert b.set(np.zeros((4, 4)), rng.random((4, 768), np.float32)) == 0
    for thr in (0.0, -0.0, -0.8):
        out = np.full(3, 77, np.int32)
        assert L.sift3d_amd_nn_match(a.h, b.h, thr, out) != 0
        # a made-up matcher: the threshold is refused before the matcher is touched
        assert L.sift3d_amd_matcher_match(0x1000, a.h, b.h, thr, out) != 0
        assert (out == 77).all()
    out = np.full(3, 77, np.int32)
    assert L.sift3d_amd_matcher_match(None, a.h, b.h, 0.8, out) != 0
    assert (out == 77).all()


# ---- RANSAC bit for bit ---------------------------------------------------------------------------------
def _c_ransac(api, src, dst, thr, iters, seed):
    src = np.ascontiguousarray(src, np.float64).reshape(-1, 3)
    dst = np.ascontiguousarray(dst, np.float64).reshape(-1, 3)
    T = np.zeros(12)
    inl = np.full(max(len(src), 1), 9, np.uint8)
    cnt = C.c_int(-7)
    rc = api.lib().sift3d_amd_ransac_affine(src.reshape(-1), dst.reshape(-1), len(src), float(thr), int(iters),
                                            int(seed), T, inl, C.byref(cnt))
    return rc, T.reshape(3, 4), inl[:len(src)], cnt.value


def _check_ransac(api, src, dst, thr, iters, seed, expect_ok=True):
    """expect_ok: True / False when the fit must succeed / fail, None when either is right."""
    rc, T, inl, cnt = _c_ransac(api, src, dst, thr, iters, seed)
    want = mr.ransac_affine(src, dst, thr, iters, seed)
    if want is None:
        assert rc != 0 and expect_ok is not True
        with pytest.raises(RuntimeError):
            api.ransac_affine(src, dst, thr, iters, seed)
        return None
    assert rc == 0 and expect_ok is not False
    np.testing.assert_array_equal(T.view(np.int64), want[0].view(np.int64))     # bitwise, -0.0 included
    np.testing.assert_array_equal(inl, want[1])
    assert cnt == want[2] == int(inl.sum())
    T2, inl2 = api.ransac_affine(src, dst, thr, iters, seed)
    np.testing.assert_array_equal(T2, T)
    np.testing.assert_array_equal(inl2, inl.astype(bool))
    return want


AFF = np.array([[0.9, -0.3, 0.1, 12.0], [0.25, 1.1, -0.05, -7.5], [-0.1, 0.2, 0.95, 3.0]])


def _outlier_case(n, frac, seed):
    rng = np.random.default_rng(seed)
    src = rng.uniform(0, 500, (n, 3))
    dst = src @ AFF[:, :3].T + AFF[:, 3] + rng.normal(0, 0.3, (n, 3))
    bad = rng.choice(n, int(frac * n), replace=False)
    dst[bad] = rng.uniform(0, 500, (len(bad), 3))
    return src, dst


@pytest.mark.parametrize("seed", [0, 1, 7, 2 ** 63 + 12345, 2 ** 64 - 1])
def test_ransac_bitexact_40pct_outliers(api, seed):
    src, dst = _outlier_case(400, 0.4, 3)
    want = _check_ransac(api, src, dst, 2.0, 500, seed)
    assert 230 <= want[2] <= 245


def test_ransac_bitexact_few_iterations_and_weak_consensus(api):
    # a consensus won by an early, mediocre sample: the first model with the largest count must win
    src, dst = _outlier_case(60, 0.7, 4)
    for seed in (0, 3, 11):
        for iters in (1, 2, 5, 37):
            _check_ransac(api, src, dst, 4.0, iters, seed, expect_ok=None)


def test_ransac_bitexact_four_points(api):
    rng = np.random.default_rng(5)
    src = rng.uniform(-50, 50, (4, 3))
    dst = src @ AFF[:, :3].T + AFF[:, 3]
    for seed in (0, 2):
        want = _check_ransac(api, src, dst, 1e-3, 3, seed)
        assert want[2] == 4


def test_ransac_bitexact_partly_coplanar_samples(api):
    # 24 of 30 points on the plane z = 5: most samples are degenerate (refused by the 1e-12 pivot)
    rng = np.random.default_rng(6)
    src = rng.uniform(0, 100, (30, 3))
    src[:24, 2] = 5.0
    dst = src @ AFF[:, :3].T + AFF[:, 3] + rng.normal(0, 0.05, (30, 3))
    for seed in (0, 1, 9):
        for iters in (3, 50):
            _check_ransac(api, src, dst, 0.5, iters, seed, expect_ok=None)
    # every sample degenerate: coplanar and collinear sets fail, in the C code and in the restatement
    flat = src.copy()
    flat[:, 2] = 5.0
    _check_ransac(api, flat, flat + 1.0, 1.0, 40, 0, expect_ok=False)
    line = np.outer(np.arange(12.0), [1.0, 2.0, -1.0])
    _check_ransac(api, line, line, 1.0, 40, 3, expect_ok=False)


def test_ransac_bitexact_points_at_threshold(api):
    # integer points under an integer translation; a third of them moved by (3, 4, 0) or (0, 0, 5): residual
    # exactly 5 = err_thresh under the exact model (e2 <= thr2 admits them), just above or below it under a
    # fitted model that is off by an ulp
    rng = np.random.default_rng(8)
    src = rng.integers(-40, 40, (45, 3)).astype(np.float64)
    dst = src + np.array([10.0, -4.0, 2.0])
    dst[::3] += np.array([3.0, 4.0, 0.0])
    dst[1::6] += np.array([0.0, 0.0, 5.0])
    for seed in (0, 5):
        for thr in (5.0, np.nextafter(5.0, 0.0), 4.0):
            _check_ransac(api, src, dst, thr, 60, seed, expect_ok=None)


def test_ransac_argument_refusals(api):
    src, dst = _outlier_case(10, 0.0, 1)
    for args in ((src[:3], dst[:3], 1.0, 10, 0), (src, dst, 0.0, 10, 0), (src, dst, -1.0, 10, 0),
                 (src, dst, 1.0, 0, 0)):
        assert _c_ransac(api, *args)[0] != 0
        assert mr.ransac_affine(*args) is None


def test_xorshift_sequence():
    s = mr.xorshift64(88172645463325252)
    # Marsaglia (2003), xorshift64 with (13, 7, 17): the first outputs from his default seed
    assert s == 8748534153485358512
    assert mr.xorshift64(s) == 3040900993826735515


# ---- the restatement's own arithmetic -------------------------------------------------------------------
def _round32(fr):
    f = np.float32(float(fr))
    cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    return min(cands, key=lambda c: (abs(Fraction(float(c)) - fr), int(np.float32(c).view(np.int32)) & 1))


def test_fma32_is_correctly_rounded():
    rng = np.random.default_rng(2)
    n = 3000
    a, b, c = ((rng.standard_normal(n) * np.exp(rng.uniform(-10, 10, n))).astype(np.float32) for _ in range(3))
    # cases where the float64 sum is inexact and a plain cast would round twice
    a[:4] = np.float32(1 + 2 ** -23)
    b[:4] = np.float32(1 + 2 ** -23)
    c[:4] = np.float32([-1.0, 2 ** -30, -(2 ** -47), 3 * 2 ** -24])
    got = mr.fma32(a, b, c)
    want = np.array([_round32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))
                     for x, y, z in zip(a, b, c)], np.float32)
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))


def test_chain_order_and_top2_ties():
    assert mr.k_order(32)[:8] == [0, 4, 1, 5, 2, 6, 3, 7] and sorted(mr.k_order(96)) == list(range(96))
    # integer data: every order is exact, so the restated nn2 equals float64 distances
    rng = np.random.default_rng(3)
    a = rng.integers(0, 4, (9, 64)).astype(np.float32)
    b = rng.integers(0, 4, (40, 64)).astype(np.float32)
    b[30] = b[7] = a[2]
    j, d1, d2 = mr.nn2(a, b)
    D = ((a.astype(np.float64)[:, None] - b[None]) ** 2).sum(-1)
    np.testing.assert_array_equal(d1, D.min(1))
    np.testing.assert_array_equal(d2, np.sort(D, 1)[:, 1])
    np.testing.assert_array_equal(j, np.argmin(D, 1))
    assert j[2] == 7 and d1[2] == d2[2] == 0
    j, d1, d2 = mr.nn2(a, b[:1])
    assert (j == 0).all() and np.isinf(d2).all()
    j, d1, d2 = mr.nn2(a, b[:0])
    assert (j == -1).all() and np.isinf(d1).all() and np.isinf(d2).all()


def test_row_norms_lane_order():
    # lane partials then the butterfly differ from a sequential sum on these values
    b = np.zeros((1, 128), np.float32)
    b[0, 0], b[0, 64], b[0, 1], b[0, 65] = 2.0 ** 12, 1.0, 1.0, 2.0 ** -1
    # lane 0: 2^24 + 1 -> 2^24 (even); lane 1: 1 + 0.25 = 1.25; sum 2^24 + 1.25 -> 2^24 + 2, where k order
    # (0, 1, 64, 65) would give 2^24
    assert mr.row_norms(b)[0] == np.float32(2.0 ** 24 + 2)
