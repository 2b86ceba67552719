"""CPU (not gpu): the host side of the thin-plate spline -- the fit against a dense float64 solve of the
saddle system, its selection rules against tests/tps_restatement.py, the device layout, and the argument
checks of the fit and of both warp entries, which refuse bad input before any device call."""
import ctypes as C

import numpy as np
import pytest

from tests import tps_restatement as tr


@pytest.fixture(scope="module")
def api():
    from sift3d_amd import api as a
    a.lib()
    return a


def _saddle(c, y, lam):
    """[Phi + lam I, P; P^T, 0] [w; a] = [y; 0] by np.linalg.solve: (w m x 3, a 4 x 3 = [const; x; y; z])"""
    m = len(c)
    D = np.sqrt(((c[:, None, :] - c[None, :, :]) ** 2).sum(-1))
    M = np.zeros((m + 4, m + 4))
    M[:m, :m] = -D + lam * np.eye(m)
    P = np.hstack([np.ones((m, 1)), c])
    M[:m, m:] = P
    M[m:, :m] = P.T
    rhs = np.zeros((m + 4, 3))
    rhs[:m] = y
    s = np.linalg.solve(M, rhs)
    return s[:m], s[m:]


def _pairs(m, seed, spread=100.0, noise=3.0):
    rng = np.random.default_rng(seed)
    c = rng.uniform(0, spread, (m, 3))
    return c, c + rng.normal(0, noise, (m, 3)) + [2.0, -1.0, 0.5]


def _fit_raw(api, src, dst, n, lam=0.0, max_points=64):
    cap = max(max_points, 1)
    ctrl, w, A, m = np.zeros(3 * cap), np.zeros(3 * cap), np.zeros(12), C.c_int(-7)
    src = np.ascontiguousarray(src, np.float64).reshape(-1)
    dst = np.ascontiguousarray(dst, np.float64).reshape(-1)
    rc = api.lib().sift3d_amd_tps_fit(src, dst, n, lam, max_points, ctrl, w, A, C.byref(m))
    return rc, ctrl, w, A, m.value


# ---- the fit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,lam", [(5, 0.0), (6, 0.0), (37, 0.0), (200, 0.0), (200, 2.5), (64, 1e3)])
def test_fit_matches_dense_saddle_solve(api, m, lam):
    c, y = _pairs(m, 100 + m)
    t = api.tps_fit(c, y, lam, 4096)
    w, a = _saddle(c, y, lam)
    np.testing.assert_array_equal(t.ctrl, c)
    assert np.abs(t.weights - w).max() <= 1e-9 * np.abs(w).max()
    A = np.hstack([a[1:].T, a[:1].T])                  # rows d: [x y z const]
    assert np.abs(t.A - A).max() <= 1e-9 * np.abs(A).max()


def test_interpolates_at_lambda_zero_and_side_conditions(api):
    c, y = _pairs(300, 5, spread=400.0, noise=6.0)
    t = api.tps_fit(c, y, 0.0, 4096)
    assert np.abs(api.tps_apply(t, c) - y).max() <= 1e-8
    scale = np.abs(t.weights).max()
    assert np.abs(t.weights.sum(0)).max() <= 1e-9 * scale * len(c)
    assert np.abs(t.weights.T @ c).max() <= 1e-9 * scale * len(c) * 400
    # with smoothing the spline misses each point by -lam * w_i (the first block row of the system)
    t2 = api.tps_fit(c, y, 4.0, 4096)
    assert np.abs(api.tps_apply(t2, c) + 4.0 * t2.weights - y).max() <= 1e-8


def test_affine_data_gives_zero_weights_and_the_affine(api):
    rng = np.random.default_rng(3)
    c = rng.uniform(-50, 250, (120, 3))
    A = np.array([[1.02, 0.05, -0.03, 4.5], [-0.04, 0.98, 0.02, -7.25], [0.01, -0.06, 1.01, 2.0]])
    y = c @ A[:, :3].T + A[:, 3]
    for lam in (0.0, 3.0):
        t = api.tps_fit(c, y, lam, 4096)
        assert np.abs(t.weights).max() <= 1e-10
        assert np.abs(t.A - A).max() <= 1e-10


def test_large_smoothing_gives_least_squares_affine(api):
    c, y = _pairs(150, 8, spread=200.0, noise=4.0)
    t = api.tps_fit(c, y, 1e12, 4096)
    P = np.hstack([c, np.ones((len(c), 1))])
    sol = np.linalg.lstsq(P, y, rcond=None)[0]          # 4 x 3: rows x, y, z, const
    assert np.abs(t.A - sol.T).max() <= 1e-6


def test_duplicates_are_dropped_keeping_the_lowest_index(api):
    c, y = _pairs(40, 11)
    src = np.vstack([c, c[[3, 17, 3]], c[:2]])
    dst = np.vstack([y, y[[3, 17, 3]] + 50.0, y[:2] - 9.0])   # later duplicates carry other targets
    src[40, 0] = src[40, 0] + 0.0                      # exact copies (and a -0.0 below)
    src[5] = [0.0, 10.0, 20.0]
    src = np.vstack([src, [[-0.0, 10.0, 20.0]]])
    dst = np.vstack([dst, [[1.0, 2.0, 3.0]]])
    keep = tr.ref_distinct(src)
    assert list(keep) == list(range(40))
    t = api.tps_fit(src, dst, 0.0, 4096)
    np.testing.assert_array_equal(t.ctrl, src[keep])
    want = api.tps_fit(src[keep], dst[keep], 0.0, 4096)
    np.testing.assert_array_equal(t.weights, want.weights)
    np.testing.assert_array_equal(t.A, want.A)
    assert np.abs(api.tps_apply(t, src[keep]) - dst[keep]).max() <= 1e-8


@pytest.mark.parametrize("n,mmax,seed", [(300, 5, 1), (300, 64, 2), (1000, 257, 3), (50, 49, 4)])
def test_farthest_point_thinning_selects_the_restated_set(api, n, mmax, seed):
    rng = np.random.default_rng(seed)
    src = np.round(rng.uniform(0, 60, (n, 3)))         # integer lattice: many exact distance ties
    src[7] = src[2]                                    # and a duplicate, dropped before thinning
    dst = src + rng.normal(0, 1, (n, 3))
    cand = tr.ref_distinct(src)
    want = tr.ref_thin(src, cand, mmax)
    t = api.tps_fit(src, dst, 1.0, mmax)
    assert len(t.ctrl) == mmax
    np.testing.assert_array_equal(t.ctrl, src[want])
    # no thinning at exactly max_points distinct points
    t2 = api.tps_fit(src[cand[:mmax]], dst[cand[:mmax]], 1.0, mmax)
    np.testing.assert_array_equal(t2.ctrl, src[cand[:mmax]])


def test_fit_refusals_write_nothing(api):
    c, y = _pairs(20, 21)
    L = api.lib()
    good = (np.ascontiguousarray(c.reshape(-1)), np.ascontiguousarray(y.reshape(-1)))
    buf = [np.full(3 * 64, 7.0), np.full(3 * 64, 7.0), np.full(12, 7.0)]
    m = C.c_int(-7)
    assert L.sift3d_amd_tps_fit(good[0], good[1], 20, 0.0, 64, buf[0], buf[1], buf[2], None) == -1
    # NULL arrays: the argtypes are ndpointers, so call through a raw prototype
    raw = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                      C.c_void_p, C.c_void_p)(("sift3d_amd_tps_fit", L))
    ptrs = [good[0].ctypes.data, good[1].ctypes.data, 20, 0.0, 64, buf[0].ctypes.data, buf[1].ctypes.data,
            buf[2].ctypes.data, C.addressof(m)]
    for k in (0, 1, 5, 6, 7, 8):
        args = list(ptrs)
        args[k] = None
        assert raw(*args) == -1, k

    def refused(src, dst, n, lam=0.0, max_points=64):
        rc, ctrl, w, A, mm = _fit_raw(api, src, dst, n, lam, max_points)
        assert rc == -1 and mm == -7 and not ctrl.any() and not w.any() and not A.any()

    refused(c, y, 4)                                   # n < 5
    for lam in (-1e-9, np.nan, np.inf):
        refused(c, y, 20, lam)
    for mp in (4, 0, -3, 16385):
        refused(c, y, 20, 0.0, mp)
    for v in (np.nan, np.inf, -np.inf):
        for which in (0, 1):
            s, d = c.copy(), y.copy()
            (s if which == 0 else d)[13, 2] = v
            refused(s, d, 20)
    four = np.vstack([c[:4], c[:4], c[1:3]])           # 10 points, 4 distinct
    refused(four, y[:10], 10)
    plane = c.copy()
    plane[:, 2] = 0.5 * plane[:, 0] - 0.25 * plane[:, 1] + 3.0   # coplanar
    refused(plane, y, 20)
    line = np.outer(np.arange(20.0), [1.0, 2.0, 3.0])
    refused(line, y, 20)
    with pytest.raises(ValueError):
        api.tps_fit(plane, y)
    with pytest.raises(ValueError):
        api.tps_fit(c, y[:19])
    assert api.tps_fit(c, y, 0.0, 64).ctrl.shape == (20, 3)


def test_apply_and_pack(api):
    c, y = _pairs(30, 31)
    t = api.tps_fit(c, y, 0.5, 64)
    p = np.random.default_rng(1).uniform(-20, 120, (50, 3))
    q = api.tps_apply(t, p)
    D = np.sqrt(((p[:, None, :] - t.ctrl[None, :, :]) ** 2).sum(-1))
    want = p @ t.A[:, :3].T + t.A[:, 3] + (-D) @ t.weights
    assert np.abs(q - want).max() <= 1e-9
    packed = api.tps_pack(t.ctrl, t.weights)
    assert packed.dtype == np.float32 and packed.shape == (30, 8)
    np.testing.assert_array_equal(packed[:, :3], t.ctrl.astype(np.float32))
    np.testing.assert_array_equal(packed[:, 4:7], -(t.weights.astype(np.float32)))
    assert not packed[:, 3].any() and not packed[:, 7].any()
    assert np.signbit(api.tps_pack(t.ctrl, np.zeros((30, 3)))[:, 4:7]).all()   # -0.0: the sign folded in
    L = api.lib()
    out = np.zeros(8 * 30, np.float32)
    cf, wf = np.ascontiguousarray(t.ctrl.reshape(-1)), np.ascontiguousarray(t.weights.reshape(-1))
    assert L.sift3d_amd_tps_pack(cf, wf, 0, out) == -1
    assert L.sift3d_amd_tps_pack(cf, wf, 16385, out) == -1
    for bad in (np.nan, np.inf, 1e39):                 # 1e39 is not finite in float
        w2 = wf.copy()
        w2[4] = bad
        assert L.sift3d_amd_tps_pack(cf, w2, 30, out) == -1
    assert not out.any()
    assert L.sift3d_amd_tps_apply(cf, wf, np.ascontiguousarray(t.A.reshape(-1)), 0, p.reshape(-1), 50,
                                  np.zeros(150)) == -1


# ---- refusals of the warp entries, before any device call --------------------------------------------
def _hip_tps(src, nx, ny, nz, dst, ox, oy, oz, A, tps, m, interp, fill=0.0):
    from sift3d_amd import hip
    a = None if A is None else np.ascontiguousarray(A, np.float64).reshape(12)
    ap = None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    return hip.lib().sift3d_hip_warp_tps(src, nx, ny, nz, dst, ox, oy, oz, ap, tps, m, interp, fill, None)


def test_device_warp_tps_refuses_bad_arguments_without_device(api):
    from sift3d_amd import hip
    ident = tr.IDENT
    # As for the affine warp: made-up addresses without a device, real allocations covering every range
    # named below with one, so that a regressed check could not make the kernel read unmapped memory.
    bufs = []
    if api.device_available():
        bufs = [hip.lib().sift3d_hip_malloc(8192), hip.lib().sift3d_hip_malloc(8192),
                hip.lib().sift3d_hip_malloc(8192)]
        assert all(bufs)
        S, D, T = bufs
    else:
        S, D, T = 0x100000, 0x900000, 0x1100000
    cases = [
        (None, 8, 8, 8, D, 8, 8, 8, ident, T, 4, 1),
        (S, 8, 8, 8, None, 8, 8, 8, ident, T, 4, 1),
        (S, 8, 8, 8, D, 8, 8, 8, None, T, 4, 1),
        (S, 8, 8, 8, D, 8, 8, 8, ident, None, 4, 1),
        (S, 0, 8, 8, D, 8, 8, 8, ident, T, 4, 1),
        (S, 8, -1, 8, D, 8, 8, 8, ident, T, 4, 1),
        (S, 8, 8, 8, D, 8, 8, 0, ident, T, 4, 0),
        (S, 8, 8, 8, D, 8, 8, 8, ident, T, 0, 1),       # m < 1
        (S, 8, 8, 8, D, 8, 8, 8, ident, T, -1, 1),
        (S, 8, 8, 8, D, 8, 8, 8, ident, T, 16385, 1),   # m above the cap
        (S, 8, 8, 8, D, 8, 8, 8, ident, T, 4, 2),
        (S, 8, 8, 8, D, 8, 8, 8, ident, T, 4, -1),
        (S, 8, 8, 8, D, 8, 8, 8, ident, T + 4, 4, 1),   # misaligned records
        (S, 8, 8, 8, S, 8, 8, 8, ident, T, 4, 1),       # in place
        (S, 8, 8, 8, S + 4 * 511, 8, 8, 8, ident, T, 4, 1),
        (S + 4 * 100, 8, 8, 8, S, 8, 8, 8, ident, T, 4, 0),
        (S, 8, 8, 8, D, 8, 8, 8, ident, D + 4 * 16, 4, 1),   # records inside dst
        (S, 8, 8, 8, T + 64, 8, 8, 2, ident, T, 4, 1),       # dst starts inside the records
    ]
    for v in (np.nan, np.inf, -np.inf):
        A = ident.copy()
        A[2, 1] = v
        cases.append((S, 8, 8, 8, D, 8, 8, 8, A, T, 4, 1))
    try:
        for c in cases:
            assert _hip_tps(*c) == -1, c
    finally:
        for b in bufs:
            hip.lib().sift3d_hip_free(b)


def test_launch_split_query():
    from sift3d_amd import hip
    assert hip.warp_tps_launches((8, 8, 8), 0) == -1
    assert hip.warp_tps_launches((8, 8, 8), 16385) == -1
    assert hip.warp_tps_launches((0, 8, 8), 4) == -1
    assert hip.warp_tps_launches((29, 31, 7), 1000) == 1
    n = [hip.warp_tps_launches((512, 512, 512), m) for m in (256, 1024, 4096, 16384)]
    assert n == sorted(n) and n[0] >= 1 and n[-1] > n[0]


def test_image_warp_tps_refuses_bad_arguments_without_device(api):
    L = api.lib()
    ident = np.ascontiguousarray(tr.IDENT.reshape(12))
    src, dst = api.Image(9, 7, 5), api.Image(6, 6, 6)
    two = api.Image(9, 7, 5, 2)
    tps = np.zeros(8 * 4, np.float32)
    tps[0::8] = [1, 2, 3, 4]
    assert L.sift3d_amd_image_warp_tps(None, ident, tps, 4, 1, 0.0, dst.h) == -1
    assert L.sift3d_amd_image_warp_tps(src.h, ident, tps, 4, 1, 0.0, None) == -1
    assert L.sift3d_amd_image_warp_tps(two.h, ident, tps, 4, 1, 0.0, dst.h) == -1
    assert L.sift3d_amd_image_warp_tps(src.h, ident, tps, 4, 1, 0.0, two.h) == -1
    assert L.sift3d_amd_image_warp_tps(src.h, ident, tps, 4, 3, 0.0, dst.h) == -1
    assert L.sift3d_amd_image_warp_tps(src.h, ident, tps, 0, 1, 0.0, dst.h) == -1
    assert L.sift3d_amd_image_warp_tps(src.h, ident, tps, 16385, 1, 0.0, dst.h) == -1
    bad = ident.copy()
    bad[5] = np.nan
    assert L.sift3d_amd_image_warp_tps(src.h, bad, tps, 4, 1, 0.0, dst.h) == -1
    for v in (np.nan, np.inf):
        t2 = tps.copy()
        t2[13] = v
        assert L.sift3d_amd_image_warp_tps(src.h, ident, t2, 4, 1, 0.0, dst.h) == -1
    t = api.TPS(np.arange(12.0).reshape(4, 3) ** 1.5, np.zeros((4, 3)), tr.IDENT)
    with pytest.raises(RuntimeError):
        api.warp_tps(two, t, (6, 6, 6))
    with pytest.raises(ValueError):
        api.warp_tps(src, t, (6, 6, 6), interp="cubic")
