"""CPU (not gpu): the host side of affine resampling -- inversion of affine maps and the argument
checks of sift3d_hip_warp_affine / sift3d_amd_image_warp_affine, which refuse bad input before any
device call (so they hold on a machine without a GPU, and under the sanitizer build)."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def api():
    from sift3d_amd import api as a
    a.lib()
    return a


def _apply(A, p):
    return p @ A[:, :3].T + A[:, 3]


def test_affine_invert_round_trips_random_maps(api):
    rng = np.random.default_rng(17)
    p = rng.uniform(-300, 300, (50, 3))
    for _ in range(200):
        q, _r = np.linalg.qr(rng.standard_normal((3, 3)))
        A = np.zeros((3, 4))
        A[:, :3] = q @ np.diag(rng.uniform(0.5, 2.0, 3)) @ (np.eye(3) + 0.2 * rng.standard_normal((3, 3)) * 0.5)
        A[:, 3] = rng.uniform(-100, 100, 3)
        if np.linalg.cond(A[:, :3]) > 20:
            continue
        Ai = api.affine_invert(A)
        M = np.vstack([A, [0, 0, 0, 1]])
        Mi = np.vstack([Ai, [0, 0, 0, 1]])
        assert np.abs(Mi @ M - np.eye(4)).max() < 1e-12
        assert np.abs(M @ Mi - np.eye(4)).max() < 1e-12
        assert np.abs(_apply(Ai, _apply(A, p)) - p).max() < 1e-12 * 300
        np.testing.assert_allclose(api.affine_invert(Ai), A, rtol=0, atol=1e-12 * (1 + np.abs(A).max()))


def test_affine_invert_integer_permutations_exact(api):
    for perm in ([0, 1, 2], [1, 0, 2], [2, 0, 1], [1, 2, 0], [2, 1, 0], [0, 2, 1]):
        for signs in ([1, 1, 1], [-1, 1, 1], [1, -1, -1], [-1, -1, -1]):
            A = np.zeros((3, 4))
            for r in range(3):
                A[r, perm[r]] = signs[r]
            A[:, 3] = [17.0, -4.0, 63.0]
            Ai = api.affine_invert(A)
            want = np.zeros((3, 4))
            want[:, :3] = A[:, :3].T
            want[:, 3] = -(A[:, :3].T @ A[:, 3])
            np.testing.assert_array_equal(Ai, want)


def test_affine_invert_refuses_singular_and_non_finite(api):
    rank2 = np.array([[1.0, 2.0, 3.0, 0.0], [4.0, 5.0, 6.0, 1.0], [5.0, 7.0, 9.0, 2.0]])
    scaled = rank2 * 1e-3
    for bad in (rank2, scaled, np.zeros((3, 4))):
        with pytest.raises(ValueError):
            api.affine_invert(bad)
    for v in (np.nan, np.inf):
        A = np.hstack([np.eye(3), np.zeros((3, 1))])
        A[1, 3] = v
        with pytest.raises(ValueError):
            api.affine_invert(A)
    # the C entry point itself
    out = np.zeros(12)
    assert api.lib().sift3d_amd_affine_invert(np.ascontiguousarray(rank2.reshape(12)), out) == -1


def _hip_warp(src, nx, ny, nz, dst, ox, oy, oz, A, interp, fill=0.0):
    from sift3d_amd import hip
    a = None if A is None else np.ascontiguousarray(A, np.float64).reshape(12)
    ap = None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    return hip.lib().sift3d_hip_warp_affine(src, nx, ny, nz, dst, ox, oy, oz, ap, interp, fill, None)


def test_device_warp_refuses_bad_arguments_without_device(api):
    from sift3d_amd import hip
    ident = np.hstack([np.eye(3), np.zeros((3, 1))])
    # Every case below is refused before any device call, so the buffers are never touched.  Without a
    # device they are made-up addresses; with one they are real allocations that cover every range named
    # below, so that a regressed check could not make the kernel read unmapped memory.
    bufs = []
    if api.device_available():
        bufs = [hip.lib().sift3d_hip_malloc(8192), hip.lib().sift3d_hip_malloc(8192)]
        assert all(bufs)
        S, D = bufs
    else:
        S, D = 0x100000, 0x900000
    cases = [
        (None, 8, 8, 8, D, 8, 8, 8, ident, 1),
        (S, 8, 8, 8, None, 8, 8, 8, ident, 1),
        (S, 8, 8, 8, D, 8, 8, 8, None, 1),
        (S, 0, 8, 8, D, 8, 8, 8, ident, 1),
        (S, 8, -1, 8, D, 8, 8, 8, ident, 1),
        (S, 8, 8, 8, D, 8, 8, 0, ident, 0),
        (S, 8, 8, 8, D, 8, 8, 8, ident, 2),
        (S, 8, 8, 8, D, 8, 8, 8, ident, -1),
        (S, 8, 8, 8, S, 8, 8, 8, ident, 1),                 # in place
        (S, 8, 8, 8, S + 4 * 511, 8, 8, 8, ident, 1),       # dst starts inside src
        (S + 4 * 100, 8, 8, 8, S, 8, 8, 8, ident, 0),       # src starts inside dst
    ]
    for v in (np.nan, np.inf, -np.inf):
        A = ident.copy()
        A[2, 1] = v
        cases.append((S, 8, 8, 8, D, 8, 8, 8, A, 1))
    try:
        for c in cases:
            assert _hip_warp(*c) == -1, c
    finally:
        for b in bufs:
            hip.lib().sift3d_hip_free(b)


def test_image_warp_refuses_bad_arguments_without_device(api):
    L = api.lib()
    ident = np.ascontiguousarray(np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(12))
    src, dst = api.Image(9, 7, 5), api.Image(6, 6, 6)
    two = api.Image(9, 7, 5, 2)
    assert L.sift3d_amd_image_warp_affine(None, ident, 1, 0.0, dst.h) == -1
    assert L.sift3d_amd_image_warp_affine(src.h, ident, 1, 0.0, None) == -1
    assert L.sift3d_amd_image_warp_affine(two.h, ident, 1, 0.0, dst.h) == -1
    assert L.sift3d_amd_image_warp_affine(src.h, ident, 1, 0.0, two.h) == -1
    assert L.sift3d_amd_image_warp_affine(src.h, ident, 3, 0.0, dst.h) == -1
    bad = ident.copy()
    bad[5] = np.nan
    assert L.sift3d_amd_image_warp_affine(src.h, bad, 1, 0.0, dst.h) == -1
    with pytest.raises(RuntimeError):
        api.warp_affine(two, ident.reshape(3, 4), (6, 6, 6))
    with pytest.raises(ValueError):
        api.warp_affine(src, ident.reshape(3, 4), (6, 6, 6), interp="cubic")
