"""CPU (not gpu): the host side of rotation-invariant dense descriptors -- the argument checks of
sift3d_amd_dense_descriptors_rotate_device, sift3d_amd_image_dense_descriptors_rotate and the two
stages, which refuse bad input before any device call -- and the numpy restatement's orientation (R2)
pinned to the oracle's assign_eig_ori (orc_orient_slab) at every voxel, bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import dense_rotate_restatement as drr


@pytest.fixture(scope="module")
def api():
    from sift3d_amd import api as a
    a.lib()
    return a


def _dev(src, nx, ny, nz, units, sigma, out, work):
    from sift3d_amd import hip
    u = None if units is None else (C.c_double * 3)(*units)
    return hip.lib().sift3d_amd_dense_descriptors_rotate_device(src, nx, ny, nz, u, sigma, out, work, None)


def test_work_floats(api):
    from sift3d_amd import hip
    L = hip.lib()
    assert L.sift3d_amd_dense_rotate_work_floats(5, 6, 7) == 9 * 5 * 6 * 7
    assert L.sift3d_amd_dense_rotate_work_floats(576, 576, 544) == 9 * 576 * 576 * 544
    assert L.sift3d_amd_dense_rotate_work_floats(0, 6, 7) == 0
    assert L.sift3d_amd_dense_rotate_work_floats(5, -1, 7) == 0


def test_device_entry_refuses_bad_arguments_without_device(api):
    from sift3d_amd import hip
    n = 8 * 8 * 8
    bufs = []
    if api.device_available():
        bufs = [hip.lib().sift3d_hip_malloc(4 * n * 40)]
        assert all(bufs)
        base = bufs[0]
    else:
        base = 0x1000000
    S, O, W = base, base + 4 * n * 2, base + 4 * n * 16
    u1 = (1.0, 1.0, 1.0)
    cases = [
        (None, 8, 8, 8, u1, 1.6, O, W),
        (S, 8, 8, 8, u1, 1.6, None, W),
        (S, 8, 8, 8, u1, 1.6, O, None),
        (S, 8, 8, 8, None, 1.6, O, W),
        (S, 0, 8, 8, u1, 1.6, O, W),
        (S, 8, -2, 8, u1, 1.6, O, W),
        (S, 8, 8, 0, u1, 1.6, O, W),
        (S, 8, 8, 8, u1, 0.0, O, W),
        (S, 8, 8, 8, u1, -1.0, O, W),
        (S, 8, 8, 8, u1, math.nan, O, W),
        (S, 8, 8, 8, u1, math.inf, O, W),
        (S, 8, 8, 8, (0.0, 1.0, 1.0), 1.6, O, W),
        (S, 8, 8, 8, (1.0, -1.0, 1.0), 1.6, O, W),
        (S, 8, 8, 8, (1.0, 1.0, math.nan), 1.6, O, W),
        (S, 8, 8, 8, (math.inf, 1.0, 1.0), 1.6, O, W),
        (S, 8, 8, 8, u1, 1.6, S, W),                      # output over the source
        (S, 8, 8, 8, u1, 1.6, S + 4 * (n - 1), W),        # output starts in the source's last voxel
        (O + 4 * 12 * n - 4, 8, 8, 8, u1, 1.6, O, W),     # source starts in the output's last voxel
        (S, 8, 8, 8, u1, 1.6, O, O + 4 * 100),            # work inside the output
        (S, 8, 8, 8, u1, 1.6, W + 4 * (9 * n - 1), W),    # output starts in the work buffer's end
        (S, 8, 8, 8, u1, 1.6, O, S + 4 * (n - 1)),        # work starts in the source's last voxel
    ]
    try:
        for c in cases:
            assert _dev(*c) == -1, c
    finally:
        for b in bufs:
            hip.lib().sift3d_hip_free(b)


def test_stage_entries_refuse_bad_arguments_without_device(api):
    from sift3d_amd import hip
    L = hip.lib()
    S, R, O, K = 0x1000000, 0x2000000, 0x4000000, 0x8000000
    n = 8 * 8 * 8
    ori = L.sift3d_hip_dense_orient
    rb = L.sift3d_hip_dense_rotate_bin
    assert ori(None, 8, 8, 8, 1.0, 1.0, 1.0, 1.6, R, K, None) == -1
    assert ori(S, 8, 8, 8, 1.0, 1.0, 1.0, 1.6, None, K, None) == -1
    assert "NULL" in L.sift3d_hip_last_error().decode()
    assert ori(S, 8, 0, 8, 1.0, 1.0, 1.0, 1.6, R, K, None) == -1
    assert ori(S, 8, 8, 8, 1.0, 0.0, 1.0, 1.6, R, K, None) == -1
    assert ori(S, 8, 8, 8, 1.0, 1.0, math.nan, 1.6, R, K, None) == -1
    assert ori(S, 8, 8, 8, 1.0, 1.0, 1.0, 0.0, R, K, None) == -1
    assert ori(S, 8, 8, 8, 1.0, 1.0, 1.0, math.inf, R, K, None) == -1
    assert ori(S, 8, 8, 8, 1.0, 1.0, 1.0, 1.6, S + 4, K, None) == -1              # R over the source
    assert ori(S, 8, 8, 8, 1.0, 1.0, 1.0, 1.6, R, R + 4 * 9 * n - 1, None) == -1  # keep in R's last byte
    assert ori(S, 8, 8, 8, 1.0, 1.0, 1.0, 1.6, R, S, None) == -1                  # keep over the source
    assert ori(S, 8, 8, 8, 0.01, 1.0, 1.0, 1.8, R, K, None) == -1                 # 540 voxels wide
    assert "wider" in L.sift3d_hip_last_error().decode()
    assert ori(S, 8, 8, 8, 1.0, 1.0, 1.0, 5.7, R, K, None) == -1                  # 20946 window voxels
    assert "more than 20000" in L.sift3d_hip_last_error().decode()
    assert rb(S, 8, 8, 8, 0.5, 1.0, 1.0, 4.5, R, O, None) == -1                   # 20613 window voxels
    assert "more than 20000" in L.sift3d_hip_last_error().decode()
    assert rb(None, 8, 8, 8, 1.0, 1.0, 1.0, 1.6, R, O, None) == -1
    assert rb(S, 8, 8, 8, 1.0, 1.0, 1.0, 1.6, None, O, None) == -1
    assert rb(S, 8, 8, 8, 1.0, 1.0, 1.0, 1.6, R, None, None) == -1
    assert rb(S, -8, 8, 8, 1.0, 1.0, 1.0, 1.6, R, O, None) == -1
    assert rb(S, 8, 8, 8, 1.0, 1.0, 1.0, -1.6, R, O, None) == -1
    assert rb(S, 8, 8, 8, 1.0, 1.0, 1.0, 1.6, R, S, None) == -1                   # out over the source
    assert rb(S, 8, 8, 8, 1.0, 1.0, 1.0, 1.6, R, R + 4 * 9 * n - 4, None) == -1   # out in R's end


def test_image_entry_refuses_bad_arguments_without_device(api):
    L = api.lib()
    im = api.Image(8, 7, 6)
    out = np.zeros(12 * 8 * 7 * 6, np.float32)
    two = api.Image(8, 7, 6, 2)
    f = L.sift3d_amd_image_dense_descriptors_rotate
    assert f(None, 1.6, out) == -1
    raw = L["sift3d_amd_image_dense_descriptors_rotate"]
    raw.restype, raw.argtypes = C.c_int, [C.c_void_p, C.c_double, C.c_void_p]
    assert raw(im.h, 1.6, None) == -1
    assert f(two.h, 1.6, np.zeros(2 * out.size, np.float32)) == -1
    for s in (0.0, -0.5, math.nan, math.inf):
        assert f(im.h, s, out) == -1, s


def test_api_without_device_raises(api):
    if api.device_available():
        pytest.skip("the device is present: tests/test_dense_rotate.py covers the entries")
    with pytest.raises(RuntimeError):
        api.dense_descriptors(np.zeros((6, 7, 8), np.float32), rotate=True)
    with pytest.raises(RuntimeError):
        api.dense_orientations(np.zeros((6, 7, 8), np.float32))


# ---- R2 pinned to the oracle --------------------------------------------------------------------
def _vol(oracle_mod, shape, seed, flat=False):
    vol = oracle_mod.synth_survey(shape, nblob=max(4, int(np.prod(shape)) // 400), seed=seed)
    vol += np.random.default_rng(seed).random(vol.shape, dtype=np.float32) * np.float32(0.05)
    if flat:
        vol[:, :, : vol.shape[2] // 2] = np.float32(0.25)     # a flat half: rejected
    return vol


ORIENT_CASES = [
    # (shape (nx, ny, nz), units, sigma, flat half)
    ((40, 36, 33), (1.0, 1.0, 1.0), 1.5, False),
    ((40, 36, 33), (1.0, 1.0, 1.0), 3.0, False),
    ((26, 22, 20), (0.8, 0.8, 2.0), 1.5, False),
    ((26, 22, 20), (0.8, 0.8, 2.0), 3.0, False),
    ((24, 20, 18), (1.0, 1.0, 1.0), 1.5, True),
    ((1, 9, 7), (1.0, 1.0, 1.0), 1.5, False),
    ((3, 2, 9), (1.0, 1.0, 1.0), 1.5, False),
    ((9, 3, 3), (1.0, 1.0, 1.0), 3.0, False),
]


@pytest.fixture(scope="module")
def oracle_orient_cache(oracle_mod):
    return {}


def _case(oracle_mod, cache, shape, units, sigma, flat):
    key = (shape, units, sigma, flat)
    if key not in cache:
        vol = _vol(oracle_mod, shape, 7, flat)
        cache[key] = (vol, drr.orient(vol, sigma, units), drr.oracle_orient(vol, sigma, units))
    return cache[key]


@pytest.mark.parametrize("shape,units,sigma,flat", ORIENT_CASES)
def test_restated_orientation_is_the_oracles(api, oracle_mod, oracle_orient_cache, shape, units, sigma, flat):
    vol, (R, keep, _, _), (oR, okeep) = _case(oracle_mod, oracle_orient_cache, shape, units, sigma, flat)
    assert np.array_equal(keep, okeep), "keep differs at %d voxels" % int((keep != okeep).sum())
    bad = R.view(np.uint32) != oR.view(np.uint32)
    assert not bad.any(), "R differs at %d values" % int(bad.sum())
    if min(shape) < 3:
        assert not keep.any() and np.array_equal(R, np.broadcast_to(np.eye(3, dtype=np.float32)[:, :, None, None, None],
                                                                     R.shape))
    elif flat:
        nx = vol.shape[2]
        # deep inside the flat half every window is flat: rejected
        assert not keep[:, :, : nx // 2 - int(3 * sigma) - 1].any()
        assert keep.any()
    else:
        assert keep.mean() > 0.5, keep.mean()
    print("%s units %s sigma %g: %d of %d voxels kept" % (shape, units, sigma, int(keep.sum()), keep.size))


@pytest.mark.parametrize("shape,units,sigma,flat", ORIENT_CASES[:4])
def test_two_jacobi_solvers_agree(api, oracle_mod, oracle_orient_cache, shape, units, sigma, flat):
    """s3d_eigen3 (the library's) and orc_eigen3 (the oracle's) on every kept voxel's structure tensor."""
    _, (_, keep, A, _), _ = _case(oracle_mod, oracle_orient_cache, shape, units, sigma, flat)
    n = 0
    for idx in zip(*np.nonzero(keep)):
        a = A[(slice(None),) + idx]
        M = [a[0], a[1], a[2], a[1], a[3], a[4], a[2], a[4], a[5]]
        Q, L = drr.eigen3(M)
        oQ, oL = oracle_mod.eigen3(M)
        assert np.array_equal(Q.view(np.uint64), oQ.view(np.uint64)) and np.array_equal(L.view(np.uint64),
                                                                                        oL.view(np.uint64)), idx
        n += 1
    assert n > 0


def _ramp(shape):
    """A volume that varies along x only: gy = gz = 0 exactly, so d = 0 exactly for the second column (the
    eigenvector e_z of a zero eigenvalue), whose sign is then -1 by sift.c's `d > 0` rule."""
    nx, ny, nz = shape
    x = np.arange(nx, dtype=np.float32)
    return np.ascontiguousarray(np.broadcast_to(x * x * np.float32(0.01) + x, (nz, ny, nx)))


def test_sign_rule_on_a_ramp(api):
    vol = _ramp((14, 9, 8))
    for sigma in (1.5, 3.0):
        R, keep, _, _ = drr.orient(vol, sigma, (1, 1, 1))
        oR, okeep = drr.oracle_orient(vol, sigma, (1, 1, 1))
        assert np.array_equal(keep, okeep) and keep.any()
        assert np.array_equal(R.view(np.uint32), oR.view(np.uint32))
        k = keep == 1
        assert np.all(R[2, 1][k] == -1.0), "column 1 of a kept ramp voxel is -e_z"
