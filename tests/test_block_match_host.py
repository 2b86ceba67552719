"""CPU (not gpu): the host side of block matching (include/sift3d_amd.h, "Block matching") -- the numpy restatement
(tests/block_match_restatement.py) against analysis, the C trimmed fit (ctypes, no device) against numpy's SVD and
lstsq, the refusals of the C entries on made-up pointers (they check their arguments before any device call), the
Python refusals, and the driver's restatement on the pairs below.

The tolerances of the fit.  200 points in a 64^3 box: the scatter matrices have entries near 200 * 64^2 / 12 ~ 7e4 and
condition numbers of a few units, so a backward-stable fit carries L to ~1e-15 and t to ~1e-13 voxel.  The bounds
asked, 1e-9 per entry of L and 1e-7 voxel for t, are five orders above that; orthonormality is held to 1e-12.

The driver's cases (figures of the restatement, recorded when the cases were chosen):
  pair48: 48^3 smooth noise (sigma 2 voxels), rotation 5 degrees about (1, 2, 3) through the centre, shift
      (1.5, -1, 0.7), gain ramp 0.6 .. 1.4 along x and offset 0.25 on the fixed side, levels 2, the defaults else:
      corner error 5.447 at the start, 0.127 at the end; with the sub-voxel step switched off 0.234 (level 0 stops
      after two iterations with every kept displacement 0).
  pair56: 56^3 smooth noise (sigma 3), rotation 4 degrees, shift (9, -8, 7), keep_blocks 1: start 17.04; levels 1 ends
      at 11.26 (the shift is outside the search cube), levels 3 at 0.065."""
import os
import re

import numpy as np
import pytest

from tests import block_match_restatement as bm
from tests.test_warp import ref_warp

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTED = ("sift3d_amd_block_match_work_bytes", "sift3d_hip_block_match", "sift3d_amd_fit_trimmed",
            "sift3d_amd_block_register_default_params", "sift3d_amd_block_register_struct_bytes",
            "sift3d_amd_block_register_work_floats", "sift3d_amd_block_register_device")


# ---- content shared with tests/test_block_match.py -------------------------------------------------------------------
def smooth_noise(shape, seed, sigma=2.0):
    rng = np.random.default_rng(seed)
    a = np.fft.fftn(rng.standard_normal(shape))
    for ax, n in enumerate(shape):
        g = np.exp(-2.0 * (np.pi * sigma) ** 2 * np.fft.fftfreq(n) ** 2)
        a = a * g.reshape([-1 if d == ax else 1 for d in range(3)])
    a = np.fft.ifftn(a).real
    return (a / a.std()).astype(F32)


def rigid_about_centre(deg, axis, shift, shape):
    ax = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    th = np.deg2rad(deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    c = (np.array(shape[::-1], np.float64) - 1) / 2.0
    return np.concatenate([R, (c - R @ c + np.asarray(shift, np.float64))[:, None]], 1)


def make_pair(n, deg, shift, sigma):
    """(F, M, A_true): M smooth noise + 3; F = M seen through A_true, times a gain ramp 0.6 .. 1.4 along x, + 0.25"""
    M = smooth_noise((n, n, n), 3, sigma) + F32(3.0)
    A = rigid_about_centre(deg, (1, 2, 3), shift, M.shape)
    W = ref_warp(M, A, M.shape, "linear", 0.0)[0].astype(F32)
    return (W * np.linspace(0.6, 1.4, n, dtype=F32)[None, None, :] + F32(0.25)).astype(F32), M, A


_PAIRS = {}


def pair48():
    if 48 not in _PAIRS:
        _PAIRS[48] = make_pair(48, 5.0, (1.5, -1.0, 0.7), 2.0)
    return _PAIRS[48]


def pair56():
    if 56 not in _PAIRS:
        _PAIRS[56] = make_pair(56, 4.0, (9.0, -8.0, 7.0), 3.0)
    return _PAIRS[56]


def period2(shape):
    """period 2 along x, varying along y and z: a shift by 2 along x is an exact copy away from the faces"""
    z, y, x = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    return ((x % 2) * (1 + (y * 7 + z * 3) % 5) + ((y * 5 + z) % 3)).astype(F32)


def ints(shape, seed, lo=-200, hi=200):
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(F32)


# ---- the restatement against analysis --------------------------------------------------------------------------------
def _on_grid_blocks(shape, s):
    """the blocks (bx, by, bz) whose block shifted by s lies on the grid and does not cross np.roll's wrap"""
    out = []
    for bz in range(shape[0] // 4):
        for by in range(shape[1] // 4):
            for bx in range(shape[2] // 4):
                lo = [4 * b + d for b, d in zip((bx, by, bz), s)]
                if all(l >= max(d, 0) and l + 3 <= n - 1 + min(d, 0) for l, d, n in zip(lo, s, shape[::-1])):
                    out.append((bx, by, bz))
    return out


@pytest.mark.parametrize("R,s", [(1, (1, 0, -1)), (3, (2, -3, 1)), (3, (0, 0, 0)), (6, (-6, 5, 2))])
def test_integer_shift_is_found_exactly(R, s):
    """W(p) = F(p - s) on random integer content: every block whose candidate s keeps the shifted block on the grid
    scores cc == 1.0 exactly there (c, vF and vW are then the same bits) and returns d = s.  The contract's sub-voxel
    formula gives 0 only where the two neighbours score alike (the next test); on random content they do not, and
    the offset is the vertex of the parabola through (c-, 1, c+): small, never beyond half a voxel."""
    shape = (20, 24, 28)
    F = ints(shape, 5)
    W = np.roll(F, (s[2], s[1], s[0]), (0, 1, 2))           # W[p] = F[p - s]; wraps at the faces
    disp, cc, var = bm.block_match(F, W, R)
    no_step = bm.block_match(F, W, R, subvoxel=False)[0]
    blocks = _on_grid_blocks(shape, s)
    assert len(blocks) >= 8
    worst = 0.0
    for bx, by, bz in blocks:
        assert cc[bz, by, bx] == F32(1.0)
        assert tuple(no_step[:, bz, by, bx]) == s
        worst = max(worst, float(np.abs(disp[:, bz, by, bx] - np.array(s, F32)).max()))
    print("largest sub-voxel offset at an exact integer shift, random content: %.4g" % worst)
    assert worst < 0.05                                      # the neighbours of a cc = 1 peak in noise score ~0: den ~ -2


@pytest.mark.parametrize("R,s", [(3, (0, 0, 0)), (3, (1, -2, 1)), (2, (-2, 0, 2))])
def test_integer_shift_has_zero_subvoxel_offset_on_symmetric_content(R, s):
    """Integer content that is even about every block's centre on every axis (period 8: a b b a c d d c): the two
    neighbours of the true shift see mirror images of one another, their sums are exact, c- == c+ in bits, and the
    offset is exactly 0: disp == s, cc == 1."""
    shape = (16, 16, 24)
    g = [np.array(v, np.float64) for v in ([3, -5, -5, 3, 7, 1, 1, 7], [2, 9, 9, 2, -4, 6, 6, -4], [1, 8, 8, 1, 5, -7, -7, 5])]
    z, y, x = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    F = (g[0][x % 8] + 11 * g[1][y % 8] + 101 * g[2][z % 8]).astype(F32)
    W = np.roll(F, (s[2], s[1], s[0]), (0, 1, 2))
    disp, cc, _ = bm.block_match(F, W, R)
    blocks = _on_grid_blocks(shape, s)
    assert len(blocks) >= 4
    for bx, by, bz in blocks:
        assert cc[bz, by, bx] == F32(1.0) and tuple(disp[:, bz, by, bx]) == s, (bx, by, bz)


@pytest.mark.parametrize("alpha,beta", [(-0.5, 7.0), (-3.0, -2.0)])
def test_negative_gain_and_offset_score_one(alpha, beta):
    F = ints((12, 12, 16), 7)
    W = (F32(alpha) * F + F32(beta)).astype(F32)
    disp, cc, var = bm.block_match(F, W, 2)
    assert np.all(np.abs(cc.astype(np.float64) - 1.0) <= 1e-9)
    assert np.array_equal(np.round(disp), np.zeros_like(disp))
    assert np.all(var > 0)


def test_subvoxel_formula():
    assert bm.subvoxel_offset(0.5, 1.0, 0.5) == 0.0
    assert bm.subvoxel_offset(0.25, 1.0, 0.75) == pytest.approx(0.25)          # 0.5 (-0.5) / (-1)
    assert bm.subvoxel_offset(0.75, 1.0, 0.25) == pytest.approx(-0.25)
    assert bm.subvoxel_offset(1.0, 1.0, 0.0) == -0.5                           # clamped: 0.5 / -1 = -0.5 exactly
    assert bm.subvoxel_offset(0.0, 1.0, 1.0) == 0.5
    assert bm.subvoxel_offset(1.0, 1.0, 1.0) == 0.0                            # den == 0: no step
    # a parabola sampled at -1, 0, 1 gives its vertex back
    v = 0.3
    c = [1.0 - 0.2 * (t - v) ** 2 for t in (-1.0, 0.0, 1.0)]
    assert bm.subvoxel_offset(*c) == pytest.approx(v, abs=1e-12)


def test_ties_go_to_the_smallest_displacement():
    """period 2 along x: d = (-2, 0, 0), (0, 0, 0) and (2, 0, 0) tie exactly at cc = 1 wherever they are on the grid;
    the winner is d = 0, and the tied neighbours at +-1 are equal, so the sub-voxel offset is 0"""
    shape = (8, 8, 24)
    F = period2(shape)
    assert np.array_equal(F[:, :, 2:], F[:, :, :-2])         # the premise: a shift by 2 is an exact copy
    disp, cc, _ = bm.block_match(F, F, 3)
    assert np.all(cc == 1) and np.array_equal(disp, np.zeros_like(disp))


def test_equal_norm_tie_takes_the_smaller_k():
    """two exact copies of the block at dx = -2 and dx = +2 and none at 0: equal cc = 1, equal |d|^2, so the smaller
    k (dx = -2) wins; it sits on the face of the R = 2 cube, so there is no sub-voxel step along x"""
    shape = (4, 4, 12)
    blk = ints((4, 4, 4), 11)
    F = np.zeros(shape, F32)
    F[:, :, 4:8] = blk                                       # block bx = 1
    W = ints(shape, 12)
    W[:, :, 2:6] = blk
    W[:, :, 6:10] = blk
    disp, cc, _ = bm.block_match(F, W, 2)
    assert cc[0, 0, 1] == 1 and tuple(disp[:, 0, 0, 1]) == (-2, 0, 0)
    assert cc[0, 0, 0] == -1 and cc[0, 0, 2] == -1           # all-zero blocks


def test_validity():
    shape = (9, 14, 19)                                      # not multiples of 4: 2 x 3 x 4 blocks
    F = ints(shape, 3)
    W = (F + ints(shape, 4, -3, 3)).astype(F32)
    disp, cc, var = bm.block_match(F, W, 1)
    assert cc.shape == (2, 3, 4) and disp.shape == (3, 2, 3, 4) and var.dtype == np.float64
    assert np.all(cc >= 0)
    # a hole in the fixed mask invalidates exactly its block
    VF = np.ones(shape, F32)
    VF[5, 9, 14] = 0.25                                      # block (3, 2, 1)
    d2, c2, v2 = bm.block_match(F, W, 1, VF, None)
    bad = np.zeros(cc.shape, bool)
    bad[1, 2, 3] = True
    assert np.array_equal(c2 < 0, bad) and c2[1, 2, 3] == -1 and v2[1, 2, 3] == 0 and not d2[:, 1, 2, 3].any()
    assert np.array_equal(c2[~bad], cc[~bad])
    # a constant block and an all-zero block are invalid; a constant W neighbourhood leaves no candidate
    F3 = F.copy()
    F3[0:4, 0:4, 0:4] = 7.0
    F3[4:8, 4:8, 4:8] = 0.0
    c3 = bm.block_match(F3, W, 1)[1]
    assert c3[0, 0, 0] == -1 and c3[1, 1, 1] == -1 and (c3 >= 0).sum() == c3.size - 2
    c4 = bm.block_match(F, np.full(shape, 5.0, F32), 1)[1]
    assert np.all(c4 == -1)
    # candidates leaving the grid: a corner block at R = 1 keeps the candidates with d >= 0 only; with W an exact copy
    # shifted by -1 along x (content moved to lower x) the corner block cannot follow
    Wm = np.roll(F, -1, 2)
    d5 = bm.block_match(F, Wm, 1)[0]
    assert d5[0, 0, 0, 1] <= -0.5 and d5[0, 0, 0, 0] >= 0    # block 1 follows to dx = -1, block 0 cannot
    # all 64 W voxels of a candidate must be in V_W
    VW = np.ones(shape, F32)
    VW[:] = 0
    assert np.all(bm.block_match(F, W, 1, None, VW)[1] == -1)


# ---- the C fit against numpy ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


def _points(n=200, seed=0):
    return np.random.default_rng(seed).uniform(0, 64, (n, 3))


def _agree(T, L, t):
    assert np.abs(T[:, :3] - L).max() <= 1e-9
    assert np.abs(T[:, 3] - t).max() <= 1e-7


RIGID = rigid_about_centre(17.0, (2, -1, 3), (4.0, -3.0, 2.0), (64, 64, 64))
AFFINE = RIGID + np.array([[0.05, 0.02, 0, 0], [-0.03, -0.04, 0.01, 0], [0, 0.02, 0.06, 0]])


@pytest.mark.parametrize("model,A", [("rigid", RIGID), ("affine", AFFINE), ("affine", RIGID),
                                     ("translation", np.eye(3, 4) + np.array([[0, 0, 0, 3.5]] * 3))])
def test_exact_maps_are_recovered(hip, model, A):
    src = _points()
    dst = src @ A[:, :3].T + A[:, 3]
    T, used, its = hip.fit_trimmed(src, dst, model, 1.0)
    assert used.all() and its == 0
    _agree(T, A[:, :3], A[:, 3])
    ref = bm.fit_trimmed(src, dst, model, 1.0)
    _agree(T, ref[0][:, :3], ref[0][:, 3])
    if model == "rigid":
        L = T[:, :3]
        assert np.abs(L.T @ L - np.eye(3)).max() <= 1e-12 and np.linalg.det(L) > 0


def test_noisy_pairs_agree_with_numpy(hip):
    src = _points(seed=1)
    dst = src @ AFFINE[:, :3].T + AFFINE[:, 3] + np.random.default_rng(2).normal(0, 0.5, src.shape)
    for model in ("rigid", "affine", "translation"):
        T, used, its = hip.fit_trimmed(src, dst, model, 1.0)
        L, t = bm.fit(src, dst, model)
        _agree(T, L, t)
        got, want = hip.fit_trimmed(src, dst, model, 0.6), bm.fit_trimmed(src, dst, model, 0.6)
        assert np.array_equal(got[1], want[1]) and got[2] == want[2] and got[1].sum() == 120
        _agree(got[0], want[0][:, :3], want[0][:, 3])


def test_reflection_prone_set_stays_a_rotation(hip):
    """nearly planar points whose best orthogonal map is a reflection: det = +1 all the same"""
    rng = np.random.default_rng(5)
    src = _points(seed=4)
    src[:, 2] = 30.0 + 1e-3 * rng.standard_normal(len(src))
    dst = src.copy()
    dst[:, 2] = 60.0 - dst[:, 2]                             # mirrored through the plane: a reflection fits exactly
    T, _, _ = hip.fit_trimmed(src, dst, "rigid", 1.0)
    L = T[:, :3]
    assert abs(np.linalg.det(L) - 1.0) <= 1e-12 and np.abs(L.T @ L - np.eye(3)).max() <= 1e-12
    ref = bm.fit_trimmed(src, dst, "rigid", 1.0)[0]
    assert np.abs(L - ref[:, :3]).max() <= 1e-6              # the rotation about the in-plane axes is ill-determined


@pytest.mark.parametrize("model,A", [("rigid", RIGID), ("affine", AFFINE)])
def test_trimming_removes_gross_outliers(hip, model, A):
    """40 % outliers stay below 1 - keep = 50 %: the exact map comes back and no outlier is used; keep = 1 does not"""
    rng = np.random.default_rng(9)
    src = _points(seed=8)
    dst = src @ A[:, :3].T + A[:, 3]
    out = rng.permutation(len(src))[:80]
    dst[out] += rng.uniform(15, 40, (80, 3)) * rng.choice([-1, 1], (80, 3))
    T, used, its = hip.fit_trimmed(src, dst, model, 0.5)
    _agree(T, A[:, :3], A[:, 3])
    assert used.sum() == 100 and not used[out].any() and its >= 1
    T1, used1, _ = hip.fit_trimmed(src, dst, model, 1.0)
    assert used1.all() and np.abs(T1 - A).max() > 1e-3


def test_anisotropic_scales_make_rigid_physical(hip):
    s = np.array([0.7, 0.7, 2.5])
    src = _points(seed=12)
    phys = (src * s) @ RIGID[:, :3].T + RIGID[:, 3]
    dst = phys / s
    T, _, _ = hip.fit_trimmed(src, dst, "rigid", 1.0, scale_src=s, scale_dst=s)
    L = T[:, :3] * s[:, None] / s[None, :]                   # S_dst T S_src^-1
    assert np.abs(L.T @ L - np.eye(3)).max() <= 1e-12
    assert np.abs(L - RIGID[:, :3]).max() <= 1e-9 and np.abs(T[:, 3] * s - RIGID[:, 3]).max() <= 1e-7
    assert np.abs(T[:, :3].T @ T[:, :3] - np.eye(3)).max() > 1e-3        # not orthonormal in voxels
    plain = hip.fit_trimmed(src, dst, "rigid", 1.0)[0]
    assert np.abs(plain - T).max() > 1e-3


def test_fit_refusals(hip):
    import ctypes as C
    L = hip.lib()
    src = _points(10)
    dst = src + 1.0
    T = np.zeros(12)
    its = C.c_int(0)
    dp = hip._dptr

    def run(s=src, d=dst, n=10, model=1, keep=0.5, max_iter=20, ss=None, sd=None, T_=T, its_=its):
        return L.sift3d_amd_fit_trimmed(None if s is None else dp(s), None if d is None else dp(d), n, model, keep,
                                        max_iter, None if ss is None else dp(np.asarray(ss, np.float64)),
                                        None if sd is None else dp(np.asarray(sd, np.float64)),
                                        None if T_ is None else dp(T_), None, None if its_ is None else C.byref(its_))
    assert run() == 0
    for kw in (dict(s=None), dict(d=None), dict(T_=None), dict(its_=None), dict(model=3), dict(model=-1),
               dict(n=2), dict(n=0), dict(model=2, n=3), dict(model=0, n=0), dict(keep=0.0), dict(keep=1.5),
               dict(keep=float("nan")), dict(keep=-0.5), dict(max_iter=-1), dict(ss=[1, 0, 1]), dict(sd=[1, 1, -2]),
               dict(ss=[1, float("inf"), 1]), dict(sd=[float("nan"), 1, 1])):
        assert run(**kw) == -1, kw
    bad = src.copy()
    bad[3, 1] = np.nan
    assert run(s=bad) == -1
    bad = dst.copy()
    bad[9, 2] = np.inf
    assert run(d=bad) == -1
    line = np.outer(np.arange(10.0), [1.0, 2.0, -1.0]) + 5.0
    assert run(s=line, d=line) == -1 and run(s=src, d=line) == -1        # collinear: rigid refuses either side
    assert run(s=line, d=line, model=0) == 0                              # translation has no degenerate set
    same = np.tile([[1.0, 2.0, 3.0]], (10, 1))
    assert run(s=same, d=same) == -1 and run(s=same, d=same, model=2) == -1
    plane = src.copy()
    plane[:, 2] = 2.0 * plane[:, 0] - plane[:, 1]
    assert run(s=plane, d=plane, model=2) == -1 and run(s=plane, d=plane, model=1) == 0
    assert bm.fit_trimmed(plane, plane, "affine", 1.0) is None and bm.fit_trimmed(line, line, "rigid", 1.0) is None


# ---- the entries' refusals, the sizes and the wrappers ---------------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, "include", "sift3d_amd.h")) as f:
        return f.read()


def test_symbols_exported_and_declared(hip):
    from sift3d_amd import _native, api
    L = _native.load()
    text = _header()
    assert "Block matching" in text
    for name in EXPORTED:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\(" % name, text), name
    assert hip.BLOCK_MAX_RADIUS == int(re.search(r"#define SIFT3D_AMD_BLOCK_MAX_RADIUS (\d+)", text).group(1)) == 6
    for fn in ("block_match", "fit_trimmed", "block_register"):
        assert callable(getattr(hip, fn))
    for fn in ("block_match", "fit_transform", "register_blocks"):
        assert callable(getattr(api, fn))
    p = hip.block_register_params()
    assert (p.model, p.levels, p.iterations, p.radius, p.keep_blocks, p.keep_inliers, p.tol) == (1, 3, 5, 3, 0.5, 0.5, 0.01)
    assert list(p.spacing_fixed) == [1, 1, 1] and list(p.spacing_moving) == [1, 1, 1]


def _pad4(x):
    return (x + 3) & ~3


def test_work_sizes_agree(hip):
    L = hip.lib()
    assert L.sift3d_amd_block_match_work_bytes(64, 64, 64, 3) == 0
    for (ox, oy, oz), (nx, ny, nz) in (((32, 32, 32), (32, 32, 32)), ((70, 35, 33), (41, 50, 37))):
        for levels in (1, 2, 3):
            for mf in (0, 1):
                for mm in (0, 1):
                    want = _pad4(6 * (ox // 4) * (oy // 4) * (oz // 4)) + 2 * _pad4(ox * oy * oz)
                    want += 0 if mm else _pad4(nx * ny * nz)
                    f, m = (ox, oy, oz), (nx, ny, nz)
                    for _ in range(1, levels):
                        f, m = tuple((d + 1) // 2 for d in f), tuple((d + 1) // 2 for d in m)
                        want += (1 + mf) * _pad4(f[0] * f[1] * f[2]) + (1 + mm) * _pad4(m[0] * m[1] * m[2])
                    assert L.sift3d_amd_block_register_work_floats(ox, oy, oz, nx, ny, nz, levels, mf, mm) == want
    for bad in ((0, 8, 8, 8, 8, 8, 1, 0, 0), (8, 8, 8, 8, 0, 8, 1, 0, 0), (8, 8, 8, 8, 8, 8, 0, 0, 0),
                (8, 8, 8, 8, 8, 8, 7, 0, 0), (7, 8, 8, 8, 8, 8, 1, 0, 0), (14, 16, 16, 16, 16, 16, 2, 0, 0),
                (16, 16, 16, 16, 16, 16, 3, 0, 0)):
        assert L.sift3d_amd_block_register_work_floats(*bad) == 0, bad
    assert L.sift3d_amd_block_register_work_floats(15, 16, 16, 3, 3, 3, 2, 0, 0) > 0       # 15 -> 8


@pytest.fixture(scope="module")
def bufs(hip):
    """made-up addresses without a device; real allocations covering every range named below with one, so that a
    regressed check could not make a kernel touch unmapped memory"""
    from sift3d_amd import api
    if api.device_available():
        b = [hip.lib().sift3d_hip_malloc(1 << 18) for _ in range(3)]
        assert all(b)
        yield b
        for p in b:
            hip.lib().sift3d_hip_free(p)
    else:
        yield [0x1000000, 0x2000000, 0x3000000]


VB = 8 * 8 * 8 * 4


def test_match_refusals(hip, bufs):
    """8^3: F, W and the masks (2048 B each) in buffer 0; disp (96 B), cc (32 B), var (64 B) in buffer 1"""
    L = hip.lib()
    A, B, _ = bufs
    base = dict(F=A, nx=8, ny=8, nz=8, W=A + 4096, VF=A + 8192, VW=A + 16384, r=3, disp=B, cc=B + 1024, var=B + 2048)

    def run(a):
        return L.sift3d_hip_block_match(a["F"], a["nx"], a["ny"], a["nz"], a["W"], a["VF"], a["VW"], a["r"], a["disp"],
                                        a["cc"], a["var"], None, None)
    for ch in (dict(F=None), dict(W=None), dict(disp=None), dict(cc=None), dict(var=None),
               dict(nx=0), dict(ny=-4), dict(nz=0), dict(nx=3), dict(ny=2), dict(nz=1),
               dict(r=0), dict(r=7), dict(r=-1),
               dict(F=A + 2), dict(W=A + 4097), dict(VF=A + 8194), dict(VW=A + 16385), dict(disp=B + 2),
               dict(cc=B + 1025), dict(var=B + 2052),
               dict(disp=A), dict(disp=A + VB - 4), dict(cc=A + 4096 + VB - 4), dict(var=A + 4096 - 56),
               dict(disp=A + 8192), dict(cc=A + 16384 + VB - 4), dict(var=A + 8192 + 8), dict(VF=None, cc=A + 16384),
               dict(cc=B + 92), dict(var=B + 88), dict(var=B + 1024 - 56), dict(cc=B + 2048 + 60), dict(disp=B + 1024 - 4)):
        a = dict(base)
        a.update(ch)
        assert run(a) == -1, ch


def test_driver_refusals(hip, bufs):
    """16^3 volumes (16 KB) and masks in buffer 0; the work buffer in buffer 2"""
    import ctypes as C
    L = hip.lib()
    Abuf, _, Wbuf = bufs
    vol = 16 * 16 * 16 * 4
    need = L.sift3d_amd_block_register_work_floats(16, 16, 16, 16, 16, 16, 2, 1, 1) * 4
    assert 0 < need <= (1 << 18)
    A = np.eye(3, 4).reshape(12).copy()
    res = hip.BlockRegisterResult()

    def run(F=Abuf, M=Abuf + vol, WF=Abuf + 2 * vol, WM=Abuf + 3 * vol, dims=(16,) * 6, A_=A, work=Wbuf, res_=res, **kw):
        p = hip.block_register_params(levels=2)
        for k, v in kw.items():
            setattr(p, k, (C.c_double * 3)(*v) if k.startswith("spacing") else v)
        return L.sift3d_amd_block_register_device(F, *dims[:3], M, *dims[3:], WF, WM,
                                                  None if A_ is None else hip._dptr(A_), C.byref(p),
                                                  None if res_ is None else C.byref(res_), work, None)
    bad_A = A.copy()
    bad_A[5] = np.nan
    for kw in (dict(F=None), dict(M=None), dict(A_=None), dict(res_=None), dict(work=None),
               dict(dims=(0, 16, 16, 16, 16, 16)), dict(dims=(16, 16, 16, 16, -1, 16)),
               dict(dims=(15, 16, 16, 16, 16, 16), levels=3), dict(dims=(7, 16, 16, 16, 16, 16), levels=1),
               dict(levels=3), dict(levels=0), dict(levels=7), dict(A_=bad_A), dict(model=3), dict(model=-1),
               dict(iterations=0), dict(iterations=65), dict(radius=0), dict(radius=7), dict(keep_blocks=0.0),
               dict(keep_blocks=1.01), dict(keep_inliers=0.0), dict(keep_inliers=float("nan")), dict(tol=-1.0),
               dict(tol=float("inf")), dict(spacing_fixed=(1, 0, 1)), dict(spacing_moving=(1, 1, float("nan"))),
               dict(F=Abuf + 2), dict(M=Abuf + vol + 1), dict(WF=Abuf + 2 * vol + 2), dict(WM=Abuf + 3 * vol + 3),
               dict(work=Wbuf + 4), dict(work=Abuf), dict(work=Abuf + vol - 8), dict(work=Abuf + 4 * vol - 8),
               dict(work=Abuf - need + 8), dict(WF=Wbuf + need - 4), dict(WM=Wbuf + 8)):
        assert run(**kw) == -1, kw


def test_python_refusals():
    from sift3d_amd import api
    F = np.zeros((32, 32, 32), F32)
    for kw, word in ((dict(model="similarity"), "model"), (dict(levels=0), "levels"), (dict(levels=7), "levels"),
                     (dict(levels=4), "levels"), (dict(iterations=0), "iterations"), (dict(iterations=65), "iterations"),
                     (dict(radius=0), "radius"), (dict(radius=7), "radius"), (dict(radius=2.0), "radius"),
                     (dict(keep_blocks=0), "keep_blocks"), (dict(keep_inliers=1.5), "keep_inliers"),
                     (dict(tol=-1), "tol"), (dict(tol=float("nan")), "tol"), (dict(A=np.eye(4)), "A"),
                     (dict(A=np.full((3, 4), np.inf)), "A"), (dict(A=np.eye(3, 4), init="centroid"), "init"),
                     (dict(spacing_fixed=(1, 1)), "spacing_fixed"), (dict(spacing_moving=(1, -1, 1)), "spacing_moving"),
                     (dict(mask_fixed=np.ones((4, 4, 4))), "mask_fixed"), (dict(mask_moving=np.ones((2, 2, 2))), "mask_moving")):
        with pytest.raises(ValueError, match=word):
            api.register_blocks(F, F, **kw)
    for kw, word in ((dict(radius=0), "radius"), (dict(radius=7), "radius"), (dict(transform=np.eye(4)), "transform"),
                     (dict(mask_fixed=np.ones((4, 4, 4))), "mask_fixed")):
        with pytest.raises(ValueError, match=word):
            api.block_match(F, F, **kw)
    with pytest.raises(ValueError, match="fixed"):
        api.block_match(np.zeros((3, 8, 8), F32), np.zeros((3, 8, 8), F32))
    pts = np.random.default_rng(0).uniform(0, 9, (8, 3))
    for args, kw, word in (((pts, pts), dict(model="similarity"), "model"), ((pts, pts), dict(keep=0), "keep"),
                           ((pts, pts), dict(keep=2), "keep"), ((pts[:, :2], pts[:, :2]), {}, "src"),
                           ((pts, pts[:4]), {}, "dst"), ((pts, pts), dict(spacing_src=(1, 2)), "spacing_src"),
                           ((pts, pts), dict(spacing_dst=(0, 1, 1)), "spacing_dst"), ((pts, pts), dict(max_iter=-1), "max_iter"),
                           ((pts[:2], pts[:2]), {}, "degenerate"), ((pts * [1, 1, 0], pts), dict(model="affine"), "degenerate")):
        with pytest.raises(ValueError, match=word):
            api.fit_transform(*args, **kw)
    fit = api.fit_transform(pts, pts + [1.0, 2.0, 3.0], "translation", keep=1.0)
    assert np.allclose(fit.A, np.eye(3, 4) + [[0, 0, 0, 1], [0, 0, 0, 2], [0, 0, 0, 3]]) and fit.used.all()


# ---- the driver's restatement ----------------------------------------------------------------------------------------
def test_driver_restatement_recovers_the_48_pair_and_needs_the_subvoxel_step():
    F, M, At = pair48()
    start = bm.corner_move(np.eye(3, 4), At, F.shape)
    A, trail, stop = bm.register(F, M, levels=2)
    err = bm.corner_move(A, At, F.shape)
    A0, trail0, _ = bm.register(F, M, levels=2, subvoxel=False)
    err0 = bm.corner_move(A0, At, F.shape)
    print("pair48: start %.4f, end %.4f (%s, %d iterations), without the sub-voxel step %.4f"
          % (start, err, stop, len(trail), err0))
    assert err < 0.5 and err < start / 10.0
    assert err0 > err
    assert [e.level for e in trail] == sorted((e.level for e in trail), reverse=True)
    assert all(e.n_selected == -(-e.n_valid // 2) and e.n_used == -(-e.n_selected // 2) for e in trail)


def test_levels_find_what_one_level_cannot():
    F, M, At = pair56()
    start = bm.corner_move(np.eye(3, 4), At, F.shape)
    one = bm.corner_move(bm.register(F, M, levels=1, keep_blocks=1.0)[0], At, F.shape)
    three = bm.corner_move(bm.register(F, M, levels=3, keep_blocks=1.0)[0], At, F.shape)
    print("pair56: start %.4f, levels 1 %.4f, levels 3 %.4f" % (start, one, three))
    assert three < 0.5 and three < start / 10.0
    assert one > 5.0
