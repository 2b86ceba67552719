"""CPU (not gpu): "Affine refinement under a linear intensity map (NCC)" (include/sift3d_amd.h) without a device.  The
host entries sift3d_amd_affine_ncc_fit and sift3d_amd_affine_ncc_lm_step against the numpy restatement
(tests/affine_ncc_restatement.py) on records the restatement makes, every argument refusal of the device entries (which
check their arguments before any device call), and the restatement's driver on the pair that tests/test_affine_ncc.py
runs on the device: it finds the true map whatever gain and offset the moving volume carries, where the MSD driver
does not."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import affine_ncc_restatement as an
from tests import affine_refine_restatement as ar
from tests.test_affine_refine_host import TOL, _a, bufs, gaussians, inverse  # noqa: F401  (bufs: a fixture)
from tests.test_warp import about_center, ref_warp, rot

MAPS = [(1.0, 0.0), (-0.5, 0.0), (0.5, 32.0)]               # (gain, offset) applied to the moving volume


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


def mapped_case(gain=1.0, offset=0.0):
    """fixed = a crop of a 40^3 sum of Gaussians (times 100); moving = the same crop of that volume pulled through the
    inverse of the integer translation T = (2, -1, 1), then mapped as gain * m + offset: no zero fill inside the moving
    grid, and at T the fit's residual is 0 up to the rounding of the map"""
    S = gaussians((40, 40, 40), 7, k=6) * 100
    T = np.eye(3, 4)
    T[:, 3] = (2.0, -1.0, 1.0)
    pulled = ref_warp(S, inverse(T), S.shape, "linear", 0.0)[0].astype(np.float32)
    crop = (slice(8, 32),) * 3
    moving = (np.float32(gain) * pulled[crop] + np.float32(offset)).astype(np.float32)
    return np.ascontiguousarray(S[crop], np.float32), np.ascontiguousarray(moving), T


def small_record(seed=0, deg=4.0):
    F, M = gaussians((9, 10, 11), 3 + seed), gaussians((10, 9, 12), 4 + seed) * 3 + 1
    A = about_center(rot((1, 2, 3), deg), M.shape, F.shape, shift=(0.3, -0.2, 0.4))
    rec = an.record(F, M, A)
    assert 2 < rec.n < F.size
    return rec


# ---- symbols, sizes ------------------------------------------------------------------------------------------------
def test_symbols_exported_and_sizes_agree(hip):
    from sift3d_amd import _native, api
    L = _native.load()
    for name in ("sift3d_hip_affine_ncc_normal_eqs", "sift3d_amd_affine_ncc_normal_work_bytes",
                 "sift3d_amd_affine_ncc_fit", "sift3d_amd_affine_ncc_lm_step",
                 "sift3d_amd_affine_ncc_refine_work_bytes", "sift3d_amd_affine_ncc_refine_device"):
        assert hasattr(L, name), name
    for name in ("affine_ncc_normal_equations", "affine_ncc_fit", "affine_ncc_lm_step", "affine_ncc_refine"):
        assert callable(getattr(hip, name)), name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "sift3d_amd.h")).read()
    stated = int(re.search(r"#define SIFT3D_AMD_AFFINE_NCC_BYTES (\d+)", header).group(1))
    assert stated == 1488 == hip.AFFINE_NCC_BYTES == hip.AFFINE_NCC_RECORD_DTYPE.itemsize
    W = hip.lib().sift3d_amd_affine_ncc_normal_work_bytes
    assert W(5, 6, 7) == hip.SIMILARITY_GRID * 102 * 8 == W(512, 512, 512) == hip.affine_ncc_normal_work_bytes((7, 6, 5))
    assert W(0, 6, 7) == 0 and W(5, -1, 7) == 0 and W(5, 6, 0) == 0
    R = hip.lib().sift3d_amd_affine_ncc_refine_work_bytes
    assert R(8, 8, 8, 8, 8, 8, 1) == W(8, 8, 8) + stated                    # the library's record size
    assert R(8, 8, 8, 6, 6, 6, 2) == R(8, 8, 8, 6, 6, 6, 1) + 2 * (4 * 64 + 4 * 28)     # volumes, and room for masks
    assert R(8, 8, 8, 8, 8, 8, 0) == 0 and R(8, 8, 8, 8, 8, 8, 7) == 0 and R(8, 0, 8, 8, 8, 8, 1) == 0
    # nothing that existed changed its size
    S = hip.lib().sift3d_amd_affine_refine_struct_bytes
    assert [S(k) for k in range(7)] == [C.sizeof(hip.AffineRefineParams), C.sizeof(hip.AffineEvaluation),
                                        C.sizeof(hip.AffineRefineResult), 1264, 128, 6, 0]
    assert api.NccAffineRefinement._fields == ("A", "cost", "count", "accepted", "lambdas", "levels", "level_slices",
                                               "evaluations", "stop", "warped", "ncc", "gain", "offset")


# ---- the host entries against the restatement ----------------------------------------------------------------------
def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), (what, got, want)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fit_against_restatement(hip, seed):
    rec = small_record(seed)
    want = an.fit(rec)
    got = hip.affine_ncc_fit(rec)
    print("fit", got)
    close(got, want, "fit")
    assert 0 < abs(want.ncc) <= 1 and want.cost > 0
    # the residual of the regression, summed directly
    direct = rec.S_ff - 2 * (want.alpha * rec.S_fm + want.beta * rec.S_f) + want.alpha ** 2 * rec.S_mm \
        + 2 * want.alpha * want.beta * rec.S_m + rec.n * want.beta ** 2
    assert abs(direct / rec.n - want.cost) <= 1e-9 * rec.S_ff / rec.n


@pytest.mark.parametrize("mask", [0xFFF, 0x888, 0x001, 0x400, 0x5A5])
@pytest.mark.parametrize("lam", [0.0, 1e-3, 10.0])
def test_lm_step_against_restatement(hip, mask, lam):
    """The restatement solves by the header's Cholesky in the header's order, so the two agree far inside 1e-12
    relative; delta is exactly 0 outside the free set.  The solution is a solution: the residual of the 14 x 14 system
    on the free set is within Higham's bound for a Cholesky solve (tests/test_affine_refine_host.py)."""
    rec = small_record(mask % 3)
    got = hip.affine_ncc_lm_step(rec, mask, lam)
    want = an.lm_step(rec, mask, lam)
    assert got is not None and want is not None
    idx = ar.free_indices(mask)
    assert not got[[i for i in range(12) if i not in idx]].any()
    close(got, want, "delta")
    H, g = an.system14(rec, an.fit(rec))
    all14 = idx + [12, 13]
    Hf = H[np.ix_(all14, all14)]
    K = Hf + lam * np.diag(np.diag(Hf))
    full = np.linalg.solve(K, -g[all14])
    m = len(all14)
    bound = 8 * m * (m + 1) * 2.0 ** -53 * (np.linalg.norm(K, 2) * np.linalg.norm(full) + np.linalg.norm(g[all14]))
    assert np.linalg.norm(K[:, :len(idx)] @ (got[idx] - full[:len(idx)])) <= 2 * bound


def test_step_at_the_optimum_of_alpha_and_beta(hip):
    """(alpha, beta) of the fit zero b14[12] and b14[13] up to rounding: the step starts from the best intensity map"""
    rec = small_record(1)
    _, g = an.system14(rec, an.fit(rec))
    assert abs(g[12]) <= 1e-9 * (rec.S_mm + rec.S_ff) and abs(g[13]) <= 1e-9 * (abs(rec.S_m) + abs(rec.S_f))


def test_fit_and_step_refusals(hip):
    rec = small_record(0)
    L = hip.lib()
    raw = hip._ncc_record(rec)
    d = (C.c_double * 12)()
    out = (C.c_double * 4)()
    assert L.sift3d_amd_affine_ncc_fit(None, out) == -1 and L.sift3d_amd_affine_ncc_fit(raw.ctypes.data, None) == -1
    assert L.sift3d_amd_affine_ncc_lm_step(None, 0xFFF, 0.0, d) == -1
    assert L.sift3d_amd_affine_ncc_lm_step(raw.ctypes.data, 0xFFF, 0.0, None) == -1
    assert hip.affine_ncc_lm_step(rec, 0, 1e-3) is None                       # empty mask
    assert hip.affine_ncc_lm_step(rec, 0x1000, 1e-3) is None                  # a bit past the 12 parameters
    assert hip.affine_ncc_lm_step(rec, 0xFFF, -1.0) is None
    assert hip.affine_ncc_lm_step(rec, 0xFFF, float("nan")) is None
    assert hip.affine_ncc_lm_step(rec, 0xFFF, 1e-3) is not None
    for n in (0, 1):                                                          # n < 2: the fit is undefined
        few = rec._replace(n=n)
        assert hip.affine_ncc_fit(few) is None and an.fit(few) is None
        assert hip.affine_ncc_lm_step(few, 0xFFF, 1e-3) is None and an.lm_step(few, 0xFFF, 1e-3) is None
    # V_m == 0 from a constant moving volume (0.75 is exact, so are its sums)
    F = gaussians((6, 7, 8), 5)
    M = np.full((7, 8, 9), 0.75, np.float32)
    flat = an.record(F, M, about_center(rot((0, 0, 1), 10.0), M.shape, F.shape))
    assert flat.n > 2 and flat.S_mm - flat.S_m * flat.S_m / flat.n == 0.0
    assert hip.affine_ncc_fit(flat) is None and an.fit(flat) is None
    assert hip.affine_ncc_lm_step(flat, 0xFFF, 1e-3) is None and an.lm_step(flat, 0xFFF, 1e-3) is None
    out = np.zeros(4)
    assert L.sift3d_amd_affine_ncc_fit(hip._ncc_record(flat).ctypes.data, hip._dptr(out)) == -1 and np.isnan(out).all()
    # alpha == 0 (f uncorrelated with m: S_fm = S_f S_m / n): K is not positive definite
    flatf = rec._replace(S_fm=rec.S_f * rec.S_m / rec.n)
    assert an.fit(flatf).alpha == 0.0 == hip.affine_ncc_fit(flatf)[0]
    assert hip.affine_ncc_lm_step(flatf, 0xFFF, 1e-3) is None and an.lm_step(flatf, 0xFFF, 1e-3) is None
    # a free parameter with H_ii == 0, and H not positive definite
    Hz = rec.H.copy()
    Hz[5, :] = Hz[:, 5] = 0.0
    assert hip.affine_ncc_lm_step(rec._replace(H=Hz), 0xFFF, 1e-3) is None
    assert hip.affine_ncc_lm_step(rec._replace(H=-rec.H), 0xFFF, 1e-3) is None


# ---- the device entries refuse bad arguments before any device call --------------------------------------------
def test_normal_equations_refusals(hip, bufs):  # noqa: F811
    L = hip.lib()
    F, M, R, W = bufs
    keep, ident = _a(np.eye(3, 4))

    def call(F=F, o=(8, 8, 8), M=M, n=(8, 8, 8), A=ident, R=R, W=W, WF=None, WM=None):
        return L.sift3d_hip_affine_ncc_normal_eqs(F, *o, M, *n, A, R, W, None, WF, WM)
    work, rb = hip.affine_ncc_normal_work_bytes(), hip.AFFINE_NCC_BYTES
    cases = [dict(F=None), dict(M=None), dict(A=None), dict(R=None), dict(W=None),
             dict(o=(0, 8, 8)), dict(o=(8, -1, 8)), dict(o=(8, 8, 0)), dict(n=(0, 8, 8)), dict(n=(8, 8, -2)),
             dict(F=F + 2), dict(M=M + 1), dict(R=R + 4), dict(W=W + 4), dict(WF=F + 4096 + 2), dict(WM=M + 4096 + 1),
             dict(R=F), dict(R=M + 4 * 500), dict(W=M), dict(W=F + 4 * 510), dict(R=F + 4 * 512 - rb),    # on inputs
             dict(R=W), dict(R=W + work - 8), dict(W=R + rb - 8), dict(W=R - work + 8),               # on each other
             dict(WF=R), dict(WM=R + rb - 4), dict(WF=W + work - 4), dict(WM=W),                      # on the masks
             dict(o=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), F=F)]                                    # too many tiles
    for kw in cases:
        assert call(**kw) == -1, kw
    for v in (np.nan, np.inf, -np.inf):
        for k in (0, 7, 11):
            A = np.eye(3, 4).reshape(12)
            A[k] = v
            kept, bad = _a(A)
            assert call(A=bad) == -1, (v, k)


def test_refine_device_refusals(hip, bufs):  # noqa: F811
    L = hip.lib()
    F, M, R, W = bufs
    res = hip.AffineRefineResult()
    fit = (C.c_double * 4)()

    def call(F=F, o=(8, 8, 8), M=M, n=(8, 8, 8), A=np.eye(3, 4), res=C.byref(res), fit=fit, W=W, WF=None, WM=None,
             **kw):
        a, ptr = _a(A) if A is not None else (None, None)
        p = C.byref(hip.affine_refine_params(**kw))
        return L.sift3d_amd_affine_ncc_refine_device(F, *o, M, *n, ptr, p, res, fit, W, None, WF, WM)
    nan, inf = float("nan"), float("inf")
    bad_A = np.eye(3, 4)
    bad_A[1, 2] = nan
    need = L.sift3d_amd_affine_ncc_refine_work_bytes(8, 8, 8, 8, 8, 8, 1)
    cases = [dict(F=None), dict(M=None), dict(A=None), dict(res=None), dict(fit=None), dict(W=None),
             dict(o=(0, 8, 8)), dict(n=(8, 8, -1)), dict(A=bad_A),
             dict(free_mask=0), dict(free_mask=0x1000), dict(levels=0), dict(levels=7),
             dict(max_evaluations=0), dict(max_evaluations=129),
             dict(lambda0=0.0), dict(lambda0=nan), dict(lambda_factor=1.0), dict(lambda_factor=inf),
             dict(lambda_min=0.0), dict(lambda_max=1e-4), dict(lambda_max=inf), dict(tol=-1.0), dict(tol=nan),
             dict(min_overlap=-0.1), dict(min_overlap=1.5), dict(min_overlap=nan),
             dict(F=F + 2), dict(M=M + 1), dict(W=W + 4), dict(WF=R + 2), dict(W=F), dict(W=M + 4 * 511),
             dict(W=F - need + 8), dict(WF=W + need - 4), dict(WM=W)]
    for kw in cases:
        assert call(**kw) == -1, kw


def test_python_value_errors():
    from sift3d_amd import api
    v = np.zeros((5, 7, 9), np.float32)
    for kw in (dict(metric="bogus"), dict(metric=None), dict(metric="ncc", free="rigid"), dict(metric="ncc", levels=0),
               dict(metric="ncc", interp="nearest"), dict(metric="ncc", bogus=1)):
        with pytest.raises(ValueError):
            api.refine_affine(v, v, **kw)
    if not api.device_available():
        with pytest.raises(RuntimeError):
            api.refine_affine(v, v, metric="ncc")


# ---- the restatement's driver: the property the metric exists for --------------------------------------------------
@pytest.fixture(scope="module")
def driven():
    """{(gain, offset, free): the restatement driver's result} on the mapped pairs"""
    out = {}
    for gain, offset in MAPS:
        fixed, moving, T = mapped_case(gain, offset)
        for free in (0x888, 0xFFF):
            out[gain, offset, free] = an.refine(fixed, moving, free_mask=free)
    return out


@pytest.mark.parametrize("free", [0x888, 0xFFF])
@pytest.mark.parametrize("gain,offset", MAPS)
def test_driver_finds_the_map_under_any_gain_and_offset(driven, gain, offset, free):
    """Measured on the restatement: converged in 5 - 6 evaluations, corner error <= 2.4e-6 voxels, alpha = 1 / gain and
    beta = -offset / gain to four digits."""
    fixed, moving, T = mapped_case(gain, offset)
    r = driven[gain, offset, free]
    err = ar.corner_distance(r.A, T, fixed.shape)
    print("gain %g offset %g free %03x: corner error %.3g after %d evaluations, stop %s; alpha %.6g beta %.6g ncc %.9f"
          % (gain, offset, free, err, r.evaluations, r.stop, r.fit.alpha, r.fit.beta, r.fit.ncc))
    assert r.stop == "converged" and r.evaluations <= 10
    assert err <= 10 * TOL
    assert abs(r.fit.alpha * gain - 1) <= 1e-3 and abs(r.fit.beta + offset / gain) <= 1e-2
    acc = r.cost[r.accepted]
    assert np.all(np.diff(acc) < 0)
    if free == 0x888:
        np.testing.assert_array_equal(r.A[:, :3], np.eye(3))


@pytest.mark.parametrize("free", [0x888, 0xFFF])
def test_driver_final_maps_agree_across_intensity_maps(driven, free):
    fixed = mapped_case()[0]
    maps = [driven[g, o, free].A for g, o in MAPS]
    for k in (1, 2):
        assert ar.corner_distance(maps[0], maps[k], fixed.shape) <= 10 * TOL


@pytest.mark.parametrize("gain,offset", MAPS[1:])
def test_msd_driver_misses_the_mapped_pairs(gain, offset):
    """The gap on the MSD path: on the two mapped pairs the MSD restatement driver ends more than a voxel from T
    (measured 2.4 - 25 voxels; it stops on lambda or on evaluations, or converges at a wrong place)."""
    fixed, moving, T = mapped_case(gain, offset)
    for free in (0x888, 0xFFF):
        r = ar.refine(fixed, moving, free_mask=free)
        err = ar.corner_distance(r.A, T, fixed.shape)
        print("gain %g offset %g free %03x: MSD driver ends %.3g voxels from T (%s)" % (gain, offset, free, err, r.stop))
        assert err > 1.0
