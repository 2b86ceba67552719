"""CPU (not gpu): the mask contract (include/sift3d_amd.h, "Masks") without a device.  The mask restatement
(tests/mask_restatement.py) against the unmasked restatements and against the rule's edge cases, the level rule, the
ValueErrors of the three api functions, the refusals of the masked C entries (which check their arguments before any
device call) and their work-buffer sizes, and the cases that tests/test_masks.py runs on the device."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import affine_refine_restatement as ar
from tests import ffd_restatement as fr
from tests import mask_restatement as mr
from tests import similarity_restatement as sr
from tests.multires_restatement import ref_restrict
from tests.test_warp import about_center, ref_warp, rot

F32 = np.float32
FSHAPE, MSHAPE = (6, 9, 70), (5, 11, 37)                     # (z, y, x): the device tests' default pair
RANGE = (-1.0, 1.5)
EDGE_VALUES = [(np.nextafter(F32(0.5), F32(0)), False), (0.5, True), (np.nan, False), (-1.0, False), (2.0, True),
               (np.inf, True), (0.0, False), (1.0, True), (-np.inf, False)]


def volumes(fshape=FSHAPE, mshape=MSHAPE, seed=1):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 1, fshape).astype(F32), rng.normal(0, 1, mshape).astype(F32)


def integer_volumes(fshape=FSHAPE, mshape=MSHAPE, seed=2, amp=30):
    rng = np.random.default_rng(seed)
    return rng.integers(-amp, amp, fshape).astype(F32), rng.integers(-amp, amp, mshape).astype(F32)


def masks(fshape=FSHAPE, mshape=MSHAPE, seed=3):
    """(W_F random binary, about 60 % in; W_M a box with random holes), float32"""
    rng = np.random.default_rng(seed)
    WF = (rng.random(fshape) < 0.6).astype(F32)
    WM = np.zeros(mshape, F32)
    box = tuple(slice(min(1, n - 1) if n > 2 else 0, n - 1 if n > 2 else n) for n in mshape)
    WM[box] = 1.0
    WM[rng.random(mshape) < 0.15] = 0.0
    return WF, WM


def rotated(fshape=FSHAPE, mshape=MSHAPE):
    """a pull map that samples part of the fixed grid outside the moving one"""
    return about_center(rot((1, 2, 3), 25.0) * 0.55, mshape, fshape, shift=(0.3, -0.2, 0.1))


def field_of(A, fshape, seed=4, noise=0.3):
    from tests.field_restatement import ref_affine_field
    rng = np.random.default_rng(seed)
    return (ref_affine_field(A, fshape) + rng.normal(0, noise, (3,) + tuple(fshape))).astype(F32)


# ---- the restatement against the unmasked ones -----------------------------------------------------------------------
@pytest.mark.parametrize("ones", [False, True])
def test_no_mask_and_all_ones_equal_the_unmasked_restatements(ones):
    F, M = volumes()
    A = rotated()
    WF, WM = (np.ones(FSHAPE, F32), np.ones(MSHAPE, F32)) if ones else (None, None)
    for T in (A, field_of(A, FSHAPE)):
        for interp in ("linear", "nearest"):
            h0, s0 = sr.joint(F, M, T, 7, RANGE, RANGE, interp)
            h1, s1 = mr.joint(F, M, T, 7, RANGE, RANGE, interp, WF, WM)
            assert np.array_equal(h0, h1) and s0.count == s1.count
            assert np.array_equal(s0.sums, s1.sums) and np.array_equal(s0.terms, s1.terms)
            assert 0 < s0.count < F.size
    n0, n1 = ar.normal_equations(F, M, A), mr.normal_equations(F, M, A, WF, WM)
    assert n0.n == n1.n and n0.see == n1.see and np.array_equal(n0.b, n1.b) and np.array_equal(n0.H, n1.H)
    assert np.array_equal(n0.H_terms, n1.H_terms)
    shape, spacing = (5, 9, 17), (4, 3, 2)
    F2, M2 = volumes(shape, (6, 11, 16), 5)
    c = np.random.default_rng(6).uniform(-1.5, 1.5, fr.lattice_shape(shape, spacing)).astype(F32)
    W2 = (np.ones(shape, F32), np.ones((6, 11, 16), F32)) if ones else (None, None)
    r0, u0 = fr.evaluate(F2, M2, c, spacing, None)
    r1, u1, force = mr.evaluate(F2, M2, c, spacing, None, *W2)
    assert r0.n == r1.n and r0.see == r1.see and np.array_equal(r0.Gc, r1.Gc) and np.array_equal(u0, u1)
    assert np.array_equal(r0.Gc_terms, r1.Gc_terms) and force.shape == (3,) + shape


def test_masks_only_remove_voxels():
    F, M = volumes()
    A = rotated()
    WF, WM = masks()
    _, both = mr.joint(F, M, A, 7, RANGE, RANGE, "linear", WF, WM)
    _, wf = mr.joint(F, M, A, 7, RANGE, RANGE, "linear", WF, None)
    _, wm = mr.joint(F, M, A, 7, RANGE, RANGE, "linear", None, WM)
    _, none = mr.joint(F, M, A, 7, RANGE, RANGE, "linear")
    assert 0 < both.count < min(wf.count, wm.count) and max(wf.count, wm.count) < none.count
    q = mr.coords(A, FSHAPE)
    ins = mr.counted(q, MSHAPE)
    assert wf.count == int((ins & (WF >= 0.5)).sum())


# ---- the rule's edges ------------------------------------------------------------------------------------------------
def test_threshold_edge_values():
    assert float(EDGE_VALUES[0][0]) < 0.5 and F32(EDGE_VALUES[0][0]) == np.nextafter(F32(0.5), F32(0))
    for v, want in EDGE_VALUES:
        assert bool(mr.mask_in(np.array([v], F32))[0]) == want, v
    F, M = volumes((2, 3, len(EDGE_VALUES)), (2, 3, len(EDGE_VALUES)))
    W = np.tile(np.array([v for v, _ in EDGE_VALUES], F32), (2, 3, 1))
    n_in = sum(w for _, w in EDGE_VALUES) * 6
    for kw in (dict(WF=W), dict(WM=W)):
        _, st = mr.joint(F, M, None, 7, RANGE, RANGE, "linear", **kw)
        assert st.count == n_in
        assert mr.normal_equations(F, M, np.eye(3, 4), **kw).n == n_in


def half_shift_case():
    """fixed 3 x 4 x 8, moving one voxel longer along x, q = p + (0.5, 0, 0); W_M is in at even x only.  floor(q + 0.5)
    = x + 1: the upper neighbour, so the fixed voxels counted are those with odd x"""
    F, M = volumes((3, 4, 8), (3, 4, 9), 7)
    A = np.eye(3, 4)
    A[0, 3] = 0.5
    WM = np.zeros((3, 4, 9), F32)
    WM[:, :, 0::2] = 1.0
    want = np.zeros((3, 4, 8), bool)
    want[:, :, 1::2] = True
    return F, M, A, WM, want


def test_nearest_rule_at_half_integer_q_reads_the_upper_neighbour():
    F, M, A, WM, want = half_shift_case()
    got = mr.counted(mr.coords(A, F.shape), M.shape, None, WM)
    assert np.array_equal(got, want)
    for interp in ("linear", "nearest"):
        _, st = mr.joint(F, M, A, 7, RANGE, RANGE, interp, None, WM)
        assert st.count == int(want.sum())
    A[0, 3] = 0.25                                                   # below the half: the lower neighbour
    got = mr.counted(mr.coords(A, F.shape), M.shape, None, WM)
    assert np.array_equal(got, ~want)


def test_fully_masked_gives_zero_and_lm_step_refuses(hip):
    F, M = volumes()
    A = rotated()
    for kw in (dict(WF=np.zeros(FSHAPE, F32)), dict(WM=np.full(MSHAPE, 0.25, F32))):
        hist, st = mr.joint(F, M, A, 7, RANGE, RANGE, "linear", **kw)
        assert st.count == 0 and not hist.any() and not st.sums.any()
        rec = mr.normal_equations(F, M, A, **kw)
        assert rec.n == 0 and rec.see == 0.0 and not rec.b.any() and not rec.H.any()
        assert ar.lm_step(rec.n, rec.b, rec.H) is None
        assert hip.affine_lm_step(rec.n, rec.see, rec.b, rec.H, 0xFFF, 1e-3) is None
    shape, spacing = (5, 9, 17), (4, 3, 2)
    F2, M2 = volumes(shape, shape, 5)
    rec, _, force = mr.evaluate(F2, M2, np.zeros(fr.lattice_shape(shape, spacing), F32), spacing, None,
                                np.zeros(shape, F32), None)
    assert rec.n == 0 and not force.any() and not rec.Gc.any()


def test_level_rule_on_an_interior_box():
    """restrict2 of the float mask, thresholded at the level: an interior box that starts and ends on even voxels keeps
    its interior (all taps 1), loses nothing outside (all taps 0), and its faces decide by the restricted value - never
    by a thresholded copy of the level above"""
    W = np.zeros((16, 20, 24), F32)
    W[4:12, 6:14, 8:20] = 1.0
    W1 = ref_restrict(W)
    assert W1.shape == (8, 10, 12) and W1.dtype == F32
    inn = mr.mask_in(W1)
    assert inn[3:5, 4:6, 5:9].all()                                  # fine 6 .. 10, 8 .. 12, 10 .. 18: interior
    assert not inn[:1].any() and not inn[:, :2].any() and not inn[:, :, :3].any()
    assert 0.0 < W1[2, 4, 5] < 1.0                                   # a face voxel carries a fraction
    pyr = mr.pyramid(W, 3)
    assert np.array_equal(pyr[1], W1) and np.array_equal(pyr[2], ref_restrict(W1))
    soft = np.full((8, 8, 8), 0.75, F32)                             # float masks pass as they are
    assert mr.mask_in(ref_restrict(soft)).all()
    assert not np.array_equal(ref_restrict(ref_restrict(W)), ref_restrict(mr.mask_in(W1).astype(F32)))


# ---- the library without a device --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


def test_python_value_errors():
    from sift3d_amd import api
    v, m = np.zeros((5, 7, 9), F32), np.zeros((4, 7, 8), F32)
    calls = (lambda **kw: api.similarity(v, m, np.eye(3, 4), **kw), lambda **kw: api.refine_affine(m, v, **kw),
             lambda **kw: api.refine_ffd(m, v, **kw))
    for call in calls:
        for kw in (dict(mask_fixed=np.ones((5, 7, 8))), dict(mask_moving=np.ones((5, 7, 9))),
                   dict(mask_fixed=np.ones((7, 9), bool)), dict(mask_moving=np.ones((1, 4, 7, 8), np.uint8)),
                   dict(mask_fixed=np.ones((5, 7, 9), complex)), dict(mask_fixed=api.Image.from_array(m))):
            with pytest.raises(ValueError):
                call(**kw)
    import torch
    for call in calls:
        with pytest.raises(ValueError):
            call(mask_fixed=torch.ones((5, 7, 9)))                   # a tensor that is not on a device
    if not api.device_available():
        for call in calls:
            with pytest.raises(RuntimeError):                        # good masks: only the device is missing
                call(mask_fixed=np.ones((5, 7, 9), bool), mask_moving=np.ones((4, 7, 8)))


@pytest.fixture(scope="module")
def bufs():
    """made-up addresses without a device; real allocations covering every range named below with one"""
    from sift3d_amd import api, hip
    if api.device_available():
        b = [hip.lib().sift3d_hip_malloc(1 << 22) for _ in range(9)]
        assert all(b)
        yield b
        for p in b:
            hip.lib().sift3d_hip_free(p)
    else:
        yield [0x10000000 * (k + 1) for k in range(9)]


def _a(A):
    a = np.ascontiguousarray(A, np.float64).reshape(12)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def refused(L, rc, before):
    """-1, and from the argument checks: no runtime call has failed since `before` (without a device one would, and
    would return -1 too; a refusal leaves the runtime's error text alone)"""
    return rc == -1 and L.sift3d_hip_last_error() == before


def test_symbols_and_work_bytes(hip):
    from sift3d_amd import _native
    L = _native.load()
    for name in ("sift3d_hip_similarity_affine_masked", "sift3d_hip_similarity_field_masked",
                 "sift3d_hip_affine_normal_eqs_masked", "sift3d_amd_affine_refine_masked_work_bytes",
                 "sift3d_amd_affine_refine_masked_device", "sift3d_hip_ffd_evaluate_masked",
                 "sift3d_amd_ffd_refine_masked_work_bytes", "sift3d_amd_ffd_refine_masked_device"):
        assert hasattr(L, name), name
    L = hip.lib()
    R, RM = L.sift3d_amd_affine_refine_work_bytes, L.sift3d_amd_affine_refine_masked_work_bytes
    assert RM(8, 8, 8, 6, 6, 6, 1) == R(8, 8, 8, 6, 6, 6, 1)
    assert RM(8, 8, 8, 6, 6, 6, 2) == R(8, 8, 8, 6, 6, 6, 2) + 4 * 64 + 4 * 28
    for lv in range(1, 7):
        assert RM(48, 40, 32, 37, 11, 5, lv) >= R(48, 40, 32, 37, 11, 5, lv) > 0
    assert RM(8, 8, 8, 8, 8, 8, 0) == 0 and RM(8, 8, 8, 8, 8, 8, 7) == 0 and RM(8, 0, 8, 8, 8, 8, 1) == 0
    assert RM(8, 8, 8, 8, 8, -1, 1) == 0
    W, WM = L.sift3d_amd_ffd_refine_work_bytes, L.sift3d_amd_ffd_refine_masked_work_bytes
    assert WM(8, 8, 8, 8, 8, 8, 8, 8, 8, 1) == W(8, 8, 8, 8, 8, 8, 8, 8, 8, 1)
    assert WM(8, 8, 8, 8, 8, 8, 8, 8, 8, 2) == W(8, 8, 8, 8, 8, 8, 8, 8, 8, 2) + 2 * 4 * 64
    for lv in range(1, 7):
        assert WM(40, 36, 32, 37, 11, 5, 8, 8, 8, lv) >= W(40, 36, 32, 37, 11, 5, 8, 8, 8, lv) > 0
    assert WM(8, 8, 8, 8, 8, 8, 8, 8, 8, 0) == 0 and WM(8, 8, 8, 8, 8, 8, 8, 8, 8, 7) == 0
    assert WM(8, 8, 8, 8, 0, 8, 8, 8, 8, 1) == 0 and WM(8, 8, 8, 8, 8, 8, 8, 300, 8, 1) == 0


def test_similarity_and_normal_equations_refusals(hip, bufs):
    L = hip.lib()
    before = L.sift3d_hip_last_error()
    F, M, H, S, W, WF, WM, U_ = bufs[:8]
    keep, ident = _a(np.eye(3, 4))
    work = L.sift3d_amd_similarity_work_bytes(8, 8, 8, 16)

    def sim(F=F, o=(8, 8, 8), M=M, n=(8, 8, 8), A=ident, U=None, H=H, S=S, W=W, WF=WF, WM=WM, bins=16):
        tail = (1, bins, -1.0, 1.0, -1.0, 1.0, H, S, W, None, WF, WM)
        if U is not None:
            return L.sift3d_hip_similarity_field_masked(F, *o, M, *n, U, *tail)
        return L.sift3d_hip_similarity_affine_masked(F, *o, M, *n, A, *tail)
    cases = [dict(F=None), dict(M=None), dict(A=None), dict(H=None), dict(S=None), dict(W=None), dict(o=(0, 8, 8)),
             dict(n=(8, 8, -1)), dict(bins=1), dict(bins=129),
             dict(WF=WF + 2), dict(WM=WM + 1), dict(WF=WF + 3, WM=None), dict(WM=WM + 2, WF=None),      # misaligned
             dict(WF=H), dict(WF=H - 4 * 511), dict(WF=H + 8 * 255), dict(WM=S), dict(WM=S + 52), dict(WM=W),
             dict(WF=W + work - 4), dict(WF=S - 4 * 511, WM=None), dict(WM=H, WF=None)]                 # on outputs
    for kw in cases:
        assert refused(L, sim(**kw), before), kw
        if "A" not in kw:
            assert refused(L, sim(U=U_, **kw), before), ("field", kw)
    assert L.sift3d_hip_similarity_field_masked(F, 8, 8, 8, M, 8, 8, 8, None, 1, 16, -1.0, 1.0, -1.0, 1.0, H, S, W, None,
                                                WF, WM) == -1

    R = S
    nwork = L.sift3d_amd_affine_normal_work_bytes(8, 8, 8)

    def neq(F=F, o=(8, 8, 8), M=M, n=(8, 8, 8), A=ident, R=R, W=W, WF=WF, WM=WM):
        return L.sift3d_hip_affine_normal_eqs_masked(F, *o, M, *n, A, R, W, None, WF, WM)
    cases = [dict(F=None), dict(M=None), dict(A=None), dict(R=None), dict(W=None), dict(o=(8, 0, 8)), dict(n=(-1, 8, 8)),
             dict(F=F + 2), dict(R=R + 4), dict(WF=WF + 1), dict(WM=WM + 2), dict(WM=WM + 3, WF=None),
             dict(WF=R), dict(WF=R + 1260), dict(WF=R - 4 * 511), dict(WM=R), dict(WM=W), dict(WM=W + nwork - 4),
             dict(WF=W - 4 * 511, WM=None), dict(WM=R + 8, WF=None),
             dict(o=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1))]
    for kw in cases:
        assert refused(L, neq(**kw), before), kw
    bad = np.eye(3, 4).reshape(12)
    bad[5] = np.nan
    assert neq(A=_a(bad)[1]) == -1


def test_driver_and_evaluate_refusals(hip, bufs):
    L = hip.lib()
    before = L.sift3d_hip_last_error()
    F, M, c, U_, R, G, W, WF, WM = bufs
    res = hip.AffineRefineResult()
    keep, ident = _a(np.eye(3, 4))

    def aff(F=F, o=(8, 8, 8), M=M, n=(8, 8, 8), A=ident, res=C.byref(res), W=W, WF=WF, WM=WM, **kw):
        return L.sift3d_amd_affine_refine_masked_device(F, *o, M, *n, A, C.byref(hip.affine_refine_params(**kw)), res,
                                                        W, None, WF, WM)
    wb = L.sift3d_amd_affine_refine_masked_work_bytes(8, 8, 8, 8, 8, 8, 2)
    cases = [dict(F=None), dict(M=None), dict(A=None), dict(res=None), dict(W=None), dict(o=(0, 8, 8)), dict(levels=0),
             dict(levels=7), dict(free_mask=0), dict(max_evaluations=0), dict(lambda0=-1.0), dict(min_overlap=2.0),
             dict(WF=WF + 2), dict(WM=WM + 1), dict(WF=WF + 1, WM=None), dict(WM=WM + 3, WF=None),
             dict(WF=W), dict(WM=W), dict(WF=W + wb - 4, levels=2), dict(WM=W - 4 * 511), dict(WM=W + wb - 4, WF=None,
                                                                                              levels=2)]
    for kw in cases:
        assert refused(L, aff(**kw), before), kw

    def ev(F=F, o=(8, 8, 8), M=M, n=(8, 8, 8), c=c, g=(4, 4, 4), d=(8, 8, 8), lam=0.0, U=U_, R=R, G=G, W=W, WF=WF, WM=WM):
        return L.sift3d_hip_ffd_evaluate_masked(F, *o, M, *n, c, *g, *d, None, lam, U, R, G, W, None, WF, WM)
    cases = [dict(F=None), dict(M=None), dict(c=None), dict(U=None), dict(R=None), dict(G=None), dict(W=None),
             dict(o=(0, 8, 8)), dict(g=(5, 4, 4)), dict(d=(8, 300, 8)), dict(lam=-1.0),
             dict(WF=WF + 2), dict(WM=WM + 1), dict(WM=WM + 2, WF=None),
             dict(WF=U_), dict(WF=U_ + 4 * 3 * 511), dict(WM=R), dict(WM=G), dict(WM=G + 4 * 191), dict(WF=W),
             dict(WM=W + 64, WF=None), dict(WF=R + 32, WM=None)]
    for kw in cases:
        assert refused(L, ev(**kw), before), kw
    fres = hip.FFDRefineResult()

    def ffd(F=F, o=(8, 8, 8), M=M, n=(8, 8, 8), res=C.byref(fres), c=c, U=U_, W=W, WF=WF, WM=WM, **kw):
        return L.sift3d_amd_ffd_refine_masked_device(F, *o, M, *n, None, C.byref(hip.ffd_refine_params(**kw)), res, c, U,
                                                     W, None, WF, WM)
    fb = L.sift3d_amd_ffd_refine_masked_work_bytes(8, 8, 8, 8, 8, 8, 8, 8, 8, 2)
    cases = [dict(F=None), dict(M=None), dict(res=None), dict(c=None), dict(U=None), dict(W=None), dict(n=(8, 8, 0)),
             dict(levels=0), dict(levels=7), dict(bending=-1.0), dict(tol=0.0),
             dict(WF=WF + 2), dict(WM=WM + 1), dict(WM=WM + 2, WF=None),
             dict(WF=c), dict(WM=c + 4 * 191), dict(WF=U_), dict(WM=U_ + 4 * 3 * 511), dict(WF=W),
             dict(WM=W + fb - 4, levels=2), dict(WF=W - 4 * 511, WM=None)]
    for kw in cases:
        assert refused(L, ffd(**kw), before), kw


# ---- the drivers' cases (the device test runs the same) --------------------------------------------------------------
AFFINE_CASE = dict(levels=3)


@functools.lru_cache(maxsize=None)
def affine_case():
    """(fixed, moving, T, W_F): 48 x 40 x 32 (x, y, z) crops of a 64^3 synth_survey volume and of the same volume pulled
    through the inverse of the translation T (by a fraction of a voxel, so that the interpolation leaves every driver a
    small error of its own), a bright block added to the fixed volume only, and the fixed mask that excludes the block
    with a margin of 4 voxels (2 at level 1, 1 at level 2: what the restriction smears)"""
    from sift3d_amd import api
    S = np.ascontiguousarray(api.synth_survey(64), F32)
    T = np.eye(3, 4)
    T[:, 3] = (2.5, -1.25, 0.75)
    Tinv = np.eye(3, 4)
    Tinv[:, 3] = -T[:, 3]
    pulled = ref_warp(S, Tinv, S.shape, "linear", 0.0)[0].astype(F32)
    crop = (slice(16, 48), slice(12, 52), slice(8, 56))
    F, M = np.ascontiguousarray(S[crop]), np.ascontiguousarray(pulled[crop])
    block = (slice(6, 18), slice(8, 22), slice(24, 42))
    F[block] += 3.0 * float(np.abs(S).max())
    WF = np.ones(F.shape, F32)
    WF[2:22, 4:26, 20:46] = 0.0
    return F, M, T, WF


@functools.lru_cache(maxsize=None)
def affine_case_restatement():
    """(masked restatement driver's result, its corner error, the unmasked restatement driver's corner error)"""
    F, M, T, WF = affine_case()
    masked = mr.refine_affine(F, M, None, WF, None, **AFFINE_CASE)
    plain = ar.refine(F, M, **AFFINE_CASE)
    return masked, ar.corner_distance(masked.A, T, F.shape), ar.corner_distance(plain.A, T, F.shape)


def test_affine_case_shows_what_the_mask_is_for():
    masked, err, err_plain = affine_case_restatement()
    print("masked restatement driver: corner error %.4g after %d evaluations, stop %s; unmasked: %.4g"
          % (err, masked.evaluations, masked.stop, err_plain))
    assert err_plain > 2 * err                                       # measured: 0.1112 masked, 2.894 unmasked
    assert masked.levels.tolist() == sorted(masked.levels.tolist(), reverse=True)


FFD_CASE = dict(spacing=8, levels=2, bending=0.005, max_evaluations=20)


@functools.lru_cache(maxsize=None)
def ffd_case():
    """(fixed, moving, truth, W_F, W_M): 40 x 36 x 32 (x, y, z) crops of tests/test_ffd_host.driver_pair's volumes and
    field; the fixed mask leaves out a block, the moving mask a slab at the low x face"""
    from tests.test_ffd_host import driver_pair
    F, M, u = driver_pair()
    crop = (slice(8, 40), slice(6, 42), slice(4, 44))
    F, M, u = np.ascontiguousarray(F[crop]), np.ascontiguousarray(M[crop]), np.ascontiguousarray(u[(slice(None),) + crop])
    WF = np.ones(F.shape, F32)
    WF[20:28, 4:14, 24:36] = 0.0
    WM = np.ones(M.shape, F32)
    WM[:, :, :3] = 0.0
    return F, M, u, WF, WM


@functools.lru_cache(maxsize=None)
def ffd_case_restatement():
    from tests.test_ffd_host import summarize
    F, M, u, WF, WM = ffd_case()
    r = mr.refine_ffd(F, M, None, WF, WM, FFD_CASE["spacing"], FFD_CASE["levels"], FFD_CASE["bending"],
                      FFD_CASE["max_evaluations"])
    return r, summarize(r.trail, r.field, u)


def test_ffd_case_restatement_driver():
    r, (ratio, rms) = ffd_case_restatement()
    print("masked restatement FFD driver: stop %s, %d evaluations, MSD ratio %.4g, RMS field error %.4g voxels"
          % (r.stop, len(r.trail), ratio, rms))
    F, M, u, WF, WM = ffd_case()
    assert r.stop in fr.STOPS and ratio < 1.0
    assert all(0 < e[3] < F.size for e in r.trail)                   # the masks remove voxels on every level
