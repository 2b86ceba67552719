"""Masks on the device (include/sift3d_amd.h, "Masks") against the mask restatement (tests/mask_restatement.py): the
histogram, the counts, the FFD field and the force bit for bit; the sums to the bounds of tests/test_similarity.py,
tests/test_affine_refine.py and tests/test_ffd.py, and exactly on integer content; NULL and all-ones masks byte for byte
the unmasked entries; the drivers on the cases of tests/test_masks_host.py."""
import numpy as np
import pytest

from tests import affine_refine_restatement as ar
from tests import ffd_restatement as fr
from tests import mask_restatement as mr
from tests.demons_restatement import gamma
from tests.test_affine_refine_host import TOL
from tests.test_masks_host import (AFFINE_CASE, EDGE_VALUES, FFD_CASE, FSHAPE, MSHAPE, RANGE, affine_case,
                                   affine_case_restatement, ffd_case, ffd_case_restatement, field_of, half_shift_case,
                                   integer_volumes, masks, rotated, volumes)

pytestmark = pytest.mark.gpu
F32 = np.float32
COMBOS = {"W_F": (True, False), "W_M": (False, True), "both": (True, True)}


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pick(which, WF, WM):
    f, m = COMBOS[which]
    return (WF if f else None), (WM if m else None)


def sim(hip, F, M, T, bins, rf, rm, interp, WF=None, WM=None):
    Td = dev(T.astype(F32)) if isinstance(T, np.ndarray) and T.ndim == 4 else T
    hist, stats = hip.similarity(dev(F), dev(M), Td, bins, rf, rm, interp, mask_fixed=dev(WF), mask_moving=dev(WM))
    count, sums = hip.similarity_stats(stats)
    return hist.cpu().numpy(), count, sums, stats.cpu().numpy()


def ffd_eval(hip, F, M, c, spacing, A, bending, WF=None, WM=None, null_masked_entry=False):
    """hip.ffd_evaluate on a work buffer of the test's own, and the force E G_d cut out of it: (record, grad, field,
    force float64 [3, oz, oy, ox]), numpy.  The work buffer holds the weight tables padded to 16 bytes, the partial
    slots, the force, then two adjoint arrays and the second derivatives (sift3d_ffd.hip, sift3d_ffd_evaluate_launch);
    the slots' size is what sift3d_amd_ffd_evaluate_work_bytes leaves after the other parts.  null_masked_entry: call
    sift3d_hip_ffd_evaluate_masked itself with both masks NULL (hip.ffd_evaluate sends None, None to the unmasked one)."""
    import torch
    L = hip.lib()
    oz, oy, ox = F.shape
    nz, ny, nx = M.shape
    dx, dy, dz = spacing
    _, gz, gy, gx = c.shape
    total = L.sift3d_amd_ffd_evaluate_work_bytes(ox, oy, oz, dx, dy, dz)
    vox = oz * oy * ox
    weights = ((dx + dy + dz) * 16 + 15) // 16 * 16
    rest = 8 * (3 * vox + 3 * ox * oy * gz + 3 * ox * gy * gz + 18 * (gx - 2) * (gy - 2) * (gz - 2))
    off = total - rest                                                   # the weights and the partial slots
    assert off > weights and (off - weights) % 16 == 0
    work = torch.zeros(total, dtype=torch.uint8, device="cuda")
    Fd, Md, cd = dev(F), dev(M), dev(c)
    if null_masked_entry:
        rec = torch.zeros(L.sift3d_amd_ffd_record_bytes(gx, gy, gz) // 8, dtype=torch.int64, device="cuda")
        grad = torch.empty_like(cd)
        fld = torch.empty((3, oz, oy, ox), dtype=torch.float32, device="cuda")
        a = np.ascontiguousarray(A, np.float64).reshape(12)
        rc = L.sift3d_hip_ffd_evaluate_masked(Fd.data_ptr(), ox, oy, oz, Md.data_ptr(), nx, ny, nz, cd.data_ptr(), gx,
                                              gy, gz, dx, dy, dz, hip._dptr(a), float(bending), fld.data_ptr(),
                                              rec.data_ptr(), grad.data_ptr(), work.data_ptr(), hip.current_stream(),
                                              None, None)
        assert rc == 0
    else:
        rec, grad, fld = hip.ffd_evaluate(Fd, Md, cd, spacing, A, bending, work, mask_fixed=dev(WF), mask_moving=dev(WM))
    force = work[off:off + 24 * vox].clone().view(torch.float64).reshape(3, oz, oy, ox)
    return rec.cpu().numpy(), grad.cpu().numpy(), fld.cpu().numpy(), force.cpu().numpy()


# ---- 1. similarity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(COMBOS))
@pytest.mark.parametrize("bins", [7, 64])
def test_similarity_against_the_restatement(hip, which, bins):
    F, M = volumes()
    Fi, Mi = integer_volumes()
    WF, WM = pick(which, *masks())
    A = rotated()
    shift = np.eye(3, 4)
    shift[:, 3] = [3, -1, 1]
    for T, Ti in ((A, shift), (field_of(A, FSHAPE), field_of(shift, FSHAPE, noise=0.0))):
        for interp in ("linear", "nearest"):
            what = "%s B=%d %s %s" % (which, bins, "affine" if T.ndim == 2 else "field", interp)
            hist, count, sums, _ = sim(hip, F, M, T, bins, RANGE, RANGE, interp, WF, WM)
            want_hist, want = mr.joint(F, M, T, bins, RANGE, RANGE, interp, WF, WM)
            np.testing.assert_array_equal(hist, want_hist.astype(np.int64), err_msg=what)
            assert count == want.count == int(want_hist.sum()) and 0 < count < F.size, (what, count, want.count)
            for k, name in enumerate(("f", "m", "ff", "mm", "fm", "dd")):
                bound = gamma(max(count, 1)) * want.terms[k]
                assert abs(sums[k] - want.sums[k]) <= bound, (what, name, sums[k], want.sums[k], bound)
            hist, count, sums, _ = sim(hip, Fi, Mi, Ti, bins, (-30.0, 30.0), (-30.0, 30.0), interp, WF, WM)
            want_hist, want = mr.joint(Fi, Mi, Ti, bins, (-30.0, 30.0), (-30.0, 30.0), interp, WF, WM)
            np.testing.assert_array_equal(hist, want_hist.astype(np.int64), err_msg=what)
            assert count == want.count > 0 and np.array_equal(sums, want.sums), (what, sums, want.sums)


# ---- 2. byte identity ------------------------------------------------------------------------------------------------
def _identity(hip, F, M, T, bins, interp):
    import torch
    h0, _, _, s0 = sim(hip, F, M, T, bins, RANGE, RANGE, interp)
    ones = (np.ones(F.shape, F32), np.ones(M.shape, F32))
    Td = dev(T.astype(F32)) if T.ndim == 4 else T
    L, st = hip.lib(), hip.current_stream()
    for WF, WM in (ones, (None, None)):
        if WF is not None:
            h1, _, _, s1 = sim(hip, F, M, T, bins, RANGE, RANGE, interp, WF, WM)
        else:                                                            # the masked entry itself with NULL masks
            Fd, Md = dev(F), dev(M)
            hist = torch.empty((bins, bins), dtype=torch.int64, device="cuda")
            stats = torch.empty(7, dtype=torch.int64, device="cuda")
            work = torch.empty(L.sift3d_amd_similarity_work_bytes(8, 8, 8, bins), dtype=torch.uint8, device="cuda")
            oz, oy, ox = F.shape
            nz, ny, nx = M.shape
            tail = (hip._interp(interp), bins, RANGE[0], RANGE[1], RANGE[0], RANGE[1], hist.data_ptr(), stats.data_ptr(),
                    work.data_ptr(), st, None, None)
            if T.ndim == 4:
                rc = L.sift3d_hip_similarity_field_masked(Fd.data_ptr(), ox, oy, oz, Md.data_ptr(), nx, ny, nz,
                                                          Td.data_ptr(), *tail)
            else:
                a = np.ascontiguousarray(T, np.float64).reshape(12)
                rc = L.sift3d_hip_similarity_affine_masked(Fd.data_ptr(), ox, oy, oz, Md.data_ptr(), nx, ny, nz,
                                                           hip._dptr(a), *tail)
            assert rc == 0
            h1, s1 = hist.cpu().numpy(), stats.cpu().numpy()
        assert np.array_equal(h0, h1) and np.array_equal(s0, s1), (interp, WF is None)


def test_null_and_all_ones_masks_are_the_unmasked_bytes_small(hip):
    F, M = volumes()
    A = rotated()
    for T in (A, field_of(A, FSHAPE)):
        for interp in ("linear", "nearest"):
            _identity(hip, F, M, T, 64, interp)
    import torch
    L = hip.lib()
    Fd, Md = dev(F), dev(M)
    n0 = hip.affine_normal_equations(Fd, Md, A, raw=True).cpu().numpy()
    n1 = hip.affine_normal_equations(Fd, Md, A, raw=True, mask_fixed=dev(np.ones(FSHAPE, F32)),
                                     mask_moving=dev(np.ones(MSHAPE, F32))).cpu().numpy()
    rec = torch.full((hip.AFFINE_NORMAL_BYTES // 8,), 7, dtype=torch.int64, device="cuda")
    work = torch.empty(hip.affine_normal_work_bytes(), dtype=torch.uint8, device="cuda")
    a = np.ascontiguousarray(A, np.float64).reshape(12)
    (oz, oy, ox), (nz, ny, nx) = FSHAPE, MSHAPE
    assert L.sift3d_hip_affine_normal_eqs_masked(Fd.data_ptr(), ox, oy, oz, Md.data_ptr(), nx, ny, nz, hip._dptr(a),
                                                 rec.data_ptr(), work.data_ptr(), hip.current_stream(), None, None) == 0
    assert np.array_equal(n0, n1) and np.array_equal(n0, rec.cpu().numpy()) and n0[0] > 0
    shape, spacing, mshape = (5, 9, 70), (7, 3, 2), (6, 11, 37)
    F2, M2 = volumes(shape, mshape, 5)
    c = np.random.default_rng(6).uniform(-1.5, 1.5, fr.lattice_shape(shape, spacing)).astype(F32)
    A2 = rotated(shape, mshape)
    plain = ffd_eval(hip, F2, M2, c, spacing, A2, 0.01)
    ones = ffd_eval(hip, F2, M2, c, spacing, A2, 0.01, np.ones(shape, F32), np.ones(mshape, F32))
    null = ffd_eval(hip, F2, M2, c, spacing, A2, 0.01, null_masked_entry=True)
    for other in (ones, null):
        for a, b in zip(plain, other):                                   # record, grad, field, force
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert plain[0][0] > 0 and plain[3].any()


def test_null_and_all_ones_masks_are_the_unmasked_bytes_multi_pass(hip):
    """192 x 132 x 88: 3 x 33 x 22 = 2 178 tiles, more than SIFT3D_AMD_SIMILARITY_GRID, so the tile walk takes a second
    pass"""
    shape = (88, 132, 192)
    assert 3 * 33 * 22 > hip.SIMILARITY_GRID
    F, M = volumes(shape, shape, 9)
    _identity(hip, F, M, rotated(shape, shape), 64, "linear")


# ---- 3. edge semantics -----------------------------------------------------------------------------------------------
def test_edge_semantics_on_the_device(hip):
    vals = np.array([v for v, _ in EDGE_VALUES], F32)
    shape = (2, 3, len(vals))
    F, M = volumes(shape, shape)
    W = np.tile(vals, (2, 3, 1))
    n_in = sum(w for _, w in EDGE_VALUES) * 6
    for kw in (dict(WF=W), dict(WM=W)):
        for interp in ("linear", "nearest"):
            hist, count, _, _ = sim(hip, F, M, np.eye(3, 4), 7, RANGE, RANGE, interp, **kw)
            want_hist, want = mr.joint(F, M, None, 7, RANGE, RANGE, interp, **kw)
            assert count == want.count == n_in and np.array_equal(hist, want_hist.astype(np.int64))
        n = hip.affine_normal_equations(dev(F), dev(M), np.eye(3, 4), mask_fixed=dev(kw.get("WF")),
                                        mask_moving=dev(kw.get("WM")))[0]
        assert n == n_in
    F, M, A, WM, want = half_shift_case()
    for interp in ("linear", "nearest"):
        _, count, _, _ = sim(hip, F, M, A, 7, RANGE, RANGE, interp, None, WM)
        assert count == int(want.sum())
        wh, _ = mr.joint(F, M, A, 7, RANGE, RANGE, interp, None, WM)
        assert np.array_equal(sim(hip, F, M, A, 7, RANGE, RANGE, interp, None, WM)[0], wh.astype(np.int64))
    assert hip.affine_normal_equations(dev(F), dev(M), A, mask_moving=dev(WM))[0] == int(want.sum())
    # all out
    F, M = volumes()
    A = rotated()
    for kw in (dict(WF=np.zeros(FSHAPE, F32)), dict(WM=np.full(MSHAPE, np.nan, F32))):
        hist, count, sums, raw = sim(hip, F, M, A, 7, RANGE, RANGE, "linear", **kw)
        assert count == 0 and not hist.any() and not raw.any()
        rec = hip.affine_normal_equations(dev(F), dev(M), A, raw=True, mask_fixed=dev(kw.get("WF")),
                                          mask_moving=dev(kw.get("WM")))
        assert not rec.cpu().numpy().any()
        shape, spacing = (5, 9, 70), (7, 3, 2)
        F2, M2 = volumes(shape, MSHAPE, 5)
        c = np.random.default_rng(6).uniform(-1.5, 1.5, fr.lattice_shape(shape, spacing)).astype(F32)
        W2 = (np.zeros(shape, F32), None) if "WF" in kw else (None, kw["WM"])
        r, _, _, force = ffd_eval(hip, F2, M2, c, spacing, rotated(shape, MSHAPE), 0.01, *W2)
        assert not r[:2].any() and not r[4:4 + c.size].any()             # n, S_ee and Gc: all-zero bytes
        assert not force.view(np.uint8).any()


# ---- 4. the normal equations -----------------------------------------------------------------------------------------
def check_normal(hip, F, M, A, WF, WM, what, exact=False):
    n, see, b, H = hip.affine_normal_equations(dev(F), dev(M), A, mask_fixed=dev(WF), mask_moving=dev(WM))
    want = mr.normal_equations(F, M, A, WF, WM)
    assert n == want.n, (what, n, want.n)
    assert np.array_equal(H, H.T), what
    g = 0.0 if exact else gamma(n + 8)
    assert abs(see - want.see) <= g * want.see_terms, (what, "S_ee", see, want.see)
    db, dH = np.abs(b - want.b), np.abs(H - want.H)
    assert np.all(db <= g * want.b_terms), (what, "b", db.max())
    assert np.all(dH <= g * want.H_terms), (what, "H", dH.max())
    return n


@pytest.mark.parametrize("which", list(COMBOS))
def test_normal_equations_against_the_restatement(hip, which):
    F, M = volumes()
    WF, WM = pick(which, *masks())
    n = check_normal(hip, F, M, rotated(), WF, WM, which)
    assert 0 < n < F.size
    fshape, mshape = (6, 9, 71), (5, 11, 80)                             # odd x: centred positions are integers or halves
    Fi, Mi = integer_volumes(fshape, mshape)
    WFi, WMi = pick(which, *masks(fshape, mshape))
    shift = np.eye(3, 4)
    shift[:, 3] = [3, -1, 1]
    assert check_normal(hip, Fi, Mi, shift, WFi, WMi, which + " integers", exact=True) > 0


def test_normal_equations_moving_axis_of_one(hip):
    """nx == 1: the LINEAR == 1 instantiation"""
    fshape, mshape = (6, 9, 70), (5, 11, 1)
    F, M = volumes(fshape, mshape)
    WF, WM = masks(fshape, mshape)
    A = np.array([[0.0, 0.0, 0.0, 0.0], [0.0, 1.1, 0.1, 0.3], [0.0, -0.1, 0.7, 0.2]])
    n = check_normal(hip, F, M, A, WF, WM, "nx == 1")
    assert 0 < n < F.size
    hist, count, _, _ = sim(hip, F, M, A, 7, RANGE, RANGE, "linear", WF, WM)
    assert count == n and np.array_equal(hist, mr.joint(F, M, A, 7, RANGE, RANGE, "linear", WF, WM)[0].astype(np.int64))


# ---- 5. FFD evaluate -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(COMBOS))
def test_ffd_evaluate_against_the_restatement(hip, which):
    shape, spacing, mshape = (5, 9, 70), (7, 3, 2), (6, 11, 37)
    F, M = volumes(shape, mshape, 5)
    WF, WM = pick(which, *masks(shape, mshape))
    c = np.random.default_rng(6).uniform(-1.5, 1.5, fr.lattice_shape(shape, spacing)).astype(F32)
    A = rotated(shape, mshape)
    import torch
    rec, grad, fld, force = ffd_eval(hip, F, M, c, spacing, A, 0.01, WF, WM)
    n, see, R, gmax, Gc, dR = hip.ffd_record(torch.from_numpy(rec), c.shape)
    want, u, wforce = mr.evaluate(F, M, c, spacing, A, WF, WM)
    assert np.array_equal(fld, u)
    assert n == want.n and 0 < n < F.size, (n, want.n)
    assert np.array_equal(force, wforce)                                 # products exact; 0 where uncounted
    assert abs(see - want.see) <= gamma(F.size + 8) * want.see_terms, (see, want.see)
    bound = np.array([gamma(int(k) + 8) for k in want.support.reshape(-1)]).reshape(want.support.shape) * want.Gc_terms
    assert np.all(np.abs(Gc - want.Gc) <= bound)
    g, gm = fr.gradient(want._replace(Gc=Gc), dR, 0.01)
    assert np.array_equal(grad, g) and gmax == gm


# ---- 6. the affine driver --------------------------------------------------------------------------------------------
def test_affine_driver(hip):
    from sift3d_amd import api
    F, M, T, WF = affine_case()
    assert F.shape == (32, 40, 48)
    plain = api.refine_affine(M, F, **AFFINE_CASE)
    ones = api.refine_affine(M, F, mask_fixed=np.ones(F.shape, F32), mask_moving=np.ones(M.shape, F32), **AFFINE_CASE)
    assert np.array_equal(plain.A, ones.A) and plain.evaluations == ones.evaluations and plain.stop == ones.stop
    for f in ("msd", "count", "accepted", "lambdas", "levels"):
        assert np.array_equal(getattr(plain, f), getattr(ones, f), equal_nan=f == "msd"), f
    r = api.refine_affine(M, F, mask_fixed=WF, **AFFINE_CASE)
    ref, err_ref, err_plain = affine_case_restatement()
    err, apart = ar.corner_distance(r.A, T, F.shape), ar.corner_distance(r.A, ref.A, F.shape)
    print("masked device driver: corner error %.4g (restatement %.4g, unmasked restatement %.4g), %.3g from the "
          "restatement's, %d evaluations, stop %s" % (err, err_ref, err_plain, apart, r.evaluations, r.stop))
    assert apart <= 10 * TOL
    assert err <= 2 * err_ref                                            # the restatement's: 0.1112 voxel
    assert err_plain > 2 * err_ref                                       # unmasked restatement: 2.894 voxels
    assert list(r.level_slices) == [2, 1, 0] and np.all(r.count[r.levels == 0] < int(WF.sum()) + 1)


# ---- 7. the FFD driver -----------------------------------------------------------------------------------------------
def test_ffd_driver(hip):
    from sift3d_amd import api
    from tests.test_ffd_host import summarize
    F, M, truth, WF, WM = ffd_case()
    assert F.shape == (32, 36, 40)
    kw = dict(max_evaluations=FFD_CASE["max_evaluations"])
    args = (M, F, None, FFD_CASE["spacing"], FFD_CASE["levels"], FFD_CASE["bending"])
    plain = api.refine_ffd(*args, **kw)
    ones = api.refine_ffd(*args, mask_fixed=np.ones(F.shape, F32), mask_moving=np.ones(M.shape, F32), **kw)
    assert np.array_equal(plain.lattice.cpu().numpy().view(np.uint32), ones.lattice.cpu().numpy().view(np.uint32))
    assert plain.trail == ones.trail and plain.stop == ones.stop
    r = api.refine_ffd(*args, mask_fixed=WF, mask_moving=WM, **kw)
    _, (ratio_ref, rms_ref) = ffd_case_restatement()
    trail = [tuple(e) for e in r.trail]
    ratio, rms = summarize(trail, r.field.cpu().numpy(), truth)
    print("masked device FFD driver: stop %s, %d evaluations, MSD ratio %.4g (restatement %.4g), RMS %.4g (restatement "
          "%.4g)" % (r.stop, len(trail), ratio, ratio_ref, rms, rms_ref))
    assert 1.0 / ratio >= 0.5 / ratio_ref
    assert rms <= 1.5 * rms_ref
    assert all(0 < e[3] < F.size for e in trail)


# ---- 8. the api layer ------------------------------------------------------------------------------------------------
def test_api_mask_kinds_agree_and_none_is_as_before(hip):
    import torch
    from sift3d_amd import api
    F, M = volumes()
    A = rotated()
    WF, WM = masks()
    kinds = [(WF, WM), (WF.astype(bool), WM.astype(bool)), (WF.astype(np.uint8) * 3, WM.astype(np.uint8) * 7),
             (dev(WF), dev(WM.astype(bool))), (api.Image.from_array(WF), torch.from_numpy(WM).cuda().to(torch.int32))]
    want_hist, want = mr.joint(F, M, A, 16, (float(F.min()), float(F.max())), (float(M.min()), float(M.max())), "linear",
                               WF, WM)
    got = [api.similarity(F, M, A, 16, mask_fixed=a, mask_moving=b) for a, b in kinds]
    for g in got:
        assert np.array_equal(g.joint, want_hist.astype(np.int64)) and g.count == want.count
        assert g[:8] == got[0][:8]
    assert api.similarity(F, M, A, 16)[:8] == api.similarity(F, M, A, 16, mask_fixed=None, mask_moving=None)[:8]
    assert np.array_equal(api.similarity(F, M, A, 16).joint, mr.joint(F, M, A, 16, (float(F.min()), float(F.max())),
                                                                      (float(M.min()), float(M.max())))[0].astype(np.int64))
    Fa, Ma, _, WFa = affine_case()
    ra = [api.refine_affine(Ma, Fa, mask_fixed=w, max_evaluations=3)
          for w in (WFa, WFa.astype(bool), WFa.astype(np.uint8), dev(WFa))]
    for r in ra[1:]:
        assert np.array_equal(r.A, ra[0].A) and np.array_equal(r.count, ra[0].count)
    before = api.refine_affine(Ma, Fa, max_evaluations=3)
    none = api.refine_affine(Ma, Fa, mask_fixed=None, mask_moving=None, max_evaluations=3)
    assert np.array_equal(before.A, none.A) and np.array_equal(before.count, none.count)
    assert np.array_equal(before.msd, none.msd) and np.array_equal(before.lambdas, none.lambdas)
    assert ra[0].count[0] < before.count[0]
    Ff, Mf, _, WFf, WMf = ffd_case()
    rf = [api.refine_ffd(Mf, Ff, None, 8, 1, 0.005, mask_fixed=a, mask_moving=b, max_evaluations=3)
          for a, b in ((WFf, WMf), (WFf.astype(bool), WMf.astype(np.uint8)), (dev(WFf), dev(WMf)))]
    for r in rf[1:]:
        assert np.array_equal(r.lattice.cpu().numpy(), rf[0].lattice.cpu().numpy()) and r.trail == rf[0].trail
    before = api.refine_ffd(Mf, Ff, None, 8, 1, 0.005, max_evaluations=3)
    none = api.refine_ffd(Mf, Ff, None, 8, 1, 0.005, mask_fixed=None, mask_moving=None, max_evaluations=3)
    assert np.array_equal(before.lattice.cpu().numpy().view(np.uint32), none.lattice.cpu().numpy().view(np.uint32))
    assert before.trail == none.trail and rf[0].trail[0].n < before.trail[0].n
    for bad in (lambda: api.similarity(F, M, A, mask_fixed=WM), lambda: api.similarity(dev(F), dev(M), A,
                                                                                      mask_moving=torch.ones(MSHAPE))):
        with pytest.raises(ValueError):
            bad()
