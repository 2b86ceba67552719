"""The Jacobian penalty on the device (include/sift3d_amd.h, "Jacobian penalty") against the numpy restatement
(tests/jacobian_penalty_restatement.py): nonpos, rmin, rmax and every entry of S bit for bit, between guard bands; `sum`
to gamma_(N + 8) sum |phi| (any order of summing N doubles whose values are the restatement's own, bit for bit; the
restatement's sum is correctly rounded; the 8 is tests/test_ffd.py's allowance); the lattice gradient to that file's
bound for Gc; the driver with weight 0 byte for byte against the existing drivers, its trail against its own penalty
array, against the restatement's driver, and on a pair that folds without the penalty."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import ffd_restatement as fr
from tests import jacobian_penalty_restatement as jp
from tests.demons_restatement import gamma
from tests.test_ffd import GRIDS
from tests.test_ffd_host import DRIVER, driver_pair, summarize
from tests.test_similarity import dev
from tests.test_warp import about_center, rot

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL = 0x7FC0DEAD                                       # a quiet NaN with a payload (tests/test_sampling_matrix.py)
GUARD = 64                                                  # 32-bit words before and after an output
TILE = (8, 4, 64)                                           # the value pass' tile (z, y, x)
# (1, 1, 1); axes of length 1, 2, 3 and 4 on every axis; one voxel more than a tile along x, y and z
SHAPES = [(1, 1, 1), (1, 2, 3), (2, 1, 4), (3, 4, 1), (TILE[0] + 1, TILE[1] + 1, TILE[2] + 1)]


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


class Carved:
    """A float64 (or int64-sized) output of n 8-byte words carved out of a larger buffer of sentinel words, 8-byte
    aligned; intact() is whether every word before and after it still holds the sentinel"""

    def __init__(self, n):
        import torch
        self.n = 2 * int(n)
        self.buf = torch.full((GUARD + self.n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.view = self.buf[GUARD:GUARD + self.n]
        assert self.view.data_ptr() % 8 == 0

    def ptr(self):
        return self.view.data_ptr()

    def numpy(self):
        return self.view.cpu().numpy().view(np.float64)

    def intact(self):
        b = self.buf.cpu().numpy()
        return bool(np.all(b[:GUARD] == SENTINEL) and np.all(b[GUARD + self.n:] == SENTINEL))


def run(hip, u, ref, gradient=True):
    """sift3d_hip_jacobian_penalty with record, S and the work buffer each of its exact size between guard bands:
    ((nonpos, sum, rmin, rmax), S or None, the record's 32 bytes)"""
    import torch
    L = hip.lib()
    _, oz, oy, ox = u.shape
    n = oz * oy * ox
    rec, S = Carved(4), Carved(3 * n) if gradient else None
    need = L.sift3d_amd_jacobian_penalty_work_bytes(ox, oy, oz)
    assert need == 8 * (4 * hip.SIMILARITY_GRID + n)
    work = Carved(need // 8)
    field = dev(u)
    rc = L.sift3d_hip_jacobian_penalty(field.data_ptr(), ox, oy, oz, float(ref), rec.ptr(),
                                       S.ptr() if gradient else None, work.ptr(), hip.current_stream())
    assert rc == 0, L.sift3d_hip_last_error()
    torch.cuda.synchronize()
    assert rec.intact() and work.intact() and (S is None or S.intact())
    raw = rec.view.cpu().numpy().view(np.uint8)
    v = raw[8:].view(np.float64)
    head = (int(raw[:8].view(np.uint64)[0]), float(v[0]), float(v[1]), float(v[2]))
    return head, (S.numpy().reshape((3, oz, oy, ox)) if gradient else None), raw.tobytes()


def same_bits(got, want, what):
    """float64 arrays bit for bit; a NaN matches a NaN whatever its payload"""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (got.view(np.uint64) != want.view(np.uint64)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


def check(hip, u, ref, what):
    want = jp.penalty(u, ref)
    (nonpos, total, rmin, rmax), S, raw = run(hip, u, ref)
    n = u[0].size
    print("%s: nonpos %d sum %.17g (off %.3g) r in [%.6g, %.6g]" % (what, nonpos, total, abs(total - want.sum), rmin,
                                                                   rmax))
    assert nonpos == want.nonpos and rmin == want.rmin and rmax == want.rmax, (what, nonpos, rmin, rmax, want[3:6])
    if np.isnan(want.sum):
        assert np.isnan(total), what
    else:
        assert abs(total - want.sum) <= gamma(n + 8) * want.sum_abs, (what, total, want.sum)
    same_bits(S, want.S, what)
    head, none, raw_value = run(hip, u, ref, gradient=False)             # d_grad == NULL: the same record bytes
    assert none is None and raw_value == raw, what
    return want


def affine_field(shape):
    """the field of a rotation and scale about the centre, float32 as the export rounds it, and the determinant of its
    linear part"""
    A = about_center(rot((1, 2, 3), 11.0) * 1.08, shape, shape, shift=(0.25, -0.5, 0.125))
    return fr.ref_affine_field(A, shape), jp.ref_of(A)


@functools.lru_cache(maxsize=None)
def random_field(shape):
    """a random float32 field in which the restatement sees r >= 1/4, 0 < r < 1/4 and r <= 0: the first (amplitude, seed)
    in a fixed order that does, chosen here on the CPU.  (1, 1, 1) has no derivative: r = 1 whatever the field."""
    for amplitude in (1.0, 1.5, 2.0, 3.0):
        for seed in range(64):
            u = np.random.default_rng(seed).uniform(-amplitude, amplitude, (3,) + shape).astype(F32)
            r = jp.penalty(u, 1.0).r
            if np.prod(shape) == 1 or ((r >= 0.25).any() and ((r > 0) & (r < 0.25)).any() and (r <= 0).any()):
                return u
    raise AssertionError("no field with all three branches on %s" % (shape,))


@pytest.mark.parametrize("shape", SHAPES)
def test_record_and_sum_form(hip, shape):
    u, ref = affine_field(shape)
    want = check(hip, u, ref, "%s affine" % (shape,))
    if min(shape) >= 2:
        # (an axis of length 1 has no derivative, so there j is not the map's linear part and r is not 1.)  float32 j
        # of an affine field whose entries stay below 16: a difference of two entries is within 2 ulp32(16) = 2^-19 of
        # the exact one, and det / ref - 1 within 3 * 1.2^2 / 1.26 = 3.5 of those to first order
        assert np.abs(u).max() < 16 and np.all(np.abs(want.r - 1.0) <= 4 * 2.0 ** -19) and want.nonpos == 0
    u = random_field(shape)
    want = check(hip, u, 1.0, "%s random" % (shape,))
    r = want.r
    if np.prod(shape) > 1:
        assert (r >= 0.25).any() and ((r > 0) & (r < 0.25)).any() and (r <= 0).any()
        assert np.abs(want.S).max() > 0
    else:
        assert r[0, 0, 0] == 1.0 and want.P == 0.0 and not want.S.any()
    check(hip, u, -0.75, "%s random, negative ref" % (shape,))
    v = u.copy()
    v[1][tuple(s // 2 for s in shape)] = np.nan
    want = check(hip, v, 1.0, "%s with a NaN" % (shape,))
    if np.prod(shape) > 1:
        assert np.isnan(want.sum) and np.isnan(want.r).any() and want.nonpos >= int(np.isnan(want.r).sum())
        assert np.isnan(want.S).any() and np.isfinite(want.rmin) and np.isfinite(want.rmax)


def test_more_tiles_than_workgroups_and_calls_repeat(hip):
    """tests/test_ffd.py's construction on this kernel's tile: more tiles than partial slots, so that workgroups take
    several tiles each; a second call repeats every byte"""
    G = hip.SIMILARITY_GRID
    ty = int(np.ceil(np.sqrt(G + 1)))
    tz = -(-(G + 1) // ty)
    shape = (TILE[0] * (tz - 1) + 1, TILE[1] * (ty - 1) + 1, 2)
    assert G < ty * tz < 2 * G
    u = np.random.default_rng(5).uniform(-1.0, 1.0, (3,) + shape).astype(F32)
    want = check(hip, u, 1.0, "grid cap")
    assert (want.r >= 0.25).any() and ((want.r > 0) & (want.r < 0.25)).any() and (want.r <= 0).any()
    _, S0, raw0 = run(hip, u, 1.0)
    _, S1, raw1 = run(hip, u, 1.0)
    assert raw0 == raw1 and S0.tobytes() == S1.tobytes()


@pytest.mark.parametrize("k", [0, 4])
def test_lattice_gradient(hip, k):
    """GJ against ffd_restatement.adjoint of the restatement's S (the device's S is that, bit for bit): tests/test_ffd.py's
    bound for Gc, gamma_(support + 8) sum |term|"""
    shape, spacing = GRIDS[k]
    u = np.random.default_rng(40 + k).uniform(-1.5, 1.5, (3,) + shape).astype(F32)
    want = jp.penalty(u, 1.25)
    rec, GJ = hip.ffd_jacobian_gradient(dev(u), spacing, 1.25)
    nonpos, total, rmin, rmax = hip.jacobian_penalty_record(rec)
    assert (nonpos, rmin, rmax) == (want.nonpos, want.rmin, want.rmax)
    GJ = GJ.cpu().numpy()
    assert GJ.shape == fr.lattice_shape(shape, spacing)
    for d in range(3):
        exact, terms, support = fr.adjoint(want.S[d], spacing)
        bound = np.array([gamma(int(s) + 8) for s in support.reshape(-1)]).reshape(support.shape) * terms
        off = np.abs(GJ[d] - exact)
        assert np.all(off <= bound), (k, d, off.max(), (off - bound).max())
    assert np.abs(GJ).max() > 0


def test_api_matches_the_entry(hip):
    from sift3d_amd import api
    u = random_field(SHAPES[-1])
    want = jp.penalty(u, 1.5)
    p = api.jacobian_penalty(u, 1.5, gradient=True)
    assert (p.nonpositive, p.min, p.max) == (want.nonpos, want.rmin, want.rmax)
    assert abs(p.value - want.P) <= gamma(u[0].size + 9) * want.sum_abs / u[0].size
    # S is the restatement's bit for bit (above); the division by N is torch's, which may multiply by the rounded 1 / N
    # instead: two roundings against one
    g, w = p.gradient.cpu().numpy(), want.S / float(u[0].size)
    assert g.shape == w.shape and np.all(np.abs(g - w) <= 3 * 2.0 ** -53 * np.abs(w))
    assert api.jacobian_penalty(dev(u), 1.5).gradient is None


# ---- the driver ------------------------------------------------------------------------------------------------------
def trail_bytes(res):
    return C.string_at(C.addressof(res), 8 + 48 * res.evaluations)       # evaluations, stop and the entries run


@pytest.mark.parametrize("metric", ["msd", "mi"])
def test_weight_zero_is_the_existing_driver_byte_for_byte(hip, metric):
    """additions only: lattice, field and trail of the new entry with jacobian = 0 against the existing entry's"""
    F, M, _ = driver_pair()
    p = hip.ffd_refine_params(spacing=DRIVER["spacing"], levels=DRIVER["levels"], bending=DRIVER["bending"],
                              max_evaluations=6)
    rf, rm = (float(F.min()), float(F.max())), (float(M.min()), float(M.max()))
    if metric == "mi":
        old = hip.ffd_mi_refine(dev(F), dev(M), 32, rf, rm, None, p)
        new = hip.ffd_refine_jacobian(dev(F), dev(M), 0.0, 32, rf, rm, None, p)
        assert bytes(memoryview(old[3])) == bytes(memoryview(new[3]))    # the measures at the end
    else:
        old = hip.ffd_refine(dev(F), dev(M), None, p)
        new = hip.ffd_refine_jacobian(dev(F), dev(M), 0.0, params=p)
    assert trail_bytes(old[0]) == trail_bytes(new[0]) and old[0].evaluations > 2
    assert old[1].cpu().numpy().tobytes() == new[1].cpu().numpy().tobytes()
    assert old[2].cpu().numpy().tobytes() == new[2].cpu().numpy().tobytes()
    pen = new[4]
    assert len(pen) == new[0].evaluations and pen[0][0] == 0.0 and pen[0][1] == 1.0      # the zero lattice: r = 1
    assert all(np.isfinite(q[0]) and q[2] == 0 for q in pen)


@pytest.mark.parametrize("metric", ["msd", "mi"])
def test_trail_is_consistent_with_the_penalty_array(metric):
    """E = (image + bending R) + jacobian P from the trail and the penalty array, bit for bit; the last accepted P is
    the final field's"""
    from sift3d_amd import api
    F, M, _ = driver_pair()
    w = 0.25
    kw = dict(metric="mi", bins=32, max_evaluations=5) if metric == "mi" else dict(max_evaluations=8)
    r = api.refine_ffd(M, F, None, DRIVER["spacing"], DRIVER["levels"], DRIVER["bending"], jacobian=w, **kw)
    assert type(r).__name__ == ("JacMiFFDRefinement" if metric == "mi" else "JacFFDRefinement")
    assert r.jacobian_weight == w and len(r.penalty) == len(r.trail) > 2
    for e, q in zip(r.trail, r.penalty):
        assert e.E == (e.msd + DRIVER["bending"] * e.R) + w * q.P, (e, q)
    for l in range(DRIVER["levels"]):
        acc = [e.E for e in r.trail if e.level == l and e.accepted]
        assert all(b < a for a, b in zip(acc, acc[1:]))
    last = [q for e, q in zip(r.trail, r.penalty) if e.level == 0 and e.accepted][-1]
    at_end = api.jacobian_penalty(r.field)
    assert (last.P, last.rmin, last.nonpositive) == (at_end.value, at_end.min, at_end.nonpositive)
    assert at_end.nonpositive == r.jacobian.folded


PENALISED = dict(jacobian=0.25, max_evaluations=8)


@functools.lru_cache(maxsize=None)
def restatement_driver():
    F, M, truth = driver_pair()
    r = jp.refine(F, M, None, DRIVER["spacing"], DRIVER["levels"], DRIVER["bending"], PENALISED["jacobian"],
                  PENALISED["max_evaluations"])
    return r, summarize(r.trail, r.field, truth), jp.penalty(r.field, 1.0).P


def test_driver_against_the_restatement():
    """tests/test_ffd.py's margins, for its reason (the device's summation order may flip one accept / reject): the MSD
    falls by at least half the factor the restatement reached, the RMS field error is at most 1.5 x the restatement's;
    and P of the final field is within a factor two of the restatement's"""
    from sift3d_amd import api
    F, M, truth = driver_pair()
    ref, (ratio_ref, rms_ref), P_ref = restatement_driver()
    r = api.refine_ffd(M, F, None, DRIVER["spacing"], DRIVER["levels"], DRIVER["bending"], **PENALISED)
    trail = [tuple(e) for e in r.trail]
    ratio, rms = summarize(trail, r.field.cpu().numpy(), truth)
    P = api.jacobian_penalty(r.field).value
    print("device driver with the penalty: stop %s, %d evaluations, MSD ratio %.4g (restatement %.4g), RMS %.4g "
          "(restatement %.4g), P %.4g (restatement %.4g)" % (r.stop, len(trail), ratio, ratio_ref, rms, rms_ref, P, P_ref))
    lv = [e[6] for e in trail]
    assert lv == sorted(lv, reverse=True) and set(lv) == set(range(DRIVER["levels"]))
    assert 1.0 / ratio >= 0.5 / ratio_ref
    assert rms <= 1.5 * rms_ref
    assert 0.5 * P_ref <= P <= 2.0 * P_ref
    assert np.array_equal(r.field.cpu().numpy(), fr.field(r.lattice.cpu().numpy(), 8, F.shape))


# ---- the point of the feature ----------------------------------------------------------------------------------------
# Fixed: a wide Gaussian blob (sigma 8) in 32^3; moving: the same blob much narrower (sigma 3).  Matching them squeezes
# the grid towards the centre by 3 / 8 per axis, a determinant near 0.05, and at spacing 4 without bending the
# unpenalised fit overshoots into folds.  Recorded from the restatement's driver (jacobian_penalty_restatement.refine,
# spacing 4, 2 levels, 40 evaluations per level, bending 0): without the penalty the final field has 2630 voxels with
# r <= 0 (rmin -0.0479); the weights 2^-14 .. 2^-8 leave 2475, 2460, 2483, 2274, 2132, 1437 and 492; 2^-7 is the
# smallest power of two that ends with none (rmin 0.0146, final MSD 0.00989 from 0.0691 before registration).
FOLD = dict(n=32, sigma_fixed=8.0, sigma_moving=3.0, spacing=4, levels=2, max_evaluations=40)
FOLD_RESTATEMENT_NONPOS = 2630
FOLD_RESTATEMENT_NONPOS_PENALISED = 0
FOLD_WEIGHT = 2.0 ** -7


def blob(n, sigma):
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    c = (n - 1) / 2.0
    return np.exp(-((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) / (2 * sigma * sigma)).astype(F32)


def test_the_penalty_keeps_a_folding_fit_invertible():
    from sift3d_amd import api
    F, M = blob(FOLD["n"], FOLD["sigma_fixed"]), blob(FOLD["n"], FOLD["sigma_moving"])
    start = float(np.mean((F.astype(np.float64) - M.astype(np.float64)) ** 2))
    kw = dict(max_evaluations=FOLD["max_evaluations"])
    free = api.refine_ffd(M, F, None, FOLD["spacing"], FOLD["levels"], 0.0, **kw)
    held = api.refine_ffd(M, F, None, FOLD["spacing"], FOLD["levels"], 0.0, jacobian=FOLD_WEIGHT, **kw)
    msd = [e.msd for e in held.trail if e.level == 0 and e.accepted][-1]
    print("unpenalised: folded %d (restatement %d), min det %.4g; jacobian = 2^-7: folded %d, min det %.4g, MSD %.4g "
          "from %.4g" % (free.jacobian.folded, FOLD_RESTATEMENT_NONPOS, free.jacobian.min, held.jacobian.folded,
                         held.jacobian.min, msd, start))
    assert free.jacobian.folded > 0
    assert held.jacobian.folded == FOLD_RESTATEMENT_NONPOS_PENALISED == 0
    assert msd < start
