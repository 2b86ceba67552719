"""The landmark term on the device (include/sift3d_amd.h, "FFD landmarks") against the numpy restatement
(tests/ffd_landmarks_restatement.py): mapped points, the count, rmax and every residual bit for bit; S, Omega and every
entry of GL to their gamma bounds (the restatement's own sums are correctly rounded); repeated calls byte for byte; the
driver with weight 0 against the existing drivers byte for byte and with the term against the restatement's driver on the
pair of tests/test_ffd_host.py; the Python interface."""
import ctypes as C

import numpy as np
import pytest

from tests import ffd_landmarks_restatement as lr
from tests import ffd_restatement as fr
from tests.demons_restatement import gamma
from tests.test_ffd import GRIDS, random_lattice, rotating
from tests.test_ffd_host import DRIVER, driver_pair, summarize
from tests.test_ffd_landmarks_host import (LANDMARKS, WEIGHT, driver_landmarks, field_rms, landmark_rms,
                                           restatement_with_landmarks)
from tests.test_similarity import dev

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
SIZES = (1, 63, 64, 65, 257, 65536)                         # 65536: two strides of the 128-workgroup grid


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


def same_bits(got, want):
    """equal bit for bit, any NaN standing for any NaN"""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got.view(np.int64)[~nan], want.view(np.int64)[~nan])


def edge_coordinates(o, delta):
    top = float((fr.lattice_dim(o, delta) - 3) * delta)
    return [0.0, -0.0, o - 1.0, np.nextafter(top, 0.0), top, -1e-300, -0.5, np.nan, np.inf, -np.inf]


def point_pool(shape, spacing, seed):
    """whole voxels, random sub-voxel points of the lattice's support and beyond it, and the edge coordinates of each
    axis beside an ordinary value of the other two"""
    oz, oy, ox = shape
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    whole = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)[:400]
    top = np.array([(fr.lattice_dim(o, d) - 3) * d for o, d in zip((ox, oy, oz), spacing)], np.float64)
    sub = rng.uniform(-0.05, 1.05, (400, 3)) * top
    edges = []
    for ax, (o, d) in enumerate(zip((ox, oy, oz), spacing)):
        for v in edge_coordinates(o, d):
            p = [0.5 * (ox - 1), 0.25 * (oy - 1), 0.75 * (oz - 1)]
            p[ax] = v
            edges.append(p)
    return np.concatenate([np.array(edges), sub, whole])


@pytest.mark.parametrize("k", range(len(GRIDS)))
@pytest.mark.parametrize("affine", [False, True])
def test_points_bit_for_bit(hip, k, affine):
    shape, spacing = GRIDS[k]
    c = random_lattice(shape, spacing, 40 + k)
    A = rotating(shape) if affine else None
    pool = point_pool(shape, spacing, k)
    lat = dev(c)
    for m in SIZES:
        P = pool[np.arange(m) % len(pool)]
        want, inside = lr.points(c, spacing, P, A)
        got = hip.ffd_points(lat, spacing, P, A).cpu().numpy()
        assert same_bits(got, want), (shape, m)
        assert m < 30 or (inside.any() and not inside.all())


def check_landmarks(hip, c, spacing, P, Q, w, A, what):
    import torch
    lat = dev(c)
    want = lr.landmarks(c, spacing, P, Q, w, A)
    rec, r, GL = hip.ffd_landmarks(lat, spacing, P, Q, w, A)
    counted, S, Om, rmax = hip.ffd_landmarks_record(rec)
    m = len(P)
    print("%s: counted %d S %.17g (off %.3g) Omega %.17g rmax %.17g" % (what, counted, S, abs(S - want.S), Om, rmax))
    assert counted == want.counted and rmax == want.rmax, (what, counted, want.counted, rmax, want.rmax)
    assert same_bits(r.cpu().numpy(), want.r), what
    assert not np.signbit(r.cpu().numpy()[~want.inside]).any()          # +0 where not counted
    assert abs(S - want.S) <= gamma(m + 8) * want.S_terms and abs(Om - want.Omega) <= gamma(m + 8) * want.Omega_terms
    G = GL.cpu().numpy()
    bound = np.array([gamma(int(n) + 8) for n in want.support.reshape(-1)]).reshape(want.support.shape) * want.GL_terms
    assert np.all(np.abs(G - want.GL) <= bound), (what, np.abs(G - want.GL).max())
    assert not np.isnan(G).any() and not np.signbit(G[:, want.support == 0]).any()
    # a call repeats its bytes; leaving GL (and the residuals) out leaves the record's bytes as they are
    rec2, r2, GL2 = hip.ffd_landmarks(lat, spacing, P, Q, w, A)
    rec3, r3, GL3 = hip.ffd_landmarks(lat, spacing, P, Q, w, A, residuals=False, gradient=False)
    assert r3 is None and GL3 is None
    raw = rec.cpu().numpy().tobytes()
    assert raw == rec2.cpu().numpy().tobytes() == rec3.cpu().numpy().tobytes()
    assert torch.equal(r.view(torch.int64), r2.view(torch.int64)) and torch.equal(GL.view(torch.int64),
                                                                                 GL2.view(torch.int64))
    return want, (counted, S, Om, rmax), G


def weights_with_zeros(m, seed):
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.0, 2.0, m)
    w[rng.integers(0, m, max(1, m // 5))] = 0.0
    return w


@pytest.mark.parametrize("k", range(len(GRIDS)))
@pytest.mark.parametrize("affine", [False, True])
def test_landmarks_record_residuals_and_gradient(hip, k, affine):
    shape, spacing = GRIDS[k]
    c = random_lattice(shape, spacing, 50 + k)
    A = rotating(shape) if affine else None
    pool = point_pool(shape, spacing, 10 + k)
    rng = np.random.default_rng(60 + k)
    P = pool[rng.permutation(len(pool))[:300]]
    Q = rng.uniform(-3.0, 3.0, (300, 3)) + np.nan_to_num(P, nan=0.0, posinf=0.0, neginf=0.0)
    want, _, _ = check_landmarks(hip, c, spacing, P, Q, weights_with_zeros(300, k), A, "%s mixed" % (shape,))
    assert 0 < want.counted < 300
    check_landmarks(hip, c, spacing, P, Q, None, A, "%s unit weights" % (shape,))


def test_landmarks_special_cases(hip):
    shape, spacing = GRIDS[0]
    c = random_lattice(shape, spacing, 70)
    rng = np.random.default_rng(71)
    d = np.array(spacing, np.float64)
    one_cell = (np.array([1.0, 1.0, 0.0]) + rng.uniform(0.0, 1.0, (300, 3))) * d          # cell (0, 1, 1)
    one_cell[:, 0] = np.minimum(one_cell[:, 0], np.nextafter(2 * d[0], 0.0))
    Q = one_cell + rng.uniform(-1.0, 1.0, (300, 3))
    want, _, G = check_landmarks(hip, c, spacing, one_cell, Q, weights_with_zeros(300, 1), None, "300 in one cell")
    assert want.counted == 300 and (want.support > 0).sum() == 64 and want.support.max() == 300
    same = np.tile(np.array([[3.3, 2.2, 1.1]]), (64, 1))
    want, (_, S, Om, rmax), _ = check_landmarks(hip, c, spacing, same, same + 0.5, None, rotating(shape),
                                                "one point 64 times")
    assert want.counted == 64 and Om == 64.0
    outside = np.stack([np.full(40, -1.0), rng.uniform(0, 5, 40), rng.uniform(0, 3, 40)], axis=1)
    outside[::3, 0] = np.nan
    outside[1::3, 0] = 1e6
    want, got, G = check_landmarks(hip, c, spacing, outside, np.zeros((40, 3)), None, None, "every landmark outside")
    assert got == (0, 0.0, 0.0, 0.0) and lr.term(want) == (0.0, 0.0)
    assert not G.view(np.int64).any()                                    # GL: all +0
    zero_w = rng.uniform(0, 1, (20, 3)) * (np.array(shape[::-1]) - 1.0)
    want, got, G = check_landmarks(hip, c, spacing, zero_w, zero_w, np.zeros(20), None, "all weights zero")
    assert got[0] == 20 and got[1] == 0.0 and got[2] == 0.0 and got[3] > 0 and not G.any()
    big = point_pool(shape, spacing, 5)
    big = big[np.arange(65536) % len(big)]
    check_landmarks(hip, c, spacing, big, np.nan_to_num(big, nan=0.0, posinf=0.0, neginf=0.0) + 0.25,
                    weights_with_zeros(65536, 2), None, "65536 landmarks")


# ---- the evaluation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 4])
@pytest.mark.parametrize("jacobian", [None, 0.0, 0.3])
def test_gradient_bit_for_bit_from_the_device_sums(hip, k, jacobian):
    """d_grad = (float)(base_g + ((lambda * 2) / Omega) * GL) from the device's own Gc, dR, (GJ,) GL and Omega; no term
    where Omega == 0; landmark_weight == 0 is the evaluation without landmarks"""
    from tests.test_similarity import volumes
    shape, spacing = GRIDS[k]
    F, M = volumes(shape, (shape[0] + 1, shape[1] + 2, shape[2] - 1), 80 + k)
    c = random_lattice(shape, spacing, 81 + k, 0.75)
    A = rotating(shape)
    rng = np.random.default_rng(82 + k)
    pool = point_pool(shape, spacing, 20 + k)
    P = pool[rng.permutation(len(pool))[:100]]
    Q = rng.uniform(-2.0, 2.0, (100, 3)) + np.nan_to_num(P, nan=0.0, posinf=0.0, neginf=0.0)
    w = weights_with_zeros(100, 3)
    lam, bend, cvox = 0.37, 0.01, int(np.prod(c.shape[1:]))
    for what, Pk, lk in (("mixed", P, lam), ("outside", np.full((7, 3), -5.0), lam), ("weight 0", P, 0.0)):
        Qk, wk = (Q, w) if len(Pk) == len(Q) else (np.zeros((7, 3)), None)
        rec, grad, fld, lm, jac = hip.ffd_evaluate_landmarks(dev(F), dev(M), dev(c), spacing, Pk, Qk, wk, lk, A, bend,
                                                            jacobian)
        n, see, R, gmax, Gc, dR = hip.ffd_record(rec, c.shape)
        counted, S, Om, rmax = hip.ffd_landmarks_record(lm)
        GL = lm.cpu().numpy()[4:4 + 3 * cvox].reshape(c.shape)
        want = lr.landmarks(c, spacing, Pk, Qk, wk, A)
        assert counted == want.counted and rmax == want.rmax and n > 0
        g = (2.0 / np.float64(n)) * Gc + bend * dR
        if jacobian:
            g = g + (jacobian / np.float64(F.size)) * jac.cpu().numpy()[4:4 + 3 * cvox].reshape(c.shape)
        if lk > 0 and Om != 0.0:
            g = g + ((lk * 2.0) / Om) * GL
            assert GL.any()
        g = g.astype(np.float32)
        assert np.array_equal(grad.cpu().numpy(), g) and gmax == float(np.abs(g).max()), (what, jacobian)
        if what != "mixed" and not jacobian:                             # no term: the evaluation without landmarks
            old = hip.ffd_evaluate(dev(F), dev(M), dev(c), spacing, A, bend)
            assert old[0].cpu().numpy().tobytes() == rec.cpu().numpy().tobytes()
            assert np.array_equal(old[1].cpu().numpy(), grad.cpu().numpy())


def grid_cap_shape(hip):
    """tests/test_ffd.py's grid-cap shape: more tiles than workgroups, a second, partial pass over them"""
    G = hip.SIMILARITY_GRID
    ty = int(np.ceil(np.sqrt(G + 1)))
    tz = -(-(G + 1) // ty)
    assert G < ty * tz < 2 * G
    return (4 * (tz - 1) + 1, 4 * (ty - 1) + 1, 2), (2, 16, 16)


# the two smallest grids; the grid cap of the image passes; a lattice of more elements than the combine's 256 lanes times
# its SIMILARITY_GRID workgroups, so that its lanes take a second element: without the landmark term and with it
COMBINE_CASES = [(2, 0.0), (0, 0.0), ("grid cap", 0.0), ("stride", 0.0), ("stride", 0.37)]


@pytest.mark.parametrize("case, lam", COMBINE_CASES)
def test_penalty_gradient_bit_for_bit_from_the_device_sums(hip, case, lam):
    """the combine with the penalty's term and landmarks of weight 0 (their record is made, no term is added), and on the
    large lattice with both terms: d_grad = (float)(((2 / n) * Gc + bending * dR) + (jacobian / N) * GJ [+ ((lambda * 2) /
    Omega) * GL]) from the device's own sums, and gmax its largest magnitude"""
    from tests.test_similarity import volumes
    shape, spacing = grid_cap_shape(hip) if case == "grid cap" else ((56, 56, 56), (1, 1, 1)) if case == "stride" \
        else GRIDS[case]
    seed = 90 + COMBINE_CASES.index((case, lam))
    F, M = volumes(shape, (shape[0] + 1, shape[1] + 2, shape[2] + 1), seed)
    c = random_lattice(shape, spacing, seed + 10, 0.75)
    rng = np.random.default_rng(seed + 20)
    P = rng.uniform(0.0, 1.0, (100, 3)) * (np.array(shape[::-1]) - 1.0)
    Q = P + rng.uniform(-2.0, 2.0, (100, 3))
    jacobian, bend, cvox = 0.3, 0.01, int(np.prod(c.shape[1:]))
    assert (case == "stride") == (3 * cvox > 256 * hip.SIMILARITY_GRID)
    rec, grad, fld, lm, jac = hip.ffd_evaluate_landmarks(dev(F), dev(M), dev(c), spacing, P, Q, None, lam, rotating(shape),
                                                        bend, jacobian)
    n, see, R, gmax, Gc, dR = hip.ffd_record(rec, c.shape)
    counted, S, Om, rmax = hip.ffd_landmarks_record(lm)
    GJ = jac.cpu().numpy()[4:4 + 3 * cvox].reshape(c.shape)
    GL = lm.cpu().numpy()[4:4 + 3 * cvox].reshape(c.shape)
    assert n > 0 and counted > 0 and Om > 0 and GJ.any() and GL.any() == (lam > 0)
    g = ((2.0 / np.float64(n)) * Gc + bend * dR) + (jacobian / np.float64(F.size)) * GJ
    if lam > 0:
        g = g + ((lam * 2.0) / Om) * GL
    g = g.astype(np.float32)
    print("%s: n %d counted %d gmax %.9g |GJ| %.3g" % (case, n, counted, gmax, np.abs(GJ).max()))
    assert np.array_equal(grad.cpu().numpy(), g) and gmax == float(np.abs(g).max()), (case, lam)


# ---- the driver ------------------------------------------------------------------------------------------------------
def trail_bytes(res):
    return C.string_at(C.addressof(res), 8 + 48 * res.evaluations)       # evaluations, stop and the entries run


@pytest.mark.parametrize("kind", ["msd", "masks", "mi", "jacobian"])
def test_weight_zero_is_the_existing_driver_byte_for_byte(hip, kind):
    """additions only: lattice, field, trail (and penalty) of the new entry with landmark_weight = 0 against the
    existing entries', with L recorded beside them"""
    F, M, _ = driver_pair()
    P, Q = driver_landmarks()
    p = hip.ffd_refine_params(spacing=DRIVER["spacing"], levels=DRIVER["levels"], bending=DRIVER["bending"],
                              max_evaluations=5)
    rf, rm = (float(F.min()), float(F.max())), (float(M.min()), float(M.max()))
    kw = {}
    if kind == "masks":
        z = np.arange(F.shape[0])[:, None, None]
        WF = np.broadcast_to((z >= 6).astype(np.float32), F.shape).copy()
        WM = np.broadcast_to((z < 44).astype(np.float32), M.shape).copy()
        kw = dict(mask_fixed=dev(WF), mask_moving=dev(WM))
        old = hip.ffd_refine(dev(F), dev(M), None, p, **kw)
        new = hip.ffd_refine_landmarks(dev(F), dev(M), P, Q, None, 0.0, params=p, **kw)
    elif kind == "mi":
        old = hip.ffd_mi_refine(dev(F), dev(M), 32, rf, rm, None, p)
        new = hip.ffd_refine_landmarks(dev(F), dev(M), P, Q, None, 0.0, bins=32, range_f=rf, range_m=rm, params=p)
        assert bytes(memoryview(old[3])) == bytes(memoryview(new[3]))    # the measures at the end
    elif kind == "jacobian":
        old = hip.ffd_refine_jacobian(dev(F), dev(M), 0.01, params=p)
        new = hip.ffd_refine_landmarks(dev(F), dev(M), P, Q, None, 0.0, jacobian=0.01, params=p)
        assert old[4] == new[4]
    else:
        old = hip.ffd_refine(dev(F), dev(M), None, p)
        new = hip.ffd_refine_landmarks(dev(F), dev(M), P, Q, None, 0.0, params=p)
    assert trail_bytes(old[0]) == trail_bytes(new[0]) and old[0].evaluations > 2
    assert old[1].cpu().numpy().tobytes() == new[1].cpu().numpy().tobytes()
    assert old[2].cpu().numpy().tobytes() == new[2].cpu().numpy().tobytes()
    terms = new[5]
    assert len(terms) == new[0].evaluations
    assert all(np.isfinite(t[0]) and t[0] > 0 and t[1] > 0 and t[2] == LANDMARKS for t in terms)
    # the zero lattice of the coarsest level: r = P - Q, reported in level-0 voxels
    first = lr.landmarks(np.zeros(fr.lattice_shape((24, 24, 24), 8), np.float32), 8, P * 0.5, Q * 0.5)
    assert abs(terms[0][0] - lr.term(first, 1)[0]) <= gamma(LANDMARKS + 12) * terms[0][0]
    assert terms[0][1] == lr.term(first, 1)[1]


@pytest.fixture(scope="module")
def device_with_landmarks():
    from sift3d_amd import api
    F, M, _ = driver_pair()
    return api.refine_ffd(M, F, None, DRIVER["spacing"], DRIVER["levels"], DRIVER["bending"],
                          max_evaluations=DRIVER["max_evaluations"], landmarks=driver_landmarks(),
                          landmark_weight=WEIGHT)


def last_accepted(trail, terms):
    return [(e, t) for e, t in zip(trail, terms) if e[6] == 0 and e[5]][-1]


def test_driver_against_the_restatement(device_with_landmarks):
    """tests/test_ffd.py's margins, for its reason (the device's summation order may flip one accept / reject): the MSD
    falls by at least half the factor the restatement reached, the RMS field error is at most 1.5 x the restatement's,
    and the final L is within a factor two of the restatement's"""
    F, M, truth = driver_pair()
    ref = restatement_with_landmarks()
    ratio_ref, rms_ref = summarize(ref.trail, ref.field, truth)
    L_ref = last_accepted(ref.trail, ref.landmarks)[1][0]
    r = device_with_landmarks
    trail = [tuple(e) for e in r.trail]
    ratio, rms = summarize(trail, r.field.cpu().numpy(), truth)
    L = last_accepted(trail, [tuple(t) for t in r.landmarks])[1][0]
    print("device driver with landmarks: stop %s, %d evaluations, MSD ratio %.4g (restatement %.4g), RMS %.4g "
          "(restatement %.4g), L %.4g (restatement %.4g)" % (r.stop, len(trail), ratio, ratio_ref, rms, rms_ref, L, L_ref))
    lv = [e[6] for e in trail]
    assert lv == sorted(lv, reverse=True) and set(lv) == set(range(DRIVER["levels"]))
    assert 1.0 / ratio >= 0.5 / ratio_ref
    assert rms <= 1.5 * rms_ref
    assert 0.5 * L_ref <= L <= 2.0 * L_ref
    assert np.array_equal(r.field.cpu().numpy(), fr.field(r.lattice.cpu().numpy(), 8, F.shape))


# ---- the Python interface --------------------------------------------------------------------------------------------
def test_refine_ffd_returns_the_extended_result(device_with_landmarks):
    r = device_with_landmarks
    assert type(r).__name__ == "LmFFDRefinement" and r.landmark_weight == WEIGHT
    assert len(r.landmarks) == len(r.trail) > 2
    for e, t in zip(r.trail, r.landmarks):
        assert e.E == (e.msd + DRIVER["bending"] * e.R) + WEIGHT * t.L, (e, t)
        assert t.counted == LANDMARKS and t.rmax > 0 and t.rmax * t.rmax >= t.L
    for l in range(DRIVER["levels"]):
        acc = [e.E for e in r.trail if e.level == l and e.accepted]
        assert all(b < a for a, b in zip(acc, acc[1:]))
    # the last accepted L is the final lattice's
    P, Q = driver_landmarks()
    want = lr.landmarks(r.lattice.cpu().numpy(), r.spacing, P, Q)
    L = last_accepted([tuple(e) for e in r.trail], r.landmarks)[1]
    assert abs(L.L - lr.term(want)[0]) <= gamma(LANDMARKS + 12) * L.L and L.rmax == want.rmax
    print("RMS landmark residual %.4g voxels" % landmark_rms(r.lattice.cpu().numpy(), r.spacing))


def test_refine_ffd_with_the_penalty_and_the_mutual_information():
    from sift3d_amd import api
    F, M, _ = driver_pair()
    r = api.refine_ffd(M, F, None, DRIVER["spacing"], DRIVER["levels"], DRIVER["bending"], max_evaluations=4,
                       metric="mi", bins=32, jacobian=0.25, landmarks=driver_landmarks(), landmark_weight=WEIGHT)
    assert type(r).__name__ == "LmJacMiFFDRefinement" and len(r.landmarks) == len(r.penalty) == len(r.trail) > 2
    for e, q, t in zip(r.trail, r.penalty, r.landmarks):
        assert e.E == ((e.msd + DRIVER["bending"] * e.R) + 0.25 * q.P) + WEIGHT * t.L, (e, q, t)
    acc = [t.L for e, t in zip(r.trail, r.landmarks) if e.accepted]
    assert acc[-1] < acc[0]


@pytest.mark.parametrize("affine", [False, True])
def test_transform_points_agrees_with_the_field(device_with_landmarks, affine):
    """T(p) - p at whole voxels against the exported field there: the field is a float32 sum of the 64 terms with the
    weights rounded to float32 (64 u32 max |c|), added in float32 to the float32 affine displacement (2 u32 of the
    field's own size more)"""
    from sift3d_amd import api
    f = device_with_landmarks
    F, _, _ = driver_pair()
    A = rotating(F.shape) if affine else None
    rng = np.random.default_rng(9)
    p = np.stack([rng.integers(0, n, 500) for n in F.shape[::-1]], axis=1).astype(np.float64)
    fld = api.ffd_field(f.lattice, f.spacing, F.shape, A).cpu().numpy().astype(np.float64)
    T, inside = api.ffd_transform_points(f.lattice, f.spacing, p, A)
    assert inside.all() and T.shape == (500, 3)
    u = fld[:, p[:, 2].astype(int), p[:, 1].astype(int), p[:, 0].astype(int)].T
    bound = 64 * U32 * float(np.abs(f.lattice.cpu().numpy()).max()) + 2 * U32 * float(np.abs(fld).max())
    assert np.abs((T - p) - u).max() <= bound
    T2, in2 = api.ffd_transform_points(f.lattice, f.spacing, [[-1.0, 0.0, 0.0], [1.5, 2.5, 3.5]], A)
    assert in2.tolist() == [False, True] and np.isnan(T2[0]).all() and not np.isnan(T2[1]).any()


def test_register_ffd_with_landmarks():
    from sift3d_amd import api
    F, M, truth = driver_pair()
    runs = {}
    for lam in (api.FFD_LANDMARK_WEIGHT, 0.0):
        runs[lam] = api.register_ffd(M, F, levels=2, landmarks=True, landmark_weight=lam,
                                     ffd_params=dict(max_evaluations=10))
    r = runs[api.FFD_LANDMARK_WEIGHT].refinement
    assert type(r).__name__ == "LmFFDRefinement" and r.landmark_weight == api.FFD_LANDMARK_WEIGHT
    p_mov, p_fix = api._matched_points(dev(M), dev(F), 0.8, {}, "test")
    _, inl = api.ransac_affine(p_mov, p_fix, api.DEFORMABLE_ERR_THRESH, 500, 1)
    assert inl.sum() > 0 and all(t.counted == inl.sum() for e, t in zip(r.trail, r.landmarks) if e.level == 0)
    assert runs[api.FFD_LANDMARK_WEIGHT].registration.num_matches == len(p_mov)
    acc = [e.E for e in r.trail if e.level == 0 and e.accepted]
    assert all(b < a for a, b in zip(acc, acc[1:]))
    res = {}
    for lam, run in runs.items():
        f = run.refinement
        L = last_accepted([tuple(e) for e in f.trail], f.landmarks)[1].L
        res[lam] = np.sqrt(L)
        print("register_ffd(landmarks=True, landmark_weight=%g): %d landmarks, RMS landmark residual %.4g voxels, RMS "
              "field error %.4g voxels" % (lam, inl.sum(), res[lam], field_rms(f.field.cpu().numpy(), truth)))
    assert res[api.FFD_LANDMARK_WEIGHT] < res[0.0]
