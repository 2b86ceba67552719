"""CPU (not gpu): the similarity contract (include/sift3d_amd.h, "Similarity measures") without a device.  The numpy
restatement (tests/similarity_restatement.py) against analysis, the host entries sift3d_amd_similarity_measures and
sift3d_amd_label_overlap against the restatement, every argument refusal of the device entries (which check their
arguments before any device call), and the discriminating-power case of the GPU end-to-end test on the restatement.

Tolerances.  u = 2^-53, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, 3.1).
  - msd and ncc are a handful of IEEE operations (+, -, *, /, sqrt, all correctly rounded) on the same doubles in the
    same order in C and in numpy: equal bits are asserted.
  - An entropy is a recursive sum of k terms p log p, each formed by a division, a log and a product; C's log and
    numpy's may differ by an ulp, which counts as one more operation.  Two evaluations in the same order differ by at
    most 2 gamma_(k + 4) sum |p log p|: the k - 1 additions plus four operations per term, for each of the two.
  - mi = (H_f + H_m) - H_fm adds two more roundings on values no larger than H_f + H_m + H_fm, and the three
    entropies' own bounds; nmi = (H_f + H_m) / H_fm is a quotient, so the relative errors of numerator and
    denominator add, plus one rounding each."""
import ctypes as C

import numpy as np
import pytest

from tests import similarity_restatement as sr
from tests.test_warp import about_center, ref_warp, rot

U = 2.0 ** -53


def gamma(k):
    return k * U / (1 - k * U)


def entropy_terms(counts):
    """(number of non-zero terms, sum |p log p|)"""
    k = np.asarray(counts, np.float64).reshape(-1)
    k = k[k > 0]
    p = k / k.sum()
    return len(k), float(np.abs(p * np.log(p)).sum())


def entropy_bound(counts):
    k, t = entropy_terms(counts)
    return 2 * gamma(k + 4) * t


def measure_bounds(hist):
    """bounds on |C - restatement| for (entropy_fixed, entropy_moving, entropy_joint, mi, nmi)"""
    h = np.asarray(hist, np.float64)
    bf, bm, bj = entropy_bound(h.sum(1)), entropy_bound(h.sum(0)), entropy_bound(h)
    hf, hm, hj = (entropy_terms(c)[1] for c in (h.sum(1), h.sum(0), h))
    mi = bf + bm + bj + 2 * 2 * U * (hf + hm + hj)
    nmi = np.inf if hj == 0 else ((bf + bm + 2 * U * (hf + hm)) / max(hf + hm, 1e-300) + bj / hj + 2 * U) \
        * (hf + hm) / hj * 1.01                      # 1.01: the second-order terms of a quotient of perturbed values
    return bf, bm, bj, mi, nmi


def int_volume(shape, hi, seed):
    return np.random.default_rng(seed).integers(0, hi, shape).astype(np.float32)


# ---- the restatement against analysis ----------------------------------------------------------------------------
def test_bin_rule_edges():
    B, lo, hi = 50, -1.0, 4.0
    v = np.array([-1.0, 4.0, -3.0, 9.0, np.nextafter(np.float32(4.0), np.float32(0)), -0.9, 1.5], np.float32)
    np.testing.assert_array_equal(sr.bin_of(v, B, lo, hi), [0, 49, 0, 49, 49, 1, 25])
    assert sr.bin_scale(5, 0.0, 5.0) == 1.0                  # labels: s == 1 exactly
    np.testing.assert_array_equal(sr.bin_of(np.arange(-1, 7, dtype=np.float32), 5, 0.0, 5.0), [0, 0, 1, 2, 3, 4, 4, 4])


@pytest.mark.parametrize("bins", [2, 50, 64, 128])
def test_histogram_sums_to_count(bins):
    F = np.random.default_rng(bins).normal(0, 1, (5, 7, 9)).astype(np.float32)
    M = np.random.default_rng(bins + 1).normal(0, 1, (6, 5, 8)).astype(np.float32)
    A = about_center(rot((0, 0, 1), 20.0), M.shape, F.shape, shift=(0.5, 0.25, 0))
    hist, st = sr.joint(F, M, A, bins, (-1.0, 1.0), (-0.5, 2.0))
    assert int(hist.sum()) == st.count and 0 < st.count < F.size
    hist0, st0 = sr.joint(F, M, np.array([[1.0, 0, 0, 100], [0, 1, 0, 0], [0, 0, 1, 0]]), bins, (-1, 1), (-1, 1))
    assert st0.count == 0 and not hist0.any()
    assert all(np.isnan(v) for v in sr.measures(hist0, st0.count, st0.sums)[1:])


def test_mi_of_a_volume_with_itself_is_its_entropy():
    F = np.random.default_rng(3).normal(0, 1, (9, 10, 11)).astype(np.float32)
    m, hist = sr.similarity(F, F, None, 50)
    assert np.count_nonzero(hist - np.diag(np.diag(hist))) == 0
    bound = 3 * entropy_bound(hist.sum(1)) + 4 * U * 3 * m.entropy_fixed
    print("mi %.17g H_f %.17g bound %.3g" % (m.mi, m.entropy_fixed, bound))
    assert abs(m.mi - m.entropy_fixed) <= bound
    assert m.msd == 0.0 and m.n == F.size


@pytest.mark.parametrize("a,b", [(3.0, 7.0), (-2.0, 5.0)])
def test_ncc_of_an_affine_remap_is_plus_or_minus_one(a, b):
    """F integer-valued, M = a F + b exact in float32: every sum is an exact integer below 2^53.  vf, vm and the
    covariance are each x - (s t) / n: two roundings on y = s t / n and one on the difference, at most
    3 u max(|x|, |y|) absolute, rho relative to the value.  ncc = cov / sqrt(vf vm): rho_cov + (rho_vf + rho_vm + u) / 2
    for the product under the root, + u for the root, + u for the quotient (first order; 1.01 covers the rest)."""
    F = int_volume((6, 7, 8), 40, 1)
    M = (np.float32(a) * F + np.float32(b)).astype(np.float32)
    hist, st = sr.joint(F, M, None, 64, (0.0, 40.0), (float(M.min()), float(M.max())))
    s, n = st.sums, float(st.count)
    m = sr.measures(hist, st.count, s)

    def rho(x, y):
        return 3 * U * max(abs(x), abs(y)) / abs(x - y)
    bound = (rho(s[4], s[0] * s[1] / n) + 0.5 * (rho(s[2], s[0] * s[0] / n) + rho(s[3], s[1] * s[1] / n) + U)
             + 2 * U) * 1.01
    print("ncc %.17g bound %.3g" % (m.ncc, bound))
    assert abs(m.ncc - np.sign(a)) <= bound
    assert m.msd == float(((F - M).astype(np.float64) ** 2).sum()) / n


def test_mi_sees_through_a_bin_permutation_and_ncc_does_not():
    """M = perm[F] on integer levels 0 .. B-1 with s == 1: each row of the joint histogram has one non-zero column,
    so H_fm adds H_f's terms in H_f's order (equal bits) and mi = (H_f + H_m) - H_f differs from H_m by two roundings;
    H_m adds the same terms in the permuted order, within the recursive-sum bound of H_f.  A random permutation of 32
    levels has a correlation of standard deviation 1 / sqrt(31) = 0.18: |ncc| < 0.9 is five of them."""
    B = 32
    F = int_volume((8, 9, 10), B, 5)
    perm = np.random.default_rng(6).permutation(B).astype(np.float32)
    M = perm[F.astype(np.int64)]
    m, hist = sr.similarity(F, M, None, B, "nearest", (0.0, float(B)), (0.0, float(B)))
    assert m.entropy_joint == m.entropy_fixed
    bound = 2 * entropy_bound(hist.sum(1)) + 4 * U * 3 * m.entropy_fixed
    print("mi %.17g H_f %.17g ncc %.3f bound %.3g" % (m.mi, m.entropy_fixed, m.ncc, bound))
    assert abs(m.mi - m.entropy_fixed) <= bound
    assert abs(m.ncc) < 0.9
    same, _ = sr.similarity(F, F, None, B, "nearest", (0.0, float(B)), (0.0, float(B)))
    assert same.ncc > 1 - 1e-12 and abs(same.mi - m.mi) <= bound


def test_dice_of_identical_and_disjoint_labels():
    lab = int_volume((5, 6, 7), 4, 2)                           # labels 0 .. 3 of 5: label 4 is absent from both
    hist, _ = sr.joint(lab, lab, None, 5, (0.0, 5.0), (0.0, 5.0), "nearest")
    dice, jac, vf, vm = sr.label_overlap(hist)
    np.testing.assert_array_equal(dice[:4], 1.0)
    np.testing.assert_array_equal(jac[:4], 1.0)
    assert np.isnan(dice[4]) and np.isnan(jac[4])
    np.testing.assert_array_equal(vf, np.bincount(lab.astype(int).ravel(), minlength=5))
    np.testing.assert_array_equal(vm, vf)
    other = (lab + 1) % 4                                       # every voxel changes its label
    hist, _ = sr.joint(lab, other, None, 5, (0.0, 5.0), (0.0, 5.0), "nearest")
    dice, jac, _, _ = sr.label_overlap(hist)
    np.testing.assert_array_equal(dice[:4], 0.0)
    np.testing.assert_array_equal(jac[:4], 0.0)
    assert np.isnan(dice[4])


# ---- the host entries against the restatement ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def api():
    from sift3d_amd import api as a
    a.lib()
    return a


def random_hist(bins, seed):
    rng = np.random.default_rng(seed)
    h = rng.integers(0, 1000, (bins, bins)) * (rng.uniform(0, 1, (bins, bins)) < 0.4)
    h[bins // 2] = 0                                            # an empty row and an empty column
    h[:, 0] = 0
    h[bins - 1, bins - 1] = 2 ** 40                             # counts past 2^32
    return h.astype(np.uint64)


def random_stats(hist, seed):
    rng = np.random.default_rng(seed)
    n = int(hist.sum())
    f, m = rng.normal(3, 2, 4000), rng.normal(-1, 5, 4000)
    k = n / 4000.0
    return n, np.array([f.sum(), m.sum(), (f * f).sum(), (m * m).sum(), (f * m).sum(), ((f - m) ** 2).sum()]) * k


@pytest.mark.parametrize("bins", [2, 50, 128])
def test_measures_entry_equals_restatement(api, bins):
    hist = random_hist(bins, bins)
    n, sums = random_stats(hist, bins + 1)
    got = api.similarity_measures(hist, (n, sums))
    want = sr.measures(hist, n, sums)
    bf, bm, bj, bmi, bnmi = measure_bounds(hist)
    print("B %d: entropies %.6f %.6f %.6f mi %.6f nmi %.6f; bounds %.2g %.2g %.2g %.2g %.2g"
          % (bins, got.entropy_fixed, got.entropy_moving, got.entropy_joint, got.mi, got.nmi, bf, bm, bj, bmi, bnmi))
    assert got.count == n == want.n
    assert got.msd == want.msd and got.ncc == want.ncc        # IEEE operations only, same order: equal bits
    assert abs(got.entropy_fixed - want.entropy_fixed) <= bf
    assert abs(got.entropy_moving - want.entropy_moving) <= bm
    assert abs(got.entropy_joint - want.entropy_joint) <= bj
    assert abs(got.mi - want.mi) <= bmi
    assert abs(got.nmi - want.nmi) <= bnmi
    np.testing.assert_array_equal(got.joint, hist.astype(np.int64))


def test_measures_entry_edge_cases(api):
    z = np.zeros((4, 4), np.uint64)
    got = api.similarity_measures(z, (0, np.zeros(6)))
    assert got.count == 0 and all(np.isnan(v) for v in got[1:8])
    one = z.copy()
    one[1, 2] = 9                                               # one bin: every entropy 0, nmi 0; constant volumes: ncc 0
    got = api.similarity_measures(one, (9, np.array([18.0, 27.0, 36.0, 81.0, 54.0, 9.0])))
    assert (got.entropy_fixed, got.entropy_moving, got.entropy_joint, got.mi, got.nmi) == (0.0, 0.0, 0.0, 0.0, 0.0)
    assert got.ncc == 0.0 and got.msd == 1.0
    with pytest.raises(ValueError):
        api.similarity_measures(np.zeros((3, 4)), (0, np.zeros(6)))
    L = api.lib()
    rec, out = np.zeros(7), (C.c_double * 8)()
    raw = L["sift3d_amd_similarity_measures"]
    raw.restype, raw.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert raw(None, 4, rec.ctypes.data, out) == -1 and raw(z.ctypes.data, 4, None, out) == -1
    assert raw(z.ctypes.data, 4, rec.ctypes.data, None) == -1
    assert raw(z.ctypes.data, 1, rec.ctypes.data, out) == -1 and raw(z.ctypes.data, 129, rec.ctypes.data, out) == -1


@pytest.mark.parametrize("L", [2, 50, 128])
def test_label_overlap_entry_equals_restatement(api, L):
    hist = random_hist(L, 7 * L)
    got = api.label_overlap_measures(hist)
    dice, jac, vf, vm = sr.label_overlap(hist)
    np.testing.assert_array_equal(got.dice, dice)               # exact integers and one division: equal bits
    np.testing.assert_array_equal(got.jaccard, jac)
    np.testing.assert_array_equal(got.volume_fixed, vf)
    np.testing.assert_array_equal(got.volume_moving, vm)
    np.testing.assert_array_equal(got.confusion, hist.astype(np.int64))
    raw = api.lib()["sift3d_amd_label_overlap"]
    raw.restype, raw.argtypes = C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    assert raw(None, L, None, None, None, None) == -1
    assert raw(hist.ctypes.data, 0, None, None, None, None) == -1
    assert raw(hist.ctypes.data, 129, None, None, None, None) == -1
    assert raw(hist.ctypes.data, L, None, None, None, None) == 0          # every output is optional


# ---- the device entries refuse bad arguments before any device call --------------------------------------------
@pytest.fixture(scope="module")
def bufs(api):
    """made-up addresses without a device; real allocations covering every range named below with one"""
    from sift3d_amd import hip
    if api.device_available():
        b = [hip.lib().sift3d_hip_malloc(1 << 18) for _ in range(6)]
        assert all(b)
        yield b
        for p in b:
            hip.lib().sift3d_hip_free(p)
    else:
        yield [0x1000000 * (k + 1) for k in range(6)]


def _a(A):
    a = np.ascontiguousarray(A, np.float64).reshape(12)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def test_symbols_exported(api):
    from sift3d_amd import _native, hip
    L = _native.load()
    for name in ("sift3d_hip_similarity_affine", "sift3d_hip_similarity_field", "sift3d_amd_similarity_work_bytes",
                 "sift3d_amd_similarity_measures", "sift3d_amd_label_overlap"):
        assert hasattr(L, name), name
    assert callable(hip.similarity) and callable(api.similarity) and callable(api.label_overlap)
    W = hip.lib().sift3d_amd_similarity_work_bytes
    assert W(5, 6, 7, 64) == hip.SIMILARITY_GRID * 56 and W(5, 6, 7, 2) == W(512, 512, 512, 128)
    assert W(0, 6, 7, 64) == 0 and W(5, -1, 7, 64) == 0 and W(5, 6, 0, 64) == 0
    assert W(5, 6, 7, 1) == 0 and W(5, 6, 7, 129) == 0


def _refusal_cases(bufs, middle):
    """argument tuples for an entry whose transform argument(s) `middle(ok=True)` builds; the good call is
    (F, 8, 8, 8, M, 8, 8, 8, <transform>, interp, bins, lo_f, hi_f, lo_m, hi_m, hist, stats, work)"""
    F, M, T, H, S, W = bufs
    good = dict(F=F, o=(8, 8, 8), M=M, n=(8, 8, 8), interp=1, bins=64, rf=(0.0, 1.0), rm=(0.0, 1.0), H=H, S=S, W=W)

    def call(**kw):
        a = dict(good, **kw)
        return (a["F"], *a["o"], a["M"], *a["n"], a.get("T", T), a["interp"], a["bins"], *a["rf"], *a["rm"], a["H"],
                a["S"], a["W"])
    nan, inf = float("nan"), float("inf")
    cases = [call(F=None), call(M=None), call(T=None), call(H=None), call(S=None), call(W=None),
             call(o=(0, 8, 8)), call(o=(8, -1, 8)), call(o=(8, 8, 0)), call(n=(0, 8, 8)), call(n=(8, 8, -2)),
             call(bins=1), call(bins=0), call(bins=-4), call(bins=129),
             call(rf=(1.0, 1.0)), call(rf=(2.0, 1.0)), call(rm=(0.0, 0.0)), call(rm=(3.0, -3.0)),     # empty
             call(rf=(nan, 1.0)), call(rf=(0.0, nan)), call(rm=(-inf, 0.0)), call(rm=(0.0, inf)),     # not finite
             call(rf=(-3e38, 3e38)),                                     # hi - lo overflows
             call(rm=(0.0, 1e-44)),                                      # bins / (hi - lo) overflows
             call(interp=2), call(interp=-1),
             call(F=F + 2), call(M=M + 1), call(H=H + 4), call(S=S + 4), call(W=W + 4),               # misaligned
             call(H=F), call(H=M + 4 * 500), call(S=F + 4 * 100), call(W=M), call(W=F + 4 * 510),     # outputs on inputs
             call(S=H + 8 * 64 * 64 - 8), call(W=H + 8 * 100), call(S=W + 56 * 2047),                 # outputs on outputs
             call(o=(16, 16, 16), H=F + 4 * 4094)]                       # hist starts on the last two voxels of F
    return cases, call


def test_similarity_affine_refusals(bufs):
    from sift3d_amd import hip
    L = hip.lib()
    keep, ident = _a(np.eye(3, 4))
    cases, call = _refusal_cases(bufs, None)
    cases = [c[:8] + (ident if c[8] is not None else None,) + c[9:] for c in cases]
    for v in (np.nan, np.inf, -np.inf):
        for k in (0, 7, 11):
            A = np.eye(3, 4).reshape(12)
            A[k] = v
            kept, bad = _a(A)
            c = call()
            assert L.sift3d_hip_similarity_affine(*c[:8], bad, *c[9:], None) == -1, (v, k)
    for c in cases:
        assert L.sift3d_hip_similarity_affine(*c, None) == -1, c


def test_similarity_field_refusals(bufs):
    from sift3d_amd import hip
    L = hip.lib()
    F, M, T, H, S, W = bufs
    cases, call = _refusal_cases(bufs, None)
    cases += [call(T=T + 2),                                             # misaligned field
              call(H=T + 4 * 3 * 512 - 8), call(S=T), call(W=T + 4 * 1000)]     # outputs on the field
    for c in cases:
        assert L.sift3d_hip_similarity_field(*c, None) == -1, c


def test_python_value_errors(api):
    v = np.zeros((5, 7, 9), np.float32)
    with pytest.raises(ValueError):
        api.similarity(np.zeros((7, 9), np.float32), v)
    if not api.device_available():
        with pytest.raises(RuntimeError):
            api.similarity(v, v)
        with pytest.raises(RuntimeError):
            api.label_overlap(v, v)


# ---- the discriminating-power case of the GPU end-to-end test, on the restatement ---------------------------------
def end_to_end_case(api):
    """fixed = synth_survey(48); T = a rotation of 3 degrees about (1, 2, 3) through the centre plus a shift, the true
    pull map fixed -> moving; moving = fixed through T's inverse (linear), and its non-monotone remap |v - median|"""
    fixed = np.ascontiguousarray(api.synth_survey(48), np.float32)
    T = about_center(rot((1, 2, 3), 3.0), fixed.shape, fixed.shape, shift=(1.5, -1.0, 0.5))
    R = np.linalg.inv(T[:, :3])
    Tinv = np.hstack([R, (-R @ T[:, 3])[:, None]])
    return fixed, T, Tinv


def shifted(T, dx):
    S = np.array(T, np.float64)
    S[0, 3] += dx
    return S


def test_end_to_end_case_on_the_restatement(api):
    """What tests/test_similarity.py asserts on the device, first here: ncc and mi at the true transform exceed their
    values at the identity; with the remapped moving volume, mi over x shifts -3 .. 3 peaks at 0."""
    fixed, T, Tinv = end_to_end_case(api)
    moving = ref_warp(fixed, Tinv, fixed.shape, "linear", 0.0)[0].astype(np.float32)
    at_true, _ = sr.similarity(fixed, moving, T, 64)
    at_ident, _ = sr.similarity(fixed, moving, None, 64)
    print("true: ncc %.4f mi %.4f; identity: ncc %.4f mi %.4f" % (at_true.ncc, at_true.mi, at_ident.ncc, at_ident.mi))
    assert at_true.ncc > at_ident.ncc and at_true.mi > at_ident.mi
    remap = np.abs(moving - np.float32(np.median(moving))).astype(np.float32)
    rows = [sr.similarity(fixed, remap, shifted(T, dx), 64)[0] for dx in range(-3, 4)]
    mi, ncc = [r.mi for r in rows], [r.ncc for r in rows]
    print("remapped, dx -3 .. 3: mi", " ".join("%.4f" % v for v in mi), "ncc", " ".join("%.4f" % v for v in ncc))
    assert int(np.argmax(mi)) == 3
