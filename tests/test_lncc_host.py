"""CPU (not gpu): the host side of local cross-correlation (include/sift3d_amd.h, "Local cross-correlation") -- the
numpy restatement (tests/lncc_restatement.py) against analysis; the exported symbols and work sizes; the refusals of
the five C entries on made-up pointers (they check their arguments before any device call); the Python refusals and
the new keywords' defaults.

The error bounds.  u = 2^-53.  The six window sums are sums of at most N = (2r + 1)^3 exact products; where a test
needs them exact it uses small integer content, whose sums are integers below 2^53.  From exact sums
    A = sfw - fl(fl(sf sw) / n) has |dA| <= eA = u (2 |sf sw| / n + |A|)      (a product, a quotient, a difference)
and likewise eB, eC with sf sf and sw sw.  cc = fl(fl(A A) / fl(B C)) then has, to first order,
    |d cc| <= cc (eB / B + eC / C + 3 u) + 2 |A| eA / (B C).
_cc_bound returns twice that (the factor 2 covers the second-order terms: every relative term is below 2^-22, since a
counted voxel has B > 2^-30 sff >= 2^-30 sf sf / n).  The coefficients a = 2A / (BC) and b = 2 cc / C obey the same kind
of bound (_coef_bounds)."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import lncc_restatement as lr

F32 = np.float32
F64 = np.float64
U = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement against analysis ----------------------------------------------------------------------------------
def _abc(F, W, v, r):
    n, sf, sw, sff, sww, sfw = lr.sums(F, W, v, r)
    with np.errstate(divide="ignore", invalid="ignore"):
        A = sfw - (sf * sw) / n
        B = sff - (sf * sf) / n
        C = sww - (sw * sw) / n
        eA = U * (2.0 * np.abs(sf * sw) / n + np.abs(A))
        eB = U * (2.0 * sf * sf / n + np.abs(B))
        eC = U * (2.0 * sw * sw / n + np.abs(C))
    return A, B, C, eA, eB, eC


def _cc_bound(F, W, v, r):
    """the absolute error bound of cc per voxel (module docstring); meaningful on counted voxels"""
    A, B, C, eA, eB, eC = _abc(F, W, v, r)
    with np.errstate(divide="ignore", invalid="ignore"):
        cc = A * A / (B * C)
        return 2.0 * (cc * (eB / B + eC / C + 3.0 * U) + 2.0 * np.abs(A) * eA / (B * C))


def _coef_bounds(F, W, v, r):
    """absolute error bounds of a and b per voxel: a = 2A / (BC): |da| <= |a| (eB / B + eC / C + 3u) + 2 eA / (BC);
    b = 2 cc / C: |db| <= |b| (eC / C + 2u) + 2 dcc / C; both doubled as _cc_bound"""
    A, B, C, eA, eB, eC = _abc(F, W, v, r)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = 2.0 * A / (B * C)
        da = 2.0 * (np.abs(a) * (eB / B + eC / C + 3.0 * U) + 2.0 * eA / (B * C))
        dcc = _cc_bound(F, W, v, r)
        b = 2.0 * (A * A / (B * C)) / C
        db = 2.0 * (np.abs(b) * (eC / C + 2.0 * U) + 2.0 * dcc / C)
    return da, db


def _ints(shape, seed, lo=-300, hi=300):
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(F32)


def _valid(shape, seed, p=0.85):
    return np.random.default_rng(seed).random(shape) < p


SHAPE = (7, 9, 11)


@pytest.mark.parametrize("r", [1, 2, 4])
@pytest.mark.parametrize("alpha,beta", [(2.0, 3.0), (-0.5, -7.0)])
def test_affine_related_volumes_score_one(r, alpha, beta):
    """W = alpha F + beta exactly (integer F, dyadic alpha): cc = 1 on every counted voxel, of either sign of alpha"""
    F = _ints(SHAPE, 1)
    W = (F32(alpha) * F + F32(beta)).astype(F32)
    assert np.array_equal(W.astype(F64), alpha * F.astype(F64) + beta)
    v = _valid(SHAPE, 2)
    cc, _, counted = lr.stats(F, W, v, r)
    assert counted.sum() > 0.5 * v.sum()
    bound = _cc_bound(F, W, v, r)
    assert np.all(np.abs(cc[counted] - 1.0) <= bound[counted])
    assert bound[counted].max() < 1e-9
    assert not cc[~counted].any()


@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("side", ["fixed", "warped"])
def test_map_unchanged_under_gain_and_offset(r, side):
    F, W = _ints(SHAPE, 3), _ints(SHAPE, 4)
    v = _valid(SHAPE, 5)
    cc0, _, c0 = lr.stats(F, W, v, r)
    F2, W2 = (F32(4.0) * F - F32(9.0), W) if side == "fixed" else (F, F32(-0.25) * W + F32(5.0))
    cc1, _, c1 = lr.stats(F2, W2, v, r)
    assert np.array_equal(c0, c1) and c0.any()
    bound = _cc_bound(F, W, v, r) + _cc_bound(F2, W2, v, r)
    assert np.all(np.abs(cc1 - cc0)[c0] <= bound[c0])
    assert 0.0 < cc0[c0].max() <= 1.0 + 1e-12


@pytest.mark.parametrize("value", [0.0, 7.0, 0.1])
@pytest.mark.parametrize("which", ["F", "W"])
def test_constant_block_is_uncounted_and_finite(which, value):
    rng = np.random.default_rng(6)
    F = rng.normal(0, 1, (9, 10, 12)).astype(F32)
    W = rng.normal(0, 1, F.shape).astype(F32)
    (F if which == "F" else W)[:, :, :7] = F32(value)
    v = np.ones(F.shape, bool)
    r = 2
    cc, coef, counted = lr.stats(F, W, v, r)
    assert not counted[:, :, :5].any()                       # windows wholly inside the constant block
    assert counted[:, :, 7:].all()
    assert np.isfinite(cc).all() and np.isfinite(coef).all()
    assert not cc[:, :, :5].any() and not coef[:, :, :, :5].any()
    g = lr.gradient(F, W, v, coef, r)
    assert np.isfinite(g).all()


def test_a_valid_voxel_alone_in_its_window_is_uncounted():
    rng = np.random.default_rng(7)
    F = rng.normal(0, 1, (9, 9, 9)).astype(F32)
    W = rng.normal(0, 1, F.shape).astype(F32)
    v = np.zeros(F.shape, bool)
    v[4, 4, 4] = True
    n = lr.sums(F, W, v, 2)[0]
    assert n[4, 4, 4] == 1.0
    cc, coef, counted = lr.stats(F, W, v, 2)
    assert not counted.any() and not cc.any() and not coef.any()
    v[4, 4, 7] = True                                        # a second one, out of reach at r = 2, in reach at r = 4
    assert not lr.stats(F, W, v, 2)[2].any()
    assert lr.stats(F, W, v, 4)[2].sum() == 2


def _window(q, r, shape):
    return tuple(slice(max(0, c - r), min(n, c + r + 1)) for c, n in zip(q, shape))


@pytest.mark.parametrize("r", [1, 2])
def test_gradient_agrees_with_central_differences(r):
    """g(q) against (S(W + h e_q) - S(W - h e_q)) / 2h of the restatement's own S = sum_p cc(p), at h = 2^-6 and h / 2,
    validity held fixed.  W lies on the grid 2^-10 Z, so W +- h is exact in float32.  The bound:
        |g - fd(h / 2)| <= |fd(h) - fd(h / 2)| + floor
    (the truncation error of fd(h / 2) is a third of the first term to leading order).  The floor is rounding alone:
    each S is a sum over the window of q, S+ - S- has error at most the cc bounds of both evaluations (_cc_bound) plus
    gamma_N (S+ + S-) of the summation, all over 2 (h / 2); g adds, per term of its defining sum over p in N(q), the
    coefficient bounds (_coef_bounds) times |F(q) - mf(p)| and |W(q) - mw(p)|, and gamma_(3 w + 6) of the sum of the
    absolute terms for the box sums and the final grouping."""
    shape = (8, 9, 10)
    rng = np.random.default_rng(10 + r)
    F = rng.normal(0, 1, shape).astype(F32)
    W = (np.round(rng.normal(0, 1, shape) * 1024.0) / 1024.0).astype(F32)
    v = _valid(shape, 11)
    cc, coef, counted = lr.stats(F, W, v, r)
    g = lr.gradient(F, W, v, coef, r)
    da, db = _coef_bounds(F, W, v, r)
    n, sf, sw = lr.sums(F, W, v, r)[:3]
    N = (2 * r + 1) ** 3
    h = 2.0 ** -6
    picks = [(0, 0, 0), (7, 8, 9), (4, 4, 5), (3, 0, 9), (2, 5, 1), (6, 7, 3)]
    picks = [q for q in picks if v[q]]
    assert len(picks) >= 4
    worst = 0.0
    for q in picks:
        win = _window(q, r, shape)

        def S(step):
            Wp = W.copy()
            Wp[q] = F32(float(W[q]) + step)
            assert float(Wp[q]) == float(W[q]) + step
            c, _, cnt = lr.stats(F, Wp, v, r)
            assert np.array_equal(cnt[win], counted[win])   # the counted set does not move
            return float(np.sum(c[win], dtype=F64)), float(np.sum(_cc_bound(F, Wp, v, r)[win][cnt[win]]))

        fd, err = [], []
        for hh in (h, h / 2):
            sp, ep = S(hh)
            sm, em = S(-hh)
            fd.append((sp - sm) / (2 * hh))
            err.append((ep + em + lr.gamma(N) * (sp + sm)) / (2 * hh))
        cw = counted[win]
        with np.errstate(divide="ignore", invalid="ignore"):
            mf, mw = (sf / n)[win], (sw / n)[win]
        a, am, b, bm = (c[win] for c in coef)
        fq, wq = float(F[q]), float(W[q])
        terms = np.abs(a) * abs(fq) + np.abs(am) + np.abs(b) * abs(wq) + np.abs(bm)
        floor_g = float(np.sum((da[win] * np.abs(fq - mf) + db[win] * np.abs(wq - mw))[cw])
                        + lr.gamma(3 * (2 * r + 1) + 6) * np.sum(terms[cw]))
        bound = abs(fd[0] - fd[1]) + err[1] + floor_g
        print("r %d q %s: g %.12g fd(h) %.12g fd(h/2) %.12g bound %.3g (rounding floor %.3g)"
              % (r, q, g[q], fd[0], fd[1], bound, err[1] + floor_g))
        assert abs(g[q] - fd[1]) <= bound, (q, g[q], fd, bound)
        assert bound <= 1e-3 * max(1.0, abs(g[q]))          # the comparison means something
        worst = max(worst, abs(g[q]))
    assert worst > 1e-3
    assert not g[~v].any()


def test_normalize_restated():
    rng = np.random.default_rng(12)
    phi = rng.normal(0, 3, (3, 4, 5, 6)).astype(F32)
    out = lr.ref_normalize(phi, 0.5)
    m = np.sqrt((out.astype(F64) ** 2).sum(0)).max()
    assert abs(m - 0.5) <= 0.5 * 4 * 2.0 ** -24
    z = np.zeros_like(phi)
    z[0, 0, 0, 0] = -0.0
    assert np.array_equal(lr.ref_normalize(z, 0.5).view(np.uint32), z.view(np.uint32))


# ---- symbols, sizes -----------------------------------------------------------------------------------------------------
EXPORTED = ["sift3d_amd_lncc_work_bytes", "sift3d_hip_lncc", "sift3d_hip_lncc_force", "sift3d_hip_field_normalize",
            "sift3d_amd_demons_lncc_work_floats", "sift3d_amd_demons_lncc_device"]


@pytest.fixture(scope="module")
def api():
    from sift3d_amd import api as a
    a.lib()
    return a


def _header():
    with open(os.path.join(ROOT, "include", "sift3d_amd.h")) as f:
        return f.read()


def _define(name):
    return int(re.search(r"#define %s (\d+)" % name, _header()).group(1))


def test_symbols_exported_and_declared(api):
    from sift3d_amd import _native, hip
    L = _native.load()
    text = _header()
    assert "Local cross-correlation" in text
    for name in EXPORTED:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\(" % name, text), name
    hip.lib()
    for fn in ("lncc", "lncc_force", "field_normalize", "demons_lncc"):
        assert callable(getattr(hip, fn))
    assert hip.LNCC_MAX_RADIUS == _define("SIFT3D_AMD_LNCC_MAX_RADIUS") == api.LNCC_MAX_RADIUS == lr.MAX_RADIUS == 4
    assert hip.FIELD_NORMALIZE_WORK_BYTES == _define("SIFT3D_AMD_FIELD_NORMALIZE_WORK_BYTES")


def _pad4(x):
    return (x + 3) & ~3


def test_work_sizes_agree():
    from sift3d_amd import hip
    L = hip.lib()
    part = _define("SIFT3D_AMD_LNCC_PARTIAL_BYTES")
    head = (part + _define("SIFT3D_AMD_FIELD_NORMALIZE_WORK_BYTES")) // 4
    assert head == 12292
    for nx, ny, nz in ((8, 8, 8), (5, 3, 7), (1, 1, 1), (70, 11, 9)):
        n = nx * ny * nz
        assert L.sift3d_amd_lncc_work_bytes(nx, ny, nz) == part + ((4 * n + 7) & ~7)
        for update in (0, 1):
            for levels in (1, 2, 3):
                want, dims = _pad4(head + (15 + 6 * update) * n), (nx, ny, nz)
                for _ in range(1, levels):
                    dims = tuple((d + 1) // 2 for d in dims)
                    want += _pad4(3 * dims[0] * dims[1] * dims[2])
                assert L.sift3d_amd_demons_lncc_work_floats(nx, ny, nz, update, levels) == want
    for bad in ((0, 8, 8, 0, 1), (8, 8, 8, 2, 1), (8, 8, 8, 0, 0), (8, 8, 8, 0, 7), (8, -1, 8, 1, 1)):
        assert L.sift3d_amd_demons_lncc_work_floats(*bad) == 0
    assert L.sift3d_amd_lncc_work_bytes(0, 1, 1) == 0 and L.sift3d_amd_lncc_work_bytes(1, 1, -2) == 0


# ---- the C entries' refusals -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bufs(api):
    """made-up addresses without a device; real allocations covering every range named below with one, so that a
    regressed check could not make a kernel touch unmapped memory"""
    from sift3d_amd import hip
    if api.device_available():
        b = [hip.lib().sift3d_hip_malloc(1 << 18) for _ in range(3)]
        assert all(b)
        yield b
        for p in b:
            hip.lib().sift3d_hip_free(p)
    else:
        yield [0x1000000, 0x2000000, 0x3000000]


VB = 512 * 4                                                # an 8^3 volume: 2048 bytes
INF, NAN = float("inf"), float("nan")


def _stats(L, a):
    return L.sift3d_hip_lncc(a["F"], a["nx"], a["ny"], a["nz"], a["W"], a["u"], a["mx"], a["my"], a["mz"], a["WF"],
                             a["WM"], a["r"], a["cc"], a["coef"], a["stats"], a["work"], None)


def _force(L, a):
    return L.sift3d_hip_lncc_force(a["F"], a["nx"], a["ny"], a["nz"], a["W"], a["u"], a["mx"], a["my"], a["mz"],
                                   a["WF"], a["WM"], a["r"], a["coef"], a["force"], a["work"], None)


def _all_refused(run, L, base, changes):
    for ch in changes:
        a = dict(base)
        a.update(ch)
        assert run(L, a) == -1, ch


def test_statistics_refusals(bufs):
    """F, W, u and the masks in buffer 0; cc, stats and coef in 1; the work buffer (34816 bytes) in 2 (8^3)"""
    from sift3d_amd import hip
    L = hip.lib()
    A, B, W = bufs
    assert L.sift3d_amd_lncc_work_bytes(8, 8, 8) == 34816
    base = dict(F=A, nx=8, ny=8, nz=8, W=A + 8192, u=A + 16384, mx=8, my=8, mz=8, WF=A + 32768, WM=A + 40960, r=2,
                cc=B, stats=B + 8192, coef=B + 16384, work=W)
    _all_refused(_stats, L, base, [
        dict(F=None), dict(W=None), dict(u=None), dict(stats=None), dict(work=None),
        dict(nx=0), dict(ny=-1), dict(nz=0), dict(mx=0), dict(my=0), dict(mz=-3),
        dict(r=0), dict(r=5), dict(r=-1),
        # misalignment: floats 4 bytes; doubles, the record and the work buffer 8
        dict(F=A + 2), dict(W=A + 8193), dict(u=A + 16386), dict(cc=B + 1), dict(coef=B + 16388), dict(stats=B + 8196),
        dict(work=W + 4), dict(WF=A + 32770), dict(WM=A + 40961), dict(WF=None, WM=A + 40962),
        # an output over an input
        dict(cc=A), dict(cc=A + 8192 + VB - 4), dict(cc=A + 16384 + 3 * VB - 4), dict(coef=A), dict(coef=A + 16384 - 8),
        dict(stats=A + 8), dict(stats=A + 16384 + 3 * VB - 8), dict(work=A), dict(work=A + 16384 - 34816 + 8),
        # an output over a mask
        dict(WF=B), dict(WM=B + VB - 4), dict(WF=B + 8192), dict(WM=B + 16384 + 4 * 4096 - 4), dict(WF=W + 34816 - 4),
        dict(WF=None, WM=W + 4 * 100),
        # an output over another output, or over the work buffer
        dict(cc=B + 8192 - VB + 4), dict(cc=B + 16384 + 8), dict(coef=B + 8), dict(coef=B + 8192 - 16384 + 8),
        dict(stats=B), dict(stats=B + 16384 + 16376), dict(cc=W + 34816 - 4), dict(coef=W + 32768), dict(stats=W + 8),
        # the optional outputs are checked when given, whichever is left out
        dict(cc=None, coef=A), dict(coef=None, cc=A + 8192), dict(cc=None, coef=None, stats=A),
        dict(cc=None, coef=None, work=A + 8),
        # the moving mask has ITS grid's size
        dict(mx=16, my=16, mz=16, WM=B - 8 * VB + 4),
    ])


def test_force_refusals(bufs):
    """F, W, u, the masks and coef in buffer 0; the force in 1; the work buffer in 2 (8^3)"""
    from sift3d_amd import hip
    L = hip.lib()
    A, B, W = bufs
    base = dict(F=A, nx=8, ny=8, nz=8, W=A + 8192, u=A + 16384, mx=8, my=8, mz=8, WF=A + 32768, WM=A + 40960, r=1,
                coef=A + 65536, force=B, work=W)
    _all_refused(_force, L, base, [
        dict(F=None), dict(W=None), dict(u=None), dict(coef=None), dict(force=None), dict(work=None),
        dict(nx=0), dict(nz=-1), dict(my=0), dict(r=0), dict(r=5),
        dict(F=A + 1), dict(u=A + 16386), dict(coef=A + 65540), dict(force=B + 2), dict(work=W + 4),
        dict(WF=A + 32769), dict(WM=A + 40962),
        dict(force=A), dict(force=A + 8192 + VB - 4), dict(force=A + 16384 - 3 * VB + 4), dict(force=A + 65536 + 16380),
        dict(force=A + 65536 - 3 * VB + 4), dict(work=A + 65536), dict(work=A + 8192),
        dict(force=W), dict(force=W + 34816 - 4), dict(work=B + 3 * VB - 8), dict(work=B - 34816 + 8),
        dict(WF=B), dict(WM=B + 3 * VB - 4), dict(WF=W + 8), dict(WF=None, WM=W + 34812),
    ])


def test_field_normalize_refusals(bufs):
    from sift3d_amd import hip
    L = hip.lib()
    A, B, W = bufs
    nb = hip.FIELD_NORMALIZE_WORK_BYTES

    def run(L, a):
        return L.sift3d_hip_field_normalize(a["f"], a["nx"], a["ny"], a["nz"], a["step"], a["work"], None)

    base = dict(f=B, nx=8, ny=8, nz=8, step=0.5, work=W)
    _all_refused(run, L, base, [
        dict(f=None), dict(work=None), dict(nx=0), dict(ny=0), dict(nz=-1),
        dict(step=0.0), dict(step=-0.5), dict(step=INF), dict(step=NAN),
        dict(f=B + 2), dict(work=W + 4),
        dict(work=B), dict(work=B + 3 * VB - 8), dict(work=B - nb + 8), dict(f=W + nb - 4), dict(f=W - 3 * VB + 4),
    ])


def _levels(hip, *rows):
    tab = (hip.DemonsLevel * len(rows))()
    for l, r in enumerate(rows):
        tab[l] = hip.DemonsLevel(*r)
    return tab


def _masks(hip, *rows):
    tab = (hip.DemonsLevelMasks * len(rows))()
    for l, r in enumerate(rows):
        tab[l] = hip.DemonsLevelMasks(*r)
    return tab


def _drv(L, a):
    return L.sift3d_amd_demons_lncc_device(a["tab"], a["masks"], a["levels"], a["r"], a["u"], a["step"], a["sf"],
                                           a["sd"], a["update"], a["K"], a["work"], a["stats"], None)


@pytest.mark.parametrize("update", [0, 1])
def test_driver_refusals(bufs, update):
    """F, M and the masks in buffer 0, u and the statistics in 1, the work buffer in 2 (8^3)"""
    from sift3d_amd import hip
    L = hip.lib()
    A, B, W = bufs
    M, WF, WM = A + 8192, A + 32768, A + 40960
    floats = L.sift3d_amd_demons_lncc_work_floats(8, 8, 8, update, 1)
    assert 0 < 4 * floats < (1 << 18)

    def lv(**ch):
        r = dict(F=A, nx=8, ny=8, nz=8, M=M, mx=8, my=8, mz=8, it=3)
        r.update(ch)
        return _levels(hip, (r["F"], r["nx"], r["ny"], r["nz"], r["M"], r["mx"], r["my"], r["mz"], r["it"]))

    base = dict(tab=lv(), masks=_masks(hip, (WF, WM)), levels=1, r=2, u=B, step=0.5, sf=1.0, sd=1.0, update=update,
                K=2, work=W, stats=B + 8192)
    two = _levels(hip, (A, 8, 8, 8, M, 8, 8, 8, 1), (A, 5, 4, 4, M, 4, 4, 4, 1))
    _all_refused(_drv, L, base, [
        dict(tab=None), dict(u=None), dict(work=None), dict(stats=None), dict(levels=0), dict(levels=7),
        dict(tab=lv(F=None)), dict(tab=lv(M=None)), dict(tab=lv(nx=0)), dict(tab=lv(mz=0)), dict(tab=lv(it=-1)),
        dict(r=0), dict(r=5), dict(step=0.0), dict(step=-1.0), dict(step=INF), dict(step=NAN),
        dict(sf=-0.1), dict(sd=INF), dict(sf=NAN), dict(K=-1), dict(K=21), dict(update=2), dict(update=-1),
        dict(u=B + 2), dict(tab=lv(F=A + 1)), dict(tab=lv(M=M + 2)), dict(work=W + 4), dict(stats=B + 8196),
        dict(u=A + 4 * 300), dict(u=M - 3 * VB + 4), dict(work=B), dict(work=A + 8), dict(stats=B + 4 * 1000),
        dict(stats=A + VB - 8), dict(stats=W + 4 * floats - 8), dict(u=W + 4 * floats - 4),
        dict(masks=None, tab=None), dict(masks=None, u=A + 4 * 300), dict(masks=None, levels=7), dict(masks=None, r=9),
        dict(levels=2, tab=two, masks=_masks(hip, (WF, WM), (None, None))), dict(levels=2, tab=two, masks=None),
        dict(masks=_masks(hip, (WF + 2, WM))), dict(masks=_masks(hip, (WF, WM + 1))),
        dict(masks=_masks(hip, (None, WM + 3))), dict(masks=_masks(hip, (WF + 1, None))),
        dict(masks=_masks(hip, (B, WM))), dict(masks=_masks(hip, (WF, B + 4 * 1535))),
        dict(masks=_masks(hip, (B - VB + 4, None))),
        dict(masks=_masks(hip, (B + 8192, WM))), dict(masks=_masks(hip, (WF, B + 8192 + 16 * 3 - 4))),
        dict(masks=_masks(hip, (W, WM))), dict(masks=_masks(hip, (None, W + 4 * floats - 4))),
        dict(masks=_masks(hip, (W + 4 * 9000, None))),
    ])
    ok2 = _levels(hip, (A, 8, 8, 8, M, 8, 8, 8, 1), (A, 4, 4, 4, M, 4, 4, 4, 1))
    floats2 = L.sift3d_amd_demons_lncc_work_floats(8, 8, 8, update, 2)
    for m in (_masks(hip, (WF, WM), (B + 4 * 100, None)), _masks(hip, (None, None), (None, W + 4 * floats2 - 4)),
              _masks(hip, (None, None), (WF + 2, None))):
        a = dict(base)
        a.update(levels=2, tab=ok2, masks=m)
        assert _drv(L, a) == -1


# ---- the Python layer ------------------------------------------------------------------------------------------------
def test_python_refusals(api):
    from sift3d_amd import hip
    vol = np.zeros((5, 6, 7), F32)
    fld = np.zeros((3, 5, 6, 7), F32)
    kw = dict(force="lncc", features="intensity")
    with pytest.raises(ValueError, match="force must be 'demons' or 'lncc'"):
        api.refine_field(vol, vol, force="ncc")
    with pytest.raises(ValueError, match="needs features 'intensity'"):
        api.refine_field(vol, vol, force="lncc")
    for upd in ("logdomain", "symmetric", "other"):
        with pytest.raises(ValueError, match="needs update 'additive' or 'diffeomorphic'"):
            api.refine_field(vol, vol, update=upd, **kw)
    for r in (0, 5, -1, 2.0, 2.5, None, True):
        with pytest.raises(ValueError, match="radius must be an integer in 1 .. 4"):
            api.refine_field(vol, vol, radius=r, **kw)
        with pytest.raises(ValueError, match="radius must be an integer in 1 .. 4"):
            api.local_ncc(vol, vol, radius=r)
    for s in (0.0, -0.5, INF, NAN, None, "0.5"):
        with pytest.raises(ValueError, match="step must be positive and finite"):
            api.refine_field(vol, vol, step=s, **kw)
    with pytest.raises(ValueError, match="mask_fixed must have its volume's shape"):
        api.refine_field(vol, vol, mask_fixed=np.ones((5, 6, 8), bool), **kw)
    with pytest.raises(ValueError, match="mask_moving must have its volume's shape"):
        api.local_ncc(vol, vol, mask_moving=np.ones((4, 6, 7), F32))
    with pytest.raises(ValueError, match="bool, integer or float"):
        api.local_ncc(vol, vol, mask_fixed=np.ones((5, 6, 7), np.complex64))
    with pytest.raises(ValueError, match="must have one shape"):
        api.local_ncc(vol, np.zeros((5, 6, 8), F32))
    # force "demons" does not read the new keywords: what it refuses is what it refused
    with pytest.raises(ValueError, match="moving must be a contiguous float32 CUDA tensor"):
        api.refine_field(vol, vol, radius=99, step=-1.0)
    with pytest.raises(ValueError, match="radius must be an integer"):
        hip.demons_lncc([vol], [vol], fld, [1], radius=7)
    with pytest.raises(ValueError, match="step must be positive and finite"):
        hip.demons_lncc([vol], [vol], fld, [1], step=0.0)
    with pytest.raises(ValueError, match="update must be"):
        hip.demons_lncc([vol], [vol], fld, [1], update="logdomain")
    with pytest.raises(ValueError, match="per level"):
        hip.demons_lncc([vol], [vol], fld, [1], masks_fixed=[None, None])
    with pytest.raises(ValueError, match="step must be positive and finite"):
        hip.field_normalize(fld, -1.0)
    # the hip wrappers refuse a wrong type as they refuse a wrong value
    for r in (None, 2.0, True, "2"):
        with pytest.raises(ValueError, match="radius must be an integer"):
            hip.demons_lncc([vol], [vol], fld, [1], radius=r)
    for s in (None, "0.5", True):
        with pytest.raises(ValueError, match="step must be positive and finite"):
            hip.demons_lncc([vol], [vol], fld, [1], step=s)
        with pytest.raises(ValueError, match="step must be positive and finite"):
            hip.field_normalize(fld, s)


REFINE_FIELD_BEFORE = ["moving", "fixed", "field", "iterations", "alpha", "sigma_fluid", "sigma_diffusion", "features",
                       "sigma", "update", "squarings", "levels", "level_iterations", "velocity", "bch", "max_motion",
                       "velocity_squarings", "mask_fixed", "mask_moving"]


def test_keyword_defaults_and_positions(api):
    from sift3d_amd import hip
    par = inspect.signature(api.refine_field).parameters
    names = list(par)
    assert names[:len(REFINE_FIELD_BEFORE)] == REFINE_FIELD_BEFORE
    assert names[len(REFINE_FIELD_BEFORE):] == ["force", "radius", "step"]
    assert (par["force"].default, par["radius"].default, par["step"].default) == ("demons", 2, 0.5)
    assert par["features"].default == "descriptors" and par["update"].default == "additive"
    par = inspect.signature(api.register_dense).parameters
    assert (par["force"].default, par["radius"].default, par["step"].default) == ("demons", 2, 0.5)
    assert list(par)[-1] == "deformable_kw" and list(par)[:5] == ["moving", "fixed", "iterations", "alpha", "sigma_fluid"]
    par = inspect.signature(api.local_ncc).parameters
    assert list(par) == ["fixed", "moving", "transform", "radius", "mask_fixed", "mask_moving", "return_map"]
    assert [par[k].default for k in list(par)[2:]] == [None, 2, None, None, False]
    assert api.LocalNcc._fields == ("value", "count", "map")
    assert api.LnccRefinement._fields == ("field", "warped", "lncc", "jacobian")
    assert api.MultiresLnccRefinement._fields == api.LnccRefinement._fields + ("level_slices",)
    assert api.LnccRegistration._fields == tuple("lncc" if f == "msd" else f for f in api.DenseRegistration._fields)
    assert api.MultiresLnccRegistration._fields == api.LnccRegistration._fields + ("level_slices",)
    par = inspect.signature(hip.demons_lncc).parameters
    assert (par["radius"].default, par["step"].default, par["work"].default) == (2, 0.5, None)
    for fn in (hip.lncc, hip.lncc_force, hip.field_normalize):
        assert inspect.signature(fn).parameters["work"].default is None
