"""CPU (not gpu): "Mutual-information free-form deformation (Mattes)" (include/sift3d_amd.h) without a device.  The
restatement (tests/ffd_mi_restatement.py) against a finite difference of its own cost, its driver on the pair that
tests/test_ffd_mi.py runs on the device (a known smooth field under a non-monotone intensity map, where the MSD driver
moves away from the truth), the exported symbols and sizes, and every argument refusal of the three device entries,
which check their arguments before any device call."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import ffd_mi_restatement as fm
from tests import ffd_restatement as fr
from tests.field_restatement import ref_jacobian_det
from tests.test_affine_mi_host import BAD_BINS_AND_RANGES, MAPS, source
from tests.test_ffd_host import BAD_A, _a, known_displacement

DRIVER = dict(spacing=8, levels=2, bending=0.005, max_evaluations=12, bins=32)


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


# ---- the driver pair ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def driver_pair():
    """(fixed, moving, plain, truth): S = tests.test_affine_mi_host.source() (56^3, a sum of Gaussians, maximum 100);
    fixed = S[4:52]^3; plain(p) = S sampled (ffd_restatement.sample_grad) at p + 4 + w(p), w the known displacement of
    tests/test_ffd_host.py (amplitude 2, so no sample leaves S); moving = the hump map of plain, which is not monotone;
    truth = the u with fixed(p) = plain(p + u(p)), that is u + w(p + u) = 0, by fixed-point iteration on the analytic
    w."""
    S = source()
    m = 48
    fixed = np.ascontiguousarray(S[4:52, 4:52, 4:52])
    w = known_displacement((m, m, m))
    plain, _, _, _, ins = fr.sample_grad(S, (w + 4.0).astype(np.float32))
    assert ins.all()
    moving = np.ascontiguousarray(MAPS["hump"](plain).astype(np.float32))

    def w_at(q):                                                         # analytic, crop coordinates (x, y, z)
        return 2.0 * np.stack([np.sin(2 * np.pi * q[1] / m), np.sin(2 * np.pi * q[2] / m),
                               np.sin(2 * np.pi * q[0] / m)])
    z, y, x = np.meshgrid(*(np.arange(m, dtype=np.float64),) * 3, indexing="ij")
    p = np.stack([x, y, z])
    u = np.zeros_like(p)
    for _ in range(60):
        u = -w_at(p + u)
    assert np.abs(u + w_at(p + u)).max() < 1e-9
    return fixed, moving, np.ascontiguousarray(plain), u


def rms_error(fld, truth):
    """RMS field error over the voxels 4 away from every face"""
    inner = (slice(None),) + (slice(4, -4),) * 3
    return float(np.sqrt(((np.asarray(fld, np.float64) - truth)[inner] ** 2).sum(axis=0).mean()))


def level0_gain(trail):
    """mi gained on level 0: -(last accepted -mi) - -(first -mi)"""
    es = [e for e in trail if e[6] == 0]
    return es[0][1] - [e for e in es if e[5]][-1][1]


@functools.lru_cache(maxsize=None)
def restatement_driver():
    fixed, moving, _, truth = driver_pair()
    r = fm.refine(fixed, moving, None, DRIVER["spacing"], DRIVER["levels"], DRIVER["bending"],
                  DRIVER["max_evaluations"], DRIVER["bins"])
    return r, rms_error(r.field, truth)


def check_trail(trail, levels, max_evaluations, bending):
    """tests/test_ffd_host.py's conventions with E = -mi + bending R"""
    lv = [e[6] for e in trail]
    assert lv == sorted(lv, reverse=True) and set(lv) == set(range(levels))
    for l in range(levels):
        es = [e for e in trail if e[6] == l]
        assert 1 <= len(es) <= max_evaluations and es[0][5] and es[0][4] == 1.0
        acc = [e[0] for e in es if e[5]]
        assert all(b < a for a, b in zip(acc, acc[1:]))
        for a, b in zip(es[1:], es[2:]):
            assert b[4] == (min(2 * a[4], 4.0) if a[5] else a[4] / 2)
        for e in es:
            assert abs(e[0] - (e[1] + bending * e[2])) <= 1e-12 * abs(e[0]) and e[3] > 0


# ---- conditions on the pair and the restatement ------------------------------------------------------------------
def test_restatement_driver_recovers_the_field_under_the_hump_map():
    """Conditions, not measurements: the driver ends with RMS field error <= 0.3 x the start's (the start is the zero
    field, whose error is the truth's own RMS), its accepted costs fall strictly per level and the field has no fold.
    A float64 prototype of this composition measured 0.556 against 2.629 (0.21 x)."""
    fixed, moving, _, truth = driver_pair()
    r, rms = restatement_driver()
    start = rms_error(np.zeros_like(truth), truth)
    print("mi restatement driver: stop %s, %d evaluations, RMS %.4g against %.4g at the start, mi gain %.4g"
          % (r.stop, len(r.trail), rms, start, level0_gain(r.trail)))
    check_trail(r.trail, DRIVER["levels"], DRIVER["max_evaluations"], DRIVER["bending"])
    assert r.stop in fr.STOPS
    assert rms <= 0.3 * start
    assert ref_jacobian_det(r.field).min() > 0
    last = [e for e in r.trail if e[6] == 0 and e[5]][-1]
    assert last[1] == -r.measures.mi


def test_the_pair_needs_the_metric():
    """The MSD restatement driver on the same pair and budget ends no nearer the truth than it started (a prototype
    measured 14.7 voxels against 2.63): the hump map makes the squared difference the wrong cost, not a weak one."""
    fixed, moving, _, truth = driver_pair()
    r = fr.refine(fixed, moving, None, DRIVER["spacing"], DRIVER["levels"], DRIVER["bending"],
                  DRIVER["max_evaluations"])
    start = rms_error(np.zeros_like(truth), truth)
    rms = rms_error(r.field, truth)
    print("msd restatement driver on the hump pair: RMS %.4g against %.4g at the start" % (rms, start))
    assert rms >= start


# ---- the gradient against a finite difference of the cost ---------------------------------------------------------
def test_gradient_is_the_finite_difference_of_the_cost():
    """The restatement's cost -mi (bending 0) along d = grad / gmax by central differences with h = 0.125, at a random
    lattice of amplitude 0.7 (not the zero lattice: at grid-aligned samples MI with linear interpolation has its known
    interpolation artefact, and a prototype's quotient there was 0.79 - 0.97 depending on h; at the random lattice it
    was 0.987 - 0.989 for h from 0.0625 to 0.25).  The quotient numeric / analytic must be within 5 % of 1; a wrong
    sign, or a missing s_m, 1 / n or psi factor, is off by 2 x or more."""
    fixed, moving, _, _ = driver_pair()
    spacing, bins, h = 8, 32, 0.125
    ranges = (fm.own_range(fixed), fm.own_range(moving))
    rng = np.random.default_rng(17)
    c = rng.uniform(-0.7, 0.7, fr.lattice_shape(fixed.shape, spacing)).astype(np.float32)
    _, n, me = fm.cost_at(fixed, moving, c, spacing, None, bins, ranges)
    rec, _ = fm.evaluate(fixed, moving, c, spacing, None, me.W, bins, ranges, exact=False)
    assert rec.n == n and 0.9 * fixed.size < n <= fixed.size          # the random lattice pushes a few samples out
    g = rec.Gc / n
    d = g / np.abs(g).max()
    analytic = float((g * d).sum())
    side = []
    for sgn in (1.0, -1.0):
        E, nn, _ = fm.cost_at(fixed, moving, (c + sgn * h * d).astype(np.float32), spacing, None, bins, ranges)
        print("count at %+g h: %d (%d at the centre)" % (sgn, nn, n))
        side.append(E)
    numeric = (side[0] - side[1]) / (2 * h)
    print("directional derivative: analytic %.6g, central difference %.6g, quotient %.4f"
          % (analytic, numeric, numeric / analytic))
    assert analytic > 0 and abs(numeric / analytic - 1.0) <= 0.05
    g32, gmax = fm.gradient(rec, np.zeros_like(rec.Gc), 0.0)
    assert np.array_equal(g32, g.astype(np.float32)) and gmax == float(np.abs(g32).max())


# ---- the library without a device --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bufs():
    """made-up addresses without a device; real allocations covering every range named below with one"""
    from sift3d_amd import api, hip
    if api.device_available():
        b = [hip.lib().sift3d_hip_malloc(1 << 22) for _ in range(8)]
        assert all(b)
        yield b
        for p in b:
            hip.lib().sift3d_hip_free(p)
    else:
        yield [0x10000000 * (k + 1) for k in range(8)]


def test_symbols_exported_and_sizes_agree(hip):
    from sift3d_amd import _native, api
    L = _native.load()
    for name in ("sift3d_hip_parzen_hist_field", "sift3d_hip_ffd_mi_evaluate", "sift3d_amd_ffd_mi_refine_work_bytes",
                 "sift3d_amd_ffd_mi_refine_device"):
        assert hasattr(L, name), name
    for name in ("parzen_histogram_field", "ffd_mi_evaluate", "ffd_mi_refine"):
        assert callable(getattr(hip, name)), name
    L = hip.lib()
    W, Wm = L.sift3d_amd_ffd_mi_refine_work_bytes, L.sift3d_amd_ffd_refine_masked_work_bytes
    extra = 2 * 64 * 64 * 8 + 16                                         # hist + count, W: the MI affine driver's
    for args in ((8, 8, 8, 8, 8, 8, 8, 8, 8, 1), (48, 48, 48, 48, 48, 48, 8, 8, 8, 2),
                 (9, 5, 130, 7, 6, 3, 7, 2, 3, 3)):
        assert W(*args) == Wm(*args) + extra, args
    assert L.sift3d_amd_affine_mi_refine_work_bytes(8, 8, 8, 8, 8, 8, 1) - \
        L.sift3d_amd_affine_refine_masked_work_bytes(8, 8, 8, 8, 8, 8, 1) == extra
    assert W(8, 8, 8, 8, 8, 8, 8, 8, 8, 0) == 0 and W(8, 8, 8, 8, 8, 8, 8, 8, 8, 7) == 0
    assert W(8, 8, 8, 8, 0, 8, 8, 8, 8, 1) == 0 and W(8, 8, 8, 8, 8, 8, 8, 300, 8, 1) == 0
    S = L.sift3d_amd_ffd_refine_struct_bytes                              # nothing that existed changed its size
    assert [S(k) for k in range(8)] == [C.sizeof(hip.FFDRefineParams), C.sizeof(hip.FFDEvaluation),
                                        C.sizeof(hip.FFDRefineResult), 32, 128, 6, 256, 0]
    assert api.MiFFDRefinement._fields == api.FFDRefinement._fields + ("mi", "nmi", "bins")
    assert api.MI_BINS == 32


def test_histogram_field_refusals(hip, bufs):
    L = hip.lib()
    F, M, U_, R, W = bufs[:5]
    hb, work = 64 * 64 * 8, hip.SIMILARITY_GRID * 8

    def call(F=F, o=(8, 8, 8), M=M, n=(8, 8, 8), U=U_, bins=64, rf=(0.0, 1.0), rm=(0.0, 1.0), H=R, Cn=R + 65536, W=W,
             WF=None, WM=None):
        return L.sift3d_hip_parzen_hist_field(F, *o, M, *n, U, bins, *rf, *rm, H, Cn, W, None, WF, WM)
    cases = [dict(F=None), dict(M=None), dict(U=None), dict(H=None), dict(Cn=None), dict(W=None),
             dict(o=(0, 8, 8)), dict(o=(8, -1, 8)), dict(n=(8, 8, 0)),
             dict(F=F + 2), dict(M=M + 1), dict(U=U_ + 2), dict(H=R + 4), dict(Cn=R + 65536 + 4), dict(W=W + 4),
             dict(WF=F + 4096 + 2), dict(WM=M + 4096 + 1),
             dict(H=F), dict(H=M + 4 * 500), dict(Cn=F + 8), dict(W=M), dict(H=F + 4 * 512 - hb),           # on inputs
             dict(H=U_), dict(H=U_ + 4 * 3 * 511), dict(Cn=U_ + 4 * 3 * 512 - 8), dict(W=U_ + 8),          # on the field
             dict(Cn=R + 8), dict(Cn=R + hb - 8), dict(H=W), dict(W=R + hb - 8), dict(W=R + 65536 - work + 8),
             dict(WF=R), dict(WM=R + 65536), dict(WF=W + work - 4),                                      # on the masks
             dict(o=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), F=F)] + BAD_BINS_AND_RANGES
    for kw in cases:
        assert call(**kw) == -1, kw


def test_mi_evaluate_refusals(hip, bufs):
    L = hip.lib()
    F, M, c, U_, R, G, W, T = bufs
    tb = 64 * 64 * 8

    def call(F=F, o=(8, 8, 8), M=M, n=(8, 8, 8), c=c, g=(5, 5, 5), d=(8, 8, 8), A=None, lam=0.0, U=U_, R=R, G=G, W=W,
             WF=None, WM=None, bins=64, rf=(0.0, 1.0), rm=(0.0, 1.0), T=T):
        keep, ptr = _a(A) if A is not None else (None, None)
        return L.sift3d_hip_ffd_mi_evaluate(F, *o, M, *n, c, *g, *d, ptr, lam, U, R, G, W, None, WF, WM, bins, *rf,
                                            *rm, T)
    nan = float("nan")
    cases = [dict(F=None), dict(M=None), dict(c=None), dict(U=None), dict(R=None), dict(G=None), dict(W=None),
             dict(T=None),
             dict(o=(0, 8, 8)), dict(n=(8, 0, 8)), dict(d=(8, -1, 8)), dict(d=(300, 8, 8)), dict(g=(5, 4, 5)),
             dict(A=BAD_A), dict(lam=-1.0), dict(lam=nan), dict(lam=float("inf")),
             dict(F=F + 2), dict(M=M + 1), dict(c=c + 3), dict(U=U_ + 2), dict(R=R + 4), dict(G=G + 2), dict(W=W + 8),
             dict(T=T + 4), dict(WF=F + 4096 + 2), dict(WM=M + 4096 + 1),
             dict(U=F), dict(R=M + 4 * 511), dict(G=c + 4 * 374), dict(W=F), dict(R=U_), dict(G=R + 32), dict(W=G),
             dict(U=W + 64),
             dict(R=T), dict(G=T + tb - 8), dict(U=T + 8), dict(W=T + tb - 16),                            # on the table
             dict(WF=R), dict(WM=U_ + 4)] + BAD_BINS_AND_RANGES
    for kw in cases:
        assert call(**kw) == -1, kw


def test_mi_refine_device_refusals(hip, bufs):
    L = hip.lib()
    F, M, c, U_, _, _, W, _ = bufs
    res = hip.FFDRefineResult()
    sim = hip.Similarity()
    need = L.sift3d_amd_ffd_mi_refine_work_bytes(8, 8, 8, 8, 8, 8, 8, 8, 8, 1)
    assert 0 < need <= 1 << 21

    def call(F=F, o=(8, 8, 8), M=M, n=(8, 8, 8), A=None, res=C.byref(res), c=c, U=U_, W=W, WF=None, WM=None, bins=32,
             rf=(0.0, 1.0), rm=(0.0, 1.0), sim=C.byref(sim), **kw):
        keep, ptr = _a(A) if A is not None else (None, None)
        p = C.byref(hip.ffd_refine_params(**kw))
        return L.sift3d_amd_ffd_mi_refine_device(F, *o, M, *n, ptr, p, res, c, U, W, None, WF, WM, bins, *rf, *rm, sim)
    nan, inf = float("nan"), float("inf")
    cases = [dict(F=None), dict(M=None), dict(res=None), dict(c=None), dict(U=None), dict(W=None), dict(sim=None),
             dict(o=(0, 8, 8)), dict(n=(8, 8, -1)), dict(A=BAD_A), dict(levels=0), dict(levels=7),
             dict(max_evaluations=0), dict(max_evaluations=129), dict(bending=-1.0), dict(bending=nan),
             dict(step0=0.0), dict(step0=nan), dict(step_max=0.5), dict(step_max=inf), dict(tol=0.0), dict(tol=nan),
             dict(min_overlap=-0.1), dict(min_overlap=1.5), dict(min_overlap=nan),
             dict(F=F + 2), dict(M=M + 1), dict(c=c + 2), dict(U=U_ + 1), dict(W=W + 8), dict(WF=F + 4096 + 2),
             dict(W=F), dict(W=M + 4 * 511), dict(c=F), dict(U=M), dict(c=U_ + 4 * 3 * 511), dict(U=W + 1024),
             dict(W=F - need + 8), dict(WF=W + need - 4), dict(WM=W), dict(WM=c)] + BAD_BINS_AND_RANGES
    for kw in cases:
        assert call(**kw) == -1, kw
    p = hip.ffd_refine_params()
    p.spacing[1] = 0
    assert L.sift3d_amd_ffd_mi_refine_device(F, 8, 8, 8, M, 8, 8, 8, None, C.byref(p), C.byref(res), c, U_, W, None,
                                             None, None, 32, 0.0, 1.0, 0.0, 1.0, C.byref(sim)) == -1


def test_python_value_errors():
    from sift3d_amd import api
    v = np.zeros((5, 7, 9), np.float32)
    for kw in (dict(metric="nope"), dict(metric=None), dict(metric="ncc"), dict(bins=32), dict(metric="msd", bins=32),
               dict(range_fixed=(0.0, 1.0)), dict(metric="msd", range_moving=(0.0, 1.0)),
               dict(metric="mi", bins=3), dict(metric="mi", bins=65), dict(metric="mi", bins=8.5),
               dict(metric="mi", bins=True), dict(metric="mi", range_fixed=(1.0, 1.0)),
               dict(metric="mi", range_fixed=(2.0, 1.0)), dict(metric="mi", range_moving=(0.0, float("nan"))),
               dict(metric="mi", range_moving=(float("-inf"), 0.0)), dict(metric="mi", spacing=0),
               dict(metric="mi", levels=0), dict(metric="mi", bending=-1.0), dict(metric="mi", max_evaluations=0),
               dict(metric="mi", bogus=1)):
        with pytest.raises(ValueError):
            api.refine_ffd(v, v, **kw)
    if not api.device_available():
        with pytest.raises(RuntimeError):
            api.refine_ffd(v, v, metric="mi")
