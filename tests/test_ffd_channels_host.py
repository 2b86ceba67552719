"""The multi-channel free-form deformation contract without a device (include/sift3d_amd.h, "Multi-channel free-form
deformation"): the restatement (tests/ffd_channels_restatement.py) against the single-channel one and against finite
differences, the exported symbols and the level struct's layout, every refusal before any device call, and the Python
value errors."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import ffd_channels_restatement as fc
from tests import ffd_restatement as fr
from tests import mask_restatement as mk
from tests.demons_restatement import gamma
from tests.test_affine_refine_host import gaussians
from tests.test_ffd_host import BAD_A, DRIVER, _a, check_trail, driver_pair, summarize

U = 2.0 ** -53
U32 = 2.0 ** -24


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


def stacks(fshape, mshape, nc, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((nc,) + fshape).astype(np.float32),
            rng.standard_normal((nc,) + mshape).astype(np.float32))


def case(nc, seed=1):
    fshape, mshape, spacing = (5, 9, 17), (6, 11, 16), (4, 3, 2)
    F, M = stacks(fshape, mshape, nc, seed)
    c = np.random.default_rng(seed + 1).uniform(-1.5, 1.5, fr.lattice_shape(fshape, spacing)).astype(np.float32)
    A = np.eye(3, 4)
    A[:, 3] = [2.3, -0.4, 0.6]                                             # partly outside
    return F, M, c, spacing, A


# ---- the restatement ---------------------------------------------------------------------------------------------
def test_one_channel_is_the_single_channel_restatement():
    F, M, c, spacing, A = case(1)
    got, u = fc.evaluate(F, M, c, spacing, A)
    want, uw = fr.evaluate(F[0], M[0], c, spacing, A)
    assert 0 < want.n < F[0].size and np.array_equal(u, uw)
    for name in fr.Record._fields:
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    rng = np.random.default_rng(3)
    WF = (rng.uniform(size=F.shape[1:]) > 0.3).astype(np.float32)
    WM = (rng.uniform(size=M.shape[1:]) > 0.3).astype(np.float32)
    got, _ = fc.evaluate(F, M, c, spacing, A, WF, WM)
    want, _, force = mk.evaluate(F[0], M[0], c, spacing, A, WF, WM)
    assert 0 < want.n < int(WF.sum())
    for name in fr.Record._fields:
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    assert np.array_equal(got.S, force)


def test_three_channels_are_the_sum_of_the_single_channel_records():
    """n is the voxels' count, the same for every channel.  S_ee: both sides round correctly rounded sums, the right
    one three of them and two additions (6 u S_ee covers it).  Gc: the stack's entry is the correctly rounded sum of
    W S_d with S_d carrying nc - 1 additions, each single-channel entry is correctly rounded and two additions join
    them: gamma_(nc + 8) sum |W E_c g_cd| covers both sides."""
    nc = 3
    F, M, c, spacing, A = case(nc, 5)
    got, _ = fc.evaluate(F, M, c, spacing, A)
    one = [fr.evaluate(F[k], M[k], c, spacing, A)[0] for k in range(nc)]
    assert all(r.n == got.n for r in one) and 0 < got.n < F[0].size
    assert abs(got.see - sum(r.see for r in one)) <= 6 * U * got.see_terms
    assert np.allclose(got.see_terms, sum(r.see_terms for r in one), rtol=1e-14, atol=0)
    terms = sum(r.Gc_terms for r in one)
    assert np.allclose(got.Gc_terms, terms, rtol=1e-13, atol=0)
    assert np.all(np.abs(got.Gc - sum(r.Gc for r in one)) <= gamma(nc + 8) * terms)
    assert np.abs(got.Gc).max() > 0 and np.array_equal(got.support, one[0].support)


def test_gradient_is_the_finite_difference_of_the_cost():
    """tests/test_ffd_host.py's construction over three channels: A = [I | 0.5], a zero lattice, h = 0.05, so that no
    sample changes its cell (asserted) and every channel's interpolant is linear in the displacement; the bound is the
    sum over the channels of that test's bound, each with its own eps = 16 u32 max |M_c|."""
    nc, fshape, mshape, spacing, h = 3, (9, 10, 11), (10, 11, 12), (4, 3, 5), 0.05
    F = np.stack([gaussians(fshape, 3 + 2 * k) for k in range(nc)])
    M = np.stack([gaussians(mshape, 4 + 2 * k) for k in range(nc)])
    A = np.eye(3, 4)
    A[:, 3] = 0.5
    shape = fr.lattice_shape(fshape, spacing)
    c0 = np.zeros(shape, np.float32)
    base, u0 = fc.evaluate(F, M, c0, spacing, A)
    assert base.n == F[0].size
    per = []
    for k in range(nc):
        m, gx, gy, gz, _ = fr.sample_grad(M[k], u0)
        per.append((16 * U32 * float(np.abs(M[k]).max()), np.abs((m - F[k]).astype(np.float64)),
                    [np.abs(v.astype(np.float64)) for v in (gx, gy, gz)]))
    rng = np.random.default_rng(0)
    picks = [(d,) + tuple(rng.integers(0, n) for n in shape[1:]) for d in range(3) for _ in range(3)]
    picks += [(0, 0, 0, 0), (2,) + tuple(n - 1 for n in shape[1:])]
    (ix, wx), (iy, wy), (iz, wz) = fr._axes(fshape, spacing)
    for pick in picks:
        d = pick[0]
        side = []
        for sgn in (1.0, -1.0):
            c = c0.copy()
            c[pick] = sgn * h
            rec, u = fc.evaluate(F, M, c, spacing, A)
            assert np.array_equal(np.floor(u.astype(np.float64)), np.floor(u0.astype(np.float64)))
            assert rec.n == base.n
            side.append(rec)
        fd = (side[0].see - side[1].see) / (2 * h) / base.n
        ind = np.zeros(shape[1:])
        ind[pick[1:]] = 1.0
        W = np.zeros(fshape)
        for cc in range(4):
            for b in range(4):
                for a in range(4):
                    hit = ind[(iz + cc)[:, None, None], (iy + b)[None, :, None], (ix + a)[None, None, :]]
                    W += hit * (wx[:, a][None, None, :] * wy[:, b][None, :, None] * wz[:, cc][:, None, None])
        bound = 0.0
        for eps, e, G in per:
            de = eps + G[d] * 2.0 ** -25
            e_side = e + h * G[d] * W
            bound += (2 * float(((2 * e_side * de + de * de) * (W > 0)).sum()) / (2 * h)
                      + 2 * float((W * (e * 2 * eps + G[d] * eps + 2 * eps * eps)).sum())) / base.n
        got = 2.0 / base.n * base.Gc[pick]
        print("control %s: gradient %.9g difference %.9g off %.3g bound %.3g" % (pick, got, fd, abs(fd - got), bound))
        assert abs(fd - got) <= bound
    assert np.abs(base.Gc).max() > 0


# ---- the library without a device --------------------------------------------------------------------------------
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


def test_symbols_layouts_and_sizes(hip):
    from sift3d_amd import _native, api
    L = _native.load()
    for name in ("sift3d_hip_ffd_evaluate_channels", "sift3d_amd_ffd_evaluate_channels_work_bytes",
                 "sift3d_amd_ffd_refine_channels_device", "sift3d_amd_ffd_refine_channels_work_bytes",
                 "sift3d_amd_ffd_level_struct_bytes"):
        assert hasattr(L, name), name
    for f in ("ffd_evaluate_channels", "ffd_refine_channels", "FFDLevel"):
        assert hasattr(hip, f), f
    L = hip.lib()
    S = L.sift3d_amd_ffd_level_struct_bytes
    assert [S(k) for k in range(8)] == [64, 0, 8, 24, 32, 48, 56, 0]
    assert C.sizeof(hip.FFDLevel) == 64
    assert [getattr(hip.FFDLevel, f).offset for f in ("d_F", "ox", "oy", "oz", "d_M", "nx", "ny", "nz", "d_WF",
                                                      "d_WM")] == [0, 8, 12, 16, 24, 32, 36, 40, 48, 56]
    E, E1 = L.sift3d_amd_ffd_evaluate_channels_work_bytes, L.sift3d_amd_ffd_evaluate_work_bytes
    for args in ((8, 8, 8, 8, 8, 8), (17, 9, 5, 2, 3, 4), (0, 8, 8, 8, 8, 8), (8, 8, 8, 8, 0, 8)):
        assert E(*args) == E1(*args)                                     # one force volume whatever nc is
    W = L.sift3d_amd_ffd_refine_channels_work_bytes
    rec = L.sift3d_amd_ffd_record_bytes(4, 4, 4)                          # (8 - 1) / 8 + 4 controls per axis
    assert W(8, 8, 8, 8, 8, 8) == E1(8, 8, 8, 8, 8, 8) + rec + 5 * 4 * 3 * 64 + 32 + 8 * 3 * 64 + \
        L.sift3d_amd_jacobian_penalty_work_bytes(8, 8, 8)
    assert W(0, 8, 8, 8, 8, 8) == 0 and W(8, 8, 8, 8, 257, 8) == 0
    import inspect
    sig = inspect.signature(api.refine_ffd)
    assert sig.parameters["features"].default == "intensity" and sig.parameters["sigma"].default == 1.6


def test_evaluate_channels_refusals(hip, bufs):
    L = hip.lib()
    F, M, c, U_, R, G, W, WF, WM = bufs

    def call(F=F, o=(8, 8, 8), M=M, n=(8, 8, 8), nc=3, c=c, g=(4, 4, 4), d=(8, 8, 8), A=None, lam=0.0, U=U_, R=R, G=G,
             W=W, WF=None, WM=None):
        keep, ptr = _a(A) if A is not None else (None, None)
        return L.sift3d_hip_ffd_evaluate_channels(F, *o, M, *n, nc, c, *g, *d, ptr, lam, U, R, G, W, None, WF, WM)
    nan = float("nan")
    cases = [dict(nc=0), dict(nc=-1),
             dict(F=None), dict(M=None), dict(c=None), dict(U=None), dict(R=None), dict(G=None), dict(W=None),
             dict(o=(0, 8, 8)), dict(n=(8, 0, 8)), dict(d=(8, -1, 8)), dict(d=(300, 8, 8)), dict(g=(4, 5, 4)),
             dict(A=BAD_A), dict(lam=-1.0), dict(lam=nan), dict(lam=float("inf")),
             dict(F=F + 2), dict(M=M + 1), dict(c=c + 3), dict(U=U_ + 2), dict(R=R + 4), dict(G=G + 2), dict(W=W + 8),
             dict(WF=WF + 2), dict(WM=WM + 1),
             dict(U=F), dict(R=M + 4 * 511), dict(G=c + 4 * 191), dict(W=F), dict(R=U_), dict(G=R + 32), dict(W=G),
             dict(U=W + 64), dict(U=WF, WF=WF), dict(W=WM + 4 * 508, WM=WM),
             dict(U=F + 4 * (3 * 512 - 1)), dict(R=M + 4 * (3 * 512 - 2))]    # the LAST channel of a stack is an input
    for kw in cases:
        assert call(**kw) == -1, kw


def test_refine_channels_refusals(hip, bufs):
    L = hip.lib()
    F, M, c, U_, F1, M1, W, WF, WM = bufs
    res = hip.FFDRefineResult()
    pen = (hip.FFDPenalty * (6 * 128))()

    def call(lv=((F, (8, 8, 8), M, (8, 8, 8), None, None), (F1, (4, 4, 4), M1, (4, 4, 4), None, None)), levels=None,
             null_table=False, nc=3, A=None, res=C.byref(res), c=c, U=U_, W=W, jac=0.0, pen=None, null_params=False,
             **kw):
        keep, ptr = _a(A) if A is not None else (None, None)
        tab = (hip.FFDLevel * len(lv))(*[hip.FFDLevel(f, *o, m, *n, wf, wm) for f, o, m, n, wf, wm in lv])
        levels = len(lv) if levels is None else levels
        kw.setdefault("levels", len(lv))
        p = None if null_params else C.byref(hip.ffd_refine_params(**kw))
        return L.sift3d_amd_ffd_refine_channels_device(None if null_table else tab, levels, nc, ptr, p, res, c, U, W,
                                                       None, jac, pen)
    l0 = (F, (8, 8, 8), M, (8, 8, 8), None, None)
    l1 = (F1, (4, 4, 4), M1, (4, 4, 4), None, None)
    nan, inf = float("nan"), float("inf")
    cases = [dict(null_table=True), dict(nc=0), dict(nc=-2), dict(levels=0), dict(levels=7), dict(levels=1),
             dict(null_params=True),                                     # the defaults have levels == 3, not 2
             dict(lv=(l0, (None,) + l1[1:])), dict(lv=(l0, l1[:2] + (None,) + l1[3:])),
             dict(lv=((None,) + l0[1:], l1)), dict(lv=(l0[:2] + (None,) + l0[3:], l1)),
             dict(lv=(l0, (F1, (5, 4, 4), M1, (4, 4, 4), None, None))),     # not the halving chain
             dict(lv=(l0, (F1, (4, 4, 4), M1, (4, 3, 4), None, None))),
             dict(lv=(l0, (F1, (4, 4, 0), M1, (4, 4, 4), None, None))),
             dict(lv=((F, (0, 8, 8), M, (8, 8, 8), None, None), l1)),
             dict(res=None), dict(c=None), dict(U=None), dict(W=None), dict(A=BAD_A),
             dict(max_evaluations=0), dict(max_evaluations=129), dict(bending=-1.0), dict(bending=nan),
             dict(step0=0.0), dict(step_max=0.5), dict(tol=0.0), dict(min_overlap=1.5), dict(spacing=(8, 8, 8), tol=nan),
             dict(jac=-1.0, pen=pen), dict(jac=nan, pen=pen), dict(jac=inf, pen=pen), dict(jac=0.5),
             dict(pen=pen, A=np.array([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0]])),    # determinant 0
             dict(lv=((F + 2,) + l0[1:], l1)), dict(lv=(l0, (F1 + 1,) + l1[1:])), dict(lv=(l0, l1[:2] + (M1 + 2,) + l1[3:])),
             dict(lv=(l0[:4] + (WF + 1, None), l1)), dict(lv=(l0, l1[:4] + (None, WM + 2))),
             dict(c=c + 2), dict(U=U_ + 1), dict(W=W + 8),
             dict(W=F), dict(c=F + 4 * (3 * 512 - 1)), dict(U=M), dict(c=U_ + 4 * 3 * 511), dict(U=W + 1024),
             dict(c=F1), dict(U=M1 + 4 * (3 * 64 - 1)), dict(W=F1),        # a coarser level's stack is an input too
             dict(lv=(l0, l1[:4] + (c, None))), dict(lv=(l0[:4] + (None, U_), l1))]
    for kw in cases:
        assert call(**kw) == -1, kw


def test_python_value_errors():
    from sift3d_amd import api
    v = np.zeros((5, 7, 9), np.float32)
    s2, s3 = np.zeros((2, 5, 7, 9), np.float32), np.zeros((3, 5, 7, 9), np.float32)
    for args, kw in (((v, v), dict(features="bogus")), ((v, v), dict(features=None)),
                     ((v, v), dict(features="descriptors", metric="mi")),
                     ((s2, s2), dict(metric="mi")), ((s2, s2), dict(bins=16)),
                     ((v, v), dict(features="descriptors", range_fixed=(0.0, 1.0))),
                     ((s2, s3), {}), ((s2, v), {}), ((v, s2), {}), ((s2, s2), dict(features="descriptors")),
                     ((s2, s2), dict(mask_fixed=np.ones((2, 5, 7, 9), np.float32))),
                     ((v, v), dict(features="descriptors", levels=0))):
        with pytest.raises(ValueError):
            api.refine_ffd(*args, **kw)
    if not api.device_available():
        for args, kw in (((v, v), dict(features="descriptors")), ((s2, s2), {})):
            with pytest.raises(RuntimeError):
                api.refine_ffd(*args, **kw)


# ---- the driver on the pair of tests/test_ffd_host.py, descriptors of every level ----------------------------------
SIGMA = 1.6
GAIN, OFFSET = 3.0, 20.0


@functools.lru_cache(maxsize=None)
def mapped_pair(gain=1.0, offset=0.0):
    """driver_pair() with the moving volume mapped m -> gain * m + offset (float32).  The whole 48^3 pair: the
    12-channel numpy driver takes about 40 s on it, so it is not cropped."""
    F, M, truth = driver_pair()
    return F, (M if (gain, offset) == (1.0, 0.0) else M * np.float32(gain) + np.float32(offset)), truth


@functools.lru_cache(maxsize=None)
def restatement_driver(features="descriptors", gain=1.0, offset=0.0):
    from oracle import sift3d_oracle as so
    so.lib()
    F, M, truth = mapped_pair(gain, offset)
    L = DRIVER["levels"]
    if features == "descriptors":
        Fs, Ms = fc.descriptor_levels(F, L, SIGMA, so), fc.descriptor_levels(M, L, SIGMA, so)
    else:
        Fs, Ms = [a[None] for a in fc.pyramid(F, L)], [a[None] for a in fc.pyramid(M, L)]
    r = fc.refine(Fs, Ms, None, None, None, DRIVER["spacing"], DRIVER["bending"], DRIVER["max_evaluations"])
    return r, summarize(r.trail, r.field, truth)


def zero_field_rms(truth):
    """summarize's RMS of the zero field: of the truth itself over the voxels 4 away from every face"""
    return summarize([(0, 1.0, 0, 1, 1.0, True, 0)], np.zeros_like(truth), truth)[1]


def test_restatement_driver_on_descriptors():
    """the figures DESIGN.md 3.4.16 records"""
    r, (ratio, rms) = restatement_driver()
    _, _, truth = mapped_pair()
    print("restatement driver, descriptors: stop %s, %d evaluations, cost ratio %.4g, RMS field error %.4g voxels "
          "(zero field %.4g)" % (r.stop, len(r.trail), ratio, rms, zero_field_rms(truth)))
    check_trail(r.trail, DRIVER["levels"], DRIVER["max_evaluations"])
    assert r.stop in fr.STOPS
    assert np.array_equal(r.field, fr.field(r.lattice, DRIVER["spacing"], truth.shape[1:]))


def test_restatement_descriptors_survive_a_gain_and_an_offset():
    """What the feature is for, on the restatement: with the moving volume mapped m -> 3 m + 20 the descriptor run
    still recovers the field (its RMS error is below the zero field's), and does better than the intensity MSD, whose
    residual is dominated by the intensity map.  The three figures are in DESIGN.md 3.4.16."""
    _, _, truth = mapped_pair()
    zero = zero_field_rms(truth)
    _, (_, rms_desc) = restatement_driver("descriptors", GAIN, OFFSET)
    _, (_, rms_int) = restatement_driver("intensity", GAIN, OFFSET)
    print("restatement, m -> 3 m + 20: RMS field error descriptors %.4g, intensity MSD %.4g, zero field %.4g"
          % (rms_desc, rms_int, zero))
    assert rms_desc < zero
    assert rms_desc < rms_int
