"""The MIND-SSC contract without a device (include/sift3d_amd.h, "MIND self-similarity descriptors"): the restatement
(tests/mind_restatement.py) against an independent brute force, the contract's exponential against numpy's, the
invariances the descriptor is built for, the exported symbols, every refusal before any device call, the Python value
errors, and the restatement's FFD driver on MIND stacks of a pair whose moving volume has another intensity scale."""
import functools
import inspect

import numpy as np
import pytest

from tests import ffd_channels_restatement as fc
from tests import mind_restatement as mr
from tests.test_ffd_channels_host import zero_field_rms
from tests.test_ffd_host import DRIVER, check_trail, driver_pair, summarize

F32 = np.float32
INF = float("inf")
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


def ulps32(got, want):
    """|got - want| in units of the float32 spacing at want (want float64, got float32)"""
    w32 = np.asarray(want, np.float64).astype(F32)
    ulp = np.spacing(np.maximum(np.abs(w32), F32(2.0 ** -126))).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) / ulp


# ---- the restatement ---------------------------------------------------------------------------------------------
def brute(I, r, d, vlo=0.0, vhi=INF):
    """(out float64 before the rounding to float, D, V) by direct loops over the clipped window, numpy's exp"""
    I = np.asarray(I, F32).astype(np.float64)
    nz, ny, nx = I.shape
    step = ((d, 0, 0), (-d, 0, 0), (0, d, 0), (0, -d, 0), (0, 0, d), (0, 0, -d))

    def s(i, x, y, z):
        dx, dy, dz = step[i]
        return I[min(max(z + dz, 0), nz - 1), min(max(y + dy, 0), ny - 1), min(max(x + dx, 0), nx - 1)]
    D = np.zeros((12, nz, ny, nx))
    for k, (i, j) in enumerate(mr.PAIRS):
        for z in range(nz):
            for y in range(ny):
                for x in range(nx):
                    a = 0.0
                    for qz in range(max(z - r, 0), min(z + r, nz - 1) + 1):
                        for qy in range(max(y - r, 0), min(y + r, ny - 1) + 1):
                            for qx in range(max(x - r, 0), min(x + r, nx - 1) + 1):
                                a += (s(i, qx, qy, qz) - s(j, qx, qy, qz)) ** 2
                    D[k, z, y, x] = a
    V = D.sum(axis=0) / 12.0
    Vc = np.minimum(np.maximum(V, vlo), vhi)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(Vc == 0.0, 0.0, (D - D.min(axis=0)) / Vc)
    return np.exp(-t), D, V


@pytest.mark.parametrize("shape", [(3, 4, 5), (1, 1, 1), (2, 1, 7)])
@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("d", [1, 2, 4])
def test_restatement_against_brute_force(shape, r, d):
    """D and V: both sides sum the same (2r + 1)^3 non-negative terms (V twelve sums of them and a division) in
    different orders: gamma_((2r + 1)^3) * sum D covers either.  The descriptor: the polynomial's truncation error is
    4.4e-10, the double roundings about 1e-15 (t itself differs by the sums' rounding, some 1e-14 relative of a t of at
    most a few tens), and the one rounding to float is 0.5 ulp: within 1 ulp of float32."""
    I = np.random.default_rng(sum(shape) + r + d).normal(0, 10, shape).astype(F32)
    out, D, V, s, n = mr.ref_mind(I, r, d)
    want, Dw, Vw = brute(I, r, d)
    bound = mr.gamma((2 * r + 1) ** 3) * Dw.sum(axis=0)
    assert np.all(np.abs(D - Dw) <= bound[None])
    assert np.all(np.abs(V - Vw) <= bound)
    assert out.dtype == F32 and out.shape == (12,) + shape and n == I.size
    worst = float(ulps32(out, want).max())
    print("shape %s r %d d %d: descriptor off by at most %.3f ulp" % (shape, r, d, worst))
    assert worst <= 1.0
    assert abs(s - Vw.sum()) <= mr.gamma(I.size + 27) * Vw.sum()


def test_cexp_against_numpy():
    t = np.concatenate([np.linspace(0.0, 110.0, 100000), [0.0, 104.0, np.nextafter(104.0, 0.0), 103.0, 87.3, 1.0, INF]])
    got = mr.cexp(t)
    assert got.dtype == np.float64 and np.all(got[t >= 104.0] == 0.0) and not np.signbit(got).any()
    worst = float(ulps32(got.astype(F32), np.exp(-t)).max())
    print("cexp on %d values of t in [0, 110]: off by at most %.3f ulp of float32" % (t.size, worst))
    assert worst <= 1.0
    assert mr.cexp(0.0) == 1.0 and mr.cexp(np.array([0.0]))[0] == 1.0
    assert len(mr.COEF) == 11 and mr.COEF[0] == 1.0 and mr.COEF[1] == -np.log(2.0)
    assert mr.LOG2E == np.log2(np.e)


def noise(shape=(6, 7, 9), seed=3):
    return np.random.default_rng(seed).normal(0, 10, shape).astype(F32)


def test_largest_channel_is_one_and_constant_gives_ones():
    for r, d in ((1, 1), (1, 2), (2, 4)):
        out = mr.ref_mind(noise(), r, d)[0]
        assert np.all(out.max(axis=0) == F32(1.0)) and out.min() >= 0 and out.min() < 1
        flat = mr.ref_mind(np.full((4, 5, 6), 3.25, F32), r, d)[0]
        assert np.all(flat == F32(1.0))
        assert np.all(mr.mind_ssc(np.full((4, 5, 6), 3.25, F32), r, d) == F32(1.0))


def test_invariance_under_a_linear_map():
    """gain -4 (a power of two) with the clamps x 16: the same bytes.  Gain -1.5 and offset 20: D and V carry the
    roundings of the mapped float32 volume, so the descriptor moves a little; 1e-4 absolute is the bound."""
    I = noise()
    V = mr.ref_mind(I)[2]
    vlo, vhi = float(np.quantile(V, 0.2)), float(np.quantile(V, 0.8))
    want = mr.ref_mind(I, 1, 2, vlo, vhi)[0]
    assert (V < vlo).any() and (V > vhi).any()                           # both clamps act
    got = mr.ref_mind(I * F32(-4.0), 1, 2, 16.0 * vlo, 16.0 * vhi)[0]
    assert got.tobytes() == want.tobytes()
    mapped = (I * F32(-1.5) + F32(20.0)).astype(F32)
    got = mr.ref_mind(mapped, 1, 2, 2.25 * vlo, 2.25 * vhi)[0]
    off = float(np.abs(got.astype(np.float64) - want).max())
    print("gain -1.5, offset 20: the descriptor moves by at most %.3g" % off)
    assert off <= 1e-4
    off = float(np.abs(mr.mind_ssc(mapped).astype(np.float64) - mr.mind_ssc(I)).max())
    print("the same through mind_ssc's own clamps: %.3g" % off)
    assert off <= 1e-4


# ---- the library without a device --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bufs():
    """made-up addresses without a device; real allocations covering every range named below with one"""
    from sift3d_amd import api, hip
    if api.device_available():
        b = [hip.lib().sift3d_hip_malloc(1 << 20) for _ in range(6)]
        assert all(b)
        yield b
        for p in b:
            hip.lib().sift3d_hip_free(p)
    else:
        yield [0x10000000 * (k + 1) for k in range(6)]


def test_symbols_and_sizes(hip):
    from sift3d_amd import _native, api
    L = _native.load()
    for name in ("sift3d_hip_mind_ssc", "sift3d_amd_mind_work_bytes"):
        assert hasattr(L, name), name
    W = hip.lib().sift3d_amd_mind_work_bytes
    assert W(8, 8, 8) == W(1, 1, 1) == 32768
    assert W(0, 8, 8) == W(8, -1, 8) == W(8, 8, 0) == 0
    assert (hip.MIND_CHANNELS, hip.MIND_MAX_RADIUS, hip.MIND_MAX_DILATION) == (12, 2, 4)
    assert (mr.CHANNELS, mr.MAX_RADIUS, mr.MAX_DILATION) == (12, 2, 4)
    par = inspect.signature(hip.mind_ssc).parameters
    assert list(par) == ["src", "out", "radius", "dilation", "vlo", "vhi", "D", "V", "stats", "work"]
    assert [par[k].default for k in list(par)[1:]] == [None, 1, 2, 0.0, INF, None, None, None, None]
    par = inspect.signature(api.mind_ssc).parameters
    assert list(par) == ["volume", "radius", "dilation", "floor", "ceiling"]
    assert [par[k].default for k in list(par)[1:]] == [1, 2, 1e-3, 1e3]
    assert inspect.signature(api.refine_ffd).parameters["mind"].default is None
    assert inspect.signature(api.register_dense).parameters["mind"].default is None


def test_refusals(hip, bufs):
    """one case per rule of the header's list; an 8^3 volume: 2048 bytes, out 24576, D 49152, V 4096"""
    L = hip.lib()
    src, out, D, V, stats, work = bufs

    def call(src=src, dims=(8, 8, 8), r=1, d=2, vlo=0.0, vhi=INF, out=out, D=D, V=V, stats=stats, work=work):
        return L.sift3d_hip_mind_ssc(src, *dims, r, d, vlo, vhi, out, D, V, stats, work, None)
    cases = [dict(src=None), dict(work=None), dict(out=None, D=None, V=None, stats=None),
             dict(dims=(0, 8, 8)), dict(dims=(8, -1, 8)), dict(dims=(8, 8, 0)),
             dict(r=0), dict(r=3), dict(d=0), dict(d=5),
             dict(vlo=-1.0), dict(vlo=NAN), dict(vlo=2.0, vhi=1.0), dict(vhi=NAN), dict(vlo=INF, vhi=1.0),
             dict(src=src + 2), dict(out=out + 1), dict(D=D + 4), dict(V=V + 4), dict(stats=stats + 4),
             dict(work=work + 4),
             dict(out=src), dict(D=src + 2040), dict(V=src + 8), dict(stats=src + 2040), dict(work=src + 2040),
             dict(src=work + 32760),                                     # the last partial slot is part of the work
             dict(D=out + 24568), dict(V=out + 8), dict(stats=out + 24568), dict(work=out + 24568),
             dict(V=D + 49144), dict(stats=D), dict(work=D + 8), dict(stats=V + 4088), dict(work=V + 4088),
             dict(stats=work + 32760), dict(work=stats - 32760), dict(out=work + 32764, D=None, V=None)]
    for kw in cases:
        assert call(**kw) == -1, kw
    from sift3d_amd import api
    if not api.device_available():
        return
    # the premise: the call the cases vary is accepted, and so are the optional outputs left out and vhi == vlo
    for kw in ({}, dict(D=None, V=None, stats=None), dict(out=None, D=None, V=None), dict(vlo=1.0, vhi=1.0),
               dict(stats=out + 24576), dict(V=src + 2048)):
        assert call(**kw) == 0, kw
    assert L.sift3d_hip_stream_sync(None) == 0


def test_python_value_errors():
    from sift3d_amd import api
    v = np.zeros((5, 7, 9), F32)
    s2 = np.zeros((2, 5, 7, 9), F32)
    for args, kw in (((v, v), dict(features="mind", metric="mi")),
                     ((v, v), dict(features="mind", landmarks=(np.zeros((2, 3)), np.zeros((2, 3))))),
                     ((s2, s2), dict(features="mind")), ((v, s2), dict(features="mind")),
                     ((v, v), dict(features="mind", mind=dict(sigma=1.0))),
                     ((v, v), dict(features="mind", mind=3)),
                     ((v, v), dict(features="intensity", mind=dict(radius=1))),
                     ((v, v), dict(features="descriptors", mind={})),
                     ((v, v), dict(features="mind", bins=16)),
                     ((v, v), dict(features="mind", levels=0))):
        with pytest.raises(ValueError):
            api.refine_ffd(*args, **kw)
    for kw in (dict(features="mind", force="lncc"), dict(features=("mind", {}), force="lncc")):
        with pytest.raises(ValueError):
            api.refine_field(v, v, **kw)
    for kw in (dict(features="descriptors", mind=dict(dilation=1)), dict(features="intensity", mind={})):
        with pytest.raises(ValueError, match="mind belongs"):
            api.register_dense(v, v, **kw)
    with pytest.raises(ValueError, match="keys among"):
        api.register_dense(v, v, features="mind", mind=dict(sigma=2.0))
    with pytest.raises(ValueError):
        api.mind_ssc(v)                                                  # not a CUDA tensor
    if not api.device_available():
        with pytest.raises(RuntimeError):
            api.refine_ffd(v, v, features="mind")


def test_python_value_errors_on_the_device_wrappers(hip):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        # (the wrappers look at the tensors first: a CPU tensor is refused whatever else is passed)
        with pytest.raises(ValueError):
            hip.mind_ssc(torch.zeros((3, 4, 5)))
    for kw in (dict(radius=0), dict(radius=3), dict(radius=1.0), dict(radius=True), dict(dilation=0), dict(dilation=5)):
        with pytest.raises(ValueError):
            hip._mind_int(kw.get("radius", kw.get("dilation")), 2 if "radius" in kw else 4, "mind_ssc", "x")
    for vlo, vhi in ((-1.0, 1.0), (NAN, 1.0), (1.0, NAN), (2.0, 1.0), ("a", 1.0), (True, 1.0)):
        with pytest.raises(ValueError):
            hip._mind_clamps(vlo, vhi, "mind_ssc")
    assert hip._mind_clamps(0, INF, "mind_ssc") == (0.0, INF)


# ---- the driver on the pair of tests/test_ffd_host.py, MIND stacks of every level ------------------------------------
MIND = dict(radius=1, dilation=1, floor=1e-3, ceiling=1e3)


def inverted(m):
    """m -> max + 10 - 1.5 m: the contrast inverted"""
    m = np.asarray(m, F32)
    return (F32(float(m.max()) + 10.0) - F32(1.5) * m).astype(F32)


def non_monotone(m):
    """m -> (m - mid)^2 / (span / 4): the mid-range darkest, both ends bright"""
    m = np.asarray(m, F32)
    lo, hi = float(m.min()), float(m.max())
    mid, span = 0.5 * (lo + hi), hi - lo
    return ((m.astype(np.float64) - mid) ** 2 / (span / 4.0)).astype(F32)


MAPS = {"unmapped": lambda m: m, "inverted": inverted, "non_monotone": non_monotone}


@functools.lru_cache(maxsize=None)
def mapped_pair(which):
    F, M, truth = driver_pair()
    return F, np.ascontiguousarray(MAPS[which](M)), truth


@functools.lru_cache(maxsize=None)
def restatement_driver(features, which, dilation=1):
    """the restatement's FFD driver with DRIVER's parameters on MIND stacks (or the intensities) of every level"""
    F, M, truth = mapped_pair(which)
    L = DRIVER["levels"]
    if features == "mind":
        kw = dict(r=MIND["radius"], d=dilation, floor=MIND["floor"], ceiling=MIND["ceiling"])
        Fs, Ms = mr.mind_levels(F, L, **kw), mr.mind_levels(M, L, **kw)
    else:
        Fs, Ms = [a[None] for a in fc.pyramid(F, L)], [a[None] for a in fc.pyramid(M, L)]
    r = fc.refine(Fs, Ms, None, None, None, DRIVER["spacing"], DRIVER["bending"], DRIVER["max_evaluations"])
    return r, summarize(r.trail, r.field, truth)


@pytest.mark.parametrize("which", ["inverted", "non_monotone"])
def test_restatement_mind_survives_another_intensity_scale(which):
    """What the feature is for, on the restatement: with the moving volume's contrast inverted, or mapped by a
    function that is not monotone, the MIND run (d = 1) still recovers the field (its RMS error is below the zero
    field's) and does better than the intensity MSD on the same pair.  DESIGN.md 3.4.25 records the figures."""
    _, _, truth = mapped_pair(which)
    zero = zero_field_rms(truth)
    r, (ratio, rms_mind) = restatement_driver("mind", which)
    check_trail(r.trail, DRIVER["levels"], DRIVER["max_evaluations"])
    ri, (_, rms_int) = restatement_driver("intensity", which)
    print("restatement, %s: RMS field error MIND d=1 %.4g (%d evaluations, cost ratio %.4g), intensity MSD %.4g "
          "(%d evaluations), zero field %.4g" % (which, rms_mind, len(r.trail), ratio, rms_int, len(ri.trail), zero))
    assert rms_mind < zero
    assert rms_mind < rms_int


@pytest.mark.parametrize("which", ["unmapped", "inverted", "non_monotone"])
def test_restatement_mind_at_dilation_two(which):
    """The same driver at mind_ssc's default dilation 2, on the unmapped pair too: the other column of DESIGN.md
    3.4.25's table.  The descriptor is invariant under the inverted map, so that run must land on the unmapped one's
    figure to the roundings of the mapped float32 volume (1e-4 in the descriptor: 1 % of the RMS is far above it and
    far below the difference to the non-monotone map's figure)."""
    _, _, truth = mapped_pair(which)
    zero = zero_field_rms(truth)
    r, (ratio, rms) = restatement_driver("mind", which, 2)
    check_trail(r.trail, DRIVER["levels"], DRIVER["max_evaluations"])
    print("restatement, %s: RMS field error MIND d=2 %.4g (%d evaluations, cost ratio %.4g), zero field %.4g"
          % (which, rms, len(r.trail), ratio, zero))
    assert rms < zero
    if which == "inverted":
        same = restatement_driver("mind", "unmapped", 2)[1][1]
        assert abs(rms - same) <= 0.01 * same
