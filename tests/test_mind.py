"""The MIND-SSC kernel and its wiring on the device (include/sift3d_amd.h, "MIND self-similarity descriptors"): every
output byte for byte against the numpy restatement (tests/mind_restatement.py), the calling contracts of
tests/test_calling_contracts.py on the new entry, api.mind_ssc, and the FFD and demons drivers on MIND stacks of a pair
whose moving volume has an inverted contrast."""
import functools
import math

import numpy as np
import pytest

from tests import mind_restatement as mr
from tests.test_calling_contracts import delay, guarded  # noqa: F401  (delay: a fixture)
from tests.test_ffd_channels_host import zero_field_rms
from tests.test_ffd_host import DRIVER, check_trail, driver_pair, summarize
from tests.test_mind_host import MIND, mapped_pair, restatement_driver
from tests.test_similarity import dev

pytestmark = pytest.mark.gpu
F32 = np.float32
INF = float("inf")
RD = [(r, d) for r in (1, 2) for d in (1, 2, 4)]


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


def bytes_of(t):
    import torch
    return t.contiguous().view(torch.uint8).cpu().numpy().reshape(-1)


def content(kind, shape, seed=0):
    rng = np.random.default_rng(seed + sum(shape))
    if kind == "noise":
        return rng.normal(0, 100, shape).astype(F32)
    if kind == "integers":
        return rng.integers(-8, 9, shape).astype(F32)
    if kind == "step":
        v = np.zeros(shape, F32)
        v[..., shape[2] // 2:] = 50.0
        v[shape[0] // 2:] += 7.0
        return v
    if kind == "constant":
        return np.full(shape, 3.25, F32)
    if kind == "subnormal":
        return (rng.normal(0, 100, shape) * 2.0 ** -140).astype(F32)
    if kind == "huge":
        return (rng.normal(0, 100, shape) * 1e30).astype(F32)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def reference(kind, shape, r, d, vlo=0.0, vhi=INF):
    return mr.ref_mind(content(kind, shape), r, d, vlo, vhi)


def device(hip, I, r, d, vlo=0.0, vhi=INF, **kw):
    """(out, D, V, stats) of one full call"""
    import torch
    src = dev(I)
    D = torch.empty((12,) + I.shape, dtype=torch.float64, device="cuda")
    V = torch.empty(I.shape, dtype=torch.float64, device="cuda")
    stats = torch.empty(2, dtype=torch.int64, device="cuda")
    out = hip.mind_ssc(src, None, r, d, vlo, vhi, D=D, V=V, stats=stats, **kw)
    return out, D, V, stats


def check(hip, kind, shape, r, d, vlo=0.0, vhi=INF):
    I = content(kind, shape)
    want, Dw, Vw, sw, nw = reference(kind, shape, r, d, vlo, vhi)
    out, D, V, stats = device(hip, I, r, d, vlo, vhi)
    what = "%s %s r %d d %d clamps (%g, %g)" % (kind, shape, r, d, vlo, vhi)
    assert D.cpu().numpy().tobytes() == Dw.tobytes(), what
    assert V.cpu().numpy().tobytes() == Vw.tobytes(), what
    assert out.cpu().numpy().tobytes() == want.tobytes(), what
    s, n = hip.demons_stats(stats)
    assert int(n[0]) == nw == I.size, what
    exact = math.fsum(Vw.ravel())                                        # the correctly rounded sum of the same V
    assert abs(float(s[0]) - exact) <= mr.gamma(I.size) * exact, what
    return out, D, V


# (nz, ny, nx): single voxels and lines; an x tile crossed, no tile multiple; a z stretch crossed at the default 32;
# axes shorter than the dilation and the radius on each axis in turn; more tiles (2050) than workgroups (2048)
SHAPES = [(1, 1, 1), (3, 1, 1), (2, 3, 1), (5, 6, 70), (7, 9, 65), (40, 5, 3), (1, 9, 10), (9, 1, 10), (9, 10, 1),
          (2, 6, 7), (6, 2, 7), (6, 7, 2), (1, 8200, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bytes_against_the_restatement(hip, shape):
    for r, d in RD:
        out, _, _ = check(hip, "noise", shape, r, d)
        assert float(out.max(dim=0).values.min()) == 1.0                 # the largest channel is exactly 1


@pytest.mark.parametrize("kind", ["integers", "step", "constant", "subnormal", "huge"])
def test_content(hip, kind):
    shape = (5, 6, 70)
    for r, d in ((1, 1), (1, 2), (2, 2), (2, 4)):
        out, D, V = check(hip, kind, shape, r, d)
        if kind == "constant":
            assert bool((out == 1.0).all()) and bool((D == 0).all())
        if kind == "integers":                                           # exact: every term an integer below 2^53
            I = content(kind, shape).astype(np.int64)
            want = mr.distances(I.astype(F32), r, d)
            assert np.array_equal(D.cpu().numpy(), want) and np.all(want == np.round(want))
        if kind in ("subnormal", "huge"):
            assert bool((V > 0).all()) and bool(torch_isfinite(V))
        if kind == "huge":                                               # 1e30 x the noise: the scale changes nothing
            same = mr.ref_mind(content("noise", shape), r, d)[0]        # but the float32 roundings of the volume
            assert float(np.abs(out.cpu().numpy().astype(np.float64) - same).max()) <= 1e-4


def torch_isfinite(t):
    import torch
    return torch.isfinite(t).all()


def test_clamps(hip):
    shape, r, d = (5, 6, 70), 1, 2
    V = reference("noise", shape, r, d)[2]
    assert V.min() > 0
    for vlo, vhi in ((0.0, INF), (2.0 * V.max(), INF), (0.0, 0.5 * V.min()), (0.0, 0.0),
                     (float(np.quantile(V, 0.3)), float(np.quantile(V, 0.7)))):
        out, _, _ = check(hip, "noise", shape, r, d, vlo, vhi)
        if vhi == 0.0:                                                   # Vc == 0: t = 0, all ones
            assert bool((out == 1.0).all())


def test_each_output_alone_and_repeated_calls(hip):
    import torch
    shape, r, d = (7, 9, 65), 2, 2
    I = content("noise", shape)
    src = dev(I)
    V = reference("noise", shape, r, d)[2]
    vlo, vhi = float(np.quantile(V, 0.2)), float(np.quantile(V, 0.9))
    full = [bytes_of(t) for t in device(hip, I, r, d, vlo, vhi)]
    again = [bytes_of(t) for t in device(hip, I, r, d, vlo, vhi)]
    for a, b in zip(full, again):
        assert np.array_equal(a, b)
    out = hip.mind_ssc(src, None, r, d, vlo, vhi)
    assert np.array_equal(bytes_of(out), full[0])
    given = torch.full((12,) + shape, 7.0, dtype=torch.float32, device="cuda")
    assert hip.mind_ssc(src, given, r, d, vlo, vhi) is given and np.array_equal(bytes_of(given), full[0])
    D = torch.empty((12,) + shape, dtype=torch.float64, device="cuda")
    assert hip.mind_ssc(src, False, r, d, vlo, vhi, D=D) is None and np.array_equal(bytes_of(D), full[1])
    Vd = torch.empty(shape, dtype=torch.float64, device="cuda")
    hip.mind_ssc(src, False, r, d, vlo, vhi, V=Vd)
    assert np.array_equal(bytes_of(Vd), full[2])
    # statistics only: 16 bytes between guard bands, nothing else written
    stats, bands = guarded(16, 0xAB, "int64")
    hip.mind_ssc(src, False, r, d, stats=stats)
    torch.cuda.synchronize()
    assert np.array_equal(bytes_of(stats), full[3])
    assert [int((b != 0xAB).sum()) for b in bands] == [0, 0]
    assert np.array_equal(bytes_of(src), I.view(np.uint8).reshape(-1))
    for kw in (dict(out=False), dict(radius=3), dict(dilation=0), dict(vlo=-1.0), dict(vlo=2.0, vhi=1.0),
               dict(D=torch.empty((12,) + shape, dtype=torch.float32, device="cuda")),
               dict(V=torch.empty((1,) + shape, dtype=torch.float64, device="cuda")),
               dict(out=torch.empty((3,) + shape, dtype=torch.float32, device="cuda")),
               dict(stats=torch.empty(3, dtype=torch.int64, device="cuda"))):
        with pytest.raises(ValueError):
            hip.mind_ssc(src, **kw)
    # the library's own refusal: V lies over the input
    raw = torch.zeros(8 * I.size, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError):
        hip.mind_ssc(raw[:4 * I.size].view(torch.float32).reshape(shape), False, r, d,
                     V=raw.view(torch.float64).reshape(shape))


# ---- calling contracts (tests/test_calling_contracts.py, A and B) -------------------------------------------------------
def test_work_of_the_librarys_size_guarded_and_poisoned(hip):
    import torch
    shape, r, d = (5, 6, 70), 2, 1
    I = content("noise", shape)
    need = hip.lib().sift3d_amd_mind_work_bytes(*shape[::-1])
    assert need == 32768
    want = [bytes_of(t) for t in device(hip, I, r, d)]
    with pytest.raises(ValueError):
        device(hip, I, r, d, work=guarded(need, 0, "uint8")[0][:-1])
    for fill in (0xFF, 0x00):
        work, bands = guarded(need, fill, "uint8")
        for run in ("first", "second"):                                  # the second finds what the first left behind
            got = [bytes_of(t) for t in device(hip, I, r, d, work=work)]
            torch.cuda.synchronize()
            assert [int((b != fill).sum()) for b in bands] == [0, 0], (run, fill)
            for a, b in zip(got, want):
                assert np.array_equal(a, b), (run, fill)


def test_entry_is_ordered_on_the_callers_stream(hip, delay):
    import torch
    shape, r, d = (5, 6, 70), 1, 2
    I = content("noise", shape)
    real = dev(I)
    hip.current_stream(refresh=True)
    want = [bytes_of(t) for t in device(hip, I, r, d)]
    zeros = [bytes_of(t) for t in device(hip, np.zeros_like(I), r, d)]
    assert any(not np.array_equal(a, b) for a, b in zip(zeros, want))
    twin = torch.zeros_like(real)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    try:
        with torch.cuda.stream(s):
            hip.current_stream(refresh=True)
            for _ in range(20):
                delay.mul_(1.0001)
            twin.copy_(real)
            D = torch.empty((12,) + shape, dtype=torch.float64, device="cuda")
            V = torch.empty(shape, dtype=torch.float64, device="cuda")
            stats = torch.empty(2, dtype=torch.int64, device="cuda")
            out = hip.mind_ssc(twin, None, r, d, D=D, V=V, stats=stats)
        hip.current_stream(refresh=True)
        torch.cuda.current_stream().wait_stream(s)
        for a, b in zip((out, D, V, stats), want):
            assert np.array_equal(bytes_of(a), b)
    finally:
        hip.current_stream(refresh=True)


# ---- api.mind_ssc ---------------------------------------------------------------------------------------------------
def test_api_mind_ssc(hip, monkeypatch):
    import torch
    from sift3d_amd import api
    shape = (9, 11, 70)
    I = content("step", shape) + content("noise", shape) * F32(0.001)    # flat regions under the floor, edges over it
    src = dev(I)
    stats = torch.empty(2, dtype=torch.int64, device="cuda")
    calls = []
    real = hip.mind_ssc
    monkeypatch.setattr(hip, "mind_ssc", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    for kw in (dict(), dict(radius=2, dilation=1), dict(floor=0.5, ceiling=2.0), dict(floor=None), dict(ceiling=None)):
        r, d = kw.get("radius", 1), kw.get("dilation", 2)
        real(src, False, r, d, stats=stats)
        s, n = hip.demons_stats(stats)
        mean = float(s[0]) / int(n[0])
        del calls[:]
        got = api.mind_ssc(src, **kw)
        assert len(calls) == 2
        want = mr.mind_ssc(I, r, d, kw.get("floor", 1e-3), kw.get("ceiling", 1e3), mean=mean)
        assert tuple(got.shape) == (12,) + shape and got.cpu().numpy().tobytes() == want.tobytes(), kw
    V = mr.ref_mind(I)[2]
    assert (V < 1e-3 * V.mean()).any()                                   # the floor acts on this content
    del calls[:]
    got = api.mind_ssc(src, floor=None, ceiling=None)
    assert len(calls) == 1 and got.cpu().numpy().tobytes() == mr.ref_mind(I)[0].tobytes()
    assert bool((api.mind_ssc(dev(content("constant", shape))) == 1.0).all())
    for kw in (dict(floor=-1.0), dict(ceiling=INF), dict(floor=2.0, ceiling=1.0), dict(radius=3), dict(dilation=5)):
        with pytest.raises(ValueError):
            api.mind_ssc(src, **kw)


# ---- the drivers on the inverted pair ---------------------------------------------------------------------------------
def field_rms(field, truth):
    return summarize([(0, 1.0, 0, 1, 1.0, True, 0)], field.cpu().numpy(), truth)[1]


def test_refine_ffd_on_mind_against_the_restatement(hip):
    """tests/test_ffd_channels.py's test_driver_against_the_restatement with features="mind" on the inverted pair, its
    margins unchanged: the cost falls by at least half the factor the restatement reached and the RMS field error is
    at most 1.5 x the restatement's.  The RMS is below the zero field's and below the intensity run's; the stacks passed
    to the channel driver by hand give the api's field byte for byte."""
    from sift3d_amd import api
    F, M, truth = mapped_pair("inverted")
    zero = zero_field_rms(truth)
    _, (ratio_ref, rms_ref) = restatement_driver("mind", "inverted")
    dF, dM = dev(F), dev(M)
    r = api.refine_ffd(dM, dF, None, DRIVER["spacing"], DRIVER["levels"], DRIVER["bending"],
                       max_evaluations=DRIVER["max_evaluations"], features="mind", mind=MIND)
    ri = api.refine_ffd(dM, dF, None, DRIVER["spacing"], DRIVER["levels"], DRIVER["bending"],
                        max_evaluations=DRIVER["max_evaluations"])
    assert type(r).__name__ == "FFDRefinement"
    trail = [tuple(e) for e in r.trail]
    ratio, rms = summarize(trail, r.field.cpu().numpy(), truth)
    rms_int = summarize([tuple(e) for e in ri.trail], ri.field.cpu().numpy(), truth)[1]
    print("device driver, MIND d=1, inverted pair: stop %s, %d evaluations, cost ratio %.4g (restatement %.4g), RMS "
          "%.4g (restatement %.4g), intensity MSD %.4g, zero field %.4g"
          % (r.stop, len(trail), ratio, ratio_ref, rms, rms_ref, rms_int, zero))
    check_trail(trail, DRIVER["levels"], DRIVER["max_evaluations"])
    assert 1.0 / ratio >= 0.5 / ratio_ref
    assert rms <= 1.5 * rms_ref
    assert r.jacobian.folded == 0
    assert rms < zero
    assert rms < rms_int
    fv, mv = [dF, hip.restrict2(dF)], [dM, hip.restrict2(dM)]
    res, lattice, field, pen = hip.ffd_refine_channels(
        [api.mind_ssc(v, **MIND) for v in fv], [api.mind_ssc(v, **MIND) for v in mv], None,
        hip.ffd_refine_params(spacing=DRIVER["spacing"], levels=DRIVER["levels"], bending=DRIVER["bending"],
                              max_evaluations=DRIVER["max_evaluations"]))
    assert pen is None and res.evaluations == len(trail)
    assert np.array_equal(bytes_of(lattice), bytes_of(r.lattice)) and np.array_equal(bytes_of(field), bytes_of(r.field))


@pytest.mark.parametrize("update", ["diffeomorphic", "symmetric"])
def test_refine_field_on_mind(hip, update):
    """refine_field(features="mind", levels=2) on the inverted pair: the RMS field error is below the zero field's and
    below that of features="descriptors", whose gradient directions flip with the contrast."""
    from sift3d_amd import api
    F, M, truth = mapped_pair("inverted")
    zero = zero_field_rms(truth)
    dF, dM = dev(F), dev(M)
    r = api.refine_field(dM, dF, features="mind", levels=2, update=update)
    rd = api.refine_field(dM, dF, features="descriptors", levels=2, update=update)
    rms, rms_desc = field_rms(r.field, truth), field_rms(rd.field, truth)
    print("device demons, %s, levels 2, inverted pair: RMS field error MIND %.4g, descriptors %.4g, zero field %.4g"
          % (update, rms, rms_desc, zero))
    assert rms < zero
    assert rms < rms_desc
    assert r.jacobian.folded == 0
    # the stacks by hand
    fv, mv = [dF, hip.restrict2(dF)], [dM, hip.restrict2(dM)]
    Fs, Ms = [api.mind_ssc(v) for v in fv], [api.mind_ssc(v) for v in mv]
    import torch
    u = torch.zeros((3,) + F.shape, dtype=torch.float32, device="cuda")
    its = [api.DEMONS_ITERATIONS] * 2
    if update == "symmetric":
        hip.logdemons(Fs, Ms, u, its, api.DEMONS_ALPHA, api.DEMONS_SIGMA_FLUID, api.DEMONS_SIGMA_DIFFUSION, True, 1,
                      api.field_squarings(16.0))
        assert np.array_equal(bytes_of(u), bytes_of(r.velocity))
    else:
        hip.demons_multires(Fs, Ms, u, its, api.DEMONS_ALPHA, api.DEMONS_SIGMA_FLUID, api.DEMONS_SIGMA_DIFFUSION,
                            update=update, squarings=api.demons_squarings(api.DEMONS_ALPHA))
        assert np.array_equal(bytes_of(u), bytes_of(r.field))
    # the keywords through features: another dilation gives another field
    r1 = api.refine_field(dM, dF, features=("mind", dict(dilation=1)), levels=2, update=update)
    assert not np.array_equal(bytes_of(r1.field), bytes_of(r.field))


# ---- the other ways in ------------------------------------------------------------------------------------------------
def test_register_dense_hands_mind_to_refine_field(hip, monkeypatch):
    """register_dense(features="mind", mind=...) is refine_field(features=("mind", ...)) after the spline stage (replaced
    here by a zero field, as tests/test_demons_masks.py does for the masks)"""
    import torch
    from sift3d_amd import api
    F, M, _ = driver_pair()
    dF, dM = dev(F), dev(M)
    Spline = type("Spline", (), dict(A=np.eye(3, 4), tps=None, inliers=0, num_matches=0))
    monkeypatch.setattr(api, "register_deformable", lambda m, f, **kw: Spline())
    monkeypatch.setattr(api, "displacement_field",
                        lambda tps, shape, device=None: torch.zeros((3,) + tuple(shape), device="cuda"))
    kw = dict(iterations=3, levels=2, update="diffeomorphic")
    r = api.register_dense(dM, dF, features="mind", mind=dict(dilation=1), **kw)
    assert type(r).__name__ == "MultiresRegistration" and len(r.msd) == 6
    want = api.refine_field(dM, dF, features=("mind", dict(dilation=1)), **kw)
    other = api.refine_field(dM, dF, features="mind", **kw)
    assert np.array_equal(bytes_of(r.field), bytes_of(want.field)) and np.array_equal(r.msd, want.msd)
    assert not np.array_equal(bytes_of(r.field), bytes_of(other.field))
    with pytest.raises(ValueError, match="mind belongs"):
        api.register_dense(dM, dF, features="descriptors", mind=dict(dilation=1))


def test_register_ffd_on_mind():
    """tests/test_ffd_channels.py's test_register_ffd_end_to_end with features="mind" (the unmapped pair: the keypoint
    stage ahead of the FFD still matches gradient descriptors)"""
    from sift3d_amd import api
    F, M, _ = driver_pair()
    r = api.register_ffd(M, F, levels=2, ffd_params=dict(features="mind", mind=dict(dilation=1), max_evaluations=6))
    assert type(r.refinement).__name__ == "FFDRefinement"
    assert r.refinement.stop in ("converged", "evaluations", "flat", "failed")
    assert r.refinement.trail[-1].level == 0 and tuple(r.refinement.field.shape) == (3,) + F.shape
    acc = [e.E for e in r.refinement.trail if e.level == 0 and e.accepted]
    assert all(b < a for a, b in zip(acc, acc[1:]))
