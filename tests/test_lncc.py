"""GPU: local cross-correlation (sift3d_hip_lncc, sift3d_hip_lncc_force, sift3d_hip_field_normalize,
sift3d_amd_demons_lncc_device, api.local_ncc, api.refine_field(force="lncc")) against the numpy restatement of the
contract in include/sift3d_amd.h, "Local cross-correlation" (tests/lncc_restatement.py): the cc map, the four
coefficient volumes, the force and the fields bit for bit, the counts exactly, the sums within the bound of any
summation order; NaN / poisoned guard bands around every output; the scratch-size and stream contracts; and what the
feature must achieve on a pair with a spatially varying intensity relation, measured against the restatement's own
driver on the CPU."""
import numpy as np
import pytest

from tests import field_restatement as fr
from tests import lncc_restatement as lr
from tests import multires_restatement as mr

pytestmark = pytest.mark.gpu

F32 = np.float32
F64 = np.float64


@pytest.fixture(scope="module")
def hip():
    import torch
    from sift3d_amd import hip as h
    h.lib()
    assert torch.cuda.is_available()
    h.current_stream(refresh=True)
    return h


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tm(w):
    return None if w is None else _t(w)


def _bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    kind = np.uint32 if got.dtype == F32 else np.uint64
    bad = got.view(kind) != want.view(kind)
    if bad.any():
        i = tuple(int(a[0]) for a in np.nonzero(bad))
        raise AssertionError("%s: %d of %d values differ, first at %s: %r != %r"
                             % (what, int(bad.sum()), bad.size, i, got[i], want[i]))


def _check_sum(s, c, want_s, want_c, what):
    print("%s: sum %.17g restated %.17g count %d" % (what, s, want_s, c))
    assert c == want_c, (what, c, want_c)
    assert abs(s - want_s) <= lr.gamma(max(want_c, 1)) * want_s, (what, s, want_s)


# (fixed [nz, ny, nx], moving [mz, my, mx], radius): two x tiles with the second ragged and nothing a multiple of four,
# at every radius class; a window wider than the grid on every axis; nx = 1; a z march across every ring wrap and more
# than one stretch of planes
CASES = [((9, 11, 70), (10, 9, 67), 1), ((9, 11, 70), (10, 9, 67), 2), ((9, 11, 70), (10, 9, 67), 4),
         ((3, 2, 5), (4, 3, 6), 4), ((6, 5, 1), (5, 6, 2), 2), ((40, 5, 6), (38, 6, 5), 1)]
IDS = ["%dx%dx%d-r%d" % (s + (r,)) for s, _, r in CASES]
# the field's amplitude: +-3 voxels; +-1 on the two grids of 30 voxels, where +-3 leaves two or three voxels inside
AMP = {(3, 2, 5): 1.0, (6, 5, 1): 1.0}


def _case(shape, mshape, seed, amp=3.0):
    """F, a W near it, M, a field random within +-amp voxels (some voxels sample outside), and two random masks"""
    rng = np.random.default_rng(seed)
    F = rng.normal(0, 1, shape).astype(F32)
    W = (F * F32(0.7) + rng.normal(0, 0.5, shape)).astype(F32)
    M = rng.normal(0, 1, mshape).astype(F32)
    u = rng.uniform(-amp, amp, (3,) + tuple(shape)).astype(F32)
    WF = (rng.random(shape) < 0.8).astype(F32)
    WM = (rng.random(mshape) < 0.8).astype(F32)
    return F, W, M, u, WF, WM


def _banded(shape, dtype, fill=float("nan")):
    """(a contiguous tensor of `shape` between two guard bands, the bands): everything filled with NaN"""
    import torch
    n = int(np.prod(shape))
    G = max(1024, n)
    whole = torch.full((G + n + G,), fill, dtype=dtype, device="cuda")
    return whole[G:G + n].view(tuple(shape)), (whole[:G], whole[G + n:])


def _bands_clean(bands, what):
    import torch
    for name, pair in bands.items():
        for b in pair:
            assert bool(torch.isnan(b).all()), "%s: %s wrote into a guard band" % (what, name)


def _passes(hip, F, W, u, mshape, r, WF=None, WM=None):
    """(cc, coef, sum, count, force) of the two passes on the device, every output between NaN guard bands"""
    import torch
    shape = F.shape
    cc, b_cc = _banded(shape, torch.float32)
    coef, b_coef = _banded((4,) + tuple(shape), torch.float64)
    force, b_force = _banded((3,) + tuple(shape), torch.float32)
    st, b_st = _banded((2,), torch.float64)
    tF, tW, tu = _t(F), _t(W), _t(u)
    kw = dict(mask_fixed=_tm(WF), mask_moving=_tm(WM))
    hip.lncc(tF, tW, tu, r, mshape, cc=cc, coef=coef, stats=st.view(torch.int64), **kw)
    hip.lncc_force(tF, tW, tu, coef, force, r, mshape, **kw)
    torch.cuda.synchronize()
    _bands_clean(dict(cc=b_cc, coef=b_coef, force=b_force, stats=b_st), "passes")
    s, c = hip.demons_stats(st.view(torch.int64))
    return cc.cpu().numpy(), coef.cpu().numpy(), float(s[0]), int(c[0]), force.cpu().numpy()


def _against_restatement(hip, F, W, u, mshape, r, WF, WM, what):
    cc, coef, s, c, force = _passes(hip, F, W, u, mshape, r, WF, WM)
    want_cc, want_coef, want_s, want_c, _ = lr.ref_lncc(F, W, u, mshape, r, WF, WM)
    _bits(cc, want_cc, what + ": cc map")
    _bits(coef, want_coef, what + ": coefficients")
    _check_sum(s, c, want_s, want_c, what)
    _bits(force, lr.ref_force(F, W, u, mshape, r, want_coef, WF, WM), what + ": force")
    return cc, coef, s, c, force


# ---- 1. the two passes against the restatement ----------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("shape,mshape,r", CASES, ids=IDS)
def test_passes_bit_exact_against_restatement(hip, shape, mshape, r, masked):
    F, W, _, u, WF, WM = _case(shape, mshape, 100 + shape[0] + r, AMP.get(shape, 3.0))
    if not masked:
        WF = WM = None
    v = lr.valid(u, mshape, WF, WM)
    assert v.any() and not v.all()                            # samples inside and outside
    got = _against_restatement(hip, F, W, u, mshape, r, WF, WM, "%s r %d %s" % (shape, r, masked))
    if shape == (9, 11, 70):
        assert got[3] > 100 and np.abs(got[4]).max() > 0
    if not masked:
        # all-in masks write the plain run's bytes: all ones, and the lowest values that are in (0.5f) beside ones
        for WFi, WMi in ((np.ones(shape, F32), np.ones(mshape, F32)), (np.ones(shape, F32), np.full(mshape, 0.5, F32))):
            ones = _passes(hip, F, W, u, mshape, r, WFi, WMi)
            for a, b, name in zip(got, ones, ("cc", "coef", "sum", "count", "force")):
                if isinstance(a, np.ndarray):
                    _bits(b, a, "all-in masks: " + name)
                else:
                    assert a == b, name


def test_optional_outputs(hip):
    """d_cc and d_coef may each be NULL: the record is the same bytes"""
    shape, mshape, r = CASES[1]
    F, W, _, u, _, _ = _case(shape, mshape, 7)
    tF, tW, tu = _t(F), _t(W), _t(u)
    both = hip.lncc(tF, tW, tu, r, mshape).cpu().numpy()
    cc = _t(np.zeros(shape, F32))
    only = hip.lncc(tF, tW, tu, r, mshape, cc=cc).cpu().numpy()
    assert np.array_equal(both, only)
    _bits(cc.cpu().numpy(), lr.ref_lncc(F, W, u, mshape, r)[0], "cc alone")


# ---- 2. content ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1e-30, 1e18])
def test_scaled_content(hip, scale):
    """The reading taken of "cc must stay within the double bound": the scaled copy is formed in float32, which rounds
    every input by up to 2^-24 (more where x1e-30 lands among the subnormals), so no tight bound between the scaled and
    the unscaled map follows from the double arithmetic.  What is asserted: the scaled map, coefficients and force are
    the restatement's bits on the scaled inputs; the counted set is the unscaled case's; and cc stays in
    [0, 1 + 2^-20], the Cauchy-Schwarz range widened by the rounding of a counted voxel (relative terms below 2^-22,
    tests/test_lncc_host.py)."""
    shape, mshape, r = CASES[1]
    F, W, _, u, WF, WM = _case(shape, mshape, 21)
    cc0, _, s0, c0, _ = _passes(hip, F, W, u, mshape, r, WF, WM)
    Fs, Ws = (F * F32(scale)).astype(F32), (W * F32(scale)).astype(F32)
    assert np.isfinite(Fs).all() and np.isfinite(Ws).all()
    cc1, coef1, s1, c1, force1 = _against_restatement(hip, Fs, Ws, u, mshape, r, WF, WM, "scale %g" % scale)
    assert c1 == c0 > 100 and np.array_equal(cc1 != 0, cc0 != 0)       # the counted set is the unscaled case's
    assert np.isfinite(coef1).all() and np.isfinite(force1).all()
    # cc within the double bound of the restatement: it is the restatement's bits (above), and at most 1 + rounding
    assert 0.0 <= cc1.min() and cc1.max() <= 1.0 + 2.0 ** -20


def test_constant_half_and_zero_background(hip):
    shape, mshape, r = CASES[1]
    F, W, _, u, _, _ = _case(shape, mshape, 22, amp=1.0)
    F[:, :, :35] = F32(3.25)                                  # an exactly constant half
    W[:4] = F32(0.0)                                          # exact-zero background
    cc, coef, s, c, force = _against_restatement(hip, F, W, u, mshape, r, None, None, "constant half")
    assert not cc[:, :, :33].any() and not coef[:, :, :, :33].any() and not cc[:2].any()
    assert c > 0 and np.isfinite(force).all() and np.isfinite(coef).all()
    z = np.zeros(shape, F32)
    cc, coef, s, c, force = _against_restatement(hip, z, z, u, mshape, r, None, None, "all zero")
    assert (s, c) == (0.0, 0) and not force.view(np.uint32).any() and not coef.view(np.uint64).any()


# ---- 3. field_normalize ----------------------------------------------------------------------------------------------
def _normalize(hip, phi, step):
    import torch
    f, bands = _banded(phi.shape, torch.float32)
    f.copy_(_t(phi))
    hip.field_normalize(f, step)
    torch.cuda.synchronize()
    _bands_clean(dict(field=bands), "field_normalize")
    return f.cpu().numpy()


@pytest.mark.parametrize("shape", [(9, 11, 70), (3, 2, 5), (64, 64, 65)])
def test_field_normalize(hip, shape):
    rng = np.random.default_rng(31)
    phi = rng.normal(0, 2, (3,) + shape).astype(F32)
    for step in (0.5, 3.0):
        _bits(_normalize(hip, phi, step), lr.ref_normalize(phi, step), "normalize %s step %g" % (shape, step))
    z = np.zeros_like(phi)
    z[1, 0, 0, 0] = F32(-0.0)
    _bits(_normalize(hip, z, 0.5), z, "an all-zero field stays as it is")
    last = (phi * F32(0.01)).astype(F32)
    last[:, -1, -1, -1] = (3.0, -4.0, 12.0)                   # the max sits in the last voxel
    got = _normalize(hip, last, 0.5)
    _bits(got, lr.ref_normalize(last, 0.5), "max in the last voxel")
    assert abs(float(np.sqrt((got[:, -1, -1, -1].astype(F64) ** 2).sum())) - 0.5) < 1e-6


# ---- 4. the driver ---------------------------------------------------------------------------------------------------
def _pyramid_case(shape, mshape, levels, seed, masked):
    rng = np.random.default_rng(seed)
    F = rng.normal(0, 1, shape).astype(F32)
    M = rng.normal(0, 1, mshape).astype(F32)
    u = rng.uniform(-3, 3, (3,) + tuple(shape)).astype(F32)
    Fs, Ms = mr.ref_pyramid(F, levels), mr.ref_pyramid(M, levels)
    WFs = WMs = None
    if masked:
        WFs = mr.ref_pyramid((rng.random(shape) < 0.8).astype(F32), levels)
        WMs = mr.ref_pyramid((rng.random(mshape) < 0.8).astype(F32), levels)
    return Fs, Ms, u, WFs, WMs


def _drive(hip, Fs, Ms, u, its, r, step, sigmas, update, K, WFs, WMs, work=None):
    """(field, sums, counts, stats bytes) of one driver run on the device"""
    import torch
    field = _t(u)
    st = hip.demons_lncc([_t(a) for a in Fs], [_t(a) for a in Ms], field, its, r, step, sigmas[0], sigmas[1],
                         work=work, update=update, squarings=K,
                         masks_fixed=None if WFs is None else [_tm(w) for w in WFs],
                         masks_moving=None if WMs is None else [_tm(w) for w in WMs])
    s, c = hip.demons_stats(st)
    return field.cpu().numpy(), s, c, st.cpu().numpy()


DRIVER = {
    "flat-additive": dict(shape=(9, 11, 70), mshape=(10, 9, 67), levels=1, its=[3], update="additive", K=0, masked=False),
    "flat-diffeomorphic": dict(shape=(9, 11, 70), mshape=(10, 9, 67), levels=1, its=[3], update="diffeomorphic", K=2,
                               masked=False),
    "two-levels": dict(shape=(12, 14, 18), mshape=(13, 12, 17), levels=2, its=[2, 2], update="additive", K=0,
                       masked=False),
    "two-levels-masked": dict(shape=(12, 14, 18), mshape=(13, 12, 17), levels=2, its=[2, 2], update="additive", K=0,
                              masked=True),
}
SIGMAS = (1.0, 1.5)


@pytest.fixture(scope="module")
def driven(oracle_mod):
    """every driver case and the restatement's result for it, computed once"""
    out = {}
    for name, d in DRIVER.items():
        Fs, Ms, u, WFs, WMs = _pyramid_case(d["shape"], d["mshape"], d["levels"], 40 + len(name), d["masked"])
        want, per = lr.ref_multires_lncc(Fs, Ms, u, d["its"], 2, 0.5, SIGMAS[0], SIGMAS[1], oracle_mod, WFs, WMs,
                                         d["update"], d["K"])
        out[name] = (Fs, Ms, u, WFs, WMs, want, per)
    return out


@pytest.mark.parametrize("name", sorted(DRIVER))
def test_driver_bit_exact_against_restatement(hip, driven, name):
    d = DRIVER[name]
    Fs, Ms, u, WFs, WMs, want, per = driven[name]
    got, s, c, _ = _drive(hip, Fs, Ms, u, d["its"], 2, 0.5, SIGMAS, d["update"], d["K"], WFs, WMs)
    _bits(got, want, name)
    assert len(s) == sum(d["its"]) == len(per)
    for k, (ws, wc) in enumerate(per):
        _check_sum(float(s[k]), int(c[k]), ws, wc, "%s record %d" % (name, k))
    assert per[0][1] > 0 and not np.array_equal(want, u)
    step = np.sqrt(((want.astype(F64) - u) ** 2).sum(0)).max()
    assert step > 0.1                                         # the field moved


@pytest.mark.parametrize("name", ["flat-diffeomorphic", "two-levels-masked"])
def test_driver_scratch_of_exactly_the_librarys_size(hip, driven, name):
    """work of exactly sift3d_amd_demons_lncc_work_floats floats between poisoned guard bands, dirty from the run
    before: the same bytes as with the wrapper's own buffer, nothing written into the bands, one float less refused"""
    import torch
    d = DRIVER[name]
    Fs, Ms, u, WFs, WMs, want, _ = driven[name]
    nz, ny, nx = d["shape"]
    need = hip.lib().sift3d_amd_demons_lncc_work_floats(nx, ny, nz, hip.DEMONS_UPDATE[d["update"]], d["levels"])
    assert need > 0
    args = (hip, Fs, Ms, u, d["its"], 2, 0.5, SIGMAS, d["update"], d["K"], WFs, WMs)
    ref_st = _drive(*args)[3]
    with pytest.raises(ValueError):
        _drive(*args, work=torch.empty(need - 1, device="cuda"))
    for fill in (0xFF, 0x00):
        G = (4 * need + 15) // 16 * 16
        whole = torch.full((G + 4 * need + G,), fill, dtype=torch.uint8, device="cuda")
        work = whole[G:G + 4 * need].view(torch.float32)
        assert work.data_ptr() % 16 == 0
        for run in ("first", "second"):
            got, _, _, st = _drive(*args, work=work)
            torch.cuda.synchronize()
            spilt = [int((b != fill).sum()) for b in (whole[:G], whole[G + 4 * need:])]
            assert spilt == [0, 0], (run, fill, spilt)
            _bits(got, want, "%s run on work of 0x%02X" % (run, fill))
            assert np.array_equal(st, ref_st)


def test_driver_on_a_side_stream_behind_queued_work(hip, driven):
    import torch
    name = "flat-additive"
    d = DRIVER[name]
    Fs, Ms, u, _, _, want, _ = driven[name]
    delay = torch.ones((128, 512, 512), device="cuda")
    twins = [torch.zeros_like(_t(a)) for a in (Fs[0], Ms[0], u)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    try:
        with torch.cuda.stream(s):
            hip.current_stream(refresh=True)
            for _ in range(20):
                delay.mul_(1.0001)
            for twin, real in zip(twins, (Fs[0], Ms[0], u)):
                twin.copy_(_t(real), non_blocking=True)
            st = hip.demons_lncc([twins[0]], [twins[1]], twins[2], d["its"], 2, 0.5, SIGMAS[0], SIGMAS[1])
            got = twins[2].clone()
        hip.current_stream(refresh=True)
        torch.cuda.current_stream().wait_stream(s)
        _bits(got.cpu().numpy(), want, "side stream")
        assert st.numel() == 2 * d["its"][0]
    finally:
        hip.current_stream(refresh=True)


# ---- 5. what it must achieve -----------------------------------------------------------------------------------------
def bias_pair(n=32, seed=5):
    """(fixed, moving, d): moving = smooth blobs; d a sinusoidal displacement of about 1.5 voxels; fixed = moving pulled
    through d, times a 0.6 -> 1.4 ramp along x, plus a ramp along y: a spatially varying intensity relation"""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    M = np.zeros((n, n, n), F64)
    for _ in range(60):
        c = rng.uniform(2, n - 2, 3)
        s = rng.uniform(1.5, 3.0)
        M += rng.uniform(0.3, 1.0) * np.exp(-((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) / (2 * s * s))
    M = (100.0 * M / M.max()).astype(F32)
    w = 2.0 * np.pi / n
    d = np.stack([1.5 * np.sin(w * y) * np.cos(w * z), 1.5 * np.sin(w * z) * np.cos(w * x),
                  1.5 * np.sin(w * x) * np.cos(w * y)]).astype(F32)
    pulled = fr.ref_warp_field(M, d, "linear", 0.0).astype(F64)
    gain = 0.6 + 0.8 * x / (n - 1.0)
    fixed = (pulled * gain + 30.0 * y / (n - 1.0)).astype(F32)
    return fixed, M, d


def field_error(u, d, lo=4, hi=28):
    """the mean of |u - d| over the interior [lo, hi)^3"""
    e = np.sqrt(((np.asarray(u, F64) - np.asarray(d, F64)) ** 2).sum(0))
    return float(e[lo:hi, lo:hi, lo:hi].mean())


# (sigma_fluid 2, sigma_diffusion 1: with refine_field's demons defaults 1 and 2 the restatement reaches 0.897 of a
# start error of 1.247 on this pair in 40 iterations, with these 0.467)
ACHIEVE = dict(radius=2, step=0.5, iterations=40, sigma_fluid=2.0, sigma_diffusion=1.0)


def test_lncc_refinement_recovers_a_displacement_under_a_bias_field(hip, oracle_mod):
    """The yardstick is the restatement's driver on the CPU: it must bring the mean interior field error below half
    the start error, and the device must be within 1.5 x of it (DESIGN 3.4.9's margin; at this size they agree in
    bits).  force="demons" on the same pair is printed for the record, not asserted."""
    from sift3d_amd import api
    fixed, moving, d = bias_pair()
    zero = np.zeros_like(d)
    start = field_error(zero, d)
    want, per = lr.ref_demons_lncc(fixed, moving, zero, ACHIEVE["iterations"], ACHIEVE["radius"], ACHIEVE["step"],
                                   ACHIEVE["sigma_fluid"], ACHIEVE["sigma_diffusion"], oracle_mod)
    ref_err = field_error(want, d)
    r = api.refine_field(_t(moving), _t(fixed), features="intensity", force="lncc", **ACHIEVE)
    assert isinstance(r, api.LnccRefinement) and r.lncc.shape == (ACHIEVE["iterations"],)
    got = r.field.cpu().numpy()
    dev_err = field_error(got, d)
    dem = api.refine_field(_t(moving), _t(fixed), features="intensity", iterations=ACHIEVE["iterations"])
    print("mean interior field error: start %.4f, restatement %.4f, device %.4f, force='demons' %.4f; "
          "mean cc %.4f -> %.4f; fields agree in bits: %s"
          % (start, ref_err, dev_err, field_error(dem.field.cpu().numpy(), d), r.lncc[0], r.lncc[-1],
             np.array_equal(got.view(np.uint32), want.view(np.uint32))))
    assert ref_err < 0.5 * start, (ref_err, start)
    assert dev_err <= 1.5 * ref_err, (dev_err, ref_err)
    assert r.lncc[-1] > r.lncc[0]
    assert abs(r.lncc[0] - per[0][0] / per[0][1]) <= 1e-12
    assert r.jacobian.folded == 0
    _bits(r.warped.cpu().numpy(), fr.ref_warp_field(moving, got, "linear", 0.0), "warped")


def test_refine_field_levels_and_default_path(hip, oracle_mod):
    """levels > 1 returns MultiresLnccRefinement with the driver's fields; force 'demons' is today's path"""
    from sift3d_amd import api
    Fs, Ms, u, _, _ = _pyramid_case((12, 14, 18), (13, 12, 17), 2, 3, False)
    r = api.refine_field(_t(Ms[0]), _t(Fs[0]), _t(u), features="intensity", force="lncc", radius=1, step=0.25,
                         levels=2, level_iterations=[2, 1], sigma_fluid=1.0, sigma_diffusion=1.5,
                         update="diffeomorphic", squarings=1)
    assert isinstance(r, api.MultiresLnccRefinement)
    assert r.level_slices == (slice(1, 3), slice(0, 1)) and r.lncc.shape == (3,)
    want, per = lr.ref_multires_lncc(Fs, Ms, u, [2, 1], 1, 0.25, 1.0, 1.5, oracle_mod, update="diffeomorphic",
                                     squarings=1)
    _bits(r.field.cpu().numpy(), want, "refine_field, two levels")
    a = api.refine_field(_t(Ms[0]), _t(Fs[0]), _t(u), 2, features="intensity")
    b = api.refine_field(_t(Ms[0]), _t(Fs[0]), _t(u), 2, features="intensity", force="demons", radius=4, step=9.0)
    assert isinstance(a, api.DemonsRefinement) and isinstance(b, api.DemonsRefinement)
    _bits(a.field.cpu().numpy(), b.field.cpu().numpy(), "force='demons' ignores the new keywords")


# ---- 6. api.local_ncc ------------------------------------------------------------------------------------------------
def test_local_ncc_through_each_transform(hip):
    from sift3d_amd import api
    rng = np.random.default_rng(50)
    shape, mshape = (9, 11, 20), (10, 9, 22)
    F = rng.normal(0, 1, shape).astype(F32)
    M = rng.normal(0, 1, mshape).astype(F32)
    A = np.array([[1.0, 0.02, 0.0, 0.75], [0.0, 0.98, 0.03, -0.5], [0.01, 0.0, 1.0, 0.25]])
    src = rng.uniform(2, 8, (12, 3))
    tps = api.tps_fit(src, src + rng.normal(0, 0.4, src.shape), smoothing=0.1)
    fld = rng.uniform(-2, 2, (3,) + shape).astype(F32)
    WF = rng.random(shape) < 0.8
    for name, T in (("affine", A), ("tps", tps), ("field", fld), ("cuda field", _t(fld))):
        u = T.cpu().numpy() if name == "cuda field" else (
            fld if name == "field" else api.displacement_field(T, shape).cpu().numpy())
        W = fr.ref_warp_field(M, u, "linear", 0.0)
        for r, mask in ((1, None), (2, WF)):
            got = api.local_ncc(F, M, T, radius=r, mask_fixed=mask, return_map=True)
            wf = None if mask is None else mask.astype(F32)
            cc, _, s, c, _ = lr.ref_lncc(F, W, u, mshape, r, wf, None)
            assert got.count == c > 0, name
            assert abs(got.value - s / c) <= 2 * lr.gamma(c) * s / c, name
            _bits(got.map.cpu().numpy(), cc, "local_ncc map, " + name)
    same = api.local_ncc(F, F, radius=2)                      # the identity: every counted voxel scores 1
    assert same.map is None and same.count == F.size and abs(same.value - 1.0) < 1e-12
    none = api.local_ncc(F, M, np.array([[1.0, 0, 0, 100.0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]]), radius=2)
    assert none.count == 0 and np.isnan(none.value)
