"""CPU (not gpu): the host side of multi-resolution demons -- the exported symbols, the work size, every refusal of
the new entries (checked before any device call) -- and the numpy restatement (tests/multires_restatement.py)
against analysis: restriction of constants and ramps, prolongation of constant and affine fields, the even-voxel
identity, one level against the single-level restatements, and the capture-range case that three levels solve at a
lower cost than one."""
import numpy as np
import pytest

from tests import demons_restatement as dm
from tests import field_algebra_restatement as fa
from tests import field_restatement as fr
from tests import multires_restatement as mr

F32 = np.float32


@pytest.fixture(scope="module")
def api():
    from sift3d_amd import api as a
    a.lib()
    return a


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


EXPORTED = ["sift3d_hip_restrict2", "sift3d_hip_field_prolong2", "sift3d_amd_demons_multires_work_floats",
            "sift3d_amd_demons_multires_device"]


def test_symbols_exported(api):
    from sift3d_amd import _native, hip
    L = _native.load()
    for name in EXPORTED:
        assert hasattr(L, name), name
    hip.lib()
    for name in ("restrict2", "field_prolong2", "demons_multires", "half_shape"):
        assert callable(getattr(hip, name))
    for name in ("restrict_volume", "prolong_field", "refine_field", "register_dense"):
        assert callable(getattr(api, name))
    assert api.MultiresRefinement._fields == ("field", "warped", "msd", "jacobian", "level_slices")
    assert api.MultiresRegistration._fields == api.DenseRegistration._fields + ("level_slices",)
    assert api.DEMONS_MAX_LEVELS == hip.DEMONS_MAX_LEVELS == 6
    assert hip.half_shape((5, 4, 1)) == (3, 2, 1) == mr.half_shape((5, 4, 1))


def _pad4(n):
    return (n + 3) // 4 * 4


def test_work_floats(api):
    from sift3d_amd import hip
    L = hip.lib()
    f = L.sift3d_amd_demons_multires_work_floats
    for upd in (0, 1):
        base = L.sift3d_amd_demons_work_floats_ex(37, 29, 23, 12, upd)
        assert f(37, 29, 23, 12, upd, 1) == _pad4(base)
        n1, n2, n3 = 19 * 15 * 12, 10 * 8 * 6, 5 * 4 * 3
        assert f(37, 29, 23, 12, upd, 2) == _pad4(base) + _pad4(3 * n1)
        assert f(37, 29, 23, 12, upd, 4) == _pad4(base) + _pad4(3 * n1) + _pad4(3 * n2) + _pad4(3 * n3)
    # axes of 1 stay 1
    assert f(1, 5, 1, 2, 0, 3) == _pad4(L.sift3d_amd_demons_work_floats_ex(1, 5, 1, 2, 0)) + _pad4(9) + _pad4(6)
    for bad in ((0, 8, 8, 1, 0, 2), (8, 8, 8, 0, 0, 2), (8, 8, 8, 1, 2, 2), (8, 8, 8, 1, 0, 0), (8, 8, 8, 1, 0, 7),
                (8, 8, 8, 1, 0, -1)):
        assert f(*bad) == 0, bad


def test_restrict2_refusals(bufs):
    from sift3d_amd import hip
    L = hip.lib()
    A, B, _ = bufs

    def run(**ch):
        a = dict(src=A, nx=8, ny=8, nz=8, nc=3, dst=B, scale=1.0)
        a.update(ch)
        return L.sift3d_hip_restrict2(a["src"], a["nx"], a["ny"], a["nz"], a["nc"], a["dst"], a["scale"], None)

    for ch in (dict(src=None), dict(dst=None), dict(nx=0), dict(ny=-1), dict(nz=0), dict(nc=0), dict(nc=-3),
               dict(scale=float("nan")), dict(scale=float("inf")), dict(src=A + 2), dict(dst=B + 1),
               dict(dst=A),                                                 # in place
               dict(dst=A + 4 * 1000),                                      # dst inside src (3 * 512 floats)
               dict(dst=A - 4 * 100),                                       # dst (3 * 64 floats) runs into src
               dict(dst=A + 4 * 1535)):                                     # src's last float
        assert run(**ch) == -1, ch


def test_prolong2_refusals(bufs):
    from sift3d_amd import hip
    L = hip.lib()
    A, B, _ = bufs

    def run(**ch):
        a = dict(coarse=A, fine=B, nx=8, ny=8, nz=8)
        a.update(ch)
        return L.sift3d_hip_field_prolong2(a["coarse"], a["fine"], a["nx"], a["ny"], a["nz"], None)

    for ch in (dict(coarse=None), dict(fine=None), dict(nx=0), dict(ny=-1), dict(nz=0), dict(coarse=A + 2),
               dict(fine=B + 1),
               dict(fine=A),                                                # in place
               dict(fine=A + 4 * 191),                                      # the coarse field's last float (3 * 64)
               dict(fine=A - 4 * 1000),                                     # fine (3 * 512 floats) runs into coarse
               dict(coarse=B + 4 * 1535)):                                  # coarse starts at fine's last float
        assert run(**ch) == -1, ch


def _levels(hip, A, dims, mdims, its):
    """a level table with F_l, M_l at 1 KiB steps of buffer A beyond level 0's 4 KiB pair"""
    tab = (hip.DemonsLevel * len(dims))()
    for l, ((nx, ny, nz), (mx, my, mz)) in enumerate(zip(dims, mdims)):
        f = A if l == 0 else A + 8192 + 2048 * (l - 1)
        m = A + 4096 if l == 0 else A + 8192 + 2048 * (l - 1) + 1024
        tab[l] = hip.DemonsLevel(f, nx, ny, nz, m, mx, my, mz, its[l])
    return tab


@pytest.mark.parametrize("upd", [0, 1])
def test_multires_refusals(bufs, upd):
    from sift3d_amd import hip
    L = hip.lib()
    A, B, W = bufs
    dims = [(8, 8, 8), (4, 4, 4), (2, 2, 2)]
    mdims = [(7, 6, 5), (4, 3, 3), (2, 2, 2)]
    work = 4 * L.sift3d_amd_demons_multires_work_floats(8, 8, 8, 1, upd, 3)
    assert 0 < work < (1 << 18)

    def run(tab_ch=None, **ch):
        a = dict(levels=3, nc=1, u=B, alpha=1.0, sf=1.0, sd=1.0, upd=upd, K=2, work=W, stats=B + 8192, tab=True)
        a.update(ch)
        tab = _levels(hip, A, dims, mdims, [3, 3, 3])
        for (l, field), v in (tab_ch or {}).items():
            setattr(tab[l], field, v)
        return L.sift3d_amd_demons_multires_device(tab if a["tab"] else None, a["levels"], a["nc"], a["u"],
                                                   a["alpha"], a["sf"], a["sd"], a["upd"], a["K"], a["work"],
                                                   a["stats"], None)

    for ch in (dict(tab=False), dict(u=None), dict(work=None), dict(stats=None),
               dict(levels=0), dict(levels=-1), dict(levels=7), dict(levels=1 << 20),
               dict(nc=0), dict(upd=2), dict(upd=-1), dict(K=-1), dict(K=21),
               dict(alpha=0.0), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(sf=-0.1),
               dict(sd=float("inf")), dict(sf=float("nan")),
               dict(stats=B + 8196), dict(work=W + 4), dict(u=B + 2),
               dict(u=A + 4 * 100),                                         # u over F_0
               dict(u=A + 8192 - 4 * 1000),                                 # u runs into F_1
               dict(work=B),                                                # the work buffer over u
               dict(work=A + 8192 + 4096 - work + 8),                       # the work buffer's end over F_2
               dict(stats=B + 4 * 1000),                                    # stats inside u
               dict(stats=W + work - 16),                                   # stats inside the last level field
               dict(stats=A + 4096 - 9 * 16 + 16)):                         # the 9th record over M_0
        assert run(**ch) == -1, ch
    for tab_ch in ({(0, "d_F"): None}, {(2, "d_M"): None}, {(1, "d_F"): None},
                   {(1, "d_F"): A + 8192 + 2}, {(2, "d_M"): A + 8192 + 3072 + 1},
                   {(0, "nx"): 0}, {(1, "ny"): -4}, {(2, "mz"): 0},
                   {(1, "nx"): 5}, {(1, "ny"): 3}, {(2, "nz"): 1}, {(2, "nx"): 3},    # not the halving chain
                   {(1, "mx"): 3}, {(1, "my"): 4}, {(2, "mz"): 1},                    # ... of the moving grid
                   {(0, "nx"): 6}, {(0, "mz"): 7},                                    # level 0 changed under level 1
                   {(0, "iterations"): -1}, {(2, "iterations"): -5},
                   {(1, "d_F"): B + 4 * 10},                                          # F_1 inside u
                   {(2, "d_M"): W + work - 32}):                                      # M_2 inside the work buffer
        assert run(tab_ch) == -1, tab_ch


def test_python_refusals(api):
    from sift3d_amd import hip
    vol = np.zeros((3, 5, 6, 7), np.float32)
    for call in (lambda: api.restrict_volume(vol), lambda: api.prolong_field(vol, (10, 12, 14)),
                 lambda: hip.restrict2(vol), lambda: hip.field_prolong2(vol, vol),
                 lambda: hip.demons_multires([vol], [vol], vol, [1], 1.0),
                 lambda: api.refine_field(vol[0], vol[0], levels=2)):
        with pytest.raises(ValueError):
            call()


# ---- the restatement against analysis -------------------------------------------------------------------------
def _eq(a, b):
    return np.array_equal(np.ascontiguousarray(a, F32).view(np.uint32), np.ascontiguousarray(b, F32).view(np.uint32))


SHAPES = [(23, 29, 37), (24, 30, 36), (1, 29, 2), (3, 2, 1), (2, 1, 3), (1, 1, 1)]      # (nz, ny, nx)


@pytest.mark.parametrize("shape", SHAPES)
def test_restriction_of_a_constant_is_exact(shape):
    """every tap is the constant c: 0.25 c + 0.5 c = 0.75 c and 0.75 c + 0.25 c = c are exact for a c with spare low
    bits, on clamped faces too; the scale 0.5 halves it exactly"""
    for c in (3.25, -100.0, 0.0):
        a = np.full((2,) + shape, c, F32)
        assert _eq(mr.ref_restrict(a), np.full((2,) + mr.half_shape(shape), c, F32))
        assert _eq(mr.ref_restrict(a, 0.5), np.full((2,) + mr.half_shape(shape), c / 2, F32))


def test_restriction_of_a_ramp_is_the_ramp_at_even_voxels():
    """a x + b y + c z + d with small integer coefficients: every product and sum is a small dyadic number, exact in
    float; away from the clamped faces (tap 2 i + 1 on the grid: the low face's clamped tap is -1 -> 0, which only
    voxel 0 has) the binomial of a linear function is its centre value"""
    shape = (23, 30, 37)
    x, y, z = fr.grid(shape)
    ramp = (3 * x - 2 * y + 5 * z + 7).astype(F32)
    got = mr.ref_restrict(ramp)
    cz, cy, cx = mr.half_shape(shape)
    assert got.shape == (cz, cy, cx)
    want = ramp[::2, ::2, ::2]
    # inner: i >= 1 and 2 i + 1 <= n - 1 per axis
    hz, hy, hx = [(n - 2) // 2 for n in shape]
    assert hz >= 5 and hy >= 5 and hx >= 5
    assert _eq(got[1:hz + 1, 1:hy + 1, 1:hx + 1], want[1:hz + 1, 1:hy + 1, 1:hx + 1])
    # on the low x face the clamped tap pulls the value up by a / 4 = 0.75
    assert _eq(got[1:hz + 1, 1:hy + 1, 0], want[1:hz + 1, 1:hy + 1, 0] + F32(0.75))


@pytest.mark.parametrize("shape", SHAPES)
def test_prolongation_of_a_constant_field_doubles_it(shape):
    c = np.array([3.25, -11.5, 0.7], F32)
    u = np.broadcast_to(c[:, None, None, None], (3,) + mr.half_shape(shape)).astype(F32)
    want = np.broadcast_to((c * F32(2))[:, None, None, None], (3,) + shape).astype(F32)
    assert _eq(mr.ref_prolong(u, shape), want)


def test_prolongation_of_an_affine_field():
    """u_c(i) = (A - I) i + t on the coarse grid, A and t dyadic: the fine field is (A - I) p + 2 t, the same map seen
    from the fine grid, exactly (every value is a small dyadic number), where p / 2 is inside the coarse grid"""
    shape = (22, 27, 36)
    B = np.array([[0.25, -0.125, 0.5], [0.0, 0.375, -0.25], [-0.5, 0.125, 0.0625]])          # A - I
    t = np.array([1.5, -2.25, 0.75])
    cshape = mr.half_shape(shape)
    x, y, z = fr.grid(cshape)
    uc = np.stack([B[d, 0] * x + B[d, 1] * y + B[d, 2] * z + t[d] for d in range(3)]).astype(F32)
    X, Y, Z = fr.grid(shape)
    want = np.stack([B[d, 0] * X + B[d, 1] * Y + B[d, 2] * Z + 2 * t[d] for d in range(3)]).astype(F32)
    got = mr.ref_prolong(uc, shape)
    # inside: p <= 2 (c - 1) per axis (all of an odd axis, all but the last voxel of an even one)
    nz, ny, nx = [2 * (c - 1) + 1 for c in cshape]
    assert (nz, ny, nx) == (21, 27, 35)
    assert _eq(got[:, :nz, :ny, :nx], want[:, :nz, :ny, :nx])
    # the clamped high face of an even axis repeats the last coarse voxel's value
    assert _eq(got[:, 21], got[:, 20]) and _eq(got[:, :, :, 35], got[:, :, :, 34])


@pytest.mark.parametrize("shape", SHAPES)
def test_prolongation_sampled_at_even_voxels_returns_the_field(shape):
    """0.5 R(P(u)) is u only up to the binomial's smoothing; P(u) at the even voxels, halved, is u bit for bit:
    0.5f (a + a) = a on every axis and 2 a / 2 = a"""
    rng = np.random.default_rng(5)
    u = rng.normal(0, 3, (3,) + mr.half_shape(shape)).astype(F32)
    fine = mr.ref_prolong(u, shape)
    assert fine.shape == (3,) + shape
    assert _eq(fine[:, ::2, ::2, ::2] * F32(0.5), u)


@pytest.mark.parametrize("update", ["additive", "diffeomorphic"])
def test_one_level_is_the_single_level_restatement(oracle_mod, update):
    rng = np.random.default_rng(3)
    F = rng.normal(0, 1, (2, 9, 10, 11)).astype(F32)
    M = rng.normal(0, 1, (2, 8, 11, 10)).astype(F32)
    u = rng.normal(0, 1, (3, 9, 10, 11)).astype(F32)
    got, per = mr.ref_multires([F], [M], u, [3], 0.7, 1.0, 1.5, oracle_mod, update, 2)
    if update == "additive":
        want, wper = dm.ref_demons(F, M, u, 3, 0.7, 1.0, 1.5, oracle_mod)
    else:
        want, wper = fa.ref_demons_diffeo(F, M, u, 3, 0.7, 1.0, 1.5, 2, oracle_mod)
    assert _eq(got, want) and len(per) == len(wper) == 3
    for (sd, ins), (wsd, wins) in zip(per, wper):
        assert np.array_equal(sd, wsd) and np.array_equal(ins, wins)


# ---- what the pyramid must achieve: capture range ---------------------------------------------------------------
# The restatement's own values on multires_restatement.capture_case() (intensity, additive, from zero, alpha 1,
# sigma_fluid 1, sigma_diffusion 1; |u - d| over [6, 42)^3; cost in level-0 iterations):
#   zero field                               cost 0     median 3.076  p90 4.884
#   1 level, 20 iterations                   cost 20    median 0.789  p90 4.041  last msd 222.8  folds 0
#   3 levels, 16 / 20 / 20 (level 0 / 1 / 2) cost 18.8  median 0.176  p90 0.479  last msd 47.4   folds 0
#   1 level, 100 iterations                  cost 100   median 0.166  p90 0.363  last msd 43.6
CAPTURE_ITERATIONS = (16, 20, 20)


def capture_runs(run):
    """the three runs of the capture-range case through run(Fs, Ms, iterations) -> (field, last msd)"""
    from oracle import sift3d_oracle as so
    F, M, d, kw = mr.capture_case(so)
    Fs, Ms = mr.ref_pyramid(F, 3), mr.ref_pyramid(M, 3)
    u1, m1 = run([F], [M], [20], kw)
    u3, m3 = run(Fs, Ms, list(CAPTURE_ITERATIONS), kw)
    u100, m100 = run([F], [M], [100], kw)
    return d, (u1, m1), (u3, m3), (u100, m100)


def check_capture(d, one, three, hundred, what):
    """the conditions of the capture-range case, with room under what the restatement gives (median 4.5x, p90 8.4x
    better, last msd 1.09x the 100-iteration run's)"""
    (u1, m1), (u3, m3), (u100, m100) = one, three, hundred
    med1, p1 = mr.capture_error(u1, d)
    med3, p3 = mr.capture_error(u3, d)
    med100, p100 = mr.capture_error(u100, d)
    folds1 = fr.ref_stats(fr.ref_jacobian_det(u1))[0]
    folds3 = fr.ref_stats(fr.ref_jacobian_det(u3))[0]
    print("%s: zero %.3f / %.3f; 1 level x 20: median %.3f p90 %.3f msd %.1f folds %d; 3 levels %s: median %.3f "
          "p90 %.3f msd %.1f folds %d; 1 level x 100: median %.3f p90 %.3f msd %.1f"
          % ((what,) + mr.capture_error(np.zeros_like(d), d) + (med1, p1, m1, folds1, CAPTURE_ITERATIONS, med3, p3,
                                                                m3, folds3, med100, p100, m100)))
    assert CAPTURE_ITERATIONS[0] + CAPTURE_ITERATIONS[1] / 8 + CAPTURE_ITERATIONS[2] / 64 < 20
    assert med3 <= 0.5 * med1
    assert p3 <= 0.25 * p1
    assert med3 <= 0.25
    assert folds1 == 0 and folds3 == 0
    assert m3 <= 1.25 * m100


def test_three_levels_capture_what_one_level_cannot(oracle_mod):
    def run(Fs, Ms, its, kw):
        u0 = np.zeros((3,) + Fs[0].shape, F32)
        u, per = mr.ref_multires(Fs, Ms, u0, its, so=oracle_mod, **kw)
        return u, mr.last_msd(per)

    d, one, three, hundred = capture_runs(run)
    check_capture(d, one, three, hundred, "restatement")
