"""Log-domain demons without a device (include/sift3d_amd.h, "Log-domain demons"): the restatement against analysis,
the antisymmetry of the symmetric driver, and the C entries' refusals and size formulas through ctypes."""
import numpy as np
import pytest

from tests import field_algebra_restatement as fa
from tests import logdemons_restatement as ld

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


def _bits(got, want, what):
    got = np.ascontiguousarray(got, F32)
    want = np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%s: %d of %d values differ" % (what, int(bad.sum()), bad.size)


def _random_pair(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 1, (3,) + shape).astype(F32), rng.normal(0, 1, (3,) + shape).astype(F32))


def _linear_field(A, shape, centre=(0.0, 0.0, 0.0)):
    """a_d(p) = sum_e A[d][e] (p_e - centre_e) on a grid (nz, ny, nx), float64"""
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    p = (x - centre[0], y - centre[1], z - centre[2])
    return np.stack([A[d][0] * p[0] + A[d][1] * p[1] + A[d][2] * p[2] for d in range(3)])


# ---- 1. the restatement against analysis -------------------------------------------------------------------------
SHAPES = [(7, 6, 5), (5, 1, 2), (1, 1, 1)]                   # (nz, ny, nx); one with an axis of 1 and one of 2


@pytest.mark.parametrize("shape", SHAPES)
def test_bracket_with_itself_is_zero_and_antisymmetric(shape):
    a, b = _random_pair(shape, 3)
    assert not ld.ref_bracket(a, a).any()
    _bits(ld.ref_bracket(a, b), -ld.ref_bracket(b, a), "[a, b] == -[b, a]")
    const = np.broadcast_to(np.array([1.5, -2.25, 0.75], F32)[:, None, None, None], (3,) + shape)
    const2 = np.broadcast_to(np.array([-0.5, 4.0, 3.0], F32)[:, None, None, None], (3,) + shape)
    assert not ld.ref_bracket(const, const2).any()


@pytest.mark.parametrize("shape", SHAPES)
def test_bch1_is_the_sum_plus_half_the_bracket(shape):
    a, b = _random_pair(shape, 4)
    _bits(ld.ref_bracket(a, b, "bch1"), (a + b) + F32(0.5) * ld.ref_bracket(a, b), "bch1")


def test_bracket_of_linear_fields_is_the_commutator():
    """a = A p, b = B p with dyadic entries: every difference and product is exact in float32, so [a, b] is
    (A B - B A) p at every voxel, the one-sided ends included; on an axis of length 1 the derivative is 0 by
    contract, so that column of A and B is taken as zero there"""
    A = np.array([[0.5, -0.25, 1.0], [2.0, 0.125, -0.5], [-1.0, 0.75, 0.25]])
    B = np.array([[-0.75, 1.0, 0.5], [0.25, -2.0, 1.5], [0.5, 0.125, -1.0]])
    for shape in [(5, 1, 2), (4, 3, 6)]:
        a = _linear_field(A, shape).astype(F32)
        b = _linear_field(B, shape).astype(F32)
        live = np.array([shape[2] > 1, shape[1] > 1, shape[0] > 1], float)       # x, y, z
        # J_a as the contract computes it: column e is zero on an axis of length 1
        Ja, Jb = A * live[None, :], B * live[None, :]
        want = np.stack([sum(Ja[d][e] * b[e].astype(np.float64) - Jb[d][e] * a[e].astype(np.float64)
                             for e in range(3)) for d in range(3)])
        got = ld.ref_bracket(a, b)
        np.testing.assert_array_equal(got.astype(np.float64), want)
        if all(live):
            np.testing.assert_array_equal(got.astype(np.float64), _linear_field(A @ B - B @ A, shape))


def test_bch1_is_closer_to_the_composition_than_the_sum():
    """exp(BCH1(v, d)) against COMPOSE(exp v, exp d), and exp(v + d) against it: linear fields about the grid's
    centre (trilinear interpolation is exact on them away from the clamped faces), compared in float64 on the inner
    voxels"""
    shape, K = (17, 17, 17), 5
    A = np.array([[0.0, -0.0625, 0.03125], [0.0625, 0.0, 0.0], [-0.03125, 0.015625, 0.03125]])
    B = np.array([[0.03125, 0.0, -0.046875], [0.0, -0.03125, 0.0625], [0.0625, 0.0, 0.0]])
    v = _linear_field(A, shape, (8, 8, 8)).astype(F32)
    d = _linear_field(B, shape, (8, 8, 8)).astype(F32)
    want = fa.ref_compose(ld.ref_exp(v, K), ld.ref_exp(d, K))[0].astype(np.float64)
    inner = (slice(None),) + (slice(5, 12),) * 3

    def err(z):
        e = ld.ref_exp(z, K).astype(np.float64) - want
        return float(np.sqrt((e[inner] ** 2).sum(0)).max())

    e_bch, e_sum = err(ld.ref_bracket(v, d, "bch1")), err((v + d).astype(F32))
    print("max error on the inner voxels: exp(BCH1) %.3g, exp(v + d) %.3g voxel" % (e_bch, e_sum))
    assert e_sum > 1e-3                                     # the pair does not commute: there is something to gain
    assert e_bch < 0.25 * e_sum


# ---- 2. the signed exponential -----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 1, 3])
def test_signed_exp_is_exp_of_the_negated_field(K):
    v = _random_pair((6, 5, 7), 5)[0]
    _bits(ld.ref_exp(v, K, True), ld.ref_exp(-v, K), "exp(-v), K %d" % K)
    _bits(ld.ref_exp(v, K, False), fa.ref_exp(v, K), "exp(v), K %d" % K)


# ---- 3. the symmetric driver is antisymmetric --------------------------------------------------------------------
@pytest.mark.parametrize("bch", [0, 1])
def test_symmetric_driver_is_antisymmetric(oracle_mod, bch):
    """Exchanging F and M and starting from -v gives -v.  Every step commutes with exact negation of the field:
    exp(-v) of one run is exp(v') of the other bit for bit (v * -2^-K == (-v) * 2^-K), so the two forces exchange;
    gradients, products and sums negate exactly in round-to-nearest, so BCH1(-v, d_b) of one run is the other's
    BCH1(v', d_f'); and 0.5f * (Z_f - Z_b) negates when its operands exchange, except that x - x is +0 in both
    runs.  So the bits agree up to the sign of zeros, which no later step turns into a nonzero difference."""
    rng = np.random.default_rng(11)
    shape = (9, 8, 7)
    F = rng.normal(0, 1, (2,) + shape).astype(F32)
    M = (F + rng.normal(0, 0.3, F.shape)).astype(F32)
    v0 = rng.normal(0, 0.7, (3,) + shape).astype(F32)
    args = (3, 0.8, 1.0, 1.0, oracle_mod)
    v, _ = ld.ref_logdemons(F, M, v0, *args, symmetric=True, bch=bch, squarings=2)
    w, _ = ld.ref_logdemons(M, F, -v0, *args, symmetric=True, bch=bch, squarings=2)
    assert not np.array_equal(v, v0)
    _bits(ld.unsigned_zero(w), ld.unsigned_zero(-v), "swapped run, bch %d" % bch)
    # and the plain log-domain run is not antisymmetric: the check above can fail
    p, _ = ld.ref_logdemons(F, M, v0, *args, symmetric=False, bch=bch, squarings=2)
    q, _ = ld.ref_logdemons(M, F, -v0, *args, symmetric=False, bch=bch, squarings=2)
    assert not np.array_equal(q, -p)


# ---- 4. the C entries without a device ---------------------------------------------------------------------------
EXPORTED = ["sift3d_hip_field_bracket", "sift3d_amd_field_exp_signed_device", "sift3d_amd_logdemons_work_floats",
            "sift3d_amd_logdemons_device"]


def test_symbols_exported(api):
    from sift3d_amd import _native, hip
    L = _native.load()
    for name in EXPORTED:
        assert hasattr(L, name), name
    hip.lib()
    for name in ("field_bracket", "field_exp", "logdemons"):
        assert callable(getattr(hip, name))
    for name in ("lie_bracket", "field_exp", "refine_field"):
        assert callable(getattr(api, name))
    assert api.LogDemonsRefinement._fields == ("field", "inverse", "velocity", "warped", "msd", "jacobian",
                                               "inverse_jacobian", "scaled_max")
    assert api.MultiresLogDemonsRefinement._fields == api.LogDemonsRefinement._fields + ("level_slices",)


def test_work_floats(api):
    from sift3d_amd import hip
    L = hip.lib()
    for nx, ny, nz, nc in ((37, 29, 23, 12), (8, 8, 8, 1)):
        for sym in (0, 1):
            for levels in (1, 3):
                assert L.sift3d_amd_logdemons_work_floats(nx, ny, nz, nc, sym, levels) == \
                    ld.work_floats(nx, ny, nz, nc, sym, levels), (nx, ny, nz, nc, sym, levels)
    assert L.sift3d_amd_logdemons_work_floats(8, 8, 8, 1, 0, 1) == 8192 + 15 * 512
    assert L.sift3d_amd_logdemons_work_floats(8, 8, 8, 1, 1, 1) == 8192 + 4 + 21 * 512
    for bad in ((0, 8, 8, 1, 0, 1), (8, -1, 8, 1, 0, 1), (8, 8, 0, 1, 0, 1), (8, 8, 8, 0, 0, 1), (8, 8, 8, 1, 2, 1),
                (8, 8, 8, 1, -1, 1), (8, 8, 8, 1, 0, 0), (8, 8, 8, 1, 0, 7)):
        assert L.sift3d_amd_logdemons_work_floats(*bad) == 0, bad
    # the existing drivers still refuse a third update
    assert L.sift3d_amd_demons_work_floats_ex(8, 8, 8, 1, 2) == 0


FB = 3 * 512 * 4                                             # an 8^3 field: 6144 bytes


def test_bracket_refusals(bufs):
    from sift3d_amd import hip
    L = hip.lib()
    A, B, _ = bufs

    def run(**ch):
        a = dict(a=A, b=A + 8192, ox=8, oy=8, oz=8, out=B, mode=0)
        a.update(ch)
        return L.sift3d_hip_field_bracket(a["a"], a["b"], a["ox"], a["oy"], a["oz"], a["out"], a["mode"], None)

    for ch in (dict(a=None), dict(b=None), dict(out=None), dict(ox=0), dict(oy=-1), dict(oz=0), dict(mode=2),
               dict(mode=-1), dict(a=A + 2), dict(b=A + 8193), dict(out=B + 1),
               dict(out=A), dict(out=A + 8192),                             # out is an input
               dict(out=A + 4 * 100), dict(out=A + 8192 - 4 * 100),         # out inside a, out running into b
               dict(a=A, b=A, out=A + FB - 4)):                             # a == b is allowed, out over it is not
        assert run(**ch) == -1, ch


def test_signed_exp_refusals(bufs):
    from sift3d_amd import hip
    L = hip.lib()
    A, B, W = bufs

    def run(**ch):
        a = dict(v=A, ox=8, oy=8, oz=8, K=2, neg=1, out=B, work=W)
        a.update(ch)
        return L.sift3d_amd_field_exp_signed_device(a["v"], a["ox"], a["oy"], a["oz"], a["K"], a["neg"], a["out"],
                                                    a["work"], None)

    for ch in (dict(v=None), dict(out=None), dict(work=None), dict(ox=0), dict(oy=-1), dict(oz=0), dict(K=-1),
               dict(K=21), dict(neg=2), dict(neg=-1), dict(v=A + 2), dict(out=B + 1), dict(work=W + 4), dict(out=A),
               dict(work=A + 4 * 100), dict(work=B + 4 * 1000), dict(neg=0, K=0, out=A)):
        assert run(**ch) == -1, ch


def _levels(hip, *rows):
    tab = (hip.DemonsLevel * len(rows))()
    for l, r in enumerate(rows):
        tab[l] = hip.DemonsLevel(*r)
    return tab


def _log(L, a):
    return L.sift3d_amd_logdemons_device(a["tab"], a["levels"], a["nc"], a["v"], a["alpha"], a["sf"], a["sd"],
                                         a["sym"], a["bch"], a["K"], a["work"], a["stats"], None)


@pytest.mark.parametrize("sym", [0, 1])
def test_logdemons_refusals(bufs, sym):
    """F and M in buffer 0, v and the statistics in 1, the work buffer in 2 (8^3, nc = 1)"""
    from sift3d_amd import hip
    L = hip.lib()
    A, B, W = bufs
    M = A + 8192
    work = 4 * L.sift3d_amd_logdemons_work_floats(8, 8, 8, 1, sym, 1)

    def lv(**ch):
        r = dict(F=A, nx=8, ny=8, nz=8, M=M, mx=8, my=8, mz=8, it=3)
        r.update(ch)
        return _levels(hip, (r["F"], r["nx"], r["ny"], r["nz"], r["M"], r["mx"], r["my"], r["mz"], r["it"]))

    base = dict(tab=lv(), levels=1, nc=1, v=B, alpha=1.0, sf=1.0, sd=1.0, sym=sym, bch=1, K=2, work=W,
                stats=B + 8192)
    changes = [
        dict(bch=2), dict(bch=-1), dict(sym=2), dict(sym=-1), dict(K=-1), dict(K=21),
        dict(tab=None), dict(v=None), dict(work=None), dict(stats=None), dict(levels=0), dict(levels=7),
        dict(tab=lv(F=None)), dict(tab=lv(M=None)), dict(tab=lv(nx=0)), dict(tab=lv(ny=-2)), dict(tab=lv(nz=0)),
        dict(tab=lv(mx=-1)), dict(tab=lv(my=0)), dict(tab=lv(mz=0)), dict(tab=lv(it=-1)),
        dict(nc=0), dict(alpha=0.0), dict(alpha=float("nan")), dict(sf=-0.1), dict(sd=float("inf")),
        dict(stats=B + 8196), dict(work=W + 4), dict(tab=lv(F=A + 2)), dict(tab=lv(M=M + 1)), dict(v=B + 2),
        dict(v=A + 4 * 300), dict(v=W + 4 * 9000), dict(stats=B + 4 * 1000), dict(work=B),
        dict(stats=W + work - 16),                                         # stats inside the work buffer's end
        # two levels whose second is not the half of the first
        dict(levels=2, tab=_levels(hip, (A, 8, 8, 8, M, 8, 8, 8, 1), (A, 5, 4, 4, M, 4, 4, 4, 1))),
    ]
    if sym:
        changes += [dict(tab=lv(mx=7)), dict(tab=lv(my=9)), dict(tab=lv(mz=4))]    # unequal shapes
    for ch in changes:
        a = dict(base)
        a.update(ch)
        assert _log(L, a) == -1, ch
    # the existing entry still refuses a third update
    assert L.sift3d_amd_demons_device_ex(A, 8, 8, 8, M, 8, 8, 8, 1, B, 3, 1.0, 1.0, 1.0, 2, 2, W, B + 8192, None) == -1


# ---- 5. the api's refusals ---------------------------------------------------------------------------------------
def test_python_refusals(api):
    vol = np.zeros((5, 6, 7), F32)
    fld = np.zeros((3, 5, 6, 7), F32)
    for upd in ("logdomain", "symmetric"):
        with pytest.raises(ValueError, match="velocity"):
            api.refine_field(vol, vol, fld, update=upd)
        with pytest.raises(ValueError, match="bch"):
            api.refine_field(vol, vol, None, update=upd, bch=2)
    with pytest.raises(ValueError, match="one shape"):
        api.refine_field(vol, np.zeros((5, 6, 8), F32), None, update="symmetric")
    for call in (lambda: api.lie_bracket(fld, fld), lambda: api.field_exp(fld, 2, negate=True)):
        with pytest.raises(ValueError):
            call()

