"""CPU (not gpu): the host side of "Discrete displacement search" (include/sift3d_amd.h) -- the numpy restatement
(tests/discrete_restatement.py) against analysis, the exported symbols, the byte- and work-size formulas against the
header's, the struct mirror of sift3d_amd/hip.py, the pinned Python signatures, and every refusal of every C entry on
made-up pointers (they check their arguments before any device call)."""
import ctypes as C
import inspect
import itertools
import os

import numpy as np
import pytest

from tests import discrete_restatement as dr

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTED = ("sift3d_amd_cost_volume_bytes", "sift3d_amd_cost_volume_work_bytes", "sift3d_hip_cost_volume",
            "sift3d_amd_cost_select_work_bytes", "sift3d_hip_cost_select", "sift3d_amd_block_field_smooth_work_bytes",
            "sift3d_hip_block_field_smooth", "sift3d_hip_block_field_expand",
            "sift3d_amd_discrete_register_default_params", "sift3d_amd_discrete_register_struct_bytes",
            "sift3d_amd_discrete_register_work_floats", "sift3d_amd_discrete_register_device")


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


# ---- content shared with tests/test_discrete.py ----------------------------------------------------------------------
def smooth_noise(shape, seed, sigma=1.5):
    rng = np.random.default_rng(seed)
    a = np.fft.fftn(rng.standard_normal(shape))
    for ax, n in enumerate(shape):
        g = np.exp(-2.0 * (np.pi * sigma) ** 2 * np.fft.fftfreq(n) ** 2)
        a = a * g.reshape([-1 if d == ax else 1 for d in range(3)])
    a = np.fft.ifftn(a).real
    return (a / a.std()).astype(F32)


def ints(shape, seed, lo=-200, hi=200):
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(F32)


# ---- the restatement against analysis --------------------------------------------------------------------------------
@pytest.mark.parametrize("R,s,nc", [(1, (1, 0, -1), 1), (2, (-2, 1, 0), 3), (3, (0, 0, 0), 2)])
def test_integer_shift_costs_exactly_zero_there_and_more_elsewhere(R, s, nc):
    """W(p) = F(p - s) on random integer content: F_i - W_(i+s) is exactly 0 at every voxel of a block whose shifted
    block stays on the grid and off np.roll's wrap, so the cost at label s is 0.0f; every other valid label sums
    squares of non-zero integers somewhere (random content repeats nowhere over a block) and is > 0."""
    shape = (16, 20, 24)
    F = np.stack([ints(shape, 5 + c) for c in range(nc)])
    W = np.roll(F, (s[2], s[1], s[0]), (1, 2, 3))
    cost = dr.cost_volume(F, W, R)
    D = 2 * R + 1
    ks = ((s[2] + R) * D + (s[1] + R)) * D + (s[0] + R)
    seen = 0
    for bz, by, bx in itertools.product(*(range(n // 4) for n in shape)):
        lo = [4 * b + d for b, d in zip((bx, by, bz), s)]
        if not all(l >= max(d, 0) and l + 3 <= n - 1 + min(d, 0) for l, d, n in zip(lo, s, shape[::-1])):
            continue
        seen += 1
        c = cost[bz, by, bx]
        assert c[ks] == F32(0.0) and not np.signbit(c[ks])
        others = np.delete(c, ks)
        assert (others > 0).all()
    assert seen >= 8
    assert np.isinf(cost).any() and not np.isnan(cost).any()   # the labels that leave the grid


def test_cost_is_the_mean_squared_difference_and_masks_give_inf():
    shape = (8, 8, 12)
    F = np.stack([smooth_noise(shape, 1), smooth_noise(shape, 2)])
    W = np.stack([smooth_noise(shape, 3), smooth_noise(shape, 4)])
    cost = dr.cost_volume(F, W, 1)
    k0 = 13                                                   # d = 0
    want = ((F.astype(np.float64) - W) ** 2)[:, 4:8, 0:4, 8:12].mean()
    assert abs(float(cost[1, 0, 2, k0]) - want) <= 1e-6 * want
    VF = np.ones(shape, F32)
    VF[5, 2, 9] = 0.25                                        # one voxel of block (2, 0, 1) out of V_F
    VW = np.ones(shape, F32)
    VW[0, 0, 0] = 0.0                                         # one voxel out of V_W
    m = dr.cost_volume(F, W, 1, VF, VW)
    assert np.isinf(m[1, 0, 2]).all()
    # block (0, 0, 0) reads W voxel (0, 0, 0) under d = 0 only (any other label of R = 1 that covers it leaves the grid)
    assert np.isinf(m[0, 0, 0, k0]) and np.isfinite(cost[0, 0, 0, k0])
    # block (1, 0, 0) covers x = 4 .. 7: d = (-1, 0, 0) covers x = 3 .. 6, not voxel 0: untouched by the hole
    untouched = np.isfinite(m)
    assert np.array_equal(m[untouched], cost[untouched])
    VF[5, 2, 9] = 0.5                                         # the threshold itself is in
    assert np.isfinite(dr.cost_volume(F, W, 1, VF, None)[1, 0, 2, k0])


def _argmin_tie_rule(cost_b, R):
    """numpy's arg-min of one block under the tie rule, written the slow way"""
    dx, dy, dz, d2 = dr.labels(R)
    order = sorted(range(len(cost_b)), key=lambda k: (cost_b[k], d2[k], k))
    return order[0]


def test_theta_zero_is_the_argmin_under_the_tie_rule():
    rng = np.random.default_rng(3)
    R, nb = 2, (2, 3, 2)
    cost = rng.integers(0, 4, nb + (125,)).astype(F32)        # few values: many exact ties
    cost[0, 0, 0] = 7.0                                       # all equal: the label of |d|^2 = 0 wins
    cost[1, 2, 1] = np.inf                                    # empty
    cost[0, 1, 0, :] = 5.0
    cost[0, 1, 0, [0, 124]] = 1.0                             # equal val and |d|^2: the smaller k
    u = rng.standard_normal((3,) + nb).astype(F32)
    v, data, (s, n) = dr.cost_select(cost, u, 0.0)
    dx, dy, dz, _ = dr.labels(R)
    for b in itertools.product(*(range(m) for m in nb)):
        if b == (1, 2, 1):
            assert v[(slice(None),) + b].tobytes() == u[(slice(None),) + b].tobytes() and np.isinf(data[b])
            continue
        k = _argmin_tie_rule(cost[b], R)
        assert tuple(v[(slice(None),) + b]) == (dx[k], dy[k], dz[k]) and data[b] == cost[b][k]
    assert tuple(v[:, 0, 0, 0]) == (0, 0, 0) and tuple(v[:, 0, 1, 0]) == (-2, -2, -2)
    assert n == 11 and s == float(data[np.isfinite(data)].astype(np.float64).sum())


def test_huge_theta_returns_the_label_nearest_u():
    rng = np.random.default_rng(4)
    R, nb = 3, (2, 2, 3)
    cost = rng.random(nb + (343,)).astype(F32)
    u = (rng.random((3,) + nb) * 8 - 4).astype(F32)           # some outside the cube: clamped by the choice
    v, data, _ = dr.cost_select(cost, u, 1e12)
    want = np.clip(np.rint(u.astype(np.float64)), -R, R)
    assert np.array_equal(v, want.astype(F32))


@pytest.mark.parametrize("nb", [(1, 1, 1), (2, 1, 3), (5, 4, 3)])
def test_smoothing_keeps_a_constant_field_bit_for_bit(nb):
    a = np.empty((3,) + nb, F32)
    a[0], a[1], a[2] = F32(0.1), F32(-3.7), F32(1e-41)        # 0.25 c + 0.5 c + 0.25 c is exact: powers of two
    for passes in (0, 1, 2, 16):
        assert dr.smooth(a, passes).tobytes() == a.tobytes()
    b = np.zeros((3,) + nb, F32)
    b[:, 0, 0, 0] = 1
    assert dr.smooth(b, 0).tobytes() == b.tobytes()
    if nb == (5, 4, 3):
        s = dr.smooth(b, 1)
        assert s[0, 0, 0, 0] == F32(0.75 ** 3) and s[0, 0, 0, 1] == F32(0.25 * 0.75 * 0.75) and s[0, 2, 0, 0] == 0
        assert abs(float(s[0].sum()) - 1.0) < 1e-6            # the clamped binomial keeps the sum


def test_expand_of_a_linear_block_field_is_linear_between_the_block_centres():
    shape = (13, 22, 34)
    nb = tuple(n // 4 for n in shape)
    bz, by, bx = np.meshgrid(*(np.arange(n) for n in nb), indexing="ij")
    b = np.stack([2 * bx - by, 0.5 * bz + bx, 3 - by]).astype(F32)      # small integers and halves: exact
    w = dr.expand(b, shape)
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    inside = np.ones(shape, bool)
    for p, n in zip((z, y, x), nb):
        inside &= (p >= 1.5) & (p <= 4 * (n - 1) + 1.5)
    cx, cy, cz = (x - 1.5) / 4, (y - 1.5) / 4, (z - 1.5) / 4
    want = np.stack([2 * cx - cy, 0.5 * cz + cx, 3 - cy])
    assert inside.sum() > 100
    assert np.abs(w - want)[:, inside].max() <= 1e-5
    # past the last block centre and before the first: the edge value
    assert w[0, 0, 0, 0] == b[0, 0, 0, 0] and w[1, -1, -1, -1] == b[1, -1, -1, -1]
    assert np.array_equal(w[:, :, :, 33], w[:, :, :, 30])    # x = 29.5 is the last centre: 30 .. 33 hold the edge value
    assert w.dtype == F32 and w.shape == (3,) + shape


def test_one_level_moves_blocks_by_a_known_shift():
    """the restatement's level on an integer shift, with numpy stand-ins for the warp and the composition at whole
    voxels: every interior block ends on the shift"""
    shape = (16, 16, 16)
    F = ints(shape, 9)
    s = (1, -1, 2)
    M = np.roll(F, (s[2], s[1], s[0]), (0, 1, 2))           # M(p + s) = F(p): the field that matches is +s

    def warp(src, u, interp):
        assert not u.any()
        return src.copy()

    def compose(u, w):
        return (u + w).astype(F32)
    u0 = np.zeros((3,) + shape, F32)
    u1, records, (W, VW, Cv, b, w) = dr.level(F, M, u0, 2, (0.0, 0.5), 0, None, None, warp, compose)
    assert np.array_equal(b[:, 1:3, 1:3, 1:3].reshape(3, -1).T, np.tile(np.array(s, F32), (8, 1)))
    assert tuple(u1[:, 8, 8, 8]) == s and len(records) == 2 and records[0][1] == 64


# ---- symbols, sizes, layouts, signatures -----------------------------------------------------------------------------
def test_symbols_exported_and_declared(hip):
    header = open(os.path.join(ROOT, "include", "sift3d_amd.h")).read()
    assert "Discrete displacement search" in header and "PARITY UNPINNED" in header
    for name in EXPORTED:
        assert hasattr(hip.lib(), name), name
        assert name + "(" in header, name


def _pad4(n):
    return (n + 3) // 4 * 4


def test_sizes_match_the_header(hip):
    L = hip.lib()
    for (nx, ny, nz), R in itertools.product([(8, 8, 8), (13, 9, 14), (4, 5, 7), (256, 256, 256)], range(1, 7)):
        assert L.sift3d_amd_cost_volume_bytes(nx, ny, nz, R) == (nx // 4) * (ny // 4) * (nz // 4) * (2 * R + 1) ** 3 * 4
        assert L.sift3d_amd_cost_volume_work_bytes(nx, ny, nz, 3, R) == 0
    assert L.sift3d_amd_cost_volume_bytes(256, 256, 256, 6) == 2303721472     # the header's 2.3 GB
    for bad in ((3, 8, 8, 2), (8, 0, 8, 2), (8, 8, -4, 2), (8, 8, 8, 0), (8, 8, 8, 7)):
        assert L.sift3d_amd_cost_volume_bytes(*bad) == 0, bad
    assert L.sift3d_amd_cost_select_work_bytes(2, 3, 4) == hip.COST_SELECT_WORK_BYTES == 16384
    assert L.sift3d_amd_cost_select_work_bytes(0, 3, 4) == 0
    for passes in range(0, 17):
        assert L.sift3d_amd_block_field_smooth_work_bytes(5, 4, 3, passes) == (720 if passes >= 2 else 0)
    assert L.sift3d_amd_block_field_smooth_work_bytes(5, 4, 3, 17) == 0
    assert L.sift3d_amd_block_field_smooth_work_bytes(5, 0, 3, 2) == 0
    P = hip.COST_SELECT_WORK_BYTES // 4
    for f, m, nc, levels, R, mf, mm in [((24, 20, 16), (24, 20, 16), 2, 2, 2, 0, 0), ((24, 20, 16), (22, 21, 17), 2, 2, 2, 1, 1),
                                        ((13, 9, 14), (11, 9, 15), 12, 1, 6, 0, 1), ((33, 35, 37), (31, 30, 29), 1, 3, 4, 1, 0),
                                        ((16, 16, 16), (5, 5, 5), 16, 3, 1, 0, 0)]:
        n0, m0 = int(np.prod(f)), int(np.prod(m))
        b0 = (f[0] // 4) * (f[1] // 4) * (f[2] // 4)
        want = (_pad4(P) + _pad4(nc * n0) + _pad4(n0) + (0 if mm else _pad4(m0)) + _pad4(b0 * (2 * R + 1) ** 3)
                + 3 * _pad4(3 * b0) + _pad4(b0) + 2 * _pad4(3 * n0))
        g, h = f, m
        for _ in range(1, levels):
            g, h = tuple((d + 1) // 2 for d in g), tuple((d + 1) // 2 for d in h)
            want += _pad4(3 * int(np.prod(g))) + mf * _pad4(int(np.prod(g))) + mm * _pad4(int(np.prod(h)))
        assert L.sift3d_amd_discrete_register_work_floats(*f, *m, nc, levels, R, mf, mm) == want
    for bad in ((0, 8, 8, 8, 8, 8, 1, 1, 1, 0, 0), (8, 8, 8, 8, -1, 8, 1, 1, 1, 0, 0), (8, 8, 8, 8, 8, 8, 0, 1, 1, 0, 0),
                (8, 8, 8, 8, 8, 8, 17, 1, 1, 0, 0), (8, 8, 8, 8, 8, 8, 1, 0, 1, 0, 0), (8, 8, 8, 8, 8, 8, 1, 7, 1, 0, 0),
                (8, 8, 8, 8, 8, 8, 1, 1, 0, 0, 0), (8, 8, 8, 8, 8, 8, 1, 1, 7, 0, 0), (3, 8, 8, 8, 8, 8, 1, 1, 1, 0, 0),
                (8, 8, 6, 8, 8, 8, 1, 2, 1, 0, 0), (16, 16, 16, 16, 16, 16, 1, 4, 1, 0, 0)):
        assert L.sift3d_amd_discrete_register_work_floats(*bad) == 0, bad
    assert L.sift3d_amd_discrete_register_work_floats(7, 8, 8, 1, 1, 1, 1, 2, 1, 0, 0) > 0       # 7 -> 4


def test_struct_mirror_and_defaults(hip):
    L = hip.lib()
    assert L.sift3d_amd_discrete_register_struct_bytes(0) == C.sizeof(hip.DiscreteRegisterParams) == 16 + 8 * 16
    assert [L.sift3d_amd_discrete_register_struct_bytes(k) for k in range(1, 7)] == [6, 16, 16, 16, 16384, 0]
    assert (hip.DISCRETE_MAX_RADIUS, hip.DISCRETE_MAX_CHANNELS, hip.DISCRETE_MAX_THETAS,
            hip.DISCRETE_MAX_PASSES) == (dr.MAX_RADIUS, dr.MAX_CHANNELS, dr.MAX_THETAS, dr.MAX_PASSES)
    assert [f[0] for f in hip.DiscreteRegisterParams._fields_] == ["radius", "passes", "n_theta", "theta"]
    p = hip.discrete_register_params()
    assert (p.radius, p.passes, p.n_theta) == (4, 2, 6)
    assert tuple(p.theta[:6]) == dr.DEFAULT_THETAS and not any(p.theta[6:])
    ratios = [p.theta[j + 1] / p.theta[j] for j in range(5)]
    assert all(2.9 < r < 3.4 for r in ratios)                # a factor ~3 apart (WBIR 2014's, scaled)
    q = hip.discrete_register_params(radius=2, passes=0, thetas=(0.5, 0.0))
    assert (q.radius, q.passes, q.n_theta, q.theta[0], q.theta[1]) == (2, 0, 2, 0.5, 0.0)
    L.sift3d_amd_discrete_register_default_params(None)      # a NULL is ignored


def test_python_signatures_are_pinned(hip):
    from sift3d_amd import api

    def sig(f):
        return str(inspect.signature(f))
    assert sig(api.cost_volume) == ("(fixed, moving, transform=None, radius=4, features='mind', mask_fixed=None, "
                                    "mask_moving=None)")
    assert sig(api.register_discrete) == ("(moving, fixed, field=None, features='mind', mind=None, levels=3, radius=4, "
                                          "thetas=None, passes=2, mask_fixed=None, mask_moving=None)")
    assert api.CostVolume._fields == ("cost", "radius", "blocks")
    assert api.DiscreteRegistration._fields == ("field", "warped", "data", "level_slices", "jacobian")
    assert sig(hip.cost_volume) == "(F, W, radius=4, valid_fixed=None, valid_warped=None, cost=None, work=None)"
    assert sig(hip.cost_select) == "(cost, u, theta, v=None, data=None, stats=None, work=None)"
    assert sig(hip.block_field_smooth) == "(src, passes=2, dst=None, work=None)"
    assert sig(hip.block_field_expand) == "(b, shape, w=None)"
    assert sig(hip.discrete_register) == "(Fs, Ms, field, params=None, mask_fixed=None, mask_moving=None, work=None)"


def test_python_refusals(hip):
    from sift3d_amd import api
    F = np.zeros((32, 32, 32), F32)
    for kw, word in ((dict(radius=0), "radius"), (dict(radius=7), "radius"), (dict(radius=2.0), "radius"),
                     (dict(passes=-1), "passes"), (dict(passes=17), "passes"), (dict(thetas=()), "thetas"),
                     (dict(thetas=[0.1] * 17), "thetas"), (dict(thetas=[-0.1]), "theta"),
                     (dict(thetas=[float("inf")]), "theta"), (dict(thetas=[float("nan")]), "theta"),
                     (dict(levels=0), "levels"), (dict(levels=7), "levels"), (dict(features="lncc"), "features"),
                     (dict(features="intensity", mind={}), "mind")):
        with pytest.raises(ValueError, match=word):
            api.register_discrete(F, F, **kw)
    with pytest.raises(ValueError, match="radius"):
        api.cost_volume(F, F, radius=9)
    with pytest.raises(ValueError, match="features"):
        api.cost_volume(F, F, features=3)


# ---- the refusals of the C entries -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bufs(hip):
    """made-up addresses without a device; real allocations covering every range named below with one, so that a
    regressed check could not make a kernel touch unmapped memory"""
    from sift3d_amd import api
    if api.device_available():
        b = [hip.lib().sift3d_hip_malloc(1 << 20) for _ in range(3)]
        assert all(b)
        yield b
        for p in b:
            hip.lib().sift3d_hip_free(p)
    else:
        yield [0x1000000, 0x2000000, 0x3000000]


VOL = 8 * 8 * 8 * 4                                           # one channel of an 8^3 volume, bytes
KB = 8 * 27 * 4                                               # the cost volume of 8^3 at R = 1


def test_cost_volume_refusals(hip, bufs):
    """8^3, nc = 2: F and W (4096 B each) and the masks (2048 B each) in buffer 0, the cost volume (864 B) in buffer 1"""
    L = hip.lib()
    A, B, _ = bufs
    base = dict(F=A, W=A + 8192, nc=2, nx=8, ny=8, nz=8, VF=A + 16384, VW=A + 32768, r=1, cost=B, work=None)

    def run(a):
        return L.sift3d_hip_cost_volume(a["F"], a["W"], a["nc"], a["nx"], a["ny"], a["nz"], a["VF"], a["VW"], a["r"],
                                        a["cost"], a["work"], None)
    for ch in (dict(F=None), dict(W=None), dict(cost=None), dict(nx=0), dict(ny=-8), dict(nz=0), dict(nx=3), dict(ny=2),
               dict(nz=1), dict(nc=0), dict(nc=17), dict(nc=-1), dict(r=0), dict(r=7), dict(r=-2),
               dict(F=A + 2), dict(W=A + 8193), dict(VF=A + 16386), dict(VW=A + 32769), dict(cost=B + 2),
               dict(cost=A), dict(cost=A + 2 * VOL - 4), dict(cost=A + 8192 + 2 * VOL - 4), dict(cost=A + 8192 - KB + 4),
               dict(cost=A + 16384 + VOL - 4), dict(cost=A + 32768), dict(cost=A + 16384 - KB + 4)):
        a = dict(base)
        a.update(ch)
        assert run(a) == -1, ch


def test_cost_select_refusals(hip, bufs):
    """2^3 blocks, R = 1: the cost volume (864 B) and u (96 B) in buffer 0; v (96 B), data (32 B), the record (16 B) in
    buffer 1; the partials in buffer 2"""
    L = hip.lib()
    A, B, Wb = bufs
    base = dict(cost=A, nbx=2, nby=2, nbz=2, r=1, u=A + 4096, theta=0.5, v=B, data=B + 1024, stats=B + 2048, work=Wb)

    def run(a):
        return L.sift3d_hip_cost_select(a["cost"], a["nbx"], a["nby"], a["nbz"], a["r"], a["u"], a["theta"], a["v"],
                                        a["data"], a["stats"], a["work"], None)
    for ch in (dict(cost=None), dict(u=None), dict(v=None), dict(data=None), dict(stats=None), dict(work=None),
               dict(nbx=0), dict(nby=-1), dict(nbz=0), dict(r=0), dict(r=7), dict(theta=-0.1), dict(theta=float("inf")),
               dict(theta=float("nan")), dict(theta=-float("inf")),
               dict(cost=A + 2), dict(u=A + 4097), dict(v=B + 2), dict(data=B + 1025), dict(stats=B + 2052),
               dict(work=Wb + 4), dict(v=A), dict(v=A + KB - 4), dict(data=A + 4096 + 92), dict(stats=A + 8),
               dict(work=A), dict(work=A + 4096), dict(work=A - 16384 + 8), dict(data=B + 92), dict(stats=B + 88),
               dict(stats=B + 1024 + 24), dict(work=B), dict(work=B + 2048 - 16384 + 8), dict(v=Wb + 16384 - 8)):
        a = dict(base)
        a.update(ch)
        assert run(a) == -1, ch


def test_smooth_and_expand_refusals(hip, bufs):
    """5 x 4 x 3 blocks (720 B a field): src in buffer 0, dst in buffer 1, the second buffer in buffer 2"""
    L = hip.lib()
    A, B, Wb = bufs
    base = dict(src=A, dst=B, nbx=5, nby=4, nbz=3, passes=2, work=Wb)

    def run(a):
        return L.sift3d_hip_block_field_smooth(a["src"], a["dst"], a["nbx"], a["nby"], a["nbz"], a["passes"], a["work"],
                                               None)
    for ch in (dict(src=None), dict(dst=None), dict(work=None), dict(nbx=0), dict(nby=-2), dict(nbz=0), dict(passes=-1),
               dict(passes=17), dict(src=A + 1), dict(dst=B + 2), dict(work=Wb + 4), dict(dst=A), dict(dst=A + 716),
               dict(dst=A - 716), dict(work=A + 8), dict(work=B + 712), dict(work=B - 712), dict(passes=0, dst=A + 360),
               dict(passes=1, dst=A + 4)):
        a = dict(base)
        a.update(ch)
        assert run(a) == -1, ch

    base = dict(b=A, nbx=2, nby=3, nbz=2, w=B, nx=9, ny=14, nz=8)

    def run2(a):
        return L.sift3d_hip_block_field_expand(a["b"], a["nbx"], a["nby"], a["nbz"], a["w"], a["nx"], a["ny"], a["nz"],
                                               None)
    for ch in (dict(b=None), dict(w=None), dict(nbx=0), dict(nby=-3), dict(nbz=0), dict(nx=0), dict(ny=-14), dict(nz=0),
               dict(nbx=3), dict(nby=2), dict(nbz=1), dict(nx=12), dict(nz=3, nbz=0), dict(b=A + 2), dict(w=B + 1),
               dict(w=A), dict(w=A + 140), dict(w=A - 3 * 9 * 14 * 8 * 4 + 4)):
        a = dict(base)
        a.update(ch)
        assert run2(a) == -1, ch


def test_driver_refusals(hip, bufs):
    """16^3, nc = 2, two levels: level 0's stacks (32 KB each) and level 1's (4 KB each) in buffer 0 with the masks
    (16 KB each) and the field (48 KB); the records in buffer 1; the work buffer in buffer 2"""
    L = hip.lib()
    Ab, Bb, Wb = bufs
    vol = 16 * 16 * 16 * 4
    need = L.sift3d_amd_discrete_register_work_floats(16, 16, 16, 16, 16, 16, 2, 2, 2, 1, 1) * 4
    assert 0 < need <= (1 << 20)
    F0, M0, F1, M1 = Ab, Ab + 2 * vol, Ab + 4 * vol, Ab + 4 * vol + 4096
    VF, VM, U = Ab + 5 * vol, Ab + 6 * vol, Ab + 7 * vol

    def run(lev=((F0, 16, 16, 16, M0, 16, 16, 16), (F1, 8, 8, 8, M1, 8, 8, 8)), levels=2, nc=2, vf=VF, vm=VM, u=U,
            stats=Bb, work=Wb, null_levels=False, null_params=False, **kw):
        tab = (hip.DemonsLevel * len(lev))(*[hip.DemonsLevel(*v, 0) for v in lev])
        p = hip.discrete_register_params(radius=2)
        for k, v in kw.items():
            if k == "theta0":
                p.theta[0] = v
            else:
                setattr(p, k, v)
        return L.sift3d_amd_discrete_register_device(None if null_levels else tab, levels, nc, vf, vm, u,
                                                     None if null_params else C.byref(p), stats, work, None)
    l0 = (F0, 16, 16, 16, M0, 16, 16, 16)
    for kw in (dict(null_levels=True), dict(u=None), dict(stats=None), dict(work=None),
               dict(lev=((None,) + l0[1:], (F1, 8, 8, 8, M1, 8, 8, 8))), dict(lev=(l0, (F1, 8, 8, 8, None, 8, 8, 8))),
               dict(lev=((F0, 0, 16, 16, M0, 16, 16, 16), (F1, 8, 8, 8, M1, 8, 8, 8))),
               dict(lev=((F0, 16, 16, 16, M0, 16, -1, 16), (F1, 8, 8, 8, M1, 8, 8, 8))),
               dict(lev=(l0, (F1, 8, 8, 7, M1, 8, 8, 8))), dict(lev=(l0, (F1, 8, 8, 8, M1, 9, 8, 8))),
               dict(lev=((F0, 6, 16, 16, M0, 16, 16, 16), (F1, 3, 8, 8, M1, 8, 8, 8))),
               dict(lev=((F0, 3, 16, 16, M0, 16, 16, 16),), levels=1),
               dict(levels=0), dict(levels=7), dict(nc=0), dict(nc=17), dict(radius=0), dict(radius=7), dict(passes=-1),
               dict(passes=17), dict(n_theta=0), dict(n_theta=17), dict(theta0=-1.0), dict(theta0=float("nan")),
               dict(theta0=float("inf")),
               dict(lev=((F0 + 2,) + l0[1:], (F1, 8, 8, 8, M1, 8, 8, 8))), dict(lev=(l0, (F1, 8, 8, 8, M1 + 1, 8, 8, 8))),
               dict(vf=VF + 2), dict(vm=VM + 3), dict(u=U + 2), dict(stats=Bb + 4), dict(work=Wb + 4),
               dict(work=Ab), dict(work=F1 - need + 8), dict(work=M1 + 4088), dict(work=VF + 8), dict(work=VM + vol - 8),
               dict(work=U + 3 * vol - 8), dict(u=F0 + 8), dict(u=M1), dict(u=VM - 3 * vol + 4), dict(stats=U + 16),
               dict(stats=F0 + 2 * vol - 8), dict(stats=Wb + need - 8), dict(u=Wb + need - 4),
               dict(stats=VF - 12 * 16 + 8)):
        assert run(**kw) == -1, kw
    # (NULL params take the defaults, radius 4: still every check passes up to the device, which this test never reaches
    # with a refusal above; the defaults themselves are test_struct_mirror_and_defaults')
