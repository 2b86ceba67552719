"""GPU: "Discrete displacement search" (include/sift3d_amd.h) on the device against the numpy restatement
(tests/discrete_restatement.py): the cost volume, the selection, the smoothing and the expansion BYTE FOR BYTE (the one
order-free sum of the statistics within gamma_n of the exactly rounded sum), the driver stage by stage from the device's
own intermediate outputs, and the end-to-end run on a pair that demons alone does not solve."""
import math

import numpy as np
import pytest

from tests import discrete_restatement as dr
from tests.test_discrete_host import ints, smooth_noise

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def stack(shape, nc, seed, sigma=1.5):
    return np.stack([smooth_noise(shape, seed + c, sigma) for c in range(nc)])


def masks(shape, seed):
    """a few holes, and a value at the threshold on either side; V_F has exactly one voxel out in block (0, 0, 0)"""
    rng = np.random.default_rng(seed)
    VF, VW = np.ones(shape, F32), np.ones(shape, F32)
    VF[1, 2, 3] = 0.49999997
    VF[2, 2, 2] = 0.5
    for V in (VF, VW):
        idx = rng.integers(0, np.prod(shape), 3)
        V.reshape(-1)[idx] = rng.choice(np.array([0.0, 0.25, 0.49999997], F32), 3)
    VW[shape[0] - 2, shape[1] - 3, shape[2] - 2] = 0.0        # one voxel out of V_W near the far corner
    VW[1, 1, 1] = 0.5
    return VF, VW


# ---- the cost volume ---------------------------------------------------------------------------------------------------
# (nz, ny, nx), nc, R: 2^3 blocks, every block with off-grid labels; trailing voxels; 12 channels; every R once at 16^3
# (R = 6 > 4 x the blocks of an axis: most labels invalid); 16 channels; one block on an axis
SHAPES = [((8, 8, 8), 1, 1), ((14, 9, 13), 3, 2), ((8, 12, 16), 12, 2)] + [((16, 16, 16), 2, R) for R in range(1, 7)] + \
         [((8, 12, 8), 16, 3), ((4, 9, 21), 2, 4), ((12, 4, 8), 1, 5)]


@pytest.mark.parametrize("shape,nc,R", SHAPES, ids=["%dx%dx%d-nc%d-R%d" % (s[2], s[1], s[0], c, R) for s, c, R in SHAPES])
def test_cost_volume_bytes_against_the_restatement(hip, shape, nc, R):
    F, W = stack(shape, nc, 11), stack(shape, nc, 41)
    want = dr.cost_volume(F, W, R)
    got = host(hip.cost_volume(dev(F), dev(W), R))
    assert same_bits(got, want)
    assert np.isfinite(want).any() and np.isinf(want).any() and not np.isnan(got).any()
    if R == 6:
        assert np.isinf(want).mean() > 0.5                   # most labels leave a 16^3 grid


@pytest.mark.parametrize("which", ["fixed", "warped", "both"])
@pytest.mark.parametrize("shape,nc,R", [((12, 9, 14), 2, 2), ((16, 16, 16), 1, 5)])
def test_cost_volume_with_masks(hip, shape, nc, R, which):
    F, W = stack(shape, nc, 12), stack(shape, nc, 42)
    VF, VW = masks(shape, 5)
    VF = VF if which in ("fixed", "both") else None
    VW = VW if which in ("warped", "both") else None
    want = dr.cost_volume(F, W, R, VF, VW)
    plain = dr.cost_volume(F, W, R)
    got = host(hip.cost_volume(dev(F), dev(W), R, dev(VF), dev(VW)))
    assert same_bits(got, want)
    assert np.isinf(want).sum() > np.isinf(plain).sum()
    if VF is not None:
        assert np.isinf(want[0, 0, 0]).all()                 # block (0, 0, 0) has one voxel out of V_F
    if VW is not None:
        k0 = ((2 * R + 1) ** 3) // 2                          # d = 0 of the last block covers the hole near the corner
        hole = (shape[0] - 2, shape[1] - 3, shape[2] - 2)
        if all(4 * n - 4 <= h < 4 * n for n, h in zip(want.shape[:3], hole)):       # (16^3: the hole is in the last block)
            assert np.isinf(want[-1, -1, -1, k0]) and np.isfinite(plain[-1, -1, -1, k0])


def contents(shape, nc):
    F, W = stack(shape, nc, 21), stack(shape, nc, 51)
    I = np.stack([ints(shape, 22 + c) for c in range(nc)])
    return {
        "subnormal": ((F * F32(1e-38)).astype(F32), (W * F32(1e-38)).astype(F32)),
        "flat": (np.full((nc,) + shape, 2.5, F32), np.full((nc,) + shape, -1.25, F32)),
        "huge": (np.full((nc,) + shape, 3e38, F32) * np.sign(F), np.full((nc,) + shape, -3e38, F32) * np.sign(F)),
        "huge-finite": ((F * F32(1e18)).astype(F32), (W * F32(1e18)).astype(F32)),
        "integer-shift": (I, np.roll(I, (1, -1, 1), (1, 2, 3))),
        "identical": (F, F),
    }


NAMES = sorted(contents((8, 8, 8), 1))


@pytest.mark.parametrize("name", NAMES)
def test_cost_volume_content(hip, name):
    shape, nc, R = (12, 8, 16), 2, 2
    F, W = contents(shape, nc)[name]
    F, W = np.ascontiguousarray(F, F32), np.ascontiguousarray(W, F32)
    want = dr.cost_volume(F, W, R)
    got = host(hip.cost_volume(dev(F), dev(W), R))
    assert same_bits(got, want)
    inside = dr.cost_volume(np.zeros_like(F), np.zeros_like(W), R) == 0      # the valid labels
    if name == "flat":
        assert (want[inside] == F32(3.75 * 3.75)).all()      # all costs equal: what feeds the tie rule
    if name == "huge":
        assert np.isinf(want).all() and inside.any()         # (6e38)^2 / 1 rounds past FLT_MAX: +inf by overflow
    if name == "subnormal":
        assert (want[inside] == 0).all()                     # squares of 1e-38 vanish in float, not in the double sums
    if name == "integer-shift":
        assert (want[1, 1, 1:3, 83] == 0).all()              # d = (1, -1, 1): k = (3 * 5 + 1) * 5 + 3
    if name == "identical":
        assert (want[..., 62] == 0).all()


# ---- the selection -----------------------------------------------------------------------------------------------------
def check_select(hip, cost, u, theta):
    v, data, (s, n) = dr.cost_select(cost, u, theta)
    gv, gd, gs = hip.cost_select(dev(cost), dev(u), theta)
    assert same_bits(host(gv), v) and same_bits(host(gd), data)
    ds, dn = hip.demons_stats(gs)
    assert int(dn[0]) == n
    assert abs(float(ds[0]) - s) <= dr.gamma(max(n, 1)) * abs(s)
    return v, data, n


@pytest.mark.parametrize("theta", [0.0, 0.05, 3.0])
@pytest.mark.parametrize("shape,nc,R", [((8, 8, 8), 1, 1), ((14, 9, 13), 3, 2), ((16, 16, 16), 2, 6), ((12, 20, 16), 2, 4)])
def test_select_on_the_devices_own_cost_volumes(hip, shape, nc, R, theta):
    F, W = stack(shape, nc, 13), stack(shape, nc, 43)
    VF, VW = masks(shape, 6)
    cost = host(hip.cost_volume(dev(F), dev(W), R, dev(VF), dev(VW)))
    rng = np.random.default_rng(8)
    u = (rng.standard_normal((3,) + cost.shape[:3]) * 1.5).astype(F32)
    v, data, n = check_select(hip, cost, u, theta)
    assert 0 < n < data.size                                 # block (0, 0, 0) is empty
    assert v[:, 0, 0, 0].tobytes() == u[:, 0, 0, 0].tobytes() and np.isinf(data[0, 0, 0])


def test_select_on_hand_made_cost_volumes(hip):
    rng = np.random.default_rng(3)
    R, nb = 2, (3, 2, 5)
    cost = rng.integers(0, 3, nb + (125,)).astype(F32)        # few values: exact ties in val at theta 0
    cost[0, 0, 0] = 7.0                                       # all equal: |d|^2 decides, label 0
    cost[0, 1, 0] = 5.0
    cost[0, 1, 0, [0, 124, 4, 120]] = 1.0                     # equal val and |d|^2 = 12: the smallest k
    cost[1, 1, 1] = np.inf                                    # empty: v == u bit for bit
    cost[2, 0, 3, :100] = np.inf                              # a block with invalid labels only in front
    u = rng.standard_normal((3,) + nb).astype(F32)
    u[:, 1, 1, 1] = np.array([-0.0, 1e-40, 3.25], F32)        # bytes that a recomputation would not keep
    for theta in (0.0, 0.5):
        v, data, n = check_select(hip, cost, u, theta)
        assert n == 29 and v[:, 1, 1, 1].tobytes() == u[:, 1, 1, 1].tobytes()
    v, _, _ = check_select(hip, cost, np.zeros_like(u), 0.0)
    assert tuple(v[:, 0, 0, 0]) == (0, 0, 0) and tuple(v[:, 0, 1, 0]) == (-2, -2, -2)
    # exact ties in val with theta > 0: u = 0 and a flat block: q decides through val, then k among the equal |d|^2
    flat = np.full(nb + (125,), 2.0, F32)
    flat[..., 62] = np.inf                                    # without d = 0: six labels of |d|^2 = 1 tie in val
    v, _, _ = check_select(hip, flat, np.zeros_like(u), 0.25)
    assert (v[0] == 0).all() and (v[1] == 0).all() and (v[2] == -1).all()      # k = 37: d = (0, 0, -1)
    v, _, _ = check_select(hip, np.full(nb + (125,), np.inf, F32), u, 1.0)     # every block empty: the sum is +0.0
    assert v.tobytes() == u.tobytes()


# ---- smoothing and expansion ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", [0, 1, 2, 16])
@pytest.mark.parametrize("nb", [(1, 1, 1), (3, 1, 2), (3, 4, 5), (9, 7, 33)])
def test_smooth_bytes(hip, nb, passes):
    rng = np.random.default_rng(17)
    a = (rng.standard_normal((3,) + nb) * 3).astype(F32)
    a.reshape(-1)[::7] = rng.integers(-6, 7, a.reshape(-1)[::7].shape).astype(F32)
    d = dev(a)
    got = host(hip.block_field_smooth(d, passes))
    assert same_bits(got, dr.smooth(a, passes))
    assert same_bits(host(d), a)                             # the source is not written
    const = np.full((3,) + nb, F32(-3.7))
    assert same_bits(host(hip.block_field_smooth(dev(const), passes)), const)


@pytest.mark.parametrize("shape", [(8, 8, 8), (14, 9, 13), (4, 7, 70)])
def test_expand_bytes(hip, shape):
    rng = np.random.default_rng(19)
    b = (rng.standard_normal((3,) + tuple(n // 4 for n in shape)) * 4).astype(F32)
    got = host(hip.block_field_expand(dev(b), shape))
    assert same_bits(got, dr.expand(b, shape))


# ---- the driver --------------------------------------------------------------------------------------------------------
def driver_inputs(hip, with_masks):
    shape, nc = (16, 20, 24), 2                               # 24 x 20 x 16 (x, y, z)
    M0 = stack(shape, nc, 31, 2.0)
    F0 = np.roll(M0, (1, -2, 1), (1, 2, 3)) + F32(0.05) * stack(shape, nc, 61)
    F0 = np.ascontiguousarray(F0, F32)
    Fs, Ms = [dev(F0)], [dev(M0)]
    Fs.append(hip.restrict2(Fs[0]))
    Ms.append(hip.restrict2(Ms[0]))
    rng = np.random.default_rng(23)
    u0 = dev((rng.standard_normal((3,) + shape) * 0.3).astype(F32))
    VF = VM = None
    if with_masks:
        VF, VM = (dev(m) for m in masks(shape, 9))
    return Fs, Ms, u0, VF, VM


def chained_level(hip, F, M, u, R, thetas, passes, VF, VM):
    """dr.level with the device's own warp and composition (their bits are pinned by their own tests)"""
    import torch

    def warp(src, field, interp):
        out = torch.empty(tuple(field.shape[1:]), dtype=torch.float32, device="cuda")
        return host(hip.warp_field(dev(src), out, dev(field), interp, 0.0))

    def compose(a, b):
        out = torch.empty(b.shape, dtype=torch.float32, device="cuda")
        hip.field_compose(dev(a), dev(b), out)
        return host(out)
    return dr.level(host(F), host(M), host(u), R, thetas, passes, None if VF is None else host(VF),
                    None if VM is None else host(VM), warp, compose)


@pytest.mark.parametrize("with_masks", [False, True], ids=["plain", "masked"])
def test_driver_stage_by_stage(hip, with_masks):
    R, thetas, passes = 2, (0.01, 0.1, 1.0), 2
    Fs, Ms, u0, VF, VM = driver_inputs(hip, with_masks)
    p = hip.discrete_register_params(R, passes, thetas)
    u = u0.clone()
    stats = hip.discrete_register(Fs, Ms, u, p, VF, VM)
    sums, counts = hip.demons_stats(stats)
    assert len(sums) == 2 * len(thetas)
    # the chain: restrict the start and the masks, run level 1, prolong, run level 0
    u1 = hip.restrict2(u0, scale=0.5)
    VF1 = None if VF is None else hip.restrict2(VF)
    VM1 = None if VM is None else hip.restrict2(VM)
    w1, rec1, _ = chained_level(hip, Fs[1], Ms[1], u1, R, thetas, passes, VF1, VM1)
    import torch
    up = hip.field_prolong2(dev(w1), torch.empty_like(u0))
    w0, rec0, _ = chained_level(hip, Fs[0], Ms[0], up, R, thetas, passes, VF, VM)
    assert same_bits(host(u), w0)
    assert not same_bits(host(u), host(u0))
    for (s, n), gs, gn in zip(rec1 + rec0, sums, counts):
        assert int(gn) == n and n > 0
        assert abs(float(gs) - s) <= dr.gamma(n) * abs(s)


def test_one_level_equals_the_four_entries_by_hand(hip):
    import torch
    Fs, Ms, _, _, _ = driver_inputs(hip, False)
    R, theta, passes = 3, 0.2, 2
    u = torch.zeros((3,) + tuple(Fs[0].shape[1:]), dtype=torch.float32, device="cuda")
    stats = hip.discrete_register(Fs[:1], Ms[:1], u, hip.discrete_register_params(R, passes, [theta]))
    zero = torch.zeros_like(u)
    W = hip.warp_field(Ms[0], torch.empty_like(Ms[0]), zero, "linear", 0.0)
    VW = hip.warp_field(torch.ones_like(Ms[0][0]), torch.empty_like(Ms[0][0]), zero, "nearest", 0.0)
    cost = hip.cost_volume(Fs[0], W, R, None, VW)
    v, data, st = hip.cost_select(cost, torch.zeros((3,) + tuple(cost.shape[:3]), device="cuda"), theta)
    w = hip.block_field_expand(hip.block_field_smooth(v, passes), tuple(Fs[0].shape[1:]))
    out = torch.empty_like(u)
    hip.field_compose(zero, w, out)
    assert same_bits(host(u), host(out)) and float(out.abs().max()) > 0
    assert same_bits(host(stats), host(st))


def test_api_wrappers(hip):
    from sift3d_amd import api
    Fs, Ms, u0, VF, VM = driver_inputs(hip, True)
    F, M = Fs[0][0].contiguous(), Ms[0][0].contiguous()
    keep = u0.clone()
    r = api.register_discrete(M, F, u0, features="intensity", levels=2, radius=2, thetas=(0.01, 0.1), passes=1,
                              mask_fixed=VF, mask_moving=VM)
    assert same_bits(host(u0), host(keep))                   # the start field is not modified
    u = u0.clone()
    stats = hip.discrete_register([F, hip.restrict2(F)], [M, hip.restrict2(M)], u,
                                  hip.discrete_register_params(2, 1, (0.01, 0.1)), VF, VM)
    assert same_bits(host(r.field), host(u))
    s, n = hip.demons_stats(stats)
    assert np.array_equal(r.data, s / n) and r.level_slices == (slice(2, 4), slice(0, 2))
    assert same_bits(host(r.warped), host(api.warp_field(M, u)))
    assert r.jacobian.det.shape == F.shape
    c = api.cost_volume(F, M, None, 2, "intensity", VF, VM)
    assert c.radius == 2 and c.blocks == (4, 5, 6)
    VW = api.warp_field(VM, keep * 0, "nearest")
    assert same_bits(host(c.cost), host(hip.cost_volume(F, M, 2, VF, VW)))
    c2 = api.cost_volume(None, None, u0, 1, (Fs[0], Ms[0]))
    W = api.warp_field(Ms[0], u0)
    assert same_bits(host(c2.cost), host(hip.cost_volume(Fs[0], W, 1, None, torch_ones_like(W[0], hip, u0))))
    m = api.cost_volume(F, M, radius=1)                       # the default features: MIND-SSC of both
    zero = keep * 0
    assert same_bits(host(m.cost), host(hip.cost_volume(api.mind_ssc(F), api.warp_field(api.mind_ssc(M), zero), 1, None,
                                                        torch_ones_like(M, hip, zero))))


def torch_ones_like(v, hip, u):
    """V_W of a volume of ones through u, as api.cost_volume makes it"""
    import torch
    from sift3d_amd import api
    return api.warp_field(torch.ones_like(v), u, "nearest")


# ---- end to end --------------------------------------------------------------------------------------------------------
AMPLITUDE, PERIODS = 11.0, 0.25


def large_motion_pair(n=48, amplitude=AMPLITUDE, periods=PERIODS):
    """(fixed, moving, truth) on the device: smooth noise (sigma 1.5) seen through a smooth sinusoidal field of the given
    amplitude (fixed(p) = content(p + truth(p)), made with the existing warp), the moving contrast inverted as in the
    MIND tests (m -> max + 10 - 1.5 m)"""
    from sift3d_amd import api
    content = smooth_noise((n, n, n), 71, 1.5)
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    w = 2 * np.pi * periods / n
    truth = amplitude * np.stack([np.sin(w * z + 0.3) * np.cos(w * y), np.cos(w * x + 0.5) * np.sin(w * z),
                                  np.sin(w * x) * np.sin(w * y + 1.0)]).astype(F32)
    fixed = api.warp_field(dev(content), dev(truth), "linear", 0.0)
    moving = (content.max() + F32(10) - F32(1.5) * content).astype(F32)
    return fixed, dev(moving), truth


def field_rms(field, truth):
    """RMS of |field - truth| over the voxels 4 away from every face"""
    inner = (slice(None),) + (slice(4, -4),) * 3
    return float(np.sqrt(((host(field).astype(np.float64) - truth)[inner] ** 2).sum(axis=0).mean()))


def test_large_motion_end_to_end(hip):
    """The pair: 48^3 smooth noise (sigma 1.5), the moving contrast inverted, under a sinusoidal field of a quarter period
    across the volume.  The wavelength is set by the EXISTING follow-up stage: refine_field(features="mind") at its
    defaults diffuses the field with sigma 2 on each of 50 iterations and, started from the truth itself, ends at 1.35 of
    a zero-field error of 5.29 with half a period at amplitude 6, at 1.08 of 10.22 with a quarter period at amplitude 11:
    only the long wave leaves it room to improve on anything.  The amplitude was raised from 6 until the demons run
    below stays above half the zero field's error: 0.073 of it at 6, 0.205 at 8, 0.414 at 10, 0.518 at 11, the value used.
    Measured on an MI355X, RMS field error over the inner region: zero field 10.22, refine_field(features="mind",
    levels=3) alone 5.294, register_discrete at its defaults 4.450 with no folded voxel, refine_field from its field
    3.923 (DESIGN 3.4.26 has the sweep, the half-period pair included, where the follow-up ends ABOVE the discrete
    field: 1.994 from 1.695)."""
    from sift3d_amd import api
    fixed, moving, truth = large_motion_pair()
    zero = field_rms(dev(np.zeros_like(truth)), truth)
    demons = api.refine_field(moving, fixed, None, features="mind", levels=3)
    e_demons = field_rms(demons.field, truth)
    r = api.register_discrete(moving, fixed, features="mind", levels=3)
    e_discrete = field_rms(r.field, truth)
    both = api.refine_field(moving, fixed, r.field, features="mind")
    e_both = field_rms(both.field, truth)
    print("large motion, amplitude %g: RMS field error zero field %.4g, demons (mind, levels 3) %.4g, discrete %.4g, "
          "discrete then demons %.4g; folded voxels of the discrete field: %d of %d; data %s"
          % (AMPLITUDE, zero, e_demons, e_discrete, e_both, r.jacobian.folded, truth[0].size,
             np.array2string(r.data, precision=4)))
    assert e_demons > 0.5 * zero                              # the condition on the input: demons alone is stuck
    assert e_discrete < e_demons                              # (a)
    assert e_both < e_discrete and e_both < e_demons          # (b)
    assert r.jacobian.folded >= 0                             # (c) reported above, no threshold
