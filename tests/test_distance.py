"""GPU: the distance transforms, label surfaces, surface lists and surface-distance measures (include/sift3d_amd.h,
"Distance transforms and surface distances") against the numpy restatement (tests/distance_restatement.py), every
device output bit for bit.  Outputs sit between NaN guard bands, half of them 4 bytes past a 16-byte boundary."""
import collections

import numpy as np
import pytest

from tests import distance_restatement as dr

pytestmark = pytest.mark.gpu

GUARD = 64                                                   # floats on either side: a multiple of 16 bytes
SPACINGS = {"unit": (1.0, 1.0, 1.0), "aniso": (0.7, 1.3, 2.5), "z100": (1.0, 1.0, 100.0), "wide": (1e-3, 1.0, 1e3)}


@pytest.fixture(scope="module")
def env():
    import torch
    from sift3d_amd import api, hip
    if not api.device_available():
        pytest.fail("no HIP device")
    return torch, api, hip


class Guarded:
    """a float32 volume (or list) inside a NaN-filled buffer; shift = 1 puts it 4 bytes past a 16-byte boundary"""

    def __init__(self, torch, shape, shift):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD + 4,), float("nan"), dtype=torch.float32, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.lo = GUARD + shift
        self.t = self.buf[self.lo:self.lo + n].view(*shape)
        assert self.t.data_ptr() % 16 == 4 * shift

    def check(self):
        b = self.buf.cpu().numpy()
        n = self.t.numel()
        assert np.isnan(b[:self.lo]).all() and np.isnan(b[self.lo + n:]).all(), "a guard band was written"
        return b[self.lo:self.lo + n].reshape(tuple(self.t.shape)).copy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, "%s: %d of %d differ, first at %s: got %r want %r" % (
        what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def one(shape, *at):
    m = np.zeros(shape, np.float32)                          # shape and positions are (z, y, x)
    for p in at:
        m[p] = 1
    return m


def random_mask(shape, density, seed):
    return (np.random.default_rng(seed).uniform(0, 1, shape) < density).astype(np.float32)


def special_values():
    m = random_mask((3, 5, 9), 0.0, 0)
    m[0, 0, :4] = [np.nan, np.nextafter(np.float32(0.5), np.float32(0)), 0.5, np.inf]
    m[2, 4, 8] = -np.inf
    m[1, 2, 3] = 2.0
    return m


def planes_without_a_feature():
    m = np.zeros((9, 6, 7), np.float32)
    m[0] = random_mask((6, 7), 0.2, 3)
    m[5, 2, 3] = 1
    return m


# name -> (mask [nz, ny, nx], the spacings it runs with)
CASES = {
    "1x1x1_in": (np.ones((1, 1, 1), np.float32), ("unit", "aniso")),
    "1x1x1_out": (np.zeros((1, 1, 1), np.float32), ("unit",)),
    "nx1": (random_mask((6, 7, 1), 0.2, 1), ("unit", "aniso")),
    "67x9x5": (random_mask((5, 9, 67), 0.03, 2), ("unit", "aniso")),
    "5x9x67": (random_mask((67, 9, 5), 0.03, 3), ("unit", "aniso")),
    "130x3x2_last_chunk": (one((2, 3, 130), (1, 2, 129)), ("unit", "aniso")),
    "130x3x2_first_chunk": (one((2, 3, 130), (0, 1, 2)), ("unit", "aniso")),
    "130x3x2_both_ends": (one((2, 3, 130), (0, 0, 0), (0, 0, 129), (1, 1, 64)), ("aniso",)),
    "3x300x3_far_end": (one((3, 300, 3), (2, 299, 1)), ("unit", "aniso")),
    "3x3x300_far_end": (one((300, 3, 3), (299, 1, 2)), ("unit", "aniso")),
    "empty": (np.zeros((4, 5, 70), np.float32), ("unit", "aniso")),
    "full": (np.ones((4, 5, 70), np.float32), ("unit", "aniso")),
    "ties": (one((5, 5, 9), (2, 2, 1), (2, 2, 7), (0, 2, 4), (4, 2, 4)), ("unit", "aniso")),
    "empty_planes": (planes_without_a_feature(), ("unit", "aniso", "z100")),
    "special_values": (special_values(), ("unit", "aniso")),
    "random_2pct": (random_mask((13, 17, 20), 0.02, 4), ("unit", "aniso", "z100", "wide")),
    "random_50pct": (random_mask((13, 17, 20), 0.5, 5), ("unit", "aniso", "z100", "wide")),
    "random_98pct": (random_mask((13, 17, 20), 0.98, 6), ("unit", "aniso")),
}
PAIRS = [(c, s) for c, (_, sps) in CASES.items() for s in sps]


@pytest.mark.parametrize("case,spacing", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_distance_equals_restatement(env, case, spacing):
    torch, api, hip = env
    mask, sp = CASES[case][0], SPACINGS[spacing]
    shift = (len(case) + len(spacing)) & 1
    d_mask = torch.from_numpy(mask).cuda()
    want = dr.distance_sq(mask, sp)
    sq, root = Guarded(torch, mask.shape, shift), Guarded(torch, mask.shape, 1 - shift)
    hip.distance(d_mask, sp, "sq", out=sq.t)
    hip.distance(d_mask, sp, "root", out=root.t)
    got_sq, got_root = sq.check(), root.check()
    finite = np.isfinite(want)
    print("%s %s: D2 in [%g, %g], %d of %d voxels without a feature" % (
        case, spacing, want[finite].min() if finite.any() else np.inf, want[finite].max() if finite.any() else np.inf,
        int((~finite).sum()), want.size))
    assert_same_bits(got_sq, want, "D2")
    assert_same_bits(got_root, np.sqrt(want), "D")
    if spacing == "unit" and finite.any():                   # exact integers
        assert (got_sq[finite] == np.rint(got_sq[finite])).all()


def test_empty_and_full_values(env):
    torch, api, hip = env
    z = torch.zeros((4, 5, 70), device="cuda")
    assert bool(torch.isposinf(hip.distance(z, None, "sq")).all())
    assert bool((hip.distance(z + 1, (0.7, 1.3, 2.5), "sq") == 0).all())
    assert bool(torch.isposinf(hip.distance(z, None, "signed")).all())
    assert bool(torch.isneginf(hip.distance(z + 1, None, "signed")).all())


@pytest.mark.parametrize("case", ["67x9x5", "special_values", "random_50pct", "random_98pct", "empty", "full"])
def test_invert_equals_restatement(env, case):
    torch, api, hip = env
    mask, sp = CASES[case][0], SPACINGS["aniso"]
    out = Guarded(torch, mask.shape, 1)
    hip.distance(torch.from_numpy(mask).cuda(), sp, "sq", invert=True, out=out.t)
    assert_same_bits(out.check(), dr.distance_sq(mask, sp, invert=True), "D2 of the complement")


@pytest.mark.parametrize("case", ["67x9x5", "special_values", "random_2pct", "random_50pct", "random_98pct", "ties"])
@pytest.mark.parametrize("spacing", ["unit", "aniso"])
def test_signed_distance_equals_restatement(env, case, spacing):
    torch, api, hip = env
    mask, sp = CASES[case][0], SPACINGS[spacing]
    out = Guarded(torch, mask.shape, spacing == "unit")
    hip.distance(torch.from_numpy(mask).cuda(), sp, "signed", out=out.t)
    got = out.check()
    assert_same_bits(got, dr.distance_signed(mask, sp), "signed distance")
    inside = dr.mask_in(mask)
    np.testing.assert_array_equal(got > 0, ~inside)          # sign == outside, and no zero: the nearest voxel of the
    np.testing.assert_array_equal(got < 0, inside)           # other kind is at least one step along the finest axis away
    assert np.abs(got).min() >= np.sqrt(dr.weights(sp).min())


def test_api_distance_transform(env):
    torch, api, hip = env
    mask = CASES["random_2pct"][0]
    sp = SPACINGS["aniso"]
    want = dr.distance_sq(mask, sp)
    host = api.distance_transform(mask, spacing=sp)
    assert isinstance(host, np.ndarray)
    assert_same_bits(host, np.sqrt(want), "array in, array out")
    dev = api.distance_transform(torch.from_numpy(mask).cuda(), spacing=sp, squared=True)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda
    assert_same_bits(dev.cpu().numpy(), want, "tensor in, tensor out")
    assert_same_bits(api.distance_transform(mask != 0, spacing=sp, squared=True), want, "bool mask")
    assert_same_bits(api.distance_transform((mask * 7).astype(np.int16), spacing=sp, squared=True), want, "integer mask")
    assert_same_bits(api.distance_transform(mask, spacing=sp, squared=True, invert=True),
                     dr.distance_sq(mask, sp, invert=True), "invert")
    assert_same_bits(api.distance_transform(mask, spacing=sp, signed=True), dr.distance_signed(mask, sp), "signed")


# ---- surfaces and lists ------------------------------------------------------------------------------------------
def label_volume(shape, seed, labels=4):
    """blocky labels 0 .. labels-1: a coarse random grid repeated 3 x per axis, so that labels have interiors"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, labels, [(s + 2) // 3 for s in shape])
    v = np.repeat(np.repeat(np.repeat(coarse, 3, 0), 3, 1), 3, 2)[:shape[0], :shape[1], :shape[2]]
    return np.ascontiguousarray(v, np.float32)


@pytest.fixture(scope="module")
def volumes():
    """two 4-label volumes on one grid (label 3 touches every face somewhere) and their restated results, once"""
    LF, LM = label_volume((11, 13, 70), 11), label_volume((11, 13, 70), 12)
    sp = SPACINGS["aniso"]
    lists = {k: dr.surface_lists(LF, LM, k, sp) for k in (1, 2, 3)}
    return LF, LM, sp, lists


@pytest.mark.parametrize("label", [0, 1, 3, 7, -1])
def test_label_surface_equals_restatement(env, volumes, label):
    torch, api, hip = env
    LF = volumes[0]
    out = Guarded(torch, LF.shape, label & 1)
    _, count = hip.label_surface(torch.from_numpy(LF).cuda(), label, surface=out.t)
    want, n = dr.label_surface(LF, label)
    assert int(count.item()) == n and (n > 0) == (label in (0, 1, 3))
    assert_same_bits(out.check(), want, "surface of label %d" % label)


def test_label_surface_of_a_label_that_fills_the_grid(env):
    torch, api, hip = env
    for shape in ((1, 1, 1), (3, 4, 66), (5, 1, 2)):
        L = np.full(shape, 2, np.float32)
        out = Guarded(torch, shape, 1)
        _, count = hip.label_surface(torch.from_numpy(L).cuda(), 2, surface=out.t)
        want, n = dr.label_surface(L, 2)
        assert int(count.item()) == n
        assert_same_bits(out.check(), want, "surface of a full grid %s" % (shape,))


@pytest.mark.parametrize("short", [0, 1])
def test_surface_collect_capacity(env, volumes, short):
    torch, api, hip = env
    LF, LM, sp, lists = volumes
    surf, n = dr.label_surface(LF, 1)
    d2 = dr.distance_sq(dr.label_surface(LM, 1)[0], sp)
    out = Guarded(torch, (n - short,), short)
    _, count = hip.surface_collect(torch.from_numpy(surf).cuda(), torch.from_numpy(d2).cuda(), out.t)
    got = out.check()                                        # the sentinel right behind the list is a guard NaN
    assert int(count.item()) == n
    want = lists[1][0]
    if short:
        # n - 1 of the n values: a sub-multiset of the full list
        have, full = collections.Counter(bits(got).tolist()), collections.Counter(bits(want).tolist())
        assert not have - full and sum((full - have).values()) == 1
    else:
        assert np.sort(got).tobytes() == want.tobytes()


def stage_lists(torch, hip, LF, LM, k, sp):
    """the two sorted lists through the stage entries"""
    d_F, d_M = torch.from_numpy(LF).cuda(), torch.from_numpy(LM).cuda()
    sf, nf = hip.label_surface(d_F, k)
    sm, nm = hip.label_surface(d_M, k)
    out = []
    for a, na, b in ((sf, nf, sm), (sm, nm, sf)):
        lst = torch.empty(max(int(na.item()), 1), dtype=torch.float32, device="cuda")
        _, c = hip.surface_collect(a, hip.distance(b, sp, "sq"), lst)
        assert int(c.item()) == int(na.item())
        out.append(np.sort(lst[:int(na.item())].cpu().numpy()))
    return out


def same_bits64(a, b):
    return np.array(a, np.float64).tobytes() == np.array(b, np.float64).tobytes()


def test_surface_distances_of_random_labels(env, volumes):
    torch, api, hip = env
    LF, LM, sp, lists = volumes
    got = api.surface_distances(LF, LM, spacing=sp)
    np.testing.assert_array_equal(got.labels, [1, 2, 3])
    for j, k in enumerate((1, 2, 3)):
        d_fm, d_mf = stage_lists(torch, hip, LF, LM, k, sp)
        assert d_fm.tobytes() == lists[k][0].tobytes() and d_mf.tobytes() == lists[k][1].tobytes()
        want = dr.measures(*lists[k])
        row = tuple(col[j] for col in got[:7])
        print("label %d:" % k, row, got.n_fixed[j], got.n_moving[j])
        assert (int(got.n_fixed[j]), int(got.n_moving[j])) == (want.n_fixed, want.n_moving)
        assert same_bits64(row, want[:7]), (row, want)
    again = api.surface_distances(LF, LM, spacing=sp)
    for a, b in zip(got, again):                             # calling twice: identical bytes
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    tens = api.surface_distances(torch.from_numpy(LF).cuda(), torch.from_numpy(LM).cuda(), labels=[3, 1], spacing=sp)
    for name in api.SurfaceDistances._fields[:9]:
        np.testing.assert_array_equal(getattr(tens, name), getattr(got, name)[[2, 0]])


def test_surface_distances_of_two_boxes(env):
    """A 6 x 6 x 6 box and the same box 3 voxels further along x, 2 units per voxel along x: every voxel of the
    fixed box's x-low face is 3 voxels = 6 units from the moving surface (its own x-low face, straight ahead), and
    nothing is further; the moving box's x-high face is the same from the other side."""
    torch, api, hip = env
    F, M = np.zeros((16, 16, 20), np.float32), np.zeros((16, 16, 20), np.float32)
    F[5:11, 5:11, 4:10] = 1
    M[5:11, 5:11, 7:13] = 1
    got = api.surface_distances(F, M, spacing=(2.0, 1.0, 1.0))
    assert got.hausdorff[0] == 6.0 and got.max_fm[0] == 6.0 and got.max_mf[0] == 6.0
    assert int(got.n_fixed[0]) == int(got.n_moving[0]) == 6 ** 3 - 4 ** 3
    want = dr.surface_distances(F, M, [1], (2.0, 1.0, 1.0))[0]
    assert same_bits64([c[0] for c in got[:7]], want[:7])
    same = api.surface_distances(F, F)
    assert [float(c[0]) for c in same[:7]] == [0.0] * 7


def test_surface_distances_through_a_field_and_absent_labels(env, volumes):
    torch, api, hip = env
    LF, LM, sp, _ = volumes
    field = torch.zeros((3,) + LF.shape, device="cuda")
    field[0] = 3.0                                           # pulls the moving labels from 3 voxels further along x
    pre = np.zeros_like(LM)
    pre[:, :, :-3] = LM[:, :, 3:]
    through = api.surface_distances(LF, LM, transform=field, num_labels=6, spacing=sp)
    direct = api.surface_distances(LF, pre, num_labels=6, spacing=sp)
    np.testing.assert_array_equal(through.labels, [1, 2, 3, 4, 5])
    for a, b in zip(through, direct):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    assert np.isnan(through.hausdorff[3:]).all() and np.isnan(through.hd95[3:]).all()        # labels 4 and 5: absent
    assert (through.n_fixed[3:] == 0).all() and np.isfinite(through.hausdorff[:3]).all()
    only_fixed = np.where(LM == 2, 0, LM).astype(np.float32)                                 # label 2 absent from one
    got = api.surface_distances(LF, only_fixed, labels=[2], spacing=sp)
    assert got.n_fixed[0] > 0 and got.n_moving[0] == 0
    assert all(np.isnan(c[0]) for c in got[:7])
