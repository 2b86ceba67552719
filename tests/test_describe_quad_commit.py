"""GPU (-m gpu): the edges of k_describe's commit (quad lane roles, two record reads per four rounds).

Caller-made keypoints on a 40^3 lattice volume through extract_descriptors, reference-order kernel (bit for bit)
and fast kernel (1e-5) against the oracle restatement, as tests/test_describe_keypoints.py does.  The list is
chosen -- and `work_items` below re-derives it on every run, from the kernel's own window arithmetic in float32
-- so that the commit meets every edge it has:

  tail      a last batch of 1..3 voxels: a partial first chunk of four rounds, the other lanes stale
  b32, b33  a last batch of exactly 32 / 33 voxels: the second commit pass has no / one live round
  corner    a keypoint at the volume's corner: a clipped box, and empty parts for the fast kernel's split
  wide      level s = 2, the widest window: every part of the split holds voxels, many full batches
  edge      every gradient direction on an icosahedron edge (R projects the gradient on the x axis, which
            bisects an edge of the mesh): the 20-face fallback feeds the same records

A work item is what one wave sums: the whole window for the reference-order kernel, one of DPARTS = 4 ranges of
the window's planes for the fast one; batches are 64 voxels, the last one holds the rest.

tests/golden/describe_quad_commit.json holds the sha1 of the fast kernel's rows for this list as the commit
BEFORE the quad layout computed them on an MI355X: the layout changes no term and no order of any sum.
"""
import json
import os

import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

RTOL = 1e-5
N, SEED = 40, 11
F = np.float32


@pytest.fixture(scope="module")
def gpu():
    import torch
    from sift3d_amd import api
    if not torch.cuda.is_available() or not api.device_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    return api


def work_items(cx, cy, cz, sd, R, n=N):
    """Voxel counts of the work items of one level-0 keypoint on an n^3 volume with unit spacing: (the whole
    window, [the DPARTS parts]) -- k_describe's expressions (sift.c:96-108, 1453-1492), rounding by rounding."""
    R = np.asarray(R, F).reshape(9)
    cx, cy, cz = F(cx), F(cy), F(cz)
    sigma = F(sd * 7.071067812)
    rad = F(2.0 * float(sigma))
    half_w = F(float(rad) / 1.4142135623730951)
    bin_f = F(1.0) / ((F(2.0) * half_w) / F(4.0))
    rad2 = rad * rad

    def bounds(c):
        lo, hi = np.floor(c - rad), np.ceil(c + rad)
        return int(max(lo, F(1.0))), int(min(hi, F(n - 2)))

    (xs, xe), (ys, ye), (bzs, bze) = bounds(cx), bounds(cy), bounds(cz)
    ortho = max(abs(R[a] * R[b] + R[3 + a] * R[3 + b] + R[6 + a] * R[6 + b] - F(a == b))
                for a in range(3) for b in range(a, 3))
    cube_z = half_w * (abs(R[6]) + abs(R[7]) + abs(R[8])) * F(1.001) if ortho <= F(1e-4) else rad * F(1.001)
    zs = max(bzs, int(np.floor(cz - cube_z - F(1.0))))
    ze = min(bze, int(np.ceil(cz + cube_z + F(1.0))))
    z, y, x = np.meshgrid(np.arange(zs, ze + 1), np.arange(ys, ye + 1), np.arange(xs, xe + 1), indexing="ij")
    dx, dy, dz = x.astype(F) - cx, y.astype(F) - cy, z.astype(F) - cz
    sq = dx * dx + dy * dy + dz * dz
    vb = [((R[i] * dx + R[3 + i] * dy + R[6 + i] * dz) + half_w) * bin_f for i in range(3)]
    lo, hi = np.minimum(np.minimum(vb[0], vb[1]), vb[2]), np.maximum(np.maximum(vb[0], vb[1]), vb[2])
    planes = (~(sq > rad2) & ~(lo < 0) & ~(hi >= 4)).sum(axis=(1, 2))
    npl = max(ze - zs + 1, 0)
    cuts = [0, (33 * npl + 50) // 100, (npl + 1) // 2, (67 * npl + 50) // 100, npl]
    return int(planes.sum()), [int(planes[a:b].sum()) for a, b in zip(cuts[:-1], cuts[1:])]


I3 = np.eye(3, dtype=F)
X_ONLY = np.diag([1.0, 0.0, 0.0]).astype(F)   # vkp = (dx, 0, 0), the rotated gradient = (gx, 0, 0)


def keypoints(oracle, dtype):
    """[(what, record)] -- see the module's docstring; `oracle` holds the pyramid of the volume."""
    sd0, sd2 = oracle.level(0, 0, 0)[2], oracle.level(0, 0, 2)[2]
    rows = [
        # (what, s, centre, sd, R); R = I: the window is the cube |d| < half_w cut by the sphere of radius rad, and
        # the first six rows were found by a search over work_items (test_list_meets_the_edges holds them to it)
        ("exact tail", 0, (20.25, 20.0, 20.0), 0.33, I3),       # 323 voxels = 5 * 64 + 3
        ("exact b32", 0, (20.25, 19.5, 20.0), 0.48, I3),        # 864 = 13 * 64 + 32
        ("exact b33", 0, (20.0, 20.0, 20.0), 0.415, I3),        # 673 = 10 * 64 + 33
        ("fast tail", 0, (20.0, 20.0, 20.0), 0.525, I3),        # parts 323, 363, 242, 323
        ("fast b32", 0, (20.25, 20.0, 20.0), 0.3675, I3),       # parts 96, 98, 49, 96
        ("fast b33", 0, (20.25, 20.0, 20.0), 0.5725, I3),       # parts 353, 363, 242, 353
        ("corner", 0, (0.0, 0.0, 0.0), 0.25, I3),
        ("corner far", 1, (39.0, 39.0, 39.0), 0.3, I3),
        ("corner wide", 0, (0.0, 0.0, 0.0), sd0, I3),
        ("wide", 2, (20.0, 19.0, 21.0), sd2, I3),
        ("edge", 0, (20.0, 20.0, 20.0), sd0, X_ONLY),
        ("edge subvoxel", 0, (19.25, 20.5, 20.75), 0.7 * sd0, X_ONLY),
    ]
    out = np.zeros(len(rows), dtype)
    for k, (_, s, c, sd, R) in zip(out, rows):
        k["o"], k["s"], k["sd"], k["R"] = 0, s, sd, R
        k["xd"], k["yd"], k["zd"] = c
    return [r[0] for r in rows], out


@pytest.fixture(scope="module")
def case(gpu, oracle_mod):
    """The volume, a detector holding its pyramid, the list and the oracle's rows for it (computed once)."""
    api = gpu
    vol = oracle_mod.synth_lattice(N, seed=SEED)
    det, kp = api.Detector(), api.KeypointStore()
    assert det.detect_keypoints(api.Image.from_array(vol), kp) == 0
    o = oracle_mod.Oracle()
    assert o.detect(vol) == 0
    what, recs = keypoints(o, oracle_mod.KP_DTYPE)
    assert o.set_keypoints(recs) == 0 and o.describe() == 0
    want = o.descriptors()["hist"] + F(0.0)
    return api, det, what, keypoints(o, api.KP_DTYPE)[1], want


def describe(api, det, recs, mode):
    assert det.set_exact_descriptors(mode) == 0
    kp = api.KeypointStore()
    assert kp.set_records(recs) == 0
    desc = api.DescriptorStore()
    assert det.extract_descriptors(kp, desc) == 0
    return desc.to_mat_rm()[:, 3:] + F(0.0)


def test_list_meets_the_edges(oracle_mod):
    """The list is what the docstring says (no GPU work: the kernel's window arithmetic, restated)."""
    o = oracle_mod.Oracle()
    assert o.detect(oracle_mod.synth_lattice(N, seed=SEED)) == 0
    what, recs = keypoints(o, oracle_mod.KP_DTYPE)
    items = {w: work_items(k["xd"], k["yd"], k["zd"], k["sd"], k["R"]) for w, k in zip(what, recs)}
    assert 1 <= items["exact tail"][0] % 64 <= 3
    assert items["exact b32"][0] % 64 == 32 and items["exact b33"][0] % 64 == 33
    assert any(1 <= p % 64 <= 3 for p in items["fast tail"][1])
    assert any(p % 64 == 32 for p in items["fast b32"][1]) and any(p % 64 == 33 for p in items["fast b33"][1])
    for w in ("corner", "corner far"):
        assert items[w][0] > 0 and 0 in items[w][1], (w, items[w])
    assert 0 not in items["corner wide"][1]
    assert all(p >= 4 * 64 for p in items["wide"][1]), items["wide"]
    assert all(items[w][0] > 64 for w in ("edge", "edge subvoxel"))


def test_exact_is_the_oracle_bit_for_bit(case):
    api, det, what, recs, want = case
    got = describe(api, det, recs, 1)
    bad = [what[i] for i in np.nonzero((got != want).any(axis=1))[0]]
    assert not bad, "rows %s differ from the oracle" % bad


def test_fast_is_within_1e5_of_the_oracle(case):
    api, det, what, recs, want = case
    got = describe(api, det, recs, -1)
    errs = {w: util.rel_err(g, r) for w, g, r in zip(what, got, want)}
    print(errs)
    assert all(e <= RTOL for e in errs.values()), errs
    np.testing.assert_array_equal(describe(api, det, recs, -1), got)   # and the same bits on every call


def test_fast_rows_are_the_parent_commits(case):
    api, det, what, recs, _ = case
    with open(os.path.join(util.GOLDEN, "describe_quad_commit.json")) as f:
        gold = json.load(f)
    got = describe(api, det, recs, -1)
    assert gold["keypoints"] == what
    assert {w: util.digest(r) for w, r in zip(what, got)} == gold["fast_row_sha1"]
    assert util.digest(got) == gold["fast_sha1"]
