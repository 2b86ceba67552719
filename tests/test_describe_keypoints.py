"""GPU (-m gpu): describe on CALLER-MADE keypoint lists against the reference (tests/golden/g7_*).

sift3d_extract_descriptors describes any keypoint store whose positions lie inside the image and whose sd is
positive (verify_keys, sift.c:1171-1212), not only the keypoints detect produced.  The g7 fixtures hold the
reference's descriptors of lists that detect never makes: sub-voxel centres, sd one ulp off / 0.5x / 2x the
level's / tiny, levels s = -1 .. K + 1 of every octave, random rotations and reflections, scaled and sheared
(non-orthonormal) R, axis-aligned gradients on icosahedron edges, windows clipped on all six faces, a window row
wider than 1024 voxels, windows of more than 1.9e5 voxels on levels 0 / 1, and the reference's refusals.

Bars: the reference-order kernel (set_exact_descriptors(1)) is the reference bit for bit; the fast commit
(automatic and -1) within 1e-5 elementwise for keypoints whose own window holds at most 1.9e5 voxels, and in the
automatic mode the rows of larger windows are the reference-order kernel's, bit for bit.
"""
import numpy as np
import pytest

from tests import util
from tests.test_oracle_golden import G7, g7_cases, g7_records

pytestmark = pytest.mark.gpu

RTOL = 1e-5
SWITCH_VOXELS = 1.9e5   # include/sift3d_amd.h, sift3d_amd_detector_set_exact_descriptors


@pytest.fixture(scope="module")
def gpu():
    import torch
    from sift3d_amd import api
    if not torch.cuda.is_available() or not api.device_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    return api


def window_voxels(k, units):
    """Voxels of a keypoint's own window, as the automatic mode counts them: the descriptor cube's side
    2 * (2 * sd * 7.071067812 / sqrt(2)) (sift.c:1453-1456) cubed, over the voxel volume of its octave."""
    side = 2.0 * (2.0 * k["sd"] * 7.071067812 / np.sqrt(2.0))
    return side ** 3 / (float(np.prod(units)) * 8.0 ** k["o"].astype(np.float64))


def detector(api, oracle_mod, g):
    vol = util.golden_input(g, oracle_mod)
    det, kp = api.Detector(), api.KeypointStore()
    assert det.detect_keypoints(api.Image.from_array(vol, tuple(g["units"])), kp) == 0
    return det, kp


def describe(api, det, recs, mode, keep=False):
    """extract_descriptors on a store filled with `recs`: (return code, descriptor store)."""
    assert det.set_exact_descriptors(mode) == 0
    kp = api.KeypointStore()
    assert kp.set_records(recs) == 0
    desc = api.DescriptorStore()
    if keep:
        assert desc.keep_device(True) == 0
    return det.extract_descriptors(kp, desc), desc


def hist(desc):
    return desc.to_mat_rm()[:, 3:] + np.float32(0.0)   # (-0.0 folded into +0.0)


@pytest.mark.parametrize("name", G7)
def test_g7_against_reference(gpu, oracle_mod, name):
    api = gpu
    g = util.load(name)
    det, _ = detector(api, oracle_mod, g)
    units = tuple(g["units"])
    failures = []
    for case in g7_cases(g):
        recs = g7_records(g, case, api.KP_DTYPE)
        ok = bool(g[case + "_ok"])
        rc1, d1 = describe(api, det, recs, 1)
        if not ok:
            # verify_keys: the reference's verdict, in every mode
            assert rc1 != 0, case
            assert describe(api, det, recs, 0)[0] != 0 and describe(api, det, recs, -1)[0] != 0, case
            continue
        assert rc1 == 0, case
        want = g[case + "_hist"] + np.float32(0.0)
        # the store's coordinates: xd * 2^o etc. (sift.c:1530-1532), exactly
        np.testing.assert_array_equal(d1.xyz(), g[case + "_desc_xyzsd"][:, :3], err_msg=case)
        m1 = hist(d1)
        bad = np.nonzero((m1 != want).any(axis=1))[0]
        if len(bad):
            failures.append("%s exact: rows %s differ from the reference (max rel %.3g)"
                            % (case, bad.tolist(), util.rel_err(m1[bad], want[bad])))
        small = window_voxels(recs, units) <= SWITCH_VOXELS
        rc0, d0 = describe(api, det, recs, 0)
        assert rc0 == 0, case
        m0 = hist(d0)
        np.testing.assert_array_equal(d0.xyz(), d1.xyz(), err_msg=case)
        if small.any():
            e = util.rel_err(m0[small], want[small])
            if not e <= RTOL:
                failures.append("%s auto: %.3g relative to the reference on windows <= 1.9e5 voxels" % (case, e))
        bigw = np.nonzero(~small & ~(m0 == m1).all(axis=1))[0]
        if len(bigw):
            failures.append("%s auto: rows %s (windows > 1.9e5 voxels) are not the reference-order kernel's "
                            "(max rel %.3g to the reference)" % (case, bigw.tolist(),
                                                                 util.rel_err(m0[bigw], want[bigw])))
        rcf, df = describe(api, det, recs, -1)
        assert rcf == 0, case
        if small.any():
            e = util.rel_err(hist(df)[small], want[small])
            if not e <= RTOL:
                failures.append("%s fast: %.3g relative to the reference on windows <= 1.9e5 voxels" % (case, e))
        # two identical calls: bitwise identical results
        np.testing.assert_array_equal(hist(describe(api, det, recs, 0)[1]), m0, err_msg=case)
    assert not failures, "\n".join(failures)


def test_g7_exact_equals_oracle(gpu, oracle_mod):
    """The reference-order kernel against the restatement on the same lists (the restatement is itself pinned
    to the g7 rows bit for bit by tests/test_oracle_golden.py)."""
    api = gpu
    g = util.load("g7_survey64")
    det, _ = detector(api, oracle_mod, g)
    o = oracle_mod.Oracle()
    assert o.detect(util.golden_input(g, oracle_mod)) == 0
    for case in ("subvox", "levels", "nonortho", "border"):
        assert o.set_keypoints(g7_records(g, case, oracle_mod.KP_DTYPE)) == 0 and o.describe() == 0
        rc, d = describe(api, det, g7_records(g, case, api.KP_DTYPE), 1)
        assert rc == 0
        np.testing.assert_array_equal(hist(d), o.descriptors()["hist"] + np.float32(0.0), err_msg=case)


def test_pyramid_levels_outside_are_refused(gpu, oracle_mod):
    """o / s outside the pyramid: refused (the GPU's own rule -- the reference would read beyond its pyramid)."""
    api = gpu
    g = util.load("g7_survey64")
    det, _ = detector(api, oracle_mod, g)
    base = g7_records(g, "subvox", api.KP_DTYPE)[:3]
    assert describe(api, det, base, 0)[0] == 0
    for o, s in ((int(g["num_octaves"]), 0), (-1, 0), (0, -2), (0, 5)):
        recs = base.copy()
        recs["o"][1], recs["s"][1] = o, s
        recs["xd"][1] = recs["yd"][1] = recs["zd"][1] = 1.0
        for mode in (0, 1, -1):
            assert describe(api, det, recs, mode)[0] != 0, (o, s, mode)
    assert describe(api, det, base[:0], 0)[0] != 0          # verify_keys: no keypoints


def _mixed_list(api, g, kp):
    """detect's keypoints and the g7 lists of every level, shuffled and three times over (duplicates)."""
    parts = [kp.records()] + [g7_records(g, c, api.KP_DTYPE) for c in ("levels", "subvox", "ulp", "scale", "rot")]
    base = np.concatenate(parts)
    rng = np.random.Generator(np.random.PCG64(77))
    idx = rng.permutation(np.tile(np.arange(len(base)), 3))
    return base, idx


@pytest.mark.parametrize("mode", [0, 1])
def test_order_duplicates_and_list_sizes(gpu, oracle_mod, mode):
    """A shuffled, mixed-level list with duplicates comes back in input order; one detector describes a list
    3x longer than detect's, then a single keypoint, then the long list again (its host and device lists grow,
    shrink and are reused) -- every result equals a fresh detector's."""
    api = gpu
    g = util.load("g7_survey64")
    det, kp = detector(api, oracle_mod, g)
    base, idx = _mixed_list(api, g, kp)
    assert len(idx) >= 3 * len(kp) and len(kp) > 0
    fresh, _ = detector(api, oracle_mod, g)
    rc, db = describe(api, fresh, base, mode)
    assert rc == 0
    mb = hist(db)
    runs = []
    for recs in (base[idx], base[idx[:1]], base[idx]):
        rc, d = describe(api, det, recs, mode)
        assert rc == 0
        runs.append(hist(d))
        f, _ = detector(api, oracle_mod, g)
        rc, df = describe(api, f, recs, mode)
        assert rc == 0
        np.testing.assert_array_equal(runs[-1], hist(df))
    np.testing.assert_array_equal(runs[0], mb[idx])
    np.testing.assert_array_equal(runs[1], mb[idx[:1]])
    np.testing.assert_array_equal(runs[2], runs[0])


def test_keep_device_copy(gpu, oracle_mod):
    """The HBM copy (keep_device) of caller-made lists: the host rows are those of a store without the copy, and
    the matcher reading the copies in place matches as on the host rows uploaded."""
    api = gpu
    g = util.load("g7_survey64")
    det, kp = detector(api, oracle_mod, g)
    parts = [kp.records()] + [g7_records(g, c, api.KP_DTYPE) for c in ("levels", "subvox", "nonortho")]
    a = np.concatenate(parts)
    perm = np.random.Generator(np.random.PCG64(5)).permutation(len(a))
    stores = []
    for recs in (a, a[perm]):
        rc, dk = describe(api, det, recs, 0, keep=True)
        assert rc == 0
        rc, dh = describe(api, det, recs, 0)
        assert rc == 0
        np.testing.assert_array_equal(hist(dk), hist(dh))
        up = api.DescriptorStore()
        mat = dh.to_mat_rm()
        assert up.set(np.concatenate([mat[:, :3], np.ones((len(mat), 1))], 1), mat[:, 3:]) == 0
        stores.append((dk, up))
    m = api.Matcher()
    on_device = m.match(stores[0][0], stores[1][0], 0.8)
    uploaded = m.match(stores[0][1], stores[1][1], 0.8)
    np.testing.assert_array_equal(on_device, uploaded)
    inv = np.argsort(perm)
    matched = on_device >= 0
    assert matched.sum() > len(a) // 2
    np.testing.assert_array_equal(on_device[matched], inv[matched])
