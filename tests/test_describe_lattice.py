"""GPU (-m gpu): the lattice variant of the fast descriptor kernel, k_describe<false, true>.

A keypoint that sits on a voxel and carries its level's own scale, at a level with equal power-of-two units, takes
the lattice variant (window coordinates from the integer offsets, table weights with no expf code); every
other record of the same list takes the generic fast kernel in a launch of its own.  Results must not depend on
which of the two computes a row:

  (a) on-voxel, caller-made keypoints with each level's own sd, through extract_descriptors, equal bit for bit
      the rows of the same records through the table-less stage entry (sift3d_hip_describe: the generic kernel,
      whose expf is bit-identical to the table by construction);
  (b) a mixed list -- the records of (a) interleaved with off-voxel records and one with a foreign sd -- gives
      every record the row it gets when described alone (the partition and the row1 mapping);
  (c) tests/golden/describe_lattice.json holds the sha1 of the rows of (a) and (b) as the commit BEFORE the
      variant computed them on an MI355X (`python -m tests.test_describe_lattice OUT.json` with that commit's
      library writes the file).

The list of (a): s = 0, 1, 2 of octave 0; a level of octave 1 (units 2: the fold with iu != 1); the volume's
corners (clipped boxes, empty parts); the widest window; a keypoint one of whose parts ends in a batch of 1..3
voxels and one with a last batch of exactly 32 (`work_items` of tests/test_describe_quad_commit.py re-derives
both on every run).
"""
import json
import os
import sys

import numpy as np
import pytest

from tests import util
from tests.test_describe_quad_commit import I3, N, SEED, work_items

F = np.float32


def rot(axis, deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    R = np.eye(3)
    i, j = [(1, 2), (0, 2), (0, 1)][axis]
    R[i, i], R[j, j], R[i, j], R[j, i] = c, c, -s, s
    return R.astype(F)


TAIL = ((20.0, 20.0, 20.0), rot(0, 45))   # s = 0: parts 7746, 6897, 7040, 8623; 7746 = 121 * 64 + 2
B32 = ((3.0, 20.0, 20.0), rot(1, 20))     # s = 0: parts 5042, 3936, 3578, 5874; 3936 = 61 * 64 + 32


def level_sd(oracle, o, s):
    return oracle.level(0, o, s)[2]


def lattice_rows(oracle):
    """[(what, o, s, centre, sd, R)]: every record sits on a voxel and carries its level's sd."""
    sd = [level_sd(oracle, 0, s) for s in range(3)]
    return [
        ("s0", 0, 0, (20.0, 20.0, 20.0), sd[0], I3),
        ("s1", 0, 1, (19.0, 21.0, 20.0), sd[1], rot(2, 30)),
        ("s2 widest", 0, 2, (20.0, 19.0, 21.0), sd[2], I3),
        ("octave 1", 1, 0, (10.0, 9.0, 11.0), level_sd(oracle, 1, 0), rot(1, 15)),
        ("corner", 0, 0, (0.0, 0.0, 0.0), sd[0], I3),
        ("corner far", 0, 1, (39.0, 39.0, 39.0), sd[1], I3),
        ("tail", 0, 0, TAIL[0], sd[0], TAIL[1]),
        ("b32", 0, 0, B32[0], sd[0], B32[1]),
    ]


def mixed_rows(oracle):
    """The lattice records interleaved with records the generic kernel must take."""
    sd = [level_sd(oracle, 0, s) for s in range(3)]
    other = [
        ("off x", 0, 0, (20.25, 20.0, 20.0), sd[0], I3),
        ("off y", 0, 1, (19.0, 21.25, 20.0), sd[1], rot(2, 30)),
        ("off z", 0, 2, (20.0, 19.0, 20.75), sd[2], I3),
        ("off octave 1", 1, 0, (10.25, 9.0, 11.0), level_sd(oracle, 1, 0), rot(1, 15)),
        ("foreign sd", 0, 0, (20.0, 20.0, 20.0), 0.9 * sd[0], I3),
        ("off corner", 0, 0, (0.25, 0.0, 0.0), sd[0], I3),
        ("foreign sd s1", 0, 1, (19.0, 21.0, 20.0), sd[0], I3),
        ("off all", 0, 0, (19.25, 20.5, 20.75), sd[0], rot(0, 45)),
    ]
    out = []
    for a, b in zip(lattice_rows(oracle), other):
        out += [b, a]
    return out


def records(rows, dtype):
    out = np.zeros(len(rows), dtype)
    for k, (_, o, s, c, sd, R) in zip(out, rows):
        k["o"], k["s"], k["sd"], k["R"] = o, s, sd, R
        k["xd"], k["yd"], k["zd"] = c
    return out


def describe(api, det, recs):
    assert det.set_exact_descriptors(-1) == 0
    kp = api.KeypointStore()
    assert kp.set_records(recs) == 0
    desc = api.DescriptorStore()
    assert det.extract_descriptors(kp, desc) == 0
    return desc.to_mat_rm()[:, 3:] + F(0.0)


def setup(api, oracle_mod):
    vol = oracle_mod.synth_lattice(N, seed=SEED)
    det, kp = api.Detector(), api.KeypointStore()
    assert det.detect_keypoints(api.Image.from_array(vol), kp) == 0
    o = oracle_mod.Oracle()
    assert o.detect(vol) == 0
    return det, o


def rows_of(api, det, o):
    """{what: rows} of the two lists through extract_descriptors."""
    return {"lattice": describe(api, det, records(lattice_rows(o), api.KP_DTYPE)),
            "mixed": describe(api, det, records(mixed_rows(o), api.KP_DTYPE))}


def digests(rows, got):
    return {r[0]: util.digest(g) for r, g in zip(rows, got)}


@pytest.fixture(scope="module")
def case(oracle_mod):
    import torch
    from sift3d_amd import api
    if not torch.cuda.is_available() or not api.device_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    det, o = setup(api, oracle_mod)
    return api, det, o, rows_of(api, det, o)


@pytest.mark.gpu
def test_list_meets_the_edges(oracle_mod):
    """The list is what the docstring says (the kernel's window arithmetic, restated; no GPU work)."""
    o = oracle_mod.Oracle()
    assert o.detect(oracle_mod.synth_lattice(N, seed=SEED)) == 0
    items = {r[0]: work_items(*r[3], r[4], r[5]) for r in lattice_rows(o) if r[1] == 0}
    assert any(1 <= p % 64 <= 3 for p in items["tail"][1]), items["tail"]
    assert any(p % 64 == 32 for p in items["b32"][1]), items["b32"]
    for w in ("corner", "corner far"):
        assert items[w][0] > 0, (w, items[w])
    assert items["s2 widest"][0] == max(v[0] for v in items.values())
    for _, _, _, c, _, _ in lattice_rows(o):
        assert all(float(v).is_integer() for v in c)


@pytest.mark.gpu
def test_lattice_rows_equal_the_generic_kernels(case):
    """(a): the API's rows against the table-less stage entry over the detector's own Gaussian levels."""
    import torch
    from sift3d_amd import hip
    api, det, o, got = case
    rows = lattice_rows(o)
    ngl, levels = 6, []
    for oc in range(2):
        for s in range(-1, ngl - 1):
            t = torch.from_numpy(det.level(0, oc, s)).cuda()
            levels.append(dict(data=t, off=0, nz_glob=t.shape[0], units=(2.0 ** oc,) * 3, octave=oc,
                               sd=level_sd(o, oc, s)))
    d_levels, _ = hip.level_table(levels)
    kps = np.zeros(len(rows), hip.KP_DTYPE)
    for k, (_, oc, s, c, sd, R) in zip(kps, rows):
        k["R"], k["level"], k["row1"], k["sd"] = np.asarray(R, F).reshape(9), oc * ngl + s + 1, 0, sd
        k["cx"], k["cy"], k["cz"] = c
    want = hip.describe(d_levels, kps) + F(0.0)
    bad = [r[0] for r, g, w in zip(rows, got["lattice"], want) if not np.array_equal(g, w)]
    assert not bad, "rows %s differ from the generic kernel's" % bad
    assert all(np.abs(g).sum() > 0 for g in got["lattice"])


@pytest.mark.gpu
def test_mixed_list_rows_equal_each_record_alone(case):
    """(b): the partition into two launches and the row1 mapping."""
    api, det, o, got = case
    rows = mixed_rows(o)
    recs = records(rows, api.KP_DTYPE)
    bad = [r[0] for i, r in enumerate(rows) if not np.array_equal(describe(api, det, recs[i:i + 1])[0], got["mixed"][i])]
    assert not bad, "rows %s of the mixed list differ from the record described alone" % bad
    # the lattice records of the mixed list are those of (a)
    np.testing.assert_array_equal(got["mixed"][1::2], got["lattice"])


@pytest.mark.gpu
def test_rows_are_the_parent_commits(case):
    """(c)"""
    api, det, o, got = case
    with open(os.path.join(util.GOLDEN, "describe_lattice.json")) as f:
        gold = json.load(f)
    assert digests(lattice_rows(o), got["lattice"]) == gold["lattice_row_sha1"]
    assert digests(mixed_rows(o), got["mixed"]) == gold["mixed_row_sha1"]
    assert util.digest(got["lattice"]) == gold["lattice_sha1"] and util.digest(got["mixed"]) == gold["mixed_sha1"]


if __name__ == "__main__":
    # python -m tests.test_describe_lattice OUT.json: the golden file, from the library that is loaded
    from oracle import sift3d_oracle
    from sift3d_amd import api as _api
    _det, _o = setup(_api, sift3d_oracle)
    _got = rows_of(_api, _det, _o)
    with open(sys.argv[1], "w") as _f:
        json.dump({"lattice_row_sha1": digests(lattice_rows(_o), _got["lattice"]),
                   "mixed_row_sha1": digests(mixed_rows(_o), _got["mixed"]),
                   "lattice_sha1": util.digest(_got["lattice"]), "mixed_sha1": util.digest(_got["mixed"])},
                  _f, indent=1)
        _f.write("\n")
