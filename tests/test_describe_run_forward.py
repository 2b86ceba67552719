"""GPU (-m gpu): k_describe's add-tid record stores (super-row record layout, histogram clear) change no bit.

The list and the three 40^3 volumes of tests/test_describe_run_forward_host.py (last batches of 1..3, 32 and 33
voxels, empty parts, the 20-face fallback, oblique windows; runs of repeated bins of every kind) through
extract_descriptors on caller-made keypoints, as tests/test_describe_keypoints.py does:

  the fast kernel's rows match the oracle restatement at 1e-5, the reference-order kernel's bit for bit;
  the fast rows' sha1 is that of tests/golden/describe_run_forward.json, which a build of the commit BEFORE the
  add-tid stores computed on an MI355X: the record layout changes no term and no order of any sum (the same
  rows pinned the register forwarding of repeated bins that DESIGN 3.3 measured and did not keep);
  a second run gives the same bytes.
"""
import json
import os

import numpy as np
import pytest

from tests import util
from tests.test_describe_run_forward_host import VOLUMES, keypoints, volume

pytestmark = pytest.mark.gpu

RTOL = 1e-5
F = np.float32


@pytest.fixture(scope="module")
def gpu():
    import torch
    from sift3d_amd import api
    if not torch.cuda.is_available() or not api.device_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    return api


def describe(api, det, recs, mode):
    assert det.set_exact_descriptors(mode) == 0
    kp = api.KeypointStore()
    assert kp.set_records(recs) == 0
    desc = api.DescriptorStore()
    assert det.extract_descriptors(kp, desc) == 0
    return desc.to_mat_rm()[:, 3:] + F(0.0)


def run_volume(api, oracle_mod, name):
    """(what, oracle rows, reference-order rows, fast rows, fast rows of a second call) of one volume."""
    vol = volume(name, oracle_mod)
    det = api.Detector()
    assert det.detect_keypoints(api.Image.from_array(vol), api.KeypointStore()) == 0
    o = oracle_mod.Oracle()
    assert o.detect(vol) == 0
    what, recs = keypoints(o, oracle_mod.KP_DTYPE)
    assert o.set_keypoints(recs) == 0 and o.describe() == 0
    want = o.descriptors()["hist"] + F(0.0)
    mine = keypoints(o, api.KP_DTYPE)[1]
    return what, want, describe(api, det, mine, 1), describe(api, det, mine, -1), describe(api, det, mine, -1)


@pytest.fixture(scope="module")
def runs(gpu, oracle_mod):
    return {name: run_volume(gpu, oracle_mod, name) for name in VOLUMES}


@pytest.mark.parametrize("name", VOLUMES)
def test_exact_is_the_oracle_bit_for_bit(runs, name):
    what, want, exact, _, _ = runs[name]
    bad = [what[i] for i in np.nonzero((exact != want).any(axis=1))[0]]
    assert not bad, "rows %s differ from the oracle" % bad


@pytest.mark.parametrize("name", VOLUMES)
def test_fast_is_within_1e5_of_the_oracle(runs, name):
    what, want, _, fast, _ = runs[name]
    errs = {w: util.rel_err(g, r) for w, g, r in zip(what, fast, want)}
    print(errs)
    assert all(e <= RTOL for e in errs.values()), errs


@pytest.mark.parametrize("name", VOLUMES)
def test_fast_rows_are_the_parent_commits(runs, name):
    what, _, _, fast, _ = runs[name]
    with open(os.path.join(util.GOLDEN, "describe_run_forward.json")) as f:
        gold = json.load(f)
    assert gold["keypoints"] == what
    assert {w: util.digest(r) for w, r in zip(what, fast)} == gold["fast_row_sha1"][name]
    assert util.digest(fast) == gold["fast_sha1"][name]


@pytest.mark.parametrize("name", VOLUMES)
def test_second_run_is_bitwise_identical(runs, name):
    _, _, _, fast, again = runs[name]
    assert fast.tobytes() == again.tobytes()
