"""Detect and describe on zero-background, integer and rescaled volumes (-m gpu): the drop-in API against the oracle.

The end-to-end tests elsewhere use dense, positive content of order 1.  Here (tests/pyramid_content.py,
detect_volume): twelve spikes on exact zero and a survey volume masked to a central box -- the reference's pyramid
then holds subnormals where the Gaussian tails run out --, CT-like integers with plateaus, and the survey volume
times 1e30, 1e-30, 1e-40 (a subnormal input, which its maximum divides back to order 1) and -1.

The assertions are those of tests/test_gpu_fuzz.py (the oracle's candidate count, every keypoint field exactly, R
and the descriptors within 1e-5 relative, identical refusals) and one more: every Gaussian and DoG level and every
max|DoG| equals the oracle's bit for bit.  The four rescaled volumes must give the counts of the plain survey volume.

Measured with the oracle on the CPU (tests/test_detect_content_host.py prints them):
  spikes64     798 candidates, 21 keypoints; 421 nonzero subnormal voxels in the Gaussian levels, 412 in the DoG levels
  boxed64       49 candidates, 10 keypoints;  61 in the Gaussian levels, 61 in the DoG levels
  integer48     94 candidates, 25 keypoints
  huge48, tiny48, subnormal48, negative48 and the plain survey volume: 92 candidates, 25 keypoints each
"""
import numpy as np
import pytest

from tests import pyramid_content as pc
from tests import util

pytestmark = pytest.mark.gpu
RTOL = 1e-5  # north_star: "descriptor and orientation floats within 1e-5 relative"


@pytest.fixture(scope="module")
def gpu():
    import torch
    from sift3d_amd import api, hip
    if not torch.cuda.is_available() or not api.device_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    hip.lib()
    return api, hip, torch


@pytest.fixture(scope="module")
def survey48_counts(oracle_mod):
    o = oracle_mod.Oracle()
    assert o.detect(oracle_mod.synth_survey(48)) == 0
    return len(o.candidates()), len(o.keypoints())


@pytest.mark.parametrize("name", pc.DETECT_CASES)
def test_detect_describe_on_hostile_content_vs_oracle(gpu, oracle_mod, survey48_counts, name):
    api, hip, torch = gpu
    vol, kw = pc.detect_volume(name, oracle_mod)
    det, kp, desc = api.Detector(**kw), api.KeypointStore(), api.DescriptorStore()
    rc = det.detect_keypoints(api.Image.from_array(vol), kp)
    o = oracle_mod.Oracle(**kw)
    assert rc == o.detect(vol) == 0
    # the pyramid, bit for bit (-0.0 and +0.0 told apart)
    dogmax = det.dogmax()
    assert len(dogmax) == o.num_octaves * 5
    subnormal = 0
    for oc in range(o.num_octaves):
        for which, n in ((0, 6), (1, 5)):
            for s in range(-1, n - 1):
                want = o.level(which, oc, s)[0]
                got = det.level(which, oc, s)
                subnormal += int(np.count_nonzero(pc.is_subnormal(want))) if which == 0 else 0
                bad = pc.bits(got) != pc.bits(want)
                assert not bad.any(), "%s: %s level octave %d, s %d: %d of %d words differ" \
                    % (name, "GD"[which], oc, s, bad.sum(), bad.size)
        # max|DoG|: the oracle keeps it for the keypoint levels s = 0, 1, 2 (sift.c:821-826 runs inside their loop);
        # the detector has it for all five DoG levels, the outer two against the oracle's level itself
        for s in range(-1, 4):
            want = np.abs(o.level(1, oc, s)[0]).max() if s in (-1, 3) else np.float32(o.dogmax(oc, s))
            assert pc.bits(dogmax[oc * 5 + s + 1]) == pc.bits(want), (name, oc, s)
    assert subnormal >= {"spikes64": 100, "boxed64": 10}.get(name, 0)
    # candidates, keypoints, orientation, descriptors: the assertions of test_gpu_fuzz.py
    assert det.num_candidates() == len(o.candidates()), name
    k, ok = kp.records(), o.keypoints()
    assert len(k) == len(ok) >= 4, name
    for f in ("o", "s", "xd", "yd", "zd", "sd", "strength"):
        np.testing.assert_array_equal(k[f], ok[f], err_msg=name + " " + f)
    assert util.rel_err(k["R"], ok["R"]) <= RTOL, name
    assert det.extract_descriptors(kp, desc) == 0 and o.describe() == 0, name
    assert util.rel_err(desc.to_mat_rm(), o.desc_mat()) <= RTOL, name
    if name in pc.SAME_AS_SURVEY48:
        assert (det.num_candidates(), len(k)) == survey48_counts, name
