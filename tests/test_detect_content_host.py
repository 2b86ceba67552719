"""CPU twin of tests/test_detect_content.py: the end-to-end volumes of tests/pyramid_content.py under the oracle
alone.  Every case must be accepted and leave enough keypoints to compare, the zero-background cases must really
put subnormals into the reference's Gaussian levels, and the rescaled survey volumes must give the counts of the
plain one.  The measured counts are printed (pytest -s); the GPU file's docstring quotes them."""
import numpy as np
import pytest

from tests import pyramid_content as pc


def _subnormal_voxels(o, which, nlevels):
    return sum(int(np.count_nonzero(pc.is_subnormal(o.level(which, oc, s)[0])))
               for oc in range(o.num_octaves) for s in range(-1, nlevels - 1))


@pytest.fixture(scope="module")
def survey48_counts(oracle_mod):
    o = oracle_mod.Oracle()
    assert o.detect(oracle_mod.synth_survey(48)) == 0
    return len(o.candidates()), len(o.keypoints())


@pytest.mark.parametrize("name", pc.DETECT_CASES)
def test_detect_case_under_the_oracle(oracle_mod, survey48_counts, name):
    vol, kw = pc.detect_volume(name, oracle_mod)
    vol2, _ = pc.detect_volume(name, oracle_mod)
    assert np.array_equal(pc.bits(vol), pc.bits(vol2))                   # seeded
    o = oracle_mod.Oracle(**kw)
    assert o.detect(vol) == 0
    ncand, nkp = len(o.candidates()), len(o.keypoints())
    sub_g, sub_d = _subnormal_voxels(o, 0, 6), _subnormal_voxels(o, 1, 5)
    print("%-12s %d candidates, %d keypoints; nonzero subnormal voxels: %d in the Gaussian levels, %d in the DoG "
          "levels; input max %.6g" % (name, ncand, nkp, sub_g, sub_d, np.abs(vol).max()))
    assert nkp >= 4
    assert o.describe() == 0 and len(o.descriptors()) == nkp
    if name == "spikes64":
        assert np.count_nonzero(vol) == 12 and sub_g >= 100
    if name == "boxed64":
        assert np.count_nonzero(vol) < vol.size // 10 and sub_g >= 10
    if name in pc.SAME_AS_SURVEY48:
        assert (ncand, nkp) == survey48_counts
