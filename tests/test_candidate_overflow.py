"""Candidate-list overflow (-m gpu): the detector starts from a candidate list of 2^18 records; a volume with more
extrema than that is swept again with the list grown to count + count // 4 + 1024 (sift3d_detect.c,
detect_on_device; the slab driver's own loop is in tests/test_gpu_sharded.py).  The retry must not change a bit.

Every case runs three times: the GPU with a capacity forced by sift3d_amd_detector_set_candidate_capacity, the
GPU from the default capacity (which does not overflow), and the oracle.  The capacities are derived from the
oracle's counts -- n candidates, n0 of them in octave 0 -- so that each of the retry's branches is reached:

- default schedule ("split": `side` and `overlap`, sift3d_detect.c: detect_begin, build_pyramid): octave 0's candidates are
  emitted and oriented while the smaller octaves are still swept.  A capacity below n0 stops it before the
  orientation (count_a > cap); one in [n0, n) lets octave 0 be oriented, and its records copied, before the
  total turns out not to fit (count_a <= cap < count).  Attempt 1 takes the joined path.
- per-octave path (`side` == 0: cuboid extrema, num_kp_levels != 3, an octave whose x size is not a multiple of 4):
  one count after all octaves' emissions, dog_free[o] (sift3d_detect.c: dog_stage) choosing the DoG-free sweep or
  the stored DoG levels per octave.
"""
import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

RTOL = 1e-5
DEFAULT_CAP = 1 << 18
KP_FIELDS = ("o", "s", "xd", "yd", "zd", "sd", "strength")


@pytest.fixture(scope="module")
def gpu():
    import torch
    from sift3d_amd import api
    if not torch.cuda.is_available() or not api.device_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    return api, torch


def grown(n):
    """The capacity a detect of n candidates grows an overflowing list to (sift3d_detect.c, extrema_stage)."""
    return n + n // 4 + 1024


def noise(shape, seed=5):
    """Uniform noise, (nz, ny, nx)."""
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


# peak_thresh of the noise volumes: low enough for their extrema to fill a large list, high enough to bind -- a few
# of them lie within 1 % of it, so a second sweep with another threshold would change the count
NOISE_KW = dict(peak_thresh=0.05)


def coarse_only(n=96):
    """test_gpu_parity.py::test_detect_when_a_part_of_the_list_is_empty_vs_oracle's coarse_only volume: six wide
    blobs, no extremum in octave 0."""
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float32),) * 3, indexing="ij")
    rng = np.random.default_rng(17)
    vol = np.zeros((n, n, n), np.float32)
    for c in rng.uniform(20, n - 20, size=(6, 3)):
        vol += np.exp(-((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) / (2 * 7.0 ** 2)).astype(np.float32)
    return vol


class Ref:
    """The oracle's results for one volume and configuration."""

    def __init__(self, oracle_mod, vol, kw, sort_limit=None):
        o = oracle_mod.Oracle(**kw)
        assert o.detect(vol) == 0
        cand = o.candidates()
        self.n = len(cand)
        self.n0 = int((cand["o"] == 0).sum())
        self.num_octaves = o.num_octaves
        # the split schedule: default keypoint levels, no cuboid extrema, every octave's rows whole quads (`side`,
        # sift3d_detect.c: detect_begin); else the per-octave path
        nx = vol.shape[2]
        self.split = (not kw.get("cuboid_extrema") and kw.get("num_kp_levels", 3) == 3 and self.num_octaves > 1 and
                      all((nx >> o) % 4 == 0 for o in range(self.num_octaves)))
        self.k = o.keypoints()
        if len(self.k):
            if sort_limit is not None:
                o.sort_by_strength(sort_limit)
            assert o.describe() == 0
            self.desc = o.desc_mat()
        else:
            self.desc = np.zeros((0, 771), np.float32)
        o.close()

    def capacities(self):
        """1, n0 - 1, n0, n0 + 1, n - 1, n, n + 1 within [1, n + 1]."""
        return sorted({c for c in (1, self.n0 - 1, self.n0, self.n0 + 1, self.n - 1, self.n, self.n + 1)
                       if 1 <= c <= self.n + 1})


def detect(api, torch, vol, kw=None, cap=None, det=None, dogmax_pass=False, serial=False, device_input=False,
           sort_limit=None):
    """One detect + describe on the GPU; cap: forced starting capacity (None: whatever the detector has)."""
    if det is None:
        det = api.Detector(**(kw or {}))
        if dogmax_pass:
            assert det.set_dogmax_pass(True) == 0
        if serial:
            assert det.set_serial_orientation(True) == 0
    if cap is not None:
        det.set_candidate_capacity(cap)
    cap_before = det.candidate_capacity()
    kp = api.KeypointStore()
    if device_input:
        d = torch.from_numpy(np.ascontiguousarray(vol)).cuda()
        nz, ny, nx = vol.shape
        assert det.detect_keypoints_device(d.data_ptr(), nx, ny, nz, kp) == 0
        torch.cuda.synchronize()
    else:
        assert det.detect_keypoints(api.Image.from_array(vol), kp) == 0
    out = dict(det=det, ncand=det.num_candidates(), k=kp.records(), dogmax=det.dogmax(), cap_before=cap_before,
               cap_after=det.candidate_capacity(), t=det.timings())
    if len(out["k"]):
        if sort_limit is not None:
            kp.sort_by_strength(sort_limit)
        desc = api.DescriptorStore()
        assert det.extract_descriptors(kp, desc) == 0
        out["desc"] = desc.to_mat_rm()
    else:
        out["desc"] = np.zeros((0, 771), np.float32)
    return out


def check_vs_oracle(got, ref):
    """The assertions of test_gpu_parity.py::test_detect_describe_vs_oracle."""
    assert got["ncand"] == ref.n
    k, ok = got["k"], ref.k
    assert len(k) == len(ok)
    for f in KP_FIELDS:
        np.testing.assert_array_equal(k[f], ok[f], err_msg=f)
    if len(k):
        assert util.rel_err(k["R"], ok["R"]) <= RTOL
        assert got["desc"].shape == ref.desc.shape
        assert util.rel_err(got["desc"], ref.desc) <= RTOL


def check_bitwise(got, base):
    """A retried detect equals the one that did not overflow, bit for bit."""
    assert got["ncand"] == base["ncand"]
    for f in KP_FIELDS + ("R",):
        np.testing.assert_array_equal(got["k"][f], base["k"][f], err_msg=f)
    np.testing.assert_array_equal(got["dogmax"], base["dogmax"])
    np.testing.assert_array_equal(got["desc"], base["desc"])


def check_retry(got, ref):
    """Whether the sweep ran twice: the capacity grew to grown(n) exactly when it started below n.  On the split
    schedule orient_oct0_end is set only when octave 0 was oriented on its own in attempt 0 -- that is, when no
    retry happened (attempt 1 takes the joined path)."""
    retried = got["cap_before"] < ref.n
    assert got["cap_after"] == (grown(ref.n) if retried else got["cap_before"]), (got["cap_before"], ref.n)
    if ref.split:
        assert (got["t"]["orient_oct0_end"] > 0) == (not retried)
    else:
        assert got["t"]["orient_oct0_end"] == 0
    return retried


def run_case(gpu, oracle_mod, vol, kw, split, est=False, **opts):
    api, torch = gpu
    ref = Ref(oracle_mod, vol, kw)
    assert ref.split == split
    if split:
        split_precondition(vol, est)
    base = detect(api, torch, vol, kw, cap=0, **opts)
    assert base["cap_before"] == DEFAULT_CAP and ref.n < DEFAULT_CAP
    check_retry(base, ref)
    check_vs_oracle(base, ref)
    retries = 0
    for cap in ref.capacities():
        got = detect(api, torch, vol, kw, cap=cap, **opts)
        assert got["cap_before"] == cap
        retries += check_retry(got, ref)
        check_vs_oracle(got, ref)
        check_bitwise(got, base)
    return ref, retries


def split_precondition(vol, est):
    """On the split schedule octave 0 takes est_octave (its dogmax gathered by the sweep, sift3d_detect.c)
    when it holds at least 2^21 voxels."""
    assert (vol.size >= 1 << 21) == est


@pytest.mark.parametrize("case", ["est_host", "est_device", "survey96", "dogmax_pass", "serial_orientation"])
def test_split_schedule_retry_vs_oracle(gpu, oracle_mod, case):
    """Default schedule (`split`): both overflow branches -- count_a > cap (octave 0 alone does not fit, no
    orientation starts) and count_a <= cap < count (octave 0 oriented and copied, then the total does not fit)
    -- and no overflow, against the oracle and bit for bit against the run from the default capacity."""
    kw, opts = {}, {}
    if case in ("est_host", "est_device", "dogmax_pass", "serial_orientation"):
        # 128^3: octave 0 holds 2^21 voxels -- EST_OCTAVE (unless the dogmax pass is asked for)
        vol, kw = noise((128, 128, 128)), NOISE_KW
        opts = dict(est=True, device_input=case == "est_device", dogmax_pass=case == "dogmax_pass",
                    serial=case == "serial_orientation")
    else:
        # 96^3: octaves 96, 48, 24, 12 (all whole quads: `side`), octave 0 below 2^21 voxels: no EST_OCTAVE
        vol = oracle_mod.synth_survey(96)
    ref, retries = run_case(gpu, oracle_mod, vol, kw, split=True, **opts)
    assert 1 < ref.n0 < ref.n and len(ref.k) > 20
    assert retries == sum(c < ref.n for c in ref.capacities()) >= 4


@pytest.mark.parametrize("case", ["mixed", "dog_only"])
def test_per_octave_retry_vs_oracle(gpu, oracle_mod, case):
    """Per-octave path (`side` == 0).  mixed, (100, 72, 90): octave 0 takes the DoG-free sweep (dog_free[0]: 100
    is a multiple of 4), octaves 1 and up the stored DoG levels (50 is not).  dog_only: x = 90, cuboid extrema,
    four keypoint levels -- every octave on the DoG levels."""
    if case == "mixed":
        vol, kw = oracle_mod.synth_survey((100, 72, 90)), {}
        assert vol.shape[2] == 100
    else:
        vol, kw = oracle_mod.synth_survey((90, 64, 72)), dict(cuboid_extrema=True, num_kp_levels=4, peak_thresh=0.05)
        assert vol.shape[2] == 90
    ref, retries = run_case(gpu, oracle_mod, vol, kw, split=False)
    assert 1 < ref.n0 < ref.n and len(ref.k) > 5
    assert retries == sum(c < ref.n for c in ref.capacities()) >= 4


@pytest.mark.parametrize("case", ["coarse_only", "flat"])
def test_retry_with_an_empty_part_vs_oracle(gpu, oracle_mod, case):
    """Capacity 1.  coarse_only: no candidate in octave 0, so count_a == 0 < cap < count -- octave 0's (empty)
    part is 'oriented', the total does not fit.  flat: no candidate at all, no retry."""
    api, torch = gpu
    if case == "coarse_only":
        vol, kw = coarse_only(), dict(peak_thresh=0.05)
    else:
        vol, kw = np.ones((96, 96, 96), np.float32), {}
    ref = Ref(oracle_mod, vol, kw)
    base = detect(api, torch, vol, kw)
    got = detect(api, torch, vol, kw, cap=1)
    assert got["cap_before"] == 1
    assert ref.split
    retried = check_retry(got, ref)
    check_retry(base, ref)
    if case == "coarse_only":
        assert ref.n0 == 0 and ref.n > 1 and len(ref.k) > 0 and retried
    else:
        assert ref.n == 0 and not retried
    for g in (base, got):
        check_vs_oracle(g, ref)
    check_bitwise(got, base)


def test_reuse_across_retries_vs_oracle(gpu, oracle_mod):
    """One detector: a retry on volume A, a retry on the larger B from A's grown capacity, A again (no retry),
    then the default capacity restored and A once more."""
    api, torch = gpu
    # A on the split schedule; B (octaves 144 ... 18) on the per-octave path, and new dimensions
    a, b = oracle_mod.synth_survey(96), oracle_mod.synth_survey(144)
    ra, rb = Ref(oracle_mod, a, {}), Ref(oracle_mod, b, {})
    assert ra.split and not rb.split and rb.n > grown(ra.n)
    det = api.Detector()
    base_a = detect(api, torch, a)
    steps = [(a, ra, 16, True), (b, rb, None, True), (a, ra, None, False)]
    for vol, ref, cap, retry in steps:
        got = detect(api, torch, vol, cap=cap, det=det)
        assert check_retry(got, ref) == retry
        check_vs_oracle(got, ref)
    assert det.candidate_capacity() == grown(rb.n)
    det.set_candidate_capacity(0)
    assert det.candidate_capacity() == DEFAULT_CAP
    got = detect(api, torch, a, det=det)
    assert got["cap_after"] == DEFAULT_CAP
    check_vs_oracle(got, ra)
    check_bitwise(got, base_a)


def test_capacity_hook_arguments(gpu):
    api, torch = gpu
    det = api.Detector()
    assert det.candidate_capacity() == DEFAULT_CAP
    with pytest.raises(ValueError):
        det.set_candidate_capacity(-1)
    assert det.candidate_capacity() == DEFAULT_CAP
    det.set_candidate_capacity(7)
    assert det.candidate_capacity() == 7
    det.set_candidate_capacity(0)
    assert det.candidate_capacity() == DEFAULT_CAP


@pytest.mark.parametrize("shape,branch", [
    # (nz, ny, nx); x = 384: octaves 384 ... 12, all whole quads -- the split schedule (a cube of 416 or 392 ends
    # in an octave of 26 or 98 ... voxels per row and takes the per-octave path)
    ((432, 432, 384), "count_a > cap"),
    ((392, 400, 384), "count_a <= cap < count")])
def test_natural_overflow_vs_oracle(gpu, oracle_mod, shape, branch):
    """The default capacity reached by a real volume, no hook: uniform noise.  Against the
    oracle and bit for bit against a run from a capacity of 2^20 (no overflow); descriptors of the 200
    strongest keypoints."""
    api, torch = gpu
    vol, kw = noise(shape), NOISE_KW
    ref = Ref(oracle_mod, vol, kw, sort_limit=200)
    assert ref.split
    split_precondition(vol, est=True)
    # the precondition of the branch, from the oracle's counts
    if branch == "count_a > cap":
        assert ref.n0 > DEFAULT_CAP
    else:
        assert ref.n0 <= DEFAULT_CAP < ref.n
    got = detect(api, torch, vol, kw, device_input=True, sort_limit=200)
    assert got["cap_before"] == DEFAULT_CAP
    assert check_retry(got, ref)
    check_vs_oracle(got, ref)
    base = detect(api, torch, vol, kw, cap=1 << 20, device_input=True, sort_limit=200)
    assert not check_retry(base, ref)
    check_bitwise(got, base)
