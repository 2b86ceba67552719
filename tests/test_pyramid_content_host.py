"""CPU twin of tests/test_pyramid_content.py: proves, with the oracle and no device, that its cases can fail.

For the classes meant to reach gradual underflow (subnormal, fade, faint_spikes) and every (shape, taps, spacing,
axes) of the GPU file's FIR table:
  * at least half of the oracle's output words are nonzero subnormals (faint_spikes is sparse: half of its nonzero
    output words), and
  * the same passes on the input with subnormals flushed to zero, every pass's output flushed too -- what a kernel
    built to flush, or one using an arithmetic form that ignores the denormal mode, would give -- differ from the
    oracle's output in at least half of the words (faint_spikes: of the nonzero words).
The halves are conditions on the content classes, not measurements: a shape that misses them gets other exponents
in tests/pyramid_content.py, never a lower bound.  The measured shares are printed (pytest -s).

The entries that divide by max|v| see an input of order 1 after the division, so the conditions are put on the
division itself: the `subnormal` class's maximum is a subnormal, and flushing the operands changes at least half
of the quotients of `subnormal` and `fade`.  `huge` gives no non-finite word anywhere.
"""
import collections

import numpy as np
import pytest

from tests import pyramid_content as pc

F = np.float32


@pytest.fixture(scope="module")
def gauss_filter():
    from sift3d_amd import api
    return api.gauss_filter


def _share(mask, of=None):
    return float(np.count_nonzero(mask if of is None else mask & of)) / max(int(mask.size if of is None
                                                                               else np.count_nonzero(of)), 1)


@pytest.mark.parametrize("path", pc.FIR_PATHS)
def test_fir_cases_reach_gradual_underflow(oracle_mod, gauss_filter, path):
    cases = [c for c in pc.FIR_CASES if c.path == path]
    assert cases
    lo = collections.defaultdict(lambda: [1.0, 1.0])
    for case in cases:
        t = pc.taps(case.taps, gauss_filter)
        for cls in case.classes():
            vol = pc.content(case, cls)
            if case.scaled:
                # the division: subnormal operands, and a result that flushing them changes
                q, mx = pc.scaled_input(vol)
                assert np.isfinite(q).all() and np.abs(q).max() == F(1.0)
                if cls == "subnormal":
                    assert pc.is_subnormal(mx), mx
                if cls in pc.UNDERFLOW_CLASSES:
                    with np.errstate(invalid="ignore", divide="ignore"):
                        fq = pc.ftz(vol) / pc.ftz(mx)
                    d = _share(pc.bits(fq) != pc.bits(q))
                    lo[cls][1] = min(lo[cls][1], d)
                    assert d >= 0.5, (case.id, cls, d)
                want = pc.oracle_fir(oracle_mod, q, t, case.axes, case.uf)
                assert np.isfinite(want).all(), (case.id, cls)
                continue
            want = pc.oracle_fir(oracle_mod, vol, t, case.axes, case.uf)
            assert np.isfinite(want).all(), (case.id, cls)       # `huge` included: no sum overflows
            if cls not in pc.UNDERFLOW_CLASSES:
                continue
            flushed = pc.oracle_fir(oracle_mod, vol, t, case.axes, case.uf, flush=True)
            of = (want != 0) if cls == "faint_spikes" else None
            assert of is None or np.count_nonzero(of) >= 20, (case.id, cls)
            sub = _share(pc.is_subnormal(want), of)
            dif = _share(pc.bits(flushed) != pc.bits(want), of)
            lo[cls][0], lo[cls][1] = min(lo[cls][0], sub), min(lo[cls][1], dif)
            assert sub >= 0.5, (case.id, cls, sub)
            assert dif >= 0.5, (case.id, cls, dif)
    for cls, (sub, dif) in sorted(lo.items()):
        print("%-16s %-13s smallest share of subnormal output words %.3f, of words a flush changes %.3f"
              % (path, cls, sub, dif))


def test_every_class_reaches_every_path_with_gaussian_taps():
    for path in pc.FIR_PATHS:
        assert any(c.taps[0] == "g" and not c.scaled for c in pc.FIR_CASES if c.path == path), path
    for path in ("1_x_u1", "3_sweep_u1_V4", "3_sweep_u1_V1", "4_dy", "9_yz_dma"):
        assert any(c.taps[0] == "s" for c in pc.FIR_CASES if c.path == path), path
    assert {c.path for c in pc.FIR_CASES} == set(pc.FIR_PATHS)
    assert len({c.id for c in pc.FIR_CASES}) == len(pc.FIR_CASES)
    assert max(int(np.prod(c.shape)) for c in pc.FIR_CASES) == 41 * 90 * 100
    # the entries that divide run on the three classes whose maxima matter
    assert [c.path for c in pc.FIR_CASES if c.scaled].count("10_xyz_dma") == 2
    assert {c.entry for c in pc.FIR_CASES if c.scaled} == {"x_scaled", "xyz_scaled"}


def test_classes_are_what_they_say():
    shape = (19, 21, 23)
    v = {k: g(shape, 5) for k, g in pc.CLASSES.items()}
    for k, a in v.items():
        assert a.dtype == F and a.shape == shape and np.isfinite(a).all(), k
        np.testing.assert_array_equal(pc.bits(a), pc.bits(pc.CLASSES[k](shape, 5)))       # seeded
    assert pc.is_subnormal(v["subnormal"]).mean() > 0.99
    f = v["fade"]
    assert not pc.is_subnormal(f[0, 0, :8]).any() and (f[0, 0, :8] != 0).all()      # a line starts normal ...
    assert pc.is_subnormal(f[0, 0, 18:]).all()                                      # ... and ends subnormal
    s = v["faint_spikes"]
    assert 0.005 < np.count_nonzero(s) / s.size < 0.02
    zero = s == 0
    assert (pc.bits(s[0::2])[zero[0::2]] == 0).all() and (pc.bits(s[1::2])[zero[1::2]] == 0x80000000).all()
    assert (np.abs(s[~zero]) >= F(2.0 ** -129)).all() and (np.abs(s[~zero]) < F(2.0 ** -128)).all()
    assert (s[~zero] > 0).any() and (s[~zero] < 0).any()
    assert np.abs(v["huge"]).max() > 2.0 ** 100
    assert (v["integer"] == np.round(v["integer"])).all() and len(np.unique(v["integer"])) < 1000
    assert (pc.bits(v["constant"]) == pc.bits(F(0.1))).all()


def test_absmax_sizes_are_what_grid_reduce_implies():
    T = pc.NTHR_MAX
    assert pc.grid_for(1, 4) == 1 and pc.grid_for(10 ** 9, 16) == 4096
    assert pc.grid_reduce(3 * 1024 * 1024) == 1024 and pc.grid_reduce(1024 * 1024 + 3) == 1024
    assert pc.grid_reduce(1023) == 1 and pc.grid_reduce(4 * 256 * 5) == 5
    zones = {n: pc.absmax_zones(n) for n in pc.ABSMAX_SIZES}
    assert [sorted(zones[n]) for n in pc.ABSMAX_SIZES[:5]] == [["tail"], ["tail"], ["quad"], ["quad", "tail"],
                                                               ["quad", "tail"]]
    assert zones[1023] == dict(quad=(0, 1019), tail=(1020, 1022))
    # one quad per thread of the full grid: still no thread with `i + 3 T < n4`
    assert zones[1024 * 1024 + 3] == dict(quad=(0, 4 * T - 1), tail=(4 * T, 4 * T + 2))
    # the smallest size with an unrolled round is 12 T + 4; at 16 T + 7 every thread has one, and thread 0 a quad more
    # (thread 0 alone: quads 0, T, 2 T and 3 T)
    assert "unrolled" not in pc.absmax_zones(12 * T + 3)
    assert pc.absmax_zones(12 * T + 4)["unrolled"] == (0, 12 * T + 3)
    big = 4 * (3 * T) + 4 * T + 7
    assert big in pc.ABSMAX_SIZES and zones[big] == dict(unrolled=(0, 16 * T - 1), quad=(16 * T, 16 * T + 3),
                                                          tail=(16 * T + 4, 16 * T + 6))
    # ... and 1000 more quads run in the one-quad zone, behind the unrolled round of the first 1000 threads
    last = pc.ABSMAX_SIZES[-1]
    assert zones[last] == dict(unrolled=(0, 16 * T - 1), quad=(16 * T, 16 * T + 3999),
                               tail=(16 * T + 4000, 16 * T + 4002))
    # a literal walk of the kernel's loop for one thread, at a size small enough to walk
    for n, t in ((last, 0), (last, 999), (last, 1000), (big, T - 1), (1024 * 1024 + 3, 5)):
        n4, nthr, i, seen = n // 4, pc.grid_reduce(n) * 256, t, {}
        while i + 3 * nthr < n4:
            for k in range(4):
                seen[i + k * nthr] = "unrolled"
            i += 4 * nthr
        while i < n4:
            seen[i] = "quad"
            i += nthr
        for q, zone in seen.items():
            first, lastq = pc.absmax_zones(n)[zone]
            assert first <= 4 * q <= lastq, (n, t, q, zone)


def test_faded_levels_have_exact_subnormal_differences():
    for shape in ((18, 21, 37), (16, 16, 16)):
        for count in (2, 6):
            lv = pc.faded_levels(shape, count, 3)
            assert len(lv) == count
            for a, b in zip(lv, lv[1:]):
                d = a - b
                exact = a.astype(np.float64) - b.astype(np.float64)
                np.testing.assert_array_equal(d.astype(np.float64), exact)
            d = lv[0] - lv[1]
            assert pc.is_subnormal(d).mean() > 0.5 and pc.is_subnormal(np.abs(d).max())
            print("faded levels %r: %.3f of the first differences are nonzero subnormals, max %.3g"
                  % (shape, pc.is_subnormal(d).mean(), np.abs(d).max()))
            if count >= 3:
                assert not pc.bits(lv[-2] - lv[-1]).any()
