"""Host (no GPU): the level-only decisions of the orientation kernels, restated in numpy (tests/orient_cases.py).

  table    k_orient_table gives a level a window table unless its sphere needs more than 8192 quads or 4096 rows
           (or an extent of 500 voxels): the sd pairs tests/test_orient_candidates.py runs on the GPU lie on either
           side of a limit, by the restatement of the table's counting -- not by a number copied from somewhere;
  lut      orient_serial's table of weights: isotropic power-of-two units with rad^2 / u^2 < 191;
  packing  sift3d_hip_orient_window_fits: orient_serial packs window-relative x and y into 10 bits each, the host
           refuses a level whose clipped box can be wider than 1023 voxels.  Level descriptors only: no volume.
"""
import math

import numpy as np
import pytest

from sift3d_amd import hip
from tests import orient_cases as oc


@pytest.mark.parametrize("units, lo, hi, what", oc.LIMIT_PAIRS)
def test_pairs_straddle_their_limit(units, lo, hi, what):
    a, b = oc.table_count(lo, units), oc.table_count(hi, units)
    print(units, lo, a["rows"], a["quads"], a["table"], "|", hi, b["rows"], b["quads"], b["table"])
    if what == "quads":
        assert a["rows"] <= oc.TAB_ROWS and b["rows"] <= oc.TAB_ROWS
        assert a["quads"] <= oc.TAB_CAP < b["quads"]
        assert a["table"] and not b["table"]
    elif what == "rows":
        assert a["quads"] <= oc.TAB_CAP and a["rows"] <= oc.TAB_ROWS < b["rows"]
        assert a["table"] and not b["table"]
    else:
        assert oc.lut_used(lo, units) and not oc.lut_used(hi, units)
        r2 = lambda sd: (4.5 * sd / units[0]) ** 2
        assert r2(lo) < 191.0 < r2(hi)
        assert a["table"] and b["table"]              # both sides keep their window table: only the weights differ


def test_counting_restatement_on_a_small_sphere():
    """The restatement itself, against a plain triple loop in Python floats of float32 values (sd 0.5, units
    (1, 1.5, 0.7): rad 2.25)."""
    units, sd = (1.0, 1.5, 0.7), 0.5
    t = oc.table_count(sd, units)
    ux, uy, uz = (np.float32(v) for v in units)
    rad2 = (1.5 * sd * 3.0) ** 2
    my, mz, mx = t["len"].shape[1] // 2, t["len"].shape[0] // 2, int(2.25 / 1.0 + 2.0)
    vox = quads = 0
    for l in range(-mz, mz + 1):
        for j in range(-my, my + 1):
            ins = [i for i in range(-mx, mx + 1)
                   if not float(np.float32(np.float32(np.float32(i * ux) ** 2 + np.float32(j * uy) ** 2)
                                           + np.float32(l * uz) ** 2)) > rad2]
            assert t["len"][l + mz, j + my] == len(ins)
            if ins:
                assert ins == list(range(ins[0], ins[0] + len(ins))) and t["first"][l + mz, j + my] == ins[0]
            vox += len(ins)
            quads += (len(ins) + 3) // 4
    assert (vox, quads) == (t["voxels"], t["quads"]) and vox > 20 and t["table"]
    assert t["rows"] == (2 * my + 1) * (2 * mz + 1)


def test_no_lut_off_powers_of_two():
    units, sd = oc.NO_LUT
    assert not oc.lut_used(sd, units) and (4.5 * sd / units[0]) ** 2 < 191.0
    assert not oc.lut_used(1.6, (1.0, 1.0, 2.0))      # anisotropic
    assert oc.lut_used(1.6, (1.0, 1.0, 1.0))
    assert oc.table_count(sd, units)["table"]


def test_extent_limit():
    """An extent of 500 voxels or more on any axis: no table, whatever the counts."""
    assert not oc.table_count(1.6, (1.0, 1.0, 0.01))["table"]
    assert oc.table_count(1.6, (1.0, 1.0, 0.5))["table"]


# ---- the 10-bit window packing -------------------------------------------------------------------------------------

def test_window_just_below_and_just_above_1023():
    # 2 ceil(4.5 sd / u) + 1 = 1023 <=> ceil = 511: sd = 511 / 4.5 = 113.55...; the level is wider than the window
    below, above = 113.5, 113.6
    assert 2 * math.ceil(4.5 * below) + 1 == 1023 and 2 * math.ceil(4.5 * above) + 1 == 1025
    assert hip.orient_window_fits(4096, 64, 1.0, 1.0, below) == 1
    assert hip.orient_window_fits(4096, 64, 1.0, 1.0, above) == 0
    assert hip.orient_window_fits(64, 4096, 1.0, 1.0, above) == 0     # y alike
    assert hip.orient_window_fits(64, 4096, 1.0, 1.0, below) == 1
    # the level bounds the box: n - 2 = 1023 fits whatever the scale, 1024 does not
    assert hip.orient_window_fits(1025, 1025, 1.0, 1.0, 1e6) == 1
    assert hip.orient_window_fits(1026, 64, 1.0, 1.0, 1e6) == 0
    assert hip.orient_window_fits(64, 1026, 1.0, 1.0, 1e6) == 0
    # coarser units, narrower windows in voxels; z does not enter
    assert hip.orient_window_fits(4096, 4096, 2.0, 2.0, 2 * below) == 1
    assert hip.orient_window_fits(4096, 4096, 2.0, 1.0, 2 * below) == 0
    assert hip.orient_window_fits(4096, 4096, 0.5, 0.5, above / 2) == 0
    # the levels of every volume the suite and the benchmark use are far inside
    assert hip.orient_window_fits(512, 512, 1.0, 1.0, 1.6 * 2 ** (4 / 3.0)) == 1


def test_window_without_a_scale_is_the_whole_row():
    for sd in (0.0, -1.0, float("nan")):
        assert hip.orient_window_fits(1025, 1025, 1.0, 1.0, sd) == 1
        assert hip.orient_window_fits(1026, 1025, 1.0, 1.0, sd) == 0
    assert hip.orient_window_fits(2000, 8, 0.0, 1.0, 1.6) == 0
    assert hip.orient_window_fits(2, 1, 1.0, 1.0, 1.6) == 1


def test_window_restatement_agrees_over_a_sweep():
    rng = np.random.Generator(np.random.PCG64(41))
    seen = [0, 0]
    for _ in range(4000):
        nx, ny = (int(v) for v in rng.integers(1, 3000, 2))
        ux, uy = (float(2.0 ** rng.integers(-2, 3)) if rng.random() < 0.5 else float(rng.uniform(0.3, 4.0))
                  for _ in range(2))
        sd = float(rng.uniform(0.2, 400.0))
        want = oc.window_fits(nx, ny, ux, uy, sd)
        seen[want] += 1
        assert hip.orient_window_fits(nx, ny, ux, uy, sd) == want, (nx, ny, ux, uy, sd)
    assert min(seen) > 200
