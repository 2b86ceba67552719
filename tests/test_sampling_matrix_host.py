"""CPU (not gpu): the bookkeeping of tests/sampling_cases.py.  Every instantiation a launcher of the sampling core can
select has a hand-picked case (MATRIX) and at least three seeded ones, and the cases test something: the restatements
alone count some, and mostly not all, of their voxels in."""
import numpy as np
import pytest

from tests import sampling_cases as sc

# the kernels of ALL_KEYS.  Adding a metric means adding its line to sampling_cases.KERNELS and its name here.
KERNEL_NAMES = ("k_warp_affine", "k_warp_tps", "k_warp_field", "k_field_compose", "k_similarity", "k_affine_normal",
                "k_affine_ncc_normal", "k_parzen_hist", "k_affine_mi_normal", "k_ffd_force")
SEEDS = (1, 2)                                              # tests/test_sampling_fuzz.py's
PER_SEED = 24


def test_kernel_names_and_key_counts():
    assert tuple(k[1] for k in sc.KERNELS) == KERNEL_NAMES
    assert {k[0] for k in sc.ALL_KEYS} == set(sc.FAMILIES)
    per = {f: len({k for k in sc.INSTANTIATIONS if k[0] == f}) for f in sc.FAMILIES}
    assert per == {"warp_affine": 3, "warp_tps": 3, "warp_field": 3, "compose": 8, "similarity": 12, "msd": 4, "ncc": 4,
                   "parzen": 4, "mi": 4, "ffd": 4}
    assert sum(per.values()) == 49


def test_matrix_has_exactly_one_case_per_key():
    keys = [sc.selection_key(c.family, c) for c in sc.MATRIX]
    missing = sorted(sc.ALL_KEYS - set(keys), key=repr)
    assert not missing, "no MATRIX case selects %s" % (missing,)
    assert set(keys) == sc.ALL_KEYS
    assert len(keys) == len(set(keys)), "two MATRIX cases select one key"


def test_matrix_shapes_are_small():
    for c in sc.MATRIX:
        assert all(a <= b for s in (c.fshape, c.mshape) for a, b in zip(s, (6, 9, 133))), c
    assert {c.fshape[2] for c in sc.MATRIX} | {c.mshape[2] for c in sc.MATRIX} >= {1, 5, 64, 70}


@pytest.mark.parametrize("family", sc.FAMILIES)
def test_matrix_cases_count_some_voxels(family):
    for c in sc.MATRIX + sc.NONFINITE:
        if c.family != family:
            continue
        n, size = sc.counted(c)
        assert 0 < n, (sc.selection_key(family, c), n)
        if family in sc.MASKED_FAMILIES:
            assert n < size, (sc.selection_key(family, c), n, size)


@pytest.mark.parametrize("family", sc.FAMILIES)
def test_fuzz_hits_every_key_and_counts_part_of_most_grids(family):
    cases = [c for seed in SEEDS for c in sc.fuzz_cases(family, seed, PER_SEED)]
    assert cases == [c for seed in SEEDS for c in sc.fuzz_cases(family, seed, PER_SEED)]      # seeded: repeatable
    hits = {}
    for c in cases:
        assert all(a <= b for s in (c.fshape, c.mshape) for a, b in zip(s, (6, 9, 133))), c
        k = sc.selection_key(family, c)
        hits[k] = hits.get(k, 0) + 1
    want = {k for k in sc.ALL_KEYS if k[0] == family}
    assert set(hits) == want and min(hits.values()) >= 3, hits
    partial = sum(0 < n < size for n, size in map(sc.counted, cases))
    print("%s: %d of %d cases partially counted" % (family, partial, len(cases)))
    assert 4 * partial >= 3 * len(cases), (family, partial, len(cases))      # a condition on the inputs


def test_axis_of_one_has_an_exact_zero_coordinate():
    c = sc.case("similarity", (3, 5, 70), (4, 1, 1), field=True, seed=9)
    d = sc.build(c)
    assert not d.A[0].any() and not d.A[1].any() and d.A[2].any()
    x = np.arange(70, dtype=np.float32)
    assert np.array_equal(d.field[0], np.broadcast_to(-x, c.fshape))
    n, size = sc.counted(c, d)
    assert 0 < n
