"""GPU: a seeded fuzz of the registration stack's sampling kernels against their restatements, as
tests/test_gpu_fuzz.py is for detect and describe.  tests/sampling_cases.fuzz_cases draws the cases, stratified by the
launchers' choices (tests/test_sampling_matrix_host.py: every choice at least three times); the comparisons are
tests/test_sampling_matrix.py's.  The outputs of the warps and of the composition are carved out of a buffer of
sentinel NaNs, half of them 4 bytes past a 16-byte boundary, and the sentinels must survive."""
import pytest

from tests import sampling_cases as sc
from tests.test_sampling_matrix import hip, run_case        # noqa: F401 (hip: the fixture)
from tests.test_sampling_matrix_host import PER_SEED, SEEDS

pytestmark = pytest.mark.gpu
PARTS = 3                                                   # a seed's cases in thirds: each test takes seconds


@pytest.mark.parametrize("part", range(PARTS))
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("family", sc.FAMILIES)
def test_fuzz(hip, family, seed, part):                     # noqa: F811
    cases = sc.fuzz_cases(family, seed, PER_SEED)
    assert len(cases) % PARTS == 0
    for c in cases[part::PARTS]:
        run_case(hip, c, identity=True)
