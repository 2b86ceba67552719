"""GPU: sift3d_hip_nn2 (hip.nn2), api.Matcher and api.nn_match pinned exactly.

  integer-valued inputs   values 0..15, dim <= 1024: every product and partial sum is exact in float32, so
                          float64 distances (any summation order) are the kernel's bit for bit, at any size;
  real-valued inputs      bit for bit against the numpy restatement (tests/match_restatement.py), with a
                          float64 error bound beside it;
  invariance              bitwise, at sizes too big to restate: other run counts, permutations, duplicates.

(nA, nB, dim, runs of B per row block of A) covered: see CASES_INT and the real-valued cases below;
mr.runs(nA, nB) gives the run count and the number of empty runs.
"""

import numpy as np
import pytest

from tests import match_restatement as mr
from tests.util import load

pytestmark = pytest.mark.gpu


def _nn2(a, b):
    """hip.nn2 of two float32 arrays / CUDA tensors, results as numpy."""
    import torch
    from sift3d_amd import hip
    ta = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    tb = b if isinstance(b, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(b, np.float32)).cuda()
    j, d1, d2 = hip.nn2(ta, tb)
    return j.cpu().numpy(), d1.cpu().numpy(), d2.cpu().numpy()


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def _assert_bitwise(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(_bits(got[1]), _bits(want[1]))
    np.testing.assert_array_equal(_bits(got[2]), _bits(want[2]))


def _exact_top2(a, b, chunk=2048):
    """Top-2 of integer-valued CUDA float32 tensors in float64 on the GPU: exact (integers below 2^53), the
    smallest index among equal minima, the second-smallest distance counting ties."""
    import torch
    na, nb = a.shape[0], b.shape[0]
    if nb == 0:
        return np.full(na, -1, np.int32), np.full(na, np.inf), np.full(na, np.inf)
    b64 = b.double()
    nrm_b = (b64 * b64).sum(1)
    ar = torch.arange(nb, device=a.device)
    js, d1s, d2s = [], [], []
    for i0 in range(0, na, chunk):
        ac = a[i0:i0 + chunk].double()
        D = (ac * ac).sum(1)[:, None] + nrm_b[None, :] - 2.0 * (ac @ b64.T)
        m1 = D.min(1).values
        j = torch.where(D == m1[:, None], ar[None, :], nb).min(1).values
        if nb > 1:
            D.scatter_(1, j[:, None], float("inf"))
            m2 = D.min(1).values
        else:
            m2 = torch.full_like(m1, float("inf"))
        js.append(j.int().cpu())
        d1s.append(m1.cpu())
        d2s.append(m2.cpu())
    cat = torch.cat
    return cat(js).numpy(), cat(d1s).numpy(), cat(d2s).numpy()


def _int_data(n, dim, seed, hi=16):
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(0, hi, (n, dim), generator=g, device="cuda").float()


def _plant_duplicates(a, b, seed):
    """Copies of one B row at positions in other lanes, waves, 128-blocks and runs of B, and rows of A equal
    to the LAST copy: the kernel must return the first one."""
    na, nb = a.shape[0], b.shape[0]
    if nb < 2:
        return []
    ns, _ = mr.runs(na, nb)
    per = -(-(-(-nb // 128)) // ns) * 128
    p = min(nb - 1, 37 + seed % 50)
    pos = sorted({q for q in (p, p + 1, p + 31, p + 32, p + 64, p + 96, p + 128, p + 300, p + per, p + 2 * per,
                              nb - 1) if q < nb})
    for q in pos[1:]:
        b[q] = b[p]
    rows = sorted({0, na // 2, na - 1, min(na - 1, 129)})
    for i in rows:
        a[i] = b[pos[-1]]
    return [(i, pos[0]) for i in rows]


CASES_INT = [
    # tiny and partial blocks
    (1, 1, 32), (5, 1, 64), (31, 127, 96), (32, 128, 768), (33, 129, 1024), (31, 129, 32), (130, 1, 1024),
    # ns = 16 with 7 empty runs
    (128, 2049, 64), (129, 2176, 96),
    # ns = 16, partial last run
    (16385, 4000, 32),
    # the bench's size: ns = 7
    (42501, 40000, 768), (40000, 42501, 768),
    # ns = 1 reached from the A side
    (262145, 200, 32),
]


@pytest.mark.parametrize("na,nb,dim", CASES_INT)
def test_nn2_integer_exact(na, nb, dim):
    a, b = _int_data(na, dim, 1 + na + dim), _int_data(nb, dim, 2 + nb + dim)
    planted = _plant_duplicates(a, b, na + nb)
    want = _exact_top2(a, b)
    got = _nn2(a, b)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1].astype(np.float32))
    np.testing.assert_array_equal(got[2], want[2].astype(np.float32))
    assert np.all(want[1] == want[1].astype(np.float32))             # (exact: no rounding in the reference)
    for i, p in planted:
        assert got[0][i] == p and got[1][i] == 0.0 and got[2][i] == 0.0
    if nb > 1:
        assert (got[1] == got[2]).any()                              # ties at the top occur


def test_nn2_integer_exact_small_range_dense_ties():
    # values 0..1: nearly every row has several nearest candidates, across lanes, waves, blocks and runs
    a, b = _int_data(700, 64, 5, hi=2), _int_data(3000, 64, 6, hi=2)
    want = _exact_top2(a, b)
    got = _nn2(a, b)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1].astype(np.float32))
    np.testing.assert_array_equal(got[2], want[2].astype(np.float32))
    assert (got[1] == got[2]).mean() > 0.1


# ---- real-valued inputs: bit for bit against the restatement ----------------------------------------------
def _real_cases():
    rng = np.random.default_rng(17)
    g = load("g5_512")["desc_hist_s"].astype(np.float32)            # 439 x 768, non-negative, unit rows
    yield "golden", g[:130], g[100:439]                              # 30 shared rows: distance 0, clamped
    yield "normal", rng.standard_normal((300, 64)).astype(np.float32), \
        rng.standard_normal((517, 64)).astype(np.float32)
    mag = lambda shape: (np.exp(rng.uniform(np.log(1e-3), np.log(1e3), shape))
                         * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    yield "loguniform", mag((129, 64)), mag((2176, 64))
    yield "normal96", rng.standard_normal((33, 96)).astype(np.float32), rng.standard_normal((260, 96)).astype(np.float32)


def _f64_bound_check(a, b, got):
    """Guard rail independent of the bitwise premise: |d - D64| within the f32 error of the chain."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    dim = a.shape[1]
    D = (a64 * a64).sum(1)[:, None] + (b64 * b64).sum(1)[None, :] - 2.0 * (a64 @ b64.T)
    S = np.abs(a64) @ np.abs(b64).T
    u = 2.0 ** -24
    tol = u * (dim + 4) * (2.0 * S + (a64 * a64).sum(1)[:, None] + (b64 * b64).sum(1)[None, :]) + 1e-30
    rows = np.arange(len(a))
    Ds = np.sort(D, 1)
    tmax = tol.max(1)
    assert np.all(np.abs(got[1] - np.maximum(Ds[:, 0], 0)) <= 2 * tmax)
    assert np.all(np.abs(got[2] - np.maximum(Ds[:, 1], 0)) <= 2 * tmax)
    assert np.all(D[rows, got[0]] <= Ds[:, 0] + 4 * tmax)


@pytest.mark.parametrize("case", ["golden", "normal", "loguniform", "normal96"])
def test_nn2_real_bitexact_against_restatement(case):
    name, a, b = next(c for c in _real_cases() if c[0] == case)
    got = _nn2(a, b)
    _f64_bound_check(a, b, got)
    _assert_bitwise(got, mr.nn2(a, b))
    if name == "golden":
        assert np.all(got[1][100:130] < 1e-5) and np.all(got[0][100:130] == np.arange(30))


# ---- invariance, bitwise, at sizes too big to restate ------------------------------------------------------
@pytest.fixture(scope="module")
def big_real():
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(99)
    a = torch.randn((20000, 768), generator=g, device="cuda").abs_()
    b = torch.randn((30000, 768), generator=g, device="cuda").abs_()
    a /= a.norm(dim=1, keepdim=True)
    b /= b.norm(dim=1, keepdim=True)
    a[130] = a[0]
    a[7000] = a[0]
    a[19999] = a[0]                                                   # duplicates in other row blocks
    return a.contiguous(), b.contiguous(), _nn2(a, b)


def test_nn2_rows_independent_of_runs(big_real):
    import torch
    a, b, full = big_real
    assert mr.runs(20000, 30000)[0] == 14 and mr.runs(1, 30000)[0] == 16 and mr.runs(3000, 30000)[0] == 16
    for i in (0, 1, 127, 128, 12345, 19999):
        one = _nn2(a[i:i + 1].contiguous(), b)
        _assert_bitwise(one, tuple(x[i:i + 1] for x in full))
    sub = torch.randperm(20000, generator=torch.Generator().manual_seed(4))[:3000].sort().values
    part = _nn2(a[sub.cuda()].contiguous(), b)
    _assert_bitwise(part, tuple(x[sub.numpy()] for x in full))
    for i in (130, 7000, 19999):
        assert full[0][i] == full[0][0] and _bits(full[1][i]) == _bits(full[1][0]) \
            and _bits(full[2][i]) == _bits(full[2][0])


def test_nn2_permuted_b(big_real):
    import torch
    a, b, full = big_real
    perm = torch.randperm(30000, generator=torch.Generator().manual_seed(5))
    got = _nn2(a, b[perm.cuda()].contiguous())
    np.testing.assert_array_equal(_bits(got[1]), _bits(full[1]))
    np.testing.assert_array_equal(_bits(got[2]), _bits(full[2]))
    untied = full[1] != full[2]
    assert untied.mean() > 0.99
    np.testing.assert_array_equal(perm.numpy()[got[0]][untied], full[0][untied])


# ---- edges -------------------------------------------------------------------------------------------------
def _nn2_raw(a, na, b, nb):
    """sift3d_hip_nn2 on the first na / nb rows of CUDA tensors a / b (an empty tensor has a NULL data_ptr(),
    which the launcher refuses); outputs of 8 + na elements prefilled with canaries."""
    import torch
    from sift3d_amd import hip
    L = hip.lib()
    j = torch.full((na + 8,), -77, dtype=torch.int32, device="cuda")
    d1 = torch.full((na + 8,), -5.0, device="cuda")
    d2 = torch.full((na + 8,), -5.0, device="cuda")
    work = torch.zeros(L.sift3d_hip_nn2_work_floats(na, nb) + 8, device="cuda")
    rc = L.sift3d_hip_nn2(a.data_ptr(), na, b.data_ptr(), nb, a.shape[1], j.data_ptr(), d1.data_ptr(),
                          d2.data_ptr(), work.data_ptr(), hip.current_stream())
    torch.cuda.synchronize()
    return rc, j.cpu().numpy(), d1.cpu().numpy(), d2.cpu().numpy()


def test_nn2_edges():
    import torch
    rng = np.random.default_rng(8)
    a = rng.standard_normal((70, 64)).astype(np.float32)
    b = rng.standard_normal((9, 64)).astype(np.float32)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    rc, j, d1, d2 = _nn2_raw(ta, 70, tb, 0)                          # nB = 0
    assert rc == 0
    assert (j[:70] == -1).all() and np.isposinf(d1[:70]).all() and np.isposinf(d2[:70]).all()
    assert (j[70:] == -77).all() and (d1[70:] == -5).all() and (d2[70:] == -5).all()
    rc, j, d1, d2 = _nn2_raw(ta, 0, tb, 9)                           # nA = 0: nothing written
    assert rc == 0 and (j == -77).all() and (d1 == -5).all() and (d2 == -5).all()
    got = _nn2(a, b[:1])                                             # nB = 1
    assert (got[0] == 0).all() and np.isposinf(got[2]).all()
    _assert_bitwise(got, mr.nn2(a, b[:1]))
    # identical rows: clamped at 0 and never negative; a duplicated B row ties d1 == d2
    bb = np.concatenate([b, a[3:4], a[5:6], a[3:4]])
    got = _nn2(a, bb)
    _assert_bitwise(got, mr.nn2(a, bb))
    assert got[0][3] == 9 and got[0][5] == 10 and got[1][3] == got[2][3] >= 0 and got[1][5] >= 0
    assert (got[1] >= 0).all() and not np.signbit(got[1]).any()


# ---- buffers: exactly the advertised length, canaries behind -----------------------------------------------
@pytest.mark.parametrize("na,nb,dim", [(5, 1, 32), (129, 2176, 64), (300, 9000, 96), (16385, 300, 32),
                                       (40, 0, 32)])
def test_nn2_writes_only_its_buffers(na, nb, dim):
    import torch
    from sift3d_amd import hip
    L = hip.lib()
    a, b = _int_data(na, dim, 3), _int_data(max(nb, 1), dim, 4)       # (an empty tensor's data_ptr() is NULL)
    wf = L.sift3d_hip_nn2_work_floats(na, nb)
    assert wf == na + nb + 8 + 3 * na * mr.runs(na, nb)[0]
    T = 257
    canary = -123456.75
    j = torch.full((na + T,), -77, dtype=torch.int32, device="cuda")
    d1 = torch.full((na + T,), canary, device="cuda")
    d2 = torch.full((na + T,), canary, device="cuda")
    work = torch.full((wf + T,), canary, device="cuda")
    rc = L.sift3d_hip_nn2(a.data_ptr(), na, b.data_ptr(), nb, dim, j.data_ptr(), d1.data_ptr(), d2.data_ptr(),
                          work.data_ptr(), hip.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert (j[na:] == -77).all() and (d1[na:] == canary).all() and (d2[na:] == canary).all()
    assert (work[wf:] == canary).all()
    want = _exact_top2(a, b[:nb])
    np.testing.assert_array_equal(j[:na].cpu().numpy(), want[0])
    np.testing.assert_array_equal(d1[:na].cpu().numpy(), want[1].astype(np.float32))
    np.testing.assert_array_equal(d2[:na].cpu().numpy(), want[2].astype(np.float32))


# ---- streams -----------------------------------------------------------------------------------------------
def test_nn2_non_default_stream():
    import torch
    from sift3d_amd import hip
    a, b = _int_data(3000, 768, 7), _int_data(5000, 768, 8)
    want = _nn2(a, b)
    # The inputs are produced on stream s behind several milliseconds of other work: a search that ran on any
    # other stream would read the zeros.
    a2, b2 = torch.zeros_like(a), torch.zeros_like(b)
    big = torch.ones((256, 512, 512), device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    try:
        with torch.cuda.stream(s):
            hip.current_stream(refresh=True)
            for _ in range(20):
                big.mul_(1.0001)
            a2.copy_(a)
            b2.copy_(b)
            j, d1, d2 = hip.nn2(a2, b2)
            got = (j.clone(), d1.clone(), d2.clone())
        hip.current_stream(refresh=True)
        torch.cuda.current_stream().wait_stream(s)
        _assert_bitwise(tuple(x.cpu().numpy() for x in got), want)
    finally:
        hip.current_stream(refresh=True)


# ---- the matcher ---------------------------------------------------------------------------------------------
def _store(x):
    from sift3d_amd import api
    d = api.DescriptorStore()
    assert d.set(np.zeros((len(x), 4)), np.ascontiguousarray(x, np.float32).reshape(-1, 768)) == 0
    return d


def _pair(na, nb, seed, noise=0.05):
    """Unit, non-negative rows; some of b are noisy copies of rows of a, so that real matches exist."""
    rng = np.random.default_rng(seed)
    a = np.abs(rng.standard_normal((na, 768))).astype(np.float32)
    b = np.abs(rng.standard_normal((nb, 768))).astype(np.float32)
    ncopy = min(na, nb // 3)
    src = rng.permutation(na)[:ncopy]
    b[:ncopy] = a[src] + noise * rng.standard_normal((ncopy, 768)).astype(np.float32)
    b = np.abs(b)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    return a, b


def test_matcher_against_restated_nn2():
    from sift3d_amd import api
    g = load("g5_512")["desc_hist_s"].astype(np.float32)
    rng = np.random.default_rng(21)
    a = g[:150].copy()
    b = g[90:330].copy()
    b[::4] += np.float32(0.02) * np.abs(rng.standard_normal((len(b[::4]), 768))).astype(np.float32)
    b[200] = b[10]                      # b[10] == a[100]: its copy ties a[100]'s nearest distance
    fwd, bwd = mr.nn2(a, b), mr.nn2(b, a)
    m = api.Matcher()
    for thr in (0.8, 0.95, 1.0, 1.5):
        want = mr.match(fwd, bwd, thr)
        np.testing.assert_array_equal(m.match(_store(a), _store(b), thr), want)
        np.testing.assert_array_equal(api.nn_match(_store(a), _store(b), thr), want)
    assert (mr.match(fwd, bwd, 0.8) >= 0).sum() > 20
    assert fwd[0][100] == 10 and fwd[1][100] == fwd[2][100] and mr.match(fwd, bwd, 0.8)[100] == -1


@pytest.mark.parametrize("na,nb", [(3000, 6000), (100, 40000), (42501, 40000)])
def test_matcher_against_gpu_nn2(na, nb):
    from sift3d_amd import api
    a, b = _pair(na, nb, 5 + na)
    fwd, bwd = _nn2(a, b), _nn2(b, a)
    got = api.Matcher().match(_store(a), _store(b), 0.8)
    want = mr.match(fwd, bwd, 0.8)
    np.testing.assert_array_equal(got, want)
    assert (want >= 0).sum() > min(na, nb) // 10
    # (a matcher from scratch and the other direction)
    np.testing.assert_array_equal(api.nn_match(_store(b), _store(a), 0.8), mr.match(bwd, fwd, 0.8))


def test_matcher_edges():
    from sift3d_amd import api
    a, b = _pair(20, 30, 3)
    m = api.Matcher()
    assert len(m.match(_store(a[:0]), _store(b), 0.8)) == 0
    np.testing.assert_array_equal(m.match(_store(a), _store(b[:0]), 0.8), np.full(20, -1))
    np.testing.assert_array_equal(m.match(_store(a[:1]), _store(b[:1]), 0.8), [0])   # d2 = inf: accepted
    np.testing.assert_array_equal(m.match(_store(a[:1]), _store(b[:1]), 3.0), [0])
    # exact ties: a row of b duplicated is tied at the top for the rows of a nearest to it: rejected
    bb = np.concatenate([b, b[:5]])
    aa = b[:5].copy()
    got = m.match(_store(aa), _store(bb), 0.8)
    np.testing.assert_array_equal(got, np.full(5, -1))
    # (above 1 the test d1 < r2 d2 of a tie passes unless the distance is exactly 0: the restatement decides)
    np.testing.assert_array_equal(m.match(_store(aa), _store(bb), 2.0), mr.match(_nn2(aa, bb), _nn2(bb, aa), 2.0))
    for thr in (1.0, 1.25, 4.0):
        want = mr.match(_nn2(a, b), _nn2(b, a), thr)
        np.testing.assert_array_equal(m.match(_store(a), _store(b), thr), want)


def test_matcher_reused_across_sizes():
    from sift3d_amd import api
    m = api.Matcher()
    for na, nb in ((100, 5000), (5000, 100), (3000, 3000), (10, 10), (6000, 4000), (1, 1)):
        a, b = _pair(na, nb, 11 + na + nb)
        sa, sb = _store(a), _store(b)
        got = m.match(sa, sb, 0.8)
        np.testing.assert_array_equal(got, api.nn_match(sa, sb, 0.8))
        np.testing.assert_array_equal(got, mr.match(_nn2(a, b), _nn2(b, a), 0.8))
