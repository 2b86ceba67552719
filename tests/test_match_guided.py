"""GPU: transform-guided matching -- sift3d_hip_nn2_gated (hip.nn2_gated), Matcher.match_guided and the rematch=
flows, against tests/match_guided_restatement.py.  Indices are compared for equality and distances by bit pattern.

The kernel tests use dim 768.  The edge-of-the-gate test takes the largest FLOAT32 below 5 as its outside radius:
the contract's r2f = (float)(radius * radius) rounds the square of the largest double below 5 (25 - 9e-15) back to
25.0f, so that radius still admits a pair at distance exactly 5, which the test asserts as well."""
import numpy as np
import pytest

from tests import match_guided_restatement as gr
from tests import match_restatement as mr

pytestmark = pytest.mark.gpu

F = np.float32
DIM = 768
BOX, RADIUS = 64.0, 12.0


def _cuda(x, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda()


def _gated(a, b, pa, pb, radius, perm_a=None, perm_b=None, work=None):
    """hip.nn2_gated of numpy arrays / CUDA tensors: ((j, d1, d2) as numpy, visited, total)"""
    import torch
    from sift3d_amd import hip
    t = lambda x, d: x if isinstance(x, torch.Tensor) else _cuda(x, d)
    p = lambda x: None if x is None else t(x, np.int32)
    j, d1, d2, vis, tot = hip.nn2_gated(t(a, F), t(b, F), t(pa, F), t(pb, F), radius, p(perm_a), p(perm_b), work)
    return (j.cpu().numpy(), d1.cpu().numpy(), d2.cpu().numpy()), vis, tot


def _bits(x):
    return np.ascontiguousarray(x, F).view(np.int32)


def _assert_bitwise(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(_bits(got[1]), _bits(want[1]))
    np.testing.assert_array_equal(_bits(got[2]), _bits(want[2]))


def _unit(rng, n, dim=DIM):
    x = np.abs(rng.standard_normal((n, dim))).astype(F)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _box(rng, n, lo=0.0, size=BOX):
    return gr.pos4(lo + rng.uniform(0, size, (n, 3)))


def _kinds(ok):
    c = ok.sum(axis=1)
    return (c == 0).any(), (c == 1).any(), (c > 1).any()


# ---- block geometry: real-valued descriptors against the restatement -----------------------------------------
GEOMETRY = [(1, 1), (127, 129), (128, 128), (129, 257), (257, 130)]
_geometry_made = {}


def _geometry(na, nb):
    """(a, b, pa, pb, restated result): computed once per case and shared"""
    if (na, nb) not in _geometry_made:
        rng = np.random.default_rng(1000 * na + nb)
        a, b, pa, pb = _unit(rng, na), _unit(rng, nb), _box(rng, na), _box(rng, nb)
        _geometry_made[na, nb] = (a, b, pa, pb, gr.nn2_gated(a, b, pa, pb, RADIUS))
    return _geometry_made[na, nb]


@pytest.mark.parametrize("na,nb", GEOMETRY)
def test_gated_block_geometry_against_restatement(na, nb):
    from sift3d_amd import api
    a, b, pa, pb, want = _geometry(na, nb)
    ok = gr.gate(pa, pb, RADIUS)
    if nb >= 128:
        assert _kinds(ok) == (True, True, True)        # rows without a candidate, with one, with many
    got, vis, tot = _gated(a, b, pa, pb, RADIUS)
    _assert_bitwise(got, want)
    assert (vis, tot) == gr.visited(pa, pb, RADIUS) and tot == -(-na // 128) * -(-nb // 128)
    none = ~ok.any(axis=1)
    assert (got[0][none] == -1).all() and np.isposinf(got[1][none]).all() and np.isposinf(got[2][none]).all()
    one = ok.sum(axis=1) == 1
    assert np.isposinf(got[2][one]).all() and np.isfinite(got[1][one]).all()
    # the walked order changes the boxes, never the result
    qa, qb = api.spatial_order(pa[:, :3], RADIUS), api.spatial_order(pb[:, :3], RADIUS)
    got, vis, tot = _gated(a, b, pa, pb, RADIUS, qa, qb)
    _assert_bitwise(got, want)
    assert (vis, tot) == gr.visited(pa, pb, RADIUS, qa, qb)


# ---- more than 16 blocks of B: integer-valued data, exact in float64 -----------------------------------------
def _int_data(n, dim, seed, hi=16):
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(0, hi, (n, dim), generator=g, device="cuda").float()


def _exact_top2_gated(a, b, ok):
    """Gated top-2 of integer-valued CUDA float32 tensors in float64 on the GPU (exact): the smallest index among
    equal minima, the second-smallest distance counting ties; -1, inf, inf without candidates."""
    import torch
    nb = b.shape[0]
    a64, b64 = a.double(), b.double()
    D = (a64 * a64).sum(1)[:, None] + (b64 * b64).sum(1)[None, :] - 2.0 * (a64 @ b64.T)
    D = torch.where(_cuda(ok), D, torch.full_like(D, float("inf")))
    m1 = D.min(1).values
    ar = torch.arange(nb, device=a.device)
    j = torch.where(D == m1[:, None], ar[None, :], nb).min(1).values
    D.scatter_(1, j[:, None], float("inf"))
    m2 = D.min(1).values
    j = torch.where(torch.isinf(m1), torch.full_like(j, -1), j)
    return j.int().cpu().numpy(), m1.cpu().numpy(), m2.cpu().numpy()


def test_gated_integer_exact_many_runs():
    na, nb = 130, 2200
    assert mr.runs(na, nb)[0] == 16 and -(-nb // 128) > 16
    rng = np.random.default_rng(7)
    a, b = _int_data(na, DIM, 1), _int_data(nb, DIM, 2)
    pa, pb = _box(rng, na), _box(rng, nb)
    ok = gr.gate(pa, pb, RADIUS)
    want = _exact_top2_gated(a, b, ok)
    assert np.all(want[1] == want[1].astype(F))                       # (exact: no rounding in the reference)
    for perms in ((None, None), (rng.permutation(na), rng.permutation(nb))):
        got, vis, tot = _gated(a, b, pa, pb, RADIUS, *perms)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1].astype(F))
        np.testing.assert_array_equal(got[2], want[2].astype(F))
        assert (vis, tot) == gr.visited(pa, pb, RADIUS, *perms) and tot == 2 * 18


# ---- r2 = +inf: the ungated search; the walked order never shows ----------------------------------------------
def test_gated_infinite_radius_equals_nn2_and_order_independence():
    from sift3d_amd import hip
    rng = np.random.default_rng(11)
    na, nb = 300, 517
    a, b, pa, pb = _unit(rng, na), _unit(rng, nb), _box(rng, na), _box(rng, nb)
    b[40] = b[400] = a[7]                                                # a tie at the top, across blocks
    ta, tb = _cuda(a), _cuda(b)
    blind = tuple(x.cpu().numpy() for x in hip.nn2(ta, tb))
    got, vis, tot = _gated(ta, tb, pa, pb, np.inf)
    _assert_bitwise(got, blind)
    assert vis == tot == 3 * 5 and blind[0][7] == 40
    got, vis, tot = _gated(ta, tb, pa, pb, np.inf, rng.permutation(na), rng.permutation(nb))
    _assert_bitwise(got, blind)
    assert vis == tot
    first, _, _ = _gated(ta, tb, pa, pb, RADIUS)
    assert not np.array_equal(first[0], blind[0])
    for _ in range(3):
        got, _, _ = _gated(ta, tb, pa, pb, RADIUS, rng.permutation(na), rng.permutation(nb))
        _assert_bitwise(got, first)


# ---- the edge of the gate, NaN coordinates ---------------------------------------------------------------------
def test_gated_edge_of_the_gate_and_nan_coordinates():
    rng = np.random.default_rng(13)
    n = 130
    a, b = _unit(rng, n), _unit(rng, n)
    # integer positions 100 apart in x; partner j = i sits at exactly (3, 4, 0) from row i, every other row of b
    # far outside.  The second block (rows 128, 129) lies over the first in x and z and 5000 away in y.
    i = np.arange(n)
    pa = gr.pos4(np.stack([100.0 * (i % 128), rng.integers(0, 50, n) + 5000.0 * (i >= 128), rng.integers(0, 50, n)],
                          axis=1))
    pb = pa.copy()
    pb[:, :3] += F([3.0, 4.0, 0.0])
    assert (gr.gate_d2(pa, pb).diagonal() == 25.0).all()
    rows = np.arange(n)
    below32 = float(np.nextafter(F(5.0), F(0.0)))                        # the largest float32 below 5
    below64 = float(np.nextafter(5.0, 0.0))                              # the largest double below 5
    assert gr.r2f(5.0) == 25.0 and gr.r2f(below32) < 25.0 and gr.r2f(below64) == 25.0
    for radius, inside in ((5.0, True), (below64, True), (below32, False)):
        got, _, _ = _gated(a, b, pa, pb, radius)
        _assert_bitwise(got, gr.nn2_gated(a, b, pa, pb, radius))
        if inside:
            np.testing.assert_array_equal(got[0], rows)
            assert np.isfinite(got[1]).all() and np.isposinf(got[2]).all()
        else:
            assert (got[0] == -1).all() and np.isposinf(got[1]).all() and np.isposinf(got[2]).all()
    assert _gated(a, b, pa, pb, 5.0)[1:] == gr.visited(pa, pb, 5.0) == (2, 4)
    # a NaN coordinate in A removes the row, in B the column.  The point's other coordinates lie over the other
    # set's second block: the box is built without the point, so that block pair stays skipped (with the point's y
    # and z in the box it would be visited: 3 pairs)
    for side in ("a", "b"):
        qa, qb = pa.copy(), pb.copy()
        (qa if side == "a" else qb)[5] = F([np.nan, 5100.0, 20.0, 0.0])
        got, vis, tot = _gated(a, b, qa, qb, 5.0)
        np.testing.assert_array_equal(got[0], np.where(rows == 5, -1, rows))
        assert np.isposinf(got[1][5]) and np.isposinf(got[2][5])
        _assert_bitwise(got, gr.nn2_gated(a, b, qa, qb, 5.0))
        assert (vis, tot) == gr.visited(qa, qb, 5.0) == (2, 4)
        boxes = [(np.stack([np.nanmin(q[k:k + 128, :3], axis=0) for k in (0, 128)]),
                  np.stack([np.nanmax(q[k:k + 128, :3], axis=0) for k in (0, 128)])) for q in (qa, qb)]
        assert (gr.gap2(*boxes[0], *boxes[1]) <= gr.r2f(5.0)).sum() == 3


# ---- ties ------------------------------------------------------------------------------------------------------
def test_gated_ties_go_to_the_smallest_original_index():
    na, nb = 130, 2200
    rng = np.random.default_rng(17)
    a, b = _int_data(na, DIM, 3), _int_data(nb, DIM, 4)
    per = -(-(-(-nb // 128)) // mr.runs(na, nb)[0]) * 128
    p = 41
    # copies of one row of B in other lanes, waves, 128-blocks and runs; rows of A equal to it
    copies = sorted({p, p + 1, p + 31, p + 32, p + 64, p + 96, p + 128, p + 300, p + per, p + 2 * per, nb - 1})
    for q in copies[1:]:
        b[q] = b[p]
    rows = [0, 64, 129]
    for i in rows:
        a[i] = b[copies[-1]]
    pa, pb = _box(rng, na), _box(rng, nb)
    pb[copies, :3] = F([32.0, 32.0, 32.0])
    pa[rows, :3] = F([33.0, 31.0, 32.0])                                 # all copies inside these rows' gates
    ok = gr.gate(pa, pb, RADIUS)
    want = _exact_top2_gated(a, b, ok)
    reverse = np.arange(nb - 1, -1, -1)
    for perm_b in (None, reverse, rng.permutation(nb)):
        got, _, _ = _gated(a, b, pa, pb, RADIUS, None, perm_b)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1].astype(F))
        np.testing.assert_array_equal(got[2], want[2].astype(F))
        for i in rows:
            assert got[0][i] == p and got[1][i] == 0.0 and got[2][i] == 0.0
    # with the first copy outside the gate the next one wins
    pb[p, :3] = F([60.0, 60.0, 60.0])
    got, _, _ = _gated(a, b, pa, pb, RADIUS, None, reverse)
    assert [got[0][i] for i in rows] == [p + 1] * 3


# ---- skipping --------------------------------------------------------------------------------------------------
SKIP_RADIUS = 8.0
_skip_made = {}


def _skip_case():
    """Each set: 256 points in [0, 64)^3 and 256 in [1024, 1088)^3, interleaved in storage; restated once"""
    if not _skip_made:
        rng = np.random.default_rng(19)
        a, b = _unit(rng, 512), _unit(rng, 512)
        pa, pb = _box(rng, 512), _box(rng, 512)
        pa[1::2, :3] += F(1024.0)
        pb[1::2, :3] += F(1024.0)
        _skip_made["x"] = (a, b, pa, pb, gr.nn2_gated(a, b, pa, pb, SKIP_RADIUS))
    return _skip_made["x"]


def test_gated_skipping_two_clusters():
    from sift3d_amd import api
    a, b, pa, pb, want = _skip_case()
    qa, qb = api.spatial_order(pa[:, :3], SKIP_RADIUS), api.spatial_order(pb[:, :3], SKIP_RADIUS)
    assert (pa[qa[:256], 0] < 64).all() and (pb[qb[:256], 0] < 64).all()       # the clusters stay contiguous
    got, vis, tot = _gated(a, b, pa, pb, SKIP_RADIUS, qa, qb)
    _assert_bitwise(got, want)
    assert tot == 16 and vis == gr.visited(pa, pb, SKIP_RADIUS, qa, qb)[0] <= 8
    # identity order on the interleaved storage: every block spans both clusters, nothing can be skipped ...
    got, vis, tot = _gated(a, b, pa, pb, SKIP_RADIUS)
    _assert_bitwise(got, want)
    assert (vis, tot) == gr.visited(pa, pb, SKIP_RADIUS) == (16, 16)
    # ... and on a shuffled copy
    rng = np.random.default_rng(23)
    sa, sb = rng.permutation(512), rng.permutation(512)
    got, vis, tot = _gated(a[sa], b[sb], pa[sa], pb[sb], SKIP_RADIUS)
    assert (vis, tot) == gr.visited(pa[sa], pb[sb], SKIP_RADIUS)
    inv = np.empty(512, int)
    inv[sa] = np.arange(512)
    j = got[0][inv]
    np.testing.assert_array_equal(np.where(j >= 0, sb[np.maximum(j, 0)], -1), want[0])
    np.testing.assert_array_equal(_bits(got[1][inv]), _bits(want[1]))
    np.testing.assert_array_equal(_bits(got[2][inv]), _bits(want[2]))


def test_gated_block_of_a_with_every_block_of_b_skipped():
    """a third cluster of A, 128 points far from all of B: its workgroups visit nothing and still write"""
    from sift3d_amd import api
    a, b, pa, pb, want = _skip_case()
    rng = np.random.default_rng(29)
    a3 = np.concatenate([a, _unit(rng, 128)])
    pa3 = np.concatenate([pa, _box(rng, 128, lo=4096.0)])
    qa, qb = api.spatial_order(pa3[:, :3], SKIP_RADIUS), api.spatial_order(pb[:, :3], SKIP_RADIUS)
    np.testing.assert_array_equal(np.sort(qa[512:]), np.arange(512, 640))
    got, vis, tot = _gated(a3, b, pa3, pb, SKIP_RADIUS, qa, qb)
    _assert_bitwise(tuple(x[:512] for x in got), want)
    assert (got[0][512:] == -1).all() and np.isposinf(got[1][512:]).all() and np.isposinf(got[2][512:]).all()
    assert tot == 20 and vis == gr.visited(pa3, pb, SKIP_RADIUS, qa, qb)[0] <= 8
    loA, hiA = gr.block_boxes(pa3, qa)
    loB, hiB = gr.block_boxes(pb, qb)
    assert (gr.gap2(loA, hiA, loB, hiB)[4] > gr.r2f(SKIP_RADIUS)).all()


# ---- the calling contracts: scratch of exactly the advertised size, any stream ----------------------------------
def _contract_cases():
    from sift3d_amd import api
    a, b, pa, pb, want = _skip_case()
    yield (a, b, pa, pb, SKIP_RADIUS, api.spatial_order(pa[:, :3], SKIP_RADIUS),
           api.spatial_order(pb[:, :3], SKIP_RADIUS)), want
    a, b, pa, pb, want = _geometry(129, 257)
    yield (a, b, pa, pb, RADIUS, None, None), want


def test_gated_work_of_the_advertised_size_guarded_and_poisoned():
    import torch
    from sift3d_amd import hip
    for args, want in _contract_cases():
        a, b = args[0], args[1]
        need = hip.nn2_gated_work_floats(len(a), len(b))
        plain = _gated(*args)
        _assert_bitwise(plain[0], want)
        with pytest.raises(ValueError):
            _gated(*args, work=torch.empty(need - 1, device="cuda"))
        G = 16384
        for fill in (0xFF, 0x00):
            whole = torch.full((4 * (G + need + G),), fill, dtype=torch.uint8, device="cuda")
            work = whole[4 * G:4 * (G + need)].view(torch.float32)
            assert work.numel() == need and work.data_ptr() % 16 == 0
            for run in ("first", "second"):                 # the second finds what the first left behind
                got = _gated(*args, work=work)
                torch.cuda.synchronize()
                spilt = [int((band != fill).sum()) for band in (whole[:4 * G], whole[4 * (G + need):])]
                assert spilt == [0, 0], "%s call on work of 0x%02X: bytes written before, behind: %s" % (run, fill, spilt)
                _assert_bitwise(got[0], plain[0])
                assert got[1:] == plain[1:]


def test_gated_is_ordered_on_the_callers_stream():
    import torch
    from sift3d_amd import hip
    delay = torch.ones((256, 512, 512), device="cuda")
    for args, want in _contract_cases():
        hip.current_stream(refresh=True)
        real = [_cuda(x, F) for x in args[:4]] + [None if q is None else _cuda(q, np.int32) for q in args[5:]]
        plain = _gated(*real[:4], args[4], *real[4:])
        _assert_bitwise(plain[0], want)
        twins = [None if x is None else torch.zeros_like(x) for x in real]
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        try:
            with torch.cuda.stream(s):
                hip.current_stream(refresh=True)
                for _ in range(20):
                    delay.mul_(1.0001)
                for twin, x in zip(twins, real):
                    if x is not None:
                        twin.copy_(x)
                got = _gated(*twins[:4], args[4], *twins[4:])
            hip.current_stream(refresh=True)
            torch.cuda.current_stream().wait_stream(s)
            _assert_bitwise(got[0], plain[0])
            assert got[1:] == plain[1:]
        finally:
            hip.current_stream(refresh=True)


# ---- the matcher -------------------------------------------------------------------------------------------------
PUSH = np.array([[0.9, -0.3, 0.1, 12.0], [0.25, 1.1, -0.05, -7.5], [-0.1, 0.2, 0.95, 3.0]])
MATCH_RADIUS = 6.0


def _store(xyz, x):
    from sift3d_amd import api
    d = api.DescriptorStore()
    xyz_sd = np.concatenate([np.asarray(xyz, np.float64), np.ones((len(x), 1))], axis=1)
    assert d.set(xyz_sd, np.ascontiguousarray(x, F).reshape(-1, DIM)) == 0
    return d


def _pair(na, nb, seed, noise=0.05):
    """test_match.py's pair (unit rows, a third of b noisy copies of rows of a) with positions: a's anywhere in
    a 200^3 box, a copy's within about a voxel of where PUSH puts its source, the other rows of b anywhere.  Every
    fourth row of a is a look-alike of its neighbour, which the blind ratio test rejects."""
    rng = np.random.default_rng(seed)
    a = np.abs(rng.standard_normal((na, DIM))).astype(F)
    a[1::4] = a[0:-1:4][:len(a[1::4])] + F(0.01) * np.abs(rng.standard_normal((len(a[1::4]), DIM))).astype(F)
    b = np.abs(rng.standard_normal((nb, DIM))).astype(F)
    ncopy = min(na, nb // 3)
    src = rng.permutation(na)[:ncopy]
    b[:ncopy] = np.abs(a[src] + noise * rng.standard_normal((ncopy, DIM)).astype(F))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    xa = rng.uniform(0, 200, (na, 3))
    pred = xa @ PUSH[:, :3].T + PUSH[:, 3]
    xb = rng.uniform(pred.min(), pred.max(), (nb, 3))
    xb[:ncopy] = pred[src] + rng.normal(0, 0.7, (ncopy, 3))
    return a, b, xa, xb, pred


def _searches(a, b, pred, xb, radius):
    ta, tb, pa, pb = _cuda(a), _cuda(b), _cuda(gr.pos4(pred)), _cuda(gr.pos4(xb))
    return _gated(ta, tb, pa, pb, radius)[0], _gated(tb, ta, pb, pa, radius)[0]


@pytest.mark.parametrize("na,nb", [(700, 300), (3000, 6000)])
def test_matcher_guided_decision_superset_and_cap(na, nb):
    from sift3d_amd import api
    a, b, xa, xb, pred = _pair(na, nb, 5 + na)
    sa, sb = _store(xa, a), _store(xb, b)
    fwd, bwd = _searches(a, b, pred, xb, MATCH_RADIUS)
    want = gr.match_guided(fwd, bwd, 0.8)
    m = api.Matcher()
    got = m.match_guided(sa, sb, PUSH, MATCH_RADIUS, 0.8)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(m.match_guided(sa, sb, pred, MATCH_RADIUS), want)     # positions for the map
    assert m.seconds() > 0
    # the counters: both searches, in the matcher's own order of both sets
    qa, qb = api.spatial_order(pred, MATCH_RADIUS), api.spatial_order(xb, MATCH_RADIUS)
    pa4, pb4 = gr.pos4(pred), gr.pos4(xb)
    v1, t1 = gr.visited(pa4, pb4, MATCH_RADIUS, qa, qb)
    v2, t2 = gr.visited(pb4, pa4, MATCH_RADIUS, qb, qa)
    assert m.blocks() == (v1 + v2, t1 + t2) and v1 == v2
    if na >= 3000:
        assert v1 + v2 < t1 + t2                        # (24 x 47 blocks in a 260^3 box: about half are skipped)
    # superset: every blind match inside the gate is a guided match, and the gate finds more
    blind = m.match(sa, sb, 0.8)
    hit = np.nonzero(blind >= 0)[0]
    inside = gr.gate_d2(pa4[hit], pb4)[np.arange(len(hit)), blind[hit]] <= gr.r2f(MATCH_RADIUS)
    assert inside.sum() > min(na, nb) // 10
    np.testing.assert_array_equal(got[hit[inside]], blind[hit[inside]])
    assert (got >= 0).sum() > inside.sum()
    # after the blind match the guided one again, on the same matcher
    np.testing.assert_array_equal(m.match_guided(sa, sb, PUSH, MATCH_RADIUS, 0.8), want)
    # the cap removes exactly the restated pairs
    cap = float(np.sqrt(np.median(fwd[1][want >= 0])))
    capped = gr.match_guided(fwd, bwd, 0.8, cap)
    assert 0 < (capped >= 0).sum() < (want >= 0).sum()
    np.testing.assert_array_equal(m.match_guided(sa, sb, PUSH, MATCH_RADIUS, 0.8, max_distance=cap), capped)
    np.testing.assert_array_equal(np.nonzero(capped != want)[0], np.nonzero((want >= 0) & (fwd[1] > F(cap * cap)))[0])


def test_matcher_guided_reused_across_sizes_and_edges():
    from sift3d_amd import api
    m = api.Matcher()
    for na, nb in ((100, 2000), (2000, 100), (10, 10), (1500, 1000), (1, 1)):
        a, b, xa, xb, pred = _pair(na, nb, 11 + na + nb)
        sa, sb = _store(xa, a), _store(xb, b)
        for radius in (MATCH_RADIUS, np.inf):
            want = gr.match_guided(*_searches(a, b, pred, xb, radius), 0.8)
            np.testing.assert_array_equal(m.match_guided(sa, sb, PUSH, radius), want)
        np.testing.assert_array_equal(want, m.match(sa, sb, 0.8))            # +inf: the blind match
        assert m.blocks()[0] == m.blocks()[1] > 0
    assert len(m.match_guided(_store(xa[:0], a[:0]), sb, PUSH, 4.0)) == 0
    np.testing.assert_array_equal(m.match_guided(sa, _store(xb[:0], b[:0]), PUSH, 4.0), [-1])
    assert m.blocks() == (0, 0)
    with pytest.raises(ValueError):
        m.match_guided(sa, sb, np.zeros((2, 3)), 4.0)
    with pytest.raises(RuntimeError):
        m.match_guided(sa, sb, PUSH, 0.0)


# ---- the flows ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def volumes():
    """the 160^3 pair of test_config5_two_volumes_match_and_register and its affine"""
    import torch
    from sift3d_amd import hip
    n, sy, sz = 160, 5, 9
    vol = torch.empty((n + 24, n + 16, n), device="cuda")
    hip.synth_lattice(vol, 0, 21)
    v1 = vol[0:n, 0:n, :].contiguous()
    v2 = vol[sz:sz + n, sy:sy + n, :].transpose(1, 2).flip(1).contiguous()
    torch.cuda.synchronize()
    return v1, v2, np.array([[0, 1.0, 0, -sy], [-1.0, 0, 0, n - 1], [0, 0, 1.0, -sz]])


def _pairs(p, q):
    return {tuple(x) + tuple(y) for x, y in zip(np.asarray(p).tolist(), np.asarray(q).tolist())}


def test_register_rematch_recovers_the_affine_and_keeps_first_pass_matches(volumes):
    from sift3d_amd import api
    v1, v2, want = volumes
    kw = dict(err_thresh=3.0, num_iter=500, seed=5)
    reg = api.register(v1, v2, rematch=6.0, **kw)
    assert type(reg).__name__ == "GuidedRegistration" and reg._fields[-1] == "first"
    T = reg.A
    assert reg.inliers.mean() > 0.8
    assert np.abs(T[:, :3] - want[:, :3]).max() < 0.01 and np.abs(T[:, 3] - want[:, 3]).max() < 0.75
    # the first pass is the blind flow's
    p1, q1 = api._matched_points(v1, v2, 0.8, {}, "test")
    A1, inl1 = api.ransac_affine(p1, q1, 3.0, 500, 5)
    np.testing.assert_array_equal(reg.first.A, A1)
    np.testing.assert_array_equal(reg.first.inliers, inl1)
    assert reg.first.num_matches == len(p1)
    # superset on real keypoints: every first-pass match inside the gate under the first A is matched again
    p2, q2, first = api._matched_points_guided(v1, v2, 0.8, {}, "test", 6.0, 3.0, 500, 5)
    np.testing.assert_array_equal(first.A, A1)
    assert reg.num_matches == len(p2)
    pred = p1 @ A1[:, :3].T + A1[:, 3]
    inside = gr.gate_d2(gr.pos4(pred), gr.pos4(q1)).diagonal() <= gr.r2f(6.0)
    assert inside.sum() >= inl1.sum() > 20
    assert _pairs(p1[inside], q1[inside]) <= _pairs(p2, q2)
    assert len(p2) >= inside.sum()
    # the dict form: the same call, and one with a stricter ratio
    same = api.register(v1, v2, rematch=dict(radius=6.0), **kw)
    np.testing.assert_array_equal(same.A, reg.A)
    assert same.num_matches == reg.num_matches
    assert api.register(v1, v2, rematch=dict(radius=6.0, nn_thresh=0.7), **kw).num_matches <= reg.num_matches
    with pytest.raises(ValueError):
        api.register(v1, v2, rematch=dict(radius=6.0, ratio=0.8))
    with pytest.raises(ValueError):
        api.register(v1, v2, rematch=-1.0)


def test_flows_without_rematch_are_the_first_pass_path(volumes):
    import torch
    from sift3d_amd import api, hip
    v1, v2, _ = volumes
    p, q = api._matched_points(v1, v2, 0.8, {}, "test")
    want = api._register_matched(v1, v2, p, q, 3.0, 500, 1, False, None)
    for got in (api.register(v1, v2), api.register(v1, v2, rematch=None)):
        assert type(got) is api.Registration
        np.testing.assert_array_equal(got.A, want.A)
        np.testing.assert_array_equal(got.inliers, want.inliers)
        assert got.num_matches == want.num_matches == len(p)
        assert torch.equal(got.warped, want.warped)
    A, inl = api.ransac_affine(p, q, api.DEFORMABLE_ERR_THRESH, 500, 1)
    tps = api.tps_fit(q[inl], p[inl], api.DEFORMABLE_SMOOTHING, 2048)
    warped = torch.empty_like(v2)
    hip.warp_tps(v1, warped, tps, "linear")
    got = api.register_deformable(v1, v2)
    assert type(got) is api.DeformableRegistration
    np.testing.assert_array_equal(got.A, A)
    np.testing.assert_array_equal(got.inliers, inl)
    np.testing.assert_array_equal(got.tps.ctrl, tps.ctrl)
    np.testing.assert_array_equal(got.tps.weights, tps.weights)
    assert got.num_matches == len(p) and torch.equal(got.warped, warped)
    # and with rematch the deformable flow carries the first pass behind its fields
    g = api.register_deformable(v1, v2, rematch=6.0)
    assert type(g).__name__ == "GuidedDeformableRegistration" and g.first.num_matches == len(p)
    np.testing.assert_array_equal(g.first.A, A)
    assert g.num_matches >= int(inl.sum())


def test_refined_and_ffd_flows_carry_the_first_pass(volumes):
    from sift3d_amd import api
    v1, v2, want = volumes
    p, q = api._matched_points(v1, v2, 0.8, {}, "test")
    A1, inl1 = api.ransac_affine(p, q, 3.0, 500, 1)
    blind = api.register(v1, v2, refine=True)
    reg = api.register(v1, v2, refine=True, rematch=6.0)
    assert type(blind) is api.RefinedRegistration and type(reg) is api.GUIDED_REGISTRATIONS[api.RefinedRegistration]
    assert reg._fields == api.RefinedRegistration._fields + ("first",)
    np.testing.assert_array_equal(reg.first.A, A1)
    np.testing.assert_array_equal(reg.first.inliers, inl1)
    np.testing.assert_array_equal(blind.A_ransac, A1)
    assert reg.first.num_matches == blind.num_matches == len(p) and reg.num_matches >= int(inl1.sum())
    for T in (reg.A, reg.A_ransac):
        assert np.abs(T[:, :3] - want[:, :3]).max() < 0.01 and np.abs(T[:, 3] - want[:, 3]).max() < 0.75
    kw = dict(spacing=16, levels=1, landmarks=True)
    fb, fg = api.register_ffd(v1, v2, **kw), api.register_ffd(v1, v2, rematch=6.0, **kw)
    assert type(fb.registration) is api.RefinedRegistration
    assert type(fg.registration) is type(reg) and fg.registration.num_matches == reg.num_matches
    np.testing.assert_array_equal(fg.registration.first.A, A1)
    np.testing.assert_array_equal(fg.registration.A_ransac, reg.A_ransac)
    assert type(fg.refinement) is type(fb.refinement)
