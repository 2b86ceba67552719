"""Registration stage (BASELINE config 5): descriptor matching + RANSAC affine.

Parity with upstream cannot be pinned: the reference fork removed this code (CHANGES.md:99-103), so
there is no oracle and no fixture.  Matching and RANSAC are pinned bit for bit to numpy restatements
instead (tests/test_match.py, tests/test_match_host.py).  The tests here check what the stage must
achieve: the matrix-core nearest-neighbour kernel against a float64 numpy computation, the RANSAC fit
against a known affine under outliers, and the whole flow by recovering a known transform between two
volumes.
"""
import numpy as np
import pytest


def test_ransac_affine_recovers_known_transform():
    from sift3d_amd import api
    rng = np.random.default_rng(3)
    A = np.array([[0.9, -0.3, 0.1, 12.0], [0.25, 1.1, -0.05, -7.5], [-0.1, 0.2, 0.95, 3.0]])
    src = rng.uniform(0, 500, (400, 3))
    dst = src @ A[:, :3].T + A[:, 3] + rng.normal(0, 0.3, (400, 3))
    bad = rng.choice(400, 160, replace=False)                 # 40 % gross outliers
    dst[bad] = rng.uniform(0, 500, (160, 3))
    T, inl = api.ransac_affine(src, dst, err_thresh=2.0, num_iter=500, seed=7)
    assert np.abs(T[:, :3] - A[:, :3]).max() < 5e-3 and np.abs(T[:, 3] - A[:, 3]).max() < 0.5
    good = np.ones(400, bool)
    good[bad] = False
    assert inl[good].mean() > 0.97 and inl[bad].mean() < 0.05
    T2, inl2 = api.ransac_affine(src, dst, err_thresh=2.0, num_iter=500, seed=7)
    np.testing.assert_array_equal(T, T2)                       # deterministic for a seed
    with pytest.raises(RuntimeError):
        api.ransac_affine(src[:3], dst[:3])
    flat = src.copy()
    flat[:, 2] = 1.0                                           # coplanar points: no affine is determined
    with pytest.raises(RuntimeError):
        api.ransac_affine(flat, flat)


@pytest.mark.gpu
def test_nn2_against_numpy():
    import torch
    from sift3d_amd import hip
    rng = np.random.default_rng(11)
    for na, nb in ((300, 517), (129, 128), (5, 1), (1, 700)):
        a = np.abs(rng.standard_normal((na, 768))).astype(np.float32)
        b = np.abs(rng.standard_normal((nb, 768))).astype(np.float32)
        a /= np.linalg.norm(a, axis=1, keepdims=True)
        b /= np.linalg.norm(b, axis=1, keepdims=True)
        if nb > 40:
            b[37] = a[min(11, na - 1)]                         # an exact duplicate: distance 0
        j, d1, d2 = hip.nn2(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
        j, d1, d2 = j.cpu().numpy(), d1.cpu().numpy(), d2.cpu().numpy()
        D = ((a.astype(np.float64)[:, None, :] - b.astype(np.float64)[None, :, :]) ** 2).sum(-1)
        order = np.argsort(D, axis=1, kind="stable")
        want1 = D[np.arange(na), order[:, 0]]
        np.testing.assert_allclose(d1, want1, rtol=0, atol=1e-5)
        # (f32 accumulation of |a|^2 + |b|^2 - 2 a.b: ~1e-6 absolute)  the index may differ only between
        # numerically tied candidates
        assert np.all(D[np.arange(na), j] <= want1 + 2e-5)
        if nb > 1:
            np.testing.assert_allclose(d2, D[np.arange(na), order[:, 1]], rtol=0, atol=1e-5)
        else:
            assert np.all(np.isinf(d2))
        if nb > 40:
            assert j[min(11, na - 1)] == 37 and d1[min(11, na - 1)] < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("na,nb", [(3000, 6000), (100, 40000), (700, 300)])
def test_nn_match_store_api_against_numpy(na, nb):
    """sift3d_amd_nn_match through the descriptor stores with very different store sizes (the
    scratch buffer serves both directions): mutual nearest neighbours under the ratio test,
    against float64 numpy.  Some of b's rows are noisy copies of rows of a, so that real
    matches exist."""
    from sift3d_amd import api
    rng = np.random.default_rng(5 + na)
    a = np.abs(rng.standard_normal((na, 768))).astype(np.float32)
    b = np.abs(rng.standard_normal((nb, 768))).astype(np.float32)
    ncopy = min(na, nb // 3)                       # every row of a is copied at most once
    src = rng.permutation(na)[:ncopy]
    b[:ncopy] = a[src] + 0.05 * rng.standard_normal((ncopy, 768)).astype(np.float32)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    da, db = api.DescriptorStore(), api.DescriptorStore()
    assert da.set(np.zeros((na, 4)), a) == 0 and db.set(np.zeros((nb, 4)), b) == 0
    thr = 0.8
    got = api.nn_match(da, db, thr)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    D = (a64 * a64).sum(1)[:, None] + (b64 * b64).sum(1)[None, :] - 2.0 * (a64 @ b64.T)
    f = np.argsort(D, axis=1)[:, :2]
    g = np.argsort(D.T, axis=1)[:, :2]
    rows, cols = np.arange(na), np.arange(nb)
    fr = D[rows, f[:, 0]] / np.maximum(D[rows, f[:, 1]], 1e-30)
    gr = D.T[cols, g[:, 0]] / np.maximum(D.T[cols, g[:, 1]], 1e-30)
    want = np.full(na, -1)
    sure = np.zeros(na, bool)                      # decisions with a margin (f32 vs f64 distances)
    for i in range(na):
        j = f[i, 0]
        ok = fr[i] < thr * thr and g[j, 0] == i and gr[j] < thr * thr
        want[i] = j if ok else -1
        sure[i] = abs(fr[i] - thr * thr) > 1e-3 and abs(gr[j] - thr * thr) > 1e-3
    assert (want >= 0).sum() > 20
    np.testing.assert_array_equal(got[sure], want[sure])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [160, 512])
def test_config5_two_volumes_match_and_register(n):
    """BASELINE configs[4]: detect + describe two volumes, match, RANSAC affine.  The second
    volume is a shifted crop of the same field rotated by 90 degrees about z (an exact, proper
    affine that needs no resampling -- a mirror image would not do: the descriptor frame is a
    rotation, so mirrored content has a different descriptor); the recovered transform must be
    that affine."""
    import torch
    from sift3d_amd import api, hip
    vol = torch.empty((n + 24, n + 16, n), device="cuda")
    hip.synth_lattice(vol, 0, 21)
    sy, sz = 5, 9
    v1 = vol[0:n, 0:n, :].contiguous()
    # crop (x, y - sy, z - sz), then v2[z, y2, x2] = crop[z, y = x2, x = n - 1 - y2]
    v2 = vol[sz:sz + n, sy:sy + n, :].transpose(1, 2).flip(1).contiguous()
    torch.cuda.synchronize()
    stores = []
    for v in (v1, v2):
        det, kp, desc = api.Detector(), api.KeypointStore(), api.DescriptorStore()
        assert det.detect_keypoints_device(v.data_ptr(), n, n, n, kp) == 0
        assert det.extract_descriptors(kp, desc) == 0
        stores.append((kp, desc))
        del det
    (kp1, d1), (kp2, d2) = stores
    m = api.nn_match(d1, d2, 0.8)
    hit = np.nonzero(m >= 0)[0]
    assert len(hit) > 0.2 * min(len(d1), len(d2)) and len(hit) >= 20
    p1 = d1.to_mat_rm()[hit, :3].astype(np.float64)
    p2 = d2.to_mat_rm()[m[hit], :3].astype(np.float64)
    T, inl = api.ransac_affine(p1, p2, err_thresh=3.0, num_iter=500, seed=5)
    want = np.array([[0, 1.0, 0, -sy], [-1.0, 0, 0, n - 1], [0, 0, 1.0, -sz]])
    assert inl.mean() > 0.8
    assert np.abs(T[:, :3] - want[:, :3]).max() < 0.01 and np.abs(T[:, 3] - want[:, 3]).max() < 0.75


@pytest.mark.gpu
def test_matcher_device_resident_stores_equal_uploaded():
    """sift3d_amd_matcher on stores that keep their histograms in HBM (written by the describe kernel
    beside the host array) == the same match on stores uploaded per call; the device copy is dropped
    when a store is refilled from the host."""
    import torch
    from sift3d_amd import api, hip
    n = 128
    vol = torch.empty((n + 24, n + 16, n), device="cuda")
    hip.synth_lattice(vol, 0, 21)
    v1 = vol[0:n, 0:n, :].contiguous()
    v2 = vol[9:9 + n, 5:5 + n, :].transpose(1, 2).flip(1).contiguous()
    torch.cuda.synchronize()
    out = {}
    for keep in (False, True):
        stores = []
        for v in (v1, v2):
            det, kp, desc = api.Detector(), api.KeypointStore(), api.DescriptorStore()
            if keep:
                assert desc.keep_device(True) == 0
            assert det.detect_keypoints_device(v.data_ptr(), n, n, n, kp) == 0
            assert det.extract_descriptors(kp, desc) == 0
            stores.append(desc)
        m = api.Matcher()
        a = m.match(stores[0], stores[1], 0.8)
        b = m.match(stores[0], stores[1], 0.8)             # scratch reused
        np.testing.assert_array_equal(a, b)
        assert m.seconds() > 0
        out[keep] = (a, stores[0].to_mat_rm(), stores[1].to_mat_rm())
        if keep:
            # refilled from host arrays: the (now stale) device copy must not be used
            mat = stores[1].to_mat_rm()
            assert stores[1].set(np.zeros((len(mat), 4)), mat[::-1, 3:].copy()) == 0
            c = m.match(stores[0], stores[1], 0.8)
            ok = a >= 0
            np.testing.assert_array_equal(c[ok], len(mat) - 1 - a[ok])
    np.testing.assert_array_equal(out[False][0], out[True][0])
    np.testing.assert_array_equal(out[False][1], out[True][1])
    assert (out[True][0] >= 0).sum() > 20
