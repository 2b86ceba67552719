"""GPU: block matching (include/sift3d_amd.h, "Block matching") on the device against the numpy restatement
(tests/block_match_restatement.py): the three records of sift3d_hip_block_match BIT FOR BIT, the calling contracts
(work buffer, stream, refusals), the driver iteration by iteration from the device's own starting map, and the public
entries against the hip layer.

The driver's comparison.  Given the same A the device's records are the restatement's bits, so selection is the same
set; what is left between the C fit (Horn's quaternion, normal equations) and numpy's (SVD, lstsq) is rounding, held
to 1e-9 of corner distance per iteration.  Each trail entry is checked from the DEVICE's A_in, so that a last-bit
difference cannot compound.  The trail carries the counts of an iteration, not the selected set itself: equal records
(above), equal counts and a produced A within 1e-9 stand for it.  The pairs and the figures the restatement reaches on
them are in tests/test_block_match_host.py; the device's run on the 48^3 pair: corner error 5.4470 at the start,
0.1267 after 9 iterations (the restatement's figures)."""
import numpy as np
import pytest

from tests import block_match_restatement as bm
from tests import test_block_match_host as th
from tests.test_warp import ref_warp

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(ts):
    return tuple(t.cpu().numpy() for t in ts)


def same_bits(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g.view(np.uint8), w.view(np.uint8))
               for g, w in zip(got, want))


def match(hip, F, W, R, VF=None, VW=None, **kw):
    return host(hip.block_match(dev(F), dev(W), R, dev(VF), dev(VW), **kw))


def noise_pair(shape, seed):
    """smooth noise, and the same moved by a fraction of a voxel with a gain ramp and fresh noise on top"""
    F = th.smooth_noise(shape, seed, 1.5)
    A = np.array([[1, 0.02, 0, 0.6], [-0.02, 1, 0.01, -0.4], [0, -0.01, 1, 0.3]])
    W = ref_warp(F, A, shape, "linear", 0.0)[0].astype(F32)
    W = (W * np.linspace(0.7, 1.3, shape[2], dtype=F32)[None, None, :] + F32(0.1) * th.smooth_noise(shape, seed + 1, 1.0))
    return F, W.astype(F32)


def masks(shape, seed):
    rng = np.random.default_rng(seed)
    VF = np.ones(shape, F32)
    VW = np.ones(shape, F32)
    for V in (VF, VW):                                       # a few holes, and a value at the threshold on either side
        idx = rng.integers(0, np.prod(shape), 4)
        V.reshape(-1)[idx] = rng.choice(np.array([0.0, 0.25, 0.49999997], F32), 4)
        V.reshape(-1)[rng.integers(0, np.prod(shape), 3)] = 0.5
    return VF, VW


CASES = [((20, 12, 16), R) for R in (1, 3, 6)] + [((9, 14, 19), R) for R in (1, 3, 6)] + [((32, 36, 40), 3)]


@pytest.mark.parametrize("shape,R", CASES, ids=["%dx%dx%d-R%d" % (s[2], s[1], s[0], R) for s, R in CASES])
@pytest.mark.parametrize("which", ["none", "fixed", "warped", "both"])
def test_records_bit_for_bit_on_smooth_noise(hip, shape, R, which):
    F, W = noise_pair(shape, 11)
    VF, VW = masks(shape, 5)
    VF = VF if which in ("fixed", "both") else None
    VW = VW if which in ("warped", "both") else None
    want = bm.block_match(F, W, R, VF, VW)
    got = match(hip, F, W, R, VF, VW)
    assert same_bits(got, want)
    valid = want[1] >= 0
    assert valid.any()
    if which == "none":
        assert valid.all()
        nbz, nby, nbx = valid.shape                          # blocks on all six faces of the grid are among them
        assert nbz >= 2 and nby >= 3 and nbx >= 4
    elif which != "warped":
        assert not valid.all()                               # a hole in V_F invalidates its block


def contents(shape, R):
    F = th.smooth_noise(shape, 21, 1.5)
    ints = th.ints(shape, 22)
    zero_bg = np.zeros(shape, F32)
    z, y, x = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    for cz, cy, cx in ((3, 4, 5), (shape[0] - 3, 6, 9), (5, shape[1] - 2, shape[2] - 4)):
        zero_bg += np.exp(-((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) / 6.0).astype(F32)
    zero_bg[zero_bg < 0.05] = 0
    p2 = th.period2(shape)
    W = noise_pair(shape, 21)[1]
    return {
        "identical": (F, F),
        "integer-shift": (ints, np.roll(ints, (1, -1, min(R, 2)), (0, 1, 2))),
        "shift-to-the-cube-face": (ints, np.roll(ints, (0, 0, R), (0, 1, 2))),
        "period-2-ties": (p2, p2),
        "zero-background-blobs": (zero_bg, np.roll(zero_bg, (0, 1, -1), (0, 1, 2))),
        "constant": (np.full(shape, 3.5, F32), F),
        "constant-warped": (F, np.full(shape, -2.0, F32)),
        "huge": ((F * F32(1e30)).astype(F32), (W * F32(1e30)).astype(F32)),
        "subnormal": ((F * F32(1e-38)).astype(F32), (W * F32(1e-38)).astype(F32)),
        "huge-against-subnormal": ((F * F32(1e30)).astype(F32), (W * F32(1e-38)).astype(F32)),
    }


NAMES = sorted(contents((8, 8, 8), 1))


@pytest.mark.parametrize("shape,R", [((20, 12, 16), 3), ((9, 14, 19), 1), ((9, 14, 19), 6)])
@pytest.mark.parametrize("name", NAMES)
def test_records_bit_for_bit_on_special_content(hip, shape, R, name):
    F, W = contents(shape, R)[name]
    want = bm.block_match(F, W, R)
    got = match(hip, F, W, R)
    assert same_bits(got, want)
    disp, cc, var = got
    if name == "identical":
        assert np.all(cc == 1) and np.array_equal(np.round(disp), np.zeros_like(disp))
    if name in ("constant", "constant-warped"):
        assert np.all(cc == -1) and not disp.any() and not var.any()
    if name == "period-2-ties":                              # d = -2, 0, 2 along x tie at 1: d = 0 wins, and its x
        assert np.all(cc == 1) and not disp[0].any()         # neighbours, one period apart, are equal: no x offset
        assert not np.round(disp).any()
    if name == "shift-to-the-cube-face":
        inner = [b for b in th._on_grid_blocks(shape, (R, 0, 0))]
        assert inner
        for bx, by, bz in inner:                             # on the face: no sub-voxel step along x
            assert disp[0, bz, by, bx] == R and cc[bz, by, bx] == 1
    if name == "zero-background-blobs":
        assert (cc == -1).any() and (cc >= 0).any()
    if name in ("huge", "subnormal"):
        assert (cc >= 0).any() and np.isfinite(var).all()
        assert var.max() > 1e38 if name == "huge" else var.max() < 1e-60


# ---- calling contracts (in the manner of tests/test_calling_contracts.py) ----------------------------------------------
def test_work_buffer_is_sized_by_the_library_and_left_alone(hip):
    """sift3d_amd_block_match_work_bytes() is what the entry may touch: 0 bytes.  A buffer of exactly that size between
    guard bands, and a larger one, poisoned with 0xFF and 0x00 and reused: the bands and the buffer keep their bytes
    and the records are those of work=None."""
    import torch
    from tests.test_calling_contracts import guarded
    shape, R = (9, 14, 19), 3
    F, W = noise_pair(shape, 31)
    nz, ny, nx = shape
    need = hip.lib().sift3d_amd_block_match_work_bytes(nx, ny, nz, R)
    assert need == 0
    want = match(hip, F, W, R)
    assert same_bits(want, bm.block_match(F, W, R))
    for size in (need, 4096):
        for fill in (0xFF, 0x00):
            work, bands = guarded(size, fill, "uint8")
            for run in ("first", "second"):
                got = match(hip, F, W, R, work=work)
                torch.cuda.synchronize()
                assert [int((b != fill).sum()) for b in bands] == [0, 0], (size, fill, run)
                assert int((work != fill).sum()) == 0
                assert same_bits(got, want), (size, fill, run)


def test_entry_is_ordered_on_the_callers_stream(hip):
    import torch
    shape, R = (20, 12, 16), 3
    F, W = (dev(a) for a in noise_pair(shape, 41))
    hip.current_stream(refresh=True)
    want = host(hip.block_match(F, W, R))
    twins = [torch.zeros_like(F), torch.zeros_like(W)]
    assert not same_bits(host(hip.block_match(*twins, R)), want)      # zeros, what another stream would read, differ
    delay = torch.ones((128, 512, 512), device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    try:
        with torch.cuda.stream(s):
            hip.current_stream(refresh=True)
            for _ in range(20):
                delay.mul_(1.0001)
            twins[0].copy_(F)
            twins[1].copy_(W)
            got = [t.clone() for t in hip.block_match(*twins, R)]
        hip.current_stream(refresh=True)
        torch.cuda.current_stream().wait_stream(s)
        assert same_bits(host(got), want)
    finally:
        hip.current_stream(refresh=True)


def test_refusals_launch_nothing(hip):
    """every refusal returns -1 before a launch: the outputs keep their poison"""
    import torch
    L = hip.lib()
    shape, R = (8, 8, 8), 2
    F, W = (dev(a) for a in noise_pair(shape, 51))
    V = torch.ones_like(F)
    disp = torch.full((3, 2, 2, 2), 7.0, device="cuda")
    cc = torch.full((2, 2, 2), 7.0, device="cuda")
    var = torch.full((2, 2, 2), 7.0, dtype=torch.float64, device="cuda")
    base = dict(F=F.data_ptr(), nx=8, ny=8, nz=8, W=W.data_ptr(), VF=V.data_ptr(), VW=None, r=R, disp=disp.data_ptr(),
                cc=cc.data_ptr(), var=var.data_ptr())

    def run(**ch):
        a = dict(base)
        a.update(ch)
        return L.sift3d_hip_block_match(a["F"], a["nx"], a["ny"], a["nz"], a["W"], a["VF"], a["VW"], a["r"], a["disp"],
                                        a["cc"], a["var"], None, hip.current_stream())
    for ch in (dict(F=None), dict(W=None), dict(disp=None), dict(cc=None), dict(var=None), dict(nx=0), dict(ny=3),
               dict(nz=-8), dict(r=0), dict(r=7), dict(F=F.data_ptr() + 2), dict(var=var.data_ptr() + 4),
               dict(disp=F.data_ptr()), dict(cc=W.data_ptr() + 64), dict(var=V.data_ptr()), dict(cc=disp.data_ptr() + 8),
               dict(VW=cc.data_ptr())):
        assert run(**ch) == -1, ch
    torch.cuda.synchronize()
    assert bool((disp == 7).all()) and bool((cc == 7).all()) and bool((var == 7).all())
    for bad in (dict(radius=0), dict(radius=7), dict(radius=1.0), dict(valid_fixed=V[:4]), dict(valid_warped=V.double())):
        with pytest.raises(ValueError):
            hip.block_match(F, W, **bad)
    with pytest.raises(ValueError):
        hip.block_match(F, W[:4], 2)
    with pytest.raises(ValueError):
        hip.block_match(F[:, :, :3].contiguous(), W[:, :, :3].contiguous(), 2)
    assert run() == 0


# ---- the driver ------------------------------------------------------------------------------------------------------
def check_trail(res, F, M, levels, WF=None, WM=None, **kw):
    """every entry of the device's trail against one restated iteration from the device's own A_in"""
    Fs, Ms, WFs, WMs = (bm.pyramid(v, levels) for v in (F, M, WF, WM))
    entries = res.trail[:res.iterations]
    assert entries
    for e in entries:
        l = e.level
        A_in = np.array(e.A_in[:]).reshape(3, 4)
        want = bm.iteration(Fs[l], Ms[l], A_in, l, WF=WFs[l], WM=WMs[l], **kw)
        assert not want.failed
        assert (e.n_valid, e.n_selected, e.n_used) == (want.n_valid, want.n_selected, want.n_used)
        A_out = np.array(e.A_out[:]).reshape(3, 4)
        assert bm.corner_move(A_out, want.A_out, Fs[l].shape) <= 1e-9
        assert e.mean_cc == pytest.approx(want.mean_cc, abs=1e-9)
        assert e.rms == pytest.approx(want.rms, abs=1e-9) and e.move == pytest.approx(want.move, abs=1e-9)
    return entries


@pytest.fixture(scope="module")
def rigid_run(hip):
    F, M, At = th.pair48()
    res = hip.block_register(dev(F), dev(M), np.eye(3, 4), hip.block_register_params(levels=2))
    return res


def test_driver_follows_the_restatement_iteration_by_iteration(hip, rigid_run):
    F, M, At = th.pair48()
    res = rigid_run
    entries = check_trail(res, F, M, 2)
    assert [e.level for e in entries] == sorted((e.level for e in entries), reverse=True)
    assert {e.level for e in entries} == {0, 1}
    # the selected set itself: the pairs' count matches, and so does the set (same records, same rule)
    e = entries[-1]
    want = bm.iteration(F, M, np.array(e.A_in[:]).reshape(3, 4), 0)
    assert want.selected.size == e.n_selected and int(want.used.sum()) == e.n_used
    A = np.array(res.A[:]).reshape(3, 4)
    assert np.array_equal(A, np.array(e.A_out[:]).reshape(3, 4))
    assert hip.BLOCK_STOPS[res.stop] in ("converged", "iterations")


def test_driver_meets_the_restatements_bars(hip, rigid_run):
    from sift3d_amd import api
    F, M, At = th.pair48()
    A = np.array(rigid_run.A[:]).reshape(3, 4)
    start = bm.corner_move(np.eye(3, 4), At, F.shape)
    err = bm.corner_move(A, At, F.shape)
    print("pair48 on the device: start %.4f, end %.4f, %d iterations" % (start, err, rigid_run.iterations))
    assert err < 0.5 and err < start / 10.0
    L = A[:, :3]
    assert np.abs(L.T @ L - np.eye(3)).max() <= 1e-12 and np.linalg.det(L) > 0
    out = api.register_blocks(M, F, levels=2)
    assert np.array_equal(out.A, A) and out.stop == hip.BLOCK_STOPS[rigid_run.stop]
    assert len(out.trail) == rigid_run.iterations
    import torch
    warped = torch.empty_like(out.warped)
    hip.warp_affine(dev(M), warped, out.A, "linear")
    assert torch.equal(out.warped, warped)
    assert same_bits([out.warped.cpu().numpy()], [ref_warp(M, out.A, F.shape, "linear", 0.0)[0].astype(F32)])


@pytest.mark.parametrize("model", ["affine", "translation"])
def test_driver_other_models(hip, model):
    F, M, At = th.pair48()
    res = hip.block_register(dev(F), dev(M), np.eye(3, 4), hip.block_register_params(model=model, levels=2, iterations=2))
    check_trail(res, F, M, 2, model=model)
    A = np.array(res.A[:]).reshape(3, 4)
    if model == "translation":
        assert np.array_equal(A[:, :3], np.eye(3))
    else:
        assert bm.corner_move(A, At, F.shape) < bm.corner_move(np.eye(3, 4), At, F.shape) / 4.0


def test_driver_with_masks(hip):
    F, M, At = th.pair48()
    z, y, x = np.meshgrid(*(np.arange(n) for n in F.shape), indexing="ij")
    WF = (((x - 24) ** 2 + (y - 22) ** 2 + (z - 25) ** 2) < 21 ** 2).astype(F32)
    WM = (((x - 23) ** 2 + (y - 25) ** 2 + (z - 24) ** 2) < 22 ** 2).astype(F32)
    res = hip.block_register(dev(F), dev(M), np.eye(3, 4), hip.block_register_params(levels=2, iterations=2),
                             mask_fixed=dev(WF), mask_moving=dev(WM))
    entries = check_trail(res, F, M, 2, WF=WF, WM=WM)
    assert entries[-1].n_valid < (48 // 4) ** 3 // 2         # the masks cut the blocks down
    one = hip.block_register(dev(F), dev(M), np.eye(3, 4), hip.block_register_params(levels=2, iterations=1),
                             mask_fixed=dev(WF))
    check_trail(one, F, M, 2, WF=WF)


def test_driver_with_spacing(hip):
    """anisotropic voxels: the fitted map is rigid in physical space, not in voxels"""
    F, M, At = th.pair48()
    sf, sm = (0.8, 0.8, 2.0), (0.8, 0.8, 2.0)
    p = hip.block_register_params(levels=2, iterations=2, spacing_fixed=sf, spacing_moving=sm)
    res = hip.block_register(dev(F), dev(M), np.eye(3, 4), p)
    check_trail(res, F, M, 2, spacing_fixed=sf, spacing_moving=sm)
    A = np.array(res.A[:]).reshape(3, 4)
    s = np.array(sf)
    L = A[:, :3] * s[:, None] / s[None, :]
    assert np.abs(L.T @ L - np.eye(3)).max() <= 1e-12
    assert np.abs(A[:, :3].T @ A[:, :3] - np.eye(3)).max() > 1e-6


def test_driver_fails_cleanly_on_flat_volumes(hip):
    flat = dev(np.full((16, 16, 16), 2.0, F32))
    A0 = np.eye(3, 4) + [[0, 0, 0, 1.0]] * 3
    res = hip.block_register(flat, flat, A0, hip.block_register_params(levels=1))
    assert hip.BLOCK_STOPS[res.stop] == "failed" and res.iterations == 1
    e = res.trail[0]
    assert e.n_valid == 0 and e.n_used == 0 and np.isnan(e.move)
    assert np.array_equal(np.array(res.A[:]).reshape(3, 4), A0)


# ---- the public entries ----------------------------------------------------------------------------------------------
def test_public_block_match_is_the_hip_layer(hip):
    import torch
    from sift3d_amd import api
    shape = (20, 12, 16)
    F, M = noise_pair(shape, 61)
    A = np.array([[1, 0.01, 0, 0.5], [0, 1, 0, -0.25], [0, -0.01, 1, 0.75]])
    VF, VM = masks(shape, 62)
    for mf, mm in ((None, None), (VF, VM)):
        W = torch.empty(shape, device="cuda")
        hip.warp_affine(dev(M), W, A)
        VW = torch.empty(shape, device="cuda")
        hip.warp_affine(dev(np.ones(shape, F32) if mm is None else mm), VW, A, "nearest")
        disp, cc, var = host(hip.block_match(dev(F), W, 3, dev(mf), VW))
        keep = np.nonzero(cc.reshape(-1) >= 0)[0]
        on_host = api.block_match(F, M, A, 3, mf, mm)
        on_dev = api.block_match(dev(F), dev(M), A, 3, dev(mf), dev(mm))
        for out in (on_host, on_dev):
            assert np.array_equal(out.cc, cc.reshape(-1)[keep]) and np.array_equal(out.variance, var.reshape(-1)[keep])
            nbx, nby = shape[2] // 4, shape[1] // 4
            centres = np.stack([4.0 * (keep % nbx) + 1.5, 4.0 * (keep // nbx % nby) + 1.5,
                                4.0 * (keep // (nbx * nby)) + 1.5], 1)
            assert np.array_equal(out.points_fixed, centres)
            q = centres + disp.reshape(3, -1)[:, keep].T.astype(np.float64)
            assert np.allclose(out.points_moving, q @ A[:, :3].T + A[:, 3], rtol=0, atol=1e-12)
    same = api.block_match(F, F)
    assert np.all(same.cc == 1) and len(same.cc) == 60


def test_public_fit_and_registration_are_the_hip_layer(hip):
    from sift3d_amd import api
    src = np.random.default_rng(1).uniform(0, 64, (50, 3))
    dst = src @ th.RIGID[:, :3].T + th.RIGID[:, 3]
    dst[:10] += 30.0
    T, used, its = hip.fit_trimmed(src, dst, "rigid", 0.5, 20, (1, 1, 2), (1, 1, 2))
    fit = api.fit_transform(src, dst, "rigid", 0.5, (1, 1, 2), (1, 1, 2))
    assert np.array_equal(fit.A, T) and np.array_equal(fit.used, used) and fit.iterations == its
    F, M, At = th.pair48()
    kw = dict(model="affine", levels=2, iterations=2, radius=2, keep_blocks=0.75, keep_inliers=0.6, tol=0.02)
    res = hip.block_register(dev(F), dev(M), np.eye(3, 4), hip.block_register_params(**kw))
    for f, m in ((F, M), (dev(F), dev(M))):
        out = api.register_blocks(m, f, **kw)
        assert np.array_equal(out.A, np.array(res.A[:]).reshape(3, 4))
        assert [(e.level, e.n_valid, e.n_selected, e.n_used) for e in out.trail] == \
            [(e.level, e.n_valid, e.n_selected, e.n_used) for e in res.trail[:res.iterations]]
    started = api.register_blocks(M, F, A=At, levels=1, iterations=1)
    assert bm.corner_move(started.A, At, F.shape) < 0.5
