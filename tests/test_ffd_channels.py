"""Multi-channel free-form deformation on the device (include/sift3d_amd.h, "Multi-channel free-form deformation")
against the numpy restatement (tests/ffd_channels_restatement.py): with one channel the bytes of the single-channel
evaluation; with more the field, the count and the force S bit for bit, S_ee to gamma_(nc voxels + 8) sum E E and every
entry of Gc to gamma_(k + nc + 8) sum |W E_c g_cd| (k the voxels under the control; the restatement's own sums are
correctly rounded), the gradient bit for bit from the device's own sums; the driver against the restatement's driver on
the pair of tests/test_ffd_host.py with the descriptors of every level; and what the feature is for."""
import numpy as np
import pytest

from tests import ffd_channels_restatement as fc
from tests import ffd_restatement as fr
from tests.demons_restatement import gamma
from tests.test_ffd import GRIDS, random_lattice, rotating
from tests.test_ffd_channels_host import GAIN, OFFSET, SIGMA, mapped_pair, restatement_driver, zero_field_rms
from tests.test_ffd_host import DRIVER, check_trail, driver_pair, summarize
from tests.test_similarity import TILE, dev, volumes

pytestmark = pytest.mark.gpu
BENDING = 0.01


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


def stacks(fshape, mshape, nc, seed):
    """nc channels of tests/test_similarity.py's volumes"""
    pairs = [volumes(fshape, mshape, seed + 100 * c) for c in range(nc)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def masks(fshape, mshape, seed):
    rng = np.random.default_rng(seed)
    return ((rng.uniform(size=fshape) > 0.25).astype(np.float32), (rng.uniform(size=mshape) > 0.25).astype(np.float32))


def bytes_of(t):
    import torch
    return t.contiguous().view(torch.uint8).cpu().numpy()


def force_of(hip, work, spacing, shape):
    """S [3, oz, oy, ox] float64 from the work buffer, at the offset the header documents"""
    import torch
    off = 16 * sum(spacing) + 16 * hip.SIMILARITY_GRID
    n = 3 * int(np.prod(shape))
    return work.view(torch.uint8)[off:off + 8 * n].cpu().numpy().view(np.float64).reshape((3,) + tuple(shape))


def check_channels(hip, F, M, c, spacing, A, WF, WM, what):
    """one evaluation against the restatement; returns (record tensor, grad tensor, n, S_ee, Gc)"""
    nc, shape = F.shape[0], F.shape[1:]
    dWF, dWM = (None if w is None else dev(w) for w in (WF, WM))
    rec, grad, fld, work = hip.ffd_evaluate_channels(dev(F), dev(M), dev(c), spacing, A, BENDING, None, dWF, dWM)
    n, see, R, gmax, Gc, dR = hip.ffd_record(rec, c.shape)
    S = force_of(hip, work, spacing, shape)
    want, u = fc.evaluate(F, M, c, spacing, A, WF, WM)
    assert np.array_equal(fld.cpu().numpy(), u), what
    assert n == want.n, (what, n, want.n)
    assert np.array_equal(S.view(np.uint64), want.S.view(np.uint64)), what           # bit for bit, signed zeros too
    print("%s: n %d S_ee %.9g (off %.3g)" % (what, n, see, abs(see - want.see)))
    assert abs(see - want.see) <= gamma(nc * F[0].size + 8) * want.see_terms, (what, see, want.see)
    bound = np.array([gamma(int(k) + nc + 8) for k in want.support.reshape(-1)]).reshape(want.support.shape)
    off = np.abs(Gc - want.Gc)
    assert np.all(off <= bound * want.Gc_terms), (what, off.max(), (off - bound * want.Gc_terms).max())
    if n:
        g, gm = fr.gradient(want._replace(Gc=Gc), dR, BENDING)           # from the device's own sums: bit for bit
        assert np.array_equal(grad.cpu().numpy(), g) and gmax == gm, what
    return rec, grad, n, see, Gc


# ---- one channel: the single-channel evaluation's bytes ------------------------------------------------------------
ONE = [(shape, spacing, (shape[0] + 1, shape[1] + 2, shape[2] - 1)) for shape, spacing in GRIDS] + \
      [((5, 6, 9), (4, 3, 2), (6, 7, 1))]                                # a moving grid of nx == 1: LINEAR 1


@pytest.mark.parametrize("k", range(len(ONE)))
@pytest.mark.parametrize("masked", [False, True])
def test_one_channel_writes_the_bytes_of_ffd_evaluate(hip, k, masked):
    shape, spacing, mshape = ONE[k]
    F, M = volumes(shape, mshape, 40 + k)
    c = random_lattice(shape, spacing, 50 + k)
    A = np.array(rotating(shape), np.float64).reshape(3, 4)
    if mshape[2] == 1:                                                   # q_x = 0 everywhere: x inside the one column
        A[0] = 0.0
        c[0] = 0.0
    W = [dev(w) for w in masks(shape, mshape, k)] if masked else [None, None]
    r0, g0, f0 = hip.ffd_evaluate(dev(F), dev(M), dev(c), spacing, A, BENDING, None, *W)
    r1, g1, f1, _ = hip.ffd_evaluate_channels(dev(F[None]), dev(M[None]), dev(c), spacing, A, BENDING, None, *W)
    n = hip.ffd_record(r0, c.shape)[0]
    assert 0 < n < F.size
    for a, b, name in ((r0, r1, "record"), (g0, g1, "gradient"), (f0, f1, "field")):
        assert np.array_equal(bytes_of(a), bytes_of(b)), name


# ---- every instantiation at nc in {2, 3, 12} -----------------------------------------------------------------------
@pytest.mark.parametrize("ox", [1, 5, 64, 70])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("linear", [1, 2])
@pytest.mark.parametrize("nc", [2, 3, 12])
def test_every_instantiation(hip, nc, linear, masked, ox):
    shape, spacing = (5, 6, ox), (4, 3, 2)
    mshape = (6, 7, 1) if linear == 1 else (6, 7, max(ox - 1, 2))
    F, M = stacks(shape, mshape, nc, 3 * nc + ox)
    c = random_lattice(shape, spacing, ox + nc, 1.0)
    A = np.eye(3, 4)
    A[:, 3] = [0.4, -0.3, 0.6]                                           # partly outside along y
    if linear == 1:
        A[0] = 0.0
        c[0] = 0.0
    WF, WM = masks(shape, mshape, ox) if masked else (None, None)
    what = "nc %d LINEAR %d masked %d ox %d" % (nc, linear, masked, ox)
    rec, grad, n, _, Gc = check_channels(hip, F, M, c, spacing, A, WF, WM, what)
    assert 0 < n < F[0].size and Gc.any(), (what, n)
    if masked:                                                           # all-ones masks: the unmasked bytes
        ones = [dev(np.ones(s, np.float32)) for s in (shape, mshape)]
        a = hip.ffd_evaluate_channels(dev(F), dev(M), dev(c), spacing, A, BENDING, None, *ones)
        b = hip.ffd_evaluate_channels(dev(F), dev(M), dev(c), spacing, A, BENDING)
        for x, y in zip(a[:3], b[:3]):
            assert np.array_equal(bytes_of(x), bytes_of(y)), what
        assert np.array_equal(force_of(hip, a[3], spacing, shape).view(np.uint64),
                              force_of(hip, b[3], spacing, shape).view(np.uint64)), what


# ---- edge cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(GRIDS)))
def test_record(hip, k):
    """tests/test_ffd.py's test_record over three channels"""
    shape, spacing = GRIDS[k]
    mshape = (shape[0] + 1, shape[1] + 2, shape[2] - 1)
    F, M = stacks(shape, mshape, 3, 20 + k)
    zero = np.zeros(fr.lattice_shape(shape, spacing), np.float32)
    rnd = random_lattice(shape, spacing, 30 + k)
    partly = np.eye(3, 4)
    partly[:, 3] = [shape[2] * 0.4, -0.3, 0.2]
    outside = np.eye(3, 4)
    outside[:, 3] = [1000.0, 0.0, 0.0]
    check_channels(hip, F, M, zero, spacing, None, None, None, "%s zero" % (shape,))
    check_channels(hip, F, M, rnd, spacing, rotating(shape), None, None, "%s random" % (shape,))
    _, _, n, _, _ = check_channels(hip, F, M, rnd, spacing, partly, None, None, "%s partly outside" % (shape,))
    assert 0 < n < F[0].size
    rec, _, n, see, Gc = check_channels(hip, F, M, zero, spacing, outside, None, None, "%s outside" % (shape,))
    assert n == 0 and see == 0.0 and not Gc.any()
    raw = rec.cpu().numpy()
    assert not raw[:2].any() and not raw[4:4 + Gc.size].any()            # n, S_ee and Gc: all-zero bytes


def test_more_tiles_than_workgroups_and_calls_repeat(hip):
    G = hip.SIMILARITY_GRID
    ty = int(np.ceil(np.sqrt(G + 1)))
    tz = -(-(G + 1) // ty)
    shape = (TILE[0] * (tz - 1) + 1, TILE[1] * (ty - 1) + 1, 2)
    assert G < ty * tz < 2 * G
    spacing = (2, 16, 16)
    F, M = stacks(shape, (shape[0] - 3, shape[1] + 2, 3), 2, 3)
    c = random_lattice(shape, spacing, 7, 0.5)
    check_channels(hip, F, M, c, spacing, None, None, None, "grid cap")
    a = hip.ffd_evaluate_channels(dev(F), dev(M), dev(c), spacing, None, BENDING)
    b = hip.ffd_evaluate_channels(dev(F), dev(M), dev(c), spacing, None, BENDING)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(bytes_of(x), bytes_of(y))


# ---- the driver ----------------------------------------------------------------------------------------------------
def run_descriptors(M, F, **kw):
    from sift3d_amd import api
    return api.refine_ffd(M, F, None, DRIVER["spacing"], DRIVER["levels"], DRIVER["bending"],
                          max_evaluations=DRIVER["max_evaluations"], features="descriptors", sigma=SIGMA, **kw)


def test_driver_against_the_restatement():
    """tests/test_ffd.py's test_driver_against_the_restatement with features="descriptors", its margins unchanged: the
    device's summation order may flip one accept / reject, so the cost falls by at least half the factor the
    restatement reached and the RMS field error is at most 1.5 x the restatement's.  The whole 48^3 pair on both
    sides (the numpy driver takes about 40 s on it)."""
    F, M, truth = driver_pair()
    _, (ratio_ref, rms_ref) = restatement_driver()
    r = run_descriptors(M, F)
    assert type(r).__name__ == "FFDRefinement"
    trail = [tuple(e) for e in r.trail]
    ratio, rms = summarize(trail, r.field.cpu().numpy(), truth)
    print("device driver, descriptors: stop %s, %d evaluations, cost ratio %.4g (restatement %.4g), RMS %.4g "
          "(restatement %.4g)" % (r.stop, len(trail), ratio, ratio_ref, rms, rms_ref))
    check_trail(trail, DRIVER["levels"], DRIVER["max_evaluations"])
    assert 1.0 / ratio >= 0.5 / ratio_ref
    assert rms <= 1.5 * rms_ref
    assert r.jacobian.folded == 0
    assert tuple(r.lattice.shape) == fr.lattice_shape(F.shape, DRIVER["spacing"]) and r.spacing == (8, 8, 8)
    assert np.array_equal(r.field.cpu().numpy(), fr.field(r.lattice.cpu().numpy(), 8, F.shape))
    assert tuple(r.warped.shape) == F.shape


def test_descriptors_survive_a_gain_and_an_offset():
    """What the feature is for, on the device: the moving volume mapped m -> 3 m + 20.  The descriptor run's RMS field
    error is below the zero field's and below the intensity-MSD run's on the same pair.  The restatement's side of the
    same two assertions is tests/test_ffd_channels_host.py's (the CPU suite); DESIGN.md 3.4.16 records the figures."""
    from sift3d_amd import api
    F, M, truth = mapped_pair(GAIN, OFFSET)
    zero = zero_field_rms(truth)
    rd = run_descriptors(M, F)
    ri = api.refine_ffd(M, F, None, DRIVER["spacing"], DRIVER["levels"], DRIVER["bending"],
                        max_evaluations=DRIVER["max_evaluations"])
    rms_desc = summarize([tuple(e) for e in rd.trail], rd.field.cpu().numpy(), truth)[1]
    rms_int = summarize([tuple(e) for e in ri.trail], ri.field.cpu().numpy(), truth)[1]
    print("device, m -> 3 m + 20: RMS field error descriptors %.4g, intensity MSD %.4g, zero field %.4g"
          % (rms_desc, rms_int, zero))
    assert rms_desc < zero
    assert rms_desc < rms_int


# ---- api.refine_ffd's other ways in ---------------------------------------------------------------------------------
def two_contrasts():
    """the driver pair as two channels: the volumes and their squares"""
    F, M, _ = driver_pair()
    return np.stack([F, F * F]), np.stack([M, M * M])


def test_two_channel_stacks(hip):
    """4-D input: the stacks restricted per level, the binding's own call, every channel warped"""
    from sift3d_amd import api
    F, M = two_contrasts()
    r = api.refine_ffd(M, F, None, DRIVER["spacing"], 2, DRIVER["bending"], max_evaluations=6)
    assert type(r).__name__ == "FFDRefinement"
    trail = [tuple(e) for e in r.trail]
    check_trail(trail, 2, 6)
    assert np.array_equal(r.field.cpu().numpy(), fr.field(r.lattice.cpu().numpy(), 8, F.shape[1:]))
    assert tuple(r.warped.shape) == F.shape
    dF, dM = dev(F), dev(M)
    res, lattice, field, pen = hip.ffd_refine_channels(
        [dF, hip.restrict2(dF)], [dM, hip.restrict2(dM)], None,
        hip.ffd_refine_params(spacing=8, levels=2, bending=DRIVER["bending"], max_evaluations=6))
    assert pen is None and res.evaluations == len(trail)
    assert np.array_equal(bytes_of(lattice), bytes_of(r.lattice)) and np.array_equal(bytes_of(field), bytes_of(r.field))
    want, _ = fc.evaluate(*(fc.pyramid(v, 2)[1] for v in (F, M)), np.zeros(fr.lattice_shape((24, 24, 24), 8), np.float32),
                          8)
    first = r.trail[0]                                                   # the coarsest level's first evaluation
    assert first.level == 1 and first.n == want.n
    assert abs(first.msd * first.n - want.see) <= (gamma(2 * 24 ** 3 + 8) + 4 * 2.0 ** -53) * want.see_terms


def test_jacobian_penalty_with_descriptors():
    from sift3d_amd import api
    F, M, _ = driver_pair()
    w = 0.01
    r = api.refine_ffd(M, F, None, DRIVER["spacing"], 2, DRIVER["bending"], max_evaluations=6, jacobian=w,
                       features="descriptors")
    assert type(r).__name__ == "JacFFDRefinement"
    assert r.jacobian_weight == w and len(r.penalty) == len(r.trail) > 2
    for e, q in zip(r.trail, r.penalty):
        assert e.E == (e.msd + DRIVER["bending"] * e.R) + w * q.P, (e, q)
    last = [q for e, q in zip(r.trail, r.penalty) if e.level == 0 and e.accepted][-1]
    at_end = api.jacobian_penalty(r.field)
    assert (last.P, last.rmin, last.nonpositive) == (at_end.value, at_end.min, at_end.nonpositive)


def test_mask_fixed_with_descriptors():
    """a fixed mask over half the grid: every level counts about half the voxels (the float mask restricted per level),
    and the all-ones mask gives the unmasked call's bytes"""
    from sift3d_amd import api
    F, M, _ = driver_pair()
    W = np.zeros(F.shape, np.float32)
    W[:, :, :24] = 1.0
    kw = dict(max_evaluations=6, features="descriptors")
    r = api.refine_ffd(M, F, None, DRIVER["spacing"], 2, DRIVER["bending"], mask_fixed=W, **kw)
    check_trail([tuple(e) for e in r.trail], 2, 6)
    for e in r.trail:
        full = (48 >> e.level) ** 3
        assert 0.25 * full <= e.n <= 0.5 * full, e
    a = api.refine_ffd(M, F, None, DRIVER["spacing"], 2, DRIVER["bending"], mask_fixed=np.ones_like(W), **kw)
    b = api.refine_ffd(M, F, None, DRIVER["spacing"], 2, DRIVER["bending"], **kw)
    assert np.array_equal(bytes_of(a.lattice), bytes_of(b.lattice)) and [tuple(e) for e in a.trail] == \
        [tuple(e) for e in b.trail]


def test_register_ffd_end_to_end():
    from sift3d_amd import api
    F, M, _ = driver_pair()
    r = api.register_ffd(M, F, levels=2, ffd_params=dict(features="descriptors", max_evaluations=10))
    assert r.refinement.stop in ("converged", "evaluations", "flat", "failed")
    assert r.refinement.trail[-1].level == 0 and tuple(r.refinement.field.shape) == (3,) + F.shape
    acc = [e.E for e in r.refinement.trail if e.level == 0 and e.accepted]
    assert all(b < a for a, b in zip(acc, acc[1:]))
