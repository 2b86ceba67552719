"""Free-form deformation on the device (include/sift3d_amd.h, "B-spline free-form deformation") against the numpy
restatement (tests/ffd_restatement.py): the field, the subdivision and the count bit for bit; S_ee and every entry of
Gc to gamma_(k + 8) sum |terms| (k the voxels under the control; gamma_n bounds any order of summing n doubles, the
restatement's own sums are correctly rounded, and a term carries at most 8 roundings however it is factored); the
bending energy to the bound of its double sums; the driver against the restatement's driver on the pair of
tests/test_ffd_host.py."""
import numpy as np
import pytest

from tests import ffd_restatement as fr
from tests.demons_restatement import gamma
from tests.test_ffd_host import DRIVER, check_trail, driver_pair, restatement_driver, summarize
from tests.test_similarity import TILE, dev, volumes
from tests.test_warp import about_center, rot

pytestmark = pytest.mark.gpu

# (oz, oy, ox), (dx, dy, dz): the issue's grids
GRIDS = [((5, 9, 17), (4, 3, 2)), ((8, 8, 64), (8, 8, 8)), ((3, 4, 5), (8, 8, 8)), ((5, 6, 33), (1, 1, 1)),
         ((9, 5, 130), (7, 2, 3))]


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


def random_lattice(shape, spacing, seed, amplitude=1.5):
    rng = np.random.default_rng(seed)
    return rng.uniform(-amplitude, amplitude, fr.lattice_shape(shape, spacing)).astype(np.float32)


def rotating(shape):
    return about_center(rot((1, 2, 3), 7.0), shape, shape, shift=(0.3, -0.2, 0.1))


@pytest.mark.parametrize("k", range(len(GRIDS)))
@pytest.mark.parametrize("affine", [False, True])
def test_field_bit_for_bit(hip, k, affine):
    import torch
    shape, spacing = GRIDS[k]
    c = random_lattice(shape, spacing, k)
    A = rotating(shape) if affine else None
    out = torch.empty((3,) + shape, dtype=torch.float32, device="cuda")
    got = hip.ffd_field(dev(c), spacing, out, A).cpu().numpy()
    assert np.array_equal(got, fr.field(c, spacing, shape, A))


def check_record(hip, F, M, c, spacing, A, what):
    rec, grad, fld = hip.ffd_evaluate(dev(F), dev(M), dev(c), spacing, A, bending=0.01)
    n, see, R, gmax, Gc, dR = hip.ffd_record(rec, c.shape)
    want, u = fr.evaluate(F, M, c, spacing, A)
    assert np.array_equal(fld.cpu().numpy(), u), what
    assert n == want.n, (what, n, want.n)
    print("%s: n %d S_ee %.9g (off %.3g)" % (what, n, see, abs(see - want.see)))
    assert abs(see - want.see) <= gamma(F.size + 8) * want.see_terms, (what, see, want.see)
    bound = np.array([gamma(int(k) + 8) for k in want.support.reshape(-1)]).reshape(want.support.shape) * want.Gc_terms
    off = np.abs(Gc - want.Gc)
    assert np.all(off <= bound), (what, off.max(), (off - bound).max())
    Rw, dRw, Rt, dRt = fr.bending(c, spacing)
    assert abs(R - Rw) <= gamma(6 * 40 + c.size) * Rt, (what, R, Rw)
    assert np.all(np.abs(dR - dRw) <= gamma(200) * dRt), what
    if n:
        g, gm = fr.gradient(want._replace(Gc=Gc), dR, 0.01)              # from the device's own sums: bit for bit
        assert np.array_equal(grad.cpu().numpy(), g) and gmax == gm, what
    return rec, n, see, Gc


@pytest.mark.parametrize("k", range(len(GRIDS)))
def test_record(hip, k):
    shape, spacing = GRIDS[k]
    mshape = (shape[0] + 1, shape[1] + 2, shape[2] - 1)
    F, M = volumes(shape, mshape, 20 + k)
    zero = np.zeros(fr.lattice_shape(shape, spacing), np.float32)
    rnd = random_lattice(shape, spacing, 30 + k)
    partly = np.eye(3, 4)
    partly[:, 3] = [shape[2] * 0.4, -0.3, 0.2]
    outside = np.eye(3, 4)
    outside[:, 3] = [1000.0, 0.0, 0.0]
    check_record(hip, F, M, zero, spacing, None, "%s zero" % (shape,))
    check_record(hip, F, M, rnd, spacing, rotating(shape), "%s random" % (shape,))
    _, n, _, _ = check_record(hip, F, M, rnd, spacing, partly, "%s partly outside" % (shape,))
    assert 0 < n < F.size
    rec, n, see, Gc = check_record(hip, F, M, zero, spacing, outside, "%s outside" % (shape,))
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
    F, M = volumes(shape, (shape[0] - 3, shape[1] + 2, 3), 3)
    c = random_lattice(shape, spacing, 7, 0.5)
    check_record(hip, F, M, c, spacing, None, "grid cap")
    r0, g0, _ = hip.ffd_evaluate(dev(F), dev(M), dev(c), spacing, None, 0.01)
    r1, g1, _ = hip.ffd_evaluate(dev(F), dev(M), dev(c), spacing, None, 0.01)
    assert np.array_equal(r0.cpu().numpy(), r1.cpu().numpy()) and np.array_equal(g0.cpu().numpy(), g1.cpu().numpy())


@pytest.mark.parametrize("shape,spacing", [((4, 4, 4), (3, 2, 1)), ((7, 6, 5), (8, 8, 8)), ((12, 9, 21), (4, 3, 2))])
def test_bending(hip, shape, spacing):
    from sift3d_amd import api
    rng = np.random.default_rng(shape[2])
    c = rng.standard_normal((3,) + shape).astype(np.float32)
    R, dR = api.ffd_bending_energy(dev(c), spacing)
    Rw, dRw, Rt, dRt = fr.bending(c, spacing)
    assert R > 0 and abs(R - Rw) <= gamma(6 * 40 + c.size) * Rt
    assert np.all(np.abs(dR - dRw) <= gamma(200) * dRt) and dR.any()


@pytest.mark.parametrize("shape,spacing", [((9, 10, 21), (4, 3, 2)), ((5, 8, 8), 8), ((3, 4, 5), 8), ((6, 7, 33), 1),
                                           ((48, 48, 48), 8)])
def test_refine2_bit_for_bit(hip, shape, spacing):
    coarse = random_lattice(tuple((o + 1) // 2 for o in shape), spacing, 11)
    got = hip.ffd_refine2(dev(coarse), shape, spacing).cpu().numpy()
    assert np.array_equal(got, fr.refine2(coarse, shape, spacing))


@pytest.fixture(scope="module")
def device_driver():
    from sift3d_amd import api
    F, M, truth = driver_pair()
    return api.refine_ffd(M, F, None, DRIVER["spacing"], DRIVER["levels"], DRIVER["bending"],
                          max_evaluations=DRIVER["max_evaluations"])


def test_driver_against_the_restatement(device_driver):
    """The device's summation order may flip one accept / reject, hence the margins: the MSD falls by at least half
    the factor the restatement reached, the RMS field error is at most 1.5 x the restatement's."""
    F, M, truth = driver_pair()
    _, (ratio_ref, rms_ref) = restatement_driver()
    r = device_driver
    trail = [tuple(e) for e in r.trail]
    ratio, rms = summarize(trail, r.field.cpu().numpy(), truth)
    print("device driver: stop %s, %d evaluations, MSD ratio %.4g (restatement %.4g), RMS %.4g (restatement %.4g)"
          % (r.stop, len(trail), ratio, ratio_ref, rms, rms_ref))
    check_trail(trail, DRIVER["levels"], DRIVER["max_evaluations"])
    assert 1.0 / ratio >= 0.5 / ratio_ref
    assert rms <= 1.5 * rms_ref
    assert r.jacobian.folded == 0
    assert tuple(r.lattice.shape) == fr.lattice_shape(F.shape, DRIVER["spacing"]) and r.spacing == (8, 8, 8)
    assert np.array_equal(r.field.cpu().numpy(), fr.field(r.lattice.cpu().numpy(), 8, F.shape))
    assert tuple(r.warped.shape) == F.shape


def test_bending_weight_smooths_the_field():
    from sift3d_amd import api
    F, M, _ = driver_pair()
    R = []
    for lam in (0.0, 1e3):
        r = api.refine_ffd(M, F, None, 8, 2, lam, max_evaluations=10)
        R.append(api.ffd_bending_energy(r.lattice, 8)[0])
    print("R at bending 0: %.4g, at 1e3: %.4g" % tuple(R))
    assert R[1] < R[0]


def test_register_ffd_end_to_end():
    from sift3d_amd import api
    F, M, _ = driver_pair()
    r = api.register_ffd(M, F, levels=2, ffd_params=dict(max_evaluations=10))
    assert r.refinement.stop in ("converged", "evaluations", "flat", "failed")
    assert r.refinement.trail[-1].level == 0 and tuple(r.refinement.field.shape) == (3,) + F.shape
    acc = [e.E for e in r.refinement.trail if e.level == 0 and e.accepted]
    assert all(b < a for a, b in zip(acc, acc[1:]))
