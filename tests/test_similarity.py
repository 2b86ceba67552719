"""Similarity measures on the device (sift3d_hip_similarity_affine / _field; include/sift3d_amd.h, "Similarity
measures") against the numpy restatement (tests/similarity_restatement.py): the joint histogram and the count bit for
bit in every case; the moments exactly where every term is an integer, and otherwise to gamma_n sum |terms|, the bound
on any order of summing n doubles (tests/demons_restatement.gamma; the restatement's own sums are correctly rounded)."""
import numpy as np
import pytest

from tests import field_restatement as fr
from tests import similarity_restatement as sr
from tests.demons_restatement import gamma
from tests.test_similarity_host import end_to_end_case, measure_bounds, shifted
from tests.test_warp import about_center, rot

pytestmark = pytest.mark.gpu

TILE = (4, 4, 64)                                           # a tile's outputs (z, y, x)

# fixed [oz, oy, ox] -> moving [nz, ny, nx]: axes of 1 and 2 (so LINEAR == 1 with nx == 1), partial tiles on every
# axis, ox % 4 != 0, several tiles, and grids that differ
SHAPES = [((1, 1, 1), (1, 1, 1)), ((1, 1, 7), (2, 3, 1)), ((2, 3, 5), (3, 2, 6)), ((5, 7, 9), (6, 5, 8)),
          ((4, 4, 64), (5, 6, 60)), ((5, 6, 70), (5, 6, 70)), ((9, 20, 133), (8, 21, 130))]
BINS = [2, 50, 64, 128]


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def volumes(fshape, mshape, seed, lo=-1.0, hi=1.5):
    """normal content with values exactly at lo, at hi and beyond both ends of the range (lo, hi)"""
    rng = np.random.default_rng(seed)
    out = []
    for shape in (fshape, mshape):
        v = rng.normal(0, 1, shape).astype(np.float32)
        flat = v.reshape(-1)
        for k, val in enumerate((lo, hi, lo - 2.0, hi + 3.0)):
            flat[(k * 7) % flat.size::max(flat.size // 3, 1)] = val
        out.append(v)
    return out


def transforms(fshape, mshape):
    """name -> 3 x 4 pull map: identity, integer shift, a rotation about the centre that samples partly outside, and
    one that samples everything outside"""
    shift = np.eye(3, 4)
    shift[:, 3] = [min(1, mshape[2] - 1), 0, min(1, mshape[0] - 1)]
    far = np.eye(3, 4)
    far[0, 3] = mshape[2] + 5.0
    return {"identity": np.eye(3, 4), "shift": shift, "outside": far,
            "rotation": about_center(rot((1, 2, 3), 25.0) * 1.1, mshape, fshape, shift=(0.3, -0.2, 0.1))}


def check(hip, F, M, T, bins, rf, rm, interp, what, exact=False):
    """one call against the restatement; T: None, a 3 x 4 array or a numpy field.  Returns (hist, count, sums)."""
    Td = dev(T.astype(np.float32)) if isinstance(T, np.ndarray) and T.ndim == 4 else T
    hist, stats = hip.similarity(dev(F), dev(M), Td, bins, rf, rm, interp)
    count, sums = hip.similarity_stats(stats)
    want_hist, want = sr.joint(F, M, T, bins, rf, rm, interp)
    np.testing.assert_array_equal(hist.cpu().numpy(), want_hist.astype(np.int64), err_msg=what)
    assert count == want.count == int(want_hist.sum()), (what, count, want.count)
    for k, name in enumerate(sr.SUMS):
        bound = 0.0 if exact else gamma(max(count, 1)) * want.terms[k]
        assert abs(sums[k] - want.sums[k]) <= bound, (what, name, sums[k], want.sums[k], bound)
    return hist.cpu().numpy(), count, sums


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_shapes_transforms_entries_interps(hip, k):
    from sift3d_amd import api
    fshape, mshape = SHAPES[k]
    F, M = volumes(fshape, mshape, 10 + k)
    rf, rm = (-1.0, 1.5), (-1.0, 1.5)
    n = 0
    for name, A in transforms(fshape, mshape).items():
        noise = np.random.default_rng(k).normal(0, 0.3, (3,) + fshape).astype(np.float32)
        field = fr.ref_affine_field(A, fshape) + (noise if name == "rotation" else 0)
        for T in (A, field.astype(np.float32)):
            for interp in ("linear", "nearest"):
                bins = BINS[n % 4]
                n += 1
                what = "%s -> %s %s %s %s B=%d" % (fshape, mshape, name, "affine" if T.ndim == 2 else "field", interp,
                                                  bins)
                hist, count, sums = check(hip, F, M, T, bins, rf, rm, interp, what)
                if name == "outside":
                    assert count == 0 and not hist.any() and not sums.any(), what
                    got = api.similarity_measures(hist, (count, sums))
                    assert all(np.isnan(v) for v in got[1:8]), what
    if fshape == mshape:
        for bins in BINS:
            check(hip, F, M, None, bins, rf, rm, "linear", "%s None B=%d" % (fshape, bins))


def test_more_tiles_than_workgroups(hip):
    """The smallest grid whose tiles exceed the launch's workgroups (SIFT3D_AMD_SIMILARITY_GRID) by a partial pass:
    one tile along x, and ty * tz >= GRID + 1 tiles with ty = ceil(sqrt(GRID + 1)): the walk takes a second pass that
    only some workgroups have a tile in, and every workgroup flushes."""
    G = hip.SIMILARITY_GRID
    ty = int(np.ceil(np.sqrt(G + 1)))
    tz = -(-(G + 1) // ty)
    fshape = (TILE[0] * (tz - 1) + 1, TILE[1] * (ty - 1) + 1, 2)
    assert G < ty * tz < 2 * G
    F, M = volumes(fshape, (fshape[0] - 3, fshape[1] + 2, 3), 3)
    A = about_center(rot((1, 0, 0), 10.0), M.shape, fshape, shift=(0.2, 0, 0))
    check(hip, F, M, A, 50, (-1.0, 1.5), (-1.0, 1.5), "linear", "grid cap affine")
    check(hip, F, M, fr.ref_affine_field(A, fshape), 128, (-1.0, 1.5), (-1.0, 1.5), "linear", "grid cap field")


@pytest.mark.parametrize("bins", BINS)
def test_one_bin_and_mixed_waves(hip, bins):
    """every voxel in one bin: each wave commits with one add.  Constant but for one voxel per tile: the waves that
    hold such a voxel commit lane by lane, the others with one add."""
    shape = (9, 20, 133)
    F = np.full(shape, 0.25, np.float32)
    M = np.full(shape, -0.5, np.float32)
    hist, count, _ = check(hip, F, M, None, bins, (-1.0, 1.0), (-1.0, 1.0), "linear", "one bin")
    assert np.count_nonzero(hist) == 1 and count == F.size
    F[1::TILE[0], 2::TILE[1], 5::TILE[2]] = -0.9
    M[2::TILE[0], 1::TILE[1], 70::TILE[2]] = 0.8
    hist, count, _ = check(hip, F, M, None, bins, (-1.0, 1.0), (-1.0, 1.0), "linear", "mixed")
    assert np.count_nonzero(hist) == 3
    field = np.zeros((3,) + shape, np.float32)
    check(hip, F, M, field, bins, (-1.0, 1.0), (-1.0, 1.0), "nearest", "mixed field")


def test_integer_content_gives_exact_moments_and_calls_repeat(hip):
    """integer-valued volumes under an integer shift: every term is an integer and every sum is below 2^53, so any
    order of adding them is exact"""
    fshape, mshape = (9, 20, 133), (11, 19, 140)
    rng = np.random.default_rng(4)
    F = rng.integers(-300, 300, fshape).astype(np.float32)
    M = rng.integers(-300, 300, mshape).astype(np.float32)
    A = np.eye(3, 4)
    A[:, 3] = [5, -2, 1]
    for T in (A, fr.ref_affine_field(A, fshape)):
        for interp in ("linear", "nearest"):
            check(hip, F, M, T, 64, (-300.0, 300.0), (-300.0, 300.0), interp, "integers %s" % interp, exact=True)
    Fg, Mg = volumes(fshape, mshape, 5)
    Fd, Md = dev(Fg), dev(Mg)
    R = about_center(rot((0, 1, 0), 12.0), mshape, fshape)
    runs = [hip.similarity(Fd, Md, R, 50, (-1.0, 1.5), (-1.0, 1.5)) for _ in range(2)]
    (h0, s0), (h1, s1) = runs
    assert np.array_equal(s0.cpu().numpy(), s1.cpu().numpy())              # the record's bytes
    assert np.array_equal(h0.cpu().numpy(), h1.cpu().numpy())


def test_caller_buffers_and_value_errors(hip):
    import torch
    F, M = (dev(v) for v in volumes((5, 7, 9), (6, 5, 8), 8))
    hist = torch.full((50, 50), 7, dtype=torch.int64, device="cuda")         # the call zeroes it
    work = torch.empty(hip.SIMILARITY_GRID * 56, dtype=torch.uint8, device="cuda")
    h, _ = hip.similarity(F, M, np.eye(3, 4), 50, (-1, 1.5), (-1, 1.5), hist=hist, work=work)
    assert h is hist
    want, _ = sr.joint(F.cpu().numpy(), M.cpu().numpy(), np.eye(3, 4), 50, (-1, 1.5), (-1, 1.5))
    np.testing.assert_array_equal(hist.cpu().numpy(), want.astype(np.int64))
    for bad in (lambda: hip.similarity(F, M, None, 50, (-1, 1), (-1, 1)),             # None needs equal shapes
                lambda: hip.similarity(F, M, np.eye(3), 50, (-1, 1), (-1, 1)),
                lambda: hip.similarity(F, M, np.eye(3, 4), 1, (-1, 1), (-1, 1)),
                lambda: hip.similarity(F, M, np.eye(3, 4), 129, (-1, 1), (-1, 1)),
                lambda: hip.similarity(F, M, np.eye(3, 4), 50, (-1, 1), (-1, 1), "cubic"),
                lambda: hip.similarity(F, M, torch.zeros((3, 5, 7, 8), device="cuda"), 50, (-1, 1), (-1, 1)),
                lambda: hip.similarity(F, M, np.eye(3, 4), 50, (-1, 1), (-1, 1), hist=hist[:49]),
                lambda: hip.similarity(F, M, np.eye(3, 4), 50, (-1, 1), (-1, 1), work=work[:100])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError):
        hip.similarity(F, M, np.eye(3, 4), 50, (1.0, 1.0), (-1, 1))                # an empty range: the entry refuses


def test_label_overlap_through_a_field(hip):
    from sift3d_amd import api
    shape = (9, 20, 70)
    rng = np.random.default_rng(11)
    z, y, x = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    lab_f = ((x // 15 + y // 6 + z // 4) % 5).astype(np.float32)
    lab_m = ((x // 14 + y // 7 + z // 4) % 5).astype(np.float32)
    field = rng.normal(0, 1.5, (3,) + shape).astype(np.float32)
    got = api.label_overlap(dev(lab_f), dev(lab_m), dev(field), 5)
    want, st = sr.joint(lab_f, lab_m, field, 5, (0.0, 5.0), (0.0, 5.0), "nearest")
    np.testing.assert_array_equal(got.confusion, want.astype(np.int64))
    assert 0 < st.count < lab_f.size and got.confusion.sum() == st.count
    dice, jac, vf, vm = sr.label_overlap(want)
    np.testing.assert_array_equal(got.dice, dice)
    np.testing.assert_array_equal(got.jaccard, jac)
    np.testing.assert_array_equal(got.volume_fixed, vf)
    np.testing.assert_array_equal(got.volume_moving, vm)
    auto = api.label_overlap(lab_f, lab_m, field)                           # host input, num_labels from the volumes
    np.testing.assert_array_equal(auto.confusion, got.confusion)
    same = api.label_overlap(dev(lab_f), dev(lab_f))
    np.testing.assert_array_equal(same.dice, 1.0)


def test_api_numpy_input_equals_tensor_path():
    from sift3d_amd import api
    F, M = volumes((5, 6, 70), (7, 6, 66), 21)
    A = about_center(rot((0, 0, 1), 8.0), M.shape, F.shape)
    a = api.similarity(dev(F), dev(M), A, 50)
    b = api.similarity(F, api.Image.from_array(M), A, 50)
    np.testing.assert_array_equal(a.joint, b.joint)
    assert a[:8] == b[:8]
    want, hist = sr.similarity(F, M, A, 50)                                  # own ranges: min and max
    np.testing.assert_array_equal(a.joint, hist.astype(np.int64))
    assert a.count == want.n
    t = api.similarity(dev(F), dev(M), api.TPS(np.zeros((5, 3)), np.zeros((5, 3)), A), 50)     # zero weights: the affine
    f = api.similarity(dev(F), dev(M), api.displacement_field(A, F.shape), 50)
    np.testing.assert_array_equal(t.joint, f.joint)
    c = api.similarity(np.full((3, 4, 5), 2.0, np.float32), np.full((3, 4, 5), 2.0, np.float32))   # constant volumes
    assert c.count == 60 and c.joint[0, 0] == 60 and c.ncc == 0.0 and c.mi == 0.0 and c.msd == 0.0


def test_end_to_end_registration_quality():
    """api.synth_survey(48); moving = fixed through a known rotation of 3 degrees plus a shift.  At the true transform
    ncc and mi exceed their values at the identity; with a non-monotone remap of the moving volume (|v - median|) mi
    over x shifts -3 .. 3 about the true transform peaks at 0, while ncc says nothing.  Measured on an MI355X, and the
    same to the printed digits on the restatement (tests/test_similarity_host.py): true: ncc 0.9893 mi 2.3330;
    identity: ncc 0.8755 mi 0.8958; remapped mi 0.4048 0.6247 1.0349 1.8601 1.0991 0.6711 0.4349, ncc -0.1096 -0.1044
    -0.1072 -0.1146 -0.1171 -0.1082 -0.0964."""
    import torch
    from sift3d_amd import api, hip
    fixed, T, Tinv = end_to_end_case(api)
    Fd = dev(fixed)
    Md = torch.empty_like(Fd)
    hip.warp_affine(Fd, Md, Tinv, "linear", 0.0)
    at_true, at_ident = api.similarity(Fd, Md, T), api.similarity(Fd, Md)
    print("true: ncc %.4f mi %.4f; identity: ncc %.4f mi %.4f" % (at_true.ncc, at_true.mi, at_ident.ncc, at_ident.mi))
    assert at_true.ncc > at_ident.ncc and at_true.mi > at_ident.mi
    remap = (Md - Md.median()).abs()
    rows = [api.similarity(Fd, remap, shifted(T, dx)) for dx in range(-3, 4)]
    mi, ncc = [r.mi for r in rows], [r.ncc for r in rows]
    print("remapped, dx -3 .. 3: mi", " ".join("%.4f" % v for v in mi), "ncc", " ".join("%.4f" % v for v in ncc))
    assert int(np.argmax(mi)) == 3
    want, hist = sr.similarity(fixed, remap.cpu().numpy(), T)
    np.testing.assert_array_equal(rows[3].joint, hist.astype(np.int64))
    assert abs(rows[3].mi - want.mi) <= measure_bounds(hist)[3]             # the same histogram: the host test's bound
