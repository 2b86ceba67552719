"""CPU (not gpu): the distance contract (include/sift3d_amd.h, "Distance transforms and surface distances") without a
device.  The numpy restatement (tests/distance_restatement.py) against scipy.ndimage.distance_transform_edt, the host
entry sift3d_amd_surface_measures against the restatement and numpy.percentile, every argument refusal of the device
entries (which check their arguments before any device call), both work_bytes functions and the Python errors.

Tolerances.  u = 2^-24 (float32).  The restatement's D2 is a minimum of c = ((w_x * a) + (w_y * b)) + (w_z * c'), every
term non-negative.  Each term carries the rounding of its weight and of its product, (1 + u)^2, so at most 2u relative;
the two additions add u each; all of it on non-negative values: c is within (1 + u)^4 - 1 < 5u relative of the real
sum, and a minimum of values that are each within 5u of their real counterparts is within 5u of the real minimum.
scipy's double result squared is exact to 2^-52 beside that.  With unit spacing every value is an integer below 2^24:
equal.  The measures are IEEE double operations in one order in C and in numpy: equal bits.  numpy.percentile
evaluates the same linear interpolation in another form (from the upper neighbour when the fraction is >= 0.5): the
header's form rounds the difference, the product and the sum, numpy's the difference, 1 - t, the product and the
subtraction, each on values no larger than the largest distance, so |difference| <= 8 * 2^-53 * max d."""
import ctypes as C

import numpy as np
import pytest

from tests import distance_restatement as dr

U = 2.0 ** -24


@pytest.fixture(scope="module")
def api():
    from sift3d_amd import api as a
    a.lib()
    return a


# ---- the restatement against scipy ---------------------------------------------------------------------------------
def random_mask(shape, density, seed):
    return (np.random.default_rng(seed).uniform(0, 1, shape) < density).astype(np.float32)


@pytest.mark.parametrize("spacing", [(1.0, 1.0, 1.0), (0.7, 1.3, 2.5), (1.0, 1.0, 100.0), (1e-3, 1.0, 1e3)])
@pytest.mark.parametrize("density", [0.02, 0.5])
def test_restatement_against_scipy(spacing, density):
    ndi = pytest.importorskip("scipy.ndimage")
    mask = random_mask((13, 17, 20), density, 7)
    got = dr.distance_sq(mask, spacing).astype(np.float64)
    want = ndi.distance_transform_edt(~(mask >= 0.5), sampling=spacing[::-1]).astype(np.float64) ** 2
    rel = np.abs(got - want) / np.maximum(want, 1e-300)
    rel[want == 0] = np.abs(got[want == 0])
    print("spacing %s density %g: max relative difference %.3g (bound %.3g)" % (spacing, density, rel.max(), 5 * U))
    assert rel.max() <= 5 * U
    if spacing == (1.0, 1.0, 1.0):
        np.testing.assert_array_equal(got, np.rint(want))
    inv = dr.distance_sq(mask, spacing, invert=True).astype(np.float64)
    want = ndi.distance_transform_edt(mask >= 0.5, sampling=spacing[::-1]).astype(np.float64) ** 2
    assert (np.abs(inv - want) <= 5 * U * want).all()


def test_restatement_edges():
    empty = np.zeros((2, 3, 4), np.float32)
    assert np.isposinf(dr.distance_sq(empty)).all() and np.isposinf(dr.distance_signed(empty)).all()
    assert (dr.distance_sq(empty + 1) == 0).all() and np.isneginf(dr.distance_signed(empty + 1)).all()
    m = np.array([[[np.nan, np.nextafter(np.float32(0.5), np.float32(0)), 0.5, np.inf]]], np.float32)
    np.testing.assert_array_equal(dr.mask_in(m).ravel(), [False, False, True, True])
    np.testing.assert_array_equal(dr.distance_sq(m, (3.0, 1.0, 1.0)).ravel(), [36.0, 9.0, 0.0, 0.0])
    np.testing.assert_array_equal(dr.distance_signed(m, (3.0, 1.0, 1.0)).ravel(), [6.0, 3.0, -3.0, -6.0])
    lab = np.zeros((4, 5, 6), np.float32)
    lab[1:4, 1:5, 1:5] = 2                                   # touches the far z and y faces
    surf, n = dr.label_surface(lab, 2)
    assert n == int(surf.sum()) and surf[2, 2, 2] == 0 and surf[3, 2, 2] == 1 and surf[2, 4, 2] == 1
    assert dr.label_surface(lab, 5)[1] == 0
    full, n = dr.label_surface(np.full((3, 3, 3), 1, np.float32), 1)
    assert n == 26 and full[1, 1, 1] == 0


# ---- the host measures against the restatement ------------------------------------------------------------------------
def sorted_list(n, seed, ties=False):
    rng = np.random.default_rng(seed)
    d = np.sqrt(rng.integers(0, 30 if ties else 100000, n).astype(np.float32))
    return np.sort(d).astype(np.float32)


def same_bits(a, b):
    return np.array(a, np.float64).tobytes() == np.array(b, np.float64).tobytes()


@pytest.mark.parametrize("n_f,n_m,ties", [(1, 1, False), (1, 7, False), (20, 21, False), (400, 333, True),
                                          (5000, 4000, False), (2, 2, True)])
def test_surface_measures_entry_equals_restatement(api, n_f, n_m, ties):
    a, b = sorted_list(n_f, n_f, ties), sorted_list(n_m, 1000 + n_m, ties)
    got, want = api.surface_measures(a, b), dr.measures(a, b)
    print(got)
    assert (got.n_fixed, got.n_moving) == (n_f, n_m)
    assert same_bits(got[:7], want[:7]), (got, want)
    pooled = np.concatenate([a, b]).astype(np.float64)
    ref = float(np.percentile(pooled, 95))
    assert abs(got.hd95 - ref) <= 8 * 2.0 ** -53 * float(pooled.max()), (got.hd95, ref)
    assert got.hausdorff == float(pooled.max()) and got.max_fm == float(a[-1]) and got.max_mf == float(b[-1])


def test_surface_measures_entry_edge_cases(api):
    some, none = np.array([1.0, 2.0], np.float32), np.zeros(0, np.float32)
    for a, b in ((none, some), (some, none), (none, none)):
        got = api.surface_measures(a, b)
        assert (got.n_fixed, got.n_moving) == (len(a), len(b)) and all(np.isnan(v) for v in got[:7])
    one = api.surface_measures([3.0], [5.0])                 # n = 2: pos = 0.95, between the two
    assert one.hausdorff == 5.0 and one.hd95 == 3.0 + 0.95 * 2.0 and one.assd == 4.0
    assert (one.mean_fm, one.mean_mf, one.max_fm, one.max_mf) == (3.0, 5.0, 3.0, 5.0)
    tie = api.surface_measures([2.0] * 10, [2.0] * 10)
    assert tie[:7] == (2.0,) * 7
    raw = api.lib()["sift3d_amd_surface_measures"]
    raw.restype, raw.argtypes = C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    out = (C.c_double * 9)()
    assert raw(some.ctypes.data, 2, some.ctypes.data, 2, None) == -1
    assert raw(None, 2, some.ctypes.data, 2, out) == -1 and raw(some.ctypes.data, 2, None, 1, out) == -1
    assert raw(None, 0, None, 0, out) == 0 and raw(some.ctypes.data, 2, some.ctypes.data, 2, out) == 0


# ---- the device entries refuse bad arguments before any device call --------------------------------------------
@pytest.fixture(scope="module")
def bufs(api):
    """made-up addresses without a device; real allocations covering every range named below with one"""
    from sift3d_amd import hip
    if api.device_available():
        b = [hip.lib().sift3d_hip_malloc(1 << 18) for _ in range(4)]
        assert all(b)
        yield b
        for p in b:
            hip.lib().sift3d_hip_free(p)
    else:
        yield [0x1000000 * (k + 1) for k in range(4)]


NAMES = ("sift3d_amd_distance_work_bytes", "sift3d_hip_distance_sq", "sift3d_hip_distance",
         "sift3d_hip_distance_signed", "sift3d_hip_label_surface", "sift3d_hip_surface_collect",
         "sift3d_amd_surface_distances_work_bytes", "sift3d_amd_surface_distances_device", "sift3d_amd_surface_measures")


def test_symbols_exported_and_declared(api):
    import os
    from sift3d_amd import _native, hip
    L = _native.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "sift3d_amd.h")).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name + "(" in header, name
    for f in (hip.distance, hip.label_surface, hip.surface_collect, hip.surface_distances, api.distance_transform,
              api.surface_distances, api.surface_measures):
        assert callable(f)
    assert api.SurfaceDistances._fields == ("hausdorff", "hd95", "assd", "mean_fm", "mean_mf", "max_fm", "max_mf",
                                            "n_fixed", "n_moving", "labels")
    assert C.sizeof(hip.SurfaceResult) == 72


def test_work_bytes(api):
    from sift3d_amd import hip
    W, S = hip.lib().sift3d_amd_distance_work_bytes, hip.lib().sift3d_amd_surface_distances_work_bytes
    assert W(5, 6, 7) == 2 * 4 * 210 and W(4096, 1, 1) == 2 * 4 * 4096 and W(4096, 4096, 4096) == 2 * 4 * 4096 ** 3
    assert S(5, 6, 7) == 5 * 4 * 210 + 32 and S(3, 3, 3) == 5 * 4 * 27 + 4 + 32      # rounded up to 8, then 4 counters
    for f in (W, S):
        for bad in ((0, 6, 7), (5, -1, 7), (5, 6, 0), (4097, 6, 7), (5, 4097, 7), (5, 6, 4097)):
            assert f(*bad) == 0, bad


def _sp(v):
    a = np.ascontiguousarray(v, np.float64)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


BAD_DIMS = [(0, 8, 8), (8, -1, 8), (8, 8, 0), (4097, 8, 8), (8, 4097, 8), (8, 8, 4097)]
BAD_SPACINGS = [(np.nan, 1, 1), (1, np.inf, 1), (1, 1, -np.inf), (0.0, 1, 1), (1, -1.0, 1), (1, 1, 9e-7), (1.1e6, 1, 1)]
VOL = 4 * 512                                                # bytes of an 8 x 8 x 8 volume


def test_transform_refusals(bufs):
    """sift3d_hip_distance_sq, sift3d_hip_distance and sift3d_hip_distance_signed: (mask, dims, spacing, [invert],
    out, work)"""
    from sift3d_amd import hip
    L = hip.lib()
    M, O, W, _ = bufs
    keep, unit = _sp((1.0, 1.0, 1.0))
    entries = [(L.sift3d_hip_distance_sq, True, 1), (L.sift3d_hip_distance, True, 1),
               (L.sift3d_hip_distance_signed, False, 2)]
    for fn, has_invert, work_vols in entries:
        def call(M=M, dims=(8, 8, 8), sp=unit, O=O, W=W):
            return fn(M, *dims, sp, *((0,) if has_invert else ()), O, W, None)
        assert call(M=None) == -1 and call(O=None) == -1 and call(W=None) == -1
        for d in BAD_DIMS:
            assert call(dims=d) == -1, d
        for s in BAD_SPACINGS:
            kept, bad = _sp(s)
            assert call(sp=bad) == -1, s
        assert call(M=M + 2) == -1 and call(O=O + 1) == -1 and call(W=W + 3) == -1            # misaligned
        assert call(O=M) == -1 and call(O=M + VOL - 4) == -1 and call(W=M + 4) == -1          # outputs on the input
        assert call(W=O) == -1 and call(O=W + work_vols * VOL - 4) == -1                      # out on the work buffer
        assert call(W=M - work_vols * VOL + 4) == -1                                          # its last float on the mask


def test_label_surface_refusals(bufs):
    from sift3d_amd import hip
    fn = hip.lib().sift3d_hip_label_surface
    Lb, S, Cn, _ = bufs

    def call(Lb=Lb, dims=(8, 8, 8), S=S, Cn=Cn):
        return fn(Lb, *dims, 1, S, Cn, None)
    assert call(Lb=None) == -1 and call(S=None) == -1 and call(Cn=None) == -1
    for d in BAD_DIMS:
        assert call(dims=d) == -1, d
    assert call(Lb=Lb + 2) == -1 and call(S=S + 1) == -1 and call(Cn=Cn + 4) == -1            # the counter: 8 bytes
    assert call(S=Lb) == -1 and call(S=Lb + VOL - 4) == -1 and call(Cn=Lb + 8) == -1
    assert call(Cn=S + VOL - 8) == -1 and call(S=Cn - VOL + 4) == -1


def test_surface_collect_refusals(bufs):
    from sift3d_amd import hip
    fn = hip.lib().sift3d_hip_surface_collect
    S, D, Li, Cn = bufs

    def call(S=S, D=D, n=512, Li=Li, cap=100, Cn=Cn):
        return fn(S, D, n, Li, cap, Cn, None)
    assert call(S=None) == -1 and call(D=None) == -1 and call(Li=None) == -1 and call(Cn=None) == -1
    assert call(n=0) == -1 and call(n=4096 ** 3 + 1) == -1 and call(cap=4096 ** 3 + 1) == -1
    assert call(S=S + 2) == -1 and call(D=D + 1) == -1 and call(Li=Li + 3) == -1 and call(Cn=Cn + 4) == -1
    assert call(Li=S) == -1 and call(Li=D + VOL - 4) == -1 and call(Li=S - 4 * 100 + 4) == -1
    assert call(Cn=S + 8) == -1 and call(Cn=D + VOL - 8) == -1 and call(Cn=Li + 4 * 100 - 8) == -1


def test_surface_distances_driver_refusals(bufs):
    from sift3d_amd import hip
    fn = hip.lib().sift3d_amd_surface_distances_device
    F, M, W, _ = bufs
    keep, unit = _sp((1.0, 1.0, 1.0))
    lab = np.array([1, 2], np.int32)
    labp = lab.ctypes.data_as(C.POINTER(C.c_int))
    many = np.arange(129, dtype=np.int32)
    res = (hip.SurfaceResult * 129)()
    work = 5 * VOL + 32

    def call(F=F, M=M, dims=(8, 8, 8), labels=labp, n=2, sp=unit, res=res, W=W):
        return fn(F, M, *dims, labels, n, sp, res, W, None)
    assert call(F=None) == -1 and call(M=None) == -1 and call(labels=None) == -1 and call(res=None) == -1
    assert call(W=None) == -1
    for d in BAD_DIMS:
        assert call(dims=d) == -1, d
    for s in BAD_SPACINGS:
        kept, bad = _sp(s)
        assert call(sp=bad) == -1, s
    assert call(n=0) == -1 and call(n=-1) == -1
    assert call(labels=many.ctypes.data_as(C.POINTER(C.c_int)), n=129) == -1
    assert call(F=F + 2) == -1 and call(M=M + 1) == -1 and call(W=W + 4) == -1                # the work buffer: 8 bytes
    assert call(W=F) == -1 and call(W=M + VOL - 8) == -1 and call(W=F - work + 8) == -1


# ---- the Python layer ---------------------------------------------------------------------------------------------
def test_python_value_errors(api):
    v = np.zeros((5, 7, 9), np.float32)
    with pytest.raises(ValueError):
        api.surface_distances(v, np.zeros((5, 7, 8), np.float32))            # shapes differ, no transform
    for bad in ((1.0, 1.0), (0.0, 1.0, 1.0), (1.0, np.nan, 1.0), (1.0, 1.0, 2e6), (-1.0, 1.0, 1.0)):
        with pytest.raises(ValueError):
            api.distance_transform(v, spacing=bad)
        with pytest.raises(ValueError):
            api.surface_distances(v, v, spacing=bad)
    with pytest.raises(ValueError):
        api.distance_transform(np.zeros((7, 9), np.float32))
    with pytest.raises(ValueError):
        api.distance_transform(v, signed=True, squared=True)
    with pytest.raises(ValueError):
        api.distance_transform(v, signed=True, invert=True)
    with pytest.raises(ValueError):
        api.distance_transform(v.astype(np.complex64))
    with pytest.raises(ValueError):
        api.surface_distances(v, v, labels=[])
    with pytest.raises(ValueError):
        api.surface_distances(v, v, labels=[1.5])
    if not api.device_available():
        with pytest.raises(RuntimeError):
            api.distance_transform(v)
        with pytest.raises(RuntimeError):
            api.surface_distances(v, v)
