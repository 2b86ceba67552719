"""CPU (not gpu): the host side of the displacement fields -- every refusal of the device entries and of the
blocking host forms, which check their arguments before any device call; the exported symbols; and the
restatement (tests/field_restatement.py) against itself and numpy.gradient."""
import ctypes as C

import numpy as np
import pytest

from tests import field_restatement as fr
from tests import tps_restatement as tr


@pytest.fixture(scope="module")
def api():
    from sift3d_amd import api as a
    a.lib()
    return a


@pytest.fixture(scope="module")
def bufs(api):
    """made-up addresses without a device; real allocations covering every range named below with one, so
    that a regressed check could not make a kernel touch unmapped memory"""
    from sift3d_amd import hip
    if api.device_available():
        b = [hip.lib().sift3d_hip_malloc(1 << 16) for _ in range(3)]
        assert all(b)
        yield b
        for p in b:
            hip.lib().sift3d_hip_free(p)
    else:
        yield [0x100000, 0x900000, 0x1100000]


EXPORTED = ["sift3d_hip_affine_field", "sift3d_hip_tps_field", "sift3d_hip_tps_field_launches",
            "sift3d_hip_warp_field", "sift3d_hip_jacobian_det", "sift3d_amd_image_warp_field",
            "sift3d_amd_jacobian_det"]


def test_symbols_exported(api):
    from sift3d_amd import _native, hip
    L = _native.load()
    for name in EXPORTED:
        assert hasattr(L, name), name
    hip.lib()
    for name in ("affine_field", "tps_field", "tps_field_launches", "warp_field", "jacobian_det"):
        assert callable(getattr(hip, name))
    for name in ("displacement_field", "warp_field", "jacobian_determinant"):
        assert callable(getattr(api, name))
    assert api.JacobianStats._fields == ("det", "folded", "min", "max")


def _a(A):
    a = np.ascontiguousarray(A, np.float64).reshape(12)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def test_affine_field_refusals(bufs):
    from sift3d_amd import hip
    F = bufs[0]
    L = hip.lib()
    keep, ident = _a(tr.IDENT)
    assert L.sift3d_hip_affine_field(None, 8, 8, 8, ident, None) == -1
    assert L.sift3d_hip_affine_field(F, 8, 8, 8, None, None) == -1
    for dims in ((0, 8, 8), (8, -1, 8), (8, 8, 0)):
        assert L.sift3d_hip_affine_field(F, *dims, ident, None) == -1
    for v in (np.nan, np.inf, -np.inf):
        A = tr.IDENT.copy()
        A[1, 3] = v
        k2, ap = _a(A)
        assert L.sift3d_hip_affine_field(F, 8, 8, 8, ap, None) == -1


def test_tps_field_refusals(bufs):
    from sift3d_amd import hip
    F, T, _ = bufs
    L = hip.lib()
    keep, ident = _a(tr.IDENT)
    cases = [(None, 8, 8, 8, ident, T, 4), (F, 8, 8, 8, None, T, 4), (F, 8, 8, 8, ident, None, 4),
             (F, 0, 8, 8, ident, T, 4), (F, 8, 8, -2, ident, T, 4),
             (F, 8, 8, 8, ident, T, 0), (F, 8, 8, 8, ident, T, 16385),
             (F, 8, 8, 8, ident, T + 4, 4),                              # misaligned records
             (F, 8, 8, 8, ident, F + 4 * 64, 4),                         # records inside the field
             (T, 8, 8, 8, ident, T + 6128, 4)]                           # the field's end holds the records
    for v in (np.nan, np.inf):
        A = tr.IDENT.copy()
        A[0, 0] = v
        cases.append((F, 8, 8, 8, _a(A)[1], T, 4))
    for c in cases:
        assert L.sift3d_hip_tps_field(*c, None) == -1, c
    assert hip.tps_field_launches((8, 8, 8), 0) == -1
    assert hip.tps_field_launches((0, 8, 8), 4) == -1
    assert hip.tps_field_launches((29, 31, 7), 1000) == 1
    for m in (256, 1024, 16384):
        assert hip.tps_field_launches((512, 512, 512), m) == hip.warp_tps_launches((512, 512, 512), m)


def test_warp_field_refusals(bufs):
    from sift3d_amd import hip
    S, F, D = bufs
    L = hip.lib()
    cases = [
        (None, 8, 8, 8, 1, F, 8, 8, 8, D, 1),
        (S, 8, 8, 8, 1, None, 8, 8, 8, D, 1),
        (S, 8, 8, 8, 1, F, 8, 8, 8, None, 1),
        (S, 0, 8, 8, 1, F, 8, 8, 8, D, 1),
        (S, 8, 8, 8, 1, F, 8, -1, 8, D, 1),
        (S, 8, 8, 8, 0, F, 8, 8, 8, D, 1),                              # nc < 1
        (S, 8, 8, 8, -3, F, 8, 8, 8, D, 0),
        (S, 8, 8, 8, 1, F, 8, 8, 8, D, 2),                              # unknown interp
        (S, 8, 8, 8, 1, F, 8, 8, 8, D, -1),
        (S + 2, 8, 8, 8, 1, F, 8, 8, 8, D, 1),                          # misaligned
        (S, 8, 8, 8, 1, F + 1, 8, 8, 8, D, 1),
        (S, 8, 8, 8, 1, F, 8, 8, 8, D + 2, 1),
        (S, 8, 8, 8, 1, F, 8, 8, 8, S, 1),                              # dst is src
        (S, 8, 8, 8, 2, F, 8, 8, 8, S + 4 * 1000, 1),                   # dst inside src's second channel
        (S, 8, 8, 8, 1, F, 8, 8, 8, F + 4 * 1500, 1),                   # dst inside the field's last channel
        (S, 8, 8, 8, 3, F + 4 * 1500, 8, 8, 8, F, 0),                   # dst's last channel runs into the field
    ]
    for c in cases:
        assert L.sift3d_hip_warp_field(*c, 0.0, None) == -1, c


def test_jacobian_refusals(bufs):
    from sift3d_amd import hip
    F, D, T = bufs
    L = hip.lib()
    cases = [(None, 8, 8, 8, D, T), (F, 8, 8, 8, D, None), (F, 0, 8, 8, D, T), (F, 8, 8, -1, None, T),
             (F, 8, 8, 8, D, T + 4),                                    # stats not 8-byte aligned
             (F + 2, 8, 8, 8, D, T), (F, 8, 8, 8, D + 2, T),
             (F, 8, 8, 8, F + 4 * 100, T),                              # det inside the field
             (F, 8, 8, 8, D, F + 4 * 1534),                             # stats inside the field
             (F, 8, 8, 8, D, D + 4 * 10)]                               # stats inside det
    for c in cases:
        assert L.sift3d_hip_jacobian_det(*c, None) == -1, c


def _native_fn(name):
    from sift3d_amd import _native
    fn = _native.load()[name]                           # a function object of its own: argtypes set here only
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return fn


def test_host_form_refusals(api):
    L = api.lib()
    src, dst = api.Image(9, 7, 5), api.Image(6, 6, 6)
    two = api.Image(9, 7, 5, 2)
    field = np.zeros(3 * 216, np.float32)
    assert L.sift3d_amd_image_warp_field(None, field, 1, 0.0, dst.h) == -1
    assert L.sift3d_amd_image_warp_field(src.h, field, 1, 0.0, None) == -1
    assert L.sift3d_amd_image_warp_field(two.h, field, 1, 0.0, dst.h) == -1
    assert L.sift3d_amd_image_warp_field(src.h, field, 1, 0.0, two.h) == -1
    assert L.sift3d_amd_image_warp_field(src.h, field, 3, 0.0, dst.h) == -1
    assert L.sift3d_amd_image_warp_field(src.h, field, -1, 0.0, dst.h) == -1
    assert L.sift3d_amd_image_warp_field(dst.h, field, 1, 0.0, dst.h) == -1       # dst is src
    # a field that holds dst's data
    data = api.lib().sift3d_image_data(dst.h)
    addr = C.cast(data, C.c_void_p).value
    F32 = C.c_float * (3 * 216)
    alias = np.ctypeslib.as_array(F32.from_address(addr - 4 * 216))
    assert L.sift3d_amd_image_warp_field(src.h, alias, 1, 0.0, dst.h) == -1
    folded, mn, mx = C.c_uint64(7), C.c_float(7), C.c_float(7)
    fa = np.zeros(3 * 60, np.float32)
    det = np.zeros(60, np.float32)
    J = _native_fn("sift3d_amd_jacobian_det")                          # raw pointers: NULL field included
    f = fa.ctypes.data
    assert J(None, 3, 4, 5, det.ctypes.data, C.byref(folded), C.byref(mn), C.byref(mx)) == -1
    assert J(f, 3, 4, 5, det.ctypes.data, None, C.byref(mn), C.byref(mx)) == -1
    assert J(f, 3, 4, 5, det.ctypes.data, C.byref(folded), None, C.byref(mx)) == -1
    assert J(f, 3, 4, 5, det.ctypes.data, C.byref(folded), C.byref(mn), None) == -1
    assert J(f, 0, 4, 5, det.ctypes.data, C.byref(folded), C.byref(mn), C.byref(mx)) == -1
    assert J(f, 3, -4, 5, None, C.byref(folded), C.byref(mn), C.byref(mx)) == -1
    assert J(f, 3, 4, 5, f + 4 * 100, C.byref(folded), C.byref(mn), C.byref(mx)) == -1
    assert (folded.value, mn.value, mx.value) == (7, 7.0, 7.0)                   # nothing written
    with pytest.raises(ValueError):
        api.warp_field(np.zeros((5, 7, 9), np.float32), np.zeros((2, 6, 6, 6), np.float32))
    with pytest.raises(ValueError):
        api.warp_field(np.zeros((5, 7, 9), np.float32), np.zeros((3, 6, 6, 6), np.float32), interp="cubic")
    with pytest.raises(ValueError):
        api.jacobian_determinant(np.zeros((4, 6, 6, 6), np.float32))
    if not api.device_available():
        with pytest.raises(RuntimeError):
            api.warp_field(np.zeros((5, 7, 9), np.float32), np.zeros((3, 6, 6, 6), np.float32))
        with pytest.raises(RuntimeError):
            api.jacobian_determinant(np.zeros((3, 6, 6, 6), np.float32))


# ---- the restatement against itself --------------------------------------------------------------------------
def test_restated_gradient_is_numpy_gradient():
    rng = np.random.default_rng(1)
    for shape in ((2, 3, 5), (7, 2, 9), (4, 6, 2)):
        u = rng.normal(0, 3, shape).astype(np.float32)
        for axis in range(3):
            want = np.gradient(u, axis=axis)
            assert want.dtype == np.float32
            np.testing.assert_array_equal(fr.ref_gradient(u, axis), want)
    u = rng.normal(0, 1, (1, 4, 5)).astype(np.float32)
    assert not fr.ref_gradient(u, 0).any()                              # an axis of length 1: no gradient
    e = fr.ref_gradient(np.array([[[1.0, 4.0]]], np.float32), 2)        # length 2: both ends one-sided
    np.testing.assert_array_equal(e, [[[3.0, 3.0]]])


def test_restated_identity_and_affine_determinants():
    for O in ((1, 1, 1), (2, 1, 3), (5, 6, 7)):
        det = fr.ref_jacobian_det(np.zeros((3,) + O, np.float32))
        assert (det == 1.0).all() and fr.ref_stats(det) == (0, 1.0, 1.0)
    A = np.array([[1.1, 0.2, -0.1, 3.0], [0.05, 0.9, 0.3, -2.0], [-0.2, 0.1, 1.3, 0.5]])
    for O in ((4, 5, 6), (2, 2, 2), (9, 3, 2)):
        det = fr.ref_jacobian_det(fr.ref_affine_field(A, O))
        assert np.abs(det - np.linalg.det(A[:, :3])).max() <= 1e-5
    # an axis of length 1 has no gradient: j = 1 along it, so a z-stretch is invisible on one plane
    S = np.diag([1.0, 1.0, 2.0])
    det = fr.ref_jacobian_det(fr.ref_affine_field(np.hstack([S, np.zeros((3, 1))]), (1, 4, 4)))
    assert (det == 1.0).all()
    det = fr.ref_jacobian_det(fr.ref_affine_field(np.hstack([S, np.zeros((3, 1))]), (2, 4, 4)))
    assert (det == 2.0).all()


def test_restated_stats():
    d = np.array([1.0, -0.5, 0.0, -0.0, np.nan, 2.5], np.float32)
    folded, mn, mx = fr.ref_stats(d)
    assert folded == 4 and mn == -0.5 and mx == 2.5
    assert fr.ref_stats(np.full(3, np.nan, np.float32)) == (3, np.inf, -np.inf)


def test_restated_export_and_warp():
    """the TPS export with zero weights is the affine export; an exact field warps like the affine warp"""
    from sift3d_amd import api
    A = np.array([[0, 0, -1.0, 10.0], [1.0, 0, 0, 2.0], [0, -1.0, 0, 12.0]])
    O = (6, 7, 8)
    t = api.TPS(np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 1.0]]), np.zeros((2, 3)), A)
    np.testing.assert_array_equal(fr.ref_tps_field(t, O).view(np.uint32), fr.ref_affine_field(A, O).view(np.uint32))
    from tests.test_warp import ref_warp
    src = np.random.default_rng(3).normal(0, 1, (11, 13, 12)).astype(np.float32)
    for interp in ("linear", "nearest"):
        got = fr.ref_warp_field(src, fr.ref_affine_field(A, O), interp, -1.0)
        np.testing.assert_array_equal(got, ref_warp(src, A, O, interp, -1.0)[0])
        many = fr.ref_warp_field(np.stack([src, 2 * src]), fr.ref_affine_field(A, O), interp, -1.0)
        np.testing.assert_array_equal(many[0], got)
