"""CPU (not gpu): the cubic B-spline contract (include/sift3d_amd.h, "Cubic B-spline resampling") without a device.
The numpy restatement (tests/bspline_restatement.py) against scipy.ndimage in float64 to derived bounds, its
properties, the round-trip quality case, and every argument refusal of the new entries, which check their arguments
before any device call."""
import ctypes as C

import numpy as np
import pytest
import scipy.ndimage as ndi

from tests import bspline_restatement as br
from tests.test_warp import about_center, ref_inside, ref_warp, rot

U = 2.0 ** -24                                          # float32 unit roundoff
GAIN = 3.0                                              # sum |h| per axis: sqrt(3) (1 + |z1|) / (1 - |z1|)
Z1 = 2.0 - np.sqrt(3.0)
TAIL = 2 * np.sqrt(3.0) * Z1 ** (br.H + 1) / (1 - Z1)   # dropped taps per axis, relative to max|s|

# shapes [nz, ny, nx]: axes of 1, 2, 3, below H, odd, and past H
SHAPES = [(1, 1, 1), (1, 1, 7), (1, 5, 1), (4, 1, 1), (2, 2, 2), (3, 3, 3), (2, 3, 5), (1, 9, 20), (5, 7, 9),
          (15, 16, 17), (9, 20, 33), (19, 35, 41)]


def prefilter_bound(m, axes):
    """|restated coefficients - exact coefficients| for max|s| = m over `axes` filtered axes.  One pass: 17 adds
    into the accumulator, the pair add, the product and the rounding of the tap, each at most U relative, on terms
    whose absolute sum is at most GAIN * max|input|: eps * GAIN * max|input| with eps = (H + 4) U.  A later pass
    multiplies the error it inherits by at most GAIN and adds its own on an input GAIN times larger, so after k passes
    k * eps * GAIN^k * m (27 for three axes); the dropped tail adds TAIL * max|input| per pass in the same way."""
    eps = (br.H + 4) * U
    return axes * (eps + TAIL) * GAIN ** axes * m * (1 + eps) ** axes


def sample_bound(cmax):
    """|restated sample - exact cubic B-spline| for coefficients up to cmax.  Per axis one dot of 4 terms with
    non-negative weights that sum to 1: each weight carries at most 5 U relative (its four or five operations), the
    product 1, the three adds 3, so 9 U * cmax per axis and 27 U * cmax for three.  The fraction f = (float)(q - i)
    is off by at most U / 2, and the interpolant's slope per axis is at most max|c[k] - c[k-1]| <= 2 cmax:
    3 * 2 * cmax * U / 2 = 3 U * cmax more."""
    return (27 + 3) * U * cmax


def volume(shape, seed, scale=10.0):
    return np.random.default_rng(seed).normal(0, scale, shape).astype(np.float32)


# ---- the restatement against scipy ----------------------------------------------------------------------------
def test_taps_are_the_closed_form():
    z1 = np.sqrt(3.0) - 2.0
    want = (np.sqrt(3.0) * z1 ** np.arange(br.H + 1)).astype(np.float32)
    np.testing.assert_array_equal(br.TAPS, want)
    assert TAIL < 2.0 ** -25 / 30                       # the header's claim: a thirtieth of half an ulp
    assert abs(float(br.C6) - 1 / 6) < U and abs(float(br.C23) - 2 / 3) < U


@pytest.mark.parametrize("shape", SHAPES)
def test_restated_prefilter_is_scipys(shape):
    v = volume(shape, sum(shape))
    got = br.prefilter(v)
    want = ndi.spline_filter(v.astype(np.float64), order=3, mode="mirror", output=np.float64)
    axes = sum(n > 1 for n in shape)
    err = np.abs(got.astype(np.float64) - want).max()
    bound = prefilter_bound(float(np.abs(v).max()), axes)
    print("prefilter", shape, "err %.3g bound %.3g" % (err, bound))
    assert err <= bound
    if axes == 0:
        np.testing.assert_array_equal(got, v)           # an axis of 1 is the identity


def test_prefilter_channels_and_lines():
    v = volume((3, 5, 18, 21), 7)
    c = br.prefilter(v)
    for k in range(3):
        np.testing.assert_array_equal(c[k], br.prefilter(v[k]))
    for axis, fixed in ((0, (0, 3, 20)), (1, (4, 0, 0)), (2, (2, 17, 0))):
        idx = list(fixed)
        idx[axis] = slice(None)
        np.testing.assert_array_equal(br.prefilter_line(v[1], axis, fixed), c[1][tuple(idx)])


def face_points(shape, rng):
    """points on and just past every face, at corners, inside, and NaNs: (qx, qy, qz) float64"""
    nz, ny, nx = shape
    hi = np.array([nx - 1, ny - 1, nz - 1], np.float64)
    pts = [rng.uniform(0, 1, (200, 3)) * hi]            # inside
    for d in range(3):
        for face, past in ((0.0, -1e-9), (hi[d], hi[d] + 1e-9), (0.0, -0.5), (hi[d], hi[d] + 0.5)):
            p = rng.uniform(0, 1, (12, 3)) * hi
            p[:, d] = face
            pts.append(p)
            p = p.copy()
            p[:, d] = past if hi[d] > 0 or past < 0 else 1e-9
            pts.append(p)
    corners = np.array([[a, b, c] for a in (0, hi[0]) for b in (0, hi[1]) for c in (0, hi[2])])
    pts.append(corners)
    pts.append(np.floor(rng.uniform(0, 1, (40, 3)) * (hi + 1)).clip(0, hi))       # grid points
    nan = rng.uniform(0, 1, (6, 3)) * hi
    nan[np.arange(6), np.arange(6) % 3] = np.nan
    pts.append(nan)
    p = np.concatenate(pts)
    return p[:, 0], p[:, 1], p[:, 2]


@pytest.mark.parametrize("shape", SHAPES)
def test_restated_sample_is_scipys(shape):
    rng = np.random.default_rng(100 + sum(shape))
    c = volume(shape, 3 * sum(shape))                   # any array serves as coefficients
    q = face_points(shape, rng)
    flat = c.reshape(-1)
    got, ins = br.sample_points(lambda k: flat[k], shape, q, fill=-7.0)
    np.testing.assert_array_equal(ins, ref_inside(q, shape))
    assert (got[~ins] == -7.0).all() and not ins[-6:].any()               # the NaNs are outside
    qi = [v[ins] for v in q]
    want = ndi.map_coordinates(c.astype(np.float64), [qi[2], qi[1], qi[0]], order=3, mode="mirror", prefilter=False)
    err = np.abs(got[ins].astype(np.float64) - want).max()
    bound = sample_bound(float(np.abs(c).max()))
    print("sample", shape, "err %.3g bound %.3g" % (err, bound))
    assert err <= bound


# ---- properties -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_grid_points_return_the_volume(shape):
    v = volume(shape, 11 * sum(shape))
    c = br.prefilter(v)
    got = br.warp_affine(c, np.eye(3, 4), shape, fill=np.nan)
    m = float(np.abs(v).max())
    axes = sum(n > 1 for n in shape)
    bound = prefilter_bound(m, axes) + sample_bound(GAIN ** axes * m)
    err = np.abs(got.astype(np.float64) - v).max()
    print("identity", shape, "err %.3g bound %.3g" % (err, bound))
    assert err <= bound                                 # to rounding; no exact-copy promise (NaN fill: all inside)


def test_constants_and_ramps_are_reproduced():
    shape = (44, 46, 48)
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    rng = np.random.default_rng(5)
    q = [rng.uniform(20.0, n - 21.0, 500) for n in shape[::-1]]            # >= 20 voxels from every face
    for name, f in (("constant", lambda x, y, z: 37.5 + 0 * x), ("ramp", lambda x, y, z: 2.0 * x - 0.75 * y + 0.5 * z + 3)):
        v = f(x, y, z).astype(np.float32)
        flat = br.prefilter(v).reshape(-1)
        got, ins = br.sample_points(lambda k: flat[k], shape, q)
        assert ins.all()
        m = float(np.abs(v).max())
        # the mirrored extension of a ramp has a kink at each face; its trace decays as |z1|^distance: 2e-11 at 20
        bound = prefilter_bound(m, 3) + sample_bound(27 * m) + m * Z1 ** 20
        err = np.abs(got.astype(np.float64) - f(*q)).max()
        print(name, "err %.3g bound %.3g" % (err, bound))
        assert err <= bound


def test_multichannel_field_sample_is_per_channel():
    c = volume((3, 6, 7, 8), 2)
    field = np.random.default_rng(3).normal(0, 1.5, (3, 5, 6, 7)).astype(np.float32)
    field[1, 2, 3, 4] = np.nan
    out = br.warp_field(c, field, fill=9.0)
    assert out.shape == (3, 5, 6, 7) and out[0, 2, 3, 4] == 9.0
    for k in range(3):
        np.testing.assert_array_equal(out[k], br.warp_field(c[k], field, fill=9.0))
    # the field of an exactly representable affine samples where the affine does
    A = np.array([[0, 1.0, 0, 0.5], [1.0, 0, 0, 0.25], [0, 0, -1.0, 5.0]])
    from tests import field_restatement as fr
    np.testing.assert_array_equal(br.warp_field(c[0], fr.ref_affine_field(A, (5, 6, 7))),
                                  br.warp_affine(c[0], A, (5, 6, 7)))


# ---- the quality case ---------------------------------------------------------------------------------------------
def quality_volume():
    v = ndi.gaussian_filter(np.random.default_rng(0).normal(0, 1, (48, 48, 48)), 1.5)
    return (v * (100.0 / np.abs(v).max())).astype(np.float32)


def quality_maps():
    """a rotation of 7 degrees about z through the centre plus a sub-voxel shift, and its inverse"""
    A = about_center(rot((0, 0, 1), 7.0), (48, 48, 48), (48, 48, 48), shift=(0.3, -0.2, 0.4))
    M = np.linalg.inv(A[:, :3])
    return A, np.hstack([M, (-M @ A[:, 3])[:, None]])


def rms_centre(a, b):
    d = (np.asarray(a, np.float64) - b)[12:36, 12:36, 12:36]
    return float(np.sqrt((d * d).mean()))


def test_round_trip_quality():
    """there and back four times: cubic loses at most a tenth of what linear loses over [12, 36)^3"""
    v = quality_volume()
    A, B = quality_maps()
    lin = cub = v
    for _ in range(4):
        for T in (A, B):
            lin = ref_warp(lin, T, v.shape, "linear", 0.0)[0]
            cub = br.warp_affine(br.prefilter(cub), T, v.shape, 0.0)
    r_lin, r_cub = rms_centre(lin, v), rms_centre(cub, v)
    print("round trip rms: linear %.4f cubic %.4f ratio %.1f" % (r_lin, r_cub, r_lin / r_cub))
    assert r_cub <= r_lin / 10


# ---- the C entries refuse bad arguments before any device call ------------------------------------------------------
@pytest.fixture(scope="module")
def api():
    from sift3d_amd import api as a
    a.lib()
    return a


@pytest.fixture(scope="module")
def bufs(api):
    """made-up addresses without a device; real allocations covering every range named below with one"""
    from sift3d_amd import hip
    if api.device_available():
        b = [hip.lib().sift3d_hip_malloc(1 << 16) for _ in range(4)]
        assert all(b)
        yield b
        for p in b:
            hip.lib().sift3d_hip_free(p)
    else:
        yield [0x100000, 0x900000, 0x1100000, 0x1900000]


def _a(A):
    a = np.ascontiguousarray(A, np.float64).reshape(12)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


IDENT = np.eye(3, 4)


def test_symbols_exported(api):
    from sift3d_amd import _native, hip
    L = _native.load()
    for name in ("sift3d_hip_bspline_prefilter", "sift3d_hip_bspline_work_floats", "sift3d_hip_bspline_warp_affine",
                 "sift3d_hip_bspline_warp_field", "sift3d_amd_bspline_prefilter",
                 "sift3d_amd_image_bspline_warp_affine", "sift3d_amd_image_bspline_warp_field"):
        assert hasattr(L, name), name
    for name in ("bspline_prefilter", "bspline_warp_affine", "bspline_warp_field"):
        assert callable(getattr(hip, name))
    for name in ("spline_coefficients", "resample_cubic"):
        assert callable(getattr(api, name))
    W = hip.lib().sift3d_hip_bspline_work_floats
    assert W(5, 6, 7) == 210 and W(2048, 2048, 2048) == 2 ** 33
    assert W(0, 6, 7) == 0 and W(5, -1, 7) == 0 and W(5, 6, 0) == 0


def test_prefilter_refusals(bufs):
    from sift3d_amd import hip
    S, D, W, _ = bufs
    L = hip.lib()
    cases = [(None, 8, 8, 8, 1, D, W), (S, 8, 8, 8, 1, None, W), (S, 8, 8, 8, 1, D, None),
             (S, 0, 8, 8, 1, D, W), (S, 8, -1, 8, 1, D, W), (S, 8, 8, 0, 1, D, W),
             (S, 8, 8, 8, 0, D, W), (S, 8, 8, 8, -2, D, W),                # nc < 1
             (S + 2, 8, 8, 8, 1, D, W), (S, 8, 8, 8, 1, D + 1, W), (S, 8, 8, 8, 1, D, W + 2),    # misaligned
             (S, 8, 8, 8, 1, S, W),                                          # in place
             (S, 8, 8, 8, 2, S + 4 * 1000, W),                               # coef inside src's second channel
             (S + 4 * 500, 8, 8, 8, 1, S, W),                                # coef's end runs into src
             (S, 8, 8, 8, 1, D, S + 4 * 100),                                # work inside src
             (S, 8, 8, 8, 1, D, D + 4 * 500),                                # work inside coef
             (S, 8, 8, 8, 3, D, D + 4 * 1500)]                               # work inside coef's last channel
    for c in cases:
        assert L.sift3d_hip_bspline_prefilter(*c, None) == -1, c


def test_warp_affine_refusals(bufs):
    from sift3d_amd import hip
    S, D, _, _ = bufs
    L = hip.lib()
    keep, ident = _a(IDENT)
    cases = [(None, 8, 8, 8, D, 8, 8, 8, ident), (S, 8, 8, 8, None, 8, 8, 8, ident), (S, 8, 8, 8, D, 8, 8, 8, None),
             (S, 0, 8, 8, D, 8, 8, 8, ident), (S, 8, 8, -3, D, 8, 8, 8, ident),
             (S, 8, 8, 8, D, 8, 0, 8, ident), (S, 8, 8, 8, D, -1, 8, 8, ident),
             (S + 2, 8, 8, 8, D, 8, 8, 8, ident), (S, 8, 8, 8, D + 1, 8, 8, 8, ident),
             (S, 8, 8, 8, S, 8, 8, 8, ident),                                # dst is the source
             (S, 8, 8, 8, S + 4 * 511, 4, 4, 4, ident),                      # dst starts on the source's last voxel
             (S + 4 * 63, 8, 8, 8, S, 4, 4, 4, ident)]                       # dst's last voxel is the source's first
    for v in (np.nan, np.inf, -np.inf):
        for k in (0, 7, 11):
            A = IDENT.copy().reshape(12)
            A[k] = v
            cases.append((S, 8, 8, 8, D, 8, 8, 8, _a(A)[1]))
    for c in cases:
        assert L.sift3d_hip_bspline_warp_affine(*c, 0.0, None) == -1, c


def test_warp_field_refusals(bufs):
    from sift3d_amd import hip
    S, F, D, _ = bufs
    L = hip.lib()
    cases = [(None, 8, 8, 8, 1, F, 8, 8, 8, D), (S, 8, 8, 8, 1, None, 8, 8, 8, D), (S, 8, 8, 8, 1, F, 8, 8, 8, None),
             (S, 0, 8, 8, 1, F, 8, 8, 8, D), (S, 8, 8, 8, 1, F, 8, -1, 8, D),
             (S, 8, 8, 8, 0, F, 8, 8, 8, D), (S, 8, 8, 8, -3, F, 8, 8, 8, D),                 # nc < 1
             (S + 2, 8, 8, 8, 1, F, 8, 8, 8, D), (S, 8, 8, 8, 1, F + 1, 8, 8, 8, D), (S, 8, 8, 8, 1, F, 8, 8, 8, D + 2),
             (S, 8, 8, 8, 1, F, 8, 8, 8, S),                                 # dst is the source
             (S, 8, 8, 8, 2, F, 8, 8, 8, S + 4 * 1000),                      # dst inside the source's second channel
             (S, 8, 8, 8, 1, F, 8, 8, 8, F + 4 * 1500),                      # dst inside the field's last channel
             (S, 8, 8, 8, 3, F + 4 * 1500, 8, 8, 8, F)]                      # dst's last channel runs into the field
    for c in cases:
        assert L.sift3d_hip_bspline_warp_field(*c, 0.0, None) == -1, c


def _raw(name):
    from sift3d_amd import _native
    fn = _native.load()[name]                           # a function object of its own: raw pointers, NULL included
    fn.restype = C.c_int
    return fn


def test_host_form_refusals(api):
    L = api.lib()
    src, dst = api.Image(9, 7, 5), api.Image(6, 6, 6)
    two = api.Image(9, 7, 5, 2)
    ident = IDENT.reshape(12).copy()
    field = np.zeros(3 * 216, np.float32)
    WA, WF = L.sift3d_amd_image_bspline_warp_affine, L.sift3d_amd_image_bspline_warp_field
    assert WA(None, ident, 0.0, dst.h) == -1 and WA(src.h, ident, 0.0, None) == -1
    assert WA(two.h, ident, 0.0, dst.h) == -1 and WA(src.h, ident, 0.0, two.h) == -1
    assert WA(dst.h, ident, 0.0, dst.h) == -1                                    # dst is src
    bad = ident.copy()
    bad[3] = np.nan
    assert WA(src.h, bad, 0.0, dst.h) == -1
    assert WF(None, field, 0.0, dst.h) == -1 and WF(src.h, field, 0.0, None) == -1
    assert WF(two.h, field, 0.0, dst.h) == -1 and WF(src.h, field, 0.0, two.h) == -1
    assert WF(dst.h, field, 0.0, dst.h) == -1
    addr = C.cast(L.sift3d_image_data(dst.h), C.c_void_p).value
    alias = np.ctypeslib.as_array((C.c_float * (3 * 216)).from_address(addr - 4 * 216))
    assert WF(src.h, alias, 0.0, dst.h) == -1                                    # a field that holds dst's data
    raw = _raw("sift3d_amd_image_bspline_warp_affine")
    raw.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
    assert raw(src.h, None, 0.0, dst.h) == -1
    raw = _raw("sift3d_amd_image_bspline_warp_field")
    raw.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
    assert raw(src.h, None, 0.0, dst.h) == -1
    P = _raw("sift3d_amd_bspline_prefilter")
    P.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    a, b = np.zeros(2 * 60, np.float32), np.full(2 * 60, 7, np.float32)
    assert P(None, 3, 4, 5, 1, b.ctypes.data) == -1 and P(a.ctypes.data, 3, 4, 5, 1, None) == -1
    assert P(a.ctypes.data, 0, 4, 5, 1, b.ctypes.data) == -1 and P(a.ctypes.data, 3, 4, -5, 1, b.ctypes.data) == -1
    assert P(a.ctypes.data, 3, 4, 5, 0, b.ctypes.data) == -1
    assert P(a.ctypes.data, 3, 4, 5, 1, a.ctypes.data) == -1                     # in place
    assert P(a.ctypes.data, 3, 4, 5, 2, a.ctypes.data + 4 * 100) == -1           # coef inside the second channel
    assert (b == 7).all()                                                        # nothing written


def test_python_value_errors(api):
    v = np.zeros((5, 7, 9), np.float32)
    t = api.TPS(np.zeros((5, 3)), np.zeros((5, 3)), IDENT)
    with pytest.raises(ValueError):
        api.resample_cubic(v, IDENT)                                             # an affine needs out_shape
    with pytest.raises(ValueError):
        api.resample_cubic(v, t)
    with pytest.raises(ValueError):
        api.resample_cubic(v, t, (5, 7, 9))                                      # a host volume takes no TPS
    with pytest.raises(ValueError):
        api.resample_cubic(v, np.zeros((2, 6, 6, 6), np.float32))                # not a field
    with pytest.raises(ValueError):
        api.resample_cubic(v, np.zeros((3, 3)), (5, 7, 9))                       # neither 3 x 4 nor a field
    with pytest.raises(ValueError):
        api.resample_cubic(v, np.zeros((3, 6, 6, 6), np.float32), (6, 6, 7))     # out_shape is not the field's grid
    with pytest.raises(ValueError):
        api.resample_cubic(v, IDENT, (5, 7, 9), prefiltered=True)                # host coefficients
    with pytest.raises(ValueError):
        api.resample_cubic(np.zeros((2, 5, 7, 9), np.float32), IDENT, (5, 7, 9))
    with pytest.raises(ValueError):
        api.spline_coefficients(np.zeros((7, 9), np.float32))
    if not api.device_available():
        with pytest.raises(RuntimeError):
            api.resample_cubic(v, IDENT, (5, 7, 9))
        with pytest.raises(RuntimeError):
            api.resample_cubic(v, np.zeros((3, 6, 6, 6), np.float32))
        with pytest.raises(RuntimeError):
            api.spline_coefficients(v)
