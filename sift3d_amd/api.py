"""Python mirror of the reference's C API, bound with ctypes to libsift3d_amd.so.

Same names and argument meaning as sift.h / imutil.h of fatimp/SIFT3D v2.0
(reference: sift3d/sift.h:24-208, sift3d/imutil.h:39-110): functions return
SIFT3D_SUCCESS (0) / SIFT3D_FAILURE (-1) and print a message on stderr, objects are
opaque handles the caller frees.  The thin classes below only add lifetime management
and numpy views; they contain no algorithmic code.

Volumes are numpy float32 arrays of shape [nz, ny, nx] (x fastest), which is the memory
layout of sift3d_image_data() (reference: sift3d/imutil.c:520-533).
"""
import collections
import ctypes as C
import math
import os
import warnings

import numpy as np

from . import _native

SIFT3D_SUCCESS = 0
SIFT3D_FAILURE = -1
SIFT3D_DOUBLE, SIFT3D_FLOAT, SIFT3D_INT = 0, 1, 2
TIMED_BLURS = 8
NUM_TIMINGS = 10 + 2 * TIMED_BLURS + 4

_f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_u64p = np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")


class _Measures(C.Structure):                               # sift3d_amd_similarity
    _fields_ = [("n", C.c_uint64)] + [(k, C.c_double) for k in ("msd", "ncc", "mi", "nmi", "entropy_fixed",
                                                                  "entropy_moving", "entropy_joint")]


class _SurfaceResult(C.Structure):                          # sift3d_amd_surface_result
    _fields_ = [("n_f", C.c_uint64), ("n_m", C.c_uint64)] + [(k, C.c_double) for k in (
        "hausdorff", "hd95", "assd", "mean_fm", "mean_mf", "max_fm", "max_mf")]


_bound = None


def lib():
    """The loaded library with argtypes/restypes declared for every exported symbol."""
    global _bound
    if _bound is not None:
        return _bound
    L = _native.load()
    vp = C.c_void_p
    sig = {
        # imutil.h
        "sift3d_make_image": (vp, [C.c_int] * 4),
        "sift3d_free_image": (None, [vp]),
        "sift3d_read_image": (vp, [C.c_char_p]),
        "sift3d_image_data": (C.POINTER(C.c_float), [vp]),
        "sift3d_make_mat_rm": (vp, []),
        "sift3d_free_mat_rm": (None, [vp]),
        "sift3d_mat_rm_data": (vp, [vp]),
        "sift3d_mat_rm_dimensions": (None, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "sift3d_mat_rm_type": (C.c_int, [vp]),
        # sift.h
        "sift3d_make_detector": (vp, []),
        "sift3d_free_detector": (None, [vp]),
        "sift3d_detector_set_peak_thresh": (C.c_int, [vp, C.c_double]),
        "sift3d_detector_set_corner_thresh": (C.c_int, [vp, C.c_double]),
        "sift3d_detector_set_num_kp_levels": (C.c_int, [vp, C.c_uint]),
        "sift3d_detector_set_sigma_n": (C.c_int, [vp, C.c_double]),
        "sift3d_detector_set_sigma0": (C.c_int, [vp, C.c_double]),
        "sift3d_detect_keypoints": (C.c_int, [vp, vp, vp]),
        "sift3d_extract_descriptors": (C.c_int, [vp, vp, vp]),
        "sift3d_make_keypoint_store": (vp, []),
        "sift3d_free_keypoint_store": (None, [vp]),
        "sift3d_keypoint_store_to_mat_rm": (C.c_int, [vp, vp]),
        "sift3d_keypoint_store_save": (C.c_int, [C.c_char_p, vp]),
        "sift3d_keypoint_store_sort_by_strength": (None, [vp, C.c_int]),
        "sift3d_make_descriptor_store": (vp, []),
        "sift3d_free_descriptor_store": (None, [vp]),
        "sift3d_descriptor_store_save": (C.c_int, [C.c_char_p, vp]),
        "sift3d_descriptor_store_to_mat_rm": (C.c_int, [vp, vp]),
        # sift3d_amd.h extensions
        "sift3d_amd_detect_keypoints_device": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int,
                                                         C.c_double, C.c_double, C.c_double, vp]),
        "sift3d_amd_image_set_units": (C.c_int, [vp, C.c_double, C.c_double, C.c_double]),
        "sift3d_amd_timings": (C.POINTER(C.c_double), [vp]),
        "sift3d_amd_num_candidates": (C.c_int, [vp]),
        "sift3d_amd_describe_clock": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "sift3d_amd_build_pyramid_device": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                                      C.c_double]),
        "sift3d_amd_image_info": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_double)]),
        "sift3d_amd_detector_set_cuboid_extrema": (C.c_int, [vp, C.c_int]),
        "sift3d_amd_detector_set_dogmax_pass": (C.c_int, [vp, C.c_int]),
        "sift3d_amd_detector_set_exact_descriptors": (C.c_int, [vp, C.c_int]),
        "sift3d_amd_detector_set_serial_orientation": (C.c_int, [vp, C.c_int]),
        "sift3d_amd_detector_set_candidate_capacity": (C.c_int, [vp, C.c_int]),
        "sift3d_amd_detector_candidate_capacity": (C.c_int, [vp]),
        "sift3d_amd_detector_dogmax": (C.c_int, [vp, vp, C.c_int]),
        "sift3d_amd_copy_level": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, _i32p]),
        "sift3d_amd_keypoint_store_size": (C.c_int, [vp]),
        "sift3d_amd_keypoint_store_get": (C.c_int, [vp, C.c_int, C.POINTER(C.c_int),
                                                    C.POINTER(C.c_int), _f64p,
                                                    C.POINTER(C.c_float), _f32p]),
        "sift3d_amd_keypoint_store_set": (C.c_int, [vp, C.c_int, _i32p, _f64p, _f32p, _f32p]),
        "sift3d_amd_descriptor_store_size": (C.c_int, [vp]),
        "sift3d_amd_descriptor_store_set": (C.c_int, [vp, C.c_int, _f64p, _f32p, C.c_int, C.c_int, C.c_int]),
        "sift3d_amd_nn_match": (C.c_int, [vp, vp, C.c_double, _i32p]),
        "sift3d_amd_descriptor_store_keep_device": (C.c_int, [vp, C.c_int]),
        "sift3d_amd_descriptor_store_xyz_all": (C.c_int, [vp, _f64p]),
        "sift3d_amd_descriptor_store_xyz": (C.c_int, [vp, C.c_int, _f64p]),
        "sift3d_amd_ransac_affine": (C.c_int, [_f64p, _f64p, C.c_int, C.c_double, C.c_int, C.c_uint64,
                                              _f64p, np.ctypeslib.ndpointer(np.uint8),
                                              C.POINTER(C.c_int)]),
        "sift3d_amd_image_warp_affine": (C.c_int, [vp, _f64p, C.c_int, C.c_float, vp]),
        "sift3d_amd_affine_invert": (C.c_int, [_f64p, _f64p]),
        "sift3d_amd_tps_fit": (C.c_int, [_f64p, _f64p, C.c_int, C.c_double, C.c_int, _f64p, _f64p, _f64p,
                                        C.POINTER(C.c_int)]),
        "sift3d_amd_tps_apply": (C.c_int, [_f64p, _f64p, _f64p, C.c_int, _f64p, C.c_int, _f64p]),
        "sift3d_amd_tps_pack": (C.c_int, [_f64p, _f64p, C.c_int, _f32p]),
        "sift3d_amd_image_warp_tps": (C.c_int, [vp, _f64p, _f32p, C.c_int, C.c_int, C.c_float, vp]),
        "sift3d_amd_image_warp_field": (C.c_int, [vp, _f32p, C.c_int, C.c_float, vp]),
        "sift3d_amd_jacobian_det": (C.c_int, [_f32p, C.c_int, C.c_int, C.c_int, vp, C.POINTER(C.c_uint64),
                                             C.POINTER(C.c_float), C.POINTER(C.c_float)]),
        "sift3d_amd_bspline_prefilter": (C.c_int, [_f32p, C.c_int, C.c_int, C.c_int, C.c_int, _f32p]),
        "sift3d_amd_image_bspline_warp_affine": (C.c_int, [vp, _f64p, C.c_float, vp]),
        "sift3d_amd_image_bspline_warp_field": (C.c_int, [vp, _f32p, C.c_float, vp]),
        "sift3d_amd_similarity_measures": (C.c_int, [_u64p, C.c_int, vp, C.POINTER(_Measures)]),
        "sift3d_amd_label_overlap": (C.c_int, [_u64p, C.c_int, _f64p, _f64p, _u64p, _u64p]),
        "sift3d_amd_surface_measures": (C.c_int, [_f32p, C.c_uint64, _f32p, C.c_uint64, C.POINTER(_SurfaceResult)]),
        "sift3d_amd_image_dense_descriptors": (C.c_int, [vp, C.c_double, _f32p]),
        "sift3d_amd_image_dense_descriptors_rotate": (C.c_int, [vp, C.c_double, _f32p]),
        "sift3d_amd_device_available": (C.c_int, []),
        "sift3d_amd_version": (C.c_char_p, []),
        "sift3d_amd_synth_survey": (None, [_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64]),
        "sift3d_amd_synth_lattice": (None, [_f32p, C.c_int, C.c_int, C.c_int, C.c_uint64]),
        "sift3d_amd_gauss_filter": (C.c_int, [C.c_double, _f32p, C.c_int]),
        "sift3d_amd_init": (C.c_int, []),
        "sift3d_amd_host_expf": (None, [_f32p, _f32p, C.c_size_t]),
        "sift3d_amd_host_eigen3": (None, [_f64p, _f64p, _f64p]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError here = the library does not export the ABI
        fn.restype = res
        fn.argtypes = args
    _bound = L
    return L


def device_available():
    return bool(lib().sift3d_amd_device_available())


class MatRm:
    """sift3d_mat_rm (reference: sift3d/imutil.h:77-110)."""

    def __init__(self):
        self.h = lib().sift3d_make_mat_rm()
        if not self.h:
            raise MemoryError("sift3d_make_mat_rm")

    def free(self):
        # (at interpreter shutdown module globals may already be gone: nothing to do then)
        if getattr(self, "h", None) and lib is not None:
            lib().sift3d_free_mat_rm(self.h)
            self.h = None

    __del__ = free

    def dimensions(self):
        c, r = C.c_int(), C.c_int()
        lib().sift3d_mat_rm_dimensions(self.h, C.byref(c), C.byref(r))
        return c.value, r.value

    def type(self):
        return lib().sift3d_mat_rm_type(self.h)

    def numpy(self):
        cols, rows = self.dimensions()
        dt = {SIFT3D_DOUBLE: np.float64, SIFT3D_FLOAT: np.float32, SIFT3D_INT: np.int32}[self.type()]
        if rows * cols == 0:
            return np.zeros((rows, cols), dt)
        p = lib().sift3d_mat_rm_data(self.h)
        buf = (C.c_char * (rows * cols * np.dtype(dt).itemsize)).from_address(p)
        return np.frombuffer(buf, dt).reshape(rows, cols).copy()


class Image:
    """sift3d_image (reference: sift3d/imutil.h:39-65)."""

    def __init__(self, nx, ny, nz, nc=1):
        self.h = lib().sift3d_make_image(nx, ny, nz, nc)
        if not self.h:
            raise ValueError("sift3d_make_image(%d, %d, %d, %d) failed" % (nx, ny, nz, nc))
        self.shape = (nz, ny, nx) if nc == 1 else (nz, ny, nx, nc)

    @classmethod
    def read(cls, path):
        """sift3d_read_image: single-file NIFTI-1 (.nii, .nii.gz).  Raises IOError on failure."""
        h = lib().sift3d_read_image(os.fsencode(path))
        if not h:
            raise IOError("sift3d_read_image(%r) failed" % (path,))
        self = cls.__new__(cls)
        self.h = h
        dims = (C.c_int * 4)()
        lib().sift3d_amd_image_info(h, dims, None)
        nx, ny, nz, nc = dims
        self.shape = (nz, ny, nx) if nc == 1 else (nz, ny, nx, nc)
        return self

    @property
    def units(self):
        u = (C.c_double * 3)()
        lib().sift3d_amd_image_info(self.h, None, u)
        return tuple(u)

    @classmethod
    def from_array(cls, vol, units=None):
        vol = np.ascontiguousarray(vol, np.float32)
        nz, ny, nx = vol.shape
        im = cls(nx, ny, nz, 1)
        im.data()[...] = vol
        if units is not None:
            if lib().sift3d_amd_image_set_units(im.h, *map(float, units)) != 0:
                raise ValueError("invalid units")
        return im

    def data(self):
        p = lib().sift3d_image_data(self.h)
        return np.ctypeslib.as_array(p, shape=self.shape)

    def free(self):
        # (at interpreter shutdown module globals may already be gone: nothing to do then)
        if getattr(self, "h", None) and lib is not None:
            lib().sift3d_free_image(self.h)
            self.h = None

    __del__ = free


KP_DTYPE = np.dtype([("R", "f4", (3, 3)), ("xd", "f8"), ("yd", "f8"), ("zd", "f8"),
                     ("sd", "f8"), ("o", "i4"), ("s", "i4"), ("strength", "f4")])


class KeypointStore:
    """sift3d_keypoint_store (reference: sift3d/sift.h:121-165)."""

    def __init__(self):
        self.h = lib().sift3d_make_keypoint_store()

    def free(self):
        # (at interpreter shutdown module globals may already be gone: nothing to do then)
        if getattr(self, "h", None) and lib is not None:
            lib().sift3d_free_keypoint_store(self.h)
            self.h = None

    __del__ = free

    def __len__(self):
        return lib().sift3d_amd_keypoint_store_size(self.h)

    def to_mat_rm(self):
        m = MatRm()
        if lib().sift3d_keypoint_store_to_mat_rm(self.h, m.h) != 0:
            raise RuntimeError("sift3d_keypoint_store_to_mat_rm failed")
        return m.numpy()

    def sort_by_strength(self, limit=0):
        lib().sift3d_keypoint_store_sort_by_strength(self.h, int(limit))

    def save(self, path):
        return lib().sift3d_keypoint_store_save(path.encode(), self.h)

    def records(self):
        """All fields of every keypoint (the reference only exposes them through "%f" CSV)."""
        n = len(self)
        out = np.zeros(n, KP_DTYPE)
        o, s, st = C.c_int(), C.c_int(), C.c_float()
        xyz = np.zeros(4, np.float64)
        R = np.zeros(9, np.float32)
        L = lib()
        for i in range(n):
            assert L.sift3d_amd_keypoint_store_get(self.h, i, C.byref(o), C.byref(s), xyz,
                                                   C.byref(st), R) == 0
            out[i] = (R.reshape(3, 3), xyz[0], xyz[1], xyz[2], xyz[3], o.value, s.value, st.value)
        return out

    def set_records(self, recs):
        n = len(recs)
        os_ = np.ascontiguousarray(np.stack([recs["o"], recs["s"]], 1), np.int32).reshape(-1)
        xyz = np.ascontiguousarray(np.stack([recs["xd"], recs["yd"], recs["zd"], recs["sd"]], 1),
                                   np.float64).reshape(-1)
        st = np.ascontiguousarray(recs["strength"], np.float32)
        R = np.ascontiguousarray(recs["R"], np.float32).reshape(-1)
        if n == 0:
            os_ = np.zeros(2, np.int32); xyz = np.zeros(4); st = np.zeros(1, np.float32)
            R = np.zeros(9, np.float32)
        return lib().sift3d_amd_keypoint_store_set(self.h, n, os_, xyz, st, R)


class DescriptorStore:
    """sift3d_descriptor_store (reference: sift3d/sift.h:175-208)."""

    def __init__(self):
        self.h = lib().sift3d_make_descriptor_store()

    def free(self):
        # (at interpreter shutdown module globals may already be gone: nothing to do then)
        if getattr(self, "h", None) and lib is not None:
            lib().sift3d_free_descriptor_store(self.h)
            self.h = None

    __del__ = free

    def __len__(self):
        return lib().sift3d_amd_descriptor_store_size(self.h)

    def to_mat_rm(self):
        m = MatRm()
        if lib().sift3d_descriptor_store_to_mat_rm(self.h, m.h) != 0:
            raise RuntimeError("sift3d_descriptor_store_to_mat_rm failed")
        return m.numpy()

    def save(self, path):
        return lib().sift3d_descriptor_store_save(path.encode(), self.h)

    def keep_device(self, on=True):
        """Keep a copy of the histograms in HBM (written by extract_descriptors) for the matcher."""
        return lib().sift3d_amd_descriptor_store_keep_device(self.h, int(bool(on)))

    def xyz(self):
        """Keypoint coordinates in octave-0 voxels, one row per descriptor."""
        out = np.zeros((max(len(self), 1), 3), np.float64)
        if lib().sift3d_amd_descriptor_store_xyz_all(self.h, out.reshape(-1)) != 0:
            raise RuntimeError("sift3d_amd_descriptor_store_xyz_all failed")
        return out[:len(self)]

    def set(self, xyz_sd, hist, dims=(0, 0, 0)):
        """Fill the store from host arrays (tests of the writers without a device)."""
        xyz_sd = np.ascontiguousarray(xyz_sd, np.float64).reshape(-1, 4)
        hist = np.ascontiguousarray(hist, np.float32).reshape(-1, 768)
        assert len(xyz_sd) == len(hist)
        if len(hist) == 0:
            xyz_sd, hist = np.zeros((1, 4)), np.zeros((1, 768), np.float32)
            return lib().sift3d_amd_descriptor_store_set(self.h, 0, xyz_sd.reshape(-1), hist.reshape(-1),
                                                         *[int(v) for v in dims])
        return lib().sift3d_amd_descriptor_store_set(self.h, len(hist), xyz_sd.reshape(-1),
                                                     hist.reshape(-1), *[int(v) for v in dims])


class Detector:
    """sift3d_detector (reference: sift3d/sift.h:24-111)."""

    def __init__(self, peak_thresh=None, corner_thresh=None, num_kp_levels=None, sigma_n=None,
                 sigma0=None, cuboid_extrema=None, exact_descriptors=None):
        self.h = lib().sift3d_make_detector()
        if not self.h:
            raise MemoryError("sift3d_make_detector")
        for name, v in (("sigma_n", sigma_n), ("sigma0", sigma0), ("peak_thresh", peak_thresh),
                        ("corner_thresh", corner_thresh), ("num_kp_levels", num_kp_levels),
                        ("cuboid_extrema", cuboid_extrema), ("exact_descriptors", exact_descriptors)):
            if v is not None and getattr(self, "set_" + name)(v) != 0:
                raise ValueError("sift3d_detector_set_%s(%r) failed" % (name, v))

    def free(self):
        # (at interpreter shutdown module globals may already be gone: nothing to do then)
        if getattr(self, "h", None) and lib is not None:
            lib().sift3d_free_detector(self.h)
            self.h = None

    __del__ = free

    def set_peak_thresh(self, v):
        return lib().sift3d_detector_set_peak_thresh(self.h, float(v))

    def set_corner_thresh(self, v):
        return lib().sift3d_detector_set_corner_thresh(self.h, float(v))

    def set_num_kp_levels(self, v):
        return lib().sift3d_detector_set_num_kp_levels(self.h, int(v))

    def set_sigma_n(self, v):
        return lib().sift3d_detector_set_sigma_n(self.h, float(v))

    def set_sigma0(self, v):
        return lib().sift3d_detector_set_sigma0(self.h, float(v))

    def set_cuboid_extrema(self, on):
        """Run-time form of the reference's compile-time CUBOID_EXTREMA (sift.c:24)."""
        return lib().sift3d_amd_detector_set_cuboid_extrema(self.h, int(bool(on)))

    def set_serial_orientation(self, on):
        """A/B switch: the reference's serial window sums for every candidate (same results bit for bit)."""
        return lib().sift3d_amd_detector_set_serial_orientation(self.h, int(bool(on)))

    def set_exact_descriptors(self, mode):
        """0: automatic (wide windows in the reference's accumulation order), 1: always (descriptors bit-exact
        with the reference), -1: never."""
        return lib().sift3d_amd_detector_set_exact_descriptors(self.h, int(mode))

    def set_dogmax_pass(self, on):
        """A/B switch: octave 0's dogmax scan as a pass of its own (True) or gathered by the extrema sweep."""
        return lib().sift3d_amd_detector_set_dogmax_pass(self.h, int(bool(on)))

    def set_candidate_capacity(self, cap):
        """Diagnostic hook: the next detect starts from a candidate list of exactly `cap` records (0: the
        default, 2^18); one that does not fit grows the list to count + count // 4 + 1024 and sweeps again."""
        if lib().sift3d_amd_detector_set_candidate_capacity(self.h, int(cap)) != 0:
            raise ValueError("sift3d_amd_detector_set_candidate_capacity(%r)" % (cap,))

    def candidate_capacity(self):
        """Records the candidate list holds (or the next detect starts from)."""
        return lib().sift3d_amd_detector_candidate_capacity(self.h)

    def dogmax(self):
        """max|DoG| of every DoG level of the last detect call (float32, octave-major)."""
        out = np.zeros(1024, np.float32)
        n = lib().sift3d_amd_detector_dogmax(self.h, out.ctypes.data, out.size)
        if n < 0:
            raise RuntimeError("sift3d_amd_detector_dogmax")
        return out[:n].copy()

    def detect_keypoints(self, image, store):
        return lib().sift3d_detect_keypoints(self.h, image.h, store.h)

    def detect_keypoints_device(self, d_ptr, nx, ny, nz, store, units=(1.0, 1.0, 1.0)):
        """sift3d_amd_detect_keypoints_device: the volume is already resident in HBM."""
        return lib().sift3d_amd_detect_keypoints_device(self.h, d_ptr, nx, ny, nz,
                                                        *map(float, units), store.h)

    def extract_descriptors(self, kp_store, desc_store):
        return lib().sift3d_extract_descriptors(self.h, kp_store.h, desc_store.h)

    def timings(self):
        p = lib().sift3d_amd_timings(self.h)
        names = ("scale", "gauss", "dog", "extrema", "orient", "describe", "gauss_dev",
                 "detect_wall", "describe_wall", "yz_last")
        out = dict(zip(names, [p[i] for i in range(len(names))]))
        out["detect_dev"] = p[10 + 2 * TIMED_BLURS]       # first to last stage event of detect
        out["compact_host"] = p[10 + 2 * TIMED_BLURS + 1]  # the host's candidate -> keypoint compaction
        # first stage event -> end of the orientation of octave 0's candidates / of the other octaves' (0: one part)
        out["orient_oct0_end"] = p[10 + 2 * TIMED_BLURS + 2]
        out["orient_rest_end"] = p[10 + 2 * TIMED_BLURS + 3]
        return out

    def describe_clock(self):
        """(shader cycles, seconds) of the fast descriptor kernel of the last extract_descriptors, measured by
        the kernel itself (its first, persistent wave); None when nothing was recorded."""
        c, t = C.c_double(), C.c_double()
        if lib().sift3d_amd_describe_clock(self.h, C.byref(c), C.byref(t)) != 0 or t.value <= 0:
            return None
        return c.value, t.value

    def launch_timings(self):
        """Octave 0's pyramid launches of the last detect, HIP events around each on its stream:
        (x-pass seconds, fused y+z seconds) per blur s = 0 .. ngl-1; 0.0 where a blur did not take the
        fused kernel."""
        p = lib().sift3d_amd_timings(self.h)
        return [(p[10 + b], p[10 + TIMED_BLURS + b]) for b in range(TIMED_BLURS)]

    def build_pyramid_device(self, ptr, nx, ny, nz, units=(1.0, 1.0, 1.0)):
        return lib().sift3d_amd_build_pyramid_device(self.h, ptr, nx, ny, nz, *map(float, units))

    def num_candidates(self):
        return lib().sift3d_amd_num_candidates(self.h)

    def level(self, which, o, s):
        dims = np.zeros(3, np.int32)
        if lib().sift3d_amd_copy_level(self.h, which, o, s, None, dims) != 0:
            raise IndexError("no such level")
        out = np.empty((dims[2], dims[1], dims[0]), np.float32)
        if lib().sift3d_amd_copy_level(self.h, which, o, s, out.ctypes.data, dims) != 0:
            raise RuntimeError("sift3d_amd_copy_level failed")
        return out


def synth_survey(n, nblob=None, seed=0):
    """SURVEY.md 8(d) volume (sequential generator, host)."""
    nx, ny, nz = (n, n, n) if np.isscalar(n) else n
    if nblob is None:
        nblob = int(round(200 * (nx * ny * nz) / 64.0 ** 3))
    v = np.zeros((nz, ny, nx), np.float32)
    lib().sift3d_amd_synth_survey(v, nx, ny, nz, nblob, seed)
    return v


def synth_lattice(n, seed=1):
    nx, ny, nz = (n, n, n) if np.isscalar(n) else n
    v = np.zeros((nz, ny, nx), np.float32)
    lib().sift3d_amd_synth_lattice(v, nx, ny, nz, seed)
    return v


def gauss_filter(sigma):
    """Normalised Gaussian taps exactly as the detector computes them (imutil.c:1267-1319)."""
    taps = np.zeros(1024, np.float32)
    w = lib().sift3d_amd_gauss_filter(float(sigma), taps, 1024)
    if w < 1 or w > 1024:
        raise ValueError("gauss_filter(%r)" % sigma)
    return taps[:w].copy()


# ---- registration (BASELINE config 5; removed from the reference fork: pinned to restatements) --
class Matcher:
    """sift3d_amd_matcher: descriptor matching with reusable device scratch."""

    def __init__(self):
        L = lib()
        L.sift3d_amd_make_matcher.restype = C.c_void_p
        L.sift3d_amd_free_matcher.argtypes = [C.c_void_p]
        L.sift3d_amd_free_matcher.restype = None
        L.sift3d_amd_matcher_match.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                               np.ctypeslib.ndpointer(np.int32)]
        L.sift3d_amd_matcher_seconds.argtypes = [C.c_void_p]
        L.sift3d_amd_matcher_seconds.restype = C.c_double
        L.sift3d_amd_matcher_match_guided.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p,
                                                      np.ctypeslib.ndpointer(np.float64), C.c_double, C.c_double,
                                                      C.c_double, np.ctypeslib.ndpointer(np.int32)]
        L.sift3d_amd_matcher_blocks.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        self.h = L.sift3d_amd_make_matcher()
        if not self.h:
            raise RuntimeError("sift3d_amd_make_matcher failed (no HIP device?)")

    def match(self, desc_a, desc_b, nn_thresh=0.8):
        """match[i] = index in desc_b of the descriptor matched to descriptor i of desc_a, or -1."""
        out = np.full(max(len(desc_a), 1), -1, np.int32)
        if lib().sift3d_amd_matcher_match(self.h, desc_a.h, desc_b.h, float(nn_thresh), out) != 0:
            raise RuntimeError("sift3d_amd_matcher_match failed")
        return out[:len(desc_a)]

    def match_guided(self, desc_a, desc_b, pred_a, radius, nn_thresh=0.8, max_distance=None):
        """match() among the candidates within `radius` (voxels of desc_b's frame) of where a transform predicts each
        descriptor of desc_a (sift3d_amd_matcher_match_guided).  pred_a: the predicted positions (n x 3), or a 3 x 4
        push map (a's voxel -> b's voxel), applied to desc_a.xyz() in float64.  max_distance: the largest accepted
        descriptor distance of a match, or None."""
        n = len(desc_a)
        pred = np.ascontiguousarray(pred_a, np.float64)
        if pred.shape == (3, 4):
            pred = desc_a.xyz().reshape(-1, 3) @ pred[:, :3].T + pred[:, 3]
        if pred.shape != (n, 3):
            raise ValueError("match_guided: pred_a must be %d x 3 positions or a 3 x 4 map, not %r" % (n, pred.shape))
        pred = np.ascontiguousarray(pred).reshape(-1)
        out = np.full(max(n, 1), -1, np.int32)
        if lib().sift3d_amd_matcher_match_guided(self.h, desc_a.h, desc_b.h, pred if n else np.zeros(3), float(radius),
                                                 float(nn_thresh), 0.0 if max_distance is None else float(max_distance),
                                                 out) != 0:
            raise RuntimeError("sift3d_amd_matcher_match_guided failed")
        return out[:n]

    def seconds(self):
        """Device seconds of the two nearest-neighbour searches of the last match."""
        return float(lib().sift3d_amd_matcher_seconds(self.h))

    def blocks(self):
        """(visited, total) 128 x 128 block pairs of the last match_guided, both searches summed."""
        v, t = C.c_uint64(), C.c_uint64()
        if lib().sift3d_amd_matcher_blocks(self.h, C.byref(v), C.byref(t)) != 0:
            raise RuntimeError("sift3d_amd_matcher_blocks failed")
        return int(v.value), int(t.value)

    def free(self):
        if getattr(self, "h", None) and lib is not None:
            lib().sift3d_amd_free_matcher(self.h)
            self.h = None

    __del__ = free


def nn_match(desc_a, desc_b, nn_thresh=0.8):
    """match[i] = index in desc_b of the descriptor matched to descriptor i of desc_a, or -1."""
    out = np.full(max(len(desc_a), 1), -1, np.int32)
    if lib().sift3d_amd_nn_match(desc_a.h, desc_b.h, float(nn_thresh), out) != 0:
        raise RuntimeError("sift3d_amd_nn_match failed")
    return out[:len(desc_a)]


def spatial_order(xyz, cell):
    """The row order match_guided walks a set in (sift3d_amd_spatial_order): the indices of the points xyz (n x 3)
    sorted by the Morton key of their cell of size `cell`, then by index; non-finite points last."""
    p = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    perm = np.zeros(max(len(p), 1), np.int32)
    L = lib()
    L.sift3d_amd_spatial_order.argtypes = [np.ctypeslib.ndpointer(np.float64), C.c_int, C.c_double,
                                           np.ctypeslib.ndpointer(np.int32)]
    if L.sift3d_amd_spatial_order(p.reshape(-1) if len(p) else np.zeros(3), len(p), float(cell), perm) != 0:
        raise ValueError("spatial_order: cell must be positive, not %r" % (cell,))
    return perm[:len(p)]


def ransac_affine(src, dst, err_thresh=5.0, num_iter=500, seed=1):
    """Affine map dst = A [src; 1]: returns (A 3x4, inlier mask)."""
    src = np.ascontiguousarray(src, np.float64).reshape(-1, 3)
    dst = np.ascontiguousarray(dst, np.float64).reshape(-1, 3)
    assert len(src) == len(dst)
    A = np.zeros(12, np.float64)
    inl = np.zeros(max(len(src), 1), np.uint8)
    cnt = C.c_int()
    rc = lib().sift3d_amd_ransac_affine(src.reshape(-1), dst.reshape(-1), len(src), float(err_thresh),
                                        int(num_iter), int(seed), A, inl, C.byref(cnt))
    if rc != 0:
        raise RuntimeError("sift3d_amd_ransac_affine: no model")
    return A.reshape(3, 4), inl[:len(src)].astype(bool)


# ---- resampling: apply an affine map to a volume -------------------------------------------------
INTERP = {"nearest": 0, "linear": 1}


def affine_invert(A):
    """Inverse of the affine map x -> A [x; 1] (3 x 4).  ValueError when the 3 x 3 part is singular."""
    a = np.ascontiguousarray(A, np.float64).reshape(12).copy()
    out = np.zeros(12, np.float64)
    if lib().sift3d_amd_affine_invert(a, out) != 0:
        raise ValueError("affine_invert: the linear part is singular or not finite")
    return out.reshape(3, 4)


def warp_affine(image_or_array, A, out_shape, interp="linear", fill=0.0):
    """Resample a host volume (an Image, or a float32 array [nz, ny, nx]) into a grid of
    out_shape = (oz, oy, ox) through sift3d_amd_image_warp_affine.  A (3 x 4) is a pull map in
    voxels: output voxel (x, y, z) takes the source at A [x; y; z; 1]; voxels that sample outside
    get `fill`.  Returns an Image for an Image, an array for an array."""
    if interp not in INTERP:
        raise ValueError("interp must be 'nearest' or 'linear', not %r" % (interp,))
    a = np.ascontiguousarray(A, np.float64).reshape(12).copy()
    src = image_or_array if isinstance(image_or_array, Image) else Image.from_array(image_or_array)
    oz, oy, ox = out_shape
    dst = Image(ox, oy, oz)
    if lib().sift3d_amd_image_warp_affine(src.h, a, INTERP[interp], float(fill), dst.h) != 0:
        raise RuntimeError("sift3d_amd_image_warp_affine failed")
    return dst if isinstance(image_or_array, Image) else dst.data().copy()


Registration = collections.namedtuple("Registration", "A inliers num_matches warped")


def _matched_points(moving, fixed, nn_thresh, detector_kw, what, keep_stores=False):
    """Detect + describe both volumes (torch CUDA float32 tensors [nz, ny, nx]) and match the
    descriptors: (moving xyz, fixed xyz) of the matched pairs, in voxels; with keep_stores also the two
    descriptor stores (moving's, fixed's), for a guided second match."""
    import torch
    from . import hip
    for name, v in (("moving", moving), ("fixed", fixed)):
        hip._tensor(v, "%s: %s must be a contiguous 3-D float32 CUDA tensor" % (what, name), dims=(3,))
    if moving.device != fixed.device:
        raise ValueError("%s: moving and fixed are on different devices (%s, %s)"
                         % (what, moving.device, fixed.device))
    torch.cuda.current_stream().synchronize()      # the detector works on its own stream
    stores = []
    for v in (moving, fixed):
        det, kp, desc = Detector(**detector_kw), KeypointStore(), DescriptorStore()
        desc.keep_device(True)
        nz, ny, nx = v.shape
        if det.detect_keypoints_device(v.data_ptr(), nx, ny, nz, kp) != 0:
            raise RuntimeError("%s: detect_keypoints_device failed" % what)
        if det.extract_descriptors(kp, desc) != 0:
            raise RuntimeError("%s: extract_descriptors failed" % what)
        stores.append(desc)
    d_mov, d_fix = stores
    m = Matcher().match(d_mov, d_fix, nn_thresh)
    hit = np.nonzero(m >= 0)[0]
    if keep_stores:
        return d_mov.xyz()[hit], d_fix.xyz()[m[hit]], (d_mov, d_fix)
    return d_mov.xyz()[hit], d_fix.xyz()[m[hit]]


FirstPass = collections.namedtuple("FirstPass", "A inliers num_matches")


def _rematch_keywords(rematch, nn_thresh, what):
    """rematch=None | radius | dict(radius=, nn_thresh=, max_distance=) -> match_guided's keyword arguments, or None"""
    if rematch is None:
        return None
    kw = dict(rematch) if isinstance(rematch, dict) else dict(radius=rematch)
    bad = set(kw) - {"radius", "nn_thresh", "max_distance"}
    if bad or "radius" not in kw or not float(kw["radius"]) > 0:
        raise ValueError("%s: rematch must be a positive radius or dict(radius=, nn_thresh=, max_distance=), not %r"
                         % (what, rematch))
    kw.setdefault("nn_thresh", nn_thresh)
    return kw


def _matched_points_guided(moving, fixed, nn_thresh, detector_kw, what, rematch, err_thresh, num_iter, seed):
    """_matched_points, then -- with rematch, and where RANSAC finds a model A in the matches -- the matches of
    Matcher.match_guided under A instead.  Returns (moving xyz, fixed xyz, first): first is FirstPass(A, inliers,
    num_matches) of the blind pass, or None where nothing was rematched (the points are then the blind matches')."""
    kw = _rematch_keywords(rematch, nn_thresh, what)
    if kw is None:
        return _matched_points(moving, fixed, nn_thresh, detector_kw, what) + (None,)
    p_mov, p_fix, (d_mov, d_fix) = _matched_points(moving, fixed, nn_thresh, detector_kw, what, keep_stores=True)
    try:
        A, inl = ransac_affine(p_mov, p_fix, err_thresh, num_iter, seed)
    except RuntimeError:
        return p_mov, p_fix, None                           # no model: nothing to guide
    m = Matcher().match_guided(d_mov, d_fix, A, **kw)
    hit = np.nonzero(m >= 0)[0]
    return d_mov.xyz()[hit], d_fix.xyz()[m[hit]], FirstPass(A, inl, len(p_mov))


def _with_first(result, first):
    """the result tuple's sibling with the first pass behind it (GUIDED_REGISTRATIONS), where there was one"""
    return result if first is None else GUIDED_REGISTRATIONS[type(result)](*result, first)


def register(moving, fixed, nn_thresh=0.8, err_thresh=3.0, num_iter=500, seed=1, refine=False, init=None,
             rematch=None, **detector_kw):
    """Register two volumes (torch CUDA float32 tensors [nz, ny, nx]): detect + describe both,
    match the descriptors, fit the moving -> fixed affine by RANSAC and resample `moving` into
    `fixed`'s grid.  detector_kw go to Detector().  Returns Registration(A (3 x 4, moving voxel ->
    fixed voxel), inliers (mask over the matches), num_matches, warped (tensor shaped like fixed)).
    refine=True (or a dict of refine_affine's keyword arguments) runs refine_affine from the RANSAC result and
    returns RefinedRegistration(A, inliers, num_matches, warped, A_ransac, refinement): A and warped are the refined
    map and its resampling, A_ransac is what refine=False returns as A, refinement the AffineRefinement (the
    NccAffineRefinement with refine=dict(metric="ncc"), the MiAffineRefinement with refine=dict(metric="mi")).
    Where the matches give RANSAC no model the call raises RuntimeError, but with refine=dict(metric="mi") it goes on
    from the identity (A_ransac is then the identity and inliers is all False): keypoints of two modalities often do
    not match, and that is the pair the mutual information is for.
    init: a mode of init_affine or a dict of its keyword arguments.  Where RANSAC finds no model the flow then goes on
    from init_affine's map, for any metric, instead of raising or taking the identity (A_ransac and inliers as above);
    its metric and masks default to the refinement's.  Where RANSAC finds a model init is not used.
    rematch: a radius in fixed voxels, or dict(radius=, nn_thresh=, max_distance=) for Matcher.match_guided.  After
    the first RANSAC gives A the descriptors are matched again among the candidates within the radius of where A
    puts them, and RANSAC (same err_thresh, num_iter, seed) and everything after it run on the new matches.  The
    result is then the GuidedRegistration / GuidedRefinedRegistration sibling, whose last field `first` is
    FirstPass(A, inliers, num_matches) of the first pass.  Where the first RANSAC finds no model there is nothing to
    guide and the call behaves as without rematch."""
    p_mov, p_fix, first = _matched_points_guided(moving, fixed, nn_thresh, detector_kw, "register", rematch, err_thresh,
                                                 num_iter, seed)
    return _with_first(_register_matched(moving, fixed, p_mov, p_fix, err_thresh, num_iter, seed, refine, init), first)


def _register_matched(moving, fixed, p_mov, p_fix, err_thresh, num_iter, seed, refine, init=None):
    """register() from the matched points on: RANSAC, the optional affine refinement, the resampling"""
    import torch
    from . import hip
    start = None                                            # the pull map to go on from, where RANSAC gave none
    try:
        A, inl = ransac_affine(p_mov, p_fix, err_thresh, num_iter, seed)
    except RuntimeError:
        # across modalities the descriptors often do not match (an inverted contrast already leaves none): the
        # mutual-information refinement, made for such pairs, then starts from the identity, and any refinement from
        # init_affine's map where the caller asked for one
        rkw = refine if isinstance(refine, dict) else {}
        if init is not None:
            start = init_affine(moving, fixed, **_init_keywords(
                init, "register", metric=rkw.get("metric", "msd"), mask_fixed=rkw.get("mask_fixed"),
                mask_moving=rkw.get("mask_moving"))).A
        elif rkw.get("metric") != "mi":
            raise
        A, inl = np.eye(3, 4), np.zeros(len(p_mov), bool)
    if refine:
        r = refine_affine(moving, fixed, affine_invert(A) if start is None else start,
                          **(refine if isinstance(refine, dict) else {}))
        return RefinedRegistration(affine_invert(r.A), inl, len(p_mov), r.warped, A, r)
    if start is not None:
        A = affine_invert(start)
    warped = torch.empty_like(fixed)
    hip.warp_affine(moving, warped, affine_invert(A), "linear")
    return Registration(A, inl, len(p_mov), warped)


# ---- thin-plate spline: deformable registration ---------------------------------------------------
TPS = collections.namedtuple("TPS", "ctrl weights A")
TPS_MAX_POINTS = 16384


def tps_fit(src, dst, smoothing=0.0, max_points=2048):
    """Thin-plate spline q = TPS(p) through (smoothing 0) or near the pairs src[i] -> dst[i] (n x 3,
    voxels) by sift3d_amd_tps_fit: exact duplicate src points dropped, farthest-point thinning to
    max_points.  Returns TPS(ctrl (m x 3), weights (m x 3), A (3 x 4)); ValueError when there is no fit."""
    src = np.ascontiguousarray(src, np.float64).reshape(-1, 3)
    dst = np.ascontiguousarray(dst, np.float64).reshape(-1, 3)
    if len(src) != len(dst):
        raise ValueError("tps_fit: src and dst hold %d and %d points" % (len(src), len(dst)))
    cap = max(int(max_points), 1)
    ctrl = np.zeros((cap, 3), np.float64)
    w = np.zeros((cap, 3), np.float64)
    A = np.zeros(12, np.float64)
    m = C.c_int()
    if lib().sift3d_amd_tps_fit(src.reshape(-1), dst.reshape(-1), len(src), float(smoothing), int(max_points),
                                ctrl.reshape(-1), w.reshape(-1), A, C.byref(m)) != 0:
        raise ValueError("tps_fit: no fit (too few distinct or coplanar points, or bad arguments)")
    return TPS(ctrl[:m.value].copy(), w[:m.value].copy(), A.reshape(3, 4))


def tps_apply(tps, points):
    """q(p) for points (n x 3, voxels) in double (sift3d_amd_tps_apply)."""
    c = np.ascontiguousarray(tps.ctrl, np.float64).reshape(-1)
    w = np.ascontiguousarray(tps.weights, np.float64).reshape(-1)
    a = np.ascontiguousarray(tps.A, np.float64).reshape(12)
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    q = np.zeros_like(p)
    if len(c) != len(w) or lib().sift3d_amd_tps_apply(c, w, a, len(c) // 3, p.reshape(-1), len(p),
                                                      q.reshape(-1)) != 0:
        raise ValueError("tps_apply: bad arguments")
    return q


def tps_pack(ctrl, weights):
    """The device layout of the control points (sift3d_amd_tps_pack): float32 [m, 8]."""
    c = np.ascontiguousarray(ctrl, np.float64).reshape(-1)
    w = np.ascontiguousarray(weights, np.float64).reshape(-1)
    m = len(c) // 3
    out = np.zeros((max(m, 1), 8), np.float32)
    if len(c) != len(w) or len(c) != 3 * m or lib().sift3d_amd_tps_pack(c, w, m, out.reshape(-1)) != 0:
        raise ValueError("tps_pack: bad control points or weights")
    return out


def warp_tps(image_or_array, tps, out_shape, interp="linear", fill=0.0):
    """Resample a host volume (an Image, or a float32 array [nz, ny, nx]) into a grid of
    out_shape = (oz, oy, ox) through the thin-plate spline tps (a pull map in voxels) with
    sift3d_amd_image_warp_tps.  Returns an Image for an Image, an array for an array."""
    if interp not in INTERP:
        raise ValueError("interp must be 'nearest' or 'linear', not %r" % (interp,))
    a = np.ascontiguousarray(tps.A, np.float64).reshape(12).copy()
    packed = tps_pack(tps.ctrl, tps.weights)
    src = image_or_array if isinstance(image_or_array, Image) else Image.from_array(image_or_array)
    oz, oy, ox = out_shape
    dst = Image(ox, oy, oz)
    if lib().sift3d_amd_image_warp_tps(src.h, a, packed.reshape(-1), len(packed), INTERP[interp], float(fill),
                                       dst.h) != 0:
        raise RuntimeError("sift3d_amd_image_warp_tps failed")
    return dst if isinstance(image_or_array, Image) else dst.data().copy()


DeformableRegistration = collections.namedtuple("DeformableRegistration", "A tps inliers num_matches warped")

# Defaults chosen on the end-to-end test (tests/test_tps.py, a 176^3 lattice under a rotation and bumps of 4
# voxels; swept over err_thresh 3 / 5 / 8 and smoothing 0 .. 100 on an MI355X).  Inliers must admit the
# non-affine part of the displacement, so the RANSAC threshold is wider than register's 3.0 (3.0 kept 488 of
# 611 matches, 5.0 569; 5.0 gave the best NCC and error, 8.0 worse).  The keypoints sit on whole voxels, so a spline through them
# (smoothing 0) follows half-voxel noise: smoothing 30 (in the units of phi(r) = -r, voxels) halved the p90 error
# at the keypoints and gave the best NCC (0.985 against 0.973 at 0 and 0.933 for the affine).
DEFORMABLE_ERR_THRESH = 5.0
DEFORMABLE_SMOOTHING = 30.0


def register_deformable(moving, fixed, nn_thresh=0.8, err_thresh=DEFORMABLE_ERR_THRESH, num_iter=500, seed=1,
                        smoothing=DEFORMABLE_SMOOTHING, max_control_points=2048, rematch=None, **detector_kw):
    """Deformable registration of two volumes (torch CUDA float32 tensors [nz, ny, nx]): detect +
    describe both, match, fit the moving -> fixed affine by RANSAC (err_thresh), then fit a
    thin-plate spline fixed -> moving through the RANSAC inliers (smoothing, at most
    max_control_points of them) and resample `moving` into `fixed`'s grid through it.  Returns
    DeformableRegistration(A (3 x 4, moving voxel -> fixed voxel), tps (TPS, fixed voxel -> moving voxel),
    inliers (mask over the matches), num_matches, warped (tensor shaped like fixed)).
    rematch: register's; the spline then goes through the inliers of the guided matches, and the result is the
    GuidedDeformableRegistration sibling with `first` behind it."""
    import torch
    from . import hip
    p_mov, p_fix, first = _matched_points_guided(moving, fixed, nn_thresh, detector_kw, "register_deformable", rematch,
                                                 err_thresh, num_iter, seed)
    A, inl = ransac_affine(p_mov, p_fix, err_thresh, num_iter, seed)
    tps = tps_fit(p_fix[inl], p_mov[inl], smoothing, max_control_points)
    warped = torch.empty_like(fixed)
    hip.warp_tps(moving, warped, tps, "linear")
    return _with_first(DeformableRegistration(A, tps, inl, len(p_mov), warped), first)


# ---- displacement fields: export, resampling through a field, Jacobian -----------------------------
JacobianStats = collections.namedtuple("JacobianStats", "det folded min max")


def displacement_field(transform, out_shape, device=None):
    """The displacement field u [3, oz, oy, ox] (channels x, y, z; source voxels) of a pull map over a grid of
    out_shape = (oz, oy, ox): output voxel p reads the source at p + u(p).  transform: a 3 x 4 affine pull map
    or a TPS (contract: include/sift3d_amd.h, "Displacement fields").  Returns a torch CUDA float32 tensor on
    `device` (default: the current device), computed on torch's current stream."""
    import torch
    from . import hip
    oz, oy, ox = (int(v) for v in out_shape)
    field = torch.empty((3, oz, oy, ox), dtype=torch.float32, device=device if device is not None else "cuda")
    if isinstance(transform, TPS):
        return hip.tps_field(field, transform)
    A = np.asarray(transform, np.float64)
    if A.shape not in ((3, 4), (12,)):
        raise ValueError("displacement_field: transform must be a 3 x 4 affine pull map or a TPS")
    return hip.affine_field(field, A)


def _host_field(field, what):
    f = np.ascontiguousarray(field, np.float32)
    if f.ndim != 4 or f.shape[0] != 3:
        raise ValueError("%s: the field must be [3, oz, oy, ox]" % what)
    return f


def warp_field(volume, field, interp="linear", fill=0.0):
    """Resample `volume` through a displacement field [3, oz, oy, ox]: output voxel p takes the volume at
    p + field(p); voxels that sample outside get `fill`.  A torch CUDA tensor [nz, ny, nx] or [nc, nz, ny, nx]
    (with a CUDA field) gives a tensor [oz, oy, ox] / [nc, oz, oy, ox] on torch's current stream; an Image or
    a float32 array (with a host field) goes through the blocking host form, and gives an Image / an array
    (a 4-D array channel by channel)."""
    if interp not in INTERP:
        raise ValueError("interp must be 'nearest' or 'linear', not %r" % (interp,))
    if _torch_tensor(volume):
        import torch
        from . import hip
        out = torch.empty(tuple(volume.shape[:-3]) + tuple(field.shape[1:]), dtype=torch.float32,
                          device=volume.device)
        return hip.warp_field(volume, out, field, interp, fill)
    f = _host_field(field, "warp_field")
    if not isinstance(volume, Image) and np.ndim(volume) == 4:
        return np.stack([warp_field(v, f, interp, fill) for v in np.asarray(volume)])
    src = volume if isinstance(volume, Image) else Image.from_array(volume)
    _, oz, oy, ox = f.shape
    dst = Image(ox, oy, oz)
    if lib().sift3d_amd_image_warp_field(src.h, f.reshape(-1), INTERP[interp], float(fill), dst.h) != 0:
        raise RuntimeError("sift3d_amd_image_warp_field failed")
    return dst if isinstance(volume, Image) else dst.data().copy()


def jacobian_determinant(field):
    """Jacobian determinant of p -> p + field(p) by numpy.gradient's differences (contract:
    include/sift3d_amd.h, "Displacement fields"): JacobianStats(det [oz, oy, ox], folded = the number of voxels
    with det <= 0 or NaN, min, max of the non-NaN dets).  A CUDA field gives a CUDA det (waits for torch's
    current stream to read the stats); a host array gives a numpy det (blocking)."""
    if _torch_tensor(field):
        import torch
        from . import hip
        det = torch.empty(tuple(field.shape[1:]), dtype=torch.float32, device=field.device)
        return JacobianStats(*hip.jacobian_det(field, det))
    f = _host_field(field, "jacobian_determinant")
    _, oz, oy, ox = f.shape
    det = np.empty((oz, oy, ox), np.float32)
    folded, mn, mx = C.c_uint64(), C.c_float(), C.c_float()
    if lib().sift3d_amd_jacobian_det(f.reshape(-1), ox, oy, oz, det.ctypes.data, C.byref(folded), C.byref(mn),
                                     C.byref(mx)) != 0:
        raise RuntimeError("sift3d_amd_jacobian_det failed")
    return JacobianStats(det, int(folded.value), float(mn.value), float(mx.value))


# ---- cubic B-spline resampling --------------------------------------------------------------------
def spline_coefficients(volume):
    """The cubic B-spline coefficients of a volume (contract: include/sift3d_amd.h, "Cubic B-spline resampling";
    whole-sample mirror boundaries, scipy's spline_filter(order=3, mode="mirror")).  A torch CUDA tensor
    [nz, ny, nx] or [nc, nz, ny, nx] gives a tensor on torch's current stream; an Image or a float32 array goes
    through the blocking host form and gives an array."""
    if _torch_tensor(volume):
        from . import hip
        return hip.bspline_prefilter(volume)
    src = volume.data() if isinstance(volume, Image) else volume
    src = np.ascontiguousarray(src, np.float32)
    if src.ndim not in (3, 4):
        raise ValueError("spline_coefficients: the volume must be [nz, ny, nx] or [nc, nz, ny, nx]")
    nc = src.shape[0] if src.ndim == 4 else 1
    nz, ny, nx = src.shape[-3:]
    out = np.empty_like(src)
    if lib().sift3d_amd_bspline_prefilter(src.reshape(-1), nx, ny, nz, nc, out.reshape(-1)) != 0:
        raise RuntimeError("sift3d_amd_bspline_prefilter failed")
    return out


def _affine_or_none(transform):
    """the transform as a 3 x 4 float64 array when it is shaped like an affine pull map, else None (a field is not
    converted to look at it)"""
    try:
        if np.shape(transform) not in ((3, 4), (12,)):
            return None
        return np.asarray(transform, np.float64).reshape(3, 4)
    except (TypeError, ValueError):
        return None


def _field_out_shape(out_shape, grid):
    if out_shape is not None and tuple(int(v) for v in out_shape) != tuple(int(v) for v in grid):
        raise ValueError("resample_cubic: out_shape %s is not the field's grid %s" % (tuple(out_shape), tuple(grid)))


def resample_cubic(volume, transform, out_shape=None, fill=0.0, prefiltered=False):
    """Resample `volume` with the cubic B-spline interpolant (scipy order 3, mode "mirror" inside the grid): sharper
    than the linear warps, which blur at every pass.  transform: a 3 x 4 affine pull map, a TPS (both need out_shape
    = (oz, oy, ox)) or a displacement field [3, oz, oy, ox], whose grid is the output's (out_shape may be omitted;
    ValueError when it is given and differs); a TPS is exported with displacement_field and sampled through that
    field.  Voxels that sample outside the volume get `fill`.  prefiltered=True: `volume` already holds
    spline_coefficients(volume), so that one prefilter serves many resamples of one volume.
    A torch CUDA tensor [nz, ny, nx] or, through a TPS or a field, [nc, nz, ny, nx] gives a tensor on torch's current
    stream; an Image or a float32 array [nz, ny, nx] goes through the blocking host forms (an affine or a host field;
    not prefiltered) and gives an Image / an array."""
    A = None if isinstance(transform, TPS) or _torch_tensor(transform) else _affine_or_none(transform)
    if (A is not None or isinstance(transform, TPS)) and out_shape is None:
        raise ValueError("resample_cubic: an affine or a TPS transform needs out_shape")
    if _torch_tensor(volume):
        import torch
        from . import hip
        if volume.dim() not in (3, 4):
            raise ValueError("resample_cubic: the volume must be [nz, ny, nx] or [nc, nz, ny, nx]")
        if A is None:
            if isinstance(transform, TPS):
                transform = displacement_field(transform, out_shape, volume.device)
            if not _torch_tensor(transform):
                raise ValueError("resample_cubic: transform must be a 3 x 4 affine pull map, a TPS or a CUDA field "
                                 "[3, oz, oy, ox]")
        elif volume.dim() != 3:
            raise ValueError("resample_cubic: an affine transform takes a volume [nz, ny, nx]; resample a "
                             "multi-channel volume through displacement_field(A, out_shape)")
        coef = volume if prefiltered else hip.bspline_prefilter(volume)
        if A is not None:
            out = torch.empty(tuple(int(v) for v in out_shape), dtype=torch.float32, device=volume.device)
            return hip.bspline_warp_affine(coef, out, A, fill)
        hip._field_tensor(transform, "resample_cubic", "transform")
        _field_out_shape(out_shape, transform.shape[1:])
        out = torch.empty(tuple(volume.shape[:-3]) + tuple(transform.shape[1:]), dtype=torch.float32,
                          device=volume.device)
        return hip.bspline_warp_field(coef, out, transform, fill)
    if prefiltered:
        raise ValueError("resample_cubic: prefiltered=True takes a CUDA tensor of coefficients")
    if isinstance(transform, TPS):
        raise ValueError("resample_cubic: a host volume takes an affine or a host field; export the TPS with "
                         "displacement_field(...).cpu().numpy()")
    src = volume if isinstance(volume, Image) else Image.from_array(volume)
    if len(src.shape) != 3:
        raise ValueError("resample_cubic: the image must have one channel")
    if A is not None:
        oz, oy, ox = (int(v) for v in out_shape)
        dst = Image(ox, oy, oz)
        if lib().sift3d_amd_image_bspline_warp_affine(src.h, np.ascontiguousarray(A).reshape(12), float(fill),
                                                      dst.h) != 0:
            raise RuntimeError("sift3d_amd_image_bspline_warp_affine failed")
    else:
        f = _host_field(transform, "resample_cubic")
        _field_out_shape(out_shape, f.shape[1:])
        _, oz, oy, ox = f.shape
        dst = Image(ox, oy, oz)
        if lib().sift3d_amd_image_bspline_warp_field(src.h, f.reshape(-1), float(fill), dst.h) != 0:
            raise RuntimeError("sift3d_amd_image_bspline_warp_field failed")
    return dst if isinstance(volume, Image) else dst.data().copy()


# ---- similarity measures ---------------------------------------------------------------------------
Similarity = collections.namedtuple("Similarity",
                                    "count msd ncc mi nmi entropy_fixed entropy_moving entropy_joint joint")
LabelOverlap = collections.namedtuple("LabelOverlap", "confusion dice jaccard volume_fixed volume_moving")
SIMILARITY_MAX_BINS = 128


def similarity_measures(hist, stats):
    """The measures of a joint histogram [B, B] (counts, indexed [b_fixed, b_moving]) and a moments record (count,
    [sum f, sum m, sum f f, sum m m, sum f m, sum (f - m)^2]) by sift3d_amd_similarity_measures (host, double):
    Similarity(count, msd, ncc, mi, nmi, entropy_fixed, entropy_moving, entropy_joint, joint = the histogram as
    int64).  Everything but the count is NaN when the count is 0."""
    h = np.ascontiguousarray(hist).astype(np.uint64)
    if h.ndim != 2 or h.shape[0] != h.shape[1]:
        raise ValueError("similarity_measures: the histogram must be [B, B]")
    count, sums = stats
    rec = np.zeros(7, np.float64)
    rec[:1].view(np.uint64)[0] = int(count)
    rec[1:] = np.asarray(sums, np.float64).reshape(6)
    out = _Measures()
    if lib().sift3d_amd_similarity_measures(h.reshape(-1), h.shape[0], rec.ctypes.data, C.byref(out)) != 0:
        raise RuntimeError("sift3d_amd_similarity_measures failed")
    return Similarity(int(out.n), out.msd, out.ncc, out.mi, out.nmi, out.entropy_fixed, out.entropy_moving,
                      out.entropy_joint, h.astype(np.int64))


def _similarity_volume(v, what, name, device=None):
    """a volume as a CUDA float32 tensor [nz, ny, nx]: a tensor as it is, an Image or an array uploaded"""
    import torch
    if not _torch_tensor(v):
        a = np.ascontiguousarray(v.data() if isinstance(v, Image) else v, np.float32)
        if a.ndim != 3:
            raise ValueError("%s: %s must be a volume [nz, ny, nx]" % (what, name))
        if not device_available():
            raise RuntimeError("%s: no HIP device is available; this library has no CPU path" % what)
        v = torch.from_numpy(a).to(device if device is not None else "cuda")
    _volume_tensor(v, what, name)
    return v


def _similarity_transform(transform, fixed, what):
    """None, a 3 x 4 float64 array, or a CUDA field on the fixed grid (a TPS exported, a host field uploaded)"""
    import torch
    if transform is None or _torch_tensor(transform):
        return transform
    if isinstance(transform, TPS):
        return displacement_field(transform, tuple(fixed.shape), fixed.device)
    A = _affine_or_none(transform)
    if A is not None:
        return A
    return torch.from_numpy(_host_field(transform, what)).to(fixed.device)


def _range_accepted(lo, hi, bins):
    """bin_scale() of the entries (sift3d_similarity.c) != 0: both ends finite floats, lo < hi, bins / (hi - lo) finite"""
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        lo, hi = np.float32(lo), np.float32(hi)
        if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
            return False
        s = np.float32(bins) / (hi - lo)
    return bool(np.isfinite(s) and s > 0)


def _own_range(v, given, bins=SIMILARITY_MAX_BINS):
    """(lo, hi) as given, else the volume's own min and max (one host synchronisation); hi = lo + 1 when constant.
    Where the entries would refuse that pair as floats (a constant beyond 2**24, whose lo + 1 rounds to lo; a span too
    narrow for bins / (hi - lo)) the range is widened by doubling until they accept it: upwards from lo, or downwards
    from hi where the float range ends above.  It always contains [min, max].  ValueError for a volume that is not
    finite or whose max - min overflows float."""
    import torch
    if given is not None:
        lo, hi = given
        return float(lo), float(hi)
    lo, hi = (float(t) for t in torch.aminmax(v))
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError("the volume must be finite to take its own range (min %r, max %r)" % (lo, hi))
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 2 <= bins <= SIMILARITY_MAX_BINS:
        bins = SIMILARITY_MAX_BINS                            # (the entry refuses such a count itself)
    pair = (lo, hi) if hi > lo else (lo, lo + 1.0)
    if _range_accepted(*pair, bins):
        return pair
    fmax = float(np.finfo(np.float32).max)
    if hi - lo > fmax:
        raise ValueError("the volume's own range [%r, %r] is wider than the largest float: give a range" % (lo, hi))
    for up in (True, False):
        w = max(pair[1] - pair[0], abs(lo) * 2.0 ** -52, 2.0 ** -150)       # (lo + 1.0 may be lo in double as well)
        while w <= 2.0 * fmax:
            w *= 2.0
            wide = (lo, lo + w) if up else (hi - w, hi)
            if _range_accepted(*wide, bins):
                return wide
    raise ValueError("the volume's own range [%r, %r] cannot be widened within float: give a range" % (lo, hi))


def _mask_host(mask, volume, what, name):
    """A region-of-interest mask (contract: include/sift3d_amd.h, "Masks") checked against its volume before anything
    is uploaded: None, a CUDA tensor as it is, or a float32 array.  bool and integer masks become float32 (mask != 0),
    float masks pass as they are (in where >= 0.5).  ValueError on a wrong shape or kind, or on a tensor that is not on
    the volume's device (the fixed volume's, where both are tensors)."""
    import torch
    if mask is None:
        return None
    vshape = tuple(volume.shape) if isinstance(volume, Image) or _torch_tensor(volume) else tuple(np.shape(volume))
    if _torch_tensor(mask):
        if not mask.is_cuda or (_torch_tensor(volume) and mask.device != volume.device):
            raise ValueError("%s: %s must be on the fixed volume's device, not %s" % (what, name, mask.device))
        if mask.dtype == torch.bool or not mask.dtype.is_floating_point:
            if mask.dtype.is_complex:
                raise ValueError("%s: %s must be a bool, integer or float mask" % (what, name))
            mask = mask != 0
        w = mask.to(torch.float32).contiguous()
    else:
        a = np.asarray(mask.data() if isinstance(mask, Image) else mask)
        if a.dtype == np.bool_ or np.issubdtype(a.dtype, np.integer):
            a = a != 0
        elif not np.issubdtype(a.dtype, np.floating):
            raise ValueError("%s: %s must be a bool, integer or float mask" % (what, name))
        w = np.ascontiguousarray(a, np.float32)
    if tuple(w.shape) != vshape:
        raise ValueError("%s: %s must have its volume's shape %s, not %s" % (what, name, vshape, tuple(w.shape)))
    return w


def _mask_tensor(w, like, what, name):
    """_mask_host's result on the device of the uploaded volume `like`"""
    import torch
    if w is None:
        return None
    if not _torch_tensor(w):
        return torch.from_numpy(w).to(like.device)
    if w.device != like.device:
        raise ValueError("%s: %s must be on the fixed volume's device, not %s" % (what, name, w.device))
    return w


def _stack_tensor(v, what, name, device=None):
    """a channel stack as a contiguous CUDA float32 tensor [nc, nz, ny, nx]: a tensor as it is, an array uploaded"""
    import torch
    from . import hip
    if not _torch_tensor(v):
        a = np.ascontiguousarray(v, np.float32)
        if not device_available():
            raise RuntimeError("%s: no HIP device is available; this library has no CPU path" % what)
        v = torch.from_numpy(a).to(device if device is not None else "cuda")
    hip._tensor(v, "%s: %s must be a contiguous float32 CUDA tensor [nc, nz, ny, nx]" % (what, name), dims=(4,))
    return v


def similarity(fixed, moving, transform=None, bins=64, interp="linear", range_fixed=None, range_moving=None,
               mask_fixed=None, mask_moving=None):
    """How well `fixed` agrees with `moving` seen through a pull map, in one pass on the device (contract:
    include/sift3d_amd.h, "Similarity measures"): the fixed voxels whose sample falls inside `moving` give
    Similarity(count, msd, ncc, mi, nmi, entropy_fixed, entropy_moving, entropy_joint, joint [bins, bins] int64
    indexed [b_fixed, b_moving]); mutual information and the entropies in nats from the joint histogram.
    transform: None (the identity; equal shapes), a 3 x 4 affine pull map, a TPS (exported with
    displacement_field) or a displacement field [3, oz, oy, ox] on the fixed grid.  The volumes are torch CUDA
    float32 tensors [nz, ny, nx], or Images / arrays, which are uploaded.  A range left None is that volume's own
    min and max, at the cost of one host synchronisation (a constant volume gets hi = lo + 1; a pair too narrow for
    the bins in float is widened until it is not; ValueError for a volume that is not finite or whose max - min
    overflows float); values outside a given range count in the end bins.  mask_fixed, mask_moving: regions of interest of the volumes' shapes (tensors,
    arrays or Images; bool and integer masks are in where non-zero, float masks where >= 0.5): a fixed voxel counts only
    where mask_fixed is in and mask_moving, at the nearest voxel to its sample point, is in too (contract: "Masks").  A
    range left None is still the whole volume's.  Reads the result, so it waits for torch's current stream."""
    from . import hip
    WF = _mask_host(mask_fixed, fixed, "similarity", "mask_fixed")
    WM = _mask_host(mask_moving, moving, "similarity", "mask_moving")
    F = _similarity_volume(fixed, "similarity", "fixed")
    M = _similarity_volume(moving, "similarity", "moving", F.device)
    WF = _mask_tensor(WF, F, "similarity", "mask_fixed")
    WM = _mask_tensor(WM, F, "similarity", "mask_moving")
    T = _similarity_transform(transform, F, "similarity")
    hist, stats = hip.similarity(F, M, T, bins, _own_range(F, range_fixed, bins), _own_range(M, range_moving, bins),
                                 interp, mask_fixed=WF, mask_moving=WM)
    return similarity_measures(hist.cpu().numpy(), hip.similarity_stats(stats))


LocalNcc = collections.namedtuple("LocalNcc", "value count map")
LNCC_MAX_RADIUS = 4


def _lncc_radius(radius, what):
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= radius <= LNCC_MAX_RADIUS:
        raise ValueError("%s: radius must be an integer in 1 .. %d, not %r" % (what, LNCC_MAX_RADIUS, radius))
    return int(radius)


def local_ncc(fixed, moving, transform=None, radius=2, mask_fixed=None, mask_moving=None, return_map=False):
    """The local (windowed) squared cross-correlation of `fixed` and `moving` seen through a pull map (contract:
    include/sift3d_amd.h, "Local cross-correlation"; the CC metric of ANTs): per fixed voxel the squared correlation
    of the two volumes over the (2 radius + 1)^3 window around it, which does not change under a gain and offset that
    vary slowly in space.  Returns LocalNcc(value = the mean over the counted voxels (NaN when nothing is counted),
    count, map = the float32 map [nz, ny, nx] as a CUDA tensor when return_map, else None).  A voxel is counted where
    it samples inside `moving`, is in both masks, has a second valid voxel in its window and neither volume is flat
    there.  transform: as similarity's (None, a 3 x 4 pull map, a TPS or a displacement field); it is turned into a
    field with displacement_field and `moving` is warped with warp_field (linear, fill 0).  The volumes and masks: as
    similarity's.  Reads the result, so it waits for torch's current stream."""
    import torch
    from . import hip
    r = _lncc_radius(radius, "local_ncc")
    WF = _mask_host(mask_fixed, fixed, "local_ncc", "mask_fixed")
    WM = _mask_host(mask_moving, moving, "local_ncc", "mask_moving")
    shapes = [tuple(v.shape) if hasattr(v, "shape") else tuple(np.shape(v)) for v in (fixed, moving)]
    if transform is None and shapes[0] != shapes[1]:
        raise ValueError("local_ncc: without a transform fixed %s and moving %s must have one shape" % tuple(shapes))
    F = _similarity_volume(fixed, "local_ncc", "fixed")
    M = _similarity_volume(moving, "local_ncc", "moving", F.device)
    WF = _mask_tensor(WF, F, "local_ncc", "mask_fixed")
    WM = _mask_tensor(WM, F, "local_ncc", "mask_moving")
    T = _similarity_transform(transform, F, "local_ncc")
    if T is None:
        u = torch.zeros((3,) + tuple(F.shape), dtype=torch.float32, device=F.device)
    elif _torch_tensor(T):
        hip._field_tensor(T, "local_ncc")
        if tuple(T.shape[1:]) != tuple(F.shape):
            raise ValueError("local_ncc: the field %s is not on the fixed grid %s" % (tuple(T.shape), tuple(F.shape)))
        u = T
    else:
        u = displacement_field(T, tuple(F.shape), F.device)
    W = warp_field(M, u, "linear", 0.0)
    cc = torch.empty(tuple(F.shape), dtype=torch.float32, device=F.device) if return_map else None
    stats = hip.lncc(F, W, u, r, tuple(M.shape), cc=cc, mask_fixed=WF, mask_moving=WM)
    sums, counts = hip.demons_stats(stats)
    return LocalNcc(float(_mean_or_nan(sums, counts)[0]), int(counts[0]), cc)


# ---- intensity-driven affine refinement ----------------------------------------------------------
AffineRefinement = collections.namedtuple(
    "AffineRefinement", "A msd count accepted lambdas levels level_slices evaluations stop warped")
RefinedRegistration = collections.namedtuple("RefinedRegistration",
                                             "A inliers num_matches warped A_ransac refinement")
# the registration results after a guided second match (rematch=): the same fields, then the first pass
GUIDED_REGISTRATIONS = {k: collections.namedtuple("Guided" + k.__name__, k._fields + ("first",))
                        for k in (Registration, RefinedRegistration, DeformableRegistration)}
NccAffineRefinement = collections.namedtuple(
    "NccAffineRefinement", "A cost count accepted lambdas levels level_slices evaluations stop warped ncc gain offset")
MiAffineRefinement = collections.namedtuple(
    "MiAffineRefinement", "A cost count accepted lambdas levels level_slices evaluations stop warped mi nmi bins")
MI_BINS = 32
AFFINE_FREE = {"affine": 0xFFF, "translation": 0x888}


def _mi_bins(what, bins):
    """bins of metric="mi" (None: MI_BINS), an integer in [4, hip.PARZEN_MAX_BINS]"""
    from . import hip
    bins = MI_BINS if bins is None else bins
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 4 <= int(bins) <= hip.PARZEN_MAX_BINS:
        raise ValueError("%s: bins must be in [4, %d]" % (what, hip.PARZEN_MAX_BINS))
    return bins


def _mi_ranges(what, range_fixed, range_moving):
    """each range of metric="mi" is None (the volume's own) or finite (lo, hi) with lo < hi as float32"""
    for r, name in ((range_fixed, "range_fixed"), (range_moving, "range_moving")):
        if r is not None:
            lo, hi = (float(np.float32(v)) for v in r)
            if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
                raise ValueError("%s: %s must be finite with lo < hi" % (what, name))


def _levels_and_evaluations(what, levels, params, max_evaluations):
    """levels an integer in [1, hip.AFFINE_MAX_LEVELS]; params' max_evaluations, where given, in [1, max_evaluations]"""
    from . import hip
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or \
            not 1 <= int(levels) <= hip.AFFINE_MAX_LEVELS:
        raise ValueError("%s: levels must be in [1, %d]" % (what, hip.AFFINE_MAX_LEVELS))
    if "max_evaluations" in params and not 1 <= int(params["max_evaluations"]) <= max_evaluations:
        raise ValueError("%s: max_evaluations must be in [1, %d]" % (what, max_evaluations))


AffineInit = collections.namedtuple(
    "AffineInit", "A cost count index candidates costs counts centroid_fixed centroid_moving axes_fixed axes_moving "
                  "order")
INIT_BINS = 32


def _init_keywords(init, what, **defaults):
    """init_affine's keyword arguments from an `init` argument: a mode name or a dict of them; `defaults` fill in what
    it leaves out"""
    if isinstance(init, str):
        kw = dict(mode=init)
    elif isinstance(init, dict):
        kw = dict(init)
    else:
        raise ValueError("%s: init must be a mode name ('centroid', 'axes', 'search') or a dict of init_affine's "
                         "keyword arguments, not %r" % (what, init))
    for k, v in defaults.items():
        if v is not None:
            kw.setdefault(k, v)
    return kw


def init_affine(moving, fixed, mode="search", metric="mi", levels=3, weight="binary", floor_fixed=None,
                floor_moving=None, mask_fixed=None, mask_moving=None, bins=None, range_fixed=None, range_moving=None,
                **search):
    """A start for refine_affine made from the two volumes alone (contract: include/sift3d_amd.h, "Initial transforms:
    moments and candidate search"): rigid candidate pull maps (fixed voxel -> moving voxel) about the two centres of
    mass, all scored by `metric` ("msd", "ncc", "mi") in one call on volumes restricted levels - 1 times (fewer where an
    axis would fall below 8), the best one returned on the full grids.  mode: "centroid" (the centres aligned, no
    rotation), "axes" (that, and the four proper rotations that map the fixed volume's principal axes onto the moving
    volume's), "search" (a grid of rotations Rz Ry Rx and offsets: range_deg and range_vox (a number or three, about /
    along x, y, z), step_deg, step_vox; the defaults, 90 degrees by 30 and no offsets, make 343 candidates).  The
    moments are taken over the voxels above a floor (None: the volume's minimum, one host synchronisation), with
    weight "binary" (geometric: what two modalities share) or "intensity".  bins (None: 32) and range_fixed,
    range_moving (None: the volume's own) are the histogram's for "mi".  min_overlap (0.5): a candidate must count that
    share of the best-overlapping candidate's voxels.  mask_fixed, mask_moving: as similarity's; they bound the moments
    too.  Returns AffineInit(A, cost, count, index: of the best candidate; candidates [K, 3, 4]: all of them on the full
    grids; costs, counts [K]; centroid_fixed, centroid_moving (x, y, z), axes_fixed, axes_moving (rows); order: the best
    candidates by ascending cost, 16 at most).  RuntimeError where a volume has nothing above its floor or no candidate
    is eligible."""
    from . import hip
    what = "init_affine"
    if metric not in hip.INIT_METRIC:
        raise ValueError("%s: metric must be 'msd', 'ncc' or 'mi', not %r" % (what, metric))
    if mode not in hip.INIT_MODE:
        raise ValueError("%s: mode must be 'centroid', 'axes' or 'search', not %r" % (what, mode))
    if weight not in hip.MOMENTS_WEIGHT:
        raise ValueError("%s: weight must be 'binary' or 'intensity', not %r" % (what, weight))
    if metric != "mi" and not (bins is None and range_fixed is None and range_moving is None):
        raise ValueError("%s: bins, range_fixed and range_moving belong to metric='mi', not %r" % (what, metric))
    for k in search:
        if k not in ("range_deg", "step_deg", "range_vox", "step_vox", "min_overlap"):
            raise ValueError("%s: unknown parameter %r" % (what, k))
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or \
            not 1 <= int(levels) <= hip.AFFINE_MAX_LEVELS:
        raise ValueError("%s: levels must be in [1, %d]" % (what, hip.AFFINE_MAX_LEVELS))
    if metric == "mi":
        bins = INIT_BINS if bins is None else bins
        if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or \
                not 2 <= int(bins) <= hip.SIMILARITY_MAX_BINS:
            raise ValueError("%s: bins must be in [2, %d]" % (what, hip.SIMILARITY_MAX_BINS))
        _mi_ranges(what, range_fixed, range_moving)
    WF = _mask_host(mask_fixed, fixed, what, "mask_fixed")
    WM = _mask_host(mask_moving, moving, what, "mask_moving")
    F = _similarity_volume(fixed, what, "fixed")
    M = _similarity_volume(moving, what, "moving", F.device)
    WF = _mask_tensor(WF, F, what, "mask_fixed")
    WM = _mask_tensor(WM, F, what, "mask_moving")
    kw = dict(mode=mode, metric=metric, levels=int(levels), weight=weight, **search)
    kw["floor_f"] = float(F.min()) if floor_fixed is None else float(floor_fixed)
    kw["floor_m"] = float(M.min()) if floor_moving is None else float(floor_moving)
    if metric == "mi":
        (kw["lo_f"], kw["hi_f"]) = _own_range(F, range_fixed, int(bins))
        (kw["lo_m"], kw["hi_m"]) = _own_range(M, range_moving, int(bins))
        kw["bins"] = int(bins)
    p = hip.affine_init_params(**kw)
    res, costs, counts = hip.affine_init(F, M, p, mask_fixed=WF, mask_moving=WM)
    # every candidate on the full grids, as the driver made them on the coarsest: the frames and offsets there (exact:
    # powers of two), the translation column back up
    scale = 2.0 ** (res.levels - 1)
    frames = [(np.array(f.centroid[:]) / scale, np.array(f.axes[:]), np.array(f.lambda_[:]))
              for f in (res.frame_f, res.frame_m)]
    kw["range_vox"] = np.array(p.range_vox[:]) / scale
    kw["step_vox"] = p.step_vox / scale
    cands = hip.affine_init_candidates(mode, frames[0], frames[1], hip.affine_init_params(**kw))
    cands[:, :, 3] *= scale
    return AffineInit(np.array(res.A[:], np.float64).reshape(3, 4), float(res.cost), int(res.n), int(res.index), cands,
                      costs, counts.astype(np.int64), np.array(res.frame_f.centroid[:]),
                      np.array(res.frame_m.centroid[:]), np.array(res.frame_f.axes[:]).reshape(3, 3),
                      np.array(res.frame_m.axes[:]).reshape(3, 3), np.array(res.keep_index[:res.kept], np.int64))


def refine_affine(moving, fixed, A=None, levels=1, free="affine", interp="linear", mask_fixed=None, mask_moving=None,
                  metric="msd", bins=None, range_fixed=None, range_moving=None, init=None, **params):
    """Move the 3 x 4 affine pull map A (fixed voxel -> moving voxel, as similarity's transform; None: the identity,
    which needs no equal shapes) towards a smaller mean squared difference between `fixed` and `moving` seen through
    it, by Levenberg-Marquardt steps on the device's Gauss-Newton normal equations (contract: include/sift3d_amd.h,
    "Intensity-driven affine refinement").  free: "affine" (all 12 parameters), "translation", or a mask whose bit
    4 d + j frees A[d][j] as centred on the fixed grid.  levels > 1 solves on volumes restricted levels - 1 times
    first.  params: max_evaluations (per level), lambda0, lambda_factor, lambda_min, lambda_max, tol (voxels),
    min_overlap.  The sample is linear.  The volumes are torch CUDA float32 tensors [nz, ny, nx], or Images / arrays,
    which are uploaded.  mask_fixed, mask_moving: regions of interest as similarity's; only voxels in both drive the
    steps and count towards min_overlap, and coarser levels use the restricted masks.  Returns AffineRefinement(A, msd,
    count, accepted, lambdas, levels: one entry per evaluation in the order run; level_slices: {level: slice into
    those}; evaluations; stop: "converged", "lambda", "evaluations" or "lm_failed" of level 0; warped: `moving` through
    A on the fixed grid).  Waits for torch's current stream once per evaluation.
    metric="ncc" fits a linear intensity map together with A, minimising sum (gain * m + offset - f)^2 over the three
    (Gauss-Newton on 1 - ncc^2; contract: "Affine refinement under a linear intensity map (NCC)"), so the result does
    not change under a gain (a negative one included) or an offset of either volume, where the MSD's does.  It returns
    NccAffineRefinement: AffineRefinement's fields with `cost` (the mean squared residual of the fit) in the place of
    `msd`, then ncc, gain and offset of the fit at the final A.  `warped` is still `moving` through A: its intensities
    are not remapped (gain * warped + offset is the fitted image).
    metric="mi" maximises the Mattes mutual information of the fixed bin and the Parzen-windowed moving bin (contract:
    "Mutual-information affine refinement (Mattes)"), for volumes whose intensities are related by an unknown map that
    need not be monotone (CT to MR, T1 to T2).  bins (None: 32; 4 .. 64) and range_fixed, range_moving ((lo, hi); None:
    the volume's own min and max, one host synchronisation each, widened and refused with ValueError as similarity's)
    set the histogram and are level 0's on every level.  It
    returns MiAffineRefinement: NccAffineRefinement's fields without gain and offset, `cost` = -mi per evaluation, then
    mi and nmi at the final A and bins; `warped` is `moving` through A, not remapped.  bins or a range with another
    metric, and any other metric, raise ValueError.
    init: a mode of init_affine ("centroid", "axes", "search") or a dict of its keyword arguments: the refinement then
    starts from init_affine's map, for pairs that the identity does not bring into the capture range.  Its metric,
    masks, bins and ranges default to the refinement's own.  Only with A=None: ValueError otherwise."""
    import torch
    from . import hip
    if metric not in ("msd", "ncc", "mi"):
        raise ValueError("refine_affine: metric must be 'msd', 'ncc' or 'mi', not %r" % (metric,))
    if init is not None and A is not None:
        raise ValueError("refine_affine: init makes the start itself; it goes with A=None only")
    if metric != "mi" and not (bins is None and range_fixed is None and range_moving is None):
        raise ValueError("refine_affine: bins, range_fixed and range_moving belong to metric='mi', not %r" % (metric,))
    if metric == "mi":
        bins = _mi_bins("refine_affine", bins)
        _mi_ranges("refine_affine", range_fixed, range_moving)
    if interp != "linear":
        raise ValueError("refine_affine: the sample is linear; interp=%r has no gradient" % (interp,))
    mask = AFFINE_FREE.get(free, free) if isinstance(free, str) else free
    if isinstance(mask, bool) or not isinstance(mask, (int, np.integer)) or not 1 <= int(mask) <= 0xFFF:
        raise ValueError("refine_affine: free must be 'affine', 'translation' or a mask in [1, 0xFFF], not %r"
                         % (free,))
    _levels_and_evaluations("refine_affine", levels, params, hip.AFFINE_MAX_EVALUATIONS)
    A0 = np.eye(3, 4) if A is None else _affine_or_none(A)
    if A0 is None or not np.isfinite(A0).all():
        raise ValueError("refine_affine: A must be a finite 3 x 4 affine pull map or None")
    p = hip.affine_refine_params(free_mask=int(mask), levels=int(levels), **params)
    WF = _mask_host(mask_fixed, fixed, "refine_affine", "mask_fixed")
    WM = _mask_host(mask_moving, moving, "refine_affine", "mask_moving")
    F = _similarity_volume(fixed, "refine_affine", "fixed")
    M = _similarity_volume(moving, "refine_affine", "moving", F.device)
    WF = _mask_tensor(WF, F, "refine_affine", "mask_fixed")
    WM = _mask_tensor(WM, F, "refine_affine", "mask_moving")
    if init is not None:
        mi = dict(bins=bins, range_fixed=range_fixed, range_moving=range_moving) if metric == "mi" else {}
        ikw = _init_keywords(init, "refine_affine", metric=metric, mask_fixed=WF, mask_moving=WM)
        if ikw["metric"] == "mi":
            ikw = _init_keywords(ikw, "refine_affine", **mi)
        A0 = init_affine(M, F, **ikw).A
    if metric == "ncc":
        res, fit = hip.affine_ncc_refine(F, M, A0, p, mask_fixed=WF, mask_moving=WM)
    elif metric == "mi":
        res, sim = hip.affine_mi_refine(F, M, A0, int(bins), _own_range(F, range_fixed, int(bins)),
                                        _own_range(M, range_moving, int(bins)), p, mask_fixed=WF, mask_moving=WM)
    else:
        res = hip.affine_refine(F, M, A0, p, mask_fixed=WF, mask_moving=WM)
    k = res.evaluations
    trail = res.trail[:k]
    lv = np.array([e.level for e in trail], np.int64)
    slices = {}
    for l in sorted(set(lv.tolist()), reverse=True):
        idx = np.nonzero(lv == l)[0]
        slices[l] = slice(int(idx[0]), int(idx[-1]) + 1)
    A1 = np.array(res.A[:], np.float64).reshape(3, 4)
    warped = torch.empty_like(F)
    hip.warp_affine(M, warped, A1, "linear")
    out = AffineRefinement(A1, np.array([e.msd for e in trail]), np.array([e.n for e in trail], np.int64),
                           np.array([bool(e.accepted) for e in trail]), np.array([e.lambda_ for e in trail]), lv,
                           slices, k, hip.AFFINE_STOPS[res.stop], warped)
    if metric == "ncc":
        return NccAffineRefinement(*out, ncc=float(fit[3]), gain=float(fit[0]), offset=float(fit[1]))
    if metric == "mi":
        return MiAffineRefinement(*out, mi=float(sim.mi), nmi=float(sim.nmi), bins=int(bins))
    return out


# ---- block matching -------------------------------------------------------------------------------
BlockMatches = collections.namedtuple("BlockMatches", "points_fixed points_moving cc variance")
TrimmedFit = collections.namedtuple("TrimmedFit", "A used iterations")
BlockRegistration = collections.namedtuple("BlockRegistration", "A warped trail stop")
BlockIteration = collections.namedtuple(
    "BlockIteration", "level A_in A_out n_valid n_selected n_used mean_cc rms move")
BLOCK_MODELS = ("translation", "rigid", "affine")


def _block_model(model, what):
    if model not in BLOCK_MODELS:
        raise ValueError("%s: model must be 'translation', 'rigid' or 'affine', not %r" % (what, model))
    return model


def _unit_fraction(v, what, name):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0 < v <= 1:
        raise ValueError("%s: %s must be in (0, 1], not %r" % (what, name, v))
    return float(v)


def _volume_shape(v):
    return tuple(int(n) for n in (v.shape if hasattr(v, "shape") else np.shape(v)))


def _affine_start(A, what, name="A"):
    A0 = np.eye(3, 4) if A is None else _affine_or_none(A)
    if A0 is None or not np.isfinite(A0).all():
        raise ValueError("%s: %s must be a finite 3 x 4 affine pull map or None" % (what, name))
    return A0


def block_match(fixed, moving, transform=None, radius=3, mask_fixed=None, mask_moving=None):
    """Match every 4^3 block of `fixed` to its best-correlated position in `moving` seen through the 3 x 4 pull map
    `transform` (None: the identity), inside a (2 radius + 1)^3 search cube with a sub-voxel step (contract:
    include/sift3d_amd.h, "Block matching").  The score is the squared local correlation, so a gain and offset that
    vary in space do not disturb it.  Returns BlockMatches(points_fixed: the centres of the valid blocks, n x 3 (x, y,
    z) in fixed voxels; points_moving: where each lands in `moving`, transform (centre + displacement); cc; variance:
    the block's sum of squared deviations, the key the driver selects blocks by).  A block is valid when it lies in
    mask_fixed, is not flat, and has a candidate that lies in the grid, in the warped mask_moving, and is not flat.
    The volumes and masks: as similarity's.  Reads the result, so it waits for torch's current stream."""
    import torch
    from . import hip
    what = "block_match"
    r = hip._block_radius(radius, what)
    A = _affine_start(transform, what, "transform")
    if len(_volume_shape(fixed)) == 3 and min(_volume_shape(fixed)) < 4:
        raise ValueError("%s: fixed %s must hold a block of 4 voxels on every axis" % (what, _volume_shape(fixed)))
    WF = _mask_host(mask_fixed, fixed, what, "mask_fixed")
    WM = _mask_host(mask_moving, moving, what, "mask_moving")
    F = _similarity_volume(fixed, what, "fixed")
    M = _similarity_volume(moving, what, "moving", F.device)
    WF = _mask_tensor(WF, F, what, "mask_fixed")
    WM = _mask_tensor(WM, F, what, "mask_moving")
    W = torch.empty_like(F)
    hip.warp_affine(M, W, A, "linear")
    VW = torch.empty_like(F)
    hip.warp_affine(WM if WM is not None else torch.ones_like(M), VW, A, "nearest")
    disp, cc, var = hip.block_match(F, W, r, WF, VW)
    cc = cc.cpu().numpy().reshape(-1)
    keep = np.nonzero(cc >= 0)[0]
    nbz, nby, nbx = var.shape
    centres = np.stack([4.0 * (keep % nbx) + 1.5, 4.0 * (keep // nbx % nby) + 1.5, 4.0 * (keep // (nbx * nby)) + 1.5], 1)
    q = centres + disp.cpu().numpy().reshape(3, -1)[:, keep].T.astype(np.float64)
    return BlockMatches(centres, q @ A[:, :3].T + A[:, 3], cc[keep], var.cpu().numpy().reshape(-1)[keep])


def fit_transform(src, dst, model="rigid", keep=0.5, spacing_src=None, spacing_dst=None, max_iter=20):
    """The least-trimmed-squares fit of a "translation", "rigid" or "affine" map dst ~ A [src; 1] to n x 3 point pairs
    (contract: "Block matching", the trimmed fit): fit, keep the ceil(keep n) pairs of smallest residual, refit, until
    the kept set repeats or max_iter refits.  Outliers below the share 1 - keep do not move the result.  spacing_src,
    spacing_dst: voxel sizes (x, y, z) of the two point spaces; "rigid" is then rigid in physical space.  Returns
    TrimmedFit(A [3, 4], used: the pairs A was fitted to, iterations: the refits).  Host only.  ValueError where the
    points are too few, not finite or degenerate for the model (collinear for rigid, coplanar for affine)."""
    from . import hip
    what = "fit_transform"
    _block_model(model, what)
    _unit_fraction(keep, what, "keep")
    for v, name in ((src, "src"), (dst, "dst")):
        a = np.asarray(v, np.float64)
        if a.ndim != 2 or a.shape[1] != 3 or not np.isfinite(a).all():
            raise ValueError("%s: %s must be finite n x 3 points" % (what, name))
    if np.shape(src) != np.shape(dst):
        raise ValueError("%s: dst must have the shape of src" % what)
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 0:
        raise ValueError("%s: max_iter must be a non-negative integer, not %r" % (what, max_iter))
    hip._scale3(spacing_src, what, "spacing_src")
    hip._scale3(spacing_dst, what, "spacing_dst")
    out = hip.fit_trimmed(src, dst, model, keep, int(max_iter), spacing_src, spacing_dst)
    if out is None:
        raise ValueError("%s: src and dst are too few or degenerate for model=%r" % (what, model))
    return TrimmedFit(*out)


def register_blocks(moving, fixed, A=None, model="rigid", levels=3, iterations=5, radius=3, keep_blocks=0.5,
                    keep_inliers=0.5, tol=0.01, mask_fixed=None, mask_moving=None, spacing_fixed=None,
                    spacing_moving=None, init=None):
    """Register `moving` to `fixed` by block matching with a trimmed fit, coarse to fine (contract:
    include/sift3d_amd.h, "Block matching"; Ourselin et al. 2001): per iteration `moving` is warped by the current pull
    map, every 4^3 block of `fixed` finds its best-correlated position within `radius` voxels, the keep_blocks share of
    the blocks with the most variance give point pairs, and a `model` ("translation", "rigid", "affine") is fitted to
    the keep_inliers share of the pairs that agree best.  It needs no keypoints, follows a gain that varies in space,
    and trims what does not match (lesions, missing tissue).  A: the start (fixed voxel -> moving voxel; None: the
    identity); init: as refine_affine's, with A=None only.  levels: the coarsest first, each halving the grid (every
    level's fixed grid must keep 8 voxels per axis); iterations: per level; tol: a level stops when no corner of its
    grid moves by that many voxels.  spacing_fixed, spacing_moving: voxel sizes (x, y, z), so that "rigid" is rigid in
    physical space.  The volumes and masks: as refine_affine's.  Returns BlockRegistration(A, warped: `moving` through
    A on the fixed grid, trail: one BlockIteration per iteration in the order run, stop: "converged", "iterations" or
    "failed" of level 0).  Waits for torch's current stream once per iteration."""
    import torch
    from . import hip
    what = "register_blocks"
    _block_model(model, what)
    if init is not None and A is not None:
        raise ValueError("%s: init makes the start itself; it goes with A=None only" % what)
    _levels_and_evaluations(what, levels, {}, 1)
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or \
            not 1 <= iterations <= hip.BLOCK_MAX_ITERATIONS:
        raise ValueError("%s: iterations must be in [1, %d], not %r" % (what, hip.BLOCK_MAX_ITERATIONS, iterations))
    r = hip._block_radius(radius, what)
    _unit_fraction(keep_blocks, what, "keep_blocks")
    _unit_fraction(keep_inliers, what, "keep_inliers")
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or \
            not (np.isfinite(tol) and tol >= 0):
        raise ValueError("%s: tol must be finite and not negative, not %r" % (what, tol))
    kw = dict(model=model, levels=int(levels), iterations=int(iterations), radius=r, keep_blocks=float(keep_blocks),
              keep_inliers=float(keep_inliers), tol=float(tol))
    for v, name in ((spacing_fixed, "spacing_fixed"), (spacing_moving, "spacing_moving")):
        if hip._scale3(v, what, name) is not None:
            kw[name] = v
    A0 = _affine_start(A, what)
    shape = _volume_shape(fixed)
    for _ in range(int(levels)):
        if len(shape) == 3 and min(shape) < 8:
            raise ValueError("%s: levels=%d leaves a fixed grid below 8 voxels on an axis of %s"
                             % (what, levels, _volume_shape(fixed)))
        shape = tuple((v + 1) // 2 for v in shape)
    WF = _mask_host(mask_fixed, fixed, what, "mask_fixed")
    WM = _mask_host(mask_moving, moving, what, "mask_moving")
    F = _similarity_volume(fixed, what, "fixed")
    M = _similarity_volume(moving, what, "moving", F.device)
    WF = _mask_tensor(WF, F, what, "mask_fixed")
    WM = _mask_tensor(WM, F, what, "mask_moving")
    if init is not None:
        A0 = init_affine(M, F, **_init_keywords(init, what, mask_fixed=WF, mask_moving=WM)).A
    res = hip.block_register(F, M, A0, hip.block_register_params(**kw), mask_fixed=WF, mask_moving=WM)
    A1 = np.array(res.A[:], np.float64).reshape(3, 4)
    warped = torch.empty_like(F)
    hip.warp_affine(M, warped, A1, "linear")
    trail = [BlockIteration(e.level, np.array(e.A_in[:]).reshape(3, 4), np.array(e.A_out[:]).reshape(3, 4), e.n_valid,
                            e.n_selected, e.n_used, e.mean_cc, e.rms, e.move) for e in res.trail[:res.iterations]]
    return BlockRegistration(A1, warped, trail, hip.BLOCK_STOPS[res.stop])


# ---- B-spline free-form deformation ---------------------------------------------------------------
FFDRefinement = collections.namedtuple("FFDRefinement", "lattice spacing A field warped trail stop jacobian")
FFDEvaluation = collections.namedtuple("FFDEvaluation", "E msd R n step accepted level")
FFDRegistration = collections.namedtuple("FFDRegistration", "registration refinement")
MiFFDRefinement = collections.namedtuple("MiFFDRefinement", FFDRefinement._fields + ("mi", "nmi", "bins"))
# what refine_ffd(jacobian > 0) returns: the metric's refinement, then the penalty's trail and weight
FFDPenalty = collections.namedtuple("FFDPenalty", "P rmin nonpositive")
JacFFDRefinement = collections.namedtuple("JacFFDRefinement", FFDRefinement._fields + ("penalty", "jacobian_weight"))
JacMiFFDRefinement = collections.namedtuple("JacMiFFDRefinement",
                                            MiFFDRefinement._fields + ("penalty", "jacobian_weight"))
JacobianPenalty = collections.namedtuple("JacobianPenalty", "value nonpositive min max gradient")
# what refine_ffd(landmarks=...) returns: the class of the same call without landmarks, then the term's trail and weight
FFDLandmarkTerm = collections.namedtuple("FFDLandmarkTerm", "L rmax counted")
LANDMARK_REFINEMENTS = {k: collections.namedtuple("Lm" + k.__name__, k._fields + ("landmarks", "landmark_weight"))
                        for k in (FFDRefinement, MiFFDRefinement, JacFFDRefinement, JacMiFFDRefinement)}
FFD_LANDMARK_WEIGHT = 0.01


def jacobian_penalty(field, ref_det=1.0, gradient=False):
    """The volume (folding) penalty of a displacement field [3, oz, oy, ox] (a torch CUDA float32 tensor, or an array,
    which is uploaded), on the discrete Jacobian that jacobian_determinant reports (contract: include/sift3d_amd.h,
    "Jacobian penalty"): with r = det / ref_det per voxel, the mean of (r - 1)^2 / r, continued below r = 1/4 by its
    second-order Taylor polynomial so that folded voxels have a finite value and a slope that unfolds them.  ref_det:
    the determinant that counts as no volume change (finite, not 0).  Returns JacobianPenalty(value, nonpositive: the
    voxels with r <= 0 or NaN, min, max of r, gradient: d value / d field as a float64 CUDA tensor [3, oz, oy, ox] when
    asked for, else None).  Waits for torch's current stream."""
    import torch
    from . import hip
    ref_det = float(ref_det)
    if not np.isfinite(ref_det) or ref_det == 0.0:
        raise ValueError("jacobian_penalty: ref_det must be finite and not 0")
    if not _torch_tensor(field):
        f = _host_field(field, "jacobian_penalty")
        if not device_available():
            raise RuntimeError("jacobian_penalty: no HIP device is available; this library has no CPU path")
        field = torch.from_numpy(f).to("cuda")
    rec, S = hip.jacobian_penalty(field, ref_det, bool(gradient))
    nonpos, total, rmin, rmax = hip.jacobian_penalty_record(rec)
    n = field[0].numel()
    return JacobianPenalty(total / n, nonpos, rmin, rmax, None if S is None else S / float(n))


def jacobian_reference(A):
    """the determinant of the linear part of a 3 x 4 map in the contract's order ("Jacobian penalty")"""
    A = np.asarray(A, np.float64).reshape(-1)
    return float(A[0] * (A[5] * A[10] - A[6] * A[9]) - A[1] * (A[4] * A[10] - A[6] * A[8]) +
                 A[2] * (A[4] * A[9] - A[5] * A[8]))


def _ffd_lattice_tensor(lattice, what):
    import torch
    if _torch_tensor(lattice):
        return lattice
    a = np.ascontiguousarray(lattice, np.float32)
    if a.ndim != 4 or a.shape[0] != 3:
        raise ValueError("%s: the lattice must be [3, gz, gy, gx]" % what)
    if not device_available():
        raise RuntimeError("%s: no HIP device is available; this library has no CPU path" % what)
    return torch.from_numpy(a).to("cuda")


def ffd_field(lattice, spacing, out_shape, A=None):
    """The displacement field [3, oz, oy, ox] of a cubic B-spline control lattice [3, gz, gy, gx] (channels x, y, z;
    voxels of the fixed grid) at integer spacing (an int, or (dx, dy, dz)) over a grid out_shape = (oz, oy, ox),
    through the 3 x 4 pull map A when given (contract: include/sift3d_amd.h, "B-spline free-form deformation").  A
    torch CUDA float32 tensor on torch's current stream; warp_field, jacobian_determinant, similarity, resample_cubic,
    compose_fields and invert_field take it as any field."""
    import torch
    from . import hip
    d = hip.ffd_spacing(spacing, "ffd_field")
    oz, oy, ox = (int(v) for v in out_shape)
    if tuple(lattice.shape) != hip.ffd_lattice_shape((oz, oy, ox), d):
        raise ValueError("ffd_field: the lattice must be %s for this grid and spacing, not %s"
                         % (hip.ffd_lattice_shape((oz, oy, ox), d), tuple(lattice.shape)))
    L = _ffd_lattice_tensor(lattice, "ffd_field")
    A0 = None
    if A is not None:
        A0 = _affine_or_none(A)
        if A0 is None or not np.isfinite(A0).all():
            raise ValueError("ffd_field: A must be a finite 3 x 4 affine pull map or None")
    field = torch.empty((3, oz, oy, ox), dtype=torch.float32, device=L.device)
    return hip.ffd_field(L, d, field, A0)


def ffd_bending_energy(lattice, spacing):
    """The bending energy R of a control lattice (the mean over the control points with all 26 neighbours of the
    squared second derivatives of the spline) and its gradient dR/dc float64 [3, gz, gy, gx], computed on the device.
    Waits for torch's current stream."""
    from . import hip
    L = _ffd_lattice_tensor(lattice, "ffd_bending_energy")
    return hip.ffd_bending(L, hip.ffd_spacing(spacing, "ffd_bending_energy"))


def ffd_transform_points(lattice, spacing, points, A=None):
    """Map points of the fixed grid through a finished free-form deformation: T(p) = A p + s(p), s the cubic B-spline
    of the control lattice [3, gz, gy, gx] at integer `spacing`, evaluated at the points themselves in double (contract:
    include/sift3d_amd.h, "FFD landmarks").  It is the FFD's tps_apply: with r = refine_ffd(...),
    ffd_transform_points(r.lattice, r.spacing, p, r.A) is where the fixed-grid points p [n, 3] (x, y, z in voxels) land
    in the moving volume, which is what a target registration error at annotated landmarks needs.  A: the 3 x 4 pull
    map the lattice was fitted around (None: the identity).  Returns (T [n, 3] float64, inside [n] bool): a point is
    inside where the lattice's support 0 <= x < (g - 3) * spacing holds it on every axis (the fixed grid is inside);
    the rows of T that are not inside are NaN.  Computed on the device; waits for torch's current stream."""
    from . import hip
    d = hip.ffd_spacing(spacing, "ffd_transform_points")
    P = hip._points(points, "ffd_transform_points", "points")
    A0 = None
    if A is not None:
        A0 = _affine_or_none(A)
        if A0 is None or not np.isfinite(A0).all():
            raise ValueError("ffd_transform_points: A must be a finite 3 x 4 affine pull map or None")
    if not _torch_tensor(lattice) and (np.ndim(lattice) != 4 or np.shape(lattice)[0] != 3):
        raise ValueError("ffd_transform_points: the lattice must be [3, gz, gy, gx]")
    if len(P) == 0:
        return np.zeros((0, 3)), np.zeros(0, bool)
    L = _ffd_lattice_tensor(lattice, "ffd_transform_points")
    T = hip.ffd_points(L, d, P, A0).cpu().numpy()
    return T, ~np.isnan(T).any(axis=1)


def refine_ffd(moving, fixed, A=None, spacing=8, levels=3, bending=0.005, mask_fixed=None, mask_moving=None,
               metric="msd", bins=None, range_fixed=None, range_moving=None, jacobian=0.0, features="intensity",
               sigma=1.6, landmarks=None, landmark_weight=FFD_LANDMARK_WEIGHT, mind=None, **params):
    """Fit a cubic B-spline free-form deformation of the fixed grid that lowers the mean squared difference between
    `fixed` and `moving` seen through it, plus bending * (bending energy), by steepest descent coarse to fine (contract:
    include/sift3d_amd.h, "B-spline free-form deformation").  A: the 3 x 4 affine pull map the deformation is added to
    (None: the identity).  spacing: control spacing in voxels, an int or (dx, dy, dz), the same on every level.  params:
    max_evaluations (per level), step0, step_max, tol (voxels), min_overlap.  The volumes are torch CUDA float32
    tensors [nz, ny, nx], or Images / arrays, which are uploaded.  mask_fixed, mask_moving: regions of interest as
    similarity's; the image force is 0 outside them (the bending term still acts everywhere).  Returns
    FFDRefinement(lattice [3, gz, gy, gx], spacing (dx, dy, dz), A, field [3, oz, oy, ox], warped: `moving` through the
    field, trail: one FFDEvaluation(E, msd, R, n, step, accepted, level) per evaluation in the order run, stop:
    "converged", "evaluations", "flat" or "failed" of level 0, jacobian: JacobianStats of the field).  Waits for
    torch's current stream once per evaluation.
    metric="mi" maximises the Mattes mutual information instead (contract: "Mutual-information free-form deformation
    (Mattes)"; cost -mi + bending * R), for volumes whose intensities are related by an unknown map that need not be
    monotone, where the MSD fit is wrong.  bins (None: 32; 4 .. 64) and range_fixed, range_moving ((lo, hi); None: the
    volume's own min and max, one host synchronisation each, widened and refused with ValueError as similarity's) set
    the histogram as in refine_affine and are level 0's on every level.  It returns MiFFDRefinement: FFDRefinement's fields (each trail entry's `msd` holds -mi), then mi and
    nmi at the final lattice and bins; `warped` is not remapped.  `bending` keeps its default of 0.005 for either
    metric: the value was chosen for the MSD of volumes of unit-order intensity, and no calibration of it against -mi
    (which is of order 1 whatever the intensities) is claimed.  bins or a range with metric="msd", and any other
    metric, raise ValueError.
    jacobian > 0 adds jacobian * (the Jacobian penalty of the field, jacobian_penalty with ref_det = det of A's linear
    part) to the cost of either metric, with or without masks (contract: "Jacobian penalty"): the optimiser then keeps
    away from the folding that `jacobian.folded` counts, without the smoothing that a larger `bending` buys it with.
    The result is then a JacFFDRefinement (JacMiFFDRefinement): the metric's fields, then penalty: one FFDPenalty(P,
    rmin, nonpositive) per trail entry, and jacobian_weight.  No calibration of the weight against the image term is
    claimed.  jacobian == 0 is the call without it.
    features="descriptors" (3-D volumes) drives the deformation by the squared difference of the two volumes' dense
    descriptor images summed over their 12 channels instead of the intensities (contract: "Multi-channel free-form
    deformation"): the descriptors do not change under a gain or an offset of either volume, so this is the MSD fit for
    volumes that differ by one.  Per level both volumes are restricted (restrict_volume) and the descriptors computed
    on the restricted volumes with the same window `sigma` in that level's voxels: refine_field's rule.  No bin is
    reoriented under the deformation (demons does not either).  With features="intensity", fixed [nc, oz, oy, ox] and
    moving [nc, nz, ny, nx] of the same nc are the channels themselves (two contrasts of one subject, say), restricted
    per level.  Masks stay 3-D, on the grids of the stacks; level l's are restrict_volume of level l - 1's float masks.
    jacobian > 0 works as above.  The result is an FFDRefinement (JacFFDRefinement); the trail's `msd` is S_ee / n
    with n counting voxels, and `warped` is `moving` through the field, every channel of a 4-D input.
    features="mind" (3-D volumes) is features="descriptors" with the MIND-SSC self-similarity descriptors (mind_ssc;
    contract: "MIND self-similarity descriptors") in the place of the dense gradient histograms: they do not change
    under a gain of EITHER sign and an offset, so this is the fit for volumes of different modalities, an inverted
    contrast included.  mind: a dict of mind_ssc's keyword arguments (None: its defaults); every level's stack is
    mind_ssc of that level's own restricted volume.  `sigma` is not used.  metric="mi",
    bins or ranges together with channels, any other `features`, a 4-D volume beside a 3-D one or with
    features="descriptors" or "mind", `mind` with other features or with keys that are not mind_ssc's, and stacks of
    unequal nc raise ValueError.
    landmarks=(p_fixed, p_moving) or (p_fixed, p_moving, weights), n x 3 arrays in voxels (x, y, z) and n weights >= 0,
    adds landmark_weight * L to the cost of either metric, with or without masks and the Jacobian penalty (contract:
    "FFD landmarks"): L is the weighted mean squared distance between the mapped fixed points T(p_fixed) and p_moving,
    in level-0 voxels^2 on every level.  It pulls the lattice across displacements beyond the image gradient's capture
    range and anchors the fit where the image term is flat or masked out.  A fixed point outside the lattice's support
    is not counted.  The result is the class the call would otherwise return with two more fields (LmFFDRefinement,
    LmMiFFDRefinement, LmJacFFDRefinement, LmJacMiFFDRefinement): landmarks, one FFDLandmarkTerm(L, rmax, counted) per
    trail entry, and landmark_weight.  The default weight 0.01 was the best of three tried on one synthetic pair; no
    calibration against the image term is claimed.  landmark_weight == 0 records L and leaves the fit unchanged.
    Landmarks together with channels are not supported and raise ValueError, as do bad shapes, n outside [1, 65536],
    non-finite moving points or weights, negative weights, and a non-finite or negative landmark_weight."""
    from . import hip
    lm = None
    if landmarks is not None:
        if not isinstance(landmarks, (tuple, list)) or len(landmarks) not in (2, 3):
            raise ValueError("refine_ffd: landmarks must be (p_fixed, p_moving) or (p_fixed, p_moving, weights)")
        lm = hip.ffd_landmark_arrays(landmarks[0], landmarks[1], landmarks[2] if len(landmarks) == 3 else None,
                                     "refine_ffd")
        landmark_weight = float(landmark_weight)
        if not (np.isfinite(landmark_weight) and landmark_weight >= 0):
            raise ValueError("refine_ffd: landmark_weight must be finite and not negative")
    if features not in ("intensity", "descriptors", "mind"):
        raise ValueError("refine_ffd: features must be 'intensity', 'descriptors' or 'mind', not %r" % (features,))
    mind = _mind_keywords("refine_ffd", features, mind)
    dims = tuple(3 if isinstance(v, Image) else v.dim() if _torch_tensor(v) else np.ndim(v) for v in (fixed, moving))
    if dims not in ((3, 3), (4, 4)) or (features != "intensity" and dims != (3, 3)):
        raise ValueError("refine_ffd: fixed and moving must both be volumes [nz, ny, nx]%s, not %d-D and %d-D"
                         % ("" if features != "intensity" else " or both stacks [nc, nz, ny, nx]", *dims))
    channels = features != "intensity" or dims == (4, 4)
    if channels and lm is not None:
        raise ValueError("refine_ffd: landmarks together with channels (features='descriptors' or 'mind', or 4-D "
                         "volumes) are not supported")
    if channels and metric != "msd":
        raise ValueError("refine_ffd: channels (features='descriptors' or 'mind', or 4-D volumes) are driven by the "
                         "MSD alone, not metric=%r" % (metric,))
    if dims == (4, 4) and tuple(fixed.shape)[0] != tuple(moving.shape)[0]:
        raise ValueError("refine_ffd: fixed and moving must have the same number of channels, not %d and %d"
                         % (tuple(fixed.shape)[0], tuple(moving.shape)[0]))
    jacobian = float(jacobian)
    if not (np.isfinite(jacobian) and jacobian >= 0):
        raise ValueError("refine_ffd: jacobian must be finite and not negative")
    if metric not in ("msd", "mi"):
        raise ValueError("refine_ffd: metric must be 'msd' or 'mi', not %r" % (metric,))
    if metric != "mi" and not (bins is None and range_fixed is None and range_moving is None):
        raise ValueError("refine_ffd: bins, range_fixed and range_moving belong to metric='mi', not %r" % (metric,))
    if metric == "mi":
        bins = _mi_bins("refine_ffd", bins)
        _mi_ranges("refine_ffd", range_fixed, range_moving)
    d = hip.ffd_spacing(spacing, "refine_ffd")
    _levels_and_evaluations("refine_ffd", levels, params, hip.FFD_MAX_EVALUATIONS)
    if not (np.isfinite(bending) and bending >= 0):
        raise ValueError("refine_ffd: bending must be finite and not negative")
    A0 = None
    if A is not None:
        A0 = _affine_or_none(A)
        if A0 is None or not np.isfinite(A0).all():
            raise ValueError("refine_ffd: A must be a finite 3 x 4 affine pull map or None")
        if jacobian > 0 and jacobian_reference(A0) == 0.0:
            raise ValueError("refine_ffd: jacobian > 0 needs an A whose linear part has a determinant that is not 0")
    p = hip.ffd_refine_params(spacing=d, levels=int(levels), bending=float(bending), **params)
    WF = _mask_host(mask_fixed, fixed[0] if dims[0] == 4 else fixed, "refine_ffd", "mask_fixed")
    WM = _mask_host(mask_moving, moving[0] if dims[1] == 4 else moving, "refine_ffd", "mask_moving")
    if dims == (4, 4):
        F = _stack_tensor(fixed, "refine_ffd", "fixed")
        M = _stack_tensor(moving, "refine_ffd", "moving", F.device)
    else:
        F = _similarity_volume(fixed, "refine_ffd", "fixed")
        M = _similarity_volume(moving, "refine_ffd", "moving", F.device)
    WF = _mask_tensor(WF, F, "refine_ffd", "mask_fixed")
    WM = _mask_tensor(WM, F, "refine_ffd", "mask_moving")
    penalty = terms = None
    mi = dict(bins=int(bins), range_f=_own_range(F, range_fixed, int(bins)),
              range_m=_own_range(M, range_moving, int(bins))) \
        if metric == "mi" else {}
    if lm is not None:
        res, lattice, field, sim, penalty, terms = hip.ffd_refine_landmarks(
            F, M, *lm, landmark_weight=landmark_weight, jacobian=jacobian if jacobian > 0 else None, A=A0, params=p,
            mask_fixed=WF, mask_moving=WM, **mi)
    elif channels:
        # every level's volumes (and float masks) by restriction; descriptors of each level's own volumes
        fv, mv, wf, wm = [F], [M], [WF], [WM]
        for _ in range(1, int(levels)):
            fv.append(hip.restrict2(fv[-1]))
            mv.append(hip.restrict2(mv[-1]))
            wf.append(None if wf[-1] is None else hip.restrict2(wf[-1]))
            wm.append(None if wm[-1] is None else hip.restrict2(wm[-1]))
        if features == "descriptors":
            fv = [dense_descriptors(v, sigma) for v in fv]
            mv = [dense_descriptors(v, sigma) for v in mv]
        elif features == "mind":
            fv = [mind_ssc(v, **mind) for v in fv]
            mv = [mind_ssc(v, **mind) for v in mv]
        res, lattice, field, penalty = hip.ffd_refine_channels(fv, mv, A0, p, masks_fixed=wf, masks_moving=wm,
                                                               jacobian=jacobian if jacobian > 0 else None)
    elif jacobian > 0:
        res, lattice, field, sim, penalty = hip.ffd_refine_jacobian(F, M, jacobian, A=A0, params=p, mask_fixed=WF,
                                                                    mask_moving=WM, **mi)
    elif metric == "mi":
        res, lattice, field, sim = hip.ffd_mi_refine(F, M, A=A0, params=p, mask_fixed=WF, mask_moving=WM, **mi)
    else:
        res, lattice, field = hip.ffd_refine(F, M, A0, p, mask_fixed=WF, mask_moving=WM)
    trail = [FFDEvaluation(e.E, e.msd, e.R, int(e.n), e.step, bool(e.accepted), e.level)
             for e in res.trail[:res.evaluations]]
    out = FFDRefinement(lattice, d, A0, field, warp_field(M, field), trail, hip.FFD_STOPS[res.stop],
                        jacobian_determinant(field))
    if metric == "mi":
        out = MiFFDRefinement(*out, mi=float(sim.mi), nmi=float(sim.nmi), bins=int(bins))
    if penalty is not None:
        kind = JacMiFFDRefinement if metric == "mi" else JacFFDRefinement
        out = kind(*out, penalty=[FFDPenalty(*q) for q in penalty], jacobian_weight=jacobian)
    if terms is not None:
        out = LANDMARK_REFINEMENTS[type(out)](*out, landmarks=[FFDLandmarkTerm(*t) for t in terms],
                                              landmark_weight=landmark_weight)
    return out


def register_ffd(moving, fixed, spacing=8, levels=3, bending=0.005, nn_thresh=0.8, err_thresh=3.0, num_iter=500, seed=1,
                 ffd_params=None, refine=True, landmarks=False, landmark_weight=FFD_LANDMARK_WEIGHT,
                 landmark_err_thresh=DEFORMABLE_ERR_THRESH, init=None, rematch=None, **detector_kw):
    """register(refine=True) (keypoints, RANSAC, intensity-driven affine refinement), then refine_ffd from its refined
    pull map (fixed voxel -> moving voxel: the refinement's A, the inverse of the registration's).  ffd_params:
    refine_ffd's further keyword arguments (dict(metric="mi") for a mutual-information FFD stage, which then returns
    a MiFFDRefinement; dict(features="descriptors") for an FFD stage driven by the dense descriptors' 12 channels,
    which needs no common intensity scale; dict(features="mind") for one driven by the MIND-SSC descriptors, which
    survive an inverted contrast too); refine: True, or register's dict of refine_affine's keyword arguments (dict(metric="ncc") or
    dict(metric="mi") for the affine stage).  The two stages' metrics are chosen separately; either defaults to the
    MSD.  The volumes are torch CUDA float32 tensors, or Images / arrays, which are uploaded.  Returns
    FFDRegistration(registration: register's RefinedRegistration, refinement: the FFDRefinement).
    landmarks=True keeps the matched keypoints for the FFD stage (they are detected once): the inliers of ransac_affine
    on the same matches at landmark_err_thresh (DEFORMABLE_ERR_THRESH, wider than err_thresh for
    register_deformable's reason: a match that a deformation moved off the affine model is the one the deformable stage
    wants) with the same num_iter and seed go to refine_ffd as landmarks (fixed xyz, moving xyz) with landmark_weight.
    Where RANSAC finds no such inlier the FFD stage runs without the term.  init: register's.
    rematch: register's; the affine stage and the landmarks then come from the guided matches, and `registration` is
    the GuidedRefinedRegistration."""
    F = _similarity_volume(fixed, "register_ffd", "fixed")
    M = _similarity_volume(moving, "register_ffd", "moving", F.device)
    p_mov, p_fix, first = _matched_points_guided(M, F, nn_thresh, detector_kw, "register_ffd", rematch, err_thresh,
                                                 num_iter, seed)
    reg = _with_first(_register_matched(M, F, p_mov, p_fix, err_thresh, num_iter, seed,
                                        refine if isinstance(refine, dict) else True, init), first)
    kw = dict(ffd_params or {})
    if landmarks:
        try:
            _, inl = ransac_affine(p_mov, p_fix, landmark_err_thresh, num_iter, seed)
        except RuntimeError:
            inl = np.zeros(len(p_mov), bool)
        if inl.any():
            kw.update(landmarks=(p_fix[inl], p_mov[inl]), landmark_weight=landmark_weight)
    ref = refine_ffd(M, F, reg.refinement.A, spacing, levels, bending, **kw)
    return FFDRegistration(reg, ref)


def label_overlap(labels_fixed, labels_moving, transform=None, num_labels=None):
    """Overlap of two label volumes (float-valued integers 0 .. L-1, as warp_field(..., interp="nearest") takes
    them), the moving one seen through `transform` (as similarity's) with nearest sampling:
    LabelOverlap(confusion [L, L] int64 indexed [fixed label, moving label], dice [L], jaccard [L] (NaN for a label
    absent from both), volume_fixed [L], volume_moving [L] in voxels), over the fixed voxels that sample inside the
    moving volume.  num_labels None: the largest label of either volume + 1 (one host synchronisation).  Labels past
    L - 1 count as L - 1.  At most 128 labels."""
    from . import hip
    F = _similarity_volume(labels_fixed, "label_overlap", "labels_fixed")
    M = _similarity_volume(labels_moving, "label_overlap", "labels_moving", F.device)
    T = _similarity_transform(transform, F, "label_overlap")
    L = int(num_labels) if num_labels is not None else int(max(float(F.max()), float(M.max()))) + 1
    L = max(L, 2)
    if L > SIMILARITY_MAX_BINS:
        raise ValueError("label_overlap: at most %d labels, not %d" % (SIMILARITY_MAX_BINS, L))
    hist, _ = hip.similarity(F, M, T, L, (0.0, float(L)), (0.0, float(L)), "nearest")
    return label_overlap_measures(hist.cpu().numpy())


def label_overlap_measures(confusion):
    """LabelOverlap of a confusion matrix [L, L] (sift3d_amd_label_overlap; host)"""
    h = np.ascontiguousarray(confusion).astype(np.uint64)
    if h.ndim != 2 or h.shape[0] != h.shape[1]:
        raise ValueError("label_overlap_measures: the confusion matrix must be [L, L]")
    L = h.shape[0]
    dice, jac = np.empty(L, np.float64), np.empty(L, np.float64)
    vf, vm = np.empty(L, np.uint64), np.empty(L, np.uint64)
    if lib().sift3d_amd_label_overlap(h.reshape(-1), L, dice, jac, vf, vm) != 0:
        raise RuntimeError("sift3d_amd_label_overlap failed")
    return LabelOverlap(h.astype(np.int64), dice, jac, vf.astype(np.int64), vm.astype(np.int64))


# ---- distance transforms and surface distances ------------------------------------------------------------------
SurfaceMeasures = collections.namedtuple("SurfaceMeasures",
                                         "hausdorff hd95 assd mean_fm mean_mf max_fm max_mf n_fixed n_moving")
SurfaceDistances = collections.namedtuple("SurfaceDistances", SurfaceMeasures._fields + ("labels",))
_SURFACE_FIELDS = ("hausdorff", "hd95", "assd", "mean_fm", "mean_mf", "max_fm", "max_mf", "n_f", "n_m")


def distance_transform(mask, spacing=None, squared=False, signed=False, invert=False):
    """The exact Euclidean distance transform of a mask [nz, ny, nx] on the device (contract: include/sift3d_amd.h,
    "Distance transforms and surface distances"): at every voxel the distance to the nearest feature voxel, a voxel
    of the mask (bool and integer masks: non-zero; float masks: >= 0.5), or with invert=True a voxel outside it; +inf
    where there is no feature.  spacing = (sx, sy, sz), the voxel's edge lengths (None: 1); squared=True: the squared
    distance.  signed=True: the signed distance of the mask, positive outside it and negative inside (it takes neither
    squared nor invert).  A torch CUDA tensor gives a tensor (torch's current stream); an array or an Image gives a
    numpy array (blocking)."""
    from . import hip
    what = "distance_transform"
    if signed and (squared or invert):
        raise ValueError("distance_transform: signed=True takes neither squared nor invert")
    hip._spacing(spacing, what)
    w = _mask_host(mask, mask, what, "mask")
    if len(w.shape) != 3:
        raise ValueError("distance_transform: mask must be a volume [nz, ny, nx]")
    host = not _torch_tensor(w)
    if host:
        import torch
        if not device_available():
            raise RuntimeError("distance_transform: no HIP device is available; this library has no CPU path")
        w = torch.from_numpy(w).to("cuda")
    out = hip.distance(w, spacing, "signed" if signed else "sq" if squared else "root", invert)
    return out.cpu().numpy() if host else out


def surface_measures(d_fm, d_mf):
    """The surface-distance measures of two lists of distances sorted ascending (sift3d_amd_surface_measures; host,
    double): SurfaceMeasures(hausdorff, hd95, assd, mean_fm, mean_mf, max_fm, max_mf, n_fixed, n_moving); every
    measure is NaN when either list is empty."""
    a, b = (np.ascontiguousarray(d, np.float32).reshape(-1) for d in (d_fm, d_mf))
    out = _SurfaceResult()
    if lib().sift3d_amd_surface_measures(a, len(a), b, len(b), C.byref(out)) != 0:
        raise RuntimeError("sift3d_amd_surface_measures failed")
    return SurfaceMeasures(*(getattr(out, k) for k in _SURFACE_FIELDS))


def surface_distances(labels_fixed, labels_moving, transform=None, num_labels=None, labels=None, spacing=None):
    """Distances between the surfaces of two label volumes (float-valued integers, as label_overlap takes them), per
    label (contract: "Distance transforms and surface distances"): SurfaceDistances(hausdorff, hd95, assd, mean_fm,
    mean_mf, max_fm, max_mf, n_fixed, n_moving, labels), arrays indexed like `labels`, in the units of `spacing` =
    (sx, sy, sz) (None: voxels).  A label's surface is its voxels with a face neighbour of another label or beyond the
    grid; *_fm are taken at the fixed surface's voxels to the moving surface, *_mf the other way; a label absent from
    either volume gives NaN.  labels: the labels to report, default 1 .. L-1 with L = num_labels or the largest label of
    either volume + 1 (one host synchronisation).  transform (as label_overlap's: a 3 x 4 affine pull map, a TPS or a
    displacement field on the fixed grid): the moving labels are first resampled onto the fixed grid with nearest
    sampling (0 outside); without one the two shapes must agree.  Blocking."""
    from . import hip
    import torch
    what = "surface_distances"
    hip._spacing(spacing, what)
    sf, sm = (tuple(v.shape) if hasattr(v, "shape") else np.shape(v) for v in (labels_fixed, labels_moving))
    if transform is None and sf != sm:
        raise ValueError("surface_distances: transform=None needs label volumes of one shape, not %s and %s" % (sf, sm))
    if labels is not None:
        labels = np.asarray(labels).reshape(-1)
        if not 1 <= len(labels) <= SIMILARITY_MAX_BINS or not np.issubdtype(labels.dtype, np.integer):
            raise ValueError("surface_distances: labels must be between 1 and %d integers" % SIMILARITY_MAX_BINS)
    F = _similarity_volume(labels_fixed, what, "labels_fixed")
    M = _similarity_volume(labels_moving, what, "labels_moving", F.device)
    T = _similarity_transform(transform, F, what)
    if T is not None:
        warped = torch.empty_like(F)
        if _torch_tensor(T):
            hip.warp_field(M, warped, T, "nearest", 0.0)
        else:
            hip.warp_affine(M, warped, T, "nearest", 0.0)
        M = warped
    if labels is None:
        L = int(num_labels) if num_labels is not None else int(max(float(F.max()), float(M.max()))) + 1
        L = max(L, 2)
        if L - 1 > SIMILARITY_MAX_BINS:
            raise ValueError("surface_distances: at most %d labels, not %d" % (SIMILARITY_MAX_BINS, L - 1))
        labels = np.arange(1, L)
    res = hip.surface_distances(F, M, labels, spacing)
    cols = [np.array([getattr(r, k) for r in res], np.int64 if k in ("n_f", "n_m") else np.float64)
            for k in _SURFACE_FIELDS]
    return SurfaceDistances(*cols, np.asarray(labels, np.int64))


# ---- dense descriptors: a 12-bin gradient histogram per voxel ------------------------------------
def _dense_image(volume, units, what):
    if isinstance(volume, Image):
        if len(volume.shape) != 3:
            raise ValueError("%s: the image must have one channel" % what)
        return volume if units is None else Image.from_array(volume.data(), units)
    return Image.from_array(volume, units)


def _torch_tensor(volume):
    try:
        import torch
    except ImportError:
        return False
    return isinstance(volume, torch.Tensor)


MIND_KEYWORDS = ("radius", "dilation", "floor", "ceiling")


def _mind_keywords(what, features, mind):
    """the dict `mind` of refine_ffd / refine_field checked: mind_ssc's keyword arguments, with features 'mind' only"""
    if mind is None:
        return {}
    if features != "mind":
        raise ValueError("%s: mind belongs to features='mind', not %r" % (what, features))
    if not isinstance(mind, dict) or any(k not in MIND_KEYWORDS for k in mind):
        raise ValueError("%s: mind must be a dict with keys among %s, not %r" % (what, ", ".join(MIND_KEYWORDS), mind))
    return dict(mind)


def mind_ssc(volume, radius=1, dilation=2, floor=1e-3, ceiling=1e3):
    """The MIND-SSC self-similarity descriptors of a volume (contract: include/sift3d_amd.h, "MIND self-similarity
    descriptors"; Heinrich et al. 2013): per voxel 12 channels exp(-(D_k - min D) / V), D_k the squared difference of
    two patches of radius `radius` (1 .. 2) around two of the voxel's six neighbours at distance `dilation` (1 .. 4),
    V their mean.  The channels describe the volume's own local structure, so those of two modalities compare with a
    plain squared difference: they are unchanged under a gain of either sign and an offset.  V is clamped to
    [floor, ceiling] x (the mean of V over the volume), Heinrich's clamps; floor=None: no floor, ceiling=None: no
    ceiling.  A constant volume gives all ones.  volume: a torch CUDA float32 tensor [nz, ny, nx]; returns a tensor
    [12, nz, ny, nx] on torch's current stream.  The mean costs a first pass over the volume and one host
    synchronisation; with floor and ceiling both None there is neither."""
    from . import hip
    _volume_tensor(volume, "mind_ssc", "volume")
    for v, name in ((floor, "floor"), (ceiling, "ceiling")):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating))
                              or not (float(v) >= 0 and math.isfinite(v))):
            raise ValueError("mind_ssc: %s must be None or a finite number >= 0, not %r" % (name, v))
    if floor is not None and ceiling is not None and float(ceiling) < float(floor):
        raise ValueError("mind_ssc: ceiling %r is below floor %r" % (ceiling, floor))
    if floor is None and ceiling is None:
        return hip.mind_ssc(volume, None, radius, dilation)
    import torch
    stats = torch.empty(hip.DEMONS_STATS_BYTES // 8, dtype=torch.int64, device=volume.device)
    hip.mind_ssc(volume, False, radius, dilation, stats=stats)
    s, n = hip.demons_stats(stats)
    mean = float(s[0]) / int(n[0])
    return hip.mind_ssc(volume, None, radius, dilation, 0.0 if floor is None else float(floor) * mean,
                        math.inf if ceiling is None else float(ceiling) * mean)


def dense_descriptors(volume, sigma=1.6, units=None, rotate=False):
    """Dense descriptor image (contract: include/sift3d_amd.h, "Dense descriptors"): one unit-length
    12-bin icosahedral gradient histogram per voxel, windowed by a Gaussian of `sigma` world units.
    rotate=True: the rotation-invariant variant, each voxel's window binned in its own eigen-frame (see
    dense_orientations).
    A torch CUDA float32 tensor [nz, ny, nx] gives a tensor [12, nz, ny, nx] (torch's current stream);
    an Image or a float32 array gives a numpy array [12, nz, ny, nx] (blocking).  units = (ux, uy, uz):
    by default the Image's units, else (1, 1, 1)."""
    if _torch_tensor(volume):
        import torch
        from . import hip
        out = torch.empty((12,) + tuple(volume.shape), dtype=torch.float32, device=volume.device)
        run = hip.dense_descriptors_rotate if rotate else hip.dense_descriptors
        return run(volume, out, sigma, (1, 1, 1) if units is None else units)
    im = _dense_image(volume, units, "dense_descriptors")
    out = np.empty((12,) + im.shape, np.float32)
    name = "sift3d_amd_image_dense_descriptors_rotate" if rotate else "sift3d_amd_image_dense_descriptors"
    if getattr(lib(), name)(im.h, float(sigma), out.reshape(-1)) != 0:
        raise RuntimeError("%s failed" % name)
    return out


def dense_orientations(volume, sigma=1.6, units=None):
    """Every voxel's eigen-orientation, as the reference's assign_eig_ori gives a keypoint's (R2 of the
    rotating dense contract): (R [3, 3, nz, ny, nx] float32, keep [nz, ny, nx] uint8); rejected voxels
    get R = I and keep = 0.  A torch CUDA float32 tensor gives tensors on its device (torch's current
    stream); an Image or a float32 array gives numpy arrays (blocking; the volume goes to the device through
    torch, and without a device this raises RuntimeError, as dense_descriptors does).  units as
    dense_descriptors."""
    import torch
    from . import hip
    if _torch_tensor(volume):
        src, u = volume, (1, 1, 1) if units is None else units
    else:
        im = _dense_image(volume, units, "dense_orientations")
        if not device_available():
            raise RuntimeError("dense_orientations: no HIP device is available; this library has no CPU path")
        src, u = torch.from_numpy(np.ascontiguousarray(im.data(), np.float32)).cuda(), im.units
    R = torch.empty((3, 3) + tuple(src.shape), dtype=torch.float32, device=src.device)
    keep = torch.empty(tuple(src.shape), dtype=torch.uint8, device=src.device)
    hip.dense_orient(src, R, keep, sigma, u)
    if src is volume:
        return R, keep
    return R.cpu().numpy(), keep.cpu().numpy()


# ---- dense demons refinement of a displacement field ----------------------------------------------
DemonsRefinement = collections.namedtuple("DemonsRefinement", "field warped msd jacobian")
DenseRegistration = collections.namedtuple("DenseRegistration",
                                           "A tps inliers num_matches field warped msd jacobian")
# what refine_field / register_dense return with levels > 1: msd holds every level's iterations in the order run
# (the coarsest level first) and level_slices[l] is level l's slice of it (level 0 the finest)
MultiresRefinement = collections.namedtuple("MultiresRefinement", "field warped msd jacobian level_slices")
MultiresRegistration = collections.namedtuple("MultiresRegistration",
                                              "A tps inliers num_matches field warped msd jacobian level_slices")
# what refine_field returns for update "logdomain" / "symmetric": velocity is the stationary velocity field, field =
# exp(velocity) and inverse = exp(-velocity) (both with the run's squarings), jacobian / inverse_jacobian their
# jacobian_determinant, scaled_max = max|velocity| 2^-Kv (Vercauteren's criterion wants it <= 0.5)
LogDemonsRefinement = collections.namedtuple(
    "LogDemonsRefinement", "field inverse velocity warped msd jacobian inverse_jacobian scaled_max")
MultiresLogDemonsRefinement = collections.namedtuple(
    "MultiresLogDemonsRefinement", LogDemonsRefinement._fields + ("level_slices",))
# what refine_field returns for force "lncc": lncc[k] is the mean local squared cross-correlation over the counted
# voxels before iteration k's update
LnccRefinement = collections.namedtuple("LnccRefinement", "field warped lncc jacobian")
MultiresLnccRefinement = collections.namedtuple("MultiresLnccRefinement", "field warped lncc jacobian level_slices")
# what register_dense returns for force "lncc": DenseRegistration / MultiresRegistration with lncc in the place of msd
LnccRegistration = collections.namedtuple("LnccRegistration", "A tps inliers num_matches field warped lncc jacobian")
MultiresLnccRegistration = collections.namedtuple("MultiresLnccRegistration",
                                                  LnccRegistration._fields + ("level_slices",))
DEMONS_MAX_LEVELS = 6

# Defaults chosen by a sweep on a case the end-to-end test (tests/test_demons.py) does not use: synth_survey(160,
# seed 5) under a 3-degree rotation plus eight Gaussian bumps of 4 voxels (sigma 22, seed 77), refining
# register_deformable's spline (359 matches, 339 inliers; composed error on every 4th voxel of the inner region:
# median 0.537, p90 1.221 voxel, NCC 0.9905).  50 iterations, descriptors, alpha 0.5 / 1 / 2 x sigma_fluid 0 / 1 x
# sigma_diffusion 1 / 2 on an MI355X: every setting improved on the spline, none folded; sigma_diffusion 2 beat 1
# everywhere (median 0.15-0.17 against 0.23-0.26), sigma_fluid 1 beat 0 by a little, and larger alpha (shorter
# steps) was better up to 2: alpha 2, sigma_fluid 1, sigma_diffusion 2 gave median 0.147, p90 0.297, NCC 0.9988.
# Bracketing it (sigma_fluid 1, sigma_diffusion 2; 25 / 50 / 100 iterations): alpha 2 median 0.154 / 0.150 / 0.150,
# p90 0.386 / 0.318 / 0.311; alpha 4: 0.182 / 0.160 / 0.159, p90 0.789 / 0.601 / 0.502; alpha 8: 0.322 / 0.239 /
# 0.222, p90 1.20 / 1.22 / 1.30.  So alpha 2 is the optimum of the three, and 50 iterations take nearly all of the
# gain of 100.  sigma_diffusion 3 was worse than 2 (alpha 2: median 0.141 but p90 0.491; alpha 4: 0.187 / 1.077).
DEMONS_ITERATIONS = 50
DEMONS_ALPHA = 2.0
DEMONS_SIGMA_FLUID = 1.0
DEMONS_SIGMA_DIFFUSION = 2.0


def _volume_tensor(v, what, name):
    from . import hip
    hip._tensor(v, "%s: %s must be a contiguous float32 CUDA tensor [nz, ny, nx]" % (what, name), dims=(3,))


def _mean_or_nan(sums, counts):
    """sums / counts per record, NaN where the count is 0"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(counts > 0, sums / np.maximum(counts, 1).astype(np.float64), np.nan)


DEMONS_UPDATES = ("additive", "diffeomorphic")
LOGDEMONS_UPDATES = ("logdomain", "symmetric")


def demons_squarings(alpha):
    """The squarings of a diffeomorphic update by default: K = max(0, ceil(log2(1 / alpha))).  The force is capped
    at |delta| <= 1 / (2 alpha) voxel (Cauchy-Schwarz; include/sift3d_amd.h, "Dense demons refinement"); the fluid
    blur does not raise the max norm, as its taps are non-negative and normalised to sum 1 (gauss_filter, up to a
    few ulps of float rounding) and its border rule is a convex combination of samples (the mirrored, linearly
    interpolated extended line); so 2^-K / (2 alpha) <= 0.5 voxel, the criterion of Vercauteren et al. (2009)."""
    a = float(alpha)
    if not (math.isfinite(a) and a > 0):
        raise ValueError("alpha must be positive and finite")
    return max(0, int(math.ceil(math.log2(1.0 / a))))


def refine_field(moving, fixed, field=None, iterations=DEMONS_ITERATIONS, alpha=DEMONS_ALPHA,
                 sigma_fluid=DEMONS_SIGMA_FLUID, sigma_diffusion=DEMONS_SIGMA_DIFFUSION, features="descriptors",
                 sigma=1.6, update="additive", squarings=None, levels=1, level_iterations=None, velocity=None, bch=1,
                 max_motion=16.0, velocity_squarings=None, mask_fixed=None, mask_moving=None, force="demons", radius=2,
                 step=0.5):
    """Dense demons refinement (contract: include/sift3d_amd.h, "Dense demons refinement") of a displacement
    field [3, nz, ny, nx] on fixed's grid (a pull map fixed voxel -> moving voxel; None: start from zero) so that
    the moving features warped through it agree with the fixed ones at every voxel.  moving, fixed: torch CUDA
    float32 tensors [nz, ny, nx] (shapes may differ).  features: "descriptors" (the dense descriptor images of
    both, window sigma, 12 channels), "mind" (the MIND-SSC self-similarity descriptors of both, mind_ssc's 12 channels,
    which survive an inverted contrast: the stacks for volumes of different modalities; with levels > 1 of every
    level's own restricted volume, as "descriptors"; ("mind", dict) hands mind_ssc the dict's keyword arguments) or
    "intensity" (the volumes themselves: classic demons).  update: "additive"
    (u += delta) or "diffeomorphic" (u <- u o exp(delta), "Field composition, exponential and inverse"), with
    `squarings` squarings of the exponential; None picks demons_squarings(alpha), which is 0 at the default alpha 2:
    the update is then u o delta, a composition with the step itself.  The caller's field is not modified.
    Returns DemonsRefinement(field, warped = moving through the field (linear, fill 0), msd [iterations] (the mean
    of s_d over the voxels that sample inside, per iteration, before its update; NaN when there is none),
    jacobian = jacobian_determinant(field)).
    levels > 1: coarse to fine ("Multi-resolution demons").  Both volumes are restricted levels - 1 times
    (restrict_volume); "intensity" uses the restricted volumes, "descriptors" the dense descriptor images of every
    level's volumes with the same sigma in that level's voxels (the window doubles in fine voxels per level; a
    restriction of the 12 channels would not be unit length).  The start field is restricted to the coarsest level
    (a low-pass: pass levels=1 to keep it exactly), refined there for level_iterations[levels - 1] iterations, handed
    up and refined again, down to level_iterations[0] on the full grid; level_iterations None: `iterations` at every
    level.  Returns MultiresRefinement: as above, msd holding every level's iterations in the order run (the
    coarsest first), and level_slices, where msd[level_slices[l]] is level l's part (level 0 the finest).
    update "logdomain" or "symmetric" ("Log-domain demons"): the state is a stationary velocity field (`velocity`
    [3, nz, ny, nx], None: zero; `field` must be None) read through its exponential; "symmetric" adds the force of
    the exchanged pair, so that exchanging moving and fixed negates the velocity (the two shapes must agree).  bch 1:
    the update with the first Lie bracket, 0: the plain sum.  velocity_squarings: the squarings Kv of every
    exponential, None: field_squarings(max_motion), enough for velocities up to max_motion voxels; a warning is
    issued when the result's max|v| 2^-Kv exceeds 0.5.  `squarings` is not used.  Returns LogDemonsRefinement (with
    levels > 1 MultiresLogDemonsRefinement, which adds level_slices): field = exp(v), inverse = exp(-v), velocity,
    warped (moving through field), msd, jacobian and inverse_jacobian (of field and inverse), scaled_max.
    mask_fixed, mask_moving ("Masks in demons"): regions of interest on fixed's and moving's grids, each None (all in)
    or a bool, integer or float array or CUDA tensor of its volume's shape (in where non-zero; floats in where >= 0.5).
    A fixed voxel drives the force only where it samples inside, is in mask_fixed and lands (nearest voxel) in
    mask_moving; elsewhere the force is 0 and the field is what the two blurs carry there, the smooth extension of its
    surroundings.  msd is then the mean over the counted voxels.  Every update accepts masks; "symmetric" exchanges
    them with the volumes in its backward force.  With levels > 1 level l's mask is the restriction (restrict_volume)
    of level l - 1's float mask, never a thresholded copy.  With features "descriptors" the descriptor images are
    still computed from the whole volumes: the masks act on the force only.  With both None the calls are the
    unmasked ones.
    force "lncc" ("Local cross-correlation"): the force is the exact derivative of the local squared cross-correlation
    over (2 radius + 1)^3 windows, for volumes whose intensity relation varies in space (bias fields, contrast uptake),
    which the demons force would follow.  Every iteration moves the field by at most `step` voxels (alpha is not
    used); it needs features "intensity" and update "additive" or "diffeomorphic" (squarings None: 0, the step being
    at most `step` <= 0.5 voxel by default).  Returns LnccRefinement(field, warped, lncc, jacobian), with levels > 1
    MultiresLnccRefinement, which adds level_slices; lncc[k] is the mean cc over the counted voxels before iteration
    k's update (NaN when there is none).  force "demons", the default, is everything above, untouched."""
    import torch
    from . import hip
    mind = None
    if isinstance(features, tuple) and len(features) == 2 and features[0] == "mind":
        features, mind = features
    if force not in ("demons", "lncc"):
        raise ValueError("force must be 'demons' or 'lncc', not %r" % (force,))
    if force == "lncc":
        # (ahead of the tensor checks and of any upload: these depend on the arguments alone)
        if features != "intensity":
            raise ValueError("force 'lncc' needs features 'intensity', not %r" % (features,))
        if update not in DEMONS_UPDATES:
            raise ValueError("force 'lncc' needs update 'additive' or 'diffeomorphic', not %r" % (update,))
        radius = _lncc_radius(radius, "refine_field")
        if isinstance(step, bool) or not isinstance(step, (int, float, np.integer, np.floating)) or \
                not (math.isfinite(step) and step > 0):
            raise ValueError("refine_field: step must be positive and finite, not %r" % (step,))
    log = update in LOGDEMONS_UPDATES
    if log:
        # (ahead of the tensor checks: these depend on the arguments alone)
        if field is not None:
            raise ValueError("update %r keeps a velocity, not a displacement: pass `velocity`, not `field`"
                             % (update,))
        if bch not in (0, 1):
            raise ValueError("bch must be 0 or 1, not %r" % (bch,))
        if update == "symmetric" and tuple(np.shape(moving)) != tuple(np.shape(fixed)):
            raise ValueError("update 'symmetric' needs moving %s and fixed %s of one shape"
                             % (tuple(np.shape(moving)), tuple(np.shape(fixed))))
    # (the masks against their volumes' shapes too: before anything is uploaded)
    wf = _mask_host(mask_fixed, fixed, "refine_field", "mask_fixed")
    wm = _mask_host(mask_moving, moving, "refine_field", "mask_moving")
    _volume_tensor(moving, "refine_field", "moving")
    _volume_tensor(fixed, "refine_field", "fixed")
    if not log and update not in DEMONS_UPDATES:
        raise ValueError("update must be 'additive', 'diffeomorphic', 'logdomain' or 'symmetric', not %r" % (update,))
    levels = int(levels)
    if not 1 <= levels <= DEMONS_MAX_LEVELS:
        raise ValueError("levels must be in 1 .. %d, not %r" % (DEMONS_MAX_LEVELS, levels))
    if level_iterations is not None:
        level_iterations = [int(k) for k in level_iterations]
        if len(level_iterations) != levels or any(k < 0 for k in level_iterations):
            raise ValueError("level_iterations must hold one count >= 0 per level")
    if features not in ("descriptors", "intensity", "mind"):
        raise ValueError("features must be 'descriptors', 'intensity' or 'mind', not %r" % (features,))
    mind = _mind_keywords("refine_field", features, mind)
    its = [int(iterations)] * levels if level_iterations is None else level_iterations
    wf = _mask_tensor(wf, fixed, "refine_field", "mask_fixed")
    wm = _mask_tensor(wm, fixed, "refine_field", "mask_moving")     # (on the fixed volume's device, as every mask)
    fv, mv = [fixed], [moving]
    for _ in range(1, levels):
        fv.append(hip.restrict2(fv[-1]))
        mv.append(hip.restrict2(mv[-1]))
    # the masks per level: the restriction of the float mask of the level above (None stays None)
    WFs, WMs = [wf], [wm]
    for _ in range(1, levels):
        WFs.append(None if WFs[-1] is None else hip.restrict2(WFs[-1]))
        WMs.append(None if WMs[-1] is None else hip.restrict2(WMs[-1]))
    if wf is None:
        WFs = None
    if wm is None:
        WMs = None
    if features == "descriptors":
        Fs = [dense_descriptors(v, sigma) for v in fv]
        Ms = [dense_descriptors(v, sigma) for v in mv]
    elif features == "mind":
        Fs = [mind_ssc(v, **mind) for v in fv]
        Ms = [mind_ssc(v, **mind) for v in mv]
    else:
        Fs, Ms = fv, mv
    if log:
        return _refine_velocity(moving, fixed, Fs, Ms, its, velocity, alpha, sigma_fluid, sigma_diffusion,
                                update == "symmetric", bch, max_motion, velocity_squarings, WFs, WMs)
    if field is None:
        u = torch.zeros((3,) + tuple(fixed.shape), dtype=torch.float32, device=fixed.device)
    else:
        hip._field_tensor(field, "refine_field")
        u = field.clone()
    if force == "lncc":
        K = 0 if update == "additive" or squarings is None else int(squarings)
        stats = hip.demons_lncc(Fs, Ms, u, its, radius, step, sigma_fluid, sigma_diffusion, update=update, squarings=K,
                                masks_fixed=WFs, masks_moving=WMs)
        cc = _mean_or_nan(*hip.demons_stats(stats))
        warped = warp_field(moving, u, "linear", 0.0)
        if levels == 1:
            return LnccRefinement(u, warped, cc, jacobian_determinant(u))
        return MultiresLnccRefinement(u, warped, cc, jacobian_determinant(u), _level_slices(its))
    K = 0
    if update != "additive":
        K = demons_squarings(alpha) if squarings is None else int(squarings)
    if levels == 1:
        stats = hip.demons(Fs[0], Ms[0], u, its[0], alpha, sigma_fluid, sigma_diffusion, update=update, squarings=K,
                           mask_fixed=wf, mask_moving=wm)
    else:
        stats = hip.demons_multires(Fs, Ms, u, its, alpha, sigma_fluid, sigma_diffusion, update=update, squarings=K,
                                    masks_fixed=WFs, masks_moving=WMs)
    msd = _mean_or_nan(*hip.demons_stats(stats))
    warped = warp_field(moving, u, "linear", 0.0)
    if levels == 1:
        return DemonsRefinement(u, warped, msd, jacobian_determinant(u))
    slices, at = [None] * levels, 0
    for l in range(levels - 1, -1, -1):
        slices[l] = slice(at, at + its[l])
        at += its[l]
    return MultiresRefinement(u, warped, msd, jacobian_determinant(u), tuple(slices))


def _level_slices(its):
    """level l's slice of the per-iteration records, which run the coarsest level first (level 0 the finest)"""
    slices, at = [None] * len(its), 0
    for l in range(len(its) - 1, -1, -1):
        slices[l] = slice(at, at + its[l])
        at += its[l]
    return tuple(slices)


def _refine_velocity(moving, fixed, Fs, Ms, its, velocity, alpha, sigma_fluid, sigma_diffusion, symmetric, bch,
                     max_motion, velocity_squarings, WFs=None, WMs=None):
    """refine_field's log-domain updates, after its checks: Fs, Ms the feature stacks per level, WFs, WMs the masks per
    level or None"""
    import torch
    from . import hip
    levels = len(Fs)
    if velocity is None:
        v = torch.zeros((3,) + tuple(fixed.shape), dtype=torch.float32, device=fixed.device)
    else:
        hip._field_tensor(velocity, "refine_field", "velocity")
        v = velocity.clone()
    Kv = field_squarings(max_motion) if velocity_squarings is None else int(velocity_squarings)
    stats = hip.logdemons(Fs, Ms, v, its, alpha, sigma_fluid, sigma_diffusion, symmetric, bch, Kv, masks_fixed=WFs,
                          masks_moving=WMs)
    msd = _mean_or_nan(*hip.demons_stats(stats))
    u = field_exp(v, Kv)
    w = field_exp(v, Kv, negate=True)
    scaled_max = float(torch.sqrt((v.double() ** 2).sum(0)).max()) * 2.0 ** -Kv
    if scaled_max > 0.5:
        warnings.warn("refine_field: max|v| 2^-Kv = %.3g exceeds 0.5 voxel with Kv = %d: the exponentials are "
                      "inaccurate; raise max_motion or velocity_squarings" % (scaled_max, Kv))
    r = (u, w, v, warp_field(moving, u, "linear", 0.0), msd, jacobian_determinant(u), jacobian_determinant(w),
         scaled_max)
    if levels == 1:
        return LogDemonsRefinement(*r)
    slices, at = [None] * levels, 0
    for l in range(levels - 1, -1, -1):
        slices[l] = slice(at, at + its[l])
        at += its[l]
    return MultiresLogDemonsRefinement(*(r + (tuple(slices),)))


def restrict_volume(volume, scale=1.0):
    """The volume (or channel stack) on the grid half as fine ("Multi-resolution demons": coarse voxel i sits at
    fine voxel 2 i, an axis of n has (n + 1) // 2): the separable binomial (1/4, 1/2, 1/4) with replicated edges,
    which keeps constants and linear ramps.  volume: a torch CUDA float32 tensor [nz, ny, nx] or [nc, nz, ny, nx];
    returns a new tensor on torch's current stream.  scale 0.5 restricts a displacement field [3, nz, ny, nx]."""
    from . import hip
    if not _torch_tensor(volume):
        raise ValueError("restrict_volume: the volume must be a CUDA tensor")
    return hip.restrict2(volume, None, scale)


def prolong_field(field, out_shape):
    """The displacement field [3, cz, cy, cx] carried to the grid out_shape = (nz, ny, nx) twice as fine (every c =
    (n + 1) // 2): 2 x its linear interpolation at p / 2, so that the fine field describes the same map in fine
    voxels.  torch CUDA float32; returns a new tensor on torch's current stream."""
    import torch
    from . import hip
    hip._field_tensor(field, "prolong_field")
    nz, ny, nx = (int(s) for s in out_shape)
    if min(nz, ny, nx) < 1 or tuple(field.shape[1:]) != hip.half_shape((nz, ny, nx)):
        raise ValueError("prolong_field: the field %s is not on the grid under %s" % (tuple(field.shape), (nz, ny, nx)))
    fine = torch.empty((3, nz, ny, nx), dtype=torch.float32, device=field.device)
    return hip.field_prolong2(field, fine)


# ---- discrete displacement search ------------------------------------------------------------------------------------
CostVolume = collections.namedtuple("CostVolume", "cost radius blocks")
DiscreteRegistration = collections.namedtuple("DiscreteRegistration", "field warped data level_slices jacobian")
DISCRETE_FEATURES = ("mind", "intensity", "descriptors")


def _discrete_features(what, features, mind):
    """(kind, mind keywords, (fixed stack, moving stack) or None) of the `features` of cost_volume / register_discrete:
    "mind", "intensity", "descriptors", ("mind", dict), or a pair of CUDA stacks [nc, nz, ny, nx]"""
    from . import hip
    if isinstance(features, tuple) and len(features) == 2 and features[0] == "mind":
        if mind is not None:
            raise ValueError("%s: features ('mind', dict) and mind= are two ways to say one thing" % what)
        features, mind = features
    if isinstance(features, (tuple, list)) and len(features) == 2 and all(_torch_tensor(t) for t in features):
        if mind is not None:
            raise ValueError("%s: mind needs features 'mind'" % what)
        for t, name in zip(features, ("fixed", "moving")):
            hip._tensor(t, "%s: the %s stack must be a contiguous float32 CUDA tensor [nc, nz, ny, nx]" % (what, name),
                        dims=(4,))
        if features[0].shape[0] != features[1].shape[0] or not 1 <= features[0].shape[0] <= hip.DISCRETE_MAX_CHANNELS:
            raise ValueError("%s: the stacks must hold the same 1 .. %d channels" % (what, hip.DISCRETE_MAX_CHANNELS))
        return "stacks", {}, tuple(features)
    if not isinstance(features, str) or features not in DISCRETE_FEATURES:
        raise ValueError("%s: features must be 'mind', 'intensity', 'descriptors' or a pair of CUDA stacks "
                         "[nc, nz, ny, nx], not %r" % (what, features))
    return features, _mind_keywords(what, features, mind), None


def _discrete_stacks(kind, mind, fv, mv):
    """the feature stacks of the level volumes fv, mv (lists, level 0 first)"""
    if kind == "mind":
        return [mind_ssc(v, **mind) for v in fv], [mind_ssc(v, **mind) for v in mv]
    if kind == "descriptors":
        return [dense_descriptors(v) for v in fv], [dense_descriptors(v) for v in mv]
    return fv, mv


def _discrete_start(what, transform, F, device):
    """the start field [3, nz, ny, nx] on F's grid of None, a 3 x 4 pull map, a TPS or a field (cloned)"""
    import torch
    from . import hip
    grid = tuple(F.shape[-3:])
    if transform is None:
        return torch.zeros((3,) + grid, dtype=torch.float32, device=device)
    if _torch_tensor(transform):
        hip._field_tensor(transform, what)
        if tuple(transform.shape[1:]) != grid:
            raise ValueError("%s: the field %s is not on the fixed grid %s" % (what, tuple(transform.shape), grid))
        return transform.clone()
    if not isinstance(transform, TPS):
        transform = _affine_start(transform, what, "the transform")
    return displacement_field(transform, grid, device)


def cost_volume(fixed, moving, transform=None, radius=4, features="mind", mask_fixed=None, mask_moving=None):
    """The cost volume of "Discrete displacement search" (include/sift3d_amd.h): for every 4^3 block of `fixed` and
    every displacement d in [-radius, radius]^3 the mean squared difference of the feature channels of the block and
    of `moving`, seen through `transform` and shifted by d.  features: "mind" (mind_ssc of both volumes; ("mind", dict)
    hands it the dict's keyword arguments), "intensity" (the volumes), "descriptors" (dense_descriptors) or a pair
    (fixed stack, moving stack) of CUDA tensors [nc, nz, ny, nx], with which fixed and moving are not read and may be
    None.  transform: None, a 3 x 4 pull map, a TPS or a displacement field on the fixed grid.  mask_fixed,
    mask_moving: as similarity's; a block with a voxel out of mask_fixed and a label whose shifted block has a voxel
    outside the grid or out of the warped mask_moving hold +inf.  Returns CostVolume(cost: a CUDA float32 tensor
    [nbz, nby, nbx, (2 radius + 1)^3], the label index k = ((dz + R)(2R + 1) + (dy + R))(2R + 1) + (dx + R); radius;
    blocks = (nbz, nby, nbx)).  On torch's current stream, no host synchronisation."""
    import torch
    from . import hip
    what = "cost_volume"
    r = hip._discrete_int(radius, 1, hip.DISCRETE_MAX_RADIUS, what, "radius")
    kind, mind, stacks = _discrete_features(what, features, None)
    if stacks is None:
        WF = _mask_host(mask_fixed, fixed, what, "mask_fixed")
        WM = _mask_host(mask_moving, moving, what, "mask_moving")
        F = _similarity_volume(fixed, what, "fixed")
        M = _similarity_volume(moving, what, "moving", F.device)
        Fs, Ms = _discrete_stacks(kind, mind, [F], [M])
        Fs, Ms = Fs[0], Ms[0]
    else:
        Fs, Ms = stacks
        F, M = Fs[0], Ms[0]
        WF = _mask_host(mask_fixed, F, what, "mask_fixed")
        WM = _mask_host(mask_moving, M, what, "mask_moving")
    if min(F.shape) < 4:
        raise ValueError("%s: fixed %s must hold a block of 4 voxels on every axis" % (what, tuple(F.shape)))
    WF = _mask_tensor(WF, F, what, "mask_fixed")
    WM = _mask_tensor(WM, F, what, "mask_moving")
    u = _discrete_start(what, transform, F, F.device)
    W = warp_field(Ms, u, "linear", 0.0)
    VW = warp_field(WM if WM is not None else torch.ones_like(M), u, "nearest", 0.0)
    cost = hip.cost_volume(Fs, W, r, WF, VW)
    return CostVolume(cost, r, tuple(cost.shape[:3]))


def register_discrete(moving, fixed, field=None, features="mind", mind=None, levels=3, radius=4, thetas=None, passes=2,
                      mask_fixed=None, mask_moving=None):
    """Deformable registration by discrete displacement search (contract: include/sift3d_amd.h, "Discrete displacement
    search"; Heinrich et al., TMI 2013 and WBIR 2014): coarse to fine, per level the cost volume of every 4^3 block
    over the displacements [-radius, radius]^3, then per coupling weight of `thetas` (None: the library's schedule)
    one displacement per block of smallest cost + theta |d - b|^2 against the smooth block field b, and `passes`
    binomial passes over the choice; the level's field is composed with the result.  There is no gradient and no
    dependence on the start inside the search range, radius 2^(levels - 1) voxels at the coarsest level: it finds the
    motions a demons or FFD stage cannot reach, and its field is their start (refine_field(moving, fixed, r.field,
    ...)).  moving, fixed: torch CUDA float32 tensors [nz, ny, nx] (shapes may differ).  features: as cost_volume's;
    with levels > 1 every level's stack is made from that level's own restricted volumes (a pair of stacks is
    restricted itself).  field: the start, None, a 3 x 4 pull map, a TPS or a displacement field on fixed's grid (not
    modified).  mask_fixed, mask_moving: as refine_field's.  Every level's fixed grid must hold a block of 4 voxels on
    every axis.  Returns DiscreteRegistration(field, warped = moving through the field (linear, fill 0; None with a
    pair of stacks), data [levels * len(thetas)]: the mean chosen data cost per (level, theta) in the order run, the
    coarsest level first (NaN where every block is empty), level_slices (data[level_slices[l]] is level l's part),
    jacobian = jacobian_determinant(field)).  Waits for torch's current stream once, to read the statistics."""
    from . import hip
    what = "register_discrete"
    kind, mind, stacks = _discrete_features(what, features, mind)
    levels = int(levels)
    if not 1 <= levels <= DEMONS_MAX_LEVELS:
        raise ValueError("%s: levels must be in 1 .. %d, not %r" % (what, DEMONS_MAX_LEVELS, levels))
    p = hip.discrete_register_params(radius, passes, thetas)
    if stacks is None:
        wf = _mask_host(mask_fixed, fixed, what, "mask_fixed")
        wm = _mask_host(mask_moving, moving, what, "mask_moving")
        _volume_tensor(moving, what, "moving")
        _volume_tensor(fixed, what, "fixed")
        F0, M0 = fixed, moving
    else:
        F0, M0 = stacks
        wf = _mask_host(mask_fixed, F0[0], what, "mask_fixed")
        wm = _mask_host(mask_moving, M0[0], what, "mask_moving")
    g = tuple(F0.shape[-3:])
    for _ in range(1, levels):
        g = hip.half_shape(g)
    if min(g) < 4:
        raise ValueError("%s: the coarsest of %d levels, %s, does not hold a block of 4 voxels on every axis"
                         % (what, levels, g))
    wf = _mask_tensor(wf, F0, what, "mask_fixed")
    wm = _mask_tensor(wm, F0, what, "mask_moving")
    fv, mv = [F0], [M0]
    for _ in range(1, levels):
        fv.append(hip.restrict2(fv[-1]))
        mv.append(hip.restrict2(mv[-1]))
    Fs, Ms = _discrete_stacks(kind, mind, fv, mv)
    u = _discrete_start(what, field, F0, F0.device)
    stats = hip.discrete_register(Fs, Ms, u, p, wf, wm)
    data = _mean_or_nan(*hip.demons_stats(stats))
    warped = None if stacks is not None else warp_field(moving, u, "linear", 0.0)
    return DiscreteRegistration(u, warped, data, _level_slices([p.n_theta] * levels), jacobian_determinant(u))


def register_dense(moving, fixed, iterations=DEMONS_ITERATIONS, alpha=DEMONS_ALPHA, sigma_fluid=DEMONS_SIGMA_FLUID,
                   sigma_diffusion=DEMONS_SIGMA_DIFFUSION, features="descriptors", sigma=1.6, update="additive",
                   squarings=None, levels=1, level_iterations=None, mask_fixed=None, mask_moving=None, force="demons",
                   radius=2, step=0.5, mind=None, **deformable_kw):
    """register_deformable, then the displacement field of its spline over fixed's grid, then refine_field (update,
    squarings, levels and level_iterations as there).  Returns DenseRegistration(A, tps, inliers, num_matches (as
    register_deformable), field, warped, msd, jacobian (as refine_field)); with levels > 1 MultiresRegistration,
    which adds refine_field's level_slices.  mask_fixed, mask_moving: handed to the refine_field stage only (as
    there); the keypoint and spline stages see the whole volumes.  force, radius, step: refine_field's; with force
    "lncc" the result is LnccRegistration (levels > 1: MultiresLnccRegistration), which has refine_field's lncc where
    the others have msd.  features="mind" drives the refine_field stage by the MIND-SSC descriptors, mind: a dict of
    mind_ssc's keyword arguments for it (the keypoint and spline stages still match the gradient descriptors, which do
    not survive an inverted contrast)."""
    if mind is not None:                                        # (ahead of the tensor checks: the arguments alone)
        features = (features, _mind_keywords("register_dense", features, mind))
    _volume_tensor(moving, "register_dense", "moving")
    _volume_tensor(fixed, "register_dense", "fixed")
    d = register_deformable(moving, fixed, **deformable_kw)
    u = displacement_field(d.tps, tuple(fixed.shape), fixed.device)
    r = refine_field(moving, fixed, u, iterations, alpha, sigma_fluid, sigma_diffusion, features, sigma, update,
                     squarings, levels, level_iterations, mask_fixed=mask_fixed, mask_moving=mask_moving, force=force,
                     radius=radius, step=step)
    head = (d.A, d.tps, d.inliers, d.num_matches, r.field, r.warped)
    if force == "lncc":
        if int(levels) > 1:
            return MultiresLnccRegistration(*head, r.lncc, r.jacobian, r.level_slices)
        return LnccRegistration(*head, r.lncc, r.jacobian)
    if int(levels) > 1:
        return MultiresRegistration(*head, r.msd, r.jacobian, r.level_slices)
    return DenseRegistration(*head, r.msd, r.jacobian)


# ---- field composition, exponential and inverse ---------------------------------------------------------------
FieldInverse = collections.namedtuple("FieldInverse", "field residual_max residual_mean inside")

# Fixed-point iterations of invert_field by default.  The step w <- -u(q + w) contracts with the factor L, u's
# infinity-norm Lipschitz constant (include/sift3d_amd.h), so the error after N steps is at most L^N times the
# first one: L^N <= 1e-6 at L <= 0.6 takes N >= log(1e-6) / log(0.6) = 27.05, so 28.
INVERT_ITERATIONS = 28


def compose_fields(u, v):
    """w = u o v on v's grid: w(p) = v(p) + u(p + v(p)), read through v, then through u (u is extended by its
    edge values outside its grid).  u [3, uz, uy, ux] and v [3, oz, oy, ox]: torch CUDA float32 pull maps, v's
    values in u-grid voxels.  One kernel on torch's current stream; returns a new tensor shaped like v."""
    import torch
    from . import hip
    hip._field_tensor(u, "compose_fields", "u")
    hip._field_tensor(v, "compose_fields", "v")
    out = torch.empty_like(v)
    hip.field_compose(u, v, out, "compose")
    return out


def field_squarings(max_norm):
    """The smallest K >= 0 with max_norm * 2^-K <= 0.5 voxel"""
    m = float(max_norm)
    if not math.isfinite(m):
        raise ValueError("field_squarings: the field is not finite")
    K = 0
    while m * 2.0 ** -K > 0.5:
        K += 1
    return K


def lie_bracket(a, b):
    """The Lie bracket [a, b] = J_a b - J_b a of two fields [3, oz, oy, ox] on one grid (torch CUDA float32), J the
    Jacobian by numpy.gradient's differences ("Log-domain demons"); exp(a + b + [a, b] / 2) approximates
    compose_fields(exp a, exp b).  One kernel on torch's current stream; returns a new tensor."""
    from . import hip
    return hip.field_bracket(a, b, None, "bracket")


def field_exp(v, squarings=None, negate=False):
    """exp(v) by scaling and squaring: w_0 = v 2^-K, w_{k+1} = w_k o w_k; negate: exp(-v), the inverse map, from
    w_0 = v (-2^-K).  v [3, oz, oy, ox] torch CUDA float32.
    squarings None: the smallest K >= 0 with max|v| 2^-K <= 0.5 voxel (Vercauteren et al., 2009); computing max|v|
    in torch costs one host synchronisation.  Returns a new tensor on torch's current stream."""
    import torch
    from . import hip
    hip._field_tensor(v, "field_exp", "v")
    if squarings is None:
        squarings = field_squarings(float(torch.sqrt((v.double() ** 2).sum(0)).max()))
    out = torch.empty_like(v)
    return hip.field_exp(v, out, squarings, negate=bool(negate))


def invert_field(u, out_shape, iterations=INVERT_ITERATIONS, init=None):
    """The inverse of the pull map p -> p + u(p) by fixed-point iteration w <- -u(q + w(q)): u [3, uz, uy, ux]
    torch CUDA float32 (e.g. fixed -> moving on the fixed grid), w on a grid of out_shape = (oz, oy, ox) (the
    moving grid), mapping back; init: the first iterate (None: zero).  Converges when u's Lipschitz constant is
    below 1.  Returns FieldInverse(field, residual_max, residual_mean, inside): per iterate w_0 .. w_N (N + 1
    values), the max and mean of |w + u(q + w)| over the voxels and the number of voxels whose sample is inside
    u's grid.  Reads the statistics, so it waits for torch's current stream."""
    import torch
    from . import hip
    hip._field_tensor(u, "invert_field", "u")
    oz, oy, ox = (int(s) for s in out_shape)
    if init is None:
        w = torch.zeros((3, oz, oy, ox), dtype=torch.float32, device=u.device)
    else:
        hip._field_tensor(init, "invert_field", "init")
        if tuple(init.shape) != (3, oz, oy, ox):
            raise ValueError("invert_field: init %s is not [3, %d, %d, %d]" % (tuple(init.shape), oz, oy, ox))
        w = init.clone()
    stats = hip.field_invert(u, w, iterations)
    s, mx, cnt, ins = hip.field_stats(stats)
    return FieldInverse(w, mx, _mean_or_nan(s, cnt), ins.astype(np.int64))
