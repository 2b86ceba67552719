"""ctypes bindings of the device-level stage ABI (include/sift3d_amd.h, `sift3d_hip_*`).

Device buffers are torch tensors on the current HIP device (torch is only the allocator /
stream / process-group plumbing); every call takes raw device pointers and runs on torch's
current stream, so results are ordered with other torch work on that stream.
"""
import collections
import ctypes as C
import math

import numpy as np

from . import _native

MAX_TAPS = 65
FACE_FLOATS = 19


class FirArgs(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("nx", C.c_int), ("ny", C.c_int),
                ("nz", C.c_int), ("axis", C.c_int), ("width", C.c_int),
                ("taps", C.POINTER(C.c_float)), ("unit_factor", C.c_float), ("n_glob", C.c_int),
                ("off", C.c_int), ("z_lo", C.c_int), ("z_hi", C.c_int), ("variant", C.c_int)]


class ExtremaLevel(C.Structure):
    _fields_ = [("prev", C.c_void_p), ("cur", C.c_void_p), ("next", C.c_void_p),
                ("d_absmax", C.c_void_p), ("z_lo", C.c_int), ("z_hi", C.c_int), ("tag", C.c_int)]


class ExtremaOct(C.Structure):                             # sift3d_hip_extrema_oct
    _fields_ = [("d_g", C.POINTER(C.c_void_p)), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int),
                ("tag0", C.c_int), ("d_work", C.c_void_p), ("work_bytes", C.c_size_t)]


EXTREMA_MAX_OCT = 12                                       # SIFT3D_HIP_EXTREMA_MAX_OCT


class Level(C.Structure):
    _fields_ = [("data", C.c_void_p), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int),
                ("z_off", C.c_int), ("nz_glob", C.c_int), ("ux", C.c_float), ("uy", C.c_float),
                ("uz", C.c_float), ("octave", C.c_int), ("sd", C.c_double)]


class DemonsLevel(C.Structure):
    _fields_ = [("d_F", C.c_void_p), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int), ("d_M", C.c_void_p),
                ("mx", C.c_int), ("my", C.c_int), ("mz", C.c_int), ("iterations", C.c_int)]


class DemonsLevelMasks(C.Structure):
    _fields_ = [("d_WF", C.c_void_p), ("d_WM", C.c_void_p)]


CAND_DTYPE = np.dtype([("idx", "u4"), ("tag", "i4"), ("val", "f4")])
KP_DTYPE = np.dtype([("R", "f4", (9,)), ("cx", "f4"), ("cy", "f4"), ("cz", "f4"),
                     ("level", "i4"), ("row1", "u4"), ("sd", "f8")], align=True)
LEVEL_DTYPE = np.dtype([("data", "u8"), ("nx", "i4"), ("ny", "i4"), ("nz", "i4"),
                        ("z_off", "i4"), ("nz_glob", "i4"), ("ux", "f4"), ("uy", "f4"),
                        ("uz", "f4"), ("octave", "i4"), ("sd", "f8")], align=True)
assert LEVEL_DTYPE.itemsize == C.sizeof(Level)
assert KP_DTYPE.itemsize == 64 and CAND_DTYPE.itemsize == 12
# the records of the slab driver's keypoint exchange (sift3d_slab.hip): as packed by a rank, as built for the host
SLAB_REC_DTYPE = np.dtype([("o", "i4"), ("s", "i4"), ("x", "i4"), ("y", "i4"), ("z", "i4"), ("R", "f4", (9,))])
SLAB_OUT_DTYPE = np.dtype([("o", "i4"), ("s", "i4"), ("x", "i4"), ("y", "i4"), ("z", "i4"), ("R", "f4", (9,)),
                           ("strength", "f4"), ("pad", "i4")])
SLAB_HEADER_BYTES = 64
ROW_FLOATS = 768
assert SLAB_REC_DTYPE.itemsize == 56 and SLAB_OUT_DTYPE.itemsize == 64


class SlabLayout(C.Structure):                             # sift3d_amd_slab_layout
    _fields_ = [(f, C.c_size_t) for f in ("tot_c", "tot_k", "maxc", "maxk", "roff", "toff", "blk")]


class AffineRefineParams(C.Structure):                     # sift3d_amd_affine_refine_params
    _fields_ = [("free_mask", C.c_uint), ("levels", C.c_int), ("max_evaluations", C.c_int),
                ("lambda0", C.c_double), ("lambda_factor", C.c_double), ("lambda_min", C.c_double),
                ("lambda_max", C.c_double), ("tol", C.c_double), ("min_overlap", C.c_double)]


class AffineEvaluation(C.Structure):                       # sift3d_amd_affine_evaluation
    _fields_ = [("msd", C.c_double), ("n", C.c_uint64), ("lambda_", C.c_double), ("accepted", C.c_int),
                ("level", C.c_int)]


AFFINE_MAX_EVALUATIONS = 128                               # checked against the library when it is bound (lib())
AFFINE_MAX_LEVELS = 6
AFFINE_NORMAL_BYTES = 1264
AFFINE_NCC_BYTES = 1488


class AffineRefineResult(C.Structure):                     # sift3d_amd_affine_refine_result
    _fields_ = [("A", C.c_double * 12), ("evaluations", C.c_int), ("stop", C.c_int),
                ("trail", AffineEvaluation * (AFFINE_MAX_LEVELS * AFFINE_MAX_EVALUATIONS))]


class BlockRegisterParams(C.Structure):                    # sift3d_amd_block_register_params
    _fields_ = [("model", C.c_int), ("levels", C.c_int), ("iterations", C.c_int), ("radius", C.c_int),
                ("keep_blocks", C.c_double), ("keep_inliers", C.c_double), ("tol", C.c_double),
                ("spacing_fixed", C.c_double * 3), ("spacing_moving", C.c_double * 3)]


class BlockIteration(C.Structure):                         # sift3d_amd_block_iteration
    _fields_ = [("level", C.c_int), ("n_valid", C.c_int), ("n_selected", C.c_int), ("n_used", C.c_int),
                ("A_in", C.c_double * 12), ("A_out", C.c_double * 12), ("mean_cc", C.c_double), ("rms", C.c_double),
                ("move", C.c_double)]


BLOCK_MAX_ITERATIONS = 64                                  # checked against the library when it is bound (lib())
BLOCK_MAX_RADIUS = 6


class BlockRegisterResult(C.Structure):                    # sift3d_amd_block_register_result
    _fields_ = [("A", C.c_double * 12), ("iterations", C.c_int), ("stop", C.c_int),
                ("trail", BlockIteration * (AFFINE_MAX_LEVELS * BLOCK_MAX_ITERATIONS))]


DISCRETE_MAX_RADIUS = 6                                    # checked against the library when it is bound (lib())
DISCRETE_MAX_CHANNELS = 16
DISCRETE_MAX_THETAS = 16
DISCRETE_MAX_PASSES = 16
COST_SELECT_WORK_BYTES = 16384


class DiscreteRegisterParams(C.Structure):                 # sift3d_amd_discrete_register_params
    _fields_ = [("radius", C.c_int), ("passes", C.c_int), ("n_theta", C.c_int),
                ("theta", C.c_double * DISCRETE_MAX_THETAS)]


class Frame(C.Structure):                                  # sift3d_amd_frame
    _fields_ = [("centroid", C.c_double * 3), ("axes", C.c_double * 9), ("lambda_", C.c_double * 3)]


class AffineInitParams(C.Structure):                       # sift3d_amd_affine_init_params
    _fields_ = [("mode", C.c_int), ("metric", C.c_int), ("levels", C.c_int), ("weight", C.c_int),
                ("floor_f", C.c_float), ("floor_m", C.c_float), ("bins", C.c_int),
                ("lo_f", C.c_float), ("hi_f", C.c_float), ("lo_m", C.c_float), ("hi_m", C.c_float),
                ("range_deg", C.c_double * 3), ("step_deg", C.c_double),
                ("range_vox", C.c_double * 3), ("step_vox", C.c_double), ("min_overlap", C.c_double)]


MOMENTS_BYTES = 88                                         # checked against the library when it is bound (lib())
SIMILARITY_BATCH_MAX = 1024
INIT_MAX_CANDIDATES = 16384
INIT_KEEP = 16


class AffineInitResult(C.Structure):                       # sift3d_amd_affine_init_result
    _fields_ = [("A", C.c_double * 12), ("index", C.c_int), ("K", C.c_int), ("levels", C.c_int), ("kept", C.c_int),
                ("cost", C.c_double), ("n", C.c_uint64), ("frame_f", Frame), ("frame_m", Frame),
                ("keep_index", C.c_int * INIT_KEEP), ("keep_cost", C.c_double * INIT_KEEP),
                ("keep_n", C.c_uint64 * INIT_KEEP)]


class Similarity(C.Structure):                             # sift3d_amd_similarity
    _fields_ = [("n", C.c_uint64), ("msd", C.c_double), ("ncc", C.c_double), ("mi", C.c_double), ("nmi", C.c_double),
                ("entropy_fixed", C.c_double), ("entropy_moving", C.c_double), ("entropy_joint", C.c_double)]


class FFDRefineParams(C.Structure):                        # sift3d_amd_ffd_refine_params
    _fields_ = [("spacing", C.c_int * 3), ("levels", C.c_int), ("max_evaluations", C.c_int),
                ("bending", C.c_double), ("step0", C.c_double), ("step_max", C.c_double), ("tol", C.c_double),
                ("min_overlap", C.c_double)]


class FFDEvaluation(C.Structure):                          # sift3d_amd_ffd_evaluation
    _fields_ = [("E", C.c_double), ("msd", C.c_double), ("R", C.c_double), ("n", C.c_uint64), ("step", C.c_double),
                ("accepted", C.c_int), ("level", C.c_int)]


FFD_MAX_EVALUATIONS = 128                                  # checked against the library when it is bound (lib())
FFD_MAX_SPACING = 256
FFD_RECORD_HEAD_BYTES = 32


class FFDRefineResult(C.Structure):                        # sift3d_amd_ffd_refine_result
    _fields_ = [("evaluations", C.c_int), ("stop", C.c_int),
                ("trail", FFDEvaluation * (AFFINE_MAX_LEVELS * FFD_MAX_EVALUATIONS))]


class FFDPenalty(C.Structure):                             # sift3d_amd_ffd_penalty
    _fields_ = [("P", C.c_double), ("rmin", C.c_double), ("nonpos", C.c_uint64)]


JACOBIAN_PENALTY_RECORD_BYTES = 32


class FFDLandmarkTerm(C.Structure):                        # sift3d_amd_ffd_landmark_term
    _fields_ = [("L", C.c_double), ("rmax", C.c_double), ("counted", C.c_uint64)]


FFD_MAX_LANDMARKS = 65536                                  # checked against the library when it is bound (lib())
FFD_LANDMARKS_RECORD_BYTES = 32


class FFDLevel(C.Structure):                               # sift3d_amd_ffd_level
    _fields_ = [("d_F", C.c_void_p), ("ox", C.c_int), ("oy", C.c_int), ("oz", C.c_int), ("d_M", C.c_void_p),
                ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int), ("d_WF", C.c_void_p), ("d_WM", C.c_void_p)]


class SurfaceResult(C.Structure):                          # sift3d_amd_surface_result
    _fields_ = [("n_f", C.c_uint64), ("n_m", C.c_uint64)] + [(k, C.c_double) for k in (
        "hausdorff", "hd95", "assd", "mean_fm", "mean_mf", "max_fm", "max_mf")]


_bound = None


def lib():
    global _bound
    if _bound is not None:
        return _bound
    L = _native.load()
    vp = C.c_void_p
    # the argument runs that the registration entries share, stated once
    dp = C.POINTER(C.c_double)                             # A: the 3 x 4 pull map (NULL where the entry allows it)
    pair = [vp, C.c_int, C.c_int, C.c_int] * 2             # the fixed volume and its grid, the moving volume and its
    lattice = [vp] + [C.c_int] * 6                         # the control lattice, its dimensions and the spacing
    parzen = [C.c_float] * 4                               # after bins: lo_f, hi_f, lo_m, hi_m
    masks = [vp, vp]                                       # d_WF, d_WM
    affine_refine = [dp, C.POINTER(AffineRefineParams), C.POINTER(AffineRefineResult)]
    ffd_refine = [dp, C.POINTER(FFDRefineParams), C.POINTER(FFDRefineResult)]
    ffd_outputs = [vp] * 5                                 # field, record, grad, work, stream
    sig = {
        "sift3d_hip_device_count": (C.c_int, []),
        "sift3d_hip_set_device": (C.c_int, [C.c_int]),
        "sift3d_hip_malloc": (vp, [C.c_size_t]),
        "sift3d_hip_free": (None, [vp]),
        "sift3d_hip_host_alloc": (vp, [C.c_size_t]),
        "sift3d_hip_host_free": (None, [vp]),
        "sift3d_hip_memcpy_h2d": (C.c_int, [vp, vp, C.c_size_t, vp]),
        "sift3d_hip_memcpy_d2h": (C.c_int, [vp, vp, C.c_size_t, vp]),
        "sift3d_hip_memcpy_d2d": (C.c_int, [vp, vp, C.c_size_t, vp]),
        "sift3d_hip_memset": (C.c_int, [vp, C.c_int, C.c_size_t, vp]),
        "sift3d_hip_stream_create": (vp, []),
        "sift3d_hip_stream_destroy": (None, [vp]),
        "sift3d_hip_stream_sync": (C.c_int, [vp]),
        "sift3d_hip_event_create": (vp, []),
        "sift3d_hip_event_destroy": (None, [vp]),
        "sift3d_hip_event_record": (C.c_int, [vp, vp]),
        "sift3d_hip_event_elapsed_ms": (C.c_double, [vp, vp]),
        "sift3d_hip_absmax": (C.c_int, [vp, C.c_size_t, vp, vp]),
        "sift3d_hip_scale": (C.c_int, [vp, vp, C.c_size_t, vp, vp]),
        "sift3d_hip_fir": (C.c_int, [C.POINTER(FirArgs), vp]),
        "sift3d_hip_fir_yz_u1": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float),
                                          C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
        "sift3d_hip_fir_xyz": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, vp, vp]),
        "sift3d_hip_fir_xyz_covers": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                               C.c_float]),
        "sift3d_hip_fir_x_scaled": (C.c_int, [C.POINTER(FirArgs), vp, vp]),
        "sift3d_hip_nn2_work_floats": (C.c_size_t, [C.c_int, C.c_int]),
        "sift3d_hip_nn2": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]),
        "sift3d_hip_nn2_gated_work_floats": (C.c_size_t, [C.c_int, C.c_int]),
        "sift3d_hip_nn2_gated": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, C.c_float, vp, vp, vp, vp, vp,
                                           vp, vp, vp]),
        "sift3d_hip_subtract_absmax": (C.c_int, [vp, vp, vp, C.c_size_t, vp, vp]),
        "sift3d_hip_dog_stack": (C.c_int, [C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_size_t, vp, vp]),
        "sift3d_hip_dogmax_stack": (C.c_int, [C.POINTER(vp), C.c_int, C.c_size_t, vp, vp]),
        "sift3d_hip_host_device_ptr": (vp, [vp]),
        "sift3d_hip_downsample2": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp]),
        "sift3d_hip_extrema_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
        "sift3d_hip_extrema": (C.c_int, [C.POINTER(ExtremaLevel), C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_double, vp, C.c_uint32, vp, vp, C.c_size_t, vp]),
        "sift3d_hip_extrema_mode": (C.c_int, [C.POINTER(ExtremaLevel), C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_double, C.c_int, vp, C.c_uint32, vp, vp, C.c_size_t, vp]),
        "sift3d_hip_extrema_gauss6": (C.c_int, [C.POINTER(vp), vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.c_int, C.c_double, vp, C.c_uint32, vp, vp, C.c_size_t, vp]),
        "sift3d_hip_extrema_gauss6_phase": (C.c_int, [C.POINTER(vp), vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                      C.c_int, C.c_double, vp, C.c_uint32, vp, vp, C.c_size_t, vp,
                                                      C.c_int]),
        "sift3d_hip_extrema_gauss6_est_phase": (C.c_int, [C.POINTER(vp), vp, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                                          C.c_double, vp, C.c_uint32, vp, vp, C.c_size_t, vp,
                                                          C.c_int]),
        "sift3d_hip_extrema_gauss6_finish": (C.c_int, [C.POINTER(ExtremaOct), C.c_int, C.c_double, vp, C.c_uint32,
                                                       vp, vp]),
        "sift3d_hip_dogmax_sub": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_int, vp, vp]),
        "sift3d_hip_orient": (C.c_int, [vp, vp, C.c_uint32, C.c_double, vp, vp, vp]),
        "sift3d_hip_orient_tab_bytes": (C.c_size_t, [C.c_int, C.c_uint32]),
        "sift3d_hip_orient_tab": (C.c_int, [vp, C.c_int, vp, C.c_uint32, C.c_double, vp, vp, vp, C.c_uint32, vp]),
        "sift3d_hip_orient_tab_part": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_uint32, C.c_uint32,
                                                 C.c_double, vp, vp, vp, C.c_uint32, C.c_int, vp]),
        "sift3d_hip_orient_window_fits": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double]),
        "sift3d_hip_describe": (C.c_int, [vp, vp, C.c_uint32, vp, vp]),
        "sift3d_hip_slab_count": (C.c_int, [vp, vp, C.c_uint32, C.c_int, C.c_int, C.c_int, vp, vp]),
        "sift3d_hip_slab_pack_scratch_bytes": (C.c_size_t, [C.c_uint32]),
        "sift3d_hip_slab_pack": (C.c_int, [vp, vp, vp, vp, C.c_uint32, C.c_int, vp, vp, vp, vp]),
        "sift3d_amd_slab_table": (C.c_int, [vp, C.c_size_t, C.c_int, C.c_int, vp, C.POINTER(SlabLayout)]),
        "sift3d_hip_slab_build": (C.c_int, [vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, vp, C.c_uint32,
                                            C.c_uint32, vp, vp]),
        "sift3d_hip_rows_scatter": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_uint32, vp]),
        "sift3d_hip_max_rows": (C.c_int, [vp, vp, C.c_int, C.c_int, vp]),
        "sift3d_hip_set_mesh": (C.c_int, [C.POINTER(C.c_float)]),
        "sift3d_hip_synth_lattice": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, vp]),
        "sift3d_hip_warp_affine": (C.c_int, pair + [dp, C.c_int, C.c_float, vp]),
        "sift3d_hip_warp_tps": (C.c_int, pair + [dp, vp, C.c_int, C.c_int, C.c_float, vp]),
        "sift3d_hip_warp_tps_launches": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
        "sift3d_hip_affine_field": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, dp, vp]),
        "sift3d_hip_tps_field": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, dp, vp, C.c_int, vp]),
        "sift3d_hip_tps_field_launches": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
        "sift3d_hip_warp_field": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int,
                                            vp, C.c_int, C.c_float, vp]),
        "sift3d_hip_jacobian_det": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
        "sift3d_hip_bspline_work_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
        "sift3d_hip_bspline_prefilter": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
        "sift3d_hip_bspline_warp_affine": (C.c_int, pair + [dp, C.c_float, vp]),
        "sift3d_hip_bspline_warp_field": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int,
                                                    C.c_int, vp, C.c_float, vp]),
        "sift3d_amd_similarity_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
        "sift3d_hip_similarity_affine": (C.c_int, pair + [dp, C.c_int, C.c_int] + parzen + [vp, vp, vp, vp]),
        "sift3d_hip_similarity_field": (C.c_int, pair + [vp, C.c_int, C.c_int] + parzen + [vp, vp, vp, vp]),
        "sift3d_hip_similarity_affine_masked": (C.c_int, pair + [dp, C.c_int, C.c_int] + parzen + [vp, vp, vp, vp]
                                                + masks),
        "sift3d_hip_similarity_field_masked": (C.c_int, pair + [vp, C.c_int, C.c_int] + parzen + [vp, vp, vp, vp]
                                               + masks),
        "sift3d_amd_moments_work_bytes": (C.c_size_t, [C.c_int] * 3),
        "sift3d_hip_moments": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_float, vp, vp, vp]),
        "sift3d_amd_moments_frame": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, dp, dp, dp]),
        "sift3d_amd_similarity_batch_work_bytes": (C.c_size_t, [C.c_int] * 5),
        "sift3d_hip_similarity_affine_batch": (C.c_int, pair + [dp, C.c_int, C.c_int, C.c_int] + parzen
                                               + [vp, vp, vp, vp]),
        "sift3d_hip_similarity_affine_batch_masked": (C.c_int, pair + [dp, C.c_int, C.c_int, C.c_int] + parzen
                                                      + [vp, vp, vp, vp] + masks),
        "sift3d_amd_affine_init_default_params": (None, [C.POINTER(AffineInitParams)]),
        "sift3d_amd_affine_init_struct_bytes": (C.c_size_t, [C.c_int]),
        "sift3d_amd_affine_init_candidates": (C.c_int, [C.c_int, C.POINTER(Frame), C.POINTER(Frame),
                                                        C.POINTER(AffineInitParams), dp, C.POINTER(C.c_int)]),
        "sift3d_amd_affine_init_rank": (C.c_int, [C.c_int, C.c_int, vp, vp, C.c_int, C.c_double, dp, vp, vp,
                                                  C.POINTER(C.c_int)]),
        "sift3d_amd_affine_init_levels": (C.c_int, [C.c_int] * 7),
        "sift3d_amd_affine_init_work_bytes": (C.c_size_t, [C.c_int] * 6 + [C.POINTER(AffineInitParams)]),
        "sift3d_amd_affine_init_device": (C.c_int, pair + masks + [C.POINTER(AffineInitParams),
                                                                   C.POINTER(AffineInitResult), dp, vp, vp, vp]),
        "sift3d_amd_affine_normal_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
        "sift3d_hip_affine_normal_eqs_masked": (C.c_int, pair + [dp, vp, vp, vp] + masks),
        "sift3d_amd_affine_refine_masked_work_bytes": (C.c_size_t, [C.c_int] * 7),
        "sift3d_amd_affine_refine_masked_device": (C.c_int, pair + affine_refine + [vp, vp] + masks),
        "sift3d_hip_ffd_evaluate_masked": (C.c_int, pair + lattice + [dp, C.c_double] + ffd_outputs + masks),
        "sift3d_amd_ffd_refine_masked_work_bytes": (C.c_size_t, [C.c_int] * 10),
        "sift3d_amd_ffd_refine_masked_device": (C.c_int, pair + ffd_refine + [vp, vp, vp, vp] + masks),
        "sift3d_hip_affine_normal_eqs": (C.c_int, pair + [dp, vp, vp, vp]),
        "sift3d_amd_affine_lm_step": (C.c_int, [vp, C.c_uint, C.c_double, dp]),
        "sift3d_amd_affine_apply_delta": (C.c_int, [dp, dp, C.c_int, C.c_int, C.c_int, dp]),
        "sift3d_amd_affine_refine_struct_bytes": (C.c_size_t, [C.c_int]),
        "sift3d_amd_affine_refine_default_params": (None, [C.POINTER(AffineRefineParams)]),
        "sift3d_amd_affine_refine_work_bytes": (C.c_size_t, [C.c_int] * 7),
        "sift3d_amd_affine_refine_device": (C.c_int, pair + affine_refine + [vp, vp]),
        "sift3d_amd_affine_ncc_normal_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
        "sift3d_hip_affine_ncc_normal_eqs": (C.c_int, pair + [dp, vp, vp, vp] + masks),
        "sift3d_amd_affine_ncc_fit": (C.c_int, [vp, dp]),
        "sift3d_amd_affine_ncc_lm_step": (C.c_int, [vp, C.c_uint, C.c_double, dp]),
        "sift3d_amd_affine_ncc_refine_work_bytes": (C.c_size_t, [C.c_int] * 7),
        "sift3d_amd_affine_ncc_refine_device": (C.c_int, pair + affine_refine + [dp, vp, vp] + masks),
        "sift3d_amd_parzen_window": (C.c_int, [C.c_float, C.c_float, C.c_float, C.c_int, C.POINTER(C.c_int),
                                               C.POINTER(C.c_uint32), dp, C.POINTER(C.c_int)]),
        "sift3d_amd_parzen_hist_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
        "sift3d_hip_parzen_hist_affine": (C.c_int, pair + [dp, C.c_int] + parzen + [vp, vp, vp, vp] + masks),
        "sift3d_amd_parzen_mi": (C.c_int, [vp, C.c_int, C.POINTER(Similarity), vp]),
        "sift3d_hip_affine_mi_normal_eqs": (C.c_int, pair + [dp, C.c_int] + parzen + [vp, vp, vp, vp] + masks),
        "sift3d_amd_affine_mi_refine_work_bytes": (C.c_size_t, [C.c_int] * 7),
        "sift3d_amd_affine_mi_refine_device": (C.c_int, pair + [dp, C.c_int] + parzen + affine_refine[1:]  # A is ahead
                                               + [C.POINTER(Similarity), vp, vp] + masks),
        "sift3d_amd_ffd_lattice_dim": (C.c_int, [C.c_int, C.c_int]),
        "sift3d_amd_ffd_weights": (C.c_int, [C.c_int, vp]),
        "sift3d_amd_ffd_field_work_bytes": (C.c_size_t, [C.c_int] * 3),
        "sift3d_amd_ffd_record_bytes": (C.c_size_t, [C.c_int] * 3),
        "sift3d_amd_ffd_evaluate_work_bytes": (C.c_size_t, [C.c_int] * 6),
        "sift3d_amd_ffd_bending_work_bytes": (C.c_size_t, [C.c_int] * 3),
        "sift3d_amd_ffd_refine_work_bytes": (C.c_size_t, [C.c_int] * 10),
        "sift3d_hip_ffd_field": (C.c_int, lattice + [dp] + [C.c_int] * 3 + [vp, vp, vp]),
        "sift3d_hip_ffd_evaluate": (C.c_int, pair + lattice + [dp, C.c_double] + ffd_outputs),
        "sift3d_hip_ffd_bending": (C.c_int, lattice + [vp, vp, vp]),
        "sift3d_hip_ffd_refine2": (C.c_int, [vp] + [C.c_int] * 6 + [vp, vp]),
        "sift3d_amd_ffd_refine_default_params": (None, [C.POINTER(FFDRefineParams)]),
        "sift3d_amd_ffd_refine_struct_bytes": (C.c_size_t, [C.c_int]),
        "sift3d_amd_ffd_refine_device": (C.c_int, pair + ffd_refine + [vp, vp, vp, vp]),
        "sift3d_hip_parzen_hist_field": (C.c_int, pair + [vp, C.c_int] + parzen + [vp, vp, vp, vp] + masks),
        "sift3d_hip_ffd_mi_evaluate": (C.c_int, pair + lattice + [dp, C.c_double] + ffd_outputs + masks + [C.c_int]
                                       + parzen + [vp]),
        "sift3d_amd_ffd_mi_refine_work_bytes": (C.c_size_t, [C.c_int] * 10),
        "sift3d_amd_ffd_mi_refine_device": (C.c_int, pair + ffd_refine + [vp, vp, vp, vp] + masks + [C.c_int] + parzen
                                            + [C.POINTER(Similarity)]),
        "sift3d_amd_jacobian_penalty_work_bytes": (C.c_size_t, [C.c_int] * 3),
        "sift3d_hip_jacobian_penalty": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_double, vp, vp, vp, vp]),
        "sift3d_amd_ffd_jacobian_gradient_work_bytes": (C.c_size_t, [C.c_int] * 6),
        "sift3d_hip_ffd_jacobian_gradient": (C.c_int, [vp] + [C.c_int] * 6 + [C.c_double, vp, vp, vp, vp]),
        "sift3d_amd_ffd_refine_jacobian_work_bytes": (C.c_size_t, [C.c_int] * 10),
        "sift3d_amd_ffd_refine_jacobian_device": (C.c_int, pair + ffd_refine + [vp, vp, vp, vp] + masks + [C.c_int]
                                                  + parzen + [C.POINTER(Similarity), C.c_double,
                                                              C.POINTER(FFDPenalty)]),
        "sift3d_amd_ffd_level_struct_bytes": (C.c_size_t, [C.c_int]),
        "sift3d_amd_ffd_evaluate_channels_work_bytes": (C.c_size_t, [C.c_int] * 6),
        "sift3d_hip_ffd_evaluate_channels": (C.c_int, pair + [C.c_int] + lattice + [dp, C.c_double] + ffd_outputs
                                             + masks),
        "sift3d_amd_ffd_refine_channels_work_bytes": (C.c_size_t, [C.c_int] * 6),
        "sift3d_amd_ffd_refine_channels_device": (C.c_int, [C.POINTER(FFDLevel), C.c_int, C.c_int] + ffd_refine
                                                  + [vp, vp, vp, vp, C.c_double, C.POINTER(FFDPenalty)]),
        "sift3d_amd_ffd_landmarks_struct_bytes": (C.c_size_t, [C.c_int]),
        "sift3d_hip_ffd_points": (C.c_int, lattice + [dp, vp, C.c_int, vp, vp]),
        "sift3d_amd_ffd_landmarks_work_bytes": (C.c_size_t, [C.c_int] * 4),
        "sift3d_hip_ffd_landmarks": (C.c_int, lattice + [dp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]),
        "sift3d_amd_ffd_evaluate_landmarks_bytes": (C.c_size_t, [C.c_int] * 8),
        "sift3d_hip_ffd_evaluate_landmarks": (C.c_int, pair + lattice + [dp, C.c_double] + ffd_outputs + masks
                                              + [C.c_double, vp, vp, vp, vp, C.c_int, C.c_double, vp]),
        "sift3d_amd_ffd_refine_landmarks_work_bytes": (C.c_size_t, [C.c_int] * 11),
        "sift3d_amd_ffd_refine_landmarks_device": (C.c_int, pair + ffd_refine + [vp, vp, vp, vp] + masks + [C.c_int]
                                                   + parzen + [C.POINTER(Similarity), C.c_double,
                                                               C.POINTER(FFDPenalty), vp, vp, vp, C.c_int, C.c_double,
                                                               C.POINTER(FFDLandmarkTerm)]),
        "sift3d_hip_dense_bin": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                           vp, vp]),
        "sift3d_hip_dense_normalize": (C.c_int, [vp, C.c_size_t, vp]),
        "sift3d_amd_dense_work_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
        "sift3d_amd_dense_descriptors_device": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double),
                                                          C.c_double, vp, vp, vp]),
        "sift3d_hip_dense_orient": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                              C.c_double, vp, vp, vp]),
        "sift3d_hip_dense_rotate_bin": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                                  C.c_double, C.c_double, vp, vp, vp]),
        "sift3d_amd_dense_rotate_work_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
        "sift3d_amd_dense_descriptors_rotate_device": (C.c_int, [vp, C.c_int, C.c_int, C.c_int,
                                                                 C.POINTER(C.c_double), C.c_double, vp, vp, vp]),
        "sift3d_hip_demons_force": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_double, vp, vp, vp, vp]),
        "sift3d_amd_demons_work_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
        "sift3d_amd_demons_device": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                               vp, C.c_int, C.c_double, C.c_double, C.c_double, vp, vp, vp]),
        "sift3d_hip_field_compose": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp,
                                               C.c_int, vp, vp, vp]),
        "sift3d_amd_field_exp_work_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
        "sift3d_amd_field_exp_device": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
        "sift3d_amd_field_invert_work_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
        "sift3d_amd_field_invert_device": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int,
                                                     C.c_int, vp, vp, vp]),
        "sift3d_amd_demons_work_floats_ex": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
        "sift3d_amd_demons_device_ex": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int,
                                                  C.c_int, vp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int,
                                                  C.c_int, vp, vp, vp]),
        "sift3d_hip_restrict2": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_float, vp]),
        "sift3d_hip_field_prolong2": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp]),
        "sift3d_amd_demons_multires_work_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
        "sift3d_amd_demons_multires_device": (C.c_int, [C.POINTER(DemonsLevel), C.c_int, C.c_int, vp, C.c_double,
                                                        C.c_double, C.c_double, C.c_int, C.c_int, vp, vp, vp]),
        "sift3d_hip_field_bracket": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]),
        "sift3d_amd_field_exp_signed_device": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
        "sift3d_amd_logdemons_work_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
        "sift3d_amd_logdemons_device": (C.c_int, [C.POINTER(DemonsLevel), C.c_int, C.c_int, vp, C.c_double,
                                                  C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
        "sift3d_hip_demons_force_masked": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int,
                                                     C.c_int, C.c_double, vp, vp, vp, vp, vp, vp]),
        "sift3d_amd_demons_masked_device": (C.c_int, [C.POINTER(DemonsLevel), C.POINTER(DemonsLevelMasks), C.c_int,
                                                      C.c_int, vp, C.c_double, C.c_double, C.c_double, C.c_int,
                                                      C.c_int, vp, vp, vp]),
        "sift3d_amd_logdemons_masked_device": (C.c_int, [C.POINTER(DemonsLevel), C.POINTER(DemonsLevelMasks), C.c_int,
                                                         C.c_int, vp, C.c_double, C.c_double, C.c_double, C.c_int,
                                                         C.c_int, C.c_int, vp, vp, vp]),
        "sift3d_amd_lncc_work_bytes": (C.c_size_t, [C.c_int] * 3),
        "sift3d_hip_lncc": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int] + masks +
                            [C.c_int, vp, vp, vp, vp, vp]),
        "sift3d_hip_lncc_force": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int] + masks +
                                  [C.c_int, vp, vp, vp, vp]),
        "sift3d_hip_field_normalize": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_double, vp, vp]),
        "sift3d_amd_demons_lncc_work_floats": (C.c_size_t, [C.c_int] * 5),
        "sift3d_amd_demons_lncc_device": (C.c_int, [C.POINTER(DemonsLevel), C.POINTER(DemonsLevelMasks), C.c_int,
                                                    C.c_int, vp, C.c_double, C.c_double, C.c_double, C.c_int,
                                                    C.c_int, vp, vp, vp]),
        "sift3d_amd_mind_work_bytes": (C.c_size_t, [C.c_int] * 3),
        "sift3d_hip_mind_ssc": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                vp, vp, vp, vp, vp, vp]),
        "sift3d_amd_block_match_work_bytes": (C.c_size_t, [C.c_int] * 4),
        "sift3d_hip_block_match": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]),
        "sift3d_amd_fit_trimmed": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_int, C.c_double,
                                             C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                             C.POINTER(C.c_double), vp, C.POINTER(C.c_int)]),
        "sift3d_amd_block_register_default_params": (None, [C.POINTER(BlockRegisterParams)]),
        "sift3d_amd_block_register_struct_bytes": (C.c_size_t, [C.c_int]),
        "sift3d_amd_block_register_work_floats": (C.c_size_t, [C.c_int] * 9),
        "sift3d_amd_block_register_device": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int,
                                                       vp, vp, C.POINTER(C.c_double),
                                                       C.POINTER(BlockRegisterParams), C.POINTER(BlockRegisterResult),
                                                       vp, vp]),
        "sift3d_amd_cost_volume_bytes": (C.c_size_t, [C.c_int] * 4),
        "sift3d_amd_cost_volume_work_bytes": (C.c_size_t, [C.c_int] * 5),
        "sift3d_hip_cost_volume": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp]),
        "sift3d_amd_cost_select_work_bytes": (C.c_size_t, [C.c_int] * 3),
        "sift3d_hip_cost_select": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_double, vp, vp, vp, vp,
                                             vp]),
        "sift3d_amd_block_field_smooth_work_bytes": (C.c_size_t, [C.c_int] * 4),
        "sift3d_hip_block_field_smooth": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
        "sift3d_hip_block_field_expand": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp]),
        "sift3d_amd_discrete_register_default_params": (None, [C.POINTER(DiscreteRegisterParams)]),
        "sift3d_amd_discrete_register_struct_bytes": (C.c_size_t, [C.c_int]),
        "sift3d_amd_discrete_register_work_floats": (C.c_size_t, [C.c_int] * 11),
        "sift3d_amd_discrete_register_device": (C.c_int, [C.POINTER(DemonsLevel), C.c_int, C.c_int, vp, vp, vp,
                                                          C.POINTER(DiscreteRegisterParams), vp, vp, vp]),
        "sift3d_amd_distance_work_bytes": (C.c_size_t, [C.c_int] * 3),
        "sift3d_hip_distance_sq": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, vp, vp, vp]),
        "sift3d_hip_distance": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, vp, vp, vp]),
        "sift3d_hip_distance_signed": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), vp, vp, vp]),
        "sift3d_hip_label_surface": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
        "sift3d_hip_surface_collect": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_size_t, vp, vp]),
        "sift3d_amd_surface_distances_work_bytes": (C.c_size_t, [C.c_int] * 3),
        "sift3d_amd_surface_distances_device": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                                          C.c_int, C.POINTER(C.c_double), C.POINTER(SurfaceResult),
                                                          vp, vp]),
        "sift3d_hip_test_expf": (C.c_int, [vp, vp, C.c_size_t, vp]),
        "sift3d_hip_test_eigen3": (C.c_int, [vp, vp, vp, C.c_size_t, vp]),
        "sift3d_hip_last_error": (C.c_char_p, []),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    # the layouts and limits restated above are the header's
    want = (C.sizeof(AffineRefineParams), C.sizeof(AffineEvaluation), C.sizeof(AffineRefineResult),
            AFFINE_NORMAL_BYTES, AFFINE_MAX_EVALUATIONS, AFFINE_MAX_LEVELS)
    got = tuple(L.sift3d_amd_affine_refine_struct_bytes(k) for k in range(6))
    if got != want:
        raise RuntimeError("sift3d_amd.hip restates the affine refinement layouts as %s, the library has %s"
                           % (want, got))
    # the NCC record's size: the one-level driver's work buffer is the partial slots and the record (a multiple of 16)
    got = (L.sift3d_amd_affine_ncc_refine_work_bytes(1, 1, 1, 1, 1, 1, 1)
           - L.sift3d_amd_affine_ncc_normal_work_bytes(1, 1, 1))
    if got != AFFINE_NCC_BYTES:
        raise RuntimeError("sift3d_amd.hip restates the NCC affine record as %d bytes, the library has %d"
                           % (AFFINE_NCC_BYTES, got))
    want = (C.sizeof(FFDRefineParams), C.sizeof(FFDEvaluation), C.sizeof(FFDRefineResult), FFD_RECORD_HEAD_BYTES,
            FFD_MAX_EVALUATIONS, AFFINE_MAX_LEVELS, FFD_MAX_SPACING)
    got = tuple(L.sift3d_amd_ffd_refine_struct_bytes(k) for k in range(7))
    if got != want:
        raise RuntimeError("sift3d_amd.hip restates the FFD layouts as %s, the library has %s" % (want, got))
    want = (C.sizeof(FFDLevel),) + tuple(getattr(FFDLevel, f).offset for f in ("d_F", "ox", "d_M", "nx", "d_WF", "d_WM"))
    got = tuple(L.sift3d_amd_ffd_level_struct_bytes(k) for k in range(7))
    if got != want:
        raise RuntimeError("sift3d_amd.hip restates the FFD level as %s, the library has %s" % (want, got))
    want = (C.sizeof(FFDLandmarkTerm), FFD_LANDMARKS_RECORD_BYTES, FFD_MAX_LANDMARKS,
            AFFINE_MAX_LEVELS * FFD_MAX_EVALUATIONS)
    got = tuple(L.sift3d_amd_ffd_landmarks_struct_bytes(k) for k in range(4))
    if got != want:
        raise RuntimeError("sift3d_amd.hip restates the FFD landmark layouts as %s, the library has %s" % (want, got))
    want = (C.sizeof(AffineInitParams), C.sizeof(Frame), C.sizeof(AffineInitResult), MOMENTS_BYTES,
            SIMILARITY_BATCH_MAX, INIT_MAX_CANDIDATES, INIT_KEEP)
    got = tuple(L.sift3d_amd_affine_init_struct_bytes(k) for k in range(7))
    if got != want:
        raise RuntimeError("sift3d_amd.hip restates the initial-transform layouts as %s, the library has %s"
                           % (want, got))
    want = (C.sizeof(BlockRegisterParams), C.sizeof(BlockIteration), C.sizeof(BlockRegisterResult),
            BLOCK_MAX_ITERATIONS, BLOCK_MAX_RADIUS)
    got = tuple(L.sift3d_amd_block_register_struct_bytes(k) for k in range(5))
    if got != want:
        raise RuntimeError("sift3d_amd.hip restates the block-matching layouts as %s, the library has %s" % (want, got))
    want = (C.sizeof(DiscreteRegisterParams), DISCRETE_MAX_RADIUS, DISCRETE_MAX_CHANNELS, DISCRETE_MAX_THETAS,
            DISCRETE_MAX_PASSES, COST_SELECT_WORK_BYTES)
    got = tuple(L.sift3d_amd_discrete_register_struct_bytes(k) for k in range(6))
    if got != want:
        raise RuntimeError("sift3d_amd.hip restates the discrete-search layouts as %s, the library has %s" % (want, got))
    _bound = L
    return L


def _check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed: %s" % (what, lib().sift3d_hip_last_error().decode()))


_stream = None


def current_stream(refresh=False):
    """torch's current HIP stream as a void*.  Looked up once and cached (the query costs
    ~0.1 ms of host time, far more than a kernel launch); call current_stream(refresh=True)
    after switching torch's current stream."""
    global _stream
    if _stream is None or refresh:
        import torch
        _stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return _stream


def fir(src, dst, axis, taps, unit_factor=1.0, n_glob=None, off=0, z_lo=0, z_hi=None, variant=0):
    """One 1-D pass (convolve_sep_gen, imutil.c:742-861) on torch CUDA tensors [nz, ny, nx]."""
    nz, ny, nx = src.shape
    assert src.is_contiguous() and dst.is_contiguous() and src.shape == dst.shape
    taps = np.ascontiguousarray(taps, np.float32)
    a = FirArgs(src.data_ptr(), dst.data_ptr(), nx, ny, nz, axis, len(taps),
                taps.ctypes.data_as(C.POINTER(C.c_float)), float(np.float32(unit_factor)),
                nz if n_glob is None else n_glob, off, z_lo, nz if z_hi is None else z_hi, variant)
    _check(lib().sift3d_hip_fir(C.byref(a), current_stream()), "sift3d_hip_fir")
    return dst


def fir_yz(src, dst, taps, n_glob=None, off=0, z_lo=0, z_hi=None):
    """Fused y+z passes with tap spacing 1.  Returns False when the configuration is not covered
    (the caller then issues the two passes separately)."""
    nz, ny, nx = src.shape
    assert src.is_contiguous() and dst.is_contiguous() and src.shape == dst.shape
    taps = np.ascontiguousarray(taps, np.float32)
    rc = lib().sift3d_hip_fir_yz_u1(src.data_ptr(), dst.data_ptr(), nx, ny, nz,
                                    taps.ctypes.data_as(C.POINTER(C.c_float)), len(taps),
                                    nz if n_glob is None else n_glob, off, z_lo,
                                    nz if z_hi is None else z_hi, current_stream())
    if rc == 1:
        return False
    _check(rc, "sift3d_hip_fir_yz_u1")
    return True


def fir_xyz(src, dst, taps, scale_max=None, unit_factors=(1.0, 1.0, 1.0)):
    """A whole blur (x, y and z passes, tap spacing 1) in one launch; scale_max (a 1-element CUDA tensor): of
    src / scale_max.  Returns False, having done nothing, when the configuration is not covered."""
    nz, ny, nx = src.shape
    assert src.is_contiguous() and dst.is_contiguous() and src.shape == dst.shape
    taps = np.ascontiguousarray(taps, np.float32)
    if tuple(unit_factors) != (1.0, 1.0, 1.0) and not lib().sift3d_hip_fir_xyz_covers(
            src.data_ptr(), dst.data_ptr(), nx, ny, nz, len(taps), *[float(np.float32(u)) for u in unit_factors]):
        return False
    rc = lib().sift3d_hip_fir_xyz(src.data_ptr(), dst.data_ptr(), nx, ny, nz,
                                  taps.ctypes.data_as(C.POINTER(C.c_float)), len(taps),
                                  None if scale_max is None else scale_max.data_ptr(), current_stream())
    if rc == 1:
        return False
    _check(rc, "sift3d_hip_fir_xyz")
    return True


def fir_x_scaled(src, dst, taps, scale_max):
    """The x pass (tap spacing 1) of src / scale_max (a 1-element CUDA tensor): im_scale folded in."""
    nz, ny, nx = src.shape
    assert src.is_contiguous() and dst.is_contiguous() and src.shape == dst.shape
    taps = np.ascontiguousarray(taps, np.float32)
    a = FirArgs(src.data_ptr(), dst.data_ptr(), nx, ny, nz, 0, len(taps),
                taps.ctypes.data_as(C.POINTER(C.c_float)), 1.0, nz, 0, 0, nz, 0)
    rc = lib().sift3d_hip_fir_x_scaled(C.byref(a), scale_max.data_ptr(), current_stream())
    if rc == 1:
        return False
    _check(rc, "sift3d_hip_fir_x_scaled")
    return True


def nn2(a, b):
    """Nearest / second-nearest row of b for every row of a (CUDA float32 tensors [n, dim]):
    returns (index int32, squared distance, second squared distance) as tensors."""
    import torch
    assert a.is_contiguous() and b.is_contiguous() and a.shape[1] == b.shape[1]
    na, nb = a.shape[0], b.shape[0]
    j = torch.empty(max(na, 1), dtype=torch.int32, device=a.device)
    d1 = torch.empty(max(na, 1), dtype=torch.float32, device=a.device)
    d2 = torch.empty_like(d1)
    work = torch.empty(lib().sift3d_hip_nn2_work_floats(na, nb), dtype=torch.float32, device=a.device)
    _check(lib().sift3d_hip_nn2(a.data_ptr(), na, b.data_ptr(), nb, a.shape[1], j.data_ptr(),
                                d1.data_ptr(), d2.data_ptr(), work.data_ptr(), current_stream()),
           "sift3d_hip_nn2")
    return j[:na], d1[:na], d2[:na]


def nn2_gated_work_floats(na, nb):
    return int(lib().sift3d_hip_nn2_gated_work_floats(int(na), int(nb)))


def nn2_gated(a, b, pos_a, pos_b, radius, perm_a=None, perm_b=None, work=None):
    """nn2 over the candidates inside the spatial gate only (sift3d_hip_nn2_gated).  pos_a / pos_b: CUDA float32
    tensors [n, 4] (x, y, z, ignored), a's already mapped into b's frame; radius: the gate's, +inf allowed; perm_a /
    perm_b: int32 row orders (None: the identity); work: a float32 tensor of at least nn2_gated_work_floats(na, nb)
    elements, or None.  Returns (index int32, squared distance, second squared distance, block pairs visited, block
    pairs in all)."""
    import torch
    assert a.is_contiguous() and b.is_contiguous() and a.shape[1] == b.shape[1]
    na, nb = a.shape[0], b.shape[0]
    for p, n, name in ((pos_a, na, "pos_a"), (pos_b, nb, "pos_b")):
        if p.dtype != torch.float32 or tuple(p.shape) != (n, 4) or not p.is_contiguous() or p.device != a.device:
            raise ValueError("nn2_gated: %s must be a contiguous float32 tensor [%d, 4] on %s" % (name, n, a.device))
    for p, n, name in ((perm_a, na, "perm_a"), (perm_b, nb, "perm_b")):
        if p is not None and (p.dtype != torch.int32 or tuple(p.shape) != (n,) or not p.is_contiguous()
                              or p.device != a.device):
            raise ValueError("nn2_gated: %s must be a contiguous int32 tensor [%d] on %s" % (name, n, a.device))
    need = nn2_gated_work_floats(na, nb)
    if work is None:
        work = torch.empty(need, dtype=torch.float32, device=a.device)
    elif work.dtype != torch.float32 or work.numel() < need or not work.is_contiguous() or work.device != a.device:
        raise ValueError("nn2_gated: work must be a contiguous float32 tensor of at least %d elements" % need)
    r2 = np.float32(float(radius) * float(radius))
    j = torch.empty(max(na, 1), dtype=torch.int32, device=a.device)
    d1 = torch.empty(max(na, 1), dtype=torch.float32, device=a.device)
    d2 = torch.empty_like(d1)
    vis = torch.zeros(2, dtype=torch.int64, device=a.device)
    _check(lib().sift3d_hip_nn2_gated(a.data_ptr(), na, b.data_ptr(), nb, a.shape[1], pos_a.data_ptr(),
                                      pos_b.data_ptr(), float(r2), perm_a.data_ptr() if perm_a is not None else None,
                                      perm_b.data_ptr() if perm_b is not None else None, j.data_ptr(), d1.data_ptr(),
                                      d2.data_ptr(), vis.data_ptr(), work.data_ptr(), current_stream()),
           "sift3d_hip_nn2_gated")
    v = vis.tolist()
    return j[:na], d1[:na], d2[:na], int(v[0]), int(v[1])


INTERP ={"nearest": 0, "linear": 1}


def _interp(interp):
    if interp not in INTERP:
        raise ValueError("interp must be 'nearest' or 'linear', not %r" % (interp,))
    return INTERP[interp]


def _tensor(t, msg, dims=None, lead=None, shape=None, device=None, dtype="float32"):
    """The one tensor check: t must be a contiguous CUDA tensor of `dtype` (None: any) and, where given, of a rank
    in `dims`, with `lead` channels first, of exactly `shape`, on `device`; ValueError(msg) otherwise."""
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and (dtype is None or t.dtype == getattr(torch, dtype))
            and t.is_contiguous() and (dims is None or t.dim() in dims)
            and (lead is None or (t.dim() >= 1 and t.shape[0] == lead))
            and (shape is None or tuple(t.shape) == tuple(shape)) and (device is None or t.device == device)):
        raise ValueError(msg)


def _field_tensor(t, what, name="field"):
    _tensor(t, "%s: %s must be a contiguous float32 CUDA tensor [3, oz, oy, ox]" % (what, name), dims=(4,), lead=3)


def _same_device(what, *ts):
    if any(t.device != ts[0].device for t in ts):
        raise ValueError("%s: the tensors are not on one device" % what)


def _work(work, need, like, what, dtype=None):
    """The work buffer of a driver: `need` floats allocated on the device of `like` when work is None, else the
    caller's, which must be a contiguous CUDA tensor (of `dtype`, where given) of that many bytes on that device."""
    import torch
    if work is None:
        return torch.empty(need, dtype=torch.float32, device=like.device)
    _tensor(work, "%s: work must be a contiguous %sCUDA tensor of >= %d bytes on the device of the other tensors"
            % (what, dtype + " " if dtype else "", 4 * need), device=like.device, dtype=dtype)
    if work.numel() * work.element_size() < 4 * need:
        raise ValueError("%s: work holds fewer than %d bytes" % (what, 4 * need))
    return work


def _byte_work(what, work, need, like, refuses=None):
    """_work for a driver that states its size in bytes.  refuses: what to say where the library answers 0 bytes,
    which is how the refinement drivers refuse their levels or spacing."""
    if need == 0 and refuses:
        raise ValueError("%s: %s" % (what, refuses))
    return _work(work, (need + 3) // 4, like, what)


def _buffer(what, name, t, shape, like, says=None):
    """An int64 output that the caller may bring: allocated (not cleared) on the device of `like` when t is None, else
    the caller's, which must be contiguous, of exactly `shape` (`says` where the message names it otherwise) there."""
    import torch
    if t is None:
        return torch.empty(shape, dtype=torch.int64, device=like.device)
    _tensor(t, "%s: %s must be a contiguous int64 CUDA tensor %s on F's device" % (what, name, says or list(shape)),
            shape=shape, device=like.device, dtype="int64")
    return t


def _run(name, *args):
    """the library's entry `name` on args; RuntimeError with the library's message where it fails"""
    _check(getattr(lib(), name)(*args), name)


def _warp_pair(src, dst, what):
    for t in (src, dst):
        _tensor(t, "%s: src and dst must be contiguous 3-D float32 CUDA tensors" % what, dims=(3,))
    if src.device != dst.device:
        raise ValueError("%s: src and dst are on different devices" % what)


def warp_affine(src, dst, A, interp="linear", fill=0.0):
    """dst[z, y, x] = src sampled at A [x; y; z; 1] (A: 3 x 4 pull map in voxels; sift3d_hip_warp_affine)
    on torch CUDA float32 contiguous tensors [nz, ny, nx] / [oz, oy, ox], on torch's current stream;
    voxels that sample outside src get `fill`."""
    _warp_pair(src, dst, "warp_affine")
    mode = _interp(interp)
    a = np.ascontiguousarray(A, np.float64).reshape(12)
    nz, ny, nx = src.shape
    oz, oy, ox = dst.shape
    _check(lib().sift3d_hip_warp_affine(src.data_ptr(), nx, ny, nz, dst.data_ptr(), ox, oy, oz,
                                        a.ctypes.data_as(C.POINTER(C.c_double)), mode,
                                        float(fill), current_stream()), "sift3d_hip_warp_affine")
    return dst


def warp_tps(src, dst, tps, interp="linear", fill=0.0):
    """dst[z, y, x] = src sampled at the thin-plate spline q(x, y, z) (sift3d_hip_warp_tps; contract in
    include/sift3d_amd.h): torch CUDA float32 contiguous tensors [nz, ny, nx] / [oz, oy, ox], on torch's
    current stream.  tps is an api.TPS (ctrl, weights, A), packed into the device layout by
    sift3d_amd_tps_pack and uploaded; voxels that sample outside src get `fill`."""
    import torch
    from . import api
    _warp_pair(src, dst, "warp_tps")
    mode = _interp(interp)
    a = np.ascontiguousarray(tps.A, np.float64).reshape(12)
    packed = api.tps_pack(tps.ctrl, tps.weights)
    d_tps = torch.from_numpy(packed).to(src.device)
    nz, ny, nx = src.shape
    oz, oy, ox = dst.shape
    _check(lib().sift3d_hip_warp_tps(src.data_ptr(), nx, ny, nz, dst.data_ptr(), ox, oy, oz,
                                     a.ctypes.data_as(C.POINTER(C.c_double)), d_tps.data_ptr(), len(packed),
                                     mode, float(fill), current_stream()), "sift3d_hip_warp_tps")
    return dst


def warp_tps_launches(out_shape, m):
    """How many launches sift3d_hip_warp_tps splits an output grid (oz, oy, ox) with m points into."""
    oz, oy, ox = out_shape
    return int(lib().sift3d_hip_warp_tps_launches(ox, oy, oz, m))


def affine_field(field, A):
    """field [3, oz, oy, ox] = the displacement field of the pull map A (3 x 4, voxels; sift3d_hip_affine_field),
    torch CUDA float32, on torch's current stream."""
    _field_tensor(field, "affine_field")
    a = np.ascontiguousarray(A, np.float64).reshape(12)
    _, oz, oy, ox = field.shape
    _check(lib().sift3d_hip_affine_field(field.data_ptr(), ox, oy, oz, a.ctypes.data_as(C.POINTER(C.c_double)),
                                         current_stream()), "sift3d_hip_affine_field")
    return field


def tps_field(field, tps):
    """field [3, oz, oy, ox] = the displacement field of the thin-plate spline tps (an api.TPS;
    sift3d_hip_tps_field), torch CUDA float32, on torch's current stream."""
    import torch
    from . import api
    _field_tensor(field, "tps_field")
    a = np.ascontiguousarray(tps.A, np.float64).reshape(12)
    packed = api.tps_pack(tps.ctrl, tps.weights)
    d_tps = torch.from_numpy(packed).to(field.device)
    _, oz, oy, ox = field.shape
    _check(lib().sift3d_hip_tps_field(field.data_ptr(), ox, oy, oz, a.ctypes.data_as(C.POINTER(C.c_double)),
                                      d_tps.data_ptr(), len(packed), current_stream()), "sift3d_hip_tps_field")
    return field


def tps_field_launches(out_shape, m):
    """How many launches sift3d_hip_tps_field splits an output grid (oz, oy, ox) with m points into."""
    oz, oy, ox = out_shape
    return int(lib().sift3d_hip_tps_field_launches(ox, oy, oz, m))


def warp_field(src, dst, field, interp="linear", fill=0.0):
    """dst = src sampled at p + field(p) (sift3d_hip_warp_field), torch CUDA float32 contiguous tensors:
    src [nz, ny, nx] / dst [oz, oy, ox], or src [nc, nz, ny, nx] / dst [nc, oz, oy, ox] (every channel at
    the same points); field [3, oz, oy, ox].  On torch's current stream; voxels that sample outside get `fill`."""
    for t in (src, dst):
        _tensor(t, "warp_field: src and dst must be contiguous 3-D or 4-D float32 CUDA tensors", dims=(3, 4))
    _field_tensor(field, "warp_field")
    if src.dim() != dst.dim() or (src.dim() == 4 and src.shape[0] != dst.shape[0]):
        raise ValueError("warp_field: src %s and dst %s differ in channels" % (tuple(src.shape), tuple(dst.shape)))
    if tuple(dst.shape[-3:]) != tuple(field.shape[1:]):
        raise ValueError("warp_field: dst %s does not match the field's grid %s"
                         % (tuple(dst.shape), tuple(field.shape[1:])))
    if not (src.device == dst.device == field.device):
        raise ValueError("warp_field: src, dst and field are not on one device")
    mode = _interp(interp)
    nc = src.shape[0] if src.dim() == 4 else 1
    nz, ny, nx = src.shape[-3:]
    oz, oy, ox = dst.shape[-3:]
    _check(lib().sift3d_hip_warp_field(src.data_ptr(), nx, ny, nz, nc, field.data_ptr(), ox, oy, oz, dst.data_ptr(),
                                       mode, float(fill), current_stream()), "sift3d_hip_warp_field")
    return dst


JACOBIAN_STATS_BYTES = 16


def jacobian_det(field, det=None):
    """Jacobian determinant of p -> p + field(p) (sift3d_hip_jacobian_det) on torch's current stream: field
    [3, oz, oy, ox] and det [oz, oy, ox] (or None: stats only) torch CUDA float32.  Returns (det, folded, min,
    max); reading the three stats waits for the stream."""
    import torch
    _field_tensor(field, "jacobian_det")
    _, oz, oy, ox = field.shape
    if det is not None:
        _tensor(det, "jacobian_det: det must be a contiguous float32 CUDA tensor [oz, oy, ox] on the field's "
                "device, or None", shape=(oz, oy, ox), device=field.device)
    stats = torch.empty(JACOBIAN_STATS_BYTES // 8, dtype=torch.int64, device=field.device)
    _check(lib().sift3d_hip_jacobian_det(field.data_ptr(), ox, oy, oz, None if det is None else det.data_ptr(),
                                         stats.data_ptr(), current_stream()), "sift3d_hip_jacobian_det")
    raw = stats.view(torch.uint8)[:JACOBIAN_STATS_BYTES].cpu().numpy()
    folded = int(raw[:8].view(np.uint64)[0])
    mn, mx = (float(v) for v in raw[8:16].view(np.float32))
    return det, folded, mn, mx


# ---- cubic B-spline resampling (contract: include/sift3d_amd.h, "Cubic B-spline resampling") -----------------
def bspline_prefilter(src, dst=None, work=None):
    """The cubic B-spline coefficients of src (sift3d_hip_bspline_prefilter): torch CUDA float32 contiguous
    [nz, ny, nx] or [nc, nz, ny, nx], into dst (allocated when None; not src: the prefilter is not in place), on
    torch's current stream.  work: nz*ny*nx floats of scratch, allocated when None."""
    import torch
    _tensor(src, "bspline_prefilter: src must be a contiguous 3-D or 4-D float32 CUDA tensor", dims=(3, 4))
    if dst is None:
        dst = torch.empty_like(src)
    _tensor(dst, "bspline_prefilter: dst must be a contiguous float32 CUDA tensor shaped like src on its device",
            shape=src.shape, device=src.device)
    nc = src.shape[0] if src.dim() == 4 else 1
    nz, ny, nx = src.shape[-3:]
    work = _work(work, lib().sift3d_hip_bspline_work_floats(nx, ny, nz), src, "bspline_prefilter")
    _check(lib().sift3d_hip_bspline_prefilter(src.data_ptr(), nx, ny, nz, nc, dst.data_ptr(), work.data_ptr(),
                                              current_stream()), "sift3d_hip_bspline_prefilter")
    return dst


def bspline_warp_affine(coef, dst, A, fill=0.0):
    """dst[z, y, x] = the cubic B-spline with coefficients coef (bspline_prefilter) at A [x; y; z; 1] (A: 3 x 4 pull
    map in voxels; sift3d_hip_bspline_warp_affine): torch CUDA float32 contiguous [nz, ny, nx] / [oz, oy, ox], on
    torch's current stream; voxels that sample outside get `fill`."""
    _warp_pair(coef, dst, "bspline_warp_affine")
    a = np.ascontiguousarray(A, np.float64).reshape(12)
    nz, ny, nx = coef.shape
    oz, oy, ox = dst.shape
    _check(lib().sift3d_hip_bspline_warp_affine(coef.data_ptr(), nx, ny, nz, dst.data_ptr(), ox, oy, oz,
                                                a.ctypes.data_as(C.POINTER(C.c_double)), float(fill),
                                                current_stream()), "sift3d_hip_bspline_warp_affine")
    return dst


def bspline_warp_field(coef, dst, field, fill=0.0):
    """dst = the cubic B-spline with coefficients coef at p + field(p) (sift3d_hip_bspline_warp_field): coef
    [nz, ny, nx] / dst [oz, oy, ox], or coef [nc, nz, ny, nx] / dst [nc, oz, oy, ox] (every channel at the same
    points); field [3, oz, oy, ox]; torch CUDA float32 contiguous, on torch's current stream."""
    for t in (coef, dst):
        _tensor(t, "bspline_warp_field: coef and dst must be contiguous 3-D or 4-D float32 CUDA tensors", dims=(3, 4))
    _field_tensor(field, "bspline_warp_field")
    if coef.dim() != dst.dim() or (coef.dim() == 4 and coef.shape[0] != dst.shape[0]):
        raise ValueError("bspline_warp_field: coef %s and dst %s differ in channels"
                         % (tuple(coef.shape), tuple(dst.shape)))
    if tuple(dst.shape[-3:]) != tuple(field.shape[1:]):
        raise ValueError("bspline_warp_field: dst %s does not match the field's grid %s"
                         % (tuple(dst.shape), tuple(field.shape[1:])))
    _same_device("bspline_warp_field", coef, dst, field)
    nc = coef.shape[0] if coef.dim() == 4 else 1
    nz, ny, nx = coef.shape[-3:]
    oz, oy, ox = dst.shape[-3:]
    _check(lib().sift3d_hip_bspline_warp_field(coef.data_ptr(), nx, ny, nz, nc, field.data_ptr(), ox, oy, oz,
                                               dst.data_ptr(), float(fill), current_stream()),
           "sift3d_hip_bspline_warp_field")
    return dst


# ---- similarity measures (contract: include/sift3d_amd.h, "Similarity measures") ------------------------------
SIMILARITY_MAX_BINS = 128
SIMILARITY_GRID = 2048
SIMILARITY_STATS_BYTES = 56


def similarity_stats(stats):
    """The record of similarity() on the host, waiting for the stream: (count, float64 [6] = the sums of f, m, f f,
    m m, f m and (f - m)^2)."""
    import torch
    raw = stats.view(torch.uint8)[:SIMILARITY_STATS_BYTES].cpu().numpy()
    return int(raw[:8].view(np.uint64)[0]), raw[8:].view(np.float64).copy()


def _masks(what, F, M, mask_fixed, mask_moving):
    """The two masks of a masked entry (include/sift3d_amd.h, "Masks") as device pointers: each None (NULL: all in) or a
    contiguous float32 CUDA tensor of its volume's shape on F's device.  Returns None when both are None (the unmasked
    entry is called), else (pointer or None, pointer or None)."""
    if mask_fixed is None and mask_moving is None:
        return None
    out = []
    for w, v, name in ((mask_fixed, F, "mask_fixed"), (mask_moving, M, "mask_moving")):
        if w is not None:
            _tensor(w, "%s: %s must be a contiguous float32 CUDA tensor of its volume's shape %s on the fixed volume's "
                    "device" % (what, name, tuple(v.shape)), shape=tuple(v.shape), device=F.device)
        out.append(None if w is None else w.data_ptr())
    return tuple(out)


def _pair(what, F, M, mask_fixed=None, mask_moving=None, *more):
    """The prelude of a wrapper over a fixed volume F [oz, oy, ox] and a moving volume M [nz, ny, nx]: both contiguous
    3-D float32 CUDA tensors, on one device with the tensors of `more` (checked by the caller as tensors), the masks as
    _masks takes them.  Returns (head, masks): head = (F, ox, oy, oz, M, nx, ny, nz) as every entry's arguments begin,
    so head[1:4] is the fixed grid and head[5:8] the moving one; masks as _masks returns them."""
    for t in (F, M):
        _tensor(t, what + ": F and M must be contiguous 3-D float32 CUDA tensors", dims=(3,))
    _same_device(what, F, M, *more)
    oz, oy, ox = F.shape
    nz, ny, nx = M.shape
    return (F.data_ptr(), ox, oy, oz, M.data_ptr(), nx, ny, nz), _masks(what, F, M, mask_fixed, mask_moving)


def _masked_entry(name, masks):
    """(entry, mask arguments) of the measures that come as two entries (the MSD's and similarity's): `name` without
    masks, name + "_masked" with the two pointers only when a mask is given.  The general entries take the two
    pointers always, NULL for none: `masks or (None, None)`."""
    return (name, ()) if masks is None else (name + "_masked", masks)


def similarity(F, M, transform, bins, range_f, range_m, interp="linear", hist=None, work=None, mask_fixed=None,
               mask_moving=None):
    """The joint histogram and moments of the fixed volume F [oz, oy, ox] and the moving volume M [nz, ny, nx] seen
    through a pull map (sift3d_hip_similarity_affine / _field), torch CUDA float32 contiguous, on torch's current
    stream.  transform: a 3 x 4 affine pull map, a field tensor [3, oz, oy, ox], or None: the identity, which needs
    equal shapes.  range_f, range_m: (lo, hi) of the bins.  Returns (hist int64 [bins, bins] indexed [b_f, b_m],
    stats): stats is the device record, read with similarity_stats (which waits for the stream), as reading hist
    does.  hist, work: the caller's buffers (int64 [bins, bins]; sift3d_amd_similarity_work_bytes bytes).  mask_fixed,
    mask_moving: float32 masks of F's and M's shapes (in where >= 0.5; header, "Masks"); with either given the call goes
    to the _masked entry, with both None to the unmasked one."""
    import torch
    head, masks = _pair("similarity", F, M, mask_fixed, mask_moving)
    mode = _interp(interp)
    bins = int(bins)
    if not 2 <= bins <= SIMILARITY_MAX_BINS:
        raise ValueError("similarity: bins must be in [2, %d]" % SIMILARITY_MAX_BINS)
    oz, oy, ox = F.shape
    field = None
    if transform is None:
        if F.shape != M.shape:
            raise ValueError("similarity: transform=None needs volumes of one shape, not %s and %s"
                             % (tuple(F.shape), tuple(M.shape)))
        transform = np.eye(3, 4)
    if isinstance(transform, torch.Tensor):
        field = transform
        _tensor(field, "similarity: a field must be a contiguous float32 CUDA tensor [3, oz, oy, ox] on F's grid",
                shape=(3, oz, oy, ox))
        _same_device("similarity", F, field)
    else:
        a = np.ascontiguousarray(transform, np.float64)
        if a.shape not in ((3, 4), (12,)):
            raise ValueError("similarity: transform must be a 3 x 4 affine pull map, a field tensor or None")
        a = a.reshape(12)
    hist = _buffer("similarity", "hist", hist, (bins, bins), F, "[bins, bins]")
    work = _byte_work("similarity", work, lib().sift3d_amd_similarity_work_bytes(ox, oy, oz, bins), F)
    stats = torch.empty(SIMILARITY_STATS_BYTES // 8, dtype=torch.int64, device=F.device)
    (lo_f, hi_f), (lo_m, hi_m) = ((float(np.float32(v)) for v in r) for r in (range_f, range_m))
    name, masks = _masked_entry("sift3d_hip_similarity_" + ("affine" if field is None else "field"), masks)
    _run(name, *head, _dptr(a) if field is None else field.data_ptr(), mode, bins, lo_f, hi_f, lo_m, hi_m,
         hist.data_ptr(), stats.data_ptr(), work.data_ptr(), current_stream(), *masks)
    return hist, stats


# ---- distance transforms and surface distances (contract: include/sift3d_amd.h, "Distance transforms and surface
# distances") ------------------------------------------------------------------------------------------------------
DISTANCE_MAX_DIM = 4096


def _spacing(spacing, what):
    """(sx, sy, sz) as a float64 [3] and its pointer, or (None, None): all 1.  ValueError on anything the entries would
    refuse."""
    if spacing is None:
        return None, None
    s = np.ascontiguousarray(spacing, np.float64)
    if s.shape != (3,) or not np.all(np.isfinite(s)) or np.any(s < 1e-6) or np.any(s > 1e6):
        raise ValueError("%s: spacing must be three finite values (sx, sy, sz) in [1e-6, 1e6]" % what)
    return s, s.ctypes.data_as(C.POINTER(C.c_double))


def _distance_volume(t, what, name):
    _tensor(t, "%s: %s must be a contiguous 3-D float32 CUDA tensor" % (what, name), dims=(3,))
    if max(t.shape) > DISTANCE_MAX_DIM or min(t.shape) < 1:
        raise ValueError("%s: every dimension of %s must be in [1, %d]" % (what, name, DISTANCE_MAX_DIM))


def distance_work_bytes(shape):
    nz, ny, nx = shape
    return lib().sift3d_amd_distance_work_bytes(nx, ny, nz)


def distance(mask, spacing=None, mode="sq", invert=False, out=None, work=None):
    """The Euclidean distance transform of a mask [nz, ny, nx] (torch CUDA float32 contiguous; in where >= 0.5) on
    torch's current stream.  mode "sq": the squared distance D2 to the nearest feature voxel (sift3d_hip_distance_sq),
    "root": D = sqrtf(D2) (sift3d_hip_distance), "signed": the signed distance of the set of in voxels
    (sift3d_hip_distance_signed; invert must be False).  spacing: (sx, sy, sz) or None: all 1.  invert: the features
    are the voxels that are out.  out, work: the caller's buffers (mask's shape; distance_work_bytes bytes)."""
    import torch
    what = "distance"
    _distance_volume(mask, what, "mask")
    if mode not in ("sq", "root", "signed"):
        raise ValueError("distance: mode must be 'sq', 'root' or 'signed', not %r" % (mode,))
    if mode == "signed" and invert:
        raise ValueError("distance: the signed distance takes no invert")
    keep, sp = _spacing(spacing, what)
    if out is None:
        out = torch.empty_like(mask)
    _tensor(out, "distance: out must be a contiguous float32 CUDA tensor of the mask's shape on its device",
            shape=tuple(mask.shape), device=mask.device)
    nz, ny, nx = mask.shape
    work = _work(work, (lib().sift3d_amd_distance_work_bytes(nx, ny, nz) + 3) // 4, mask, what)
    if mode == "signed":
        _check(lib().sift3d_hip_distance_signed(mask.data_ptr(), nx, ny, nz, sp, out.data_ptr(), work.data_ptr(),
                                                current_stream()), "sift3d_hip_distance_signed")
    else:
        name = "sift3d_hip_distance_sq" if mode == "sq" else "sift3d_hip_distance"
        _check(getattr(lib(), name)(mask.data_ptr(), nx, ny, nz, sp, int(bool(invert)), out.data_ptr(),
                                    work.data_ptr(), current_stream()), name)
    return out


def label_surface(labels, label, surface=None, count=None):
    """The six-neighbour surface of one label of a label volume [nz, ny, nx] (sift3d_hip_label_surface), torch CUDA
    float32, on torch's current stream: (surface float32 0 / 1 of labels' shape, count int64 [1] on the device)."""
    import torch
    _distance_volume(labels, "label_surface", "labels")
    if surface is None:
        surface = torch.empty_like(labels)
    _tensor(surface, "label_surface: surface must be a contiguous float32 CUDA tensor of labels' shape on its device",
            shape=tuple(labels.shape), device=labels.device)
    if count is None:
        count = torch.empty(1, dtype=torch.int64, device=labels.device)
    _tensor(count, "label_surface: count must be an int64 CUDA tensor [1] on labels' device", shape=(1,),
            device=labels.device, dtype="int64")
    nz, ny, nx = labels.shape
    _check(lib().sift3d_hip_label_surface(labels.data_ptr(), nx, ny, nz, int(label), surface.data_ptr(),
                                          count.data_ptr(), current_stream()), "sift3d_hip_label_surface")
    return surface, count


def surface_collect(surface, d2, out, count=None):
    """Appends sqrtf(d2) at the voxels where `surface` is in (>= 0.5) to the list `out` (float32 CUDA [capacity]) in no
    particular order (sift3d_hip_surface_collect), on torch's current stream; returns (out, count int64 [1] on the
    device): the number of surface voxels, also where it exceeds the capacity, past which nothing is written."""
    import torch
    _distance_volume(surface, "surface_collect", "surface")
    _tensor(d2, "surface_collect: d2 must be a contiguous float32 CUDA tensor of surface's shape on its device",
            shape=tuple(surface.shape), device=surface.device)
    _tensor(out, "surface_collect: out must be a contiguous 1-D float32 CUDA tensor on surface's device", dims=(1,),
            device=surface.device)
    if count is None:
        count = torch.empty(1, dtype=torch.int64, device=surface.device)
    _tensor(count, "surface_collect: count must be an int64 CUDA tensor [1] on surface's device", shape=(1,),
            device=surface.device, dtype="int64")
    _check(lib().sift3d_hip_surface_collect(surface.data_ptr(), d2.data_ptr(), surface.numel(), out.data_ptr(),
                                            out.numel(), count.data_ptr(), current_stream()),
           "sift3d_hip_surface_collect")
    return out, count


def surface_distances(LF, LM, labels, spacing=None, work=None):
    """The surface-distance measures of the label volumes LF and LM (torch CUDA float32 contiguous, one shape) for every
    label of `labels` (sift3d_amd_surface_distances_device): a list of SurfaceResult records.  Synchronous: it waits
    for torch's current stream twice per label."""
    what = "surface_distances"
    _distance_volume(LF, what, "labels_fixed")
    _tensor(LM, "surface_distances: both label volumes must be contiguous float32 CUDA tensors of one shape on one "
            "device", shape=tuple(LF.shape), device=LF.device)
    lab = np.ascontiguousarray(labels, np.int32).reshape(-1)
    if not 1 <= len(lab) <= SIMILARITY_MAX_BINS:
        raise ValueError("surface_distances: between 1 and %d labels, not %d" % (SIMILARITY_MAX_BINS, len(lab)))
    keep, sp = _spacing(spacing, what)
    nz, ny, nx = LF.shape
    work = _work(work, (lib().sift3d_amd_surface_distances_work_bytes(nx, ny, nz) + 3) // 4, LF, what)
    if work.data_ptr() % 8:
        raise ValueError("surface_distances: work must be 8-byte aligned")
    res = (SurfaceResult * len(lab))()
    _check(lib().sift3d_amd_surface_distances_device(LF.data_ptr(), LM.data_ptr(), nx, ny, nz,
                                                     lab.ctypes.data_as(C.POINTER(C.c_int)), len(lab), sp, res,
                                                     work.data_ptr(), current_stream()),
           "sift3d_amd_surface_distances_device")
    return list(res)


# ---- intensity-driven affine refinement (contract: include/sift3d_amd.h, "Intensity-driven affine refinement") ----
AFFINE_FREE_ALL, AFFINE_FREE_TRANSLATION = 0xFFF, 0x888
AFFINE_STOPS = ("converged", "lambda", "evaluations", "lm_failed")
AFFINE_RECORD_DTYPE = np.dtype([("n", "u8"), ("see", "f8"), ("b", "f8", (12,)), ("H", "f8", (12, 12))])
assert AFFINE_RECORD_DTYPE.itemsize == AFFINE_NORMAL_BYTES


def affine_normal_work_bytes(fixed_shape=(1, 1, 1)):
    """sift3d_amd_affine_normal_work_bytes for a fixed grid (oz, oy, ox)"""
    oz, oy, ox = (int(v) for v in fixed_shape)
    return lib().sift3d_amd_affine_normal_work_bytes(ox, oy, oz)


def _affine12(A, what):
    a = np.ascontiguousarray(A, np.float64)
    if a.shape not in ((3, 4), (12,)):
        raise ValueError("%s: A must be a 3 x 4 affine pull map" % what)
    return a.reshape(12).copy()


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def affine_normal_record(record):
    """The record of affine_normal_equations() on the host, waiting for the stream: (n, S_ee, b float64 [12],
    H float64 [12, 12])."""
    import torch
    raw = record.view(torch.uint8)[:AFFINE_NORMAL_BYTES].cpu().numpy().view(AFFINE_RECORD_DTYPE)[0]
    return int(raw["n"]), float(raw["see"]), raw["b"].copy(), raw["H"].copy()


def affine_normal_equations(F, M, A, record=None, work=None, raw=False, mask_fixed=None, mask_moving=None):
    """The Gauss-Newton normal equations of the mean squared difference of the fixed volume F [oz, oy, ox] and the
    moving volume M [nz, ny, nx] seen through the 3 x 4 pull map A, over A's 12 parameters centred on F's grid
    (sift3d_hip_affine_normal_eqs), torch CUDA float32 contiguous, on torch's current stream.  Returns
    (n, S_ee, b [12], H [12, 12]) on the host (which waits for the stream), or with raw=True the device record (read
    it with affine_normal_record).  record, work: the caller's buffers (int64 [158]; sift3d_amd_affine_normal_work_bytes
    bytes).  mask_fixed, mask_moving: as similarity's (sift3d_hip_affine_normal_eqs_masked)."""
    what = "affine_normal_equations"
    head, masks = _pair(what, F, M, mask_fixed, mask_moving)
    a = _affine12(A, what)
    record = _buffer(what, "record", record, (AFFINE_NORMAL_BYTES // 8,), F)
    work = _byte_work(what, work, lib().sift3d_amd_affine_normal_work_bytes(*head[1:4]), F)
    name, masks = _masked_entry("sift3d_hip_affine_normal_eqs", masks)
    _run(name, *head, _dptr(a), record.data_ptr(), work.data_ptr(), current_stream(), *masks)
    return record if raw else affine_normal_record(record)


def affine_lm_step(n, see, b, H, free_mask=AFFINE_FREE_ALL, lam=0.0):
    """delta float64 [12] of sift3d_amd_affine_lm_step (host): (H + lam diag H) delta = -b on the parameters that
    free_mask frees, 0 elsewhere; None where the entry refuses (n == 0, an empty mask, not positive definite)."""
    rec = np.zeros(1, AFFINE_RECORD_DTYPE)
    rec["n"], rec["see"], rec["b"], rec["H"] = n, see, b, H
    delta = np.zeros(12)
    rc = lib().sift3d_amd_affine_lm_step(rec.ctypes.data, int(free_mask) & 0xFFFFFFFF, float(lam), _dptr(delta))
    return delta if rc == 0 else None


def affine_apply_delta(A, delta, fixed_shape):
    """A' [3, 4] of sift3d_amd_affine_apply_delta (host): A moved by delta, the parameters centred on the grid
    fixed_shape = (oz, oy, ox)."""
    a = _affine12(A, "affine_apply_delta")
    d = np.ascontiguousarray(delta, np.float64).reshape(12)
    out = np.zeros(12)
    oz, oy, ox = (int(v) for v in fixed_shape)
    if lib().sift3d_amd_affine_apply_delta(_dptr(a), _dptr(d), ox, oy, oz, _dptr(out)) != 0:
        raise ValueError("affine_apply_delta: the grid's dimensions must be positive")
    return out.reshape(3, 4)


def affine_refine_params(**kw):
    """sift3d_amd_affine_refine_params: the defaults, overridden by free_mask, levels, max_evaluations, lambda0,
    lambda_factor, lambda_min, lambda_max, tol, min_overlap"""
    p = AffineRefineParams()
    lib().sift3d_amd_affine_refine_default_params(C.byref(p))
    names = [f[0] for f in AffineRefineParams._fields_]
    for k, v in kw.items():
        if k not in names:
            raise ValueError("refine_affine: unknown parameter %r" % (k,))
        setattr(p, k, v)
    return p


def _affine_refine(what, stem, F, M, A, params, work, mask_fixed, mask_moving, before=(), after=None):
    """The body of the affine refinement drivers, stem + "_device" sized by stem + "_work_bytes": the pair, A, `before`
    (the MI driver's bins and ranges), params (None: the defaults), the result, `after` (where the driver leaves its
    fit or measures), work, the stream, both masks.  after=None is the MSD driver, which takes nothing there and has
    its masked entry (_masked_entry).  Returns the AffineRefineResult."""
    head, masks = _pair(what, F, M, mask_fixed, mask_moving)
    a = _affine12(A, what)
    p = params if params is not None else affine_refine_params()
    stem, masks = _masked_entry(stem, masks) if after is None else (stem, masks or (None, None))
    need = getattr(lib(), stem + "_work_bytes")(*head[1:4], *head[5:8], p.levels)
    work = _byte_work(what, work, need, F, "levels must be in [1, %d]" % AFFINE_MAX_LEVELS)
    res = AffineRefineResult()
    _run(stem + "_device", *head, _dptr(a), *before, C.byref(p), C.byref(res), *(after or ()), work.data_ptr(),
         current_stream(), *masks)
    return res


def affine_refine(F, M, A, params=None, work=None, mask_fixed=None, mask_moving=None):
    """sift3d_amd_affine_refine_device on torch CUDA float32 contiguous volumes, on torch's current stream (the call
    waits for it once per evaluation).  Returns the AffineRefineResult.  mask_fixed, mask_moving: as similarity's
    (sift3d_amd_affine_refine_masked_device)."""
    return _affine_refine("affine_refine", "sift3d_amd_affine_refine", F, M, A, params, work, mask_fixed, mask_moving)


# ---- affine refinement under a linear intensity map (contract: "Affine refinement under a linear intensity map (NCC)")
AFFINE_NCC_RECORD_DTYPE = np.dtype([("n", "u8"), ("S_m", "f8"), ("S_f", "f8"), ("S_mm", "f8"), ("S_fm", "f8"),
                                    ("S_ff", "f8"), ("u", "f8", (12,)), ("v", "f8", (12,)), ("w", "f8", (12,)),
                                    ("H", "f8", (12, 12))])
assert AFFINE_NCC_RECORD_DTYPE.itemsize == AFFINE_NCC_BYTES


def affine_ncc_normal_work_bytes(fixed_shape=(1, 1, 1)):
    """sift3d_amd_affine_ncc_normal_work_bytes for a fixed grid (oz, oy, ox)"""
    oz, oy, ox = (int(v) for v in fixed_shape)
    return lib().sift3d_amd_affine_ncc_normal_work_bytes(ox, oy, oz)


def affine_ncc_record(record):
    """The record of affine_ncc_normal_equations() on the host, waiting for the stream: a numpy record of
    AFFINE_NCC_RECORD_DTYPE (n, S_m, S_f, S_mm, S_fm, S_ff, u, v, w [12], H [12, 12])."""
    import torch
    return record.view(torch.uint8)[:AFFINE_NCC_BYTES].cpu().numpy().view(AFFINE_NCC_RECORD_DTYPE)[0].copy()


def affine_ncc_normal_equations(F, M, A, record=None, work=None, raw=False, mask_fixed=None, mask_moving=None):
    """The sums of the Gauss-Newton normal equations of sum (alpha m + beta - f)^2 over A's 12 parameters and the
    linear intensity map (alpha, beta), of the fixed volume F [oz, oy, ox] and the moving volume M [nz, ny, nx] seen
    through the 3 x 4 pull map A (sift3d_hip_affine_ncc_normal_eqs), torch CUDA float32 contiguous, on torch's current
    stream.  Returns the record on the host as affine_ncc_record does (which waits for the stream), or with raw=True
    the device record.  record, work: the caller's buffers (int64 [186]; sift3d_amd_affine_ncc_normal_work_bytes
    bytes).  mask_fixed, mask_moving: as similarity's."""
    what = "affine_ncc_normal_equations"
    head, masks = _pair(what, F, M, mask_fixed, mask_moving)
    a = _affine12(A, what)
    record = _buffer(what, "record", record, (AFFINE_NCC_BYTES // 8,), F)
    work = _byte_work(what, work, lib().sift3d_amd_affine_ncc_normal_work_bytes(*head[1:4]), F)
    _run("sift3d_hip_affine_ncc_normal_eqs", *head, _dptr(a), record.data_ptr(), work.data_ptr(), current_stream(),
         *(masks or (None, None)))
    return record if raw else affine_ncc_record(record)


def _ncc_record(rec):
    """a host record (AFFINE_NCC_RECORD_DTYPE, or a mapping / object with its fields) as a 1-element array"""
    out = np.zeros(1, AFFINE_NCC_RECORD_DTYPE)
    for name in AFFINE_NCC_RECORD_DTYPE.names:
        out[name] = rec[name] if isinstance(rec, (dict, np.void, np.ndarray)) else getattr(rec, name)
    return out


def affine_ncc_fit(rec):
    """(alpha, beta, cost, ncc) of sift3d_amd_affine_ncc_fit (host) on a record: the regression of f on m, its mean
    squared residual and the correlation; None where the fit is undefined (n < 2 or no variance in m)."""
    r = _ncc_record(rec)
    out = np.zeros(4)
    rc = lib().sift3d_amd_affine_ncc_fit(r.ctypes.data, _dptr(out))
    return tuple(float(v) for v in out) if rc == 0 else None


def affine_ncc_lm_step(rec, free_mask=AFFINE_FREE_ALL, lam=0.0):
    """delta float64 [12] of sift3d_amd_affine_ncc_lm_step (host): the first 12 entries of the damped Gauss-Newton
    step over the freed parameters and (alpha, beta), 0 elsewhere; None where the entry refuses."""
    r = _ncc_record(rec)
    delta = np.zeros(12)
    rc = lib().sift3d_amd_affine_ncc_lm_step(r.ctypes.data, int(free_mask) & 0xFFFFFFFF, float(lam), _dptr(delta))
    return delta if rc == 0 else None


def affine_ncc_refine(F, M, A, params=None, work=None, mask_fixed=None, mask_moving=None):
    """sift3d_amd_affine_ncc_refine_device on torch CUDA float32 contiguous volumes, on torch's current stream (the
    call waits for it once per evaluation).  Returns (AffineRefineResult, fit float64 [4] = alpha, beta, cost, ncc at
    the final A).  mask_fixed, mask_moving: as similarity's."""
    fit = np.zeros(4)
    res = _affine_refine("affine_ncc_refine", "sift3d_amd_affine_ncc_refine", F, M, A, params, work, mask_fixed,
                         mask_moving, after=(_dptr(fit),))
    return res, fit


# ---- Mattes mutual-information affine refinement (contract: "Mutual-information affine refinement (Mattes)") ---------
PARZEN_MAX_BINS = 64
PARZEN_Q = 65536
ParzenMeasures = collections.namedtuple("ParzenMeasures", "n mi nmi entropy_fixed entropy_moving entropy_joint cost W")


def _parzen_bins(bins, what):
    bins = int(bins)
    if not 4 <= bins <= PARZEN_MAX_BINS:
        raise ValueError("%s: bins must be in [4, %d]" % (what, PARZEN_MAX_BINS))
    return bins


def _parzen_ranges(range_f, range_m):
    return tuple(float(np.float32(v)) for r in (range_f, range_m) for v in r)


def parzen_window(m, lo, hi, bins):
    """(k0, q uint32 [4], dw float64 [4], out) of sift3d_amd_parzen_window (host): the first of the four bins that the
    moving value m is spread over, the cubic B-spline weights in fixed point (2^16), their derivatives and whether m
    lies outside [lo, hi]; None where the entry refuses (bins outside [4, 64], a range that is not finite or empty)."""
    k0, out = C.c_int(), C.c_int()
    q = (C.c_uint32 * 4)()
    dw = (C.c_double * 4)()
    rc = lib().sift3d_amd_parzen_window(float(np.float32(m)), float(np.float32(lo)), float(np.float32(hi)), int(bins),
                                        C.byref(k0), q, dw, C.byref(out))
    return (k0.value, np.array(q[:], np.uint32), np.array(dw[:], np.float64), bool(out.value)) if rc == 0 else None


def parzen_histogram(F, M, A, bins, range_f, range_m, hist=None, work=None, mask_fixed=None, mask_moving=None):
    """The Parzen joint histogram in fixed point of the fixed volume F [oz, oy, ox] and the moving volume M [nz, ny, nx]
    seen through the 3 x 4 pull map A (sift3d_hip_parzen_hist_affine), torch CUDA float32 contiguous, on torch's current
    stream.  Returns (hist int64 [bins, bins] indexed [b_f, b_m], count int64 [1]) on the device; reading either waits
    for the stream.  hist, work: the caller's buffers (int64 [bins, bins]; sift3d_amd_parzen_hist_work_bytes bytes).
    mask_fixed, mask_moving: as similarity's."""
    what = "parzen_histogram"
    head, masks = _pair(what, F, M, mask_fixed, mask_moving)
    a = _affine12(A, what)
    return _parzen_hist(what, "sift3d_hip_parzen_hist_affine", F, head, masks, _dptr(a), bins, range_f, range_m, hist,
                        work)


def _parzen_hist(what, name, F, head, masks, T, bins, range_f, range_m, hist, work):
    """The body of the two Parzen histograms after the pair (_pair's head and masks) and the pull map or field T:
    returns (hist, count)."""
    import torch
    bins = _parzen_bins(bins, what)
    hist = _buffer(what, "hist", hist, (bins, bins), F, "[bins, bins]")
    count = torch.empty(1, dtype=torch.int64, device=F.device)
    work = _byte_work(what, work, lib().sift3d_amd_parzen_hist_work_bytes(*head[1:4]), F)
    _run(name, *head, T, bins, *_parzen_ranges(range_f, range_m), hist.data_ptr(), count.data_ptr(), work.data_ptr(),
         current_stream(), *(masks or (None, None)))
    return hist, count


def _parzen_table(what, W, F):
    """(W, bins) of the table W [bins, bins] that the MI kernels take psi from: a host array is uploaded to F's device
    as float64, a tensor must be contiguous float64 [bins, bins] there."""
    import torch
    if not isinstance(W, torch.Tensor):
        W = torch.from_numpy(np.ascontiguousarray(W, np.float64)).to(F.device)
    if W.dim() != 2 or W.shape[0] != W.shape[1]:
        raise ValueError(what + ": W must be [bins, bins]")
    bins = _parzen_bins(W.shape[0], what)
    _tensor(W, what + ": W must be a contiguous float64 tensor [bins, bins] on F's device", shape=(bins, bins),
            device=F.device, dtype="float64")
    return W, bins


def parzen_mi(hist):
    """ParzenMeasures(n, mi, nmi, entropy_fixed, entropy_moving, entropy_joint, cost, W) of sift3d_amd_parzen_mi (host)
    on a histogram [bins, bins] (a tensor is copied to the host, which waits for its stream): n the histogram's total,
    cost = -mi, W float64 [bins, bins] the table log(hist / column sum) that affine_mi_normal_equations takes."""
    if hasattr(hist, "cpu"):
        hist = hist.cpu().numpy()
    h = np.ascontiguousarray(hist).astype(np.uint64)
    if h.ndim != 2 or h.shape[0] != h.shape[1]:
        raise ValueError("parzen_mi: hist must be [bins, bins]")
    bins = _parzen_bins(h.shape[0], "parzen_mi")
    out = Similarity()
    W = np.zeros((bins, bins))
    _check(lib().sift3d_amd_parzen_mi(h.ctypes.data, bins, C.byref(out), W.ctypes.data), "sift3d_amd_parzen_mi")
    return ParzenMeasures(int(out.n), out.mi, out.nmi, out.entropy_fixed, out.entropy_moving, out.entropy_joint,
                          -out.mi, W)


def affine_mi_normal_equations(F, M, A, W, range_f, range_m, record=None, work=None, raw=False, mask_fixed=None,
                               mask_moving=None):
    """The Fisher-scoring normal equations of the mutual information over A's 12 parameters
    (sift3d_hip_affine_mi_normal_eqs): the MSD record with the pseudo-gradient psi * g and the pseudo-residual -1, psi
    from the table W [bins, bins] (float64; a numpy array is uploaded, a CUDA tensor is used as it is).  Returns
    (n, S_pp, b [12], H [12, 12]) on the host as affine_normal_equations does, or with raw=True the device record.
    record, work: the caller's buffers (int64 [158]; sift3d_amd_affine_normal_work_bytes bytes).  mask_fixed,
    mask_moving: as similarity's."""
    what = "affine_mi_normal_equations"
    head, masks = _pair(what, F, M, mask_fixed, mask_moving)
    a = _affine12(A, what)
    W, bins = _parzen_table(what, W, F)
    record = _buffer(what, "record", record, (AFFINE_NORMAL_BYTES // 8,), F)
    work = _byte_work(what, work, lib().sift3d_amd_affine_normal_work_bytes(*head[1:4]), F)
    _run("sift3d_hip_affine_mi_normal_eqs", *head, _dptr(a), bins, *_parzen_ranges(range_f, range_m), W.data_ptr(),
         record.data_ptr(), work.data_ptr(), current_stream(), *(masks or (None, None)))
    return record if raw else affine_normal_record(record)


def affine_mi_refine(F, M, A, bins, range_f, range_m, params=None, work=None, mask_fixed=None, mask_moving=None):
    """sift3d_amd_affine_mi_refine_device on torch CUDA float32 contiguous volumes, on torch's current stream (the call
    waits for it once per pass).  Returns (AffineRefineResult, Similarity: the measures at the final A, n the
    histogram's total).  mask_fixed, mask_moving: as similarity's."""
    what = "affine_mi_refine"
    sim = Similarity()
    res = _affine_refine(what, "sift3d_amd_affine_mi_refine", F, M, A, params, work, mask_fixed, mask_moving,
                         before=(_parzen_bins(bins, what), *_parzen_ranges(range_f, range_m)), after=(C.byref(sim),))
    return res, sim


# ---- initial transforms (contract: include/sift3d_amd.h, "Initial transforms: moments and candidate search") ----
MOMENTS_WEIGHT = {"intensity": 0, "binary": 1}
INIT_MODE = {"centroid": 0, "axes": 1, "search": 2}
INIT_METRIC = {"msd": 0, "ncc": 1, "mi": 2}
MOMENTS_DTYPE = np.dtype([("n", "u8"), ("S0", "f8"), ("S1", "f8", (3,)), ("S2", "f8", (6,))])
assert MOMENTS_DTYPE.itemsize == MOMENTS_BYTES


def _named(table, value, what, name):
    if value not in table:
        raise ValueError("%s: %s must be one of %s, not %r" % (what, name, sorted(table), value))
    return table[value]


def moments_record(record):
    """The record of moments() on the host, waiting for the stream: a numpy record (n, S0, S1 [3], S2 [6])."""
    import torch
    return record.view(torch.uint8)[:MOMENTS_BYTES].cpu().numpy().view(MOMENTS_DTYPE)[0].copy()


def moments(V, weight="binary", floor=0.0, mask=None, record=None, work=None, raw=False):
    """The count, mass and first and second moments about the grid's centre of the voxels of V [nz, ny, nx] above
    `floor` (sift3d_hip_moments), torch CUDA float32 contiguous, on torch's current stream.  weight: "binary" or
    "intensity".  mask: a float32 mask of V's shape (in where >= 0.5) or None.  Returns the record on the host (which
    waits for the stream; moments_record), or with raw=True the device record.  record, work: the caller's buffers
    (int64 [11]; sift3d_amd_moments_work_bytes bytes)."""
    what = "moments"
    _tensor(V, what + ": V must be a contiguous 3-D float32 CUDA tensor", dims=(3,))
    if mask is not None:
        _tensor(mask, "%s: mask must be a contiguous float32 CUDA tensor of V's shape %s on V's device"
                % (what, tuple(V.shape)), shape=tuple(V.shape), device=V.device)
    nz, ny, nx = V.shape
    record = _buffer(what, "record", record, (MOMENTS_BYTES // 8,), V)
    work = _byte_work(what, work, lib().sift3d_amd_moments_work_bytes(nx, ny, nz), V)
    _run("sift3d_hip_moments", V.data_ptr(), nx, ny, nz, None if mask is None else mask.data_ptr(),
         _named(MOMENTS_WEIGHT, weight, what, "weight"), float(np.float32(floor)), record.data_ptr(), work.data_ptr(),
         current_stream())
    return record if raw else moments_record(record)


def moments_frame(record, shape):
    """(centroid [3], axes [3, 3] with the eigenvectors as rows, lambda [3]) of sift3d_amd_moments_frame (host) for a
    moments record of a grid shape = (nz, ny, nx), (x, y, z) order throughout; None where the entry refuses (nothing
    counted, or not finite)."""
    rec = np.zeros(1, MOMENTS_DTYPE)
    rec[0] = record
    nz, ny, nx = (int(v) for v in shape)
    c, a, lam = np.zeros(3), np.zeros(9), np.zeros(3)
    if lib().sift3d_amd_moments_frame(rec.ctypes.data, nx, ny, nz, _dptr(c), _dptr(a), _dptr(lam)) != 0:
        return None
    return c, a.reshape(3, 3), lam


def _affine_list(A, what):
    a = np.ascontiguousarray(A, np.float64)
    if a.ndim < 2 or a.shape[1:] not in ((3, 4), (12,)):
        raise ValueError("%s: A must be K affine pull maps [K, 3, 4]" % what)
    return a.reshape(len(a), 12).copy()


def similarity_batch(F, M, A, bins=0, range_f=(0.0, 1.0), range_m=(0.0, 1.0), interp="linear", hist=None, stats=None,
                     work=None, mask_fixed=None, mask_moving=None):
    """similarity() for K affine pull maps A [K, 3, 4] in one call (sift3d_hip_similarity_affine_batch / _masked), on
    torch's current stream: candidate k's histogram and stats record are similarity()'s for A[k], byte for byte.
    bins=0: no histograms (MSD and NCC need none).  Returns (hist int64 [K, bins, bins] or None, stats int64 [K, 7]:
    row k read with similarity_stats).  hist, stats, work: the caller's buffers
    (sift3d_amd_similarity_batch_work_bytes bytes).  mask_fixed, mask_moving: as similarity's."""
    what = "similarity_batch"
    head, masks = _pair(what, F, M, mask_fixed, mask_moving)
    mode = _interp(interp)
    a = _affine_list(A, what)
    K, bins = len(a), int(bins)
    if not 1 <= K <= SIMILARITY_BATCH_MAX:
        raise ValueError("%s: K must be in [1, %d]" % (what, SIMILARITY_BATCH_MAX))
    if bins != 0 and not 2 <= bins <= SIMILARITY_MAX_BINS:
        raise ValueError("%s: bins must be 0 or in [2, %d]" % (what, SIMILARITY_MAX_BINS))
    if bins == 0 and hist is not None:
        raise ValueError("%s: bins=0 takes no hist" % what)
    if bins:
        hist = _buffer(what, "hist", hist, (K, bins, bins), F, "[K, bins, bins]")
    stats = _buffer(what, "stats", stats, (K, SIMILARITY_STATS_BYTES // 8), F)
    work = _byte_work(what, work, lib().sift3d_amd_similarity_batch_work_bytes(*head[1:4], bins, K), F,
                      "the fixed grid has too many tiles")
    (lo_f, hi_f), (lo_m, hi_m) = ((float(np.float32(v)) for v in r) for r in (range_f, range_m))
    name, masks = _masked_entry("sift3d_hip_similarity_affine_batch", masks)
    _run(name, *head, _dptr(a), K, mode, bins, lo_f, hi_f, lo_m, hi_m, hist.data_ptr() if bins else None,
         stats.data_ptr(), work.data_ptr(), current_stream(), *masks)
    return hist, stats


def affine_init_params(**kw):
    """sift3d_amd_affine_init_params: the defaults, overridden by mode, metric and weight (names or numbers), levels,
    floor_f, floor_m, bins, lo_f, hi_f, lo_m, hi_m, range_deg and range_vox (a number or three, about / along x, y, z),
    step_deg, step_vox, min_overlap"""
    p = AffineInitParams()
    lib().sift3d_amd_affine_init_default_params(C.byref(p))
    names = [f[0] for f in AffineInitParams._fields_]
    tables = {"mode": INIT_MODE, "metric": INIT_METRIC, "weight": MOMENTS_WEIGHT}
    for k, v in kw.items():
        if k not in names:
            raise ValueError("affine_init: unknown parameter %r" % (k,))
        if k in tables and isinstance(v, str):
            v = _named(tables[k], v, "affine_init", k)
        if k in ("range_deg", "range_vox"):
            v = (C.c_double * 3)(*(np.broadcast_to(np.asarray(v, np.float64), (3,))))
        setattr(p, k, v)
    return p


def _frame(f, what):
    if isinstance(f, Frame):
        return f
    c, a, lam = f
    out = Frame()
    out.centroid[:] = np.asarray(c, np.float64).reshape(3)
    out.axes[:] = np.asarray(a, np.float64).reshape(9)
    out.lambda_[:] = np.asarray(lam, np.float64).reshape(3)
    return out


def affine_init_candidates(mode, frame_F, frame_M, params=None):
    """A [K, 3, 4] of sift3d_amd_affine_init_candidates (host): the candidate pull maps of `mode` ("centroid", "axes",
    "search") about the two frames, each (centroid, axes, lambda) as moments_frame returns it or a Frame; params: an
    AffineInitParams for the search ranges (None: the defaults)."""
    what = "affine_init_candidates"
    fF, fM = _frame(frame_F, what), _frame(frame_M, what)
    mode = _named(INIT_MODE, mode, what, "mode") if isinstance(mode, str) else int(mode)
    pp = None if params is None else C.byref(params)
    K = C.c_int(0)
    if lib().sift3d_amd_affine_init_candidates(mode, C.byref(fF), C.byref(fM), pp, None, C.byref(K)) != 0:
        raise ValueError("%s: %s" % (what, lib().sift3d_hip_last_error().decode() or "refused"))
    A = np.zeros((K.value, 12))
    if lib().sift3d_amd_affine_init_candidates(mode, C.byref(fF), C.byref(fM), pp, _dptr(A), C.byref(K)) != 0:
        raise ValueError("%s: refused" % what)
    return A.reshape(-1, 3, 4)


def affine_init_rank(metric, stats, hist=None, min_overlap=0.5):
    """(costs float64 [K], counts uint64 [K], order: the eligible candidates by ascending cost) of
    sift3d_amd_affine_init_rank (host) on K stats records (int64 [K, 7], host or device) and, for "mi", K histograms
    [K, bins, bins]; order is empty where the entry finds no candidate eligible."""
    import torch
    what = "affine_init_rank"
    metric = _named(INIT_METRIC, metric, what, "metric") if isinstance(metric, str) else int(metric)

    def host(t, dtype):
        return np.ascontiguousarray(t.cpu().numpy() if isinstance(t, torch.Tensor) else t).view(dtype)
    st = host(stats, np.uint64).reshape(-1, SIMILARITY_STATS_BYTES // 8)
    K = len(st)
    bins = 0
    hp = None
    if hist is not None:
        hs = host(hist, np.uint64)
        if hs.ndim != 3 or hs.shape[0] != K or hs.shape[1] != hs.shape[2]:
            raise ValueError("%s: hist must be [K, bins, bins]" % what)
        bins, hp = hs.shape[1], hs.ctypes.data
    if not (metric in INIT_METRIC.values() and 1 <= K <= INIT_MAX_CANDIDATES and 0 <= min_overlap <= 1
            and (metric != INIT_METRIC["mi"] or (hp is not None and 2 <= bins <= SIMILARITY_MAX_BINS))):
        raise ValueError("%s: K in [1, %d], min_overlap in [0, 1] and, for \"mi\", histograms of 2 to %d bins"
                         % (what, INIT_MAX_CANDIDATES, SIMILARITY_MAX_BINS))
    cost, n, order = np.zeros(K), np.zeros(K, np.uint64), np.zeros(K, np.int32)
    m = C.c_int(0)
    lib().sift3d_amd_affine_init_rank(metric, K, st.ctypes.data, hp, bins, float(min_overlap), _dptr(cost),
                                      n.ctypes.data, order.ctypes.data, C.byref(m))      # -1: none eligible, m == 0
    return cost, n, order[:m.value].copy()


def affine_init(F, M, params=None, work=None, mask_fixed=None, mask_moving=None):
    """sift3d_amd_affine_init_device on torch CUDA float32 contiguous volumes, on torch's current stream (the call waits
    for it once for the moments and once per chunk of candidates).  params: an AffineInitParams (None: the defaults).
    Returns (AffineInitResult, costs float64 [K], counts uint64 [K]); RuntimeError where the library refuses or finds
    no candidate eligible.  mask_fixed, mask_moving: as similarity's."""
    what = "affine_init"
    head, masks = _pair(what, F, M, mask_fixed, mask_moving)
    p = params if params is not None else affine_init_params()
    need = lib().sift3d_amd_affine_init_work_bytes(*head[1:4], *head[5:8], C.byref(p))
    work = _byte_work(what, work, need, F, "a parameter is out of range")
    K = C.c_int(0)
    f = Frame()
    if lib().sift3d_amd_affine_init_candidates(p.mode, C.byref(f), C.byref(f), C.byref(p), None, C.byref(K)) != 0:
        raise ValueError("%s: a parameter is out of range" % what)
    costs, counts = np.full(K.value, np.nan), np.zeros(K.value, np.uint64)
    res = AffineInitResult()
    _run("sift3d_amd_affine_init_device", *head, *(masks or (None, None)), C.byref(p), C.byref(res), _dptr(costs),
         counts.ctypes.data, work.data_ptr(), current_stream())
    return res, costs, counts


# ---- B-spline free-form deformation (contract: include/sift3d_amd.h, "B-spline free-form deformation") ----
FFD_STOPS = ("converged", "evaluations", "flat", "failed")
_FFD_TRAIL = AFFINE_MAX_LEVELS * FFD_MAX_EVALUATIONS       # the entries of a driver's trail and of the terms' beside it
FFD_HEAD_DTYPE = np.dtype([("n", "u8"), ("see", "f8"), ("R", "f8"), ("gmax", "f8")])
assert FFD_HEAD_DTYPE.itemsize == FFD_RECORD_HEAD_BYTES


def ffd_spacing(spacing, what="ffd"):
    """(dx, dy, dz) from an int or three ints in x, y, z order"""
    d = tuple(spacing) if isinstance(spacing, (tuple, list, np.ndarray, C.Array)) else (spacing,) * 3
    if len(d) != 3 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or
                          not 1 <= int(v) <= FFD_MAX_SPACING for v in d):
        raise ValueError("%s: spacing must be an integer or three (x, y, z) in [1, %d]" % (what, FFD_MAX_SPACING))
    return tuple(int(v) for v in d)


def ffd_lattice_shape(out_shape, spacing):
    """[3, gz, gy, gx] of the lattice over a grid (oz, oy, ox) (sift3d_amd_ffd_lattice_dim)"""
    oz, oy, ox = (int(v) for v in out_shape)
    dx, dy, dz = ffd_spacing(spacing)
    g = [lib().sift3d_amd_ffd_lattice_dim(o, d) for o, d in ((oz, dz), (oy, dy), (ox, dx))]
    if 0 in g:
        raise ValueError("ffd_lattice_shape: the grid's dimensions must be positive")
    return (3,) + tuple(g)


def ffd_weights(delta):
    """the table w [delta, 4] float32 of sift3d_amd_ffd_weights (host)"""
    if isinstance(delta, bool) or not isinstance(delta, (int, np.integer)) or not 1 <= int(delta) <= FFD_MAX_SPACING:
        raise ValueError("ffd_weights: spacing must be in [1, %d]" % FFD_MAX_SPACING)
    w = np.zeros((int(delta), 4), np.float32)
    if lib().sift3d_amd_ffd_weights(int(delta), w.ctypes.data) != 0:
        raise ValueError("ffd_weights: refused")
    return w


def _ffd_lattice(lattice, what):
    _tensor(lattice, "%s: lattice must be a contiguous float32 CUDA tensor [3, gz, gy, gx]" % what, dims=(4,), lead=3)
    _, gz, gy, gx = lattice.shape
    return gx, gy, gz


def _ffd_A(A, what):
    return (None, None) if A is None else (lambda a: (a, _dptr(a)))(_affine12(A, what))


def ffd_field(lattice, spacing, field, A=None, work=None):
    """field [3, oz, oy, ox] = the displacement field of the control lattice [3, gz, gy, gx] at integer spacing
    (dx, dy, dz), through the 3 x 4 pull map A when given (sift3d_hip_ffd_field), on torch's current stream."""
    gx, gy, gz = _ffd_lattice(lattice, "ffd_field")
    _field_tensor(field, "ffd_field")
    _same_device("ffd_field", lattice, field)
    dx, dy, dz = ffd_spacing(spacing, "ffd_field")
    _, oz, oy, ox = field.shape
    a, ap = _ffd_A(A, "ffd_field")
    work = _work(work, (lib().sift3d_amd_ffd_field_work_bytes(dx, dy, dz) + 3) // 4, lattice, "ffd_field")
    _check(lib().sift3d_hip_ffd_field(lattice.data_ptr(), gx, gy, gz, dx, dy, dz, ap, ox, oy, oz, field.data_ptr(),
                                      work.data_ptr(), current_stream()), "sift3d_hip_ffd_field")
    return field


def ffd_record(record, lattice_shape):
    """A device record on the host, waiting for the stream: (n, S_ee, R, gmax, Gc float64 [3, gz, gy, gx], dR same)"""
    import torch
    raw = record.view(torch.uint8).cpu().numpy()
    head = raw[:FFD_RECORD_HEAD_BYTES].view(FFD_HEAD_DTYPE)[0]
    m = int(np.prod(lattice_shape))
    body = raw[FFD_RECORD_HEAD_BYTES:FFD_RECORD_HEAD_BYTES + 16 * m].view(np.float64)
    return (int(head["n"]), float(head["see"]), float(head["R"]), float(head["gmax"]),
            body[:m].reshape(lattice_shape).copy(), body[m:].reshape(lattice_shape).copy())


def _ffd_record_tensor(lattice):
    import torch
    _, gz, gy, gx = lattice.shape
    return torch.zeros(lib().sift3d_amd_ffd_record_bytes(gx, gy, gz) // 8, dtype=torch.int64, device=lattice.device)


def ffd_evaluate(F, M, lattice, spacing, A=None, bending=0.0, work=None, mask_fixed=None, mask_moving=None):
    """One evaluation of the FFD cost at `lattice` (sift3d_hip_ffd_evaluate) on torch's current stream.  Returns
    (record, grad, field): the device record (read it with ffd_record), the float32 gradient lattice and the field.
    mask_fixed, mask_moving: as similarity's (sift3d_hip_ffd_evaluate_masked)."""
    what = "ffd_evaluate"
    _ffd_lattice(lattice, what)
    head, masks = _pair(what, F, M, mask_fixed, mask_moving, lattice)
    args, out, work = _ffd_evaluate_args(what, head, F, lattice, spacing, A, bending, work)
    name, masks = _masked_entry("sift3d_hip_ffd_evaluate", masks)
    _run(name, *args, *masks)
    return out


def _ffd_outputs(F, lattice):
    """(record, grad, field) of an FFD evaluation at `lattice` over the grid of the volume or stack F: the record
    cleared (ffd_record reads its whole length), the float32 gradient lattice and the field [3, oz, oy, ox]"""
    import torch
    return (_ffd_record_tensor(lattice), torch.empty_like(lattice),
            torch.empty((3,) + tuple(F.shape[-3:]), dtype=torch.float32, device=F.device))


def _ffd_evaluate_args(what, head, F, lattice, spacing, A, bending, work,
                       bytes_of="sift3d_amd_ffd_evaluate_work_bytes"):
    """What the FFD evaluation entries take up to the stream, from the pair's `head` (the stacks': with nc) on: the
    lattice and spacing, A, bending, the outputs of _ffd_outputs and the work buffer (the caller's, or `bytes_of` bytes
    allocated here).  Returns (args, (record, grad, field), work)."""
    gx, gy, gz = _ffd_lattice(lattice, what)
    d = ffd_spacing(spacing, what)
    a, ap = _ffd_A(A, what)
    record, grad, field = out = _ffd_outputs(F, lattice)
    work = _byte_work(what, work, getattr(lib(), bytes_of)(*head[1:4], *d), F)
    return (*head, lattice.data_ptr(), gx, gy, gz, *d, ap, float(bending), field.data_ptr(), record.data_ptr(),
            grad.data_ptr(), work.data_ptr(), current_stream()), out, work


def ffd_bending(lattice, spacing, work=None):
    """(R, dR float64 [3, gz, gy, gx]) of sift3d_hip_ffd_bending, on the host (waits for the stream)"""
    gx, gy, gz = _ffd_lattice(lattice, "ffd_bending")
    dx, dy, dz = ffd_spacing(spacing, "ffd_bending")
    record = _ffd_record_tensor(lattice)
    work = _work(work, (lib().sift3d_amd_ffd_bending_work_bytes(gx, gy, gz) + 3) // 4, lattice, "ffd_bending")
    _check(lib().sift3d_hip_ffd_bending(lattice.data_ptr(), gx, gy, gz, dx, dy, dz, record.data_ptr(),
                                        work.data_ptr(), current_stream()), "sift3d_hip_ffd_bending")
    rec = ffd_record(record, tuple(lattice.shape))
    return rec[2], rec[5]


def ffd_refine2(coarse, out_shape, spacing):
    """The lattice over the grid out_shape = (oz, oy, ox) from the lattice over the grid half as fine
    (sift3d_hip_ffd_refine2), on torch's current stream."""
    import torch
    _ffd_lattice(coarse, "ffd_refine2")
    oz, oy, ox = (int(v) for v in out_shape)
    dx, dy, dz = ffd_spacing(spacing, "ffd_refine2")
    if tuple(coarse.shape) != ffd_lattice_shape(((oz + 1) // 2, (oy + 1) // 2, (ox + 1) // 2), (dx, dy, dz)):
        raise ValueError("ffd_refine2: coarse is not the lattice over the grid half as fine as out_shape")
    fine = torch.empty(ffd_lattice_shape((oz, oy, ox), (dx, dy, dz)), dtype=torch.float32, device=coarse.device)
    _check(lib().sift3d_hip_ffd_refine2(coarse.data_ptr(), ox, oy, oz, dx, dy, dz, fine.data_ptr(), current_stream()),
           "sift3d_hip_ffd_refine2")
    return fine


def ffd_refine_params(**kw):
    """sift3d_amd_ffd_refine_params: the defaults, overridden by spacing (dx, dy, dz), levels, max_evaluations,
    bending, step0, step_max, tol, min_overlap"""
    p = FFDRefineParams()
    lib().sift3d_amd_ffd_refine_default_params(C.byref(p))
    names = [f[0] for f in FFDRefineParams._fields_]
    for k, v in kw.items():
        if k not in names:
            raise ValueError("refine_ffd: unknown parameter %r" % (k,))
        if k == "spacing":
            v = (C.c_int * 3)(*ffd_spacing(v, "refine_ffd"))
        setattr(p, k, v)
    return p


def ffd_refine(F, M, A=None, params=None, work=None, mask_fixed=None, mask_moving=None):
    """sift3d_amd_ffd_refine_device on torch CUDA float32 contiguous volumes, on torch's current stream (the call
    waits for it once per evaluation).  Returns (FFDRefineResult, lattice, field).  mask_fixed, mask_moving: as
    similarity's (sift3d_amd_ffd_refine_masked_device)."""
    return _ffd_refine_pair("ffd_refine", "sift3d_amd_ffd_refine", F, M, A, params, work, mask_fixed, mask_moving)


def _ffd_refine(what, stem, head, like, grid, ap, p, work, need, refuses, tail):
    """The body of every FFD refinement driver, stem + "_device": after `head` (the pair, or the levels' table) it
    takes A (ap: _ffd_A's pointer), params, the result, the lattice over `grid` = (oz, oy, ox) and the field, allocated
    here on the device of `like`, the work buffer of `need` bytes (0: ValueError with `refuses`), the stream, and
    `tail`.  Returns (FFDRefineResult, lattice, field)."""
    import torch
    work = _byte_work(what, work, need, like, refuses)
    lattice = torch.empty(ffd_lattice_shape(grid, tuple(p.spacing)), dtype=torch.float32, device=like.device)
    field = torch.empty((3,) + tuple(grid), dtype=torch.float32, device=like.device)
    res = FFDRefineResult()
    _run(stem + "_device", *head, ap, C.byref(p), C.byref(res), lattice.data_ptr(), field.data_ptr(), work.data_ptr(),
         current_stream(), *tail)
    return res, lattice, field


def _ffd_refine_pair(what, stem, F, M, A, params, work, mask_fixed, mask_moving, tail=None, count=()):
    """_ffd_refine for the drivers over one pair of volumes, sized by stem + "_work_bytes" of the two grids, the
    spacing, the levels and `count` (the landmarks').  params None: the defaults.  tail: what the general drivers take
    after both masks; None is the MSD driver, which has its masked entry (_masked_entry)."""
    head, masks = _pair(what, F, M, mask_fixed, mask_moving)
    a, ap = _ffd_A(A, what)
    p = params if params is not None else ffd_refine_params()
    stem, tail = _masked_entry(stem, masks) if tail is None else (stem, (*(masks or (None, None)), *tail))
    need = getattr(lib(), stem + "_work_bytes")(*head[1:4], *head[5:8], *p.spacing, p.levels, *count)
    return _ffd_refine(what, stem, head, F, F.shape, ap, p, work, need,
                       "levels must be in [1, %d] and the spacing in [1, %d]" % (AFFINE_MAX_LEVELS, FFD_MAX_SPACING),
                       tail)


def _trail(entries, res, *fields):
    """What a driver left beside its trail (FFDPenalty, FFDLandmarkTerm), one tuple of `fields` per evaluation; None
    where the term was not asked for"""
    return None if entries is None else [tuple(getattr(e, f) for f in fields) for e in entries[:res.evaluations]]


# ---- Mattes mutual-information free-form deformation ("Mutual-information free-form deformation (Mattes)") ----
def parzen_histogram_field(F, M, field, bins, range_f, range_m, hist=None, work=None, mask_fixed=None,
                           mask_moving=None):
    """parzen_histogram with the displacement field [3, oz, oy, ox] in the place of A (sift3d_hip_parzen_hist_field):
    (hist int64 [bins, bins], count int64 [1]) on the device, on torch's current stream."""
    what = "parzen_histogram_field"
    _field_tensor(field, what)
    head, masks = _pair(what, F, M, mask_fixed, mask_moving, field)
    if tuple(field.shape[1:]) != tuple(F.shape):
        raise ValueError(what + ": the field must be [3, oz, oy, ox] on F's grid")
    return _parzen_hist(what, "sift3d_hip_parzen_hist_field", F, head, masks, field.data_ptr(), bins, range_f, range_m,
                        hist, work)


def ffd_mi_evaluate(F, M, lattice, spacing, W, range_f, range_m, A=None, bending=0.0, work=None, mask_fixed=None,
                    mask_moving=None):
    """ffd_evaluate for the mutual information (sift3d_hip_ffd_mi_evaluate): psi from the table W [bins, bins] (float64;
    a numpy array is uploaded, a CUDA tensor is used as it is).  Returns (record, grad, field); ffd_record reads the
    record, whose S_ee slot holds S_pp."""
    what = "ffd_mi_evaluate"
    _ffd_lattice(lattice, what)
    head, masks = _pair(what, F, M, mask_fixed, mask_moving, lattice)
    W, bins = _parzen_table(what, W, F)
    args, out, work = _ffd_evaluate_args(what, head, F, lattice, spacing, A, bending, work)
    _run("sift3d_hip_ffd_mi_evaluate", *args, *(masks or (None, None)), bins, *_parzen_ranges(range_f, range_m),
         W.data_ptr())
    return out


def ffd_mi_refine(F, M, bins, range_f, range_m, A=None, params=None, work=None, mask_fixed=None, mask_moving=None):
    """sift3d_amd_ffd_mi_refine_device on torch CUDA float32 contiguous volumes, on torch's current stream (the call
    waits for it once per evaluation and once per gradient).  Returns (FFDRefineResult, lattice, field, Similarity: the
    measures at the final lattice)."""
    what = "ffd_mi_refine"
    sim = Similarity()
    tail = (_parzen_bins(bins, what), *_parzen_ranges(range_f, range_m), C.byref(sim))
    return (*_ffd_refine_pair(what, "sift3d_amd_ffd_mi_refine", F, M, A, params, work, mask_fixed, mask_moving, tail),
            sim)


# ---- Jacobian penalty ("Jacobian penalty") ----
def _term_record(record, nbytes):
    """a term's device record, a count and three doubles in its first nbytes = 32, on the host; waits for the stream"""
    import torch
    raw = record.view(torch.uint8)[:nbytes].cpu().numpy()
    v = raw[8:32].view(np.float64)
    return int(raw[:8].view(np.uint64)[0]), float(v[0]), float(v[1]), float(v[2])


def jacobian_penalty_record(record):
    """(nonpos, sum, rmin, rmax) of a penalty record (a CUDA tensor of JACOBIAN_PENALTY_RECORD_BYTES); waits for the
    stream"""
    return _term_record(record, JACOBIAN_PENALTY_RECORD_BYTES)


def jacobian_penalty(field, ref=1.0, gradient=False, work=None):
    """sift3d_hip_jacobian_penalty on torch's current stream: field [3, oz, oy, ox] torch CUDA float32, ref the
    reference determinant.  Returns (record: int64 CUDA tensor, read by jacobian_penalty_record; S: float64 CUDA tensor
    [3, oz, oy, ox], the gradient in sum form, or None)."""
    import torch
    what = "jacobian_penalty"
    _field_tensor(field, what)
    _, oz, oy, ox = field.shape
    need = lib().sift3d_amd_jacobian_penalty_work_bytes(ox, oy, oz)
    work = _work(work, (need + 3) // 4, field, what)
    record = torch.empty(JACOBIAN_PENALTY_RECORD_BYTES // 8, dtype=torch.int64, device=field.device)
    S = torch.empty((3, oz, oy, ox), dtype=torch.float64, device=field.device) if gradient else None
    _check(lib().sift3d_hip_jacobian_penalty(field.data_ptr(), ox, oy, oz, float(ref), record.data_ptr(),
                                             None if S is None else S.data_ptr(), work.data_ptr(), current_stream()),
           "sift3d_hip_jacobian_penalty")
    return record, S


def ffd_jacobian_gradient(field, spacing, ref=1.0, work=None):
    """sift3d_hip_ffd_jacobian_gradient on torch's current stream: (record, GJ float64 CUDA tensor [3, gz, gy, gx]), the
    penalty of the field and the derivative of its sum over the control lattice of the field's grid at `spacing`"""
    import torch
    what = "ffd_jacobian_gradient"
    _field_tensor(field, what)
    _, oz, oy, ox = field.shape
    dx, dy, dz = ffd_spacing(spacing, what)
    need = lib().sift3d_amd_ffd_jacobian_gradient_work_bytes(ox, oy, oz, dx, dy, dz)
    work = _work(work, (need + 3) // 4, field, what)
    record = torch.empty(JACOBIAN_PENALTY_RECORD_BYTES // 8, dtype=torch.int64, device=field.device)
    GJ = torch.empty(ffd_lattice_shape((oz, oy, ox), (dx, dy, dz)), dtype=torch.float64, device=field.device)
    _check(lib().sift3d_hip_ffd_jacobian_gradient(field.data_ptr(), ox, oy, oz, dx, dy, dz, float(ref),
                                                  record.data_ptr(), GJ.data_ptr(), work.data_ptr(), current_stream()),
           "sift3d_hip_ffd_jacobian_gradient")
    return record, GJ


def ffd_refine_jacobian(F, M, jacobian, bins=0, range_f=(0.0, 1.0), range_m=(0.0, 1.0), A=None, params=None, work=None,
                        mask_fixed=None, mask_moving=None):
    """sift3d_amd_ffd_refine_jacobian_device on torch CUDA float32 contiguous volumes, on torch's current stream: the
    FFD drivers with the Jacobian penalty of weight `jacobian`; bins == 0: the MSD (the ranges are not read), else the
    mutual information as ffd_mi_refine.  Returns (FFDRefineResult, lattice, field, Similarity or None, penalty: one
    (P, rmin, nonpos) per trail entry)."""
    what = "ffd_refine_jacobian"
    bins = _parzen_bins(bins, what) if bins else 0
    ranges = _parzen_ranges(range_f, range_m) if bins else (0.0, 1.0, 0.0, 1.0)
    sim, pen = Similarity(), (FFDPenalty * _FFD_TRAIL)()
    res, lattice, field = _ffd_refine_pair(what, "sift3d_amd_ffd_refine_jacobian", F, M, A, params, work, mask_fixed,
                                           mask_moving, (bins, *ranges, C.byref(sim), float(jacobian), pen))
    return res, lattice, field, (sim if bins else None), _trail(pen, res, "P", "rmin", "nonpos")


# ---- points and landmarks ("FFD landmarks") ----
def _points(a, what, name):
    """an n x 3 array as contiguous float64 on the host"""
    a = np.ascontiguousarray(a, np.float64)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("%s: %s must be n x 3 (x, y, z)" % (what, name))
    return a


def ffd_landmark_arrays(P, Q, w, what):
    """(P, Q, w or None) as the entries take them; ValueError on what they refuse of the landmarks"""
    P, Q = _points(P, what, "the fixed landmarks"), _points(Q, what, "the moving landmarks")
    if len(P) != len(Q) or not 1 <= len(P) <= FFD_MAX_LANDMARKS:
        raise ValueError("%s: the two point lists must have one length in [1, %d]" % (what, FFD_MAX_LANDMARKS))
    if not np.isfinite(Q).all():
        raise ValueError("%s: the moving landmarks must be finite" % what)
    if w is not None:
        w = np.ascontiguousarray(w, np.float64)
        if w.shape != (len(P),) or not np.isfinite(w).all() or (w < 0).any():
            raise ValueError("%s: the landmark weights must be n finite values that are not negative" % what)
    return P, Q, w


def _landmark_args(P, Q, w, landmark_weight):
    """ffd_landmark_arrays' three and the term's weight as the evaluation and the driver with landmarks take them"""
    return P.ctypes.data, Q.ctypes.data, None if w is None else w.ctypes.data, len(P), float(landmark_weight)


def ffd_points(lattice, spacing, points, A=None):
    """T [m, 3] float64 CUDA tensor: the points [m, 3] (float64, x y z in voxels of the fixed grid; a CUDA tensor is
    used as it is, an array is uploaded) through the lattice and the pull map A (sift3d_hip_ffd_points), on torch's
    current stream; three NaNs where a point is outside the lattice's support."""
    import torch
    what = "ffd_points"
    gx, gy, gz = _ffd_lattice(lattice, what)
    dx, dy, dz = ffd_spacing(spacing, what)
    if not isinstance(points, torch.Tensor):
        points = torch.from_numpy(_points(points, what, "points")).to(lattice.device)
    _tensor(points, what + ": points must be a contiguous float64 CUDA tensor [m, 3] on the lattice's device",
            dims=(2,), device=lattice.device, dtype="float64")
    if points.shape[1] != 3 or points.shape[0] < 1:
        raise ValueError(what + ": points must be [m, 3] with m >= 1")
    a, ap = _ffd_A(A, what)
    T = torch.empty_like(points)
    _check(lib().sift3d_hip_ffd_points(lattice.data_ptr(), gx, gy, gz, dx, dy, dz, ap, points.data_ptr(),
                                       int(points.shape[0]), T.data_ptr(), current_stream()), "sift3d_hip_ffd_points")
    return T


def ffd_landmarks_record(record):
    """(counted, S, Omega, rmax) of a landmark record (a CUDA tensor of FFD_LANDMARKS_RECORD_BYTES); waits for the
    stream"""
    return _term_record(record, FFD_LANDMARKS_RECORD_BYTES)


def ffd_landmarks(lattice, spacing, P, Q, w=None, A=None, residuals=True, gradient=True, work=None):
    """sift3d_hip_ffd_landmarks on torch's current stream: lattice a CUDA float32 tensor [3, gz, gy, gx]; P, Q n x 3
    host arrays (fixed and moving voxels, xyz), w n weights or None.  Returns (record: int64 CUDA tensor, read by
    ffd_landmarks_record; r: float64 CUDA tensor [n, 3] or None; GL: float64 CUDA tensor [3, gz, gy, gx] or None)."""
    import torch
    what = "ffd_landmarks"
    gx, gy, gz = _ffd_lattice(lattice, what)
    dx, dy, dz = ffd_spacing(spacing, what)
    P, Q, w = ffd_landmark_arrays(P, Q, w, what)
    m = len(P)
    a, ap = _ffd_A(A, what)
    work = _work(work, (lib().sift3d_amd_ffd_landmarks_work_bytes(m, gx, gy, gz) + 3) // 4, lattice, what)
    record = torch.empty(FFD_LANDMARKS_RECORD_BYTES // 8, dtype=torch.int64, device=lattice.device)
    r = torch.empty((m, 3), dtype=torch.float64, device=lattice.device) if residuals else None
    GL = torch.empty(tuple(lattice.shape), dtype=torch.float64, device=lattice.device) if gradient else None
    _check(lib().sift3d_hip_ffd_landmarks(lattice.data_ptr(), gx, gy, gz, dx, dy, dz, ap, P.ctypes.data, Q.ctypes.data,
                                          None if w is None else w.ctypes.data, m, work.data_ptr(), record.data_ptr(),
                                          None if r is None else r.data_ptr(), None if GL is None else GL.data_ptr(),
                                          current_stream()), "sift3d_hip_ffd_landmarks")
    return record, r, GL


def ffd_evaluate_landmarks(F, M, lattice, spacing, P, Q, w=None, landmark_weight=0.0, A=None, bending=0.0, jacobian=None,
                           mask_fixed=None, mask_moving=None):
    """One evaluation of the FFD cost with the landmark term (sift3d_hip_ffd_evaluate_landmarks) on torch's current
    stream.  jacobian: None evaluates without the Jacobian penalty, a weight >= 0 with it.  Returns (record, grad,
    field, lm, jac): ffd_evaluate's three, then the landmarks' buffer (float64 CUDA tensor: the record in its first
    four words, read by ffd_landmarks_record, then GL [3, gz, gy, gx]) and the penalty's (the same with GJ) or None."""
    import torch
    what = "ffd_evaluate_landmarks"
    _ffd_lattice(lattice, what)
    head, masks = _pair(what, F, M, mask_fixed, mask_moving, lattice)
    P, Q, w = ffd_landmark_arrays(P, Q, w, what)
    args, out, _ = _ffd_evaluate_args(what, head, F, lattice, spacing, A, bending, None)
    sizes = (len(P), *head[1:4], *ffd_spacing(spacing, what))
    size = lib().sift3d_amd_ffd_evaluate_landmarks_bytes
    lm = torch.zeros(size(0, *sizes) // 8 + 1, dtype=torch.float64, device=F.device)
    jac = None if jacobian is None else torch.zeros(size(1, *sizes) // 8 + 1, dtype=torch.float64, device=F.device)
    _run("sift3d_hip_ffd_evaluate_landmarks", *args, *(masks or (None, None)),
         0.0 if jacobian is None else float(jacobian), None if jac is None else jac.data_ptr(),
         *_landmark_args(P, Q, w, landmark_weight), lm.data_ptr())
    return (*out, lm, jac)


def ffd_refine_landmarks(F, M, P, Q, w=None, landmark_weight=0.0, jacobian=None, bins=0, range_f=(0.0, 1.0),
                         range_m=(0.0, 1.0), A=None, params=None, work=None, mask_fixed=None, mask_moving=None):
    """sift3d_amd_ffd_refine_landmarks_device on torch CUDA float32 contiguous volumes, on torch's current stream: the
    FFD drivers with the landmark term of weight `landmark_weight` on the landmarks P, Q (n x 3 host arrays, fixed and
    moving voxels) with weights w (None: all 1).  jacobian: None runs without the Jacobian penalty, a weight >= 0 with
    it; bins == 0: the MSD, else the mutual information as ffd_mi_refine.  Returns (FFDRefineResult, lattice, field,
    Similarity or None, penalty: one (P, rmin, nonpos) per trail entry or None, landmarks: one (L, rmax, counted) per
    trail entry)."""
    what = "ffd_refine_landmarks"
    P, Q, w = ffd_landmark_arrays(P, Q, w, what)
    bins = _parzen_bins(bins, what) if bins else 0
    ranges = _parzen_ranges(range_f, range_m) if bins else (0.0, 1.0, 0.0, 1.0)
    sim, terms = Similarity(), (FFDLandmarkTerm * _FFD_TRAIL)()
    pen = None if jacobian is None else (FFDPenalty * _FFD_TRAIL)()
    tail = (bins, *ranges, C.byref(sim), 0.0 if jacobian is None else float(jacobian), pen,
            *_landmark_args(P, Q, w, landmark_weight), terms)
    res, lattice, field = _ffd_refine_pair(what, "sift3d_amd_ffd_refine_landmarks", F, M, A, params, work, mask_fixed,
                                           mask_moving, tail, count=(len(P),))
    return (res, lattice, field, (sim if bins else None), _trail(pen, res, "P", "rmin", "nonpos"),
            _trail(terms, res, "L", "rmax", "counted"))


# ---- multi-channel free-form deformation ("Multi-channel free-form deformation") ----
def _ffd_stacks(F, M, what, level=""):
    """(nc, fixed grid, moving grid) of a pair of contiguous float32 CUDA stacks [nc, z, y, x] with one nc"""
    for t in (F, M):
        _tensor(t, "%s: %sF and M must be contiguous float32 CUDA tensors [nc, nz, ny, nx]" % (what, level), dims=(4,))
    _same_device(what, F, M)
    if F.shape[0] != M.shape[0] or F.shape[0] < 1:
        raise ValueError("%s: %sF and M must have the same number of channels, at least one" % (what, level))
    return int(F.shape[0]), tuple(F.shape[1:]), tuple(M.shape[1:])


def _ffd_stack_masks(what, F, M, mask_fixed, mask_moving):
    """(d_WF, d_WM) pointers or None of masks on the grids of the stacks F and M"""
    for w, t, name in ((mask_fixed, F, "mask_fixed"), (mask_moving, M, "mask_moving")):
        if w is not None:
            _tensor(w, "%s: %s must be a contiguous float32 CUDA tensor of its stack's grid %s"
                    % (what, name, tuple(t.shape[1:])), shape=tuple(t.shape[1:]), device=t.device)
    return tuple(None if w is None else w.data_ptr() for w in (mask_fixed, mask_moving))


def ffd_evaluate_channels(F, M, lattice, spacing, A=None, bending=0.0, work=None, mask_fixed=None, mask_moving=None):
    """ffd_evaluate for stacks F [nc, oz, oy, ox] and M [nc, nz, ny, nx] (sift3d_hip_ffd_evaluate_channels) on torch's
    current stream.  Returns (record, grad, field, work): the force S is left in `work` (the header gives its offset)."""
    what = "ffd_evaluate_channels"
    nc, (oz, oy, ox), (nz, ny, nx) = _ffd_stacks(F, M, what)
    masks = _ffd_stack_masks(what, F, M, mask_fixed, mask_moving)
    _ffd_lattice(lattice, what)
    _same_device(what, F, lattice)
    head = (F.data_ptr(), ox, oy, oz, M.data_ptr(), nx, ny, nz, nc)
    args, out, work = _ffd_evaluate_args(what, head, F, lattice, spacing, A, bending, work,
                                         "sift3d_amd_ffd_evaluate_channels_work_bytes")
    _run("sift3d_hip_ffd_evaluate_channels", *args, *masks)
    return (*out, work)


def ffd_refine_channels(Fs, Ms, A=None, params=None, work=None, masks_fixed=None, masks_moving=None, jacobian=None):
    """sift3d_amd_ffd_refine_channels_device on torch's current stream: Fs, Ms are the fixed and moving stacks per
    level, level 0 the finest, every level the half ((n + 1) // 2 per axis) of the one above; masks_fixed, masks_moving:
    one mask per level on that level's grid, or None.  jacobian: None runs without the penalty, a weight >= 0 with it.
    Returns (FFDRefineResult, lattice, field, penalty: one (P, rmin, nonpos) per trail entry, or None)."""
    what = "ffd_refine_channels"
    levels = len(Fs)
    if not (1 <= levels <= AFFINE_MAX_LEVELS) or len(Ms) != levels:
        raise ValueError("%s: 1 .. %d levels of fixed and as many of moving stacks" % (what, AFFINE_MAX_LEVELS))
    p = params if params is not None else ffd_refine_params(levels=levels)
    if p.levels != levels:
        raise ValueError("%s: params.levels must be the number of levels given" % what)
    WFs = [None] * levels if masks_fixed is None else list(masks_fixed)
    WMs = [None] * levels if masks_moving is None else list(masks_moving)
    if len(WFs) != levels or len(WMs) != levels:
        raise ValueError("%s: one mask (or None) per level" % what)
    tab = (FFDLevel * levels)()
    nc0 = None
    for l, (F, M) in enumerate(zip(Fs, Ms)):
        nc, fg, mg = _ffd_stacks(F, M, what, "level %d " % l)
        if F.device != Fs[0].device or nc0 not in (None, nc):
            raise ValueError("%s: level %d differs in channels or device" % (what, l))
        nc0 = nc
        if l and (fg != half_shape(Fs[l - 1].shape[1:]) or mg != half_shape(Ms[l - 1].shape[1:])):
            raise ValueError("%s: level %d is not the half of level %d" % (what, l, l - 1))
        wf, wm = _ffd_stack_masks(what, F, M, WFs[l], WMs[l])
        tab[l] = FFDLevel(F.data_ptr(), fg[2], fg[1], fg[0], M.data_ptr(), mg[2], mg[1], mg[0], wf, wm)
    a, ap = _ffd_A(A, what)
    oz, oy, ox = Fs[0].shape[1:]
    need = lib().sift3d_amd_ffd_refine_channels_work_bytes(ox, oy, oz, *p.spacing)
    pen = None if jacobian is None else (FFDPenalty * _FFD_TRAIL)()
    res, lattice, field = _ffd_refine(what, "sift3d_amd_ffd_refine_channels", (tab, levels, nc0), Fs[0], (oz, oy, ox),
                                      ap, p, work, need, "the spacing must be in [1, %d]" % FFD_MAX_SPACING,
                                      (0.0 if jacobian is None else float(jacobian), pen))
    return res, lattice, field, _trail(pen, res, "P", "rmin", "nonpos")


def _dense_args(src, out, what):
    for t, dim in ((src, 3), (out, 4)):
        _tensor(t, "%s: src must be a contiguous float32 CUDA tensor [nz, ny, nx] and out one of [12, nz, ny, nx]"
                % what, dims=(dim,))
    if out.shape != (12,) + tuple(src.shape):
        raise ValueError("%s: out has shape %s, not [12, %d, %d, %d]" % ((what, tuple(out.shape)) + tuple(src.shape)))
    if src.device != out.device:
        raise ValueError("%s: src and out are on different devices" % what)
    nz, ny, nx = src.shape
    return nx, ny, nz


def dense_bin(src, out, units=(1, 1, 1)):
    """Steps 1-2 of the dense descriptor contract (sift3d_hip_dense_bin): per-voxel gradient histograms
    of src [nz, ny, nx] into out [12, nz, ny, nx] (torch CUDA float32), on torch's current stream."""
    nx, ny, nz = _dense_args(src, out, "dense_bin")
    _check(lib().sift3d_hip_dense_bin(src.data_ptr(), nx, ny, nz, *map(float, units), out.data_ptr(),
                                      current_stream()), "sift3d_hip_dense_bin")
    return out


def dense_normalize(hist):
    """Step 4 of the dense descriptor contract (sift3d_hip_dense_normalize), in place on a torch CUDA
    float32 tensor [12, ...] on torch's current stream."""
    _tensor(hist, "dense_normalize: hist must be a contiguous float32 CUDA tensor [12, ...]", lead=12)
    _check(lib().sift3d_hip_dense_normalize(hist.data_ptr(), hist.numel() // 12, current_stream()),
           "sift3d_hip_dense_normalize")
    return hist


def dense_descriptors(src, out, sigma, units=(1, 1, 1), work=None):
    """Dense descriptor image (sift3d_amd_dense_descriptors_device): out [12, nz, ny, nx] from src
    [nz, ny, nx], torch CUDA float32, on torch's current stream.  work: a float32 CUDA tensor of at least
    sift3d_amd_dense_work_floats elements (2 * nz*ny*nx), or None to allocate one here."""
    nx, ny, nz = _dense_args(src, out, "dense_descriptors")
    work = _work(work, lib().sift3d_amd_dense_work_floats(nx, ny, nz), src, "dense_descriptors", "float32")
    u = (C.c_double * 3)(*map(float, units))
    _check(lib().sift3d_amd_dense_descriptors_device(src.data_ptr(), nx, ny, nz, u, float(sigma), out.data_ptr(),
                                                     work.data_ptr(), current_stream()),
           "sift3d_amd_dense_descriptors_device")
    return out


def _dense_r(src, R):
    _tensor(R, "R must be a contiguous float32 CUDA tensor [3, 3, nz, ny, nx] on the device of src",
            shape=(3, 3) + tuple(src.shape), device=src.device)


def dense_orient(src, R, keep=None, sigma=1.6, units=(1, 1, 1)):
    """R2 of the rotating dense contract (sift3d_hip_dense_orient): every voxel's eigen-orientation R
    [3, 3, nz, ny, nx] float32 and keep [nz, ny, nx] uint8 (or None) from src [nz, ny, nx], torch CUDA
    tensors, on torch's current stream."""
    _tensor(src, "dense_orient: src must be a contiguous float32 CUDA tensor [nz, ny, nx]", dims=(3,))
    _dense_r(src, R)
    if keep is not None:
        _tensor(keep, "dense_orient: keep must be a contiguous uint8 CUDA tensor shaped like src, or None",
                shape=src.shape, device=src.device, dtype="uint8")
    nz, ny, nx = src.shape
    _check(lib().sift3d_hip_dense_orient(src.data_ptr(), nx, ny, nz, *map(float, units), float(sigma), R.data_ptr(),
                                         None if keep is None else keep.data_ptr(), current_stream()),
           "sift3d_hip_dense_orient")
    return R, keep


def dense_rotate_bin(src, R, out, sigma=1.6, units=(1, 1, 1)):
    """R3 of the rotating dense contract (sift3d_hip_dense_rotate_bin): unnormalised histograms out
    [12, nz, ny, nx] of src's window gradients rotated by R^T, on torch's current stream."""
    nx, ny, nz = _dense_args(src, out, "dense_rotate_bin")
    _dense_r(src, R)
    _check(lib().sift3d_hip_dense_rotate_bin(src.data_ptr(), nx, ny, nz, *map(float, units), float(sigma),
                                             R.data_ptr(), out.data_ptr(), current_stream()),
           "sift3d_hip_dense_rotate_bin")
    return out


def dense_descriptors_rotate(src, out, sigma, units=(1, 1, 1), work=None):
    """Rotation-invariant dense descriptor image (sift3d_amd_dense_descriptors_rotate_device): out
    [12, nz, ny, nx] from src [nz, ny, nx], torch CUDA float32, on torch's current stream.  work: a float32
    CUDA tensor of at least sift3d_amd_dense_rotate_work_floats elements (9 * nz*ny*nx), or None to
    allocate one here."""
    nx, ny, nz = _dense_args(src, out, "dense_descriptors_rotate")
    work = _work(work, lib().sift3d_amd_dense_rotate_work_floats(nx, ny, nz), src, "dense_descriptors_rotate",
                 "float32")
    u = (C.c_double * 3)(*map(float, units))
    _check(lib().sift3d_amd_dense_descriptors_rotate_device(src.data_ptr(), nx, ny, nz, u, float(sigma),
                                                            out.data_ptr(), work.data_ptr(), current_stream()),
           "sift3d_amd_dense_descriptors_rotate_device")
    return out


DEMONS_STATS_BYTES = 16
DEMONS_FORCE_WORK_BYTES = 32768


def _demons_pair(F, M, what, level=""):
    """The checks of one demons level's features: F, M [nz, ny, nx] or [nc, nz, ny, nx] with the same channels, on
    one device.  Returns nc and the two grids (x, y, z)."""
    for t, name in ((F, "fixed"), (M, "moving")):
        _tensor(t, "%s: %s%s must be a contiguous float32 CUDA tensor [nz, ny, nx] or [nc, nz, ny, nx]"
                % (what, level, name), dims=(3, 4))
    nc = F.shape[0] if F.dim() == 4 else 1
    if M.dim() != F.dim() or (M.shape[0] if M.dim() == 4 else 1) != nc:
        raise ValueError("%s: %sfixed %s and moving %s differ in channels"
                         % (what, level, tuple(F.shape), tuple(M.shape)))
    if F.device != M.device:
        raise ValueError("%s: %sfixed and moving are not on one device" % (what, level))
    nz, ny, nx = F.shape[-3:]
    mz, my, mx = M.shape[-3:]
    return nc, (nx, ny, nz), (mx, my, mz)


def _demons_images(F, M, field, what, level=""):
    """_demons_pair, and the field [3, nz, ny, nx] on F's grid and device"""
    out = _demons_pair(F, M, what, level)
    _field_tensor(field, what)
    if tuple(field.shape[1:]) != tuple(F.shape[-3:]):
        raise ValueError("%s: the field %s is not on the fixed grid %s"
                         % (what, tuple(field.shape), tuple(F.shape)))
    if field.device != F.device:
        raise ValueError("%s: fixed, moving and field are not on one device" % what)
    return out


def demons_stats(stats):
    """(sum float64 array, count uint64 array) of demons statistics (a CUDA tensor of 16-byte records); waits
    for the stream that wrote them"""
    import torch
    raw = stats.view(torch.uint8).cpu().numpy().reshape(-1, DEMONS_STATS_BYTES)
    return raw[:, :8].copy().view(np.float64)[:, 0], raw[:, 8:].copy().view(np.uint64)[:, 0]


class _Grid:
    """A stand-in for a volume in _masks: the grid (nz, ny, nx) a demons mask lies on (one plane whatever nc)"""
    def __init__(self, shape):
        self.shape = tuple(int(v) for v in shape)


def _demons_masks(what, F, moving_grid, mask_fixed, mask_moving):
    """_masks for demons features: the masks are [nz, ny, nx] on F's grid and [mz, my, mx] = moving_grid"""
    return _masks(what, F if F.dim() == 3 else F[0], _Grid(moving_grid), mask_fixed, mask_moving)


def demons_force(F, W, field, step, alpha, moving_shape=None, stats=None, work=None, mask_fixed=None,
                 mask_moving=None):
    """One demons force (sift3d_hip_demons_force; contract in include/sift3d_amd.h, "Dense demons refinement"):
    step [3, nz, ny, nx] from the fixed features F and the warped moving features W ([nz, ny, nx] or
    [nc, nz, ny, nx]) and the field [3, nz, ny, nx]; moving_shape (mz, my, mx) is the moving grid of the inside
    test (None: the fixed grid).  torch CUDA float32, on torch's current stream.  Returns the stats tensor
    (16 bytes; read it with demons_stats).  mask_fixed [nz, ny, nx], mask_moving [mz, my, mx]: float32 masks (in where
    >= 0.5; header, "Masks in demons"); with either given the call goes to sift3d_hip_demons_force_masked, with both
    None to the unmasked entry."""
    import torch
    nc, (nx, ny, nz), _ = _demons_images(F, W, field, "demons_force")
    if tuple(W.shape[-3:]) != tuple(F.shape[-3:]):
        raise ValueError("demons_force: W %s is not on the fixed grid %s" % (tuple(W.shape), tuple(F.shape)))
    _field_tensor(step, "demons_force", "step")
    if tuple(step.shape) != tuple(field.shape) or step.device != F.device:
        raise ValueError("demons_force: step must be shaped like the field, on its device")
    mz, my, mx = (nz, ny, nx) if moving_shape is None else tuple(int(v) for v in moving_shape)
    if stats is None:
        stats = torch.empty(DEMONS_STATS_BYTES // 8, dtype=torch.int64, device=F.device)
    if work is None:
        work = torch.empty(DEMONS_FORCE_WORK_BYTES // 8, dtype=torch.int64, device=F.device)
    masks = _demons_masks("demons_force", F, (mz, my, mx), mask_fixed, mask_moving)
    args = (F.data_ptr(), nx, ny, nz, W.data_ptr(), field.data_ptr(), mx, my, mz, nc, float(alpha), step.data_ptr(),
            stats.data_ptr(), work.data_ptr(), current_stream())
    if masks is not None:
        _check(lib().sift3d_hip_demons_force_masked(*args, *masks), "sift3d_hip_demons_force_masked")
    else:
        _check(lib().sift3d_hip_demons_force(*args), "sift3d_hip_demons_force")
    return stats


DEMONS_UPDATE = {"additive": 0, "diffeomorphic": 1}


def _demons_update(update, what):
    if update not in DEMONS_UPDATE:
        raise ValueError("%s: update must be 'additive' or 'diffeomorphic', not %r" % (what, update))
    return DEMONS_UPDATE[update]


def demons(F, M, field, iterations, alpha, sigma_fluid=0.0, sigma_diffusion=0.0, work=None, update="additive",
           squarings=0, mask_fixed=None, mask_moving=None):
    """`iterations` demons iterations (sift3d_amd_demons_device_ex): the field [3, nz, ny, nx] is refined in
    place so that the moving features M ([mz, my, mx] or [nc, mz, my, mx]) warped through it approach the fixed
    features F ([nz, ny, nx] / [nc, nz, ny, nx]).  update "additive": u += delta (`squarings` is not used);
    "diffeomorphic": u <- u o exp(delta) with `squarings` squarings.  torch CUDA float32, on torch's current
    stream, no host synchronisation.  Returns the stats tensor (16 bytes per iteration; read it with
    demons_stats).  mask_fixed, mask_moving: as demons_force's, on F's and M's grids (with either given:
    sift3d_amd_demons_masked_device with one level)."""
    import torch
    if mask_fixed is not None or mask_moving is not None:
        return _demons_pyramid("demons", [F], [M], field, [iterations], alpha, sigma_fluid, sigma_diffusion, work,
                               update, int(squarings) if update == "diffeomorphic" else 0, [mask_fixed], [mask_moving])
    nc, (nx, ny, nz), (mx, my, mz) = _demons_images(F, M, field, "demons")
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError("demons: iterations must not be negative")
    mode = _demons_update(update, "demons")
    work = _work(work, lib().sift3d_amd_demons_work_floats_ex(nx, ny, nz, nc, mode), F, "demons")
    stats = torch.empty(max(iterations, 1) * DEMONS_STATS_BYTES // 8, dtype=torch.int64, device=F.device)
    _check(lib().sift3d_amd_demons_device_ex(F.data_ptr(), nx, ny, nz, M.data_ptr(), mx, my, mz, nc,
                                             field.data_ptr(), iterations, float(alpha), float(sigma_fluid),
                                             float(sigma_diffusion), mode, int(squarings) if mode else 0,
                                             work.data_ptr(), stats.data_ptr(), current_stream()),
           "sift3d_amd_demons_device_ex")
    return stats[:iterations * DEMONS_STATS_BYTES // 8]


FIELD_STATS_BYTES = 32
FIELD_WORK_BYTES = 65536
FIELD_MAX_SQUARINGS = 20
FIELD_MODE = {"compose": 0, "invert": 1}


def field_stats(stats):
    """(sum, max float64 arrays, count, inside uint64 arrays) of field composition statistics (a CUDA tensor of
    32-byte records); waits for the stream that wrote them"""
    import torch
    raw = stats.view(torch.uint8).cpu().numpy().reshape(-1, FIELD_STATS_BYTES)
    f = raw[:, :16].copy().view(np.float64)
    c = raw[:, 16:].copy().view(np.uint64)
    return f[:, 0], f[:, 1], c[:, 0], c[:, 1]


def field_compose(u, v, out=None, mode="compose", stats=None, work=None):
    """One composition sample pass (sift3d_hip_field_compose; contract in include/sift3d_amd.h, "Field
    composition, exponential and inverse"): u [3, uz, uy, ux], v and out [3, oz, oy, ox] torch CUDA float32 on
    torch's current stream.  mode "compose": out = v + u(p + v) (u extended by its edge values outside its grid);
    "invert": out = -u(p + v).  out None: statistics only.  stats: a CUDA tensor of >= 32 bytes for the residual
    statistics, True to allocate one, or None for none.  Returns the stats tensor (read it with field_stats) or
    None."""
    import torch
    _field_tensor(u, "field_compose", "u")
    _field_tensor(v, "field_compose", "v")
    if mode not in FIELD_MODE:
        raise ValueError("field_compose: mode must be 'compose' or 'invert', not %r" % (mode,))
    if out is not None:
        _field_tensor(out, "field_compose", "out")
        if out.shape != v.shape:
            raise ValueError("field_compose: out %s is not shaped like v %s" % (tuple(out.shape), tuple(v.shape)))
        _same_device("field_compose", u, v, out)
    _same_device("field_compose", u, v)
    if stats is True:
        stats = torch.empty(FIELD_STATS_BYTES // 8, dtype=torch.int64, device=v.device)
    if stats is not None and work is None:
        work = torch.empty(FIELD_WORK_BYTES // 8, dtype=torch.int64, device=v.device)
    if stats is None and out is None:
        raise ValueError("field_compose: neither out nor stats")
    _, uz, uy, ux = u.shape
    _, oz, oy, ox = v.shape
    _check(lib().sift3d_hip_field_compose(u.data_ptr(), ux, uy, uz, v.data_ptr(), ox, oy, oz,
                                          None if out is None else out.data_ptr(), FIELD_MODE[mode],
                                          None if stats is None else stats.data_ptr(),
                                          None if work is None else work.data_ptr(), current_stream()),
           "sift3d_hip_field_compose")
    return stats


def field_exp(v, out, squarings, work=None, negate=False):
    """out = exp(v) by scaling and squaring (sift3d_amd_field_exp_device), or exp(-v) with negate
    (sift3d_amd_field_exp_signed_device: the scaling's factor is -2^-K): v, out [3, oz, oy, ox] torch CUDA float32,
    on torch's current stream."""
    _field_tensor(v, "field_exp", "v")
    _field_tensor(out, "field_exp", "out")
    if out.shape != v.shape:
        raise ValueError("field_exp: out %s is not shaped like v %s" % (tuple(out.shape), tuple(v.shape)))
    _same_device("field_exp", v, out)
    _, oz, oy, ox = v.shape
    work = _work(work, lib().sift3d_amd_field_exp_work_floats(ox, oy, oz), v, "field_exp")
    if negate:
        _check(lib().sift3d_amd_field_exp_signed_device(v.data_ptr(), ox, oy, oz, int(squarings), 1, out.data_ptr(),
                                                        work.data_ptr(), current_stream()),
               "sift3d_amd_field_exp_signed_device")
        return out
    _check(lib().sift3d_amd_field_exp_device(v.data_ptr(), ox, oy, oz, int(squarings), out.data_ptr(),
                                             work.data_ptr(), current_stream()), "sift3d_amd_field_exp_device")
    return out


FIELD_BRACKET_MODE = {"bracket": 0, "bch1": 1}


def field_bracket(a, b, out=None, mode="bracket"):
    """The Lie bracket [a, b] = J_a b - J_b a (mode "bracket") or the first-order BCH update a + b + [a, b] / 2
    (mode "bch1") of two fields (sift3d_hip_field_bracket; contract in include/sift3d_amd.h, "Log-domain demons"):
    a, b, out [3, oz, oy, ox] torch CUDA float32 on one grid (out None: allocated), on torch's current stream.  a may
    be b; out must be neither."""
    import torch
    _field_tensor(a, "field_bracket", "a")
    _field_tensor(b, "field_bracket", "b")
    if mode not in FIELD_BRACKET_MODE:
        raise ValueError("field_bracket: mode must be 'bracket' or 'bch1', not %r" % (mode,))
    if b.shape != a.shape:
        raise ValueError("field_bracket: b %s is not shaped like a %s" % (tuple(b.shape), tuple(a.shape)))
    if out is None:
        out = torch.empty_like(a)
    _field_tensor(out, "field_bracket", "out")
    if out.shape != a.shape:
        raise ValueError("field_bracket: out %s is not shaped like a %s" % (tuple(out.shape), tuple(a.shape)))
    _same_device("field_bracket", a, b, out)
    _, oz, oy, ox = a.shape
    _check(lib().sift3d_hip_field_bracket(a.data_ptr(), b.data_ptr(), ox, oy, oz, out.data_ptr(),
                                          FIELD_BRACKET_MODE[mode], current_stream()), "sift3d_hip_field_bracket")
    return out


def field_invert(u, w, iterations, work=None):
    """`iterations` fixed-point steps w <- -u(p + w) (sift3d_amd_field_invert_device): u [3, uz, uy, ux], w
    [3, oz, oy, ox] (the initial iterate in, the result out) torch CUDA float32, on torch's current stream.  Returns
    the stats tensor: iterations + 1 records of 32 bytes (read them with field_stats)."""
    import torch
    _field_tensor(u, "field_invert", "u")
    _field_tensor(w, "field_invert", "w")
    _same_device("field_invert", u, w)
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError("field_invert: iterations must not be negative")
    _, uz, uy, ux = u.shape
    _, oz, oy, ox = w.shape
    work = _work(work, lib().sift3d_amd_field_invert_work_floats(ox, oy, oz), w, "field_invert")
    stats = torch.empty((iterations + 1) * FIELD_STATS_BYTES // 8, dtype=torch.int64, device=w.device)
    _check(lib().sift3d_amd_field_invert_device(u.data_ptr(), ux, uy, uz, w.data_ptr(), ox, oy, oz, iterations,
                                                work.data_ptr(), stats.data_ptr(), current_stream()),
           "sift3d_amd_field_invert_device")
    return stats


DEMONS_MAX_LEVELS = 6


def half_shape(shape):
    """the grid under (nz, ny, nx) in the pyramid: (n + 1) // 2 per axis"""
    return tuple((int(n) + 1) // 2 for n in shape)


def restrict2(src, dst=None, scale=1.0):
    """dst = src halved on every axis by the separable binomial (1/4, 1/2, 1/4), times `scale`
    (sift3d_hip_restrict2; contract in include/sift3d_amd.h, "Multi-resolution demons"): src [nz, ny, nx] or
    [nc, nz, ny, nx], dst the same with every grid axis (n + 1) // 2 (None: allocated), torch CUDA float32
    contiguous, on torch's current stream.  scale 0.5 restricts a displacement field."""
    import torch
    _tensor(src, "restrict2: src must be a contiguous float32 CUDA tensor [nz, ny, nx] or [nc, nz, ny, nx]",
            dims=(3, 4))
    want = tuple(src.shape[:-3]) + half_shape(src.shape[-3:])
    if dst is None:
        dst = torch.empty(want, dtype=torch.float32, device=src.device)
    _tensor(dst, "restrict2: dst must be a contiguous float32 CUDA tensor %s on the device of src" % (want,),
            shape=want, device=src.device)
    nc = src.shape[0] if src.dim() == 4 else 1
    nz, ny, nx = src.shape[-3:]
    _check(lib().sift3d_hip_restrict2(src.data_ptr(), nx, ny, nz, nc, dst.data_ptr(), float(scale),
                                      current_stream()), "sift3d_hip_restrict2")
    return dst


def field_prolong2(coarse, fine):
    """fine = the field `coarse` carried to the grid twice as fine: 2 x its linear interpolation at p / 2
    (sift3d_hip_field_prolong2; contract in include/sift3d_amd.h, "Multi-resolution demons"): coarse
    [3, cz, cy, cx], fine [3, nz, ny, nx] with c = (n + 1) // 2 on every axis, torch CUDA float32, on torch's
    current stream."""
    _field_tensor(coarse, "field_prolong2", "coarse")
    _field_tensor(fine, "field_prolong2", "fine")
    _same_device("field_prolong2", coarse, fine)
    if tuple(coarse.shape[1:]) != half_shape(fine.shape[1:]):
        raise ValueError("field_prolong2: coarse %s is not the grid under fine %s"
                         % (tuple(coarse.shape), tuple(fine.shape)))
    _, nz, ny, nx = fine.shape
    _check(lib().sift3d_hip_field_prolong2(coarse.data_ptr(), fine.data_ptr(), nx, ny, nz, current_stream()),
           "sift3d_hip_field_prolong2")
    return fine


def _demons_levels(what, Fs, Ms, field, iterations):
    """The level table of a pyramid driver and its checks: (table, levels, nc, iterations per level)"""
    levels = len(Fs)
    if not (1 <= levels <= DEMONS_MAX_LEVELS) or len(Ms) != levels:
        raise ValueError("%s: 1 .. %d levels of fixed and as many of moving features" % (what, DEMONS_MAX_LEVELS))
    its = [int(k) for k in iterations]
    if len(its) != levels or any(k < 0 for k in its):
        raise ValueError("%s: iterations must hold one count >= 0 per level" % what)
    _field_tensor(field, what)
    tab = (DemonsLevel * levels)()
    nc0 = None
    for l, (F, M) in enumerate(zip(Fs, Ms)):
        # a level's checks are those of demons; only level 0 has its field here (the others' are in the work buffer)
        level = "level %d " % l
        nc, (nx, ny, nz), (mx, my, mz) = (_demons_pair(F, M, what, level) if l else
                                          _demons_images(F, M, field, what, level))
        if F.device != field.device or nc0 not in (None, nc):
            raise ValueError("%s: level %d differs in channels or is not on the field's device" % (what, l))
        nc0 = nc
        if l and ((nz, ny, nx) != half_shape(Fs[l - 1].shape[-3:]) or (mz, my, mx) != half_shape(Ms[l - 1].shape[-3:])):
            raise ValueError("%s: level %d is not the half of level %d" % (what, l, l - 1))
        tab[l] = DemonsLevel(F.data_ptr(), nx, ny, nz, M.data_ptr(), mx, my, mz, its[l])
    return tab, levels, nc0, its


def _demons_mask_lists(what, levels, masks_fixed, masks_moving):
    """masks_fixed, masks_moving (None, or one mask or None per level) as two lists of `levels` entries; checked ahead
    of the tensors, as it depends on the arguments alone"""
    WFs = [None] * levels if masks_fixed is None else list(masks_fixed)
    WMs = [None] * levels if masks_moving is None else list(masks_moving)
    if len(WFs) != levels or len(WMs) != levels:
        raise ValueError("%s: masks_fixed and masks_moving must hold one mask (or None) per level" % what)
    return WFs, WMs


def _demons_level_masks(what, Fs, Ms, WFs, WMs):
    """The mask table of a masked pyramid driver, or None when every mask is None (the unmasked entry is called): one
    mask (or None) per level on that level's fixed / moving grid"""
    levels = len(Fs)
    if all(w is None for w in WFs + WMs):
        return None
    tab = (DemonsLevelMasks * levels)()
    for l, (F, M) in enumerate(zip(Fs, Ms)):
        wf, wm = _demons_masks("%s: level %d" % (what, l), F, M.shape[-3:], WFs[l], WMs[l]) or (None, None)
        tab[l] = DemonsLevelMasks(wf, wm)
    return tab


def demons_multires(Fs, Ms, field, iterations, alpha, sigma_fluid=0.0, sigma_diffusion=0.0, work=None,
                    update="additive", squarings=0, masks_fixed=None, masks_moving=None):
    """Coarse-to-fine demons (sift3d_amd_demons_multires_device; contract in include/sift3d_amd.h,
    "Multi-resolution demons"): Fs, Ms are the fixed and moving feature stacks per level, level 0 the finest, every
    level the half ((n + 1) // 2 per axis) of the one above; iterations one count per level; the field
    [3, nz, ny, nx] on Fs[0]'s grid is restricted to the coarsest level, refined there and handed up, in place.
    torch CUDA float32, on torch's current stream, no host synchronisation.  Returns the stats tensor: 16 bytes per
    iteration in the order run, the coarsest level's first (read it with demons_stats).  masks_fixed, masks_moving:
    None, or one float32 mask (or None) per level on that level's fixed / moving grid (header, "Masks in demons"); with
    any mask given the call goes to sift3d_amd_demons_masked_device, with none to the unmasked entry."""
    return _demons_pyramid("demons_multires", Fs, Ms, field, iterations, alpha, sigma_fluid, sigma_diffusion, work,
                           update, squarings, masks_fixed, masks_moving)


def _demons_pyramid(what, Fs, Ms, field, iterations, alpha, sigma_fluid, sigma_diffusion, work, update, squarings,
                    masks_fixed, masks_moving):
    """demons_multires, and demons with a mask (one level), under the caller's name in the messages"""
    import torch
    mode = _demons_update(update, what)
    WFs, WMs = _demons_mask_lists(what, len(Fs), masks_fixed, masks_moving)
    tab, levels, nc0, its = _demons_levels(what, Fs, Ms, field, iterations)
    wtab = _demons_level_masks(what, Fs, Ms, WFs, WMs)
    _, nz, ny, nx = field.shape
    work = _work(work, lib().sift3d_amd_demons_multires_work_floats(nx, ny, nz, nc0, mode, levels), field, what)
    total = sum(its)
    stats = torch.empty(max(total, 1) * DEMONS_STATS_BYTES // 8, dtype=torch.int64, device=field.device)
    tail = (levels, nc0, field.data_ptr(), float(alpha), float(sigma_fluid), float(sigma_diffusion), mode,
            int(squarings), work.data_ptr(), stats.data_ptr(), current_stream())
    if wtab is not None:
        _check(lib().sift3d_amd_demons_masked_device(tab, wtab, *tail), "sift3d_amd_demons_masked_device")
    else:
        _check(lib().sift3d_amd_demons_multires_device(tab, *tail), "sift3d_amd_demons_multires_device")
    return stats[:total * DEMONS_STATS_BYTES // 8]


def logdemons(Fs, Ms, velocity, iterations, alpha, sigma_fluid=0.0, sigma_diffusion=0.0, symmetric=False, bch=1,
              velocity_squarings=0, work=None, masks_fixed=None, masks_moving=None):
    """Log-domain demons (sift3d_amd_logdemons_device; contract in include/sift3d_amd.h, "Log-domain demons"): the
    stationary velocity [3, nz, ny, nx] on Fs[0]'s grid is refined in place so that the moving features read through
    exp(velocity) approach the fixed ones.  Fs, Ms, iterations: the levels as in demons_multires (one level: a flat
    run).  symmetric: forces from both directions (fixed and moving shapes must agree); bch 0: v += delta, 1: the
    BCH update with the first Lie bracket; velocity_squarings: the squarings of every exponential.  torch CUDA
    float32, on torch's current stream, no host synchronisation.  Returns the stats tensor: 16 bytes per iteration
    in the order run (read it with demons_stats).  masks_fixed, masks_moving: as demons_multires's
    (sift3d_amd_logdemons_masked_device; the backward force of the symmetric update exchanges them)."""
    import torch
    what = "logdemons"
    if bch not in (0, 1):
        raise ValueError("logdemons: bch must be 0 or 1, not %r" % (bch,))
    WFs, WMs = _demons_mask_lists(what, len(Fs), masks_fixed, masks_moving)
    tab, levels, nc0, its = _demons_levels(what, Fs, Ms, velocity, iterations)
    sym = 1 if symmetric else 0
    if sym and any(tuple(F.shape) != tuple(M.shape) for F, M in zip(Fs, Ms)):
        raise ValueError("logdemons: the symmetric update needs fixed and moving volumes of one shape")
    _, nz, ny, nx = velocity.shape
    work = _work(work, lib().sift3d_amd_logdemons_work_floats(nx, ny, nz, nc0, sym, levels), velocity, what)
    total = sum(its)
    stats = torch.empty(max(total, 1) * DEMONS_STATS_BYTES // 8, dtype=torch.int64, device=velocity.device)
    wtab = _demons_level_masks(what, Fs, Ms, WFs, WMs)
    tail = (levels, nc0, velocity.data_ptr(), float(alpha), float(sigma_fluid), float(sigma_diffusion), sym, int(bch),
            int(velocity_squarings), work.data_ptr(), stats.data_ptr(), current_stream())
    if wtab is not None:
        _check(lib().sift3d_amd_logdemons_masked_device(tab, wtab, *tail), "sift3d_amd_logdemons_masked_device")
    else:
        _check(lib().sift3d_amd_logdemons_device(tab, *tail), "sift3d_amd_logdemons_device")
    return stats[:total * DEMONS_STATS_BYTES // 8]


LNCC_MAX_RADIUS = 4
FIELD_NORMALIZE_WORK_BYTES = 16400


def _lncc_radius(radius, what):
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= radius <= LNCC_MAX_RADIUS:
        raise ValueError("%s: radius must be an integer in 1 .. %d, not %r" % (what, LNCC_MAX_RADIUS, radius))
    return int(radius)


def _lncc_step(step, what):
    if isinstance(step, bool) or not isinstance(step, (int, float, np.integer, np.floating)) or \
            not (math.isfinite(step) and step > 0):
        raise ValueError("%s: step must be positive and finite, not %r" % (what, step))
    return float(step)


def _lncc_pass(what, F, W, field, moving_shape, radius, mask_fixed, mask_moving, work):
    """The checks the two windowed passes share: F, W [nz, ny, nx] and the field [3, nz, ny, nx] on one grid and
    device, the masks as demons_force's.  Returns (the entry's arguments up to the radius, work)."""
    for t, name in ((F, "F"), (W, "W")):
        _tensor(t, "%s: %s must be a contiguous float32 CUDA tensor [nz, ny, nx]" % (what, name), dims=(3,))
    _demons_images(F, W, field, what)
    if tuple(W.shape) != tuple(F.shape):
        raise ValueError("%s: W %s is not on the fixed grid %s" % (what, tuple(W.shape), tuple(F.shape)))
    r = _lncc_radius(radius, what)
    nz, ny, nx = F.shape
    mz, my, mx = (nz, ny, nx) if moving_shape is None else tuple(int(v) for v in moving_shape)
    masks = _demons_masks(what, F, (mz, my, mx), mask_fixed, mask_moving) or (None, None)
    work = _byte_work(what, work, lib().sift3d_amd_lncc_work_bytes(nx, ny, nz), F)
    return (F.data_ptr(), nx, ny, nz, W.data_ptr(), field.data_ptr(), mx, my, mz) + tuple(masks) + (r,), work


def lncc(F, W, field, radius=2, moving_shape=None, cc=None, coef=None, stats=None, work=None, mask_fixed=None,
         mask_moving=None):
    """The statistics pass of local cross-correlation (sift3d_hip_lncc; contract in include/sift3d_amd.h, "Local
    cross-correlation"): the fixed volume F and the warped moving volume W [nz, ny, nx], the field [3, nz, ny, nx] that
    made W, moving_shape (mz, my, mx) the moving grid of the validity test (None: the fixed grid).  cc: a float32
    tensor [nz, ny, nx] that receives the map, or None; coef: a float64 tensor [4, nz, ny, nx] that receives the
    coefficient volumes, or None.  mask_fixed, mask_moving: as demons_force's.  torch CUDA, on torch's current stream.
    Returns the stats tensor (16 bytes: the sum of cc over the counted voxels and their count; demons_stats)."""
    import torch
    head, work = _lncc_pass("lncc", F, W, field, moving_shape, radius, mask_fixed, mask_moving, work)
    if cc is not None:
        _tensor(cc, "lncc: cc must be a contiguous float32 CUDA tensor of F's shape on its device",
                shape=tuple(F.shape), device=F.device)
    if coef is not None:
        _tensor(coef, "lncc: coef must be a contiguous float64 CUDA tensor [4, nz, ny, nx] on F's device",
                shape=(4,) + tuple(F.shape), device=F.device, dtype="float64")
    if stats is None:
        stats = torch.empty(DEMONS_STATS_BYTES // 8, dtype=torch.int64, device=F.device)
    _run("sift3d_hip_lncc", *head, None if cc is None else cc.data_ptr(), None if coef is None else coef.data_ptr(),
         stats.data_ptr(), work.data_ptr(), current_stream())
    return stats


def lncc_force(F, W, field, coef, force, radius=2, moving_shape=None, work=None, mask_fixed=None, mask_moving=None):
    """The force of local cross-correlation (sift3d_hip_lncc_force): force [3, nz, ny, nx] float32 from the coefficient
    volumes coef (float64 [4, nz, ny, nx]) that lncc wrote for the same F, W, field, masks and radius.  Returns force."""
    head, work = _lncc_pass("lncc_force", F, W, field, moving_shape, radius, mask_fixed, mask_moving, work)
    _tensor(coef, "lncc_force: coef must be a contiguous float64 CUDA tensor [4, nz, ny, nx] on F's device",
            shape=(4,) + tuple(F.shape), device=F.device, dtype="float64")
    _field_tensor(force, "lncc_force", "force")
    if tuple(force.shape) != tuple(field.shape) or force.device != F.device:
        raise ValueError("lncc_force: force must be shaped like the field, on its device")
    _run("sift3d_hip_lncc_force", *head, coef.data_ptr(), force.data_ptr(), work.data_ptr(), current_stream())
    return force


def field_normalize(field, step, work=None):
    """The field [3, nz, ny, nx] scaled in place so that its longest vector is `step` voxels
    (sift3d_hip_field_normalize); an all-zero field is left as it is.  No host synchronisation.  Returns field."""
    s = _lncc_step(step, "field_normalize")
    _field_tensor(field, "field_normalize")
    work = _byte_work("field_normalize", work, FIELD_NORMALIZE_WORK_BYTES, field)
    _, nz, ny, nx = field.shape
    _run("sift3d_hip_field_normalize", field.data_ptr(), nx, ny, nz, s, work.data_ptr(), current_stream())
    return field


def demons_lncc(Fs, Ms, field, iterations, radius=2, step=0.5, sigma_fluid=0.0, sigma_diffusion=0.0, work=None,
                update="additive", squarings=0, masks_fixed=None, masks_moving=None):
    """Demons-style ascent of the local cross-correlation (sift3d_amd_demons_lncc_device; contract in
    include/sift3d_amd.h, "Local cross-correlation"): Fs, Ms are the fixed and moving volumes [nz, ny, nx] per level,
    level 0 the finest (one level: a flat run), iterations one count per level; the field [3, nz, ny, nx] on Fs[0]'s
    grid is refined in place.  Every iteration moves the field by at most `step` voxels.  update, squarings,
    masks_fixed, masks_moving: as demons_multires's.  torch CUDA float32, on torch's current stream, no host
    synchronisation.  Returns the stats tensor: 16 bytes per iteration in the order run (demons_stats: the sum of cc
    over the counted voxels and their count, before the iteration's update)."""
    import torch
    what = "demons_lncc"
    mode = _demons_update(update, what)
    r = _lncc_radius(radius, what)
    s = _lncc_step(step, what)
    WFs, WMs = _demons_mask_lists(what, len(Fs), masks_fixed, masks_moving)
    for t in list(Fs) + list(Ms):
        _tensor(t, "%s: every level's volumes must be contiguous float32 CUDA tensors [nz, ny, nx]" % what, dims=(3,))
    tab, levels, _, its = _demons_levels(what, Fs, Ms, field, iterations)
    wtab = _demons_level_masks(what, Fs, Ms, WFs, WMs)
    _, nz, ny, nx = field.shape
    work = _work(work, lib().sift3d_amd_demons_lncc_work_floats(nx, ny, nz, mode, levels), field, what)
    total = sum(its)
    stats = torch.empty(max(total, 1) * DEMONS_STATS_BYTES // 8, dtype=torch.int64, device=field.device)
    _run("sift3d_amd_demons_lncc_device", tab, wtab, levels, r, field.data_ptr(), s, float(sigma_fluid),
         float(sigma_diffusion), mode, int(squarings) if mode else 0, work.data_ptr(), stats.data_ptr(),
         current_stream())
    return stats[:total * DEMONS_STATS_BYTES // 8]


# ---- MIND-SSC self-similarity descriptors (contract: include/sift3d_amd.h, "MIND self-similarity descriptors") -----
MIND_CHANNELS = 12
MIND_MAX_RADIUS = 2
MIND_MAX_DILATION = 4


def _mind_int(value, hi, what, name):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 1 <= value <= hi:
        raise ValueError("%s: %s must be an integer in 1 .. %d, not %r" % (what, name, hi, value))
    return int(value)


def _mind_clamps(vlo, vhi, what):
    for v in (vlo, vhi):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError("%s: vlo and vhi must be numbers, not %r" % (what, v))
    vlo, vhi = float(vlo), float(vhi)
    if not (vlo >= 0 and vhi >= vlo):
        raise ValueError("%s: the clamps must satisfy 0 <= vlo <= vhi, not %r and %r" % (what, vlo, vhi))
    return vlo, vhi


def mind_ssc(src, out=None, radius=1, dilation=2, vlo=0.0, vhi=math.inf, D=None, V=None, stats=None, work=None):
    """The MIND-SSC descriptor of a volume (sift3d_hip_mind_ssc; contract in include/sift3d_amd.h, "MIND
    self-similarity descriptors"): src [nz, ny, nx] float32; out: a float32 tensor [12, nz, ny, nx] that receives the
    descriptor, None: allocated.  radius: the patch radius (1 .. 2), dilation: the neighbours' distance (1 .. 4), vlo,
    vhi: the clamps of the variance.  D: a float64 tensor [12, nz, ny, nx] that receives the distances, or None; V: a
    float64 tensor [nz, ny, nx] that receives the unclamped variance, or None; stats: an int64 tensor of 2 words that
    receives the sum of V and the voxel count (demons_stats), or None.  out=False asks for no descriptor (then one of
    D, V, stats must be given).  torch CUDA, on torch's current stream, no host synchronisation.  Returns out (None
    with out=False)."""
    import torch
    what = "mind_ssc"
    _tensor(src, "%s: src must be a contiguous float32 CUDA tensor [nz, ny, nx]" % what, dims=(3,))
    r = _mind_int(radius, MIND_MAX_RADIUS, what, "radius")
    d = _mind_int(dilation, MIND_MAX_DILATION, what, "dilation")
    vlo, vhi = _mind_clamps(vlo, vhi, what)
    shape = tuple(src.shape)
    nz, ny, nx = shape
    if out is None:
        out = torch.empty((MIND_CHANNELS,) + shape, dtype=torch.float32, device=src.device)
    elif out is False:
        out = None
        if D is None and V is None and stats is None:
            raise ValueError("%s: out=False needs one of D, V and stats" % what)
    else:
        _tensor(out, "%s: out must be a contiguous float32 CUDA tensor [12, nz, ny, nx] on src's device" % what,
                shape=(MIND_CHANNELS,) + shape, device=src.device)
    if D is not None:
        _tensor(D, "%s: D must be a contiguous float64 CUDA tensor [12, nz, ny, nx] on src's device" % what,
                shape=(MIND_CHANNELS,) + shape, device=src.device, dtype="float64")
    if V is not None:
        _tensor(V, "%s: V must be a contiguous float64 CUDA tensor [nz, ny, nx] on src's device" % what,
                shape=shape, device=src.device, dtype="float64")
    if stats is not None:
        _tensor(stats, "%s: stats must be a contiguous int64 CUDA tensor of %d words on src's device"
                % (what, DEMONS_STATS_BYTES // 8), shape=(DEMONS_STATS_BYTES // 8,), device=src.device, dtype="int64")
    work = _byte_work(what, work, lib().sift3d_amd_mind_work_bytes(nx, ny, nz), src)
    _run("sift3d_hip_mind_ssc", src.data_ptr(), nx, ny, nz, r, d, vlo, vhi, *(None if t is None else t.data_ptr()
                                                                                for t in (out, D, V, stats)),
         work.data_ptr(), current_stream())
    return out


# ---- block matching (contract: include/sift3d_amd.h, "Block matching") ----------------------------------------------
BLOCK_MODEL = {"translation": 0, "rigid": 1, "affine": 2}
BLOCK_STOPS = ("converged", "iterations", "failed")


def _block_radius(radius, what):
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= radius <= BLOCK_MAX_RADIUS:
        raise ValueError("%s: radius must be an integer in 1 .. %d, not %r" % (what, BLOCK_MAX_RADIUS, radius))
    return int(radius)


def block_match(F, W, radius=3, valid_fixed=None, valid_warped=None, work=None, stream=None):
    """sift3d_hip_block_match: every 4^3 block of the fixed volume F [nz, ny, nx] finds its best-correlated position in
    W (the moving volume warped onto F's grid) inside the (2 radius + 1)^3 search cube.  valid_fixed, valid_warped:
    float32 masks on the same grid (in where >= 0.5) or None.  work: a CUDA tensor of at least
    sift3d_amd_block_match_work_bytes bytes or None (this build needs none).  stream: a stream handle, or None for
    torch's current stream.  torch CUDA float32 contiguous; no host synchronisation.  Returns (disp float32
    [3, nbz, nby, nbx] (x, y, z), cc float32 [nbz, nby, nbx], var float64 [nbz, nby, nbx]); an invalid block has
    disp 0, cc -1, var 0."""
    import torch
    what = "block_match"
    for t, name in ((F, "F"), (W, "W")):
        _tensor(t, "%s: %s must be a contiguous float32 CUDA tensor [nz, ny, nx]" % (what, name), dims=(3,))
    if tuple(W.shape) != tuple(F.shape) or W.device != F.device:
        raise ValueError("%s: W %s is not on the fixed grid %s and device" % (what, tuple(W.shape), tuple(F.shape)))
    r = _block_radius(radius, what)
    nz, ny, nx = F.shape
    if min(nx, ny, nz) < 4:
        raise ValueError("%s: F %s must hold a block of 4 voxels on every axis" % (what, tuple(F.shape)))
    for w, name in ((valid_fixed, "valid_fixed"), (valid_warped, "valid_warped")):
        if w is not None:
            _tensor(w, "%s: %s must be a contiguous float32 CUDA tensor of F's shape %s on its device"
                    % (what, name, tuple(F.shape)), shape=tuple(F.shape), device=F.device)
    need = lib().sift3d_amd_block_match_work_bytes(nx, ny, nz, r)
    if work is not None or need:
        work = _byte_work(what, work, need, F)
    nb = (nz // 4, ny // 4, nx // 4)
    disp = torch.empty((3,) + nb, dtype=torch.float32, device=F.device)
    cc = torch.empty(nb, dtype=torch.float32, device=F.device)
    var = torch.empty(nb, dtype=torch.float64, device=F.device)
    _run("sift3d_hip_block_match", F.data_ptr(), nx, ny, nz, W.data_ptr(),
         None if valid_fixed is None else valid_fixed.data_ptr(),
         None if valid_warped is None else valid_warped.data_ptr(), r, disp.data_ptr(), cc.data_ptr(), var.data_ptr(),
         work.data_ptr() if work is not None and work.numel() else None,
         current_stream() if stream is None else stream)
    return disp, cc, var


def _scale3(v, what, name):
    if v is None:
        return None
    a = np.ascontiguousarray(v, np.float64)
    if a.shape != (3,) or not (np.isfinite(a).all() and (a > 0).all()):
        raise ValueError("%s: %s must be three positive finite numbers (x, y, z), not %r" % (what, name, v))
    return a.copy()


def fit_trimmed(src, dst, model="rigid", keep=0.5, max_iter=20, scale_src=None, scale_dst=None):
    """sift3d_amd_fit_trimmed (host): the least-trimmed-squares fit of dst ~ T [src; 1] on n x 3 float64 points.
    Returns (T [3, 4], used bool [n], refits), or None where the entry refuses (too few or non-finite points, a
    degenerate set).  ValueError on arguments that no point set could make valid."""
    what = "fit_trimmed"
    if model not in BLOCK_MODEL:
        raise ValueError("%s: model must be 'translation', 'rigid' or 'affine', not %r" % (what, model))
    if isinstance(keep, bool) or not isinstance(keep, (int, float, np.integer, np.floating)) or not 0 < keep <= 1:
        raise ValueError("%s: keep must be in (0, 1], not %r" % (what, keep))
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 0:
        raise ValueError("%s: max_iter must be a non-negative integer, not %r" % (what, max_iter))
    s = np.ascontiguousarray(src, np.float64)
    d = np.ascontiguousarray(dst, np.float64)
    if s.ndim != 2 or s.shape[1] != 3:
        raise ValueError("%s: src must be n x 3 points" % what)
    if d.shape != s.shape:
        raise ValueError("%s: dst must have src's shape %s" % (what, s.shape))
    ss, sd = _scale3(scale_src, what, "scale_src"), _scale3(scale_dst, what, "scale_dst")
    T = np.zeros(12)
    used = np.zeros(max(len(s), 1), np.uint8)
    its = C.c_int(0)
    rc = lib().sift3d_amd_fit_trimmed(_dptr(s), _dptr(d), len(s), BLOCK_MODEL[model], float(keep), int(max_iter),
                                      None if ss is None else _dptr(ss), None if sd is None else _dptr(sd), _dptr(T),
                                      used.ctypes.data, C.byref(its))
    if rc != 0:
        return None
    return T.reshape(3, 4), used[:len(s)].astype(bool), int(its.value)


def block_register_params(**kw):
    """sift3d_amd_block_register_params: the defaults, overridden by model (a name), levels, iterations, radius,
    keep_blocks, keep_inliers, tol, spacing_fixed, spacing_moving"""
    p = BlockRegisterParams()
    lib().sift3d_amd_block_register_default_params(C.byref(p))
    names = [f[0] for f in BlockRegisterParams._fields_]
    for k, v in kw.items():
        if k not in names:
            raise ValueError("block_register: unknown parameter %r" % (k,))
        if k == "model":
            if v not in BLOCK_MODEL:
                raise ValueError("block_register: model must be 'translation', 'rigid' or 'affine', not %r" % (v,))
            v = BLOCK_MODEL[v]
        elif k.startswith("spacing"):
            v = (C.c_double * 3)(*_scale3(v, "block_register", k))
        setattr(p, k, v)
    return p


def block_register(F, M, A, params=None, work=None, mask_fixed=None, mask_moving=None):
    """sift3d_amd_block_register_device on torch CUDA float32 contiguous volumes F [oz, oy, ox] and M [nz, ny, nx], on
    torch's current stream (the call waits for it once per iteration).  A: the 3 x 4 start pull map.  Returns the
    BlockRegisterResult."""
    what = "block_register"
    head, masks = _pair(what, F, M, mask_fixed, mask_moving)
    masks = masks or (None, None)
    a = _affine12(A, what)
    p = params if params is not None else block_register_params()
    need = lib().sift3d_amd_block_register_work_floats(*head[1:4], *head[5:8], p.levels, masks[0] is not None,
                                                       masks[1] is not None)
    if need == 0:
        raise ValueError("%s: levels must be in [1, %d] and every level's fixed grid at least 8 voxels on every axis"
                         % (what, AFFINE_MAX_LEVELS))
    work = _work(work, need + (need & 1), F, what)
    res = BlockRegisterResult()
    _run("sift3d_amd_block_register_device", *head, *masks, _dptr(a), C.byref(p), C.byref(res), work.data_ptr(),
         current_stream())
    return res


# ---- discrete displacement search (contract: include/sift3d_amd.h, "Discrete displacement search") -------------------
def _discrete_int(value, lo, hi, what, name):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not lo <= value <= hi:
        raise ValueError("%s: %s must be an integer in %d .. %d, not %r" % (what, name, lo, hi, value))
    return int(value)


def _discrete_theta(theta, what):
    if isinstance(theta, bool) or not isinstance(theta, (int, float, np.integer, np.floating)) or \
            not (math.isfinite(theta) and theta >= 0):
        raise ValueError("%s: theta must be finite and not negative, not %r" % (what, theta))
    return float(theta)


def _block_field(t, what, name, shape=None, device=None):
    _tensor(t, "%s: %s must be a contiguous float32 CUDA tensor [3, nbz, nby, nbx]%s" %
            (what, name, "" if shape is None else " = %s on the device of the other tensors" % (tuple(shape),)),
            dims=(4,), lead=3, shape=shape, device=device)


def cost_volume(F, W, radius=4, valid_fixed=None, valid_warped=None, cost=None, work=None):
    """sift3d_hip_cost_volume: the mean squared channel difference of every 4^3 block of the fixed stack F [nz, ny, nx]
    or [nc, nz, ny, nx] against W (the moving stack warped onto F's grid) at every displacement of the
    (2 radius + 1)^3 label cube.  valid_fixed, valid_warped: float32 masks [nz, ny, nx] (in where >= 0.5) or None.
    cost: a float32 tensor [nbz, nby, nbx, K] that receives the result, None: allocated.  work: a CUDA tensor of at
    least sift3d_amd_cost_volume_work_bytes bytes or None (this build needs none).  torch CUDA float32 contiguous, on
    torch's current stream, no host synchronisation.  Returns cost; an invalid label or block holds +inf."""
    import torch
    what = "cost_volume"
    nc, (nx, ny, nz), _ = _demons_pair(F, W, what)
    if tuple(W.shape) != tuple(F.shape):
        raise ValueError("%s: W %s is not on the fixed grid %s" % (what, tuple(W.shape), tuple(F.shape)))
    r = _discrete_int(radius, 1, DISCRETE_MAX_RADIUS, what, "radius")
    if not 1 <= nc <= DISCRETE_MAX_CHANNELS:
        raise ValueError("%s: 1 .. %d channels, not %d" % (what, DISCRETE_MAX_CHANNELS, nc))
    if min(nx, ny, nz) < 4:
        raise ValueError("%s: F %s must hold a block of 4 voxels on every axis" % (what, tuple(F.shape)))
    grid = tuple(F.shape[-3:])
    for w, name in ((valid_fixed, "valid_fixed"), (valid_warped, "valid_warped")):
        if w is not None:
            _tensor(w, "%s: %s must be a contiguous float32 CUDA tensor of F's grid %s on its device"
                    % (what, name, grid), shape=grid, device=F.device)
    shape = (nz // 4, ny // 4, nx // 4, (2 * r + 1) ** 3)
    if cost is None:
        cost = torch.empty(shape, dtype=torch.float32, device=F.device)
    else:
        _tensor(cost, "%s: cost must be a contiguous float32 CUDA tensor %s on F's device" % (what, shape),
                shape=shape, device=F.device)
    need = lib().sift3d_amd_cost_volume_work_bytes(nx, ny, nz, nc, r)
    if work is not None or need:
        work = _byte_work(what, work, need, F)
    _run("sift3d_hip_cost_volume", F.data_ptr(), W.data_ptr(), nc, nx, ny, nz,
         None if valid_fixed is None else valid_fixed.data_ptr(),
         None if valid_warped is None else valid_warped.data_ptr(), r, cost.data_ptr(),
         work.data_ptr() if work is not None and work.numel() else None, current_stream())
    return cost


def _cost_radius(cost, what):
    _tensor(cost, "%s: cost must be a contiguous float32 CUDA tensor [nbz, nby, nbx, K]" % what, dims=(4,))
    K = cost.shape[3]
    r = (round(K ** (1.0 / 3)) - 1) // 2
    if not 1 <= r <= DISCRETE_MAX_RADIUS or (2 * r + 1) ** 3 != K or min(cost.shape[:3]) < 1:
        raise ValueError("%s: cost %s does not hold (2 R + 1)^3 labels, R in 1 .. %d, per block"
                         % (what, tuple(cost.shape), DISCRETE_MAX_RADIUS))
    return r


def cost_select(cost, u, theta, v=None, data=None, stats=None, work=None):
    """sift3d_hip_cost_select: per block of the cost volume [nbz, nby, nbx, K] the label d of smallest
    cost + theta |d - u|^2 (ties: the smaller |d|^2, then the smaller index).  u: the block field [3, nbz, nby, nbx]
    the choice is coupled to.  v [3, nbz, nby, nbx], data [nbz, nby, nbx] (the chosen costs), stats (an int64 tensor
    of 2 words: the sum of data over the non-empty blocks and their count, read with demons_stats): the outputs, None:
    allocated.  An empty block (every label +inf) keeps u and has data +inf.  On torch's current stream, no host
    synchronisation.  Returns (v, data, stats)."""
    import torch
    what = "cost_select"
    r = _cost_radius(cost, what)
    nb = tuple(cost.shape[:3])
    th = _discrete_theta(theta, what)
    _block_field(u, what, "u", (3,) + nb, cost.device)
    if v is None:
        v = torch.empty_like(u)
    else:
        _block_field(v, what, "v", (3,) + nb, cost.device)
    if data is None:
        data = torch.empty(nb, dtype=torch.float32, device=cost.device)
    else:
        _tensor(data, "%s: data must be a contiguous float32 CUDA tensor %s on cost's device" % (what, nb), shape=nb,
                device=cost.device)
    stats = _buffer(what, "stats", stats, (DEMONS_STATS_BYTES // 8,), cost)
    nbz, nby, nbx = nb
    work = _byte_work(what, work, lib().sift3d_amd_cost_select_work_bytes(nbx, nby, nbz), cost)
    _run("sift3d_hip_cost_select", cost.data_ptr(), nbx, nby, nbz, r, u.data_ptr(), th, v.data_ptr(), data.data_ptr(),
         stats.data_ptr(), work.data_ptr(), current_stream())
    return v, data, stats


def block_field_smooth(src, passes=2, dst=None, work=None):
    """sift3d_hip_block_field_smooth: `passes` (0 .. 16) passes of the separable binomial (1/4, 1/2, 1/4) with clamped
    indices over every channel of the block field src [3, nbz, nby, nbx]; dst: the output, None: allocated.  On
    torch's current stream.  Returns dst."""
    import torch
    what = "block_field_smooth"
    _block_field(src, what, "src")
    n = _discrete_int(passes, 0, DISCRETE_MAX_PASSES, what, "passes")
    if dst is None:
        dst = torch.empty_like(src)
    else:
        _block_field(dst, what, "dst", tuple(src.shape), src.device)
    nbz, nby, nbx = src.shape[1:]
    need = lib().sift3d_amd_block_field_smooth_work_bytes(nbx, nby, nbz, n)
    if work is not None or need:
        work = _byte_work(what, work, need, src)
    _run("sift3d_hip_block_field_smooth", src.data_ptr(), dst.data_ptr(), nbx, nby, nbz, n,
         work.data_ptr() if work is not None and work.numel() else None, current_stream())
    return dst


def block_field_expand(b, shape, w=None):
    """sift3d_hip_block_field_expand: the block field b [3, nbz, nby, nbx] carried to the voxel grid shape =
    (nz, ny, nx), nb = n // 4 per axis, by trilinear interpolation between the block centres 4 b + 1.5 (edge values
    outside them).  w: the output [3, nz, ny, nx], None: allocated.  On torch's current stream.  Returns w."""
    import torch
    what = "block_field_expand"
    _block_field(b, what, "b")
    nz, ny, nx = (int(n) for n in shape)
    if min(nz, ny, nx) < 4 or tuple(b.shape[1:]) != (nz // 4, ny // 4, nx // 4):
        raise ValueError("%s: b %s is not the block grid of %s" % (what, tuple(b.shape), (nz, ny, nx)))
    if w is None:
        w = torch.empty((3, nz, ny, nx), dtype=torch.float32, device=b.device)
    else:
        _tensor(w, "%s: w must be a contiguous float32 CUDA tensor %s on b's device" % (what, (3, nz, ny, nx)),
                shape=(3, nz, ny, nx), device=b.device)
    _run("sift3d_hip_block_field_expand", b.data_ptr(), nx // 4, ny // 4, nz // 4, w.data_ptr(), nx, ny, nz,
         current_stream())
    return w


def discrete_register_params(radius=None, passes=None, thetas=None):
    """sift3d_amd_discrete_register_params: the defaults, overridden by radius, passes and thetas (1 .. 16 values)"""
    what = "discrete_register"
    p = DiscreteRegisterParams()
    lib().sift3d_amd_discrete_register_default_params(C.byref(p))
    if radius is not None:
        p.radius = _discrete_int(radius, 1, DISCRETE_MAX_RADIUS, what, "radius")
    if passes is not None:
        p.passes = _discrete_int(passes, 0, DISCRETE_MAX_PASSES, what, "passes")
    if thetas is not None:
        th = [_discrete_theta(t, what) for t in thetas]
        if not 1 <= len(th) <= DISCRETE_MAX_THETAS:
            raise ValueError("%s: 1 .. %d thetas, not %d" % (what, DISCRETE_MAX_THETAS, len(th)))
        p.n_theta = len(th)
        for j in range(DISCRETE_MAX_THETAS):
            p.theta[j] = th[j] if j < len(th) else 0.0
    return p


def discrete_register(Fs, Ms, field, params=None, mask_fixed=None, mask_moving=None, work=None):
    """Coarse-to-fine discrete displacement search (sift3d_amd_discrete_register_device): Fs, Ms are the fixed and
    moving feature stacks per level as demons_multires takes them (level 0 the finest, every level the half of the one
    above); the field [3, nz, ny, nx] on Fs[0]'s grid is the start and is updated in place.  params: a
    DiscreteRegisterParams (discrete_register_params), None: the defaults.  mask_fixed, mask_moving: float32 masks on
    level 0's fixed / moving grid or None (the driver restricts them).  torch CUDA float32, on torch's current stream,
    no host synchronisation.  Returns the stats tensor: 16 bytes per (level, theta) in the order run, the coarsest
    level's first (read it with demons_stats)."""
    import torch
    what = "discrete_register"
    p = params if params is not None else discrete_register_params()
    tab, levels, nc, _ = _demons_levels(what, Fs, Ms, field, [0] * len(Fs))
    if not 1 <= nc <= DISCRETE_MAX_CHANNELS:
        raise ValueError("%s: 1 .. %d channels, not %d" % (what, DISCRETE_MAX_CHANNELS, nc))
    wf, wm = _demons_masks(what, Fs[0], Ms[0].shape[-3:], mask_fixed, mask_moving) or (None, None)
    _, nz, ny, nx = field.shape
    mz, my, mx = Ms[0].shape[-3:]
    need = lib().sift3d_amd_discrete_register_work_floats(nx, ny, nz, mx, my, mz, nc, levels, p.radius,
                                                          wf is not None, wm is not None)
    if need == 0:
        raise ValueError("%s: every level's fixed grid must hold a block of 4 voxels on every axis" % what)
    work = _work(work, need, field, what)
    total = levels * p.n_theta
    stats = torch.empty(total * DEMONS_STATS_BYTES // 8, dtype=torch.int64, device=field.device)
    _run("sift3d_amd_discrete_register_device", tab, levels, nc, wf, wm, field.data_ptr(), C.byref(p),
         stats.data_ptr(), work.data_ptr(), current_stream())
    return stats


def absmax(src, out):
    _check(lib().sift3d_hip_absmax(src.data_ptr(), src.numel(), out.data_ptr(), current_stream()),
           "sift3d_hip_absmax")


def scale(src, dst, d_max):
    _check(lib().sift3d_hip_scale(src.data_ptr(), dst.data_ptr(), src.numel(), d_max.data_ptr(),
                                  current_stream()), "sift3d_hip_scale")


def subtract_absmax(a, b, dst, d_absmax=None):
    _check(lib().sift3d_hip_subtract_absmax(a.data_ptr(), b.data_ptr(), dst.data_ptr(), a.numel(),
                                            d_absmax.data_ptr() if d_absmax is not None else None,
                                            current_stream()), "sift3d_hip_subtract_absmax")


def dog_stack(gauss, dogs, d_absmax):
    """dogs[k] = gauss[k] - gauss[k+1] for one octave in a single pass; d_absmax: float32 tensor
    of len(gauss)-1 running maxima.  Returns False when the kernel does not cover the case."""
    n = len(gauss)
    assert len(dogs) == n - 1 and d_absmax.numel() >= n - 1
    g = (C.c_void_p * n)(*[t.data_ptr() for t in gauss])
    d = (C.c_void_p * (n - 1))(*[t.data_ptr() for t in dogs])
    rc = lib().sift3d_hip_dog_stack(g, d, n, gauss[0].numel(), d_absmax.data_ptr(), current_stream())
    if rc == 1:
        return False
    _check(rc, "sift3d_hip_dog_stack")
    return True


def dogmax_stack(gauss, d_absmax):
    """The maxima of dog_stack alone: d_absmax[k] = max(d_absmax[k], max |gauss[k] - gauss[k+1]|), no difference
    stored.  Returns False when the kernel does not cover the case."""
    n = len(gauss)
    assert d_absmax.numel() >= n - 1
    g = (C.c_void_p * n)(*[t.data_ptr() for t in gauss])
    rc = lib().sift3d_hip_dogmax_stack(g, n, gauss[0].numel(), d_absmax.data_ptr(), current_stream())
    if rc == 1:
        return False
    _check(rc, "sift3d_hip_dogmax_stack")
    return True


def downsample2(src, dst):
    nz, ny, nx = src.shape
    mz, my, mx = dst.shape
    _check(lib().sift3d_hip_downsample2(src.data_ptr(), nx, ny, dst.data_ptr(), mx, my, mz,
                                        current_stream()), "sift3d_hip_downsample2")


def synth_lattice(dst, z_off=0, seed=1):
    nz, ny, nx = dst.shape
    _check(lib().sift3d_hip_synth_lattice(dst.data_ptr(), nx, ny, nz, z_off, seed, current_stream()),
           "sift3d_hip_synth_lattice")
    return dst


def level_table(levels):
    """levels: list of dicts(data=tensor, off, nz_glob, units, octave, sd) -> device table
    (torch uint8 tensor) + the numpy mirror."""
    import torch
    tab = np.zeros(len(levels), LEVEL_DTYPE)
    for i, L in enumerate(levels):
        t = L["data"]
        tab[i] = (t.data_ptr(), t.shape[2], t.shape[1], t.shape[0], L["off"], L["nz_glob"],
                  np.float32(L["units"][0]), np.float32(L["units"][1]), np.float32(L["units"][2]),
                  L["octave"], L["sd"])
    dev = torch.from_numpy(tab.view(np.uint8).copy()).cuda()
    return dev, tab


def extrema(levels, nx, ny, nz, peak_thresh, cap=1 << 18, cuboid=False):
    """levels: list of dict(prev, cur, next (tensors), absmax (1-elem tensor), z_lo, z_hi, tag).
    Returns CAND_DTYPE records in the reference's scan order."""
    import torch
    L = lib()
    arr = (ExtremaLevel * len(levels))()
    for i, lv in enumerate(levels):
        arr[i] = ExtremaLevel(lv["prev"].data_ptr(), lv["cur"].data_ptr(), lv["next"].data_ptr(),
                              lv["absmax"].data_ptr(), lv["z_lo"], lv["z_hi"], lv["tag"])
    wb = L.sift3d_hip_extrema_work_bytes(nx, ny, nz, len(levels))
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    while True:
        out = torch.empty(cap * CAND_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        count.zero_()
        _check(L.sift3d_hip_extrema_mode(arr, len(levels), nx, ny, nz, float(peak_thresh),
                                         int(bool(cuboid)), out.data_ptr(), cap, count.data_ptr(),
                                         work.data_ptr(), wb, current_stream()),
               "sift3d_hip_extrema_mode")
        n = int(count.item())
        if n <= cap:
            break
        cap = n + n // 4 + 1024
    return out[:n * CAND_DTYPE.itemsize].cpu().numpy().view(CAND_DTYPE).copy()


# ---- the extrema stage on the caller's buffers ----------------------------------------------------------------------
# d_out / d_count / d_work: tensors or raw device addresses (an output carved out of a larger buffer).  Records are
# appended at *d_count, which the caller initialises; nothing is allocated, grown or read back here.  A return of 1
# ("configuration not covered", nothing done) reaches the caller as a value; any other non-zero code raises.

def _ptr(t):
    return t if t is None or isinstance(t, int) else t.data_ptr()


def _covered(rc, what):
    if rc not in (0, 1):
        _check(rc, what)
    return rc


def _gauss_ptrs(gauss):
    assert len(gauss) == 6
    return (C.c_void_p * 6)(*[_ptr(t) for t in gauss])


def extrema_work_bytes(nx, ny, nz, nlevels=3):
    return int(lib().sift3d_hip_extrema_work_bytes(nx, ny, nz, nlevels))


def extrema_into(levels, nx, ny, nz, peak_thresh, d_out, cap, d_count, d_work, work_bytes, cuboid=False):
    """sift3d_hip_extrema_mode with the caller's d_out, cap and starting count (levels as for extrema())."""
    arr = (ExtremaLevel * len(levels))()
    for i, lv in enumerate(levels):
        arr[i] = ExtremaLevel(_ptr(lv["prev"]), _ptr(lv["cur"]), _ptr(lv["next"]), _ptr(lv["absmax"]), lv["z_lo"],
                              lv["z_hi"], lv["tag"])
    return _covered(lib().sift3d_hip_extrema_mode(arr, len(levels), nx, ny, nz, float(peak_thresh), int(bool(cuboid)),
                                                  _ptr(d_out), int(cap), _ptr(d_count), _ptr(d_work),
                                                  int(work_bytes), current_stream()), "sift3d_hip_extrema_mode")


def extrema_gauss6(gauss, d_absmax, nx, ny, nz, z_lo, z_hi, tag0, peak_thresh, d_out, cap, d_count, d_work,
                   work_bytes, phase=None):
    """sift3d_hip_extrema_gauss6 (phase None) or sift3d_hip_extrema_gauss6_phase (0: both, 1: sweep, 2: scan + emit)
    on six Gaussian levels; d_absmax: the octave's five max|DoG|."""
    L, g = lib(), _gauss_ptrs(gauss)
    a = (g, _ptr(d_absmax), nx, ny, nz, z_lo, z_hi, tag0, float(peak_thresh), _ptr(d_out), int(cap), _ptr(d_count),
         _ptr(d_work), int(work_bytes), current_stream())
    if phase is None:
        return _covered(L.sift3d_hip_extrema_gauss6(*a), "sift3d_hip_extrema_gauss6")
    return _covered(L.sift3d_hip_extrema_gauss6_phase(*(a + (int(phase),))), "sift3d_hip_extrema_gauss6_phase")


def extrema_gauss6_est_phase(gauss, d_est, d_exact, nx, ny, nz, tag0, peak_thresh, d_out, cap, d_count, d_work,
                             work_bytes, phase):
    """sift3d_hip_extrema_gauss6_est_phase: d_est the lower bounds (dogmax_sub), d_exact zeroed before phase 1."""
    return _covered(lib().sift3d_hip_extrema_gauss6_est_phase(
        _gauss_ptrs(gauss), _ptr(d_est), _ptr(d_exact), nx, ny, nz, tag0, float(peak_thresh), _ptr(d_out), int(cap),
        _ptr(d_count), _ptr(d_work), int(work_bytes), current_stream(), int(phase)),
        "sift3d_hip_extrema_gauss6_est_phase")


def extrema_gauss6_finish(octs, peak_thresh, d_out, cap, d_count):
    """sift3d_hip_extrema_gauss6_finish: octs = dicts(gauss, nx, ny, nz, tag0, d_work, work_bytes) of what phase 1 of
    each octave was given."""
    keep = [_gauss_ptrs(o["gauss"]) for o in octs]
    arr = (ExtremaOct * max(len(octs), 1))()
    for i, o in enumerate(octs):
        arr[i] = ExtremaOct(keep[i], o["nx"], o["ny"], o["nz"], o["tag0"], _ptr(o["d_work"]), int(o["work_bytes"]))
    return _covered(lib().sift3d_hip_extrema_gauss6_finish(arr, len(octs), float(peak_thresh), _ptr(d_out), int(cap),
                                                           _ptr(d_count), current_stream()),
                    "sift3d_hip_extrema_gauss6_finish")


def dogmax_sub(gauss, nx, ny, nz, d_est):
    """sift3d_hip_dogmax_sub: the sub-lattice maxima of the five |DoG| levels maxed into d_est[0..4]."""
    return _covered(lib().sift3d_hip_dogmax_sub(_gauss_ptrs(gauss), nx, ny, nz, _ptr(d_est), current_stream()),
                    "sift3d_hip_dogmax_sub")



def orient(d_levels, cands, corner_thresh):
    import torch
    n = len(cands)
    if n == 0:
        return np.zeros((0, 9), np.float32), np.zeros(0, np.int32)
    dc = torch.from_numpy(np.ascontiguousarray(cands).view(np.uint8)).cuda()
    R = torch.empty((n, 9), dtype=torch.float32, device="cuda")
    keep = torch.empty(n, dtype=torch.int32, device="cuda")
    _check(lib().sift3d_hip_orient(d_levels.data_ptr(), dc.data_ptr(), n, float(corner_thresh),
                                   R.data_ptr(), keep.data_ptr(), current_stream()),
           "sift3d_hip_orient")
    return R.cpu().numpy(), keep.cpu().numpy()


def orient_window_fits(nx, ny, ux, uy, sd):
    """The host check of the orientation kernels' 10-bit window packing for one level's numbers (no volume): 1 =
    the clipped window box spans at most 1023 voxels in x and in y."""
    return lib().sift3d_hip_orient_window_fits(int(nx), int(ny), float(ux), float(uy), float(sd))


def orient_tab_bytes(nlevels, n):
    """sift3d_hip_orient_tab_bytes: the scratch of orient_tab for nlevels levels and up to n candidates."""
    return int(lib().sift3d_hip_orient_tab_bytes(int(nlevels), int(n)))


def orient_tab(d_levels, nlevels, cands, corner_thresh, parts=None, tab=None):
    """sift3d_hip_orient_tab over the whole list, or -- parts = [(lv_lo, lv_hi, first, n), (..)] -- the list
    in two parts that run at the same time on two streams (sift3d_hip_orient_tab_part).  tab: a caller-owned
    scratch (contiguous uint8 CUDA tensor of at least orient_tab_bytes(nlevels, n) bytes, zeroed when it was
    allocated) used instead of a fresh one -- the window tables in it survive from call to call."""
    import torch
    n = len(cands)
    L = lib()
    dc = torch.from_numpy(np.ascontiguousarray(cands).view(np.uint8)).cuda()
    R = torch.zeros((n, 9), dtype=torch.float32, device="cuda")
    keep = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    if tab is None:
        tab = torch.zeros(L.sift3d_hip_orient_tab_bytes(nlevels, n), dtype=torch.uint8, device="cuda")
    elif (not isinstance(tab, torch.Tensor) or not tab.is_cuda or tab.dtype != torch.uint8 or
          not tab.is_contiguous() or tab.numel() < L.sift3d_hip_orient_tab_bytes(nlevels, n)):
        raise ValueError("orient_tab: tab must be a contiguous uint8 CUDA tensor of at least "
                         "sift3d_hip_orient_tab_bytes(nlevels, n) bytes")
    torch.cuda.synchronize()
    if parts is None:
        _check(L.sift3d_hip_orient_tab(d_levels.data_ptr(), nlevels, dc.data_ptr(), n, float(corner_thresh),
                                       R.data_ptr(), keep.data_ptr(), tab.data_ptr(), n, current_stream()),
               "sift3d_hip_orient_tab")
    else:
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        for slot, (lv_lo, lv_hi, first, m) in enumerate(parts):
            _check(L.sift3d_hip_orient_tab_part(d_levels.data_ptr(), nlevels, lv_lo, lv_hi, dc.data_ptr(), first, m,
                                                float(corner_thresh), R.data_ptr(), keep.data_ptr(),
                                                tab.data_ptr(), n, slot, streams[slot].cuda_stream),
                   "sift3d_hip_orient_tab_part")
    torch.cuda.synchronize()
    return R.cpu().numpy(), keep.cpu().numpy()


def describe(d_levels, kps):
    import torch
    n = len(kps)
    if n == 0:
        return np.zeros((0, 768), np.float32)
    dk = torch.from_numpy(np.ascontiguousarray(kps).view(np.uint8)).cuda()
    hist = torch.empty((n, 768), dtype=torch.float32, device="cuda")
    _check(lib().sift3d_hip_describe(d_levels.data_ptr(), dk.data_ptr(), n, hist.data_ptr(),
                                     current_stream()), "sift3d_hip_describe")
    return hist.cpu().numpy()


def describe_addr_mode(mode):
    """Form of k_describe's sample addresses for every later launch of the process (tests): 0 the callers' guard,
    1 scalar base + 32-bit offsets, 2 64-bit addresses per lane.  Returns the previous mode."""
    f = lib().sift3d_hip_describe_addr_mode
    f.restype, f.argtypes = C.c_int, [C.c_int]
    return f(int(mode))


def describe_addr32_level(nx, ny, nz, uz, sd):
    """The host guard for one level descriptor (no volume behind it) and one scale: 1 = 32-bit offsets fit."""
    f = lib().sift3d_hip_describe_addr32_level
    f.restype, f.argtypes = C.c_int, [C.POINTER(Level), C.c_double]
    L = Level(None, nx, ny, nz, 0, nz, 1.0, 1.0, uz, 0, sd)
    return f(C.byref(L), float(sd))


def describe_addr32_records(levels, kps):
    """The guard over a record list: levels as (nx, ny, nz, uz, sd) tuples, kps a KP_DTYPE array (host)."""
    f = lib().sift3d_hip_describe_addr32_records
    f.restype, f.argtypes = C.c_int, [C.POINTER(Level), C.c_int, C.c_void_p, C.c_uint32]
    tab = (Level * len(levels))(*[Level(None, nx, ny, nz, 0, nz, 1.0, 1.0, uz, 0, sd)
                                  for nx, ny, nz, uz, sd in levels])
    kps = np.ascontiguousarray(kps, KP_DTYPE)
    return f(tab, len(levels), kps.ctypes.data, len(kps))


def describe_rcp_check(e_lo, n_exp):
    """The fast kernels' reciprocal against 1.0f / x on the device, every float of both signs with biased exponent
    e_lo .. e_lo + n_exp - 1: (mismatches, smallest mismatching bit pattern or 0xffffffff)."""
    f = lib().sift3d_hip_describe_rcp_check
    f.restype, f.argtypes = C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                      C.c_void_p]
    bad, first = C.c_uint64(0), C.c_uint32(0)
    _check(f(int(e_lo), int(n_exp), C.byref(bad), C.byref(first), current_stream()),
           "sift3d_hip_describe_rcp_check")
    return int(bad.value), int(first.value)


# ---- the device stages of the slab driver's keypoint exchange on the caller's buffers (sift3d_slab.hip) -------------
# Every buffer is the caller's (a slice of a larger tensor is fine: guard bands around it stay the caller's business);
# nothing is allocated, sized or read back here.  What the C entries refuse (nkey, n) reaches the caller as RuntimeError.

def _dev_bytes(t, need, what, name, dtype=None):
    _tensor(t, "%s: %s must be a contiguous %sCUDA tensor of >= %d bytes" % (what, name, dtype + " " if dtype else "",
                                                                             need), dtype=dtype)
    if t.numel() * t.element_size() < need:
        raise ValueError("%s: %s holds fewer than %d bytes" % (what, name, need))
    return t.data_ptr()


def slab_count(cand, keep, n, ngl, K, nkey, cnt):
    """sift3d_hip_slab_count: cand n CAND_DTYPE records (uint8 tensor), keep int32 [>= n], cnt int32 [2 nkey]."""
    what, n = "slab_count", int(n)
    _tensor(cnt, "slab_count: cnt must be a contiguous int32 CUDA tensor [2 * nkey]", shape=(2 * max(int(nkey), 0),),
            dtype="int32")
    _check(lib().sift3d_hip_slab_count(_dev_bytes(cand, CAND_DTYPE.itemsize * n, what, "cand", "uint8"),
                                       _dev_bytes(keep, 4 * n, what, "keep", "int32"), n, int(ngl), int(K),
                                       int(nkey), cnt.data_ptr(), current_stream()), "sift3d_hip_slab_count")


def slab_pack_scratch_bytes(n):
    return int(lib().sift3d_hip_slab_pack_scratch_bytes(int(n)))


def slab_pack(d_levels, cand, keep, R, n, ngl, vals, recs, scratch):
    """sift3d_hip_slab_pack: vals float32 [>= n]; recs a uint8 tensor of whole SLAB_REC_DTYPE records, room for every
    kept candidate (the caller's count); scratch >= slab_pack_scratch_bytes(n) bytes."""
    what, n = "slab_pack", int(n)
    _tensor(d_levels, "slab_pack: d_levels must be the uint8 CUDA tensor of level_table()", dtype="uint8")
    _dev_bytes(recs, 0, what, "recs", "uint8")
    if d_levels.numel() % LEVEL_DTYPE.itemsize or recs.numel() % SLAB_REC_DTYPE.itemsize:
        raise ValueError("slab_pack: d_levels / recs must hold whole records")
    _check(lib().sift3d_hip_slab_pack(d_levels.data_ptr(), _dev_bytes(cand, CAND_DTYPE.itemsize * n, what, "cand",
                                                                      "uint8"),
                                      _dev_bytes(keep, 4 * n, what, "keep", "int32"),
                                      _dev_bytes(R, 36 * n, what, "R", "float32"), n, int(ngl),
                                      _dev_bytes(vals, 4 * n, what, "vals", "float32"), recs.data_ptr(),
                                      _dev_bytes(scratch, slab_pack_scratch_bytes(n), what, "scratch"),
                                      current_stream()), "sift3d_hip_slab_pack")


def slab_table_words(world, nkey):
    return 2 * (nkey * world + 1) + 2 * world * (nkey + 1)


def slab_table(cnt, nkey):
    """sift3d_amd_slab_table (host): cnt a C-contiguous int32 numpy array [world, >= 2 nkey], a row per rank ->
    (the table as uint32 words, the layout as a dict of the header's fields)."""
    cnt = np.asarray(cnt)
    if cnt.dtype != np.int32 or cnt.ndim != 2 or not cnt.flags.c_contiguous or cnt.shape[0] < 1:
        raise ValueError("slab_table: cnt must be a C-contiguous int32 array [world, >= 2 * nkey]")
    world, nkey = cnt.shape[0], int(nkey)
    tab = np.zeros(slab_table_words(world, min(max(nkey, 1), 256)), np.uint32)
    lay = SlabLayout()
    _check(lib().sift3d_amd_slab_table(cnt.ctypes.data, cnt.strides[0], world, nkey, tab.ctypes.data, C.byref(lay)),
           "sift3d_amd_slab_table")
    return tab, {f: int(getattr(lay, f)) for f, _ in SlabLayout._fields_}


def slab_build(all_blocks, blk_bytes, roff, toff, world, nkey, tab, tot_k, tot_c, out):
    """sift3d_hip_slab_build: all_blocks world blocks of blk_bytes; tab the words of slab_table on the device; out
    SLAB_HEADER_BYTES + tot_k SLAB_OUT_DTYPE records."""
    what = "slab_build"
    _check(lib().sift3d_hip_slab_build(_dev_bytes(all_blocks, int(world) * int(blk_bytes), what, "all_blocks"),
                                       int(blk_bytes), int(roff), int(toff), int(world), int(nkey),
                                       _dev_bytes(tab, 4 * slab_table_words(int(world), int(nkey)), what, "tab"),
                                       int(tot_k), int(tot_c),
                                       _dev_bytes(out, SLAB_HEADER_BYTES + SLAB_OUT_DTYPE.itemsize * int(tot_k), what,
                                                  "out"), current_stream()), "sift3d_hip_slab_build")


def rows_scatter(dst, all_blocks, blk_bytes, rows_map, n):
    """sift3d_hip_rows_scatter: dst float32 [>= n * ROW_FLOATS], row g = row (map[g] & 0xffffff) of block map[g] >> 24;
    blk_bytes and both buffers on 16-byte boundaries (the rows move as float4)."""
    what, n = "rows_scatter", int(n)
    p = (_dev_bytes(dst, 4 * ROW_FLOATS * n, what, "dst", "float32"), _dev_bytes(all_blocks, 0, what, "all_blocks"),
         _dev_bytes(rows_map, 4 * n, what, "rows_map"))
    if int(blk_bytes) % 16 or (n and (p[0] % 16 or p[1] % 16)):
        raise ValueError("rows_scatter: blk_bytes, dst and all_blocks must be multiples of 16 bytes")
    _check(lib().sift3d_hip_rows_scatter(p[0], p[1], int(blk_bytes), p[2], n, current_stream()),
           "sift3d_hip_rows_scatter")


def max_rows(dst, rows, nrows, n):
    """sift3d_hip_max_rows: dst[i] = max over r of rows[r * n + i] (float32 tensors of >= n and >= nrows * n)."""
    what, nrows, n = "max_rows", int(nrows), int(n)
    _check(lib().sift3d_hip_max_rows(_dev_bytes(dst, 4 * max(n, 0), what, "dst", "float32"),
                                     _dev_bytes(rows, 4 * max(nrows, 0) * max(n, 0), what, "rows", "float32"), nrows, n,
                                     current_stream()), "sift3d_hip_max_rows")
