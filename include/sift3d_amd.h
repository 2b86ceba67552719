/* sift3d_amd.h -- MI355X-side C ABI underneath the drop-in API (include/sift3d/).
 *
 * Two groups of entry points, all `extern "C"`, plain pointers and sizes:
 *
 *  sift3d_amd_*  extensions of the reference API that only make sense with a
 *                device: hand the detector a volume that is already resident in
 *                HBM, query stage timings, generate synthetic volumes.
 *  sift3d_hip_*  the stage kernels themselves, operating on DEVICE pointers and a
 *                HIP stream.  The C host code of the drop-in library calls these;
 *                so does the Z-slab multi-GPU driver (sift3d_amd/sharded.py), which
 *                is why every stage takes local-slab geometry (global length,
 *                offset of the local buffer, plane range to produce).
 *
 * Each stage cites the reference function (file:line under /root/reference/sift3d/)
 * whose results it reproduces.  Volumes are float32, x fastest:
 * index = x + nx*(y + ny*z) (reference: imutil.c:520-533).
 */
#ifndef SIFT3D_AMD_H
#define SIFT3D_AMD_H

#include <stddef.h>
#include <stdint.h>

#include "sift3d/imtypes.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIFT3D_AMD_API __attribute__((visibility("default")))

/* ------------------------------------------------------------------------ */
/* Extensions of the drop-in API                                            */
/* ------------------------------------------------------------------------ */

/* As sift3d_detect_keypoints (reference: sift.c:1217-1249) for a single-channel
 * nx*ny*nz float32 volume that already lives in device memory (`d_volume`), with
 * voxel spacing (ux,uy,uz) > 0.  The volume is not modified.
 * Synchronisation contract: the work is issued on the detector's own stream, which is NOT
 * ordered after other streams -- the caller makes sure the producer of d_volume has finished
 * (e.g. torch.cuda.synchronize(), or an event wait) before calling; on return the results are
 * complete (the call synchronises its stream).  A detector belongs to the HIP device that was
 * current at its first detect call. */
SIFT3D_AMD_API int
sift3d_amd_detect_keypoints_device(sift3d_detector *det, const float *d_volume,
                                   int nx, int ny, int nz, double ux, double uy,
                                   double uz, sift3d_keypoint_store *store);

/* Voxel spacing of an image made by sift3d_make_image (the reference sets units
 * only through its NIfTI reader, nifti.c:52-167). */
SIFT3D_AMD_API int
sift3d_amd_image_set_units(sift3d_image *im, double ux, double uy, double uz);

/* Extremum neighbourhood of the following detect calls: 0 (default) = the default build's
 * 8-neighbour test, non-zero = the reference's compile-time CUBOID_EXTREMA variant
 * (sift.c:24, 761-796), here a run-time option. */
SIFT3D_AMD_API int
sift3d_amd_detector_set_cuboid_extrema(sift3d_detector *det, int on);

/* The dogmax scan (sift.c:821-826) of octave 0 as a pass of its own over the octave's Gaussian levels
 * (non-zero) or gathered by the extrema sweep from lower bounds (0, the default: see
 * sift3d_hip_extrema_gauss6_est_phase).  Same candidates either way; an A/B switch for tests and profiles. */
SIFT3D_AMD_API int
sift3d_amd_detector_set_dogmax_pass(sift3d_detector *det, int on);
/* Orientation window sums: 0 (default) = parallel sums with decisions by margin and a serial re-run of the
 * undecided candidates; non-zero = the reference's serial sums (sift.c:978-990) for every candidate.  Same
 * keypoints and R bit for bit either way; an A/B switch for tests and profiles. */
SIFT3D_AMD_API int
sift3d_amd_detector_set_serial_orientation(sift3d_detector *det, int on);
/* Candidate list capacity, a diagnostic hook: cap >= 1 waits for the detector's streams, releases the
 * candidate arrays and makes the next detect start from exactly cap records; 0 restores the default (2^18);
 * negative values fail.  A detect whose extrema do not fit grows the arrays to count + count / 4 + 1024 and
 * sweeps again, as it does from the default.  sift3d_amd_detector_candidate_capacity returns the capacity the
 * arrays have (or the next detect starts from), -1 for a NULL detector. */
SIFT3D_AMD_API int
sift3d_amd_detector_set_candidate_capacity(sift3d_detector *det, int cap);
SIFT3D_AMD_API int
sift3d_amd_detector_candidate_capacity(const sift3d_detector *det);
/* Descriptor accumulation (sift3d_extract_descriptors): 0 (default) = automatic: keypoints whose OWN window
 * holds more than ~1.9e5 voxels -- (20 sd)^3 / (ux uy uz 8^o), from the keypoint's own sd and octave, so also
 * for caller-made keypoints whose sd is not their level's; for detect's keypoints sigma0 * 2^(s/K) above ~2.9
 * voxels, never with the default parameters -- are computed in the reference's accumulation order (their
 * histograms are the reference's bit for bit), the others by the fast two-histogram commit (within 1e-5
 * relative, elementwise); 1 = every keypoint in the reference's order (bit-exact descriptors, ~1.5x the time);
 * -1 = never.
 * sift3d_extract_descriptors accepts what the reference's verify_keys accepts (sift.c:1171-1212) and keypoints
 * of any sd and any finite R (not only rotations); in addition it refuses, before any launch, a keypoint whose
 * (o, s) is not a level of the pyramid, and one whose window box would span more than 2^32 voxels (its packed
 * voxel offsets would not fit in 32 bits -- only possible on volumes of more than 2^32 voxels). */
SIFT3D_AMD_API int
sift3d_amd_detector_set_exact_descriptors(sift3d_detector *det, int mode);
/* max|DoG| of every DoG level of the last detect call, out[octave * levels + level] (the values
 * detect_extrema scales peak_thresh with, sift.c:821-829); returns their number, -1 on failure. */
SIFT3D_AMD_API int
sift3d_amd_detector_dogmax(const sift3d_detector *det, float *out, int cap);

/* Dimensions (nx, ny, nz, nc) and voxel spacing of an image, e.g. one returned by
 * sift3d_read_image (the reference keeps both private).  Either output may be NULL. */
SIFT3D_AMD_API int
sift3d_amd_image_info(const sift3d_image *im, int *dims4, double *units3);

/* Wall-clock seconds of the stages of the last detect/describe on `det`:
 * [0] upload+scale  [1] Gaussian pyramid  [2] DoG  [3] extrema  [4] orientation
 * [5] describe  [6] pyramid kernels only, device time from HIP events
 * [7] whole detect, device time  [8] whole describe, device time
 * [9] the LAST fused y+z FIR launch of octave 0 alone (HIP events on its stream; 0 when that blur did
 *     not take the fused kernel) -- in the pipeline it shares the device with the octave streams.
 * [10 .. 10+B-1]    the x-pass launch of blur s = 0 .. B-1 of octave 0 (B = SIFT3D_AMD_TIMED_BLURS),
 * [10+B .. 10+2B-1] its fused y+z launch: HIP events around each launch on the stream it runs on (0 for a
 *     blur that did not take the fused kernel).  Every octave-0 pyramid launch of the step is timed, so the
 *     LONGEST in-step launch can be named (bench.py's roofline.kernel).
 * Since round 5 the stages overlap: [1] ends with the last of the pyramid's three chains, [2] and [3] start on
 * the main stream when octave 0 is complete -- their sum can exceed [7]. */
#define SIFT3D_AMD_TIMED_BLURS 8
/* [10+2B] the device span of the whole detect call (first to last stage event): [7] minus this is what the host
 * adds (enqueueing, its synchronisations, the candidate -> keypoint compaction); [10+2B+1] the compaction alone;
 * [10+2B+2], [10+2B+3] first stage event -> end of the orientation kernels of octave 0's candidates / of the
 * other octaves' (the default schedule orients octave 0 while the smaller octaves are still swept; 0 otherwise) */
#define SIFT3D_AMD_NUM_TIMINGS (10 + 2 * SIFT3D_AMD_TIMED_BLURS + 4)
SIFT3D_AMD_API const double *
sift3d_amd_timings(const sift3d_detector *det);

/* max|v| + the Gaussian pyramid alone of a float32 volume in device memory (the first part of
 * sift3d_amd_detect_keypoints_device: sift.c:645-649, 662-711), blocking; timings()[1] is its device time. */
SIFT3D_AMD_API int
sift3d_amd_build_pyramid_device(sift3d_detector *det, const float *d_volume, int nx, int ny, int nz,
                                double ux, double uy, double uz);

/* Shader cycles and seconds (from the device's constant 100 MHz counter) of the fast descriptor kernel of the
 * last sift3d_extract_descriptors on `det`, measured by the kernel itself (sift3d_hip_describe_clock). */
SIFT3D_AMD_API int
sift3d_amd_describe_clock(const sift3d_detector *det, double *cycles, double *seconds);

/* Number of DoG extrema before orientation filtering in the last detect. */
SIFT3D_AMD_API int
sift3d_amd_num_candidates(const sift3d_detector *det);

/* Copy level (o, s) of the Gaussian (which=0) or DoG (which=1) pyramid, or the
 * scaled input (which=2), of the last detect to host memory.  dims receives
 * nx,ny,nz.  `out` may be NULL to query dims only. */
SIFT3D_AMD_API int
sift3d_amd_copy_level(const sift3d_detector *det, int which, int o, int s,
                      float *out, int *dims);

/* Raw views of the stores (the reference keeps these private; the parity tests
 * need R, sd, strength without the "%f" CSV rounding of *_save). */
SIFT3D_AMD_API int
sift3d_amd_keypoint_store_size(const sift3d_keypoint_store *);
SIFT3D_AMD_API int
sift3d_amd_keypoint_store_get(const sift3d_keypoint_store *, int i, int *o, int *s,
                              double *xyz_sd /*4*/, float *strength, float *R /*9*/);
SIFT3D_AMD_API int
sift3d_amd_keypoint_store_set(sift3d_keypoint_store *, int n, const int *os /*2n*/,
                              const double *xyz_sd /*4n*/, const float *strength,
                              const float *R /*9n*/);
SIFT3D_AMD_API int
sift3d_amd_descriptor_store_size(const sift3d_descriptor_store *);
/* Fill a descriptor store from host arrays (n records of {x, y, z, sd} and 768 floats; the image
 * dimensions the reference keeps in the store): lets the writers and converters be checked
 * against reference-written files without a device. */
SIFT3D_AMD_API int
sift3d_amd_descriptor_store_set(sift3d_descriptor_store *, int n, const double *xyz_sd /*4n*/,
                                const float *hist /*768n*/, int nx, int ny, int nz);

/* init_Gauss_filter (imutil.c:1267-1319) on the host: normalised taps for `sigma`.
 * Returns the width (taps are written when width <= max_taps) or -1. */
SIFT3D_AMD_API int sift3d_amd_gauss_filter(double sigma, float *taps, int max_taps);

/* Uploads the icosahedron tables the descriptor kernel needs (done implicitly by the first
 * detect); for callers that drive the sift3d_hip_* stages themselves. */
SIFT3D_AMD_API int sift3d_amd_init(void);

/* 1 when a usable HIP device is present. */
SIFT3D_AMD_API int sift3d_amd_device_available(void);
SIFT3D_AMD_API const char *sift3d_amd_version(void);

/* ------------------------------------------------------------------------ */
/* Registration: descriptor matching + RANSAC affine (BASELINE config 5)     */
/* ------------------------------------------------------------------------ */
/* Removed from the reference fork (CHANGES.md:99-103; upstream: README-OLD.md:5) -- no reference
 * code, no oracle: parity with upstream cannot be pinned.  Matching and RANSAC are pinned bit for bit
 * to numpy restatements instead (tests/match_restatement.py).  See sift3d_amd/csrc/sift3d_register.c. */

/* Nearest / second-nearest neighbour of each of the nA rows of d_A (nA x dim floats, row-major)
 * among the nB rows of d_B under the squared L2 distance, on the matrix cores
 * (v_mfma_f32_32x32x2_f32).  d_j1[i] = index of the nearest row (-1: nB == 0), d_d1 / d_d2 =
 * squared distances to the nearest and second nearest (+inf when absent).  dim % 16 == 0.
 * d_work: sift3d_hip_nn2_work_floats(nA, nB) floats of device scratch. */
SIFT3D_AMD_API size_t sift3d_hip_nn2_work_floats(int nA, int nB);
SIFT3D_AMD_API int
sift3d_hip_nn2(const float *d_A, int nA, const float *d_B, int nB, int dim, int *d_j1, float *d_d1,
               float *d_d2, float *d_work, void *stream);

/* ---- Transform-guided (spatially gated) nearest neighbours ----
 * The same search over the candidates inside a spatial gate only.  Set A has positions pa_i -- A's keypoints
 * MAPPED INTO B's FRAME by the caller --, set B positions pb_j; d_posA / d_posB: float32, n x 4 (x, y, z and an
 * ignored float), 16-byte aligned.  r2 = (float)(radius * radius), the product taken in double.
 *   gate(i, j):  dx = pa_i.x - pb_j.x, dy, dz likewise, all in f32
 *                d2 = (dx*dx + dy*dy) + dz*dz          (no contraction)
 *                d2 <= r2                              (a NaN anywhere: false)
 * Swapping the roles only negates dx, dy, dz: a backward search (B against A) over the SAME two position arrays
 * evaluates bit-identical d2, so the gate is symmetric by construction.
 * For every row of A: the lexicographic (distance, original index) top-2 over the gated candidates.  The
 * distance of a pair is bit for bit sift3d_hip_nn2's (the same fma chain, |b|^2 - 2 a.b, max(|a|^2 + e, 0)
 * after the merge).  No candidate: d_j1 = -1, d_d1 = d_d2 = +inf; one candidate: d_d2 = +inf.  With r2 = +inf
 * and finite positions the three outputs equal sift3d_hip_nn2's bit for bit.
 * d_permA / d_permB (int32, NULL: the identity): the row order in which the kernel walks each set -- block row r
 * is original row perm[r]; a permutation is trusted to be one.  Results never depend on it (ties go to the
 * smaller ORIGINAL index); what depends on it is the work: the box of every 128-row block is computed first
 * (fminf / fmaxf; a point with a NaN coordinate stays out), and a block of A skips a block of B when
 *   gap2 = (gx*gx + gy*gy) + gz*gz > r2,   g = max(0, max(loA - hiB, loB - hiA)) per axis, in f32.
 * f32 rounding is monotone, so every pair of the two blocks has d2 >= gap2: the skip is exact, no epsilon.
 * d_visited (NULL or 2 counters): set to {block pairs visited, block pairs in all}, a pure function of the
 * positions, the permutations and r2.  Nothing synchronises with the host.
 * Refused before any device call: what sift3d_hip_nn2 refuses, a NULL or misaligned position array, r2 < 0 or NaN.
 * d_work: sift3d_hip_nn2_gated_work_floats(nA, nB) floats
 *   = sift3d_hip_nn2_work_floats(nA, nB) + 8 (ceil(nA / 128) + ceil(nB / 128)). */
SIFT3D_AMD_API size_t sift3d_hip_nn2_gated_work_floats(int nA, int nB);
SIFT3D_AMD_API int
sift3d_hip_nn2_gated(const float *d_A, int nA, const float *d_B, int nB, int dim, const float *d_posA,
                     const float *d_posB, float r2, const int *d_permA, const int *d_permB, int *d_j1,
                     float *d_d1, float *d_d2, unsigned long long *d_visited, float *d_work, void *stream);

/* A row order that makes 128-row blocks spatially compact (device-free).  perm[0 .. n) = the indices of the n
 * points xyz[3 i ..] sorted by (key, index); key = the Morton interleave (bit 3 b + k of the key = bit b of axis
 * k's cell) of floor(p / cell) per axis, offset by the smallest cell of the set on that axis and clamped to 21
 * bits.  Points with a non-finite coordinate go last, by index.  cell > 0 (+inf: the identity). */
SIFT3D_AMD_API int sift3d_amd_spatial_order(const double *xyz, int n, double cell, int *perm);

/* match_ab[i] (i < size of a) = index in b of the descriptor matched to descriptor i of a, or -1:
 * nearest neighbour accepted when (nearest distance) / (second nearest) < nn_thresh (e.g. 0.8)
 * in BOTH directions and mutual. */
SIFT3D_AMD_API int
sift3d_amd_nn_match(const sift3d_descriptor_store *a, const sift3d_descriptor_store *b,
                    double nn_thresh, int *match_ab);
/* A matcher object: its own stream and scratch (grown on demand, reused from call to call: no
 * allocation per match).  sift3d_amd_matcher_match is sift3d_amd_nn_match on it;
 * sift3d_amd_matcher_seconds returns the device time of the two nearest-neighbour searches of the last
 * match (HIP events on the matcher's stream).  Descriptor stores marked with
 * sift3d_amd_descriptor_store_keep_device(store, 1) keep a copy of their histograms in HBM (written by
 * sift3d_extract_descriptors beside the host array), which the matcher reads in place; other stores
 * are uploaded per call. */
typedef struct sift3d_amd_matcher sift3d_amd_matcher;
SIFT3D_AMD_API sift3d_amd_matcher *sift3d_amd_make_matcher(void);
SIFT3D_AMD_API void sift3d_amd_free_matcher(sift3d_amd_matcher *);
SIFT3D_AMD_API int sift3d_amd_matcher_match(sift3d_amd_matcher *, const sift3d_descriptor_store *a,
                                            const sift3d_descriptor_store *b, double nn_thresh,
                                            int *match_ab);
SIFT3D_AMD_API double sift3d_amd_matcher_seconds(const sift3d_amd_matcher *);
/* Guided matching: sift3d_amd_matcher_match's rule on the gated searches.  pred_a: the position of every
 * descriptor of a predicted in b's frame (3 doubles each; rounded to nearest float, as b's own coordinates);
 * radius > 0 (+inf allowed).  Both sets are walked in sift3d_amd_spatial_order(.., cell = radius); the forward
 * and the backward search take the same two position arrays.  Accepted: forward ratio test, backward ratio
 * test, mutual, and -- when max_distance > 0 -- d1 <= (float)(max_distance * max_distance) on the squared
 * descriptor distance (a sole candidate in the gate passes the ratio test against +inf: the cap guards that
 * case).  Without max_distance every blind match (i -> j) with gate(i, j) true is also a guided match.
 * sift3d_amd_matcher_blocks: the block pairs visited and in all of the last guided match, both searches summed. */
SIFT3D_AMD_API int sift3d_amd_matcher_match_guided(sift3d_amd_matcher *, const sift3d_descriptor_store *a,
                                                   const sift3d_descriptor_store *b, const double *pred_a,
                                                   double radius, double nn_thresh, double max_distance,
                                                   int *match_ab);
SIFT3D_AMD_API int sift3d_amd_matcher_blocks(const sift3d_amd_matcher *, uint64_t *visited, uint64_t *total);
SIFT3D_AMD_API int sift3d_amd_descriptor_store_keep_device(sift3d_descriptor_store *, int on);
SIFT3D_AMD_API int
sift3d_amd_descriptor_store_xyz(const sift3d_descriptor_store *, int i, double *xyz /*3*/);
SIFT3D_AMD_API int
sift3d_amd_descriptor_store_xyz_all(const sift3d_descriptor_store *, double *xyz /*3 per descriptor*/);

/* RANSAC fit of the affine map dst = A [src; 1] (tform: 3 x 4 doubles, row-major) to n point
 * pairs (n x 3 doubles each): num_iter minimal samples of 4 pairs, inliers = residual <=
 * err_thresh, least-squares refit on the best consensus set.  inlier (n bytes, may be NULL)
 * receives 0 / 1.  Deterministic for a given seed. */
SIFT3D_AMD_API int
sift3d_amd_ransac_affine(const double *src, const double *dst, int n, double err_thresh, int num_iter,
                         uint64_t seed, double *tform, unsigned char *inlier, int *num_inliers);

/* ------------------------------------------------------------------------ */
/* Resampling: apply an affine map to a volume                               */
/* ------------------------------------------------------------------------ */
/* A is 3 x 4 doubles, row-major, a PULL map: output voxel (x, y, z) reads the source at
 *   q_d = A[d][0] x + ((A[d][1] y + A[d][2] z) + A[d][3])      (double, in this order, unfused)
 * in octave-0 voxel units -- the units of sift3d_amd_descriptor_store_xyz and of
 * sift3d_amd_ransac_affine (converting physical, anisotropic units is the caller's job).  To resample
 * the moving image of a registration into the fixed image's grid, pass the inverse of the
 * moving -> fixed affine (sift3d_amd_affine_invert).  A sample is inside when 0 <= q_d <= n_d - 1 on
 * every axis (a NaN is outside); outside voxels get `fill`.
 *   LINEAR : i = floor(q), f = (float)(q - i), j = min(i + 1, n - 1); lerp(a, b, f) = a + f (b - a) in
 *            float, along x for the four (y, z) corner rows, then along y, then along z
 *   NEAREST: the value at floor(q + 0.5)
 * The arithmetic is fixed: identity maps, integer translations and axis permutations / flips are exact
 * copies.  Arguments are checked before any device call (-1 on NULL pointers, dims <= 0, an unknown
 * interp, a non-finite A, overlapping src / dst). */
#define SIFT3D_AMD_INTERP_NEAREST 0
#define SIFT3D_AMD_INTERP_LINEAR 1
/* device buffers, asynchronous on `stream`, no allocation */
SIFT3D_AMD_API int
sift3d_hip_warp_affine(const float *d_src, int nx, int ny, int nz, float *d_dst, int ox, int oy, int oz,
                       const double *A /*12*/, int interp, float fill, void *stream);
/* host image objects (nc == 1); the output grid is dst's; blocking */
SIFT3D_AMD_API int
sift3d_amd_image_warp_affine(const sift3d_image *src, const double *A, int interp, float fill,
                             sift3d_image *dst);
/* inverse of the affine map x -> A [x; 1]; -1 when the 3x3 part is singular or not finite */
SIFT3D_AMD_API int sift3d_amd_affine_invert(const double *A /*12*/, double *Ainv /*12*/);

/* ------------------------------------------------------------------------ */
/* Thin-plate spline: a smooth deformable pull map                            */
/* ------------------------------------------------------------------------ */
/* A PULL map in voxel units, like sift3d_hip_warp_affine: output (fixed-grid) voxel p = (x, y, z) reads
 * the source (moving volume) at q(p).  Control points c_i (fixed voxels, i = 0 .. m-1), weights
 * w_i in R^3 and an affine A (3 x 4, row-major):
 *   q_d(p)      = affine_d(p) + (double) s_d(p)
 *   affine_d(p) = A[d][0] x + ((A[d][1] y + A[d][2] z) + A[d][3])     double, warp_affine's order
 *   s_d(p)      = float sum over i = 0 .. m-1 in this order, from 0.0f:  s_d = s_d + w_i,d * (-r_i),
 *                 r_i = sqrtf((dx dx + dy dy) + dz dz), dx = (float) x - cx_i, ...  (float, unfused,
 *                 correctly rounded sqrt)
 * The radial basis is phi(r) = -r (the 3-D biharmonic kernel, with the sign that makes it conditionally
 * positive definite); the weights keep their sign in the contract and in sift3d_amd_tps_fit, and the
 * DEVICE layout stores them negated (s + (-w) r equals s + w (-r) bit for bit).  c_i and w_i above are
 * the float32 values of the device layout (sift3d_amd_tps_pack): per point SIFT3D_AMD_TPS_FLOATS floats
 *   { (float) cx, (float) cy, (float) cz, 0, -(float) wx, -(float) wy, -(float) wz, 0 }.
 * Inside test, `fill`, LINEAR and NEAREST sampling at q are sift3d_hip_warp_affine's, word for word.  With
 * all weights zero the result is warp_affine's with the same A, bit for bit. */
#define SIFT3D_AMD_TPS_MAX_POINTS 16384
#define SIFT3D_AMD_TPS_FLOATS 8
/* Fit q = TPS(p) to n point pairs src[i] (fixed voxels) -> dst[i] (moving voxels), n x 3 doubles each.
 * Solves [Phi + lambda I, P; P^T, 0] [w; a] = [dst; 0] in double (Phi_ij = phi(|c_i - c_j|),
 * P = [1 x y z], lambda = smoothing): QR of P, Cholesky of the projected (m - 4)^2 block.
 *   - exact duplicate src points are dropped, the lowest index kept;
 *   - when more than max_points remain, greedy farthest-point sampling over src thins them: start at the
 *     first remaining index; repeatedly add the remaining point whose squared distance
 *     (dx dx + dy dy) + dz dz (double) to its nearest chosen point is largest, the lowest index on ties;
 *   - the control points keep their input order (ascending index).
 * Outputs: ctrl (m x 3), weights (m x 3), A (12), *m; ctrl and weights hold max_points rows.
 * -1 and no output written on: NULL pointers, n < 5, non-finite input, smoothing < 0 or not finite,
 * max_points < 5 or > SIFT3D_AMD_TPS_MAX_POINTS, fewer than 5 distinct points, coplanar control points,
 * a failed factorisation or allocation.  OpenMP team of at most 16 threads; the result does not depend
 * on the team size. */
SIFT3D_AMD_API int
sift3d_amd_tps_fit(const double *src, const double *dst, int n, double smoothing, int max_points,
                   double *ctrl, double *weights, double *A /*12*/, int *m);
/* q(p) for n points p (n x 3 doubles) in double: affine_d(p) + sum_i w_i,d phi(|p - c_i|), for checking
 * fits.  -1 on NULL pointers, m < 1 or n < 0. */
SIFT3D_AMD_API int
sift3d_amd_tps_apply(const double *ctrl, const double *weights, const double *A, int m, const double *p,
                     int n, double *q);
/* the device layout of m points: out holds m * SIFT3D_AMD_TPS_FLOATS floats.  -1 on NULL, m < 1,
 * m > SIFT3D_AMD_TPS_MAX_POINTS, or a value that is not finite in float. */
SIFT3D_AMD_API int
sift3d_amd_tps_pack(const double *ctrl, const double *weights, int m, float *out);
/* device buffers, asynchronous on `stream`, no allocation.  d_tps: the packed layout (16-byte aligned),
 * 1 <= m <= SIFT3D_AMD_TPS_MAX_POINTS.  The output is split into launches of consecutive tiles
 * (64 x 4 x 8 voxels, numbered x, y, then z: whole z-ranges whenever one 8-plane slab fits) so that no
 * launch is estimated above ~50 ms; the split does not change any result.  Arguments are checked
 * before any device call (-1 on NULL pointers, dims <= 0, m out of range, an unknown interp, a
 * non-finite A, a misaligned d_tps, a destination that overlaps the source or d_tps). */
SIFT3D_AMD_API int
sift3d_hip_warp_tps(const float *d_src, int nx, int ny, int nz, float *d_dst, int ox, int oy, int oz,
                    const double *A /*12*/, const float *d_tps, int m, int interp, float fill, void *stream);
/* the number of launches sift3d_hip_warp_tps makes for this output grid and m (-1 for bad arguments) */
SIFT3D_AMD_API int sift3d_hip_warp_tps_launches(int ox, int oy, int oz, int m);
/* host image objects (nc == 1), tps in the packed layout on the host; the output grid is dst's;
 * blocking.  Also refuses non-finite packed values. */
SIFT3D_AMD_API int
sift3d_amd_image_warp_tps(const sift3d_image *src, const double *A, const float *tps, int m, int interp,
                          float fill, sift3d_image *dst);

/* ------------------------------------------------------------------------ */
/* Displacement fields: export, resampling through a field, Jacobian         */
/* ------------------------------------------------------------------------ */
/* A displacement field is float u[3][oz][oy][ox], planar: channel 0 holds x, 1 y, 2 z, in source (moving)
 * voxels.  It is a PULL map, as for the warps above: output voxel p = (x, y, z) reads the source at
 * q(p) = p + u(p).  Voxel units only (physical / anisotropic spacing is the caller's job).
 *
 * Export (p_d is x, y or z as a double; q_d as in the blocks above):
 *   affine : u_d = (float)(q_d - (double) p_d), q_d = A[d][0] x + ((A[d][1] y + A[d][2] z) + A[d][3])
 *            (double, warp_affine's order, unfused)
 *   TPS    : u_d = (float)((affine_d(p) + (double) s_d(p)) - (double) p_d), s_d the float radial sum of
 *            "Thin-plate spline" (point order, from 0.0f, unfused, correctly rounded sqrtf).  With all weights
 *            zero this is the affine export bit for bit (but for the sign of a zero: an affine_d that is
 *            exactly -0.0 at p_d = 0 becomes +0.0, as adding (double) 0.0f does).
 * Resampling through a field (nc >= 1 channels, src [nc][nz][ny][nx], dst [nc][oz][oy][ox]): every channel
 * is sampled at the same point
 *   q_d = (double) p_d + (double) u_d(p)
 * with sift3d_hip_warp_affine's inside test, `fill`, LINEAR and NEAREST, word for word (a NaN in the field
 * samples outside).  So channel c of an nc-channel warp is the single-channel warp of channel c, and when
 * every u is exact (u = (float)(q - p) with no rounding: the affine field of the identity, of an integer
 * translation, of axis permutations / flips) the result is warp_affine's with that A, bit for bit.
 * Jacobian determinant of q(p), per voxel, float unless stated:
 *   1. g_de = d u_d / d x_e by numpy.gradient's rules: (u[i+1] - u[i-1]) * 0.5f inside, u[1] - u[0] and
 *      u[n-1] - u[n-2] at the ends, 0 on an axis of length 1;
 *   2. j_de = (d == e ? 1.0f : 0.0f) + g_de;
 *   3. det = j00 (j11 j22 - j12 j21) - j01 (j10 j22 - j12 j20) + j02 (j10 j21 - j11 j20) in double, this
 *      order, unfused, from the float j; 4. rounded to float.
 * Stats (SIFT3D_AMD_JACOBIAN_STATS_BYTES of device memory, 8-byte aligned; after the call completes):
 *   bytes 0-7  : uint64 folded, the number of voxels with !(det > 0) (a NaN counts as folded);
 *   bytes 8-11 : float min, bytes 12-15: float max, of the non-NaN dets (+inf / -inf when there is none).
 * All three are order-independent, so the result does not depend on the reduction.  The buffer is
 * initialised on `stream` by the call; its content while the call runs is not the result.
 * All device entries are asynchronous on `stream`, allocate nothing, use 64-bit offsets and check their
 * arguments before any device call (-1 on NULL pointers, dims <= 0, nc < 1, m out of range, an unknown
 * interp, a non-finite A, misalignment: d_tps 16 B, d_stats 8 B, the rest 4 B; an output that overlaps
 * an input or another output). */
#define SIFT3D_AMD_JACOBIAN_STATS_BYTES 16
SIFT3D_AMD_API int sift3d_hip_affine_field(float *d_field, int ox, int oy, int oz, const double *A /*12*/,
                                           void *stream);
/* d_tps: the packed layout of "Thin-plate spline".  Launches are split as sift3d_hip_warp_tps's; the split
 * does not change any result. */
SIFT3D_AMD_API int sift3d_hip_tps_field(float *d_field, int ox, int oy, int oz, const double *A /*12*/,
                                        const float *d_tps, int m, void *stream);
/* the number of launches sift3d_hip_tps_field makes for this output grid and m (-1 for bad arguments) */
SIFT3D_AMD_API int sift3d_hip_tps_field_launches(int ox, int oy, int oz, int m);
SIFT3D_AMD_API int
sift3d_hip_warp_field(const float *d_src, int nx, int ny, int nz, int nc, const float *d_field, int ox, int oy,
                      int oz, float *d_dst, int interp, float fill, void *stream);
/* d_det [oz][oy][ox] may be NULL (stats only) */
SIFT3D_AMD_API int sift3d_hip_jacobian_det(const float *d_field, int ox, int oy, int oz, float *d_det /*NULL*/,
                                           void *d_stats, void *stream);
/* host forms, blocking; arguments are checked before the device is touched.  warp_field: host image
 * objects (nc == 1), the field on the host, shaped by dst's grid (-1 also when dst's data overlaps src's or
 * the field).  jacobian_det: a host field; det (may be NULL) and the three stats on the host (-1 also when
 * det overlaps the field). */
SIFT3D_AMD_API int sift3d_amd_image_warp_field(const sift3d_image *src, const float *field, int interp,
                                               float fill, sift3d_image *dst);
SIFT3D_AMD_API int sift3d_amd_jacobian_det(const float *field, int ox, int oy, int oz, float *det /*NULL*/,
                                           uint64_t *folded, float *min, float *max);

/* ------------------------------------------------------------------------ */
/* Cubic B-spline resampling: prefilter and 64-tap sampling                  */
/* ------------------------------------------------------------------------ */
/* LINEAR sampling is a low-pass filter: every pass blurs.  The cubic B-spline interpolant (scipy order = 3, ITK
 * BSpline) does not: the volume is first turned into B-spline coefficients, which are then sampled with the 4 x 4 x 4
 * cubic B-spline weights.  No upstream counterpart: pinned to this contract (tests/bspline_restatement.py), and
 * compared with scipy.ndimage (spline_filter / map_coordinates, order 3, mode "mirror") to a derived bound.
 *
 * 1. Coefficients (prefilter).  Per axis the coefficients c of a line s of n samples satisfy
 *      sum_k c[k] beta3(i - k) = s[i],  beta3(0) = 2/3, beta3(+-1) = 1/6,
 *    on the whole-sample mirror extension (period 2n - 2; scipy's mode "mirror").  The inverse of that filter is the
 *    two-sided exponential sqrt(3) z1^|k|, z1 = sqrt(3) - 2 = -0.2679..., truncated here to |k| <= H = 16:
 *      c[i] = acc after:  acc = +0.0f;  for k = H down to 1: acc = acc + h[k] * (s[m(i - k)] + s[m(i + k)]);
 *                         acc = acc + h[0] * s[i]                    (float, this order, unfused)
 *      m(j): j reduced into [0, 2n - 2) (mathematical modulus, so it reflects as often as needed when n <= H),
 *            then 2n - 2 - j when j >= n
 *      h[k] = (float)(sqrt(3) z1^k), the table SIFT3D_AMD_BSPLINE_TAPS below.
 *    Every c[i] is a fixed expression of the line, so the result does not depend on how a kernel tiles it.  The
 *    dropped tail is at most 2 sqrt(3) |z1|^(H+1) / (1 - |z1|) = 8.9e-10 of max|s|: a thirtieth of half a float ulp
 *    (2^-25 = 3.0e-8) of a result as large as max|s|, and still below half an ulp for results down to max|s| / 33
 *    (H = 14 leaves 1.2e-8, no margin for smaller results; the largest kept tap, h[16] = 1.2e-9, shows the size).
 *    An axis of n = 1 is skipped: its pass is the identity.  The passes run x, then y, then z; each reads the result
 *    of the one before.  (The taps sum to 1 - 2.9e-8 in float: constants are reproduced to rounding, not exactly.)
 * 2. Sample.  c [nz][ny][nx] are coefficients; q is the sample point, as in the blocks above (the affine pull map
 *    q_d = A[d][0] x + ((A[d][1] y + A[d][2] z) + A[d][3]) in double, or q_d = (double) p_d + (double) u_d(p) through
 *    a field).  Inside when 0 <= q_d <= n_d - 1 on every axis (a NaN is outside); outside voxels get `fill`.  Per axis
 *      i = floor(q), f = (float)(q - i), g = 1.0f - f, taps t_j = m(i - 1 + j), j = 0 .. 3 (m as above; n = 1: 0)
 *      w0 = ((g * g) * g) * C6             C6  = (float)(1.0 / 6.0) = 0x1.555556p-3f
 *      w1 = C23 - (0.5f * (f * f)) * (2.0f - f)      C23 = (float)(2.0 / 3.0) = 0x1.555556p-1f
 *      w2 = C23 - (0.5f * (g * g)) * (2.0f - g)
 *      w3 = ((f * f) * f) * C6
 *    dot(w, a) = ((w0 * a0 + w1 * a1) + w2 * a2) + w3 * a3 in float, unfused.  The sum runs along x for the 16
 *    (y, z) tap rows, r[jz][jy] = dot(wx, c[t_jz][t_jy][t_0..3]); then along y, s[jz] = dot(wy, r[jz][0..3]); then
 *    along z, value = dot(wz, s[0..3]).
 *    An identity map reproduces the volume only to rounding (w = (1/6, 2/3, 1/6, 0) undoes the prefilter in float),
 *    not bit for bit: unlike LINEAR there is no exact-copy promise.
 * Through a field every channel of an nc-channel coefficient image is sampled at the same point with the same taps
 * and weights, so channel c of an nc-channel resample is the single-channel resample of channel c.
 * The device entries are asynchronous on `stream`, allocate nothing, use 64-bit offsets and check their arguments
 * before any device call: -1 on NULL pointers, dims <= 0, nc < 1, a non-finite A, a buffer that is not 4-byte
 * aligned, an output (or the work buffer) that overlaps an input, the work buffer or another output.  The
 * prefilter is not in place: d_coef must not overlap d_src. */
#define SIFT3D_AMD_BSPLINE_H 16
#define SIFT3D_AMD_BSPLINE_TAPS                                                                                   \
    { 0x1.bb67aep+0f, -0x1.db3d74p-2f, 0x1.fd5c5ap-4f, -0x1.10f732p-5f, 0x1.24904cp-7f, -0x1.39919cp-9f,          \
      0x1.5014fep-11f, -0x1.68362cp-13f, 0x1.8212dap-15f, -0x1.9dcaep-17f, 0x1.bb805ep-19f, -0x1.db57eap-21f,     \
      0x1.fd78b6p-23f, -0x1.110664p-24f, 0x1.24a096p-26f, -0x1.39a31p-28f, 0x1.5027b4p-30f }
/* device scratch of sift3d_hip_bspline_prefilter: nx*ny*nz floats, one channel's volume (0 for bad dims) */
SIFT3D_AMD_API size_t sift3d_hip_bspline_work_floats(int nx, int ny, int nz);
/* d_src, d_coef [nc][nz][ny][nx]; channel by channel through d_work */
SIFT3D_AMD_API int
sift3d_hip_bspline_prefilter(const float *d_src, int nx, int ny, int nz, int nc, float *d_coef, float *d_work,
                             void *stream);
/* d_coef [nz][ny][nx] coefficients -> d_dst [oz][oy][ox] through the affine pull map A */
SIFT3D_AMD_API int
sift3d_hip_bspline_warp_affine(const float *d_coef, int nx, int ny, int nz, float *d_dst, int ox, int oy, int oz,
                               const double *A /*12*/, float fill, void *stream);
/* d_coef [nc][nz][ny][nx] coefficients -> d_dst [nc][oz][oy][ox] through the field d_field [3][oz][oy][ox] */
SIFT3D_AMD_API int
sift3d_hip_bspline_warp_field(const float *d_coef, int nx, int ny, int nz, int nc, const float *d_field, int ox,
                              int oy, int oz, float *d_dst, float fill, void *stream);
/* host forms, blocking; arguments are checked before the device is touched.  prefilter: a host volume
 * [nc][nz][ny][nx] into coef (which must not overlap it).  warp_affine / warp_field: host image objects (nc == 1)
 * holding SAMPLES; the source is prefiltered on the device, then resampled into dst's grid (the field on the host,
 * shaped by dst's grid; -1 also when dst's data overlaps src's or the field). */
SIFT3D_AMD_API int sift3d_amd_bspline_prefilter(const float *src, int nx, int ny, int nz, int nc, float *coef);
SIFT3D_AMD_API int sift3d_amd_image_bspline_warp_affine(const sift3d_image *src, const double *A, float fill,
                                                        sift3d_image *dst);
SIFT3D_AMD_API int sift3d_amd_image_bspline_warp_field(const sift3d_image *src, const float *field, float fill,
                                                       sift3d_image *dst);

/* ------------------------------------------------------------------------ */
/* Similarity measures: MSD, NCC, joint histogram, mutual information, Dice  */
/* ------------------------------------------------------------------------ */
/* How well a fixed volume F[oz][oy][ox] agrees with a moving volume M[nz][ny][nx] seen through a pull map, in one
 * gather-and-reduce pass over the fixed grid: no warped volume is written.  No upstream counterpart: PARITY UNPINNED,
 * pinned to this contract (tests/similarity_restatement.py).
 *
 * The pull map is a 3 x 4 affine, q_d = A[d][0] x + ((A[d][1] y + A[d][2] z) + A[d][3]) (double, this order, unfused:
 * "Resampling"), or a displacement field u[3][oz][oy][ox], q_d = (double) p_d + (double) u_d(p) ("Displacement
 * fields").  interp is LINEAR or NEAREST; inside test and sample are sift3d_hip_warp_affine's / _warp_field's, word
 * for word.  Per fixed voxel p:
 *   - q outside the moving grid (a NaN is outside): the voxel is skipped and does not count;
 *   - else f = F(p) and m = the sample: bit for bit what the warp entries write at p.
 * Both volumes must be finite.
 * Bins.  B = bins, 2 <= B <= SIFT3D_AMD_SIMILARITY_MAX_BINS (any B, not only powers of two), and per volume a range
 * lo < hi (finite floats).  All float, unfused:
 *     s = (float) B / (hi - lo)            once on the host (it must be finite: a range too narrow for float is refused)
 *     t = (v - lo) * s
 *     b = t < 0 ? 0 : t >= B ? B - 1 : (int) t
 * so v == hi lands in the last bin and values past either end clamp into the end bins.
 * Outputs of a call:
 *   hist [B][B] uint64, indexed [b_f][b_m]: the exact counts (integer adds: bit-exact however they are reduced);
 *   stats, SIFT3D_AMD_SIMILARITY_STATS_BYTES, 8-byte aligned:
 *     bytes 0-7 uint64 count n; then six doubles: sum f, sum m, sum f f, sum m m, sum f m, sum d d, where the products
 *     are formed in double from the floats (exact) and d = f - m is a float subtraction first (as demons' d_c).
 *     The sums are per-lane, then per-workgroup partials (one slot per workgroup of a grid of
 *     min(tiles, SIFT3D_AMD_SIMILARITY_GRID) workgroups, whatever the device; a tile is 64 x 4 x 4 voxels), then the
 *     slots in a fixed order: a call repeats its bits, and the bits depend on the shapes only.
 * Both buffers are zeroed / written on `stream` by the call itself.  Every workgroup counts in 32-bit words of its
 * own before it adds them to hist: it visits at most ceil(tiles / grid) tiles of 1024 voxels, below 2^32 voxels for
 * every grid the tiling accepts (tiles < 2^32 - 2^20), so no counter wraps.
 * The entries are asynchronous on `stream`, allocate nothing, use 64-bit offsets and check their arguments before any
 * device call: -1 on NULL pointers, dims <= 0, bins out of range, a range that is not finite, empty (lo >= hi) or so
 * narrow that s overflows, an unknown interp, a non-finite A, a misaligned buffer (hist, stats, work: 8 bytes; the
 * rest 4), an output that overlaps an input, the work buffer or another output, a grid with too many tiles.
 * d_work: sift3d_amd_similarity_work_bytes() bytes, 8-byte aligned.
 *
 * Measures (host, double).  From hist and stats, with n = count (everything NaN when n == 0):
 *   msd = S_dd / n
 *   ncc = (S_fm - S_f S_m / n) / sqrt((S_ff - S_f S_f / n) * (S_mm - S_m S_m / n)), 0 when either variance is <= 0
 *   marginals  r[i] = sum over j = 0 .. B-1 of hist[i][j], c[j] = sum over i = 0 .. B-1 of hist[i][j], in uint64
 *   N = sum over i of r[i] (uint64; equal to n for the histogram of a call)
 *   entropy H(counts) = acc after: acc = 0.0; for each count k in order, k != 0: p = (double) k / (double) N,
 *                       acc = acc - p * log(p)        (natural log, empty bins skipped)
 *   H_f = H(r[0 .. B-1]), H_m = H(c[0 .. B-1]), H_fm = H(hist in row-major order)
 *   mi = (H_f + H_m) - H_fm,  nmi = (H_f + H_m) / H_fm, 0 when H_fm is 0.
 * Label overlap needs no kernel of its own: with NEAREST, lo = 0, hi = L, B = L, s is exactly 1 and hist is the
 * confusion matrix of the integer labels 0 .. L-1 (fixed label = row).  For label k, row_k = r[k], col_k = c[k]:
 *   dice_k = 2 h_kk / (row_k + col_k), jaccard_k = h_kk / (row_k + col_k - h_kk): the integers exactly, one double
 *   division each, NaN for a label absent from both; vol_f[k] = row_k, vol_m[k] = col_k. */
#define SIFT3D_AMD_SIMILARITY_MAX_BINS 128
#define SIFT3D_AMD_SIMILARITY_GRID 2048            /* workgroups (and partial slots) of a call, at most */
#define SIFT3D_AMD_SIMILARITY_STATS_BYTES 56
typedef struct {
    uint64_t n;
    double msd, ncc, mi, nmi, entropy_fixed, entropy_moving, entropy_joint;
} sift3d_amd_similarity;
/* bytes of d_work for a call with these arguments (0 for dims <= 0 or bins out of range) */
SIFT3D_AMD_API size_t sift3d_amd_similarity_work_bytes(int ox, int oy, int oz, int bins);
/* d_F [oz][oy][ox], d_M [nz][ny][nx], d_hist [bins][bins] uint64, d_stats the record above */
SIFT3D_AMD_API int
sift3d_hip_similarity_affine(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                             const double *A /*12*/, int interp, int bins, float lo_f, float hi_f, float lo_m,
                             float hi_m, uint64_t *d_hist, void *d_stats, void *d_work, void *stream);
/* d_field [3][oz][oy][ox] */
SIFT3D_AMD_API int
sift3d_hip_similarity_field(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                            const float *d_field, int interp, int bins, float lo_f, float hi_f, float lo_m,
                            float hi_m, uint64_t *d_hist, void *d_stats, void *d_work, void *stream);
/* host only: hist [bins][bins] and the stats record, both on the host.  -1 on NULL pointers or bins out of range. */
SIFT3D_AMD_API int
sift3d_amd_similarity_measures(const uint64_t *hist, int bins, const void *stats, sift3d_amd_similarity *out);
/* host only: hist [L][L] a confusion matrix, 1 <= L <= SIFT3D_AMD_SIMILARITY_MAX_BINS; dice, jaccard (double [L])
 * and vol_f, vol_m (uint64 [L]) may each be NULL.  -1 on a NULL hist or L out of range. */
SIFT3D_AMD_API int
sift3d_amd_label_overlap(const uint64_t *hist, int L, double *dice, double *jaccard, uint64_t *vol_f,
                         uint64_t *vol_m);

/* ------------------------------------------------------------------------ */
/* Intensity-driven affine refinement: Gauss-Newton on the MSD               */
/* ------------------------------------------------------------------------ */
/* Moves a 3 x 4 affine pull map towards a smaller mean squared difference between a fixed volume F[oz][oy][ox] and a
 * moving volume M[nz][ny][nx] seen through it: the normal equations of a Gauss-Newton step in one gather-and-reduce
 * pass on the device, the damped (Levenberg-Marquardt) solve and the update on the host, and a driver that iterates
 * them, optionally coarse to fine.  No upstream counterpart: PARITY UNPINNED, pinned to this contract and its numpy
 * restatement (tests/affine_refine_restatement.py).
 *
 * Sample with gradient.  Pull map, inside test and LINEAR sample are "Similarity measures"' / "Resampling"'s, word for
 * word: a voxel p whose q falls outside the moving grid (a NaN is outside) is skipped and not counted, and m is what
 * sift3d_hip_warp_affine writes at p, bit for bit.  With a, b the values at ix, jx of the corner rows 00, 10, 01, 11
 * (y then z), c.. = lerp(a.., b.., fx) and lerp(a, b, f) = a + f * (b - a), all float, unfused:
 *     gx = lerp(lerp(b00 - a00, b10 - a10, fy), lerp(b01 - a01, b11 - a11, fy), fz)
 *     gy = lerp(c10 - c00, c11 - c01, fz)
 *     gz = lerp(c01, c11, fy) - lerp(c00, c10, fy)
 * the derivative of the trilinear interpolant from the eight values the sample reads.  On a clamped last plane
 * (j == i: q on the high face of the grid, or an axis of 1) the difference along that axis is 0.
 *
 * Normal equations (sift3d_hip_affine_normal_eqs).  The 12 parameters are centred on the fixed grid,
 * c = ((ox - 1) / 2, (oy - 1) / 2, (oz - 1) / 2) (exact in double): q = L (p - c) + t, parameter 4 d + j is L[d][j]
 * for j < 3 and t[d] for j = 3, and P = (x - cx, y - cy, z - cz, 1).  The centring keeps the 12 x 12 system well
 * scaled.  Per counted voxel e = m - f (a float subtraction), and in double E = e, G_d = g_d, J[4 d + j] = G_d P_j.
 * The record, SIFT3D_AMD_AFFINE_NORMAL_BYTES, 8-byte aligned:
 *     uint64 n;  double S_ee = sum E E;  double b[12] = sum J E;  double H[12][12] = sum J J^T,
 * H stored in full and symmetric bit for bit.  Only the 60 distinct values of H (6 pairs G_d G_e x 10 pairs P_j P_k)
 * and the 12 of b are summed; how a term is factored and in which order the terms are added is the
 * implementation's (every term carries at most 8 roundings), but it is a function of the shapes only: per-lane
 * sums, per-workgroup partials (one slot per workgroup of a grid of min(tiles, SIFT3D_AMD_SIMILARITY_GRID)
 * workgroups, whatever the device), then the slots in a fixed order.  A call repeats its bytes on any device.  S_ee
 * is the similarity record's sum d d up to the order of the sum.  The whole record is written on `stream` by the call;
 * n == 0 leaves it all zero.
 * The entry is asynchronous on `stream`, allocates nothing, uses 64-bit offsets and checks its arguments before any
 * device call: -1 on NULL pointers, dims <= 0, a non-finite A, a misaligned buffer (record, work: 8 bytes; the rest
 * 4), an output that overlaps an input, the work buffer or another output, a grid with too many tiles.
 * d_work: sift3d_amd_affine_normal_work_bytes() bytes, 8-byte aligned.
 *
 * LM step (sift3d_amd_affine_lm_step, host, double).  Bit 4 d + j of free_mask frees parameter (d, j); 0xFFF is the
 * full affine, 0x888 the translation.  On the free set, K = H + lambda diag(H) (K_ii = H_ii + lambda * H_ii),
 * K delta = -b by Cholesky (K = C C^T row by row, then the two triangular solves); the other entries of delta are 0.
 * -1 when n == 0, the mask is empty or has bits past 0xFFF, lambda is negative or not finite, or K is not positive
 * definite (a free parameter with H_ii == 0 makes it so); delta is then all zero.
 *
 * Update (sift3d_amd_affine_apply_delta, host, double, unfused), per row d with L = A[d][0..2]:
 *     t   = A[d][3] + ((L[0] * cx + L[1] * cy) + L[2] * cz)
 *     L'[j] = L[j] + delta[4 d + j]
 *     A_out[d] = [ L' | (t + delta[4 d + 3]) - ((L'[0] * cx + L'[1] * cy) + L'[2] * cz) ]
 *
 * Driver (sift3d_amd_affine_refine_device).  Per level, with lambda = lambda0:
 *   1. evaluate at A (record r, n_first = r.n);
 *   2. delta = lm_step(r, free_mask, lambda), A' = apply_delta(A, delta), evaluate at A' (record r');
 *   3. accept when n' >= min_overlap * n_first and S_ee' / n' < S_ee / n.  Accepted: A = A', r = r' (the evaluation is
 *      the next iteration's record), lambda = max(lambda / lambda_factor, lambda_min).  Rejected: lambda = lambda *
 *      lambda_factor;
 *   4. stop when an accepted step moved no corner of the fixed grid by tol voxels or more (CONVERGED; the distance
 *      |A' p - A p| over the 8 corners p), when lambda > lambda_max (LAMBDA), when the level has made max_evaluations
 *      evaluations (EVALUATIONS), or when the LM step fails or gives a map that is not finite (LM_FAILED); else 2.
 * Each iteration therefore costs one kernel pass and one copy of the 1.2 KB record to the host with a wait for the
 * stream: the host decides the next step, the same trade as sift3d_amd_field_exp_device's single wait.
 * Levels: level 0 is the given pair; level l's volumes are sift3d_hip_restrict2 (scale 1) of level l - 1's, fixed and
 * moving, held in d_work.  Coarse voxel i is fine voxel 2 i, so going down a level halves A[:][3] and going up doubles
 * it; the linear part is unchanged.  The coarsest level runs first.
 * The result holds the final A (also written to A_io), one entry per evaluation in the order run (MSD = S_ee / n, NaN
 * when n == 0; n; the lambda of the step that led to it; accepted, 1 for a level's first; the level), their number
 * (at most levels * max_evaluations) and the stop reason of level 0.  params == NULL takes the defaults.  Once the
 * arguments have passed the checks the result is valid whatever the call returns (no evaluations, A as given, when
 * a device call fails before the first).
 * -1 before any device call on NULL pointers, dims <= 0, a non-finite A, free_mask outside [1, 0xFFF], levels outside
 * [1, SIFT3D_AMD_DEMONS_MAX_LEVELS], max_evaluations outside [1, SIFT3D_AMD_AFFINE_MAX_EVALUATIONS], lambda0,
 * lambda_min <= 0, lambda_factor <= 1, lambda_max < lambda0, tol < 0, min_overlap outside [0, 1] (or any of them not
 * finite), misalignment (d_work 8 B, the volumes 4 B), a work buffer that overlaps a volume.
 * d_work: sift3d_amd_affine_refine_work_bytes() bytes. */
#define SIFT3D_AMD_AFFINE_NORMAL_BYTES 1264        /* 8 + 8 + 12 * 8 + 144 * 8 */
#define SIFT3D_AMD_AFFINE_MAX_EVALUATIONS 128      /* per level */
#define SIFT3D_AMD_AFFINE_MAX_TRAIL (6 * SIFT3D_AMD_AFFINE_MAX_EVALUATIONS)    /* SIFT3D_AMD_DEMONS_MAX_LEVELS levels */
#define SIFT3D_AMD_AFFINE_FREE_ALL 0xFFFu
#define SIFT3D_AMD_AFFINE_FREE_TRANSLATION 0x888u
#define SIFT3D_AMD_AFFINE_STOP_CONVERGED 0
#define SIFT3D_AMD_AFFINE_STOP_LAMBDA 1
#define SIFT3D_AMD_AFFINE_STOP_EVALUATIONS 2
#define SIFT3D_AMD_AFFINE_STOP_LM_FAILED 3
typedef struct {
    unsigned free_mask;        /* 0xFFF */
    int levels;                /* 1 */
    int max_evaluations;       /* 30, per level */
    double lambda0;            /* 1e-3: the damping a level starts with */
    double lambda_factor;      /* 10: lambda goes down by it on an accepted step, up on a rejected one */
    double lambda_min;         /* 1e-9: floor */
    double lambda_max;         /* 1e7: stop above it */
    double tol;                /* 1e-3 voxels */
    double min_overlap;        /* 0.5 of the level's first count */
} sift3d_amd_affine_refine_params;
typedef struct {
    double msd;
    uint64_t n;
    double lambda;
    int accepted, level;
} sift3d_amd_affine_evaluation;
typedef struct {
    double A[12];
    int evaluations, stop;
    sift3d_amd_affine_evaluation trail[SIFT3D_AMD_AFFINE_MAX_TRAIL];
} sift3d_amd_affine_refine_result;
/* bytes of d_work for sift3d_hip_affine_normal_eqs on this fixed grid (0 for dims <= 0) */
SIFT3D_AMD_API size_t sift3d_amd_affine_normal_work_bytes(int ox, int oy, int oz);
/* d_F [oz][oy][ox], d_M [nz][ny][nx], d_record the record above */
SIFT3D_AMD_API int
sift3d_hip_affine_normal_eqs(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                             const double *A /*12*/, void *d_record, void *d_work, void *stream);
/* host only: record on the host */
SIFT3D_AMD_API int
sift3d_amd_affine_lm_step(const void *record, unsigned free_mask, double lambda, double *delta /*12*/);
/* host only: (ox, oy, oz) is the fixed grid; A_out may be A */
SIFT3D_AMD_API int
sift3d_amd_affine_apply_delta(const double *A /*12*/, const double *delta /*12*/, int ox, int oy, int oz,
                              double *A_out /*12*/);
SIFT3D_AMD_API void sift3d_amd_affine_refine_default_params(sift3d_amd_affine_refine_params *p);
/* for bindings that restate the layouts: sizeof the params (0), evaluation (1) and result (2) structs, then
 * SIFT3D_AMD_AFFINE_NORMAL_BYTES (3), SIFT3D_AMD_AFFINE_MAX_EVALUATIONS (4), the most levels (5); 0 otherwise */
SIFT3D_AMD_API size_t sift3d_amd_affine_refine_struct_bytes(int which);
/* bytes of d_work for the driver (0 for bad arguments) */
SIFT3D_AMD_API size_t
sift3d_amd_affine_refine_work_bytes(int ox, int oy, int oz, int nx, int ny, int nz, int levels);
/* A_io [12] on the host, in / out; waits for `stream` once per evaluation */
SIFT3D_AMD_API int
sift3d_amd_affine_refine_device(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                double *A_io, const sift3d_amd_affine_refine_params *params,
                                sift3d_amd_affine_refine_result *result, void *d_work, void *stream);

/* ------------------------------------------------------------------------ */
/* B-spline free-form deformation: an intensity-driven control lattice       */
/* ------------------------------------------------------------------------ */
/* A cubic B-spline free-form deformation (FFD) of the fixed grid, driven by the mean squared difference between a
 * fixed volume F[oz][oy][ox] and a moving volume M[nz][ny][nx], with an explicit bending-energy penalty.  No upstream
 * counterpart: PARITY UNPINNED, pinned to this contract and its numpy restatement (tests/ffd_restatement.py).
 *
 * Lattice.  c[3][gz][gy][gx] float32, channels x, y, z in voxels of the fixed grid, a pull map like every field.  The
 * spacing delta = (dx, dy, dz) is integer, 1 <= delta <= SIFT3D_AMD_FFD_MAX_SPACING.  Along an axis of o voxels control
 * i sits at voxel (i - 1) * delta and g = (o - 1) / delta + 4 (integer division; sift3d_amd_ffd_lattice_dim).  Voxel x
 * has i0 = x / delta, r = x % delta and the four weights w[r][0..3] on the controls i0 .. i0 + 3.  The table w[delta][4]
 * (sift3d_amd_ffd_weights, host) is made in double and rounded to float, with t = (double) r / (double) delta,
 * u = 1.0 - t, t2 = t * t, t3 = t2 * t, every operation in this order and unfused:
 *     w[r][0] = (float)(((u * u) * u) / 6.0)
 *     w[r][1] = (float)(((3.0 * t3 - 6.0 * t2) + 4.0) / 6.0)
 *     w[r][2] = (float)((((-3.0 * t3 + 3.0 * t2) + 3.0 * t) + 1.0) / 6.0)
 *     w[r][3] = (float)(t3 / 6.0)
 *
 * Spline value.  s_d(p) = sum_c sum_b sum_a wz[c] * (wy[b] * (wx[a] * c_d[k0 + c][j0 + b][i0 + a])), float, unfused:
 * s starts at +0 and takes the 64 terms one by one, c outermost, then b, then a (x innermost), each term the three
 * multiplications in the order written.
 *
 * Field export (sift3d_hip_ffd_field) writes d_field[3][oz][oy][ox].  With A (a 3 x 4 pull map)
 *     field_d(p) = (float)(pull_d(A, p) - (double) p_d) + s_d(p)            (a float addition),
 * pull "Resampling"'s, word for word, so the first operand is sift3d_hip_affine_field's value; without A (NULL)
 * field_d = s_d.  The result is an ordinary field: sift3d_hip_warp_field, sift3d_hip_jacobian_det, the similarity,
 * cubic resampling, composition and inversion entries take it unchanged.  d_work: sift3d_amd_ffd_field_work_bytes()
 * bytes, 16-byte aligned (the weight tables, copied there by the call).
 *
 * Evaluation (sift3d_hip_ffd_evaluate) exports the field of the lattice to d_field, then per fixed voxel p with
 * u = field(p): the inside test and LINEAR sample m are sift3d_hip_warp_field's, bit for bit; e = m - f (a float
 * subtraction); g = the gradient of the sample, as in "Intensity-driven affine refinement"; a voxel that is not inside
 * adds nothing.  In double E = e, G_d = g_d.  The record, sift3d_amd_ffd_record_bytes() bytes, 8-byte aligned:
 *     uint64 n;  double S_ee = sum E E;  double R;  double gmax;                        (the head, 32 bytes)
 *     double Gc[3][gz][gy][gx] = sum_p W(p; k, j, i) E G_d;  double dR[3][gz][gy][gx] = dR / dc
 * W(p; k, j, i) is the product of the float weights of p on control (k, j, i) along x, y and z, widened to double:
 * Gc is the adjoint of the spline evaluation applied to the force E G.  How the sum is organised is the
 * implementation's (here: the force E G_d, exact in double, then one pass per axis, z, y, x, each
 * sum_x (double) w * v in ascending x), but it is a function of the shapes only, without atomics, every partial slot
 * reduced in a fixed order: a call repeats its bytes.  Every entry of Gc is within gamma_(k + 8) sum |term| of the
 * exact sum in double (u = 2^-53), k the number of voxels in the control's support.
 * Bending energy, on the lattice, over the N = (gx - 2)(gy - 2)(gz - 2) controls that have all 26 neighbours: for
 * each channel the six second derivatives of the spline at the control's own position by the stencils value
 * (1/6, 4/6, 1/6), first derivative (-1/2, 0, 1/2) / delta and second derivative (1, -2, 1) / delta^2 per axis (double:
 * 1.0 / 6.0, 4.0 / 6.0, -0.5 / d, 0.5 / d, 1.0 / (d * d), -2.0 / (d * d)), the coefficient of neighbour (a, b, c)
 * being (sz[c] * sy[b]) * sx[a] and the 27 products added in ascending (c, b, a), and
 *     R = (1 / N) sum (s_xx^2 + s_yy^2 + s_zz^2 + 2 s_xy^2 + 2 s_xz^2 + 2 s_yz^2),
 * dR / dc the exact adjoint of the same stencils, (2 / N) sum m_t coef_t s_t.  A lattice sampled from an affine
 * function has R = 0 in exact arithmetic.  sift3d_hip_ffd_bending writes R and dR alone into a record (n, S_ee, gmax and
 * Gc are left untouched).
 * Cost and gradient: E = S_ee / n + bending * R; d_grad[3][gz][gy][gx] = (float)((2.0 / n) * Gc + bending * dR), formed
 * in double; gmax = the largest |d_grad| as stored.  n == 0 makes E and the gradient NaN.
 *
 * Subdivision (sift3d_hip_ffd_refine2) takes the lattice over the grid o_c = (o + 1) / 2 at spacing delta to the
 * lattice over o at the same delta, the displacements doubled.  Per axis, fine j = 2 i - 1 takes
 * ((c[i - 1] + 6 c[i]) + c[i + 1]) * 0.125 and fine j = 2 i takes (c[i] + c[i + 1]) * 0.5; x first, then y, then z, then
 * * 2, all float.  The largest coarse index needed is floor(floor((o - 1) / delta) / 2) + 3 = g_c - 1.
 *
 * Driver (sift3d_amd_ffd_refine_device), steepest descent with a step measured in voxels.  Level l's volumes are
 * sift3d_hip_restrict2 (scale 1) of level l - 1's, held in d_work; A[:][3] is halved going down a level and doubled
 * going up; the spacing is the same on every level; the coarsest level runs first from a zero lattice, every other
 * from the subdivision of the coarser level's.  Per level, with s = step0:
 *   1. evaluate at c (E, n_first = n; trail entry with accepted = 1).  A non-finite E stops the level (FAILED);
 *   2. stop when the level has made max_evaluations evaluations (EVALUATIONS) or gmax == 0 (FLAT); else
 *      c' = c - (float)(s / gmax) * grad (float, unfused) and evaluate at c' (E');
 *   3. a non-finite E' stops the level (FAILED).  Accept when n' >= min_overlap * n_first and E' < E: c = c', the
 *      evaluation is the next iteration's, s = min(2 s, step_max).  Otherwise s = s / 2;
 *   4. stop when s < tol (CONVERGED); else 2.
 * Each evaluation waits for the stream once, for the 32-byte head; the lattices never leave the device.  The result
 * holds one entry per evaluation in the order run (E, MSD = S_ee / n, R, n, the step s that led to it, accepted, level),
 * their number and the stop reason of level 0.  d_lattice receives the final lattice of level 0 and d_field its field
 * (through A when given).  params == NULL takes the defaults.
 *
 * The device entries are asynchronous on `stream` (the driver waits as said), allocate nothing, use 64-bit offsets and
 * check every argument before any device call: -1 on NULL pointers (A may be NULL), dims <= 0, a spacing outside
 * [1, SIFT3D_AMD_FFD_MAX_SPACING], a lattice shape that is not g, a non-finite A, a bending weight that is negative or
 * not finite, misalignment (records 8 bytes, work buffers 16, the rest 4), an output that overlaps an input, the work
 * buffer or another output, levels outside [1, SIFT3D_AMD_DEMONS_MAX_LEVELS], max_evaluations outside
 * [1, SIFT3D_AMD_FFD_MAX_EVALUATIONS], step0 <= 0, step_max < step0, tol <= 0, min_overlap outside [0, 1]. */
#define SIFT3D_AMD_FFD_MAX_SPACING 256
#define SIFT3D_AMD_FFD_MAX_EVALUATIONS 128         /* per level */
#define SIFT3D_AMD_FFD_MAX_TRAIL (6 * SIFT3D_AMD_FFD_MAX_EVALUATIONS)          /* SIFT3D_AMD_DEMONS_MAX_LEVELS levels */
#define SIFT3D_AMD_FFD_RECORD_HEAD_BYTES 32
#define SIFT3D_AMD_FFD_STOP_CONVERGED 0
#define SIFT3D_AMD_FFD_STOP_EVALUATIONS 1
#define SIFT3D_AMD_FFD_STOP_FLAT 2
#define SIFT3D_AMD_FFD_STOP_FAILED 3
typedef struct {
    int spacing[3];            /* 8, 8, 8: dx, dy, dz */
    int levels;                /* 3 */
    int max_evaluations;       /* 60, per level */
    double bending;            /* 0.005 */
    double step0;              /* 1 voxel: the largest control displacement of a level's first step */
    double step_max;           /* 4 voxels */
    double tol;                /* 0.01 voxels */
    double min_overlap;        /* 0.5 of the level's first count */
} sift3d_amd_ffd_refine_params;
typedef struct {
    double E, msd, R;
    uint64_t n;
    double step;
    int accepted, level;
} sift3d_amd_ffd_evaluation;
typedef struct {
    int evaluations, stop;
    sift3d_amd_ffd_evaluation trail[SIFT3D_AMD_FFD_MAX_TRAIL];
} sift3d_amd_ffd_refine_result;
/* host only: g of an axis (0 for o <= 0 or delta <= 0); the table w[delta][4] (-1 on NULL or a spacing out of range) */
SIFT3D_AMD_API int sift3d_amd_ffd_lattice_dim(int o, int delta);
SIFT3D_AMD_API int sift3d_amd_ffd_weights(int delta, float *w);
/* bytes of the buffers below; 0 for bad arguments */
SIFT3D_AMD_API size_t sift3d_amd_ffd_field_work_bytes(int dx, int dy, int dz);
SIFT3D_AMD_API size_t sift3d_amd_ffd_record_bytes(int gx, int gy, int gz);
SIFT3D_AMD_API size_t sift3d_amd_ffd_evaluate_work_bytes(int ox, int oy, int oz, int dx, int dy, int dz);
SIFT3D_AMD_API size_t sift3d_amd_ffd_bending_work_bytes(int gx, int gy, int gz);
SIFT3D_AMD_API size_t
sift3d_amd_ffd_refine_work_bytes(int ox, int oy, int oz, int nx, int ny, int nz, int dx, int dy, int dz, int levels);
SIFT3D_AMD_API int
sift3d_hip_ffd_field(const float *d_lattice, int gx, int gy, int gz, int dx, int dy, int dz,
                     const double *A /*12 or NULL*/, int ox, int oy, int oz, float *d_field, void *d_work, void *stream);
SIFT3D_AMD_API int
sift3d_hip_ffd_evaluate(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                        const float *d_lattice, int gx, int gy, int gz, int dx, int dy, int dz,
                        const double *A /*12 or NULL*/, double bending, float *d_field, void *d_record, float *d_grad,
                        void *d_work, void *stream);
SIFT3D_AMD_API int
sift3d_hip_ffd_bending(const float *d_lattice, int gx, int gy, int gz, int dx, int dy, int dz, void *d_record,
                       void *d_work, void *stream);
/* (ox, oy, oz) is the FINE grid; d_coarse is the lattice over ((ox + 1) / 2, (oy + 1) / 2, (oz + 1) / 2) */
SIFT3D_AMD_API int
sift3d_hip_ffd_refine2(const float *d_coarse, int ox, int oy, int oz, int dx, int dy, int dz, float *d_fine,
                       void *stream);
SIFT3D_AMD_API void sift3d_amd_ffd_refine_default_params(sift3d_amd_ffd_refine_params *p);
/* for bindings that restate the layouts: sizeof the params (0), evaluation (1) and result (2) structs, then
 * SIFT3D_AMD_FFD_RECORD_HEAD_BYTES (3), SIFT3D_AMD_FFD_MAX_EVALUATIONS (4), the most levels (5),
 * SIFT3D_AMD_FFD_MAX_SPACING (6); 0 otherwise */
SIFT3D_AMD_API size_t sift3d_amd_ffd_refine_struct_bytes(int which);
/* A [12] on the host or NULL (the identity); waits for `stream` once per evaluation and once at the end */
SIFT3D_AMD_API int
sift3d_amd_ffd_refine_device(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                             const double *A, const sift3d_amd_ffd_refine_params *params,
                             sift3d_amd_ffd_refine_result *result, float *d_lattice, float *d_field, void *d_work,
                             void *stream);

/* ------------------------------------------------------------------------ */
/* Masks: regions of interest for similarity, affine and FFD refinement      */
/* ------------------------------------------------------------------------ */
/* Which fixed voxels the three intensity-driven stages above count.  Each `_masked` entry below is its unmasked
 * counterpart with two more arguments, d_WF and d_WM, at the end; this section is the one place the rule is stated.
 *
 * A mask is a float32 volume on the grid it belongs to: the fixed mask W_F[oz][oy][ox], the moving mask
 * W_M[nz][ny][nx].  Either may be NULL: all in.  A mask voxel is IN when w >= 0.5f, one float compare: a NaN, a negative
 * value and nextafterf(0.5f, 0) are out; 0.5f, 1, 2 and +inf are in; a binary 0 / 1 mask behaves as expected.  The same
 * test holds at every pyramid level.  Weighted (soft) masks are not provided.
 *
 * A fixed voxel p is counted only when all three hold:
 *   - its q is inside the moving grid (the unmasked sections' test, word for word);
 *   - W_F(p) is in;
 *   - W_M sampled at q is in.  The sample is "Resampling"'s NEAREST rule, the voxel at floor(q + 0.5) per axis (double),
 *     of the same q that drives the intensity sample, whatever interpolation that sample uses.
 * A masked-out voxel is treated exactly like a voxel whose q is outside: it is skipped, adds nothing to the count, the
 * sums or the histogram, and the FFD force written at it is 0.  Mask values need not be finite; the volumes must be, as
 * before, masked-out voxels included (they are read).  Binning, the sums, the partial slots, the order of the
 * reductions and the record layouts are those of the unmasked sections, word for word: a masked call repeats its
 * bytes, and they depend on the shapes and the inputs only.  With both masks NULL, or both all in, every masked entry
 * writes the same bytes as its unmasked counterpart.
 *
 * Levels (the two drivers): level l's masks are sift3d_hip_restrict2 (scale 1) of level l - 1's masks - always the
 * float mask of the level above, never a thresholded copy - held in d_work beside the restricted volumes (per level:
 * fixed, moving, then the fixed mask and the moving mask where given).  min_overlap compares counts of counted
 * voxels.  Params and result structs are the unmasked drivers'.
 *
 * Arguments are checked before any device call as in the unmasked entries, and in addition: a non-NULL mask must be
 * 4-byte aligned and must not overlap any output or the work buffer; -1 otherwise.  The masked drivers need
 * sift3d_amd_*_refine_masked_work_bytes() bytes of d_work (never less than the unmasked figure; 0 for bad arguments),
 * whether or not a mask is NULL. */
SIFT3D_AMD_API int
sift3d_hip_similarity_affine_masked(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                    const double *A /*12*/, int interp, int bins, float lo_f, float hi_f, float lo_m,
                                    float hi_m, uint64_t *d_hist, void *d_stats, void *d_work, void *stream,
                                    const float *d_WF, const float *d_WM);
SIFT3D_AMD_API int
sift3d_hip_similarity_field_masked(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                   const float *d_field, int interp, int bins, float lo_f, float hi_f, float lo_m,
                                   float hi_m, uint64_t *d_hist, void *d_stats, void *d_work, void *stream,
                                   const float *d_WF, const float *d_WM);
SIFT3D_AMD_API int
sift3d_hip_affine_normal_eqs_masked(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                    const double *A /*12*/, void *d_record, void *d_work, void *stream,
                                    const float *d_WF, const float *d_WM);
SIFT3D_AMD_API size_t
sift3d_amd_affine_refine_masked_work_bytes(int ox, int oy, int oz, int nx, int ny, int nz, int levels);
SIFT3D_AMD_API int
sift3d_amd_affine_refine_masked_device(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny,
                                       int nz, double *A_io, const sift3d_amd_affine_refine_params *params,
                                       sift3d_amd_affine_refine_result *result, void *d_work, void *stream,
                                       const float *d_WF, const float *d_WM);
SIFT3D_AMD_API int
sift3d_hip_ffd_evaluate_masked(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                               const float *d_lattice, int gx, int gy, int gz, int dx, int dy, int dz,
                               const double *A /*12 or NULL*/, double bending, float *d_field, void *d_record,
                               float *d_grad, void *d_work, void *stream, const float *d_WF, const float *d_WM);
SIFT3D_AMD_API size_t
sift3d_amd_ffd_refine_masked_work_bytes(int ox, int oy, int oz, int nx, int ny, int nz, int dx, int dy, int dz,
                                        int levels);
SIFT3D_AMD_API int
sift3d_amd_ffd_refine_masked_device(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                    const double *A, const sift3d_amd_ffd_refine_params *params,
                                    sift3d_amd_ffd_refine_result *result, float *d_lattice, float *d_field,
                                    void *d_work, void *stream, const float *d_WF, const float *d_WM);

/* ------------------------------------------------------------------------ */
/* Affine refinement under a linear intensity map (NCC)                      */
/* ------------------------------------------------------------------------ */
/* "Intensity-driven affine refinement" with a linear intensity map fitted together with the pull map:
 *     minimise over A, alpha, beta:   sum over counted p of (alpha * m_A(p) + beta - f(p))^2
 * The MSD is meaningful only when both volumes share one intensity scale; this cost does not change under any gain
 * (negative ones included) or offset of either volume.  For a fixed A the best (alpha, beta) is the regression of f on
 * m and the residual is V_f (1 - ncc^2), so this is Gauss-Newton on 1 - ncc^2.  Every sum that the 14-parameter normal
 * equations need is free of alpha and beta: one gather-and-reduce pass per evaluation, as for the MSD.  No upstream
 * counterpart: PARITY UNPINNED, pinned to this contract and its numpy restatement (tests/affine_ncc_restatement.py).
 *
 * The pull map, the inside test, the LINEAR sample m, its gradient g, the centring c, P and J[4 d + j] = G_d P_j are
 * those of "Intensity-driven affine refinement", word for word; d_WF and d_WM are "Masks"' masks, word for word, and
 * either may be NULL.  Per counted voxel, in double: f = F(p), m the sample, G_d = g_d (floats widened; every product of
 * two of them is exact).
 *
 * The record (sift3d_hip_affine_ncc_normal_eqs), SIFT3D_AMD_AFFINE_NCC_BYTES, 8-byte aligned:
 *     uint64 n;
 *     double S_m = sum m, S_f = sum f, S_mm = sum m m, S_fm = sum f m, S_ff = sum f f;
 *     double u[12] = sum J;   double v[12] = sum J m;   double w[12] = sum J f;
 *     double H[12][12] = sum J J^T,
 * H stored in full and symmetric bit for bit: 60 + 36 + 5 = 101 summed doubles and the count.  The rules are the MSD
 * record's: how a term is factored and in which order the terms are added is the implementation's (every term carries
 * at most 8 roundings), but it is a function of the shapes only: per-lane sums, per-workgroup partials (one slot per
 * workgroup of a grid of min(tiles, SIFT3D_AMD_SIMILARITY_GRID) workgroups, whatever the device), then the slots in a
 * fixed order.  A call repeats its bytes on any device.  (This implementation sums H as sift3d_hip_affine_normal_eqs
 * does, operation for operation: the two H agree bit for bit.  The five moments are the similarity record's up to the
 * order of the sums.)  The whole record is written on `stream` by the call; n == 0 leaves it all zero.
 * The entry is asynchronous on `stream`, allocates nothing, uses 64-bit offsets and checks its arguments before any
 * device call: -1 on NULL pointers (but the masks), dims <= 0, a non-finite A, a misaligned buffer (record, work: 8
 * bytes; the rest 4), an output that overlaps an input, a mask, the work buffer or another output, a grid with too many
 * tiles.  d_work: sift3d_amd_affine_ncc_normal_work_bytes() bytes, 8-byte aligned.
 *
 * Fit (sift3d_amd_affine_ncc_fit, host, double, in this order, unfused):
 *     nd = (double) n;  V_m = S_mm - S_m * S_m / nd;  V_f = S_ff - S_f * S_f / nd;  C = S_fm - S_f * S_m / nd
 * The fit is defined when n >= 2 and V_m > 0.  Then
 *     alpha = C / V_m;  beta = (S_f - alpha * S_m) / nd;  cost = max((V_f - alpha * C) / nd, 0)
 *     ncc   = C / sqrt(V_f * V_m), 0 when V_f <= 0           ("Similarity measures"' formula on these sums)
 * out = (alpha, beta, cost, ncc).  -1 on a NULL pointer or an undefined fit; out is all NaN when the fit is undefined.
 *
 * Step (sift3d_amd_affine_ncc_lm_step, host, double).  The 14 parameters are the 12 of the pull map, then alpha (12) and
 * beta (13); the system is built at (alpha, beta) of the fit:
 *     H14[i][j] = (alpha * alpha) * H[i][j]      H14[i][12] = alpha * v[i]      H14[i][13] = alpha * u[i]
 *     H14[12][12] = S_mm    H14[12][13] = S_m    H14[13][13] = nd
 *     b14[i] = alpha * ((alpha * v[i] + beta * u[i]) - w[i])
 *     b14[12] = (alpha * S_mm + beta * S_m) - S_fm      b14[13] = (alpha * S_m + beta * nd) - S_f
 * (i, j < 12; H14 symmetric).  The free set is the bits of free_mask plus parameters 12 and 13, which are always free.
 * K = H14 + lambda diag(H14) (K_ii = H14_ii + lambda * H14_ii) on the free set, K delta14 = -b14 by the Cholesky
 * factorisation and the two triangular solves of sift3d_amd_affine_lm_step (one routine); delta is the first 12 entries
 * of delta14, 0 outside the free set.  -1, with delta all zero, on that step's refusals (NULL pointers, an empty mask
 * or bits past 0xFFF, lambda negative or not finite), on an undefined fit (n < 2 included), and when K is not positive
 * definite (alpha == 0 makes it so).  The update is sift3d_amd_affine_apply_delta.
 *
 * Driver (sift3d_amd_affine_ncc_refine_device).  sift3d_amd_affine_refine_device's loop, levels (sift3d_hip_restrict2 of
 * volumes and masks, the translation halved and doubled) and stop reasons, one loop in the code too, with `cost` of the
 * fit in the place of S_ee / n.  An evaluation whose fit is undefined has no cost: as a trial it is rejected, and as a
 * level's first evaluation it stops the level with LM_FAILED (the step refuses).  Params and result are
 * sift3d_amd_affine_refine_params and sift3d_amd_affine_refine_result as they are; the trail's `msd` field carries
 * `cost` (NaN where undefined).  fit_out = (alpha, beta, cost, ncc) of the fit at the final A on level 0, all NaN where
 * that is undefined or no evaluation was made.  Checks, alignment, overlap rules, asynchrony and "allocates nothing"
 * are the masked MSD driver's, and fit_out must not be NULL.
 * d_work: sift3d_amd_affine_ncc_refine_work_bytes() bytes, whether or not a mask is NULL: the partial slots, the record
 * rounded up to 16 bytes, then the levels as in the masked MSD driver. */
#define SIFT3D_AMD_AFFINE_NCC_BYTES 1488           /* 8 + 5 * 8 + 3 * 12 * 8 + 144 * 8 */
/* bytes of d_work for sift3d_hip_affine_ncc_normal_eqs on this fixed grid (0 for dims <= 0) */
SIFT3D_AMD_API size_t sift3d_amd_affine_ncc_normal_work_bytes(int ox, int oy, int oz);
/* d_F [oz][oy][ox], d_M [nz][ny][nx], d_record the record above; d_WF, d_WM the masks or NULL */
SIFT3D_AMD_API int
sift3d_hip_affine_ncc_normal_eqs(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                 const double *A /*12*/, void *d_record, void *d_work, void *stream,
                                 const float *d_WF, const float *d_WM);
/* host only: record on the host */
SIFT3D_AMD_API int sift3d_amd_affine_ncc_fit(const void *record, double *out /*4*/);
SIFT3D_AMD_API int
sift3d_amd_affine_ncc_lm_step(const void *record, unsigned free_mask, double lambda, double *delta /*12*/);
/* bytes of d_work for the driver (0 for bad arguments) */
SIFT3D_AMD_API size_t
sift3d_amd_affine_ncc_refine_work_bytes(int ox, int oy, int oz, int nx, int ny, int nz, int levels);
/* A_io [12] and fit_out [4] on the host; waits for `stream` once per evaluation */
SIFT3D_AMD_API int
sift3d_amd_affine_ncc_refine_device(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                    double *A_io, const sift3d_amd_affine_refine_params *params,
                                    sift3d_amd_affine_refine_result *result, double *fit_out /*4*/, void *d_work,
                                    void *stream, const float *d_WF, const float *d_WM);

/* ------------------------------------------------------------------------ */
/* Mutual-information affine refinement (Mattes)                             */
/* ------------------------------------------------------------------------ */
/* "Intensity-driven affine refinement" for two volumes whose intensities are related by an unknown map that need not be
 * monotone (CT to MR, T1 to T2): the pull map is moved towards a larger mutual information of the fixed bin and a
 * Parzen-windowed moving bin (Mattes et al.).  The histogram is accumulated in fixed point, so it is exact and a
 * function of the inputs alone; the device never takes a logarithm: the host turns the integer histogram into the cost
 * and a table W, and hands W to the second pass.  No upstream counterpart: PARITY UNPINNED, pinned to this contract and
 * its numpy restatement (tests/affine_mi_restatement.py).
 *
 * The pull map, the inside test, the LINEAR sample m, its gradient g, the centring c, P and J[4 d + j] = G_d P_j are
 * those of "Intensity-driven affine refinement", word for word; d_WF and d_WM are "Masks"' masks, word for word, and
 * either may be NULL.
 *
 * Bins.  B = bins, 4 <= B <= SIFT3D_AMD_PARZEN_MAX_BINS, and per volume a range lo < hi (finite floats); each range is
 * refused as "Similarity measures" refuses it with this B.
 * Fixed bin.  b_f is "Similarity measures"' rule on (lo_f, hi_f, B), in float, word for word: s = (float) B / (hi_f -
 * lo_f), t = (f - lo_f) * s, b_f = t < 0 ? 0 : t >= B ? B - 1 : (int) t.
 * Moving window.  The moving value is spread over four bins by a cubic B-spline, with one padding bin at each end.
 * s_m = (double)(B - 3) / ((double) hi_m - (double) lo_m) once on the host; per voxel, double, this order, unfused:
 *     t   = 1.0 + ((double) m - (double) lo_m) * s_m
 *     out = t < 1.0 || t > (double)(B - 2)                         (m outside its range)
 *     t   = clamp(t, 1.0, B - 2)
 *     k0  = min((int) floor(t) - 1, B - 4)
 *     r   = t - (double)(k0 + 1)                                   (exact, in [0, 1])
 *     w[0..3]  = the four cubic weights of "B-spline free-form deformation" at t := r, kept in double
 *     dw[0..3] = -(u * u) / 2,  (3 * t2 - 4 * r) / 2,  ((-3 * t2 + 2 * r) + 1) / 2,  t2 / 2     (u = 1 - r, t2 = r * r)
 *     q[k]     = (uint32) llrint(w[k] * 65536.0)                   (round to nearest even)
 * One inline function (sift3d_parzen.h) states this for the kernels and the host; sift3d_amd_parzen_window exports it.
 *
 * Parzen histogram (sift3d_hip_parzen_hist_affine).  Every counted voxel adds q[k] to hist[b_f][k0 + k], k = 0 .. 3, and
 * 1 to the count: integer adds only, so hist [B][B] uint64 and the uint64 count are exact however they are reduced.
 * Tiles, grid (min(tiles, SIFT3D_AMD_SIMILARITY_GRID) workgroups), XCD grouping and the merge of workgroup-private
 * counters into hist are "Similarity measures"'; the private counters are 64 bits wide (a voxel adds up to 43691 to a
 * bin), so none wraps for any grid the tiling accepts.  Both outputs are zeroed / written on `stream` by the call.
 * Checks, alignment (hist, count, work: 8 bytes; the rest 4), overlap rules, asynchrony and "allocates nothing" are
 * sift3d_hip_similarity_affine_masked's.  d_work: sift3d_amd_parzen_hist_work_bytes() bytes.
 *
 * Cost and table (sift3d_amd_parzen_mi, host).  With r, c, N of "Similarity measures" on hist: out->n = N, the three
 * entropies, mi and nmi by that section's formulas (one routine; all NaN when N == 0), msd = ncc = NaN; cost = -mi.
 *     W[i][j] = log((double) hist[i][j] / (double) c[j]) where hist[i][j] != 0, else 0.0         (W may be NULL)
 * -1 on a NULL hist or out, or bins out of range.
 *
 * MI record (sift3d_hip_affine_mi_normal_eqs).  d_W [B][B] double on the device.  Per counted voxel, double, unfused:
 *     psi   = out ? 0.0 : s_m * (((dw[0] * W0 + dw[1] * W1) + dw[2] * W2) + dw[3] * W3),   Wk = W[b_f][k0 + k]
 *     G'_d  = psi * (double) g_d,   J'[4 d + j] = G'_d P_j,   E = -1
 * The record has the layout of the MSD record, SIFT3D_AMD_AFFINE_NORMAL_BYTES:
 *     uint64 n;  double S_pp = sum psi psi;  double b[12] = sum J' E;  double H[12][12] = sum J' J'^T,
 * H full and symmetric bit for bit; partial slots, finish and ordering rules are the MSD record's (a term carries at
 * most 11 roundings: that record's 8, the two products psi * g_d and their now inexact product).  -mi is, up to a term
 * that does not depend on A to first order, the mean negative log-likelihood -(1 / n) sum log p(m | f); psi J is its
 * per-voxel score and sum psi^2 J J^T its Fisher information, so sift3d_amd_affine_lm_step on this record is a damped
 * Fisher-scoring step, positive semi-definite and free of the scale of psi.  Checks are sift3d_hip_affine_normal_eqs_
 * masked's, with d_W an 8-byte aligned input.  d_work: sift3d_amd_affine_normal_work_bytes() bytes.
 *
 * Driver (sift3d_amd_affine_mi_refine_device).  sift3d_amd_affine_refine_device's loop, levels, masks and stop reasons,
 * one loop in the code too.  An evaluation is one histogram pass and sift3d_amd_parzen_mi on the host; its n is the
 * count.  The MI record is computed only at the map the next step starts from (a level's first map and each accepted
 * trial that does not end the level): one copy of W to the device and one pass; a rejected trial costs the histogram
 * pass alone.  Accept when n' >= min_overlap * n_first and cost' < cost.  An evaluation with N == 0 has no cost: as a
 * trial it is rejected, as a level's first evaluation it stops the level with LM_FAILED.  Ranges and bins are level 0's
 * at every level (restriction averages, so values stay in range).  Params and result are the existing structs; the
 * trail's `msd` field carries `cost`.  mi_out: the measures at the final A on level 0 (n = N; all NaN and n = 0 when no
 * evaluation was made).  Checks are the NCC driver's, then bins and ranges; mi_out must not be NULL.
 * d_work: sift3d_amd_affine_mi_refine_work_bytes() bytes, whatever `bins` is. */
#define SIFT3D_AMD_PARZEN_MAX_BINS 64
/* host only: the window of one moving value.  -1 on NULL pointers, bins out of range or a refused range. */
SIFT3D_AMD_API int
sift3d_amd_parzen_window(float m, float lo, float hi, int bins, int *k0, uint32_t *q /*4*/, double *dw /*4*/, int *out);
/* bytes of d_work for sift3d_hip_parzen_hist_affine on this fixed grid (0 for dims <= 0) */
SIFT3D_AMD_API size_t sift3d_amd_parzen_hist_work_bytes(int ox, int oy, int oz);
/* d_F [oz][oy][ox], d_M [nz][ny][nx], d_hist [bins][bins] uint64, d_count one uint64; d_WF, d_WM the masks or NULL */
SIFT3D_AMD_API int
sift3d_hip_parzen_hist_affine(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                              const double *A /*12*/, int bins, float lo_f, float hi_f, float lo_m, float hi_m,
                              uint64_t *d_hist, uint64_t *d_count, void *d_work, void *stream, const float *d_WF,
                              const float *d_WM);
/* host only: hist [bins][bins] on the host; W [bins][bins] or NULL */
SIFT3D_AMD_API int sift3d_amd_parzen_mi(const uint64_t *hist, int bins, sift3d_amd_similarity *out, double *W);
/* d_W [bins][bins] double on the device; d_record the MSD record's layout */
SIFT3D_AMD_API int
sift3d_hip_affine_mi_normal_eqs(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                const double *A /*12*/, int bins, float lo_f, float hi_f, float lo_m, float hi_m,
                                const double *d_W, void *d_record, void *d_work, void *stream, const float *d_WF,
                                const float *d_WM);
/* bytes of d_work for the driver (0 for bad arguments) */
SIFT3D_AMD_API size_t
sift3d_amd_affine_mi_refine_work_bytes(int ox, int oy, int oz, int nx, int ny, int nz, int levels);
/* A_io [12] and mi_out on the host; waits for `stream` once per pass */
SIFT3D_AMD_API int
sift3d_amd_affine_mi_refine_device(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                   double *A_io, int bins, float lo_f, float hi_f, float lo_m, float hi_m,
                                   const sift3d_amd_affine_refine_params *params,
                                   sift3d_amd_affine_refine_result *result, sift3d_amd_similarity *mi_out,
                                   void *d_work, void *stream, const float *d_WF, const float *d_WM);

/* ------------------------------------------------------------------------ */
/* Initial transforms: moments and candidate search                          */
/* ------------------------------------------------------------------------ */
/* Every intensity refinement here is a local descent and has to be handed a start.  This section makes one from the
 * two volumes alone: the moments of each (centre of mass, principal axes), a list of candidate rigid pull maps about
 * the two centres (the centres alone, the four proper rotations that map one principal frame onto the other, or a
 * coarse grid of rotations and offsets), all candidates scored in one call at a coarse level, and the best of them
 * carried to level 0.  Everything is in voxels.  No upstream counterpart: PARITY UNPINNED, pinned to this contract and
 * to its numpy restatement (tests/affine_init_restatement.py).
 *
 * Moments (sift3d_hip_moments).  Per voxel p of V[nz][ny][nx]: w = V(p) - floor (a float subtraction); the voxel counts
 * when w > 0 (a NaN never does) and, with a mask d_W, when the mask is in ("Masks": in where >= 0.5).  Its weight is
 * W = (double) w (SIFT3D_AMD_MOMENTS_INTENSITY) or W = 1.0 (SIFT3D_AMD_MOMENTS_BINARY, the geometric form: moments
 * weighted by intensity change with the contrast, so the binary form is the one that serves two modalities).
 * Coordinates are centred on the grid, P = p - c, c = ((nx-1)/2, (ny-1)/2, (nz-1)/2), exact in double: the centring
 * of the affine normal equations.  The record, SIFT3D_AMD_MOMENTS_BYTES, 8-byte aligned:
 *     bytes 0-7 uint64 n; then ten doubles: S0 = sum W; S1[3] = sum W P_d; S2[6] = sum (W P_d) P_e for (d, e) = xx, xy,
 *     xz, yy, yz, zz; the products unfused, in the order written.
 * The sums are per-lane, then per-workgroup partials (one slot per workgroup of a grid of min(tiles,
 * SIFT3D_AMD_SIMILARITY_GRID) workgroups, whatever the device; a tile is 64 x 4 x 4 voxels), then the slots in a fixed
 * order: a call repeats its bytes, and the bytes depend on the shapes only.  n == 0 leaves the record all zero.
 * The entry is asynchronous on `stream`, allocates nothing, uses 64-bit offsets and checks its arguments before any
 * device call: -1 on NULL pointers (d_W may be NULL), dims <= 0, a floor that is not finite, an unknown weight, a
 * misaligned buffer (record, work: 8 bytes; the rest 4), an output that overlaps an input or the other output, a grid
 * with too many tiles.  d_work: sift3d_amd_moments_work_bytes() bytes.
 *
 * Frame (sift3d_amd_moments_frame; host, double).  mu = S1 / S0, centroid = c + mu, C_de = S2_de / S0 - mu_d mu_e; the
 * eigen-decomposition of C by cyclic Jacobi (rotations (0,1), (0,2), (1,2) per sweep; theta = (C_qq - C_pp) / (2 C_pq),
 * t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c; until the squared off-diagonal sum is
 * at most 1e-60 of the squared absolute trace).  lambda[3]: the eigenvalues, descending (equal ones in the order of
 * their diagonal position); axes[9]: the eigenvectors as ROWS.  Signs: in rows 0 and 1 the component of largest
 * magnitude is positive (the lowest index among equal magnitudes); row 2 = row 0 x row 1, so det = +1 always.
 * -1, with nothing written, when n == 0, S0 <= 0 or anything is not finite.
 *
 * Batched similarity (sift3d_hip_similarity_affine_batch, _masked).  K affine pull maps A[K][12] (host), 1 <= K <=
 * SIFT3D_AMD_SIMILARITY_BATCH_MAX, scored in one call.  The contract is one sentence: candidate k's histogram
 * d_hist[k][bins][bins] and stats record (d_stats + k * SIFT3D_AMD_SIMILARITY_STATS_BYTES) are, byte for byte, what
 * sift3d_hip_similarity_affine (_masked) writes for A_k with the same other arguments.  bins == 0 with d_hist == NULL
 * asks for the stats records alone: no histogram, in memory or in LDS (what MSD and NCC scoring use); bins == 0 with a
 * histogram, or bins > 0 without one, is refused.  The maps are read from the caller's array inside the call (they
 * travel as kernel arguments), so the array may be reused when the call returns; the entry waits for nothing.  It
 * refuses what the single entry refuses, for every candidate, before any device call: a non-finite A_k anywhere gives
 * -1 and nothing is launched.  d_work: sift3d_amd_similarity_batch_work_bytes() bytes, 8-byte aligned.
 *
 * Candidates (sift3d_amd_affine_init_candidates; host, double).  A candidate is a rigid pull map about the two
 * centroids, q = R (p - c_F) + c_M + t, stored as L = R and
 *     A[d][3] = (c_M[d] + t[d]) - ((R[d][0] c_Fx + R[d][1] c_Fy) + R[d][2] c_Fz)        (unfused).
 *   CENTROID: K = 1, R = I, t = 0.
 *   AXES:     K = 5.  Candidate 0 is the centroid one; candidates 1-4 are R = V_M^T (D_s V_F), V the axes matrices
 *             (rows are eigenvectors), D_s = diag(1,1,1), (1,-1,-1), (-1,1,-1), (-1,-1,1) in that order: the four
 *             proper rotations that map F's principal frame onto M's.
 *   SEARCH:   R = Rz(gamma) (Ry(beta) Rx(alpha)); each angle runs over -range_deg[d] .. +range_deg[d] in steps of
 *             step_deg, value i of 2 floor(range / step) + 1 being (i - floor(range / step)) * step (range 0: the single
 *             value 0); crossed with offsets t_d over -range_vox[d] .. +range_vox[d] in steps of step_vox, formed the
 *             same way.  The index runs alpha fastest, then beta, gamma, t_x, t_y, t_z.  cos and sin are taken of
 *             a * (pi / 180) in double; a matrix product's entry is (a0 b0 + a1 b1) + a2 b2, unfused.  The defaults
 *             (90, 90, 90 by 30 degrees, no offsets) make 343 candidates.
 * *K on entry: the maps A_out holds; on return: the count.  A_out == NULL asks for the count alone.  -1 on a frame that
 * is not finite, an unknown mode, a range < 0 or a step <= 0 (or either not finite), more than
 * SIFT3D_AMD_INIT_MAX_CANDIDATES candidates, or an A_out that is too small.
 *
 * Ranking (sift3d_amd_affine_init_rank; host).  stats: K records; hist: K histograms (MI; else it may be NULL).  Cost:
 *   MSD: msd;  NCC: 1 - ncc^2 (a negative gain is as good as a positive one, as in the NCC refinement);  MI: -mi, of
 *   sift3d_amd_similarity_measures on the candidate's histogram.  NaN when n_k == 0.
 * A candidate is eligible when n_k >= min_overlap * max_j n_j, n_k > 0 and its cost is finite.  order_out lists the
 * *count_out eligible candidates by ascending cost, ties going to the lower index.  cost_out and n_out (K each) are
 * written for every candidate.  -1 when none is eligible (the outputs are written all the same), or on bad arguments.
 *
 * Driver (sift3d_amd_affine_init_device).
 *   1. levels' = sift3d_amd_affine_init_levels(): the largest l <= levels for which no axis of either volume falls
 *      below 8 on level l - 1.  Volumes and masks are restricted levels' - 1 times, as sift3d_amd_affine_refine_device
 *      restricts them (sift3d_hip_restrict2 at scale 1; the masks as floats).
 *   2. The moments of both on the coarsest level (floor_f, floor_m, weight; each volume's mask).
 *   3. The frames and the candidates there; range_vox and step_vox are level-0 voxels and are halved per level.
 *   4. The scores, LINEAR, through the batch entry in chunks of at most SIFT3D_AMD_SIMILARITY_BATCH_MAX: one copy to
 *      the host and one wait per chunk (and one for the two moments records).  MI scores with bins and the two ranges;
 *      MSD and NCC with bins == 0.
 *   5. The ranking.  The best map goes to level 0 as the affine driver carries a map up: the translation column
 *      doubles per level.  The frames are reported in level-0 voxels (centroid x 2, lambda x 4 per level).
 * costs_out, counts_out: K doubles / uint64 for every candidate's cost and count, or NULL.  The driver keeps host
 * scratch of its own (malloc) for the candidates and a chunk's records.  -1 on bad arguments (as the refinement
 * drivers), when a volume has nothing above its floor, or when no candidate is eligible (result->K, levels and the
 * frames are then written, and the caller's arrays too). */
#define SIFT3D_AMD_MOMENTS_BYTES 88                /* 8 + 10 * 8 */
#define SIFT3D_AMD_MOMENTS_INTENSITY 0
#define SIFT3D_AMD_MOMENTS_BINARY 1
#define SIFT3D_AMD_SIMILARITY_BATCH_MAX 1024
#define SIFT3D_AMD_INIT_MAX_CANDIDATES 16384
#define SIFT3D_AMD_INIT_KEEP 16
#define SIFT3D_AMD_INIT_CENTROID 0
#define SIFT3D_AMD_INIT_AXES 1
#define SIFT3D_AMD_INIT_SEARCH 2
#define SIFT3D_AMD_INIT_MSD 0
#define SIFT3D_AMD_INIT_NCC 1
#define SIFT3D_AMD_INIT_MI 2
typedef struct {
    double centroid[3], axes[9], lambda[3];
} sift3d_amd_frame;
typedef struct {
    int mode, metric, levels, weight;
    float floor_f, floor_m;
    int bins;                                    /* MI */
    float lo_f, hi_f, lo_m, hi_m;                /* MI */
    double range_deg[3], step_deg;               /* SEARCH: about x, y, z */
    double range_vox[3], step_vox;               /* SEARCH: level-0 voxels */
    double min_overlap;
} sift3d_amd_affine_init_params;
typedef struct {
    double A[12];                                /* the best candidate on level 0 */
    int index, K, levels, kept;                  /* its index; the candidates; the levels run; entries of keep_* */
    double cost;
    uint64_t n;
    sift3d_amd_frame frame_f, frame_m;   /* level-0 voxels */
    int keep_index[SIFT3D_AMD_INIT_KEEP];        /* the best candidates, ascending cost */
    double keep_cost[SIFT3D_AMD_INIT_KEEP];
    uint64_t keep_n[SIFT3D_AMD_INIT_KEEP];
} sift3d_amd_affine_init_result;
/* bytes of d_work for sift3d_hip_moments on this grid (0 for dims <= 0) */
SIFT3D_AMD_API size_t sift3d_amd_moments_work_bytes(int nx, int ny, int nz);
/* d_V [nz][ny][nx]; d_W its mask or NULL; d_record the record above */
SIFT3D_AMD_API int
sift3d_hip_moments(const float *d_V, int nx, int ny, int nz, const float *d_W, int weight, float floor, void *d_record,
                   void *d_work, void *stream);
/* host only: record on the host */
SIFT3D_AMD_API int
sift3d_amd_moments_frame(const void *record, int nx, int ny, int nz, double *centroid /*3*/, double *axes /*9*/,
                         double *lambda /*3*/);
/* bytes of d_work for a batch call with these arguments (0 for dims <= 0, bins or K out of range, too many tiles) */
SIFT3D_AMD_API size_t sift3d_amd_similarity_batch_work_bytes(int ox, int oy, int oz, int bins, int K);
/* A [K][12] on the host; d_hist [K][bins][bins] uint64 or NULL (bins == 0); d_stats K records */
SIFT3D_AMD_API int
sift3d_hip_similarity_affine_batch(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                   const double *A, int K, int interp, int bins, float lo_f, float hi_f, float lo_m,
                                   float hi_m, uint64_t *d_hist, void *d_stats, void *d_work, void *stream);
SIFT3D_AMD_API int
sift3d_hip_similarity_affine_batch_masked(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny,
                                          int nz, const double *A, int K, int interp, int bins, float lo_f, float hi_f,
                                          float lo_m, float hi_m, uint64_t *d_hist, void *d_stats, void *d_work,
                                          void *stream, const float *d_WF, const float *d_WM);
SIFT3D_AMD_API void sift3d_amd_affine_init_default_params(sift3d_amd_affine_init_params *p);
/* sizeof the params (0), the frame (1), the result (2); SIFT3D_AMD_MOMENTS_BYTES (3), SIFT3D_AMD_SIMILARITY_BATCH_MAX
 * (4), SIFT3D_AMD_INIT_MAX_CANDIDATES (5), SIFT3D_AMD_INIT_KEEP (6); 0 otherwise */
SIFT3D_AMD_API size_t sift3d_amd_affine_init_struct_bytes(int which);
/* host only; params NULL: the defaults */
SIFT3D_AMD_API int
sift3d_amd_affine_init_candidates(int mode, const sift3d_amd_frame *frame_F,
                                  const sift3d_amd_frame *frame_M, const sift3d_amd_affine_init_params *params,
                                  double *A_out /* K x 12 */, int *K);
/* host only */
SIFT3D_AMD_API int
sift3d_amd_affine_init_rank(int metric, int K, const void *stats, const uint64_t *hist, int bins, double min_overlap,
                            double *cost_out, uint64_t *n_out, int *order_out, int *count_out);
/* the levels the driver runs for `levels` asked (0 for levels < 1) */
SIFT3D_AMD_API int sift3d_amd_affine_init_levels(int ox, int oy, int oz, int nx, int ny, int nz, int levels);
/* bytes of d_work for the driver (0 for bad arguments); params NULL: the defaults */
SIFT3D_AMD_API size_t
sift3d_amd_affine_init_work_bytes(int ox, int oy, int oz, int nx, int ny, int nz,
                                  const sift3d_amd_affine_init_params *params);
/* d_WF, d_WM the masks or NULL; result, costs_out, counts_out on the host; waits for `stream` */
SIFT3D_AMD_API int
sift3d_amd_affine_init_device(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                              const float *d_WF, const float *d_WM, const sift3d_amd_affine_init_params *params,
                              sift3d_amd_affine_init_result *result, double *costs_out, uint64_t *counts_out,
                              void *d_work, void *stream);

/* ------------------------------------------------------------------------ */
/* Mutual-information free-form deformation (Mattes)                         */
/* ------------------------------------------------------------------------ */
/* "B-spline free-form deformation" for two volumes whose intensities are related by an unknown map that need not be
 * monotone: the lattice is moved towards a larger mutual information of "Mutual-information affine refinement
 * (Mattes)", plus the same bending penalty.  The lattice, the weight table, the spline value, the field export, the
 * bending energy, the subdivision and the masks are those of "B-spline free-form deformation" and "Masks", word for
 * word; bins, the two ranges, the fixed bin, the moving window (sift3d_parzen.h), the fixed-point histogram and
 * sift3d_amd_parzen_mi are those of "Mutual-information affine refinement (Mattes)", word for word.  No upstream
 * counterpart: PARITY UNPINNED, pinned to this contract and its numpy restatement (tests/ffd_mi_restatement.py).
 *
 * Histogram through a field (sift3d_hip_parzen_hist_field).  sift3d_hip_parzen_hist_affine with d_field[3][oz][oy][ox]
 * in the place of A: the sample point q = p + u(p), the inside test and the LINEAR sample m are sift3d_hip_warp_field's,
 * bit for bit; a non-finite field entry is outside, as in sift3d_hip_similarity_field_masked.  Bins, ranges, the window,
 * the fixed-point adds and the 64-bit workgroup-private counters are the affine entry's, word for word; so are the grid,
 * the merge, the zeroing of both outputs, the masks, checks (d_field a 4-byte aligned input that no output may
 * overlap), alignment, overlap rules and work size (sift3d_amd_parzen_hist_work_bytes).  hist and count are exact
 * integers: a function of the inputs alone.
 *
 * MI evaluation (sift3d_hip_ffd_mi_evaluate).  The arguments of sift3d_hip_ffd_evaluate_masked, then bins, the two
 * ranges and d_W [B][B] double on the device (8-byte aligned; sift3d_amd_parzen_mi's table).  The call exports the field
 * of the lattice to d_field, then per counted fixed voxel (the masked evaluation's test, word for word), with m, g as
 * there and b_f, k0, dw, out as in the affine section, in double, unfused:
 *     psi  = out ? 0.0 : s_m * (((dw[0] * W0 + dw[1] * W1) + dw[2] * W2) + dw[3] * W3),   Wk = W[b_f][k0 + k]
 *     G'_d = psi * (double) g_d,   E = -1
 * The record has the layout of the FFD record (sift3d_amd_ffd_record_bytes):
 *     uint64 n;  double S_pp = sum psi psi;  double R;  double gmax;
 *     double Gc[3][gz][gy][gx] = sum_p W(p; k, j, i) E G'_d;  double dR[3][gz][gy][gx]
 * n is the count: a voxel with `out` is counted, with psi = 0, so n equals the histogram's count on the same inputs.  R,
 * dR and gmax are "B-spline free-form deformation"'s.  The rule for everything after the histogram is that section's: a
 * function of the shapes only, no atomics, every partial slot reduced in a fixed order; a call repeats its bytes.  The
 * force E G'_d = -(psi * g_d) carries one rounding where E G_d was exact (the sign is exact), so every entry of Gc is
 * within gamma_(k + 9) sum |term| of the exact sum of the terms W(p; k, j, i) (-(psi g_d)) in double, k the number of
 * voxels in the control's support; S_pp within gamma_(n + 1) sum psi psi.
 * Gradient.  d_grad = (float)((1.0 / n) * Gc + bending * dR), formed in double; the cost is -mi + bending * R.  The
 * factor is 1 / n, not the MSD's 2 / n: with p(b_m | b_f) read off the histogram, -mi is, up to the entropy of the fixed
 * marginal and a term that does not depend on the lattice to first order, -(1 / n) sum_p log p(m(p) | f(p)); moving a
 * control by dc moves m(p) by W(p) g_d dc, the window's weights by s_m dw[k] W(p) g_d dc, and the mean log-likelihood
 * by (1 / n) sum_p W(p) psi g_d dc, so d(-mi) / dc = (1 / n) sum_p W(p) (-1)(psi g_d) = Gc / n.  (A constant added to a
 * row of W drops out because sum_k dw[k] = 0: the partition of unity of the window, as in the affine section; that
 * is why W = log(hist / column sum) may stand for log p(b_m | b_f), which differs from it by the row's log-total.)
 *
 * Driver (sift3d_amd_ffd_mi_refine_device).  sift3d_amd_ffd_refine_masked_device's arguments, then bins, the two ranges
 * and mi_out.  sift3d_amd_ffd_refine_device's loop, levels, subdivision, step rule and stop reasons, one loop in the
 * code too, with cost E = -mi + bending * R.  An evaluation is the field, the histogram pass and the bending value; the
 * histogram, the count and the head go to the host (one wait) and sift3d_amd_parzen_mi gives -mi and W; its n is the
 * count.  The force, adjoint, bending-gradient and combine passes run only at the lattice the next step starts from (a
 * level's first lattice and each accepted trial that does not end the level): one copy of W to the device, the passes
 * and one more wait, for gmax.  A rejected trial costs the field, the histogram and the bending value alone.  An
 * evaluation with N == 0 has no cost: as a trial it is rejected (s = s / 2), as a level's first evaluation it stops the
 * level with FAILED.  Ranges and bins are level 0's on every level.  Params and result are the existing structs; the
 * trail's `msd` field carries -mi.  mi_out: the measures at the final lattice on level 0 (all NaN and n = 0 when no
 * evaluation was made).  Checks are the masked FFD driver's, then bins and ranges; mi_out must not be NULL.
 * d_work: sift3d_amd_ffd_mi_refine_work_bytes() bytes, whatever `bins` is: the masked FFD driver's layout, then the
 * histogram, the count and W. */
/* d_F [oz][oy][ox], d_M [nz][ny][nx], d_field [3][oz][oy][ox], d_hist [bins][bins] uint64, d_count one uint64 */
SIFT3D_AMD_API int
sift3d_hip_parzen_hist_field(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                             const float *d_field, int bins, float lo_f, float hi_f, float lo_m, float hi_m,
                             uint64_t *d_hist, uint64_t *d_count, void *d_work, void *stream, const float *d_WF,
                             const float *d_WM);
/* d_work: sift3d_amd_ffd_evaluate_work_bytes() bytes */
SIFT3D_AMD_API int
sift3d_hip_ffd_mi_evaluate(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                           const float *d_lattice, int gx, int gy, int gz, int dx, int dy, int dz,
                           const double *A /*12 or NULL*/, double bending, float *d_field, void *d_record,
                           float *d_grad, void *d_work, void *stream, const float *d_WF, const float *d_WM, int bins,
                           float lo_f, float hi_f, float lo_m, float hi_m, const double *d_W);
/* bytes of d_work for the driver (0 for bad arguments) */
SIFT3D_AMD_API size_t
sift3d_amd_ffd_mi_refine_work_bytes(int ox, int oy, int oz, int nx, int ny, int nz, int dx, int dy, int dz, int levels);
/* A [12] on the host or NULL; mi_out on the host; waits for `stream` once per evaluation and once per gradient */
SIFT3D_AMD_API int
sift3d_amd_ffd_mi_refine_device(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                const double *A, const sift3d_amd_ffd_refine_params *params,
                                sift3d_amd_ffd_refine_result *result, float *d_lattice, float *d_field, void *d_work,
                                void *stream, const float *d_WF, const float *d_WM, int bins, float lo_f, float hi_f,
                                float lo_m, float hi_m, sift3d_amd_similarity *mi_out);

/* ------------------------------------------------------------------------ */
/* Jacobian penalty: a volume (folding) term on a field and in the FFD drivers */
/* ------------------------------------------------------------------------ */
/* A penalty on the SAME discrete Jacobian that sift3d_hip_jacobian_det reports ("Displacement fields", steps 1 - 3), not
 * on the analytic derivative of a spline: what an optimiser lowers here is what the caller later reads as `folded`.  It
 * is defined on any field u[3][oz][oy][ox], N = ox oy oz, with a reference determinant `ref` (double, finite, not 0: the
 * determinant that counts as "no volume change", 1 for a field around the identity, det of A's linear part for a field
 * around A).  No upstream counterpart: PARITY UNPINNED, pinned to this contract and its numpy restatement
 * (tests/jacobian_penalty_restatement.py).  Double, unfused, unless stated.
 *
 * Per voxel p:
 *   j_de(p) float and det(p) double: "Displacement fields" steps 1 - 3 (det before its rounding to float in step 4);
 *   r = det / ref;
 *   r >= 1/4 :  phi = (r + 1.0 / r) - 2.0,                     phi' = 1.0 - 1.0 / (r * r);
 *   otherwise (r <= 0 and a NaN r included), t = r - 0.25:
 *               phi = (2.25 - 15.0 * t) + 64.0 * (t * t),      phi' = -15.0 + 128.0 * t.
 * phi is the symmetric volume term (r - 1)^2 / r, phi(r) = phi(1 / r), continued below 1/4 by its own second-order
 * Taylor polynomial there (phi(1/4) = 9/4, phi'(1/4) = -15, phi''(1/4) = 128): C^1 (C^2) at 1/4, finite for every finite
 * r, so a folded field needs no special case; only IEEE add, multiply and divide.  A NaN r gives a NaN phi.
 * Record (SIFT3D_AMD_JACOBIAN_PENALTY_RECORD_BYTES of device memory, 8-byte aligned; after the call completes):
 *   uint64 nonpos = the number of voxels with !(r > 0) (a NaN counts);
 *   double sum    = sum_p phi(r_p): per-workgroup partials (one slot per workgroup of a grid of min(tiles,
 *                   SIFT3D_AMD_SIMILARITY_GRID) workgroups, whatever the device; a tile is 64 x 4 x 8 voxels, x fastest),
 *                   then the slots in a fixed order; no atomics: its bits depend on the shapes and the field only, and it
 *                   is within gamma_(N) sum |phi| of the exact sum of the phi;
 *   double rmin, rmax over the non-NaN r (+inf, -inf when there is none): order-independent.
 *   The penalty is P = sum / N (the caller's division).
 * Gradient in sum form (d_grad, double [3][oz][oy][ox], the layout of the FFD force): d P / d u_d(q) = S_d(q) / N,
 *   S_d(q) = sum_e sum_p K_de(p) D_e[p][q],      K_de(p) = a(p) * C_de(p),      a(p) = phi'(r_p) / ref
 *   C(p): the cofactors of j(p) from the float j widened to double.  With d1 < d2 the two rows other than d and e1 < e2
 *         the two columns other than e,
 *           d + e even:  C_de = j[d1][e1] * j[d2][e2] - j[d2][e1] * j[d1][e2]
 *           d + e odd :  C_de = j[d2][e1] * j[d1][e2] - j[d1][e1] * j[d2][e2]
 *         (each product of two floats is exact in double, so every entry is one rounded difference, with its sign);
 *   D_e:  the matrix of numpy.gradient along axis e (0: x, 1: y, 2: z), g_e(p) = sum_q D_e[p][q] u(q), n the axis'
 *         length and i the coordinate of q along it: D_e[i - 1][i] = 1/2 (1 when i - 1 == 0), D_e[i + 1][i] = -1/2 (-1
 *         when i + 1 == n - 1), D_e[0][0] = -1, D_e[n - 1][n - 1] = 1, every other entry 0, and all of D_e is 0 when
 *         n == 1;
 *   order: from +0.0, S = S + (a(p) * C_de(p)) * D_e[p][q], axis e ascending, then p ascending (q - 1, q, q + 1 along
 *         e); a p with D_e[p][q] == 0 is not a term (nothing is added for it, a NaN there stays there).  The last
 *         multiply is exact.  One lane owns one S_d(q) and there are no atomics, so S is defined bit for bit.
 *
 * Lattice gradient (sift3d_hip_ffd_jacobian_gradient): the record of the field, and GJ [3][gz][gy][gx] double =
 * sum_p W(p; k, j, i) S_d(p) on the lattice of the field's grid at spacing (dx, dy, dz): S through the adjoint of the
 * spline exactly as the force of "B-spline free-form deformation" goes through it (one axis at a time, z, then y, then
 * x, each sum ascending from +0, double, unfused), so d P / d c = GJ / N and every entry is within gamma_(k + 8) sum
 * |term| of the exact sum of its terms, k the voxels under the control.  d_work: sift3d_amd_ffd_jacobian_gradient_
 * work_bytes() bytes, 16-byte aligned.  Checks as below, with the spacing in [1, SIFT3D_AMD_FFD_MAX_SPACING].
 *
 * sift3d_hip_jacobian_penalty: asynchronous on `stream`, allocates nothing, 64-bit offsets.  d_grad may be NULL (the
 * record alone; the record's bytes are the same either way).  d_work: sift3d_amd_jacobian_penalty_work_bytes() bytes, 8-
 * byte aligned.  -1 before any device call on a NULL d_field, d_record or d_work, dims <= 0, a `ref` that is not finite
 * or is 0, misalignment (d_field 4 B, the rest 8 B), an output (record, gradient, work) that overlaps the field or
 * another output.
 *
 * Driver (sift3d_amd_ffd_refine_jacobian_device).  sift3d_amd_ffd_mi_refine_device's arguments with bins == 0 meaning
 * the MSD of "B-spline free-form deformation" (the ranges are then not read and mi_out may be NULL; it is filled as by
 * that driver otherwise) and masks that may be NULL with either metric; then `jacobian` (the weight, finite, >= 0) and
 * `penalty`, a caller array of SIFT3D_AMD_FFD_MAX_TRAIL entries parallel to result->trail: {P, rmin, nonpos} of every
 * evaluation's field.  The loop, levels, subdivision, step rule and stop reasons are that driver's, one loop in the code
 * too, with
 *     E    = (image + bending * R) + jacobian * P               (image: S_ee / n, or -mi)
 *     grad = (float)(((scale / n) * Gc + bending * dR) + (jacobian / N) * GJ)        (scale: 2, or 1 for -mi)
 * where P = sum / N on the level's grid with ref = A[0] * (A[5] * A[10] - A[6] * A[9]) - A[1] * (A[4] * A[10] - A[6] *
 * A[8]) + A[2] * (A[4] * A[9] - A[5] * A[8]) (double, this order, unfused, on the host; 1.0 without A; the same on every
 * level), and GJ [3][gz][gy][gx] is S through the adjoint of the spline, the three passes of the evaluation (z, then y,
 * then x) on S in the place of the force.  The penalty acts on every voxel of the grid: masks limit the image force only,
 * as with the bending term.  With jacobian == 0 the two formulas are the existing drivers', to the letter (no third term
 * is added), P is still recorded, and lattice, field and trail are those drivers' byte for byte.  A non-finite P makes E
 * non-finite: the existing rule for a non-finite E applies.  The value pass runs in every evaluation; the gradient pass
 * runs where the image force runs (every evaluation of the MSD, the MI driver's gradient step).  -1 before any device
 * call on what the MI driver refuses (bins and ranges only when bins != 0), a NULL `penalty`, a `jacobian` that is not
 * finite or is negative, an A whose linear part has determinant 0.  d_work: sift3d_amd_ffd_refine_jacobian_work_bytes()
 * bytes: the MI driver's layout, then the penalty's record, GJ and the penalty's work. */
#define SIFT3D_AMD_JACOBIAN_PENALTY_RECORD_BYTES 32
typedef struct {
    double P;                                       /* sum / N */
    double rmin;
    uint64_t nonpos;
} sift3d_amd_ffd_penalty;
/* bytes of d_work (0 for bad arguments) */
SIFT3D_AMD_API size_t sift3d_amd_jacobian_penalty_work_bytes(int ox, int oy, int oz);
SIFT3D_AMD_API int sift3d_hip_jacobian_penalty(const float *d_field, int ox, int oy, int oz, double ref, void *d_record,
                                               double *d_grad /*NULL: value only*/, void *d_work, void *stream);
SIFT3D_AMD_API size_t sift3d_amd_ffd_jacobian_gradient_work_bytes(int ox, int oy, int oz, int dx, int dy, int dz);
SIFT3D_AMD_API int sift3d_hip_ffd_jacobian_gradient(const float *d_field, int ox, int oy, int oz, int dx, int dy, int dz,
                                                    double ref, void *d_record, double *d_GJ, void *d_work,
                                                    void *stream);
SIFT3D_AMD_API size_t
sift3d_amd_ffd_refine_jacobian_work_bytes(int ox, int oy, int oz, int nx, int ny, int nz, int dx, int dy, int dz,
                                          int levels);
/* A [12] on the host or NULL; mi_out (NULL allowed when bins == 0) and penalty on the host */
SIFT3D_AMD_API int
sift3d_amd_ffd_refine_jacobian_device(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                      const double *A, const sift3d_amd_ffd_refine_params *params,
                                      sift3d_amd_ffd_refine_result *result, float *d_lattice, float *d_field,
                                      void *d_work, void *stream, const float *d_WF, const float *d_WM, int bins,
                                      float lo_f, float hi_f, float lo_m, float hi_m, sift3d_amd_similarity *mi_out,
                                      double jacobian, sift3d_amd_ffd_penalty *penalty);

/* ------------------------------------------------------------------------ */
/* Multi-channel free-form deformation: the MSD of a stack of channels        */
/* ------------------------------------------------------------------------ */
/* "B-spline free-form deformation" driven by the squared difference summed over nc >= 1 channels: the dense descriptor
 * images of the two volumes (12 unit-length channels, which do not change under a gain or an offset of either volume),
 * or several contrasts of one subject.  No upstream counterpart: PARITY UNPINNED, pinned to this contract and its numpy
 * restatement (tests/ffd_channels_restatement.py).
 *
 * Inputs.  F[nc][oz][oy][ox] and M[nc][nz][ny][nx] float32, planar; one lattice, one field and one pair of masks
 * (W_F[oz][oy][ox], W_M[nz][ny][nx], either may be NULL) for all channels.
 * Per fixed voxel p with u = field(p): the sample point q = p + u(p), the inside test, the mask rule and the taps are
 * those of sift3d_hip_ffd_evaluate_masked, word for word, and are the same for every channel.  Per channel c, on
 * channel c of M with those taps: the LINEAR sample m_c and its gradient g_c (float, unfused, as in "Intensity-driven
 * affine refinement"); e_c = m_c - f_c, a float subtraction; in double E_c = e_c, g_cd widened.
 * Force.  Each product E_c g_cd is exact in double (two floats).  The additions are in double, in ascending c, and start
 * from channel 0's product, not from +0.0:
 *     S_d(p) = ((E_0 g_0d + E_1 g_1d) + E_2 g_2d) + ...
 * A voxel that is not counted stores +0.0.  With nc == 1 this is the single-channel force, signed zeros included.  S_d
 * is defined bit for bit.  After sift3d_hip_ffd_evaluate_channels it is left in d_work as double [3][oz][oy][ox] at
 * byte offset 16 * (dx + dy + dz) + 16 * SIFT3D_AMD_SIMILARITY_GRID (behind the weight tables and the partial slots).
 * Record: the layout of the FFD record (sift3d_amd_ffd_record_bytes).
 *     n counts voxels, not voxel-channels;
 *     S_ee = sum_p sum_c E_c E_c, in an order that is a function of the shapes only (per lane c ascending within a voxel,
 *     then the partial slots of "B-spline free-form deformation"), no atomics: a call repeats its bytes; within
 *     gamma_(nc * ox oy oz + 8) sum E_c E_c of the exact sum;
 *     Gc[3][gz][gy][gx] = sum_p W(p; k, j, i) S_d(p): the adjoint passes of that section applied to S.  The computed
 *     S_d is sum_c E_c g_cd (1 + theta_c) with |theta_c| <= gamma_(nc - 1) (nc - 1 additions of exact products), and the
 *     adjoint adds at most k + 8 roundings to each of its terms as there (k the voxels under the control), so every
 *     entry of Gc is within gamma_(k + nc + 8) sum_p sum_c |W E_c g_cd| of the exact sum: the single-channel bound plus
 *     the nc - 1 additions of S;
 *     R, dR and gmax are that section's.
 * Cost and gradient: E = S_ee / n + bending * R (+ jacobian * P); d_grad = (float)((2.0 / n) * Gc + bending * dR) (+ the
 * penalty's term), through the combine passes of the single-channel evaluation, unchanged.  With nc == 1 the record,
 * the gradient and the field are sift3d_hip_ffd_evaluate_masked's byte for byte.
 * sift3d_hip_ffd_evaluate_channels: the arguments of sift3d_hip_ffd_evaluate_masked with nc behind the moving grid.
 * d_work: sift3d_amd_ffd_evaluate_channels_work_bytes() bytes, 16-byte aligned: the single-channel figure, one force
 * volume whatever nc is.
 *
 * Driver (sift3d_amd_ffd_refine_channels_device).  The caller supplies every level's stacks and masks, level 0 the
 * finest, as in "Multi-resolution demons": how they are made is the caller's choice (restrict2 of the level above, or
 * features computed on the restricted volumes), and the driver restricts nothing.  Every dimension of level l >= 1,
 * fixed and moving, must be the half (n + 1) / 2 of level l - 1's.  The loop, the halving of A[:][3] per level, the
 * subdivision, the step rule, the stop reasons and the trail are sift3d_amd_ffd_refine_device's, one loop in the code
 * too; the trail's msd is S_ee / n.  params->levels must equal `levels` (NULL params: the defaults, so levels == 3).
 * `jacobian` and `penalty` are sift3d_amd_ffd_refine_jacobian_device's: penalty == NULL runs without the penalty (and
 * jacobian must be 0); otherwise P is recorded per evaluation and jacobian > 0 adds the third term.
 * d_work: sift3d_amd_ffd_refine_channels_work_bytes() bytes for level 0's fixed grid, 16-byte aligned: the evaluation's
 * work, the record, five lattices, then the penalty's record, GJ and work.
 *
 * Refusals, before any device call: those of sift3d_hip_ffd_evaluate_masked and of the masked driver, and nc < 1, a NULL
 * level table or a NULL d_F or d_M of a level, levels outside [1, SIFT3D_AMD_DEMONS_MAX_LEVELS] or != params->levels,
 * dimensions that are not the halving chain, a level's stack or mask that is misaligned (4 bytes) or overlaps an output
 * or the work buffer, a Jacobian weight that is negative, not finite, or not 0 without `penalty`; -1. */
typedef struct {
    const float *d_F;          /* fixed stack  [nc][oz][oy][ox] */
    int ox, oy, oz;
    const float *d_M;          /* moving stack [nc][nz][ny][nx] */
    int nx, ny, nz;
    const float *d_WF;         /* fixed mask [oz][oy][ox], or NULL */
    const float *d_WM;         /* moving mask [nz][ny][nx], or NULL */
} sift3d_amd_ffd_level;
/* for bindings that restate the layout: sizeof the level struct (0), then the offsets of d_F (1), ox (2), d_M (3),
 * nx (4), d_WF (5), d_WM (6); 0 otherwise */
SIFT3D_AMD_API size_t sift3d_amd_ffd_level_struct_bytes(int which);
SIFT3D_AMD_API size_t sift3d_amd_ffd_evaluate_channels_work_bytes(int ox, int oy, int oz, int dx, int dy, int dz);
SIFT3D_AMD_API int
sift3d_hip_ffd_evaluate_channels(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                 int nc, const float *d_lattice, int gx, int gy, int gz, int dx, int dy, int dz,
                                 const double *A /*12 or NULL*/, double bending, float *d_field, void *d_record,
                                 float *d_grad, void *d_work, void *stream, const float *d_WF, const float *d_WM);
/* bytes of d_work for the driver, (ox, oy, oz) level 0's fixed grid (0 for bad arguments) */
SIFT3D_AMD_API size_t sift3d_amd_ffd_refine_channels_work_bytes(int ox, int oy, int oz, int dx, int dy, int dz);
/* level [levels] (host memory, level 0 the finest); A [12] on the host or NULL; penalty on the host or NULL */
SIFT3D_AMD_API int
sift3d_amd_ffd_refine_channels_device(const sift3d_amd_ffd_level *level, int levels, int nc, const double *A,
                                      const sift3d_amd_ffd_refine_params *params,
                                      sift3d_amd_ffd_refine_result *result, float *d_lattice, float *d_field,
                                      void *d_work, void *stream, double jacobian,
                                      sift3d_amd_ffd_penalty *penalty /*NULL when jacobian == 0*/);

/* ------------------------------------------------------------------------ */
/* FFD landmarks: the spline at points, and a matched-point term in the FFD drivers */
/* ------------------------------------------------------------------------ */
/* The cubic B-spline of "B-spline free-form deformation" evaluated at arbitrary points of the fixed grid instead of its
 * voxels, the adjoint of that evaluation, and the corresponding-points term built from the two: "these two points
 * correspond" next to the image term of the FFD drivers.  No upstream counterpart: PARITY UNPINNED, pinned to this
 * contract and its numpy restatement (tests/ffd_landmarks_restatement.py).  All arithmetic is double, unfused, in the
 * order written.
 *
 * Point weights.  Along an axis with spacing delta and lattice size g, for a coordinate x (double, voxels of the fixed
 * grid): v = x / (double) delta, i0 = floor(v), t = v - (double) i0, and the four weights are the formulas of
 * sift3d_amd_ffd_weights with this t, left in double (not rounded to float).  A point is INSIDE when every coordinate is
 * finite and 0 <= i0 <= g - 4 on every axis: the lattice's own support 0 <= x < (g - 3) delta, which contains the grid.
 * Spline at a point: s_d(p) = sum_c sum_b sum_a wz[c] * (wy[b] * (wx[a] * (double) c_d[k0 + c][j0 + b][i0 + a])), from
 * +0, the 64 terms one by one in the voxel spline's order (c outermost, x innermost).
 * Map: T_d(p) = q_d + s_d(p), q_d = A[d][0] x + ((A[d][1] y + A[d][2] z) + A[d][3]) with A, q_d = p_d with A NULL.
 *
 * sift3d_hip_ffd_points: T [m][3] double from P [m][3] double (device memory, xyz), m >= 1; a point that is not inside
 * gets three NaNs.  Asynchronous on `stream`, allocates nothing.  -1 before any device call on a NULL d_lattice, d_P or
 * d_T, a lattice dimension < 4, a spacing outside [1, SIFT3D_AMD_FFD_MAX_SPACING], m < 1, a non-finite A, misalignment
 * (lattice 4 B, d_P and d_T 8 B), a d_T that overlaps the lattice or d_P.
 *
 * Landmarks.  Host arrays P [m][3] (fixed voxels, xyz), Q [m][3] (moving voxels) and w [m] (NULL: all 1), 1 <= m <=
 * SIFT3D_AMD_FFD_MAX_LANDMARKS.  A landmark whose P is not inside is not COUNTED (no error).  The residual of a counted
 * landmark is r_i = T(P_i) - Q_i.  Record (SIFT3D_AMD_FFD_LANDMARKS_RECORD_BYTES of device memory, 8-byte aligned):
 *   uint64 counted;
 *   double S     = sum_i w_i * ((rx rx + ry ry) + rz rz);
 *   double Omega = sum_i w_i;
 *   double rmax  = max_i sqrt((rx rx + ry ry) + rz rz), fmax from +0 (correctly rounded sqrt);
 * every sum and the maximum over the counted landmarks only (all four are 0 when there is none).
 * Optional outputs (device memory, 8-byte aligned, NULL to leave out; the record's bytes are the same either way):
 *   d_r  [m][3] double: the residuals in the caller's order, +0 where not counted;
 *   d_GL [3][gz][gy][gx] double = sum_i (w_i * ((wz * wy) * wx)) * r_{i,d} over the counted landmarks whose support
 *        holds the control (wx = wx[i - i0] and so on): the derivative of S / 2 over the control points.
 * counted, rmax and every entry of d_r are defined to the bit.  S and Omega are within gamma_(m + 8) sum |term| of the
 * exact sums; each entry of GL within gamma_(k + 8) sum |term|, k the landmarks in that control's support.  The sums are
 * organised as follows, a function of the inputs only, without atomics, so that a call repeats its bytes: the host puts
 * the counted landmarks in the order of their cells (k0, j0, i0), i0 fastest, by a stable counting sort; S and Omega:
 * one lane per landmark in that order, per-workgroup partials of a grid of min(ceil(counted / 256), 128) workgroups,
 * then the slots in a fixed order; GL: one lane per control visits the at most 64 cells of its support in ascending
 * order and each cell's landmarks in ascending order, from +0.
 * sift3d_hip_ffd_landmarks: d_work of sift3d_amd_ffd_landmarks_work_bytes(m, gx, gy, gz) bytes, 16-byte aligned.  It
 * waits for `stream` once before it returns.  -1 before any device call on a NULL d_lattice, P, Q, d_work or d_record,
 * a lattice dimension < 4, a bad spacing, a non-finite A, m out of range, a non-finite Q or w, a negative w,
 * misalignment, an output (record, work, d_r, d_GL) that overlaps the lattice or another output.
 *
 * Evaluation (sift3d_hip_ffd_evaluate_landmarks): one evaluation of the MSD cost with the term, as the driver makes it
 * on level 0.  sift3d_hip_ffd_evaluate_masked's arguments and outputs, then `jacobian` with d_jac (the penalty's record,
 * GJ [3][gz][gy][gx] double at byte 32, then the penalty's work; NULL: no penalty, and jacobian must be 0), the landmarks,
 * landmark_weight and d_lm (the landmark record, GL [3][gz][gy][gx] double at byte 32, then the landmarks' work), both of
 * sift3d_amd_ffd_evaluate_landmarks_bytes(which = 1 / 0, ...) bytes, 8-byte aligned.  d_grad is the driver's formula
 * below with l = 0; landmark_weight == 0 (jacobian == 0) launches the combine without that term.  It waits for `stream`
 * once before it returns.  Refusals: those of the two entries it is made of.
 *
 * Driver (sift3d_amd_ffd_refine_landmarks_device).  sift3d_amd_ffd_refine_jacobian_device's arguments with their
 * meanings (bins == 0: the MSD, otherwise the mutual information; the masks may be NULL; jacobian >= 0, and `penalty`
 * may be NULL only when jacobian == 0: the penalty is then not evaluated at all), then P, Q, w, m as above,
 * landmark_weight (lambda, finite, >= 0) and landmarks_out, a host array of SIFT3D_AMD_FFD_MAX_TRAIL entries parallel
 * to result->trail.  The loop, levels, subdivision, step rule and stop reasons are that driver's, one loop in the code
 * too.  Level l uses P * 0.5^l and Q * 0.5^l (exact), the level's lattice for the inside test, and the level's A.  The
 * term is reported in level-0 units on every level: L = (4^l * S) / Omega and rmax * 2^l; L = 0 and no gradient term
 * when Omega == 0.
 *     E    = base_E + lambda * L
 *     grad = (float)(base_g + ((lambda * (2 * 4^l)) / Omega) * GL)
 * with base_E and base_g the double expressions of the existing drivers, to the letter ("Jacobian penalty").  With
 * lambda == 0 no term is added to either formula, L is still recorded, and lattice, field, trail (and `penalty`) are
 * the existing drivers' byte for byte.  The value pass runs in every evaluation; the adjoint runs where the image force
 * runs (every evaluation of the MSD, the MI driver's gradient step); S, Omega and rmax come to the host in the
 * evaluation's existing wait.  The inside test, the scaling and the ordering by cell are made once per level.
 * -1 before any device call on what that driver refuses (without `penalty` only when jacobian != 0), what
 * sift3d_hip_ffd_landmarks refuses of P, Q, w and m, a NULL landmarks_out, a landmark_weight that is not finite or is
 * negative.  d_work: sift3d_amd_ffd_refine_landmarks_work_bytes() bytes, 16-byte aligned: the Jacobian driver's layout,
 * then the landmark record, GL and the landmarks' work. */
#define SIFT3D_AMD_FFD_MAX_LANDMARKS 65536
#define SIFT3D_AMD_FFD_LANDMARKS_RECORD_BYTES 32
typedef struct {
    double L;                                       /* (4^l * S) / Omega, 0 when Omega == 0 */
    double rmax;                                    /* in level-0 voxels */
    uint64_t counted;
} sift3d_amd_ffd_landmark_term;
/* for bindings that restate them: sizeof the term (0), SIFT3D_AMD_FFD_LANDMARKS_RECORD_BYTES (1),
 * SIFT3D_AMD_FFD_MAX_LANDMARKS (2), SIFT3D_AMD_FFD_MAX_TRAIL (3); 0 otherwise */
SIFT3D_AMD_API size_t sift3d_amd_ffd_landmarks_struct_bytes(int which);
SIFT3D_AMD_API int sift3d_hip_ffd_points(const float *d_lattice, int gx, int gy, int gz, int dx, int dy, int dz,
                                         const double *A /*12 or NULL*/, const double *d_P, int m, double *d_T,
                                         void *stream);
/* bytes of d_work (0 for bad arguments) */
SIFT3D_AMD_API size_t sift3d_amd_ffd_landmarks_work_bytes(int m, int gx, int gy, int gz);
/* A, P, Q, w on the host */
SIFT3D_AMD_API int sift3d_hip_ffd_landmarks(const float *d_lattice, int gx, int gy, int gz, int dx, int dy, int dz,
                                            const double *A /*12 or NULL*/, const double *P, const double *Q,
                                            const double *w /*NULL: all 1*/, int m, void *d_work, void *d_record,
                                            double *d_r /*or NULL*/, double *d_GL /*or NULL*/, void *stream);
/* bytes of d_lm (which == 0) and of d_jac (which == 1); 0 for bad arguments */
SIFT3D_AMD_API size_t sift3d_amd_ffd_evaluate_landmarks_bytes(int which, int m, int ox, int oy, int oz, int dx, int dy,
                                                              int dz);
SIFT3D_AMD_API int
sift3d_hip_ffd_evaluate_landmarks(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                  const float *d_lattice, int gx, int gy, int gz, int dx, int dy, int dz,
                                  const double *A /*12 or NULL*/, double bending, float *d_field, void *d_record,
                                  float *d_grad, void *d_work, void *stream, const float *d_WF, const float *d_WM,
                                  double jacobian, void *d_jac /*NULL when jacobian == 0*/, const double *P,
                                  const double *Q, const double *w, int m, double landmark_weight, void *d_lm);
SIFT3D_AMD_API size_t
sift3d_amd_ffd_refine_landmarks_work_bytes(int ox, int oy, int oz, int nx, int ny, int nz, int dx, int dy, int dz,
                                           int levels, int m);
/* A [12], mi_out (NULL allowed when bins == 0), penalty (NULL allowed when jacobian == 0), P, Q, w and landmarks_out on
 * the host */
SIFT3D_AMD_API int
sift3d_amd_ffd_refine_landmarks_device(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny,
                                       int nz, const double *A, const sift3d_amd_ffd_refine_params *params,
                                       sift3d_amd_ffd_refine_result *result, float *d_lattice, float *d_field,
                                       void *d_work, void *stream, const float *d_WF, const float *d_WM, int bins,
                                       float lo_f, float hi_f, float lo_m, float hi_m, sift3d_amd_similarity *mi_out,
                                       double jacobian, sift3d_amd_ffd_penalty *penalty, const double *P,
                                       const double *Q, const double *w, int m, double landmark_weight,
                                       sift3d_amd_ffd_landmark_term *landmarks_out);

/* ------------------------------------------------------------------------ */
/* Dense descriptors: a 12-bin icosahedral gradient histogram per voxel      */
/* ------------------------------------------------------------------------ */
/* Upstream SIFT3D's dense descriptor image, non-rotating variant; the fork removed the code
 * (traces: dense_rotate, imtypes_private.h:222, sift.c:580,598).  PARITY UNPINNED against
 * upstream; pinned to this contract instead, built from the reference's per-voxel expressions.
 * Input I[nz][ny][nx] float (finite), voxel sizes (ux, uy, uz) > 0, window sigma > 0 (world units).
 * Output D[12][nz][ny][nx] float, planar, channel c = icosahedron vertex c (init_geometry order,
 * the order of the bins of a sparse descriptor's 12-bin histograms).  Float arithmetic, no contraction:
 *  1. gradient (IM_GET_GRAD_ISO, sift.c:140-145), neighbours outside clamped to the nearest voxel:
 *       gx = 0.5f * (I[min(x+1, nx-1)] - I[max(x-1, 0)]);  gx = gx * (1.0f / (float)ux);  same for y, z
 *  2. bin (icos_hist_bin, sift.c:1253-1290): m2 = gx*gx + gy*gy + gz*gz (left to right); when
 *     m2 < 1.1920928955078125e-6f all 12 values are +0.0f.  Else the first face in table order that
 *     cart2bary (sift.c:268-297) accepts; mag = sqrtf(m2), correctly rounded; the vertex whose
 *     barycentric bary_j is (cart2bary's vertex j, j = x, y, z) gets mag * bary_j, the other 9 channels
 *     +0.0f.  (The sparse descriptor's bins follow the reference's quirk Q1 -- every face of
 *     init_geometry swaps v[0] and v[1] but keeps idx[], so bary_x lands in the bin of the other
 *     vertex.  The dense image does not: channel c holds the weight of direction c, and mirroring the
 *     volume permutes the channels.)
 *  3. window: each channel through apply_Sep_FIR_filter (imutil.c:1127-1206), unit 1.0, the taps of
 *     init_Gauss_filter(sigma) (sift3d_amd_gauss_filter): x, then y, then z, unit_factor =
 *     (float)(1 / u_axis), the reference's edge rules -- the detector's blur of a level
 *  4. normalise (normalize_desc, sift.c:1402-1430, without truncation): per voxel
 *       s = sum_{c=0..11} (double)h_c * h_c  (in c order);  norm = sqrt(s) + DBL_EPSILON;
 *       inv = (float)(1.0 / norm);  D_c = h_c * inv      (an all-zero voxel stays all zero)
 * Arguments are checked before any device call: -1 on NULL pointers, dims <= 0, sigma or units not
 * positive and finite, nc != 1, d_out overlapping d_src or d_work. */
/* Stages (device buffers, asynchronous on `stream`, no allocation): steps 1 + 2 into d_out (12 planes of
 * nx*ny*nz floats); step 4 in place on 12 planes of n floats.  Step 3 is sift3d_hip_fir /
 * sift3d_hip_fir_yz_u1 per plane. */
SIFT3D_AMD_API int
sift3d_hip_dense_bin(const float *d_src, int nx, int ny, int nz, double ux, double uy, double uz, float *d_out,
                     void *stream);
SIFT3D_AMD_API int sift3d_hip_dense_normalize(float *d_hist, size_t n, void *stream);
/* device scratch of sift3d_amd_dense_descriptors_device: 2 * nx*ny*nz floats (0 for bad dims) */
SIFT3D_AMD_API size_t sift3d_amd_dense_work_floats(int nx, int ny, int nz);
/* the whole descriptor image on device buffers: d_out 12 * nx*ny*nz floats, d_work
 * sift3d_amd_dense_work_floats(nx, ny, nz) floats; units3 = (ux, uy, uz).  Asynchronous on `stream`, no
 * allocation, no host synchronisation. */
SIFT3D_AMD_API int
sift3d_amd_dense_descriptors_device(const float *d_src, int nx, int ny, int nz, const double *units3,
                                    double sigma, float *d_out, float *d_work, void *stream);
/* host image (nc == 1, its units); out: 12 * nx*ny*nz floats, planar.  Blocking. */
SIFT3D_AMD_API int
sift3d_amd_image_dense_descriptors(const sift3d_image *im, double sigma, float *out);

/* Rotation-invariant dense descriptors: upstream's dense_rotate variant (imtypes_private.h:222,
 * sift.c:580,598).  Each voxel's window is binned in the voxel's own eigen-frame, so the image follows
 * the anatomy when the volume is rotated.  Inputs as above: I[nz][ny][nx] float (finite), units > 0,
 * sigma > 0 (world units).  Output D[12][nz][ny][nx] float, planar, channel c = icosahedron vertex c
 * (no Q1 swap).  Float arithmetic, no contraction:
 *  R1. gradient g(q) = IM_GET_GRAD_ISO (sift.c:140-145), taken only at window voxels q, which all lie in
 *      1 <= x <= nx-2 (same for y, z): no clamping, the values of step 1 above.
 *  R2. orientation: at every voxel v, vcenter = ((float)x, (float)y, (float)z), assign_eig_ori(I,
 *      vcenter, sigma) (sift.c:926-1085) exactly:
 *      window IM_LOOP_SPHERE (sift.c:86-107), radius 3.0 * sigma (ori_rad_fctr; the loop bounds from
 *      floorf / ceilf of (float)(c -+ rad / (double)(float)u), clipped to 1 .. n-2; disp = ((float)q - c) *
 *      (float)u, sq = dx*dx + dy*dy + dz*dz in float, inside when !((double)sq > rad * rad)), scan order
 *      z, y, x; weight w = expf((float)(-0.5 * sq / (sigma * sigma))) (double expression, sift.c:972);
 *      sums A_ab += (double)g_a * g_b * w (six, double, left to right) and vd_win += g * w (three,
 *      float), in window order (sift.c:978-987);
 *      reject when |vd_win|^2 < (float)1e-10 (sift.c:997); eigen-decomposition s3d_eigen3 (cyclic
 *      Jacobi, sift3d_amd_host_eigen3; ascending L); reject when |L_i / L_{i+1}| > 0.9, i = 0, 1
 *      (sift.c:1011-1015); for i = 0, 1 the eigenvector of L_{2-i} as float, d = (double)(float dot of
 *      vd_win and it), sign +1 when d > 0 else -1, column i of R (sift.c:1017-1049); column 2 = column 0
 *      x column 1 in float (sift.c:1054-1059).  No corner threshold.  A rejected voxel gets R = I and
 *      keep = 0, a kept one keep = 1.
 *  R3. histogram: the same sphere, order and weights.  For each window voxel q (extract_descrip,
 *      sift.c:1497-1502): g' = g(q) * w (float, per component); gr = R^T g' (SIFT3D_MUL_MAT_RM_CVEC
 *      on the transpose, immacros.h:330: gr_a = R[0][a]*g'x + R[1][a]*g'y + R[2][a]*g'z, left to right);
 *      gr binned by step 2 above (the m2 threshold, the first face cart2bary accepts, mag * bary_j to
 *      vertex channel j); accumulated in float from +0, in window order.  R3 uses R whether kept or not.
 *  R4. normalise: step 4 above, unchanged (sift3d_hip_dense_normalize).
 * Edge cases: an axis shorter than 3 voxels empties every window (R = I, keep = 0, D = 0); a flat region
 * is rejected and its D is 0.  Cost grows with the window: about (4/3) pi (3 sigma)^3 / (ux uy uz) window
 * voxels per voxel, each visited once by R2 and once by R3.  Refused windows: more than 20000 voxels by
 * that estimate (about 3 sigma / u > 16.8 on an isotropic grid; each launch walks at least one tile's
 * whole window, so this bounds a launch's length), or more than 509 voxels from the centre on an axis.
 * Parity: R2 is pinned to the reference's assign_eig_ori through the oracle (orc_orient_slab with
 * corner_thresh 0).  R3 is this project's own contract: the fork has no dense code.
 * Arguments are checked before any device call: -1 on NULL pointers, dims <= 0, sigma or units not
 * positive and finite, nc != 1, an output overlapping the source, R or the work buffer. */
/* Stages (device buffers, asynchronous on `stream`, no allocation).  R2: d_R 9 planes of nx*ny*nz floats,
 * element (i, j) of R in plane 3i + j; d_keep nx*ny*nz bytes, or NULL.  R3: d_out 12 unnormalised planes,
 * from d_R.  Each stage is split into launches of bounded length for wide windows. */
SIFT3D_AMD_API int
sift3d_hip_dense_orient(const float *d_src, int nx, int ny, int nz, double ux, double uy, double uz, double sigma,
                        float *d_R, unsigned char *d_keep, void *stream);
SIFT3D_AMD_API int
sift3d_hip_dense_rotate_bin(const float *d_src, int nx, int ny, int nz, double ux, double uy, double uz,
                            double sigma, const float *d_R, float *d_out, void *stream);
/* device scratch of sift3d_amd_dense_descriptors_rotate_device: 9 * nx*ny*nz floats, R (0 for bad dims) */
SIFT3D_AMD_API size_t sift3d_amd_dense_rotate_work_floats(int nx, int ny, int nz);
/* R1-R4 on device buffers: d_out 12 * nx*ny*nz floats, d_work sift3d_amd_dense_rotate_work_floats floats.
 * Asynchronous on `stream`, no allocation, no host synchronisation. */
SIFT3D_AMD_API int
sift3d_amd_dense_descriptors_rotate_device(const float *d_src, int nx, int ny, int nz, const double *units3,
                                           double sigma, float *d_out, float *d_work, void *stream);
/* host image (nc == 1, its units); out: 12 * nx*ny*nz floats, planar.  Blocking. */
SIFT3D_AMD_API int
sift3d_amd_image_dense_descriptors_rotate(const sift3d_image *im, double sigma, float *out);

/* ------------------------------------------------------------------------ */
/* Dense demons refinement of a displacement field                          */
/* ------------------------------------------------------------------------ */
/* Multi-channel demons (Thirion's force with the symmetric, ESM gradient) moves a field until a moving feature
 * image, warped through it, agrees with a fixed one at every voxel.  No upstream counterpart: pinned to this
 * contract.  Inputs: fixed F[nc][nz][ny][nx], moving M[nc][mz][my][mx] (shapes may differ), nc >= 1, and a field
 * u[3][nz][ny][nx] on the fixed grid, a pull map in moving voxels ("Displacement fields").  Voxel units only.
 *
 * Force delta = force(F, W, u), W = M warped through u (LINEAR, fill 0; [nc][nz][ny][nx]).  Per fixed voxel p:
 *   1. inside(p): warp_field's inside test of q_d = (double) p_d + (double) u_d(p) against (mx, my, mz).  Not
 *      inside: delta(p) = +0.0f on all three channels, and p adds nothing to the statistics.
 *   2. d_c = F_c(p) - W_c(p) (float).
 *   3. d_e is the derivative along axis e by step 1 of the Jacobian above (numpy.gradient's rules on the fixed
 *      grid, float); g_ce = 0.5f * (d_e F_c(p) + d_e W_c(p)), the symmetric gradient.
 *   4. In double, c = 0 .. nc-1 in order, unfused, every sum from 0.0:
 *        num_e = sum_c (double) d_c * (double) g_ce
 *        s_g   = sum_c (((double) g_c0 * g_c0 + (double) g_c1 * g_c1) + (double) g_c2 * g_c2)
 *        s_d   = sum_c (double) d_c * d_c
 *   5. den = s_g + a2 * s_d, a2 = alpha * alpha (double); delta_e = den > 0 ? (float)(num_e / den) : +0.0f.
 * By Cauchy-Schwarz |num| <= sqrt(s_g) sqrt(s_d) and den >= 2 alpha sqrt(s_g) sqrt(s_d), so |delta(p)| <=
 * 1 / (2 alpha) voxel before rounding: alpha (Thirion's normaliser) caps the step.
 * Statistics of a call (SIFT3D_AMD_DEMONS_STATS_BYTES, 8-byte aligned): bytes 0-7 double sum = the sum of s_d
 * over the inside voxels, bytes 8-15 uint64 count = the number of inside voxels.  The sum is reduced from
 * per-workgroup partials in a fixed order (no float atomics): the same inputs give the same bits on every run;
 * the order of the sum is not part of the contract.
 *
 * Iteration k = 0 .. iterations-1, every stage on `stream`:
 *   1. W = sift3d_hip_warp_field(M, u, LINEAR, fill 0);
 *   2. delta, stats[k] = force(F, W, u);
 *   3. sigma_fluid > 0: each of delta's 3 channels blurred in place by the detector's blur (blur_level) with
 *      the taps of sift3d_amd_gauss_filter(sigma_fluid), units (1, 1, 1), unit 1.0 (step 3 of "Dense
 *      descriptors");
 *   4. u_d = u_d + delta_d per element (float add);
 *   5. sigma_diffusion > 0: each of u's 3 channels blurred the same way.
 * iterations == 0 leaves u untouched.
 *
 * Arguments are checked before any device call: -1 on NULL pointers, dims <= 0, nc < 1, iterations < 0, alpha
 * not positive and finite, a sigma negative or not finite, misalignment (d_stats and d_work 8 B, the rest 4 B),
 * an output (or the work buffer) that overlaps an input, the work buffer or another output.  Asynchronous on
 * `stream`, no allocation, no host synchronisation, 64-bit offsets. */
#define SIFT3D_AMD_DEMONS_STATS_BYTES 16
/* d_work of sift3d_hip_demons_force: the per-workgroup partials */
#define SIFT3D_AMD_DEMONS_FORCE_WORK_BYTES 32768
/* one force: d_F, d_W [nc][nz][ny][nx], d_u and d_step [3][nz][ny][nx], d_stats 16 B, d_work
 * SIFT3D_AMD_DEMONS_FORCE_WORK_BYTES */
SIFT3D_AMD_API int
sift3d_hip_demons_force(const float *d_F, int nx, int ny, int nz, const float *d_W, const float *d_u, int mx, int my,
                        int mz, int nc, double alpha, float *d_step, void *d_stats, void *d_work, void *stream);
/* device scratch of sift3d_amd_demons_device, in floats: the force's partials, W (nc planes), delta (3) and the
 * blur's two intermediates (0 for bad arguments) */
SIFT3D_AMD_API size_t sift3d_amd_demons_work_floats(int nx, int ny, int nz, int nc);
/* `iterations` iterations on device buffers: d_u in / out, d_stats 16 B per iteration (iteration k at 16 k) */
SIFT3D_AMD_API int
sift3d_amd_demons_device(const float *d_F, int nx, int ny, int nz, const float *d_M, int mx, int my, int mz, int nc,
                         float *d_u, int iterations, double alpha, double sigma_fluid, double sigma_diffusion,
                         float *d_work, void *d_stats, void *stream);

/* ------------------------------------------------------------------------ */
/* Field composition, exponential and inverse                               */
/* ------------------------------------------------------------------------ */
/* Fields are float [3][z][y][x] pull maps in the source grid's voxels, as in "Displacement fields".
 *
 * Composition sample.  u on grid (ux, uy, uz); v on the output grid (ox, oy, oz), its values in u-grid voxels.
 * Per output voxel p:
 *   1. q_d = (double) p_d + (double) v_d(p);
 *   2. inside: warp_field's inside test of q against u's grid;
 *   3. qc_d = min(max(q_d, 0), n_d - 1) in double: outside its grid u is extended by its nearest edge value (ITK's
 *      convention for composition and inversion); for inside voxels qc = q;
 *   4. s_d = the LINEAR sample of u_d at qc, warp_field's arithmetic word for word (one set of taps for the three
 *      channels).  For inside voxels s is bit-equal to warp_field(u, v, LINEAR);
 *   5. a NaN in any v_d(p) makes all three outputs the quiet NaN 0x7fc00000; such a voxel is not inside and adds
 *      nothing to the statistics.
 * Modes: SIFT3D_AMD_FIELD_COMPOSE: out_d = v_d + s_d (float add), i.e. w(p) = v(p) + u(p + v(p)), read through v,
 *   then through u.  SIFT3D_AMD_FIELD_INVERT: out_d = -s_d, one fixed-point step of the inverse of u.
 * Statistics (SIFT3D_AMD_FIELD_STATS_BYTES, 8-byte aligned) are those of the residual r = v + s (float) whatever
 * the mode, |r| = sqrt(((double) rx rx + (double) ry ry) + (double) rz rz): bytes 0-7 double sum of |r| and 8-15
 * double max of |r| (0 when there is no voxel) over the non-NaN voxels, 16-23 uint64 count of non-NaN voxels,
 * 24-31 uint64 count of inside voxels.  The sum is reduced from per-workgroup partials in a fixed order (no float
 * atomics), so a call repeats its bits; the order of the sum is not part of the contract; the max and the counts
 * are exact.  u is assumed finite.  d_out NULL: statistics only.  d_work (SIFT3D_AMD_FIELD_WORK_BYTES, the
 * partials) may be NULL when d_stats is.
 *
 * Exponential by scaling and squaring (K squarings, 0 <= K <= SIFT3D_AMD_FIELD_MAX_SQUARINGS):
 *   w_0 = v * 2^-K (float multiply), w_{k+1} = COMPOSE(u = w_k, v = w_k), exp(v) = w_K; K == 0 copies v.
 * Inverse by fixed-point iteration (N >= 0 iterations): d_w holds the initial iterate on the output grid and
 * receives w_N; w_{k+1} = INVERT(u, w_k), so a converged w satisfies w(q) = -u(q + w(q)).  Stats record k < N is
 * the residual of w_k (from INVERT pass k), record N that of the returned w_N (a final statistics-only pass): N + 1
 * records of SIFT3D_AMD_FIELD_STATS_BYTES.  For u fixed -> moving on the fixed grid, w lives on the moving grid
 * (ox, oy, oz = the moving shape) and maps moving -> fixed.  The iteration contracts when u's Lipschitz constant
 * L = max_d sum_e max |Delta_e u_d| over grid edges (the infinity-norm constant of the trilinear interpolant; the
 * clamp is 1-Lipschitz) is below 1: |w_N - w*| <= L^N |w_0 - w*|.
 *
 * Diffeomorphic demons (sift3d_amd_demons_device_ex): update SIFT3D_AMD_DEMONS_ADDITIVE is step 4 of "Dense demons
 * refinement" bit for bit (sift3d_amd_demons_device is it); SIFT3D_AMD_DEMONS_DIFFEOMORPHIC replaces step 4 with
 *   4'. e = exp(delta) with `squarings` squarings, then u <- COMPOSE(u, e): u_new(p) = e(p) + u(p + e(p))
 * (Vercauteren et al., Diffeomorphic demons, NeuroImage 2009).  Steps 1-3 and 5 are unchanged.  d_work holds
 * sift3d_amd_demons_work_floats_ex floats: sift3d_amd_demons_work_floats, plus 6 n for DIFFEOMORPHIC (u_new and the
 * exponential's second buffer).
 *
 * All entries are asynchronous on `stream`, allocate nothing, do not synchronise with the host, use 64-bit offsets
 * and check their arguments before any device call: -1 on NULL pointers, dims <= 0, K out of range, N < 0, an
 * unknown mode or update, misalignment (d_stats and d_work 8 B, fields 4 B), an output that overlaps an input, the
 * work buffer or another output (in-place composition included: neighbours are read). */
#define SIFT3D_AMD_FIELD_COMPOSE 0
#define SIFT3D_AMD_FIELD_INVERT 1
#define SIFT3D_AMD_FIELD_STATS_BYTES 32
#define SIFT3D_AMD_FIELD_WORK_BYTES 65536
#define SIFT3D_AMD_FIELD_MAX_SQUARINGS 20
#define SIFT3D_AMD_DEMONS_ADDITIVE 0
#define SIFT3D_AMD_DEMONS_DIFFEOMORPHIC 1
/* one composition sample pass; d_out [3][oz][oy][ox] may be NULL, d_stats may be NULL (then d_work may be too) */
SIFT3D_AMD_API int
sift3d_hip_field_compose(const float *d_u, int ux, int uy, int uz, const float *d_v, int ox, int oy, int oz,
                         float *d_out /*NULL*/, int mode, void *d_stats /*NULL*/, void *d_work, void *stream);
/* device scratch of sift3d_amd_field_exp_device: 3 ox*oy*oz floats (0 for bad dims) */
SIFT3D_AMD_API size_t sift3d_amd_field_exp_work_floats(int ox, int oy, int oz);
SIFT3D_AMD_API int
sift3d_amd_field_exp_device(const float *d_v, int ox, int oy, int oz, int squarings, float *d_out, float *d_work,
                            void *stream);
/* device scratch of sift3d_amd_field_invert_device: the partials plus 3 ox*oy*oz floats (0 for bad dims) */
SIFT3D_AMD_API size_t sift3d_amd_field_invert_work_floats(int ox, int oy, int oz);
/* d_w [3][oz][oy][ox] in / out; d_stats (iterations + 1) records */
SIFT3D_AMD_API int
sift3d_amd_field_invert_device(const float *d_u, int ux, int uy, int uz, float *d_w, int ox, int oy, int oz,
                               int iterations, float *d_work, void *d_stats, void *stream);
SIFT3D_AMD_API size_t sift3d_amd_demons_work_floats_ex(int nx, int ny, int nz, int nc, int update);
SIFT3D_AMD_API int
sift3d_amd_demons_device_ex(const float *d_F, int nx, int ny, int nz, const float *d_M, int mx, int my, int mz,
                            int nc, float *d_u, int iterations, double alpha, double sigma_fluid,
                            double sigma_diffusion, int update, int squarings, float *d_work, void *d_stats,
                            void *stream);

/* ------------------------------------------------------------------------ */
/* Multi-resolution demons                                                  */
/* ------------------------------------------------------------------------ */
/* Demons is local: one iteration moves the field by at most 1 / (2 alpha) voxel and finds only motion within about
 * a feature's width.  The pyramid solves on grids halved `levels - 1` times first, where a voxel's step is 2, 4, ...
 * fine voxels and an iteration costs 1/8, 1/64, ... of a fine one.
 * Grids (the detector's im_downsample_2x convention): coarse voxel i sits at fine voxel 2 i on every axis; a fine
 * axis of n voxels has c = (n + 1) / 2 (integer division) coarse ones, so an axis of 1 stays 1.  Displacements are in
 * voxels of the grid they index: a field's values halve going down and double going up.  Float arithmetic, unfused.
 *
 * Restriction (sift3d_hip_restrict2): src [nc][nz][ny][nx] -> dst [nc][cz][cy][cx], per channel the separable
 * binomial (1/4, 1/2, 1/4) on the taps 2 i - 1, 2 i, 2 i + 1, indices clamped onto the grid (edge replication):
 *   R_x(a)(i) = (0.25f * a[max(2 i - 1, 0)] + 0.5f * a[2 i]) + 0.25f * a[min(2 i + 1, n - 1)]
 * along x, then the same along y on the result, then along z, then dst = that * scale (float multiply, applied
 * last; 1.0f for an image, 0.5f for a field going down).  The weights are powers of two: only the adds round.
 * Consequences: a constant stays that constant; a function linear in the voxel index is sampled at 2 i exactly away
 * from the clamped faces; NaN and inf propagate as IEEE arithmetic has them (0.25f * inf + 0.5f * -inf is NaN).
 *
 * Field prolongation (sift3d_hip_field_prolong2): coarse [3][cz][cy][cx] -> fine [3][nz][ny][nx],
 * u_fine(p) = 2 L(u_coarse)(p / 2), L the linear interpolation, clamped at the high face where p / 2 passes the
 * last coarse voxel (even n).  p / 2 is an integer or a half, so per axis, for fine index p with i0 = p / 2 (integer
 * division) and i1 = min(i0 + (p & 1), c - 1):
 *   P_x(a)(p) = 0.5f * (a[i0] + a[i1])            (for even or clamped p this is 0.5f * (a + a))
 * along x, then the same along y on the result, then along z, then fine = 2.0f * that.  Consequences: a constant
 * field c becomes 2 c; the fine field at the even voxels, halved, is the coarse field bit for bit (barring
 * overflow); the field of an affine map on the coarse grid becomes the field of that map seen from the fine grid,
 * exactly when its values are dyadic.
 *
 * Pyramid (sift3d_amd_demons_multires_device): level 0 is the finest.  The caller passes, per level, the fixed and
 * moving feature stacks F_l [nc][nz_l][ny_l][nx_l], M_l [nc][mz_l][my_l][mx_l] and the iterations N_l; every
 * dimension of level l >= 1, fixed and moving, must be the half (n + 1) / 2 of level l - 1's.  How the stacks are made
 * is the caller's choice (restrict2 of level l - 1's, or features computed on the restricted volumes).
 *   1. u_0 = d_u; for l = 1 .. levels-1: u_l = restrict2(u_{l-1}, nc = 3, scale 0.5f).
 *   2. for l = levels-1 .. 0: N_l iterations of sift3d_amd_demons_device_ex on (F_l, M_l, u_l) with alpha, the sigmas
 *      (in level-l voxels), update and squarings as given; then, when l > 0, u_{l-1} = field_prolong2(u_l), which
 *      replaces u_{l-1}.
 * d_u receives u_0.  levels == 1 is sift3d_amd_demons_device_ex bit for bit.  With levels > 1 the start field only
 * enters through its restriction, a low-pass: what the binomial removes from it is lost (a spline's field is
 * smooth and loses little; a caller who wants the start field kept exactly passes levels = 1).
 * Statistics: one record of SIFT3D_AMD_DEMONS_STATS_BYTES per iteration in the order run, coarsest level first
 * (N_{levels-1} records, then N_{levels-2}, ...): sum_l N_l records (room for one when the sum is 0).
 * d_work holds sift3d_amd_demons_multires_work_floats floats: the finest level's demons scratch
 * (sift3d_amd_demons_work_floats_ex, which every level uses in turn) and the fields u_1 .. u_{levels-1}, each
 * rounded up to a multiple of 4 floats: about 3 n (1/8 + 1/64 + ...) more.
 *
 * All entries are asynchronous on `stream`, allocate nothing, do not synchronise with the host, use 64-bit offsets
 * and check their arguments before any device call: -1 on NULL pointers (a level's included), dims <= 0, nc < 1, a
 * scale that is not finite, levels outside [1, SIFT3D_AMD_DEMONS_MAX_LEVELS], dimensions that are not the halving
 * chain, a negative iteration count, the refusals of sift3d_amd_demons_device_ex for alpha, the sigmas, update and
 * squarings, misalignment (d_stats and d_work 8 B, the rest 4 B), an output that overlaps an input, the work buffer
 * or another output.  The transfers use 16-byte accesses on the fine side when nx % 4 == 0 and the buffers are
 * 16-byte (fine) and 8-byte (restrict2's dst) aligned; the result does not depend on it. */
#define SIFT3D_AMD_DEMONS_MAX_LEVELS 6
typedef struct {
    const float *d_F;          /* fixed features  [nc][nz][ny][nx] */
    int nx, ny, nz;
    const float *d_M;          /* moving features [nc][mz][my][mx] */
    int mx, my, mz;
    int iterations;            /* of this level, >= 0 */
} sift3d_amd_demons_level;
/* d_src [nc][nz][ny][nx] -> d_dst [nc][(nz+1)/2][(ny+1)/2][(nx+1)/2] */
SIFT3D_AMD_API int
sift3d_hip_restrict2(const float *d_src, int nx, int ny, int nz, int nc, float *d_dst, float scale, void *stream);
/* d_coarse [3][(nz+1)/2][(ny+1)/2][(nx+1)/2] -> d_fine [3][nz][ny][nx]; (nx, ny, nz) is the fine grid */
SIFT3D_AMD_API int
sift3d_hip_field_prolong2(const float *d_coarse, float *d_fine, int nx, int ny, int nz, void *stream);
/* device scratch of sift3d_amd_demons_multires_device, in floats, for a finest fixed grid (nx, ny, nz) (0 for bad
 * arguments) */
SIFT3D_AMD_API size_t
sift3d_amd_demons_multires_work_floats(int nx, int ny, int nz, int nc, int update, int levels);
/* level [levels] (host memory, level 0 the finest); d_u [3][nz_0][ny_0][nx_0] in / out */
SIFT3D_AMD_API int
sift3d_amd_demons_multires_device(const sift3d_amd_demons_level *level, int levels, int nc, float *d_u, double alpha,
                                  double sigma_fluid, double sigma_diffusion, int update, int squarings,
                                  float *d_work, void *d_stats, void *stream);

/* ------------------------------------------------------------------------ */
/* Log-domain demons                                                        */
/* ------------------------------------------------------------------------ */
/* Log-domain demons keeps a stationary velocity field v [3][nz][ny][nx] on the fixed grid and reads the moving
 * features through exp(v); the inverse map is exp(-v), one more exponential, and forces from both directions make
 * the result independent of which volume is called fixed (Vercauteren et al., Symmetric log-domain diffeomorphic
 * registration, MICCAI 2008).  No upstream counterpart: pinned to this contract.  Float arithmetic, unfused.
 *
 * Lie bracket and BCH update (sift3d_hip_field_bracket).  a, b, out are fields [3][oz][oy][ox] on one grid.  Per
 * voxel, g^a_de = d a_d / d x_e by step 1 of the Jacobian above (numpy.gradient's rules: (a[i+1] - a[i-1]) * 0.5f
 * inside, one-sided differences at the ends, 0 on an axis of length 1), g^b_de the same on b, then
 *   t_d  = (g^a_d0 * b_0 + g^a_d1 * b_1) + g^a_d2 * b_2
 *   s_d  = (g^b_d0 * a_0 + g^b_d1 * a_1) + g^b_d2 * a_2
 *   br_d = t_d - s_d
 * i.e. [a, b] = J_a b - J_b a; for linear fields a = A p, b = B p it is (A B - B A) p.  With it
 * exp(a + b + [a, b] / 2) ~ exp(a) o exp(b) in this library's composition order COMPOSE(u = exp a, v = exp b).
 * Modes: SIFT3D_AMD_FIELD_BRACKET: out_d = br_d.  SIFT3D_AMD_FIELD_BCH1: out_d = (a_d + b_d) + 0.5f * br_d.
 * NaN and inf propagate as IEEE arithmetic has them.  d_a == d_b is allowed (BRACKET then gives zeros wherever the
 * fields are finite); d_out must not overlap d_a or d_b (neighbours are read).
 *
 * Signed exponential (sift3d_amd_field_exp_signed_device): negate == 0 is sift3d_amd_field_exp_device bit for bit;
 * negate == 1 scales by w_0 = v * (-2^-K), the same float multiply with the sign flipped, then squares K times:
 * exp(-v).  K == 0 with negate gives v * -1.0f.
 *
 * Iteration, mode LOG (symmetric == 0), Kv = velocity_squarings in [0, SIFT3D_AMD_FIELD_MAX_SQUARINGS]:
 *   1. e = exp(v) with Kv squarings (Kv == 0: v itself);
 *   2. W = sift3d_hip_warp_field(M, e, LINEAR, fill 0);
 *   3. delta, stats[k] = force(F, W, e), the force of "Dense demons refinement" bit for bit;
 *   4. sigma_fluid > 0: delta blurred as in step 3 there;
 *   5. bch == 0: v_d = v_d + delta_d (float add); bch == 1: v <- BCH1(v, delta) (a = v, b = delta);
 *   6. sigma_diffusion > 0: each of v's 3 channels blurred as in step 5 there.
 * Mode SYMMETRIC (symmetric == 1) needs equal fixed and moving shapes at every level.  Steps 1-4 give delta_f; then
 * e- = exp(-v) (the signed exponential, Kv squarings), W_b = warp_field(F, e-), delta_b = force(M, W_b, e-) (its
 * statistics are discarded), the same fluid blur on delta_b; with n = -v (v * -1.0f),
 *   bch == 0: Z_f = v + delta_f, Z_b = n + delta_b;  bch == 1: Z_f = BCH1(v, delta_f), Z_b = BCH1(n, delta_b);
 *   5'. v_d = 0.5f * (Z_f,d - Z_b,d);
 * then step 6.  Exchanging F and M exchanges Z_f and Z_b bit for bit (every operation above commutes with exact
 * negation of its field argument), so the run started from -v ends at -v: equal bits but for the sign of zeros
 * (x - x is +0 in both runs).
 * Statistics: one SIFT3D_AMD_DEMONS_STATS_BYTES record per iteration, the forward force's.
 *
 * Pyramid (sift3d_amd_logdemons_device): that of "Multi-resolution demons" with v in place of u: restrict2 (scale
 * 0.5f) down, the iterations of each level coarsest first, field_prolong2 up (a velocity in voxels of its grid
 * rescales like a displacement).  levels == 1 is the flat run; the level table, the statistics' order and the
 * refusals are sift3d_amd_demons_multires_device's, plus bch or symmetric outside {0, 1}, Kv out of range, and
 * unequal fixed and moving shapes under SYMMETRIC.  iterations == 0 everywhere leaves v untouched (levels == 1).
 * d_work holds sift3d_amd_logdemons_work_floats floats; with n = nx*ny*nz of the finest level, pad4(x) = x rounded
 * up to a multiple of 4 and n_l the voxels of level l:
 *   pad4(8192 + 4 s + (nc + 14 + 6 s) n) + sum_{l = 1 .. levels-1} pad4(3 n_l),     s = symmetric
 * (the force's partials, with s the backward statistics; W (nc n), delta (3 n), the blur's intermediates (2 n), the
 * exponential's two buffers (6 n), the BCH output (3 n); with s delta_b and Z_b (6 n); then the coarser levels'
 * velocities).
 *
 * Out of scope: a start displacement field or affine map under the velocity (v starts from the caller's velocity
 * or zero); BCH terms beyond the first bracket; a device-side choice of Kv; the backward statistics; physical
 * spacing, multi-GPU.  (Masks: "Masks in demons" below.)
 *
 * Measured on an MI355X: on the 176^3 lattice case from zero, three levels, the forward error of
 * LOG is 1.0087 (median) and 1.0006 (p90) times the diffeomorphic update's, SYMMETRIC's 1.0086 and 1.0081; neither
 * exp(v) nor exp(-v) folds; exp(-v) is the inverse to a median of 0.164 voxel (forward 0.133).  At 512^3 the bracket
 * kernel takes 1.49 x the Jacobian kernel's time (the bound set for it: 36 / 16 = 2.25, the ratio of their bytes).
 *
 * All entries are asynchronous on `stream`, allocate nothing, do not synchronise with the host, use 64-bit offsets
 * and check their arguments before any device call (-1): NULL pointers, dims <= 0, an unknown mode, misalignment
 * (d_stats and d_work 8 B, the rest 4 B), an output that overlaps an input, the work buffer or another output. */
#define SIFT3D_AMD_FIELD_BRACKET 0
#define SIFT3D_AMD_FIELD_BCH1 1
SIFT3D_AMD_API int
sift3d_hip_field_bracket(const float *d_a, const float *d_b, int ox, int oy, int oz, float *d_out, int mode,
                         void *stream);
/* d_work: sift3d_amd_field_exp_work_floats floats */
SIFT3D_AMD_API int
sift3d_amd_field_exp_signed_device(const float *d_v, int ox, int oy, int oz, int squarings, int negate, float *d_out,
                                   float *d_work, void *stream);
/* device scratch of sift3d_amd_logdemons_device, in floats, for a finest fixed grid (nx, ny, nz): the formula above
 * (0 for bad arguments) */
SIFT3D_AMD_API size_t sift3d_amd_logdemons_work_floats(int nx, int ny, int nz, int nc, int symmetric, int levels);
/* level [levels] (host memory, level 0 the finest); d_v [3][nz_0][ny_0][nx_0] in / out */
SIFT3D_AMD_API int
sift3d_amd_logdemons_device(const sift3d_amd_demons_level *level, int levels, int nc, float *d_v, double alpha,
                            double sigma_fluid, double sigma_diffusion, int symmetric, int bch, int velocity_squarings,
                            float *d_work, void *d_stats, void *stream);

/* ------------------------------------------------------------------------ */
/* Masks in demons                                                          */
/* ------------------------------------------------------------------------ */
/* Regions of interest for the dense path: which fixed voxels the demons force counts.  A delta on "Dense demons
 * refinement" and "Masks"; everything not restated here is theirs, word for word.
 *
 * The masks: W_F [nz][ny][nx] on the fixed grid, W_M [mz][my][mx] on the moving grid, float32, one plane each whatever
 * nc.  Either may be NULL: all in.  A voxel is in when w >= 0.5f ("Masks"' rule: a NaN, a negative value and
 * nextafterf(0.5f, 0) are out; 0.5f, 1, 2 and +inf are in).
 *
 * The masked force delta = force_masked(F, W, u, W_F, W_M) replaces step 1 of the force by counted(p): all of
 *   - inside(p), the unmasked test;
 *   - W_F(p) is in;
 *   - W_M at the voxel floor(q_d + 0.5) per axis (double) is in, for the same q_d = (double) p_d + (double) u_d(p) that
 *     the inside test uses ("Resampling"'s NEAREST rule; for an inside q the voxel is on the grid).
 * A voxel that is not counted gets delta(p) = +0.0f on all three channels and adds nothing to the statistics.  Steps
 * 2 - 5 are unchanged; the statistics are the sum of s_d and the count over the counted voxels, through the unmasked partial
 * slots in the unmasked order.  The derivative stencils still read F and W at masked-out neighbours: the volumes must
 * be finite everywhere, masked-out voxels included; mask values need not be.  With both masks NULL, or both all in, a
 * masked entry writes the bytes of its unmasked counterpart.
 *
 * Iterations: step 2 of "Dense demons refinement" (ADDITIVE and DIFFEOMORPHIC) and step 3 of LOG use force_masked with
 * the level's masks; every other step is word for word.  The fluid and diffusion blurs are the unmasked ones: they
 * carry the field into masked-out voxels, where it is the smooth extension of its surroundings and no measurement.
 * With both sigmas 0 and the additive update a voxel that is never counted keeps its start bits (u + 0.0f; a start -0.0f
 * becomes +0.0f).  What F holds where the whole 3 x 3 x 3 neighbourhood of a voxel is out of W_F never reaches the
 * result: the stencil reaches one voxel and W does not depend on F.
 * SYMMETRIC: the backward force is force_masked(M, W_b, e-, W_M, W_F): the roles exchange with the volumes, W_M tested
 * at p and W_F at floor(p + e-(p) + 0.5).  Exchanging (F, W_F) with (M, W_M) therefore exchanges Z_f and Z_b bit for
 * bit, as the unmasked property does.
 * Levels: the caller passes the masks per level, as it passes the feature stacks; a mask's dimensions are those of its
 * level's fixed or moving grid; each pointer of each level may be NULL independently.  (sift3d_amd.api restricts the
 * float masks with sift3d_hip_restrict2, scale 1, level by level, never a thresholded copy, as "Masks"' drivers do.)
 * No new scratch: the work-float figures are the unmasked ones.
 *
 * Entries: sift3d_hip_demons_force_masked is sift3d_hip_demons_force with d_WF, d_WM at the end ("Masks"' convention).
 * sift3d_amd_demons_masked_device takes masks [levels] after the level table and the rest as
 * sift3d_amd_demons_multires_device (levels == 1: the flat run; masks == NULL: the unmasked entry bit for bit);
 * sift3d_amd_logdemons_masked_device the same over sift3d_amd_logdemons_device.  Refusals (-1, before any device call)
 * are the unmasked entries', and: a non-NULL mask that is not 4-byte aligned; a non-NULL mask that overlaps d_u / d_v,
 * d_step, d_stats or d_work.
 *
 * Out of scope: weighted (soft) masks; masks in the keypoint stages of registration and in label overlap; a
 * mask-aware (normalised) smoothing of the field. */
typedef struct {
    const float *d_WF;         /* fixed mask  [nz][ny][nx] of the level, or NULL */
    const float *d_WM;         /* moving mask [mz][my][mx] of the level, or NULL */
} sift3d_amd_demons_level_masks;
SIFT3D_AMD_API int
sift3d_hip_demons_force_masked(const float *d_F, int nx, int ny, int nz, const float *d_W, const float *d_u, int mx,
                               int my, int mz, int nc, double alpha, float *d_step, void *d_stats, void *d_work,
                               void *stream, const float *d_WF, const float *d_WM);
/* level [levels], masks [levels] or NULL (host memory, level 0 the finest); d_u [3][nz_0][ny_0][nx_0] in / out; d_work
 * sift3d_amd_demons_multires_work_floats floats */
SIFT3D_AMD_API int
sift3d_amd_demons_masked_device(const sift3d_amd_demons_level *level, const sift3d_amd_demons_level_masks *masks,
                                int levels, int nc, float *d_u, double alpha, double sigma_fluid,
                                double sigma_diffusion, int update, int squarings, float *d_work, void *d_stats,
                                void *stream);
/* the same for a velocity; d_work sift3d_amd_logdemons_work_floats floats */
SIFT3D_AMD_API int
sift3d_amd_logdemons_masked_device(const sift3d_amd_demons_level *level, const sift3d_amd_demons_level_masks *masks,
                                   int levels, int nc, float *d_v, double alpha, double sigma_fluid,
                                   double sigma_diffusion, int symmetric, int bch, int velocity_squarings,
                                   float *d_work, void *d_stats, void *stream);

/* ------------------------------------------------------------------------ */
/* Local cross-correlation                                                  */
/* ------------------------------------------------------------------------ */
/* The squared correlation of two volumes over a small window around every voxel (the CC metric of ANTs / SyN), its
 * exact derivative with respect to the warped volume as a demons-style force, and a driver that climbs it.  It is the
 * measure for a SPATIALLY VARYING intensity relation (bias fields, contrast uptake, drift along z), which the MSD
 * force follows and which one global gain and offset ("NCC affine refinement") cannot absorb.  No upstream
 * counterpart: PARITY UNPINNED, pinned to this contract and its numpy restatement (tests/lncc_restatement.py).
 *
 * Inputs.  Fixed F[nz][ny][nx]; W[nz][ny][nx], the moving volume warped onto the fixed grid (LINEAR, fill 0); the
 * field u[3][nz][ny][nx] that made W; the moving dims (mx, my, mz); optional masks W_F (fixed grid) and W_M (moving
 * grid) with the conventions of "Masks in demons"; radius r in [1, SIFT3D_AMD_LNCC_MAX_RADIUS].  One channel.  Voxel
 * units.  F and W must be finite.
 *
 * Validity.  v(p) = 1 where p is counted by k_demons_force<true>'s rule, word for word: inside(p) (warp_field's test
 * of q_d = (double) p_d + (double) u_d(p) against (mx, my, mz)), W_F(p) in, W_M at floor(q_d + 0.5) in; a NULL mask is
 * all in.  Elsewhere v(p) = 0.
 *
 * Window sums.  N(p) is the set of grid voxels q with |q_d - p_d| <= r on every axis, clipped to the grid.  For a
 * per-voxel double t, box(t)(p) is summed separably in three steps: the x sums over the offsets -r .. r ascending, the
 * y sums of those ascending, the z sums of those ascending.  Every sum starts from +0.0, an off-grid position adds
 * +0.0, additions are unfused.  THIS ORDER IS PART OF THE CONTRACT: it makes the outputs comparable byte for byte.
 * The six sums, with the floats promoted to double first so that every product is exact:
 *   n = box(v), sf = box(v F), sw = box(v W), sff = box(v F F), sww = box(v W W), sfw = box(v F W)
 * where a voxel with v = 0 contributes +0.0 to each whatever F and W hold there (a select, not a multiply).
 *
 * Per voxel, in double, in this written order:
 *   A = sfw - (sf * sw) / n,  B = sff - (sf * sf) / n,  C = sww - (sw * sw) / n
 * p is COUNTED when v(p) = 1, n >= 2, B > tau * sff and C > tau * sww, tau = 2^-30: a window that is flat in either
 * volume carries no correlation, and the relative test keeps the rule free of the intensity scale.  Counted voxels get
 *   cc = (A * A) / (B * C),  a = (2 * A) / (B * C),  b = (2 * cc) / C,  mf = sf / n,  mw = sw / n
 * and uncounted ones cc = a = b = 0.  cc is the SQUARED correlation: a locally inverted contrast scores like a direct
 * one (cc = 1 for W = alpha F + beta with alpha of either sign).
 *
 * Outputs of the statistics pass (sift3d_hip_lncc): the optional map d_cc, float [nz][ny][nx] = (float) cc; the
 * optional coefficient volumes d_coef, DOUBLE [4][nz][ny][nx] = a, a * mf, b, b * mw (+0.0 where uncounted; double
 * because a scales with 1 / intensity^2 and leaves float's range on subnormal and huge content); and d_stats, a
 * record with the layout and reduction rule of SIFT3D_AMD_DEMONS_STATS_BYTES: bytes 0-7 the double sum of cc over the
 * counted voxels, bytes 8-15 the uint64 count; per-workgroup partials reduced in a fixed order, no float atomics; the
 * order of that one sum is not part of the contract.
 *
 * Exact gradient and force (sift3d_hip_lncc_force).  With validity held fixed, d cc(p) / d W(q) = a(p) (F(q) - mf(p))
 * - b(p) (W(q) - mw(p)) for valid q in N(p).  Windows are symmetric, so the derivative of sum_p cc(p) is
 *   g(q) = (F(q) * box(a)(q) - box(a mf)(q)) - (W(q) * box(b)(q) - box(b mw)(q))
 * in double, with that grouping and the same box order.  The force is phi_e(q) = (float)(g(q) * (double) d_e W(q)) at
 * voxels with v(q) = 1 and +0.0f elsewhere; d_e is the derivative of "Dense demons refinement" step 3
 * (numpy.gradient's rules on the fixed grid, in float).  Moving u along +phi increases the mean cc.
 *
 * Normalisation of a field to a step length (sift3d_hip_field_normalize): m2 = max_p (((double) phi_x^2 +
 * (double) phi_y^2) + (double) phi_z^2), exact and order-free; s = (float)(step / sqrt(m2)); every component is
 * replaced by s * phi_e (float multiply).  m2 == 0 leaves the field as it is.  No host synchronisation: the scale is
 * read from device memory by the kernel that applies it.  The field is assumed finite.
 *
 * Iteration k (sift3d_amd_demons_lncc_device), every stage on `stream`:
 *   1. W = sift3d_hip_warp_field(M, u, LINEAR, fill 0);
 *   2. the statistics, giving the coefficients and stats[k];
 *   3. phi = the force;
 *   4. sigma_fluid > 0: phi blurred exactly as step 3 of "Dense demons refinement";
 *   5. phi normalised to `step` voxels (positive and finite);
 *   6. ADDITIVE: u += phi.  DIFFEOMORPHIC: u <- COMPOSE(u, exp(phi)) with `squarings` squarings, step 4' of
 *      "Diffeomorphic demons" word for word;
 *   7. sigma_diffusion > 0: u blurred as step 5 there.
 * stats[k] is therefore the statistic before iteration k's update.  Levels, restriction and prolongation follow
 * "Multi-resolution demons" unchanged (levels == 1 is the flat run); the caller passes the masks per level as in
 * "Masks in demons" (masks == NULL: none).  The radius is in voxels of the level it runs on.
 * d_work of the driver holds sift3d_amd_demons_lncc_work_floats floats: with n the finest level's voxels,
 * pad4(12292 + 15 n (+ 6 n for DIFFEOMORPHIC)) + sum_{l >= 1} pad4(3 n_l) (the partials and the normalisation's work;
 * the coefficients, 8 n; v, W, phi, the blur's intermediates; u_new and the exponential's second buffer).
 *
 * Refusals, -1 before any device call: NULL pointers (d_cc, d_coef of the statistics pass and the masks may be NULL),
 * dims <= 0, radius out of range, step not positive and finite, the sigmas', update's, squarings' and levels' rules of
 * the demons drivers, misalignment (d_stats, d_work and doubles 8 B, floats 4 B), any output or the work buffer
 * overlapping an input, a mask or another output.  All entries are asynchronous on `stream`, allocate nothing, do no
 * host synchronisation and use 64-bit offsets.
 *
 * Out of scope: LNCC in the log-domain and symmetric updates, in FFD and in the affine stage; more than one channel;
 * Gaussian windows, or a signed (un-squared) correlation; radii above 4; physical or anisotropic spacing; multi-GPU;
 * any convergence test that stops the iteration early. */
#define SIFT3D_AMD_LNCC_MAX_RADIUS 4
/* the per-workgroup partials at the head of the two passes' d_work */
#define SIFT3D_AMD_LNCC_PARTIAL_BYTES 32768
/* d_work of sift3d_hip_field_normalize: the partial maxima, then m2 (double) and s (float) */
#define SIFT3D_AMD_FIELD_NORMALIZE_WORK_BYTES 16400
/* d_work of sift3d_hip_lncc and sift3d_hip_lncc_force, in bytes: the partials and v (0 for bad dims) */
SIFT3D_AMD_API size_t sift3d_amd_lncc_work_bytes(int nx, int ny, int nz);
/* the statistics pass: d_F, d_W [nz][ny][nx], d_u [3][nz][ny][nx], d_WF, d_WM masks or NULL, d_cc float [nz][ny][nx]
 * or NULL, d_coef double [4][nz][ny][nx] or NULL, d_stats 16 B */
SIFT3D_AMD_API int
sift3d_hip_lncc(const float *d_F, int nx, int ny, int nz, const float *d_W, const float *d_u, int mx, int my, int mz,
                const float *d_WF, const float *d_WM, int radius, float *d_cc /*NULL*/, double *d_coef /*NULL*/,
                void *d_stats, void *d_work, void *stream);
/* the force: d_coef as the statistics pass wrote it (same inputs, masks and radius), d_force [3][nz][ny][nx] */
SIFT3D_AMD_API int
sift3d_hip_lncc_force(const float *d_F, int nx, int ny, int nz, const float *d_W, const float *d_u, int mx, int my,
                      int mz, const float *d_WF, const float *d_WM, int radius, const double *d_coef, float *d_force,
                      void *d_work, void *stream);
/* d_field [3][nz][ny][nx] in / out; d_work SIFT3D_AMD_FIELD_NORMALIZE_WORK_BYTES, 8-byte aligned */
SIFT3D_AMD_API int
sift3d_hip_field_normalize(float *d_field, int nx, int ny, int nz, double step, void *d_work, void *stream);
/* device scratch of sift3d_amd_demons_lncc_device, in floats, for a finest fixed grid (nx, ny, nz) (0 for bad
 * arguments) */
SIFT3D_AMD_API size_t sift3d_amd_demons_lncc_work_floats(int nx, int ny, int nz, int update, int levels);
/* level [levels], masks [levels] or NULL (host memory, level 0 the finest; one channel per volume); then the radius
 * where sift3d_amd_demons_masked_device has nc and the step where it has alpha; d_u [3][nz_0][ny_0][nx_0] in / out;
 * d_stats 16 B per iteration in the order run, coarsest level first (room for one when there is none) */
SIFT3D_AMD_API int
sift3d_amd_demons_lncc_device(const sift3d_amd_demons_level *level, const sift3d_amd_demons_level_masks *masks,
                              int levels, int radius, float *d_u, double step, double sigma_fluid,
                              double sigma_diffusion, int update, int squarings, float *d_work, void *d_stats,
                              void *stream);

/* ------------------------------------------------------------------------ */
/* MIND self-similarity descriptors                                         */
/* ------------------------------------------------------------------------ */
/* The self-similarity context of the modality-independent neighbourhood descriptor (MIND-SSC: Heinrich et al.,
 * MICCAI 2013; MIND: Heinrich et al., MedIA 2012): every voxel gets 12 channels that say how much the patches around
 * it resemble EACH OTHER within the same volume.  The channels of two volumes are therefore comparable with a plain
 * squared difference whatever relates the two intensity scales, an inverted contrast included, and the stack
 * [12][nz][ny][nx] is a drop-in for the channel stacks of "Multi-channel free-form deformation" and of every demons
 * update.  No upstream counterpart: PARITY UNPINNED, pinned to this contract and its numpy restatement
 * (tests/mind_restatement.py); the device reproduces every output but the one sum of d_stats bit for bit.
 *
 * Inputs.  I[nz][ny][nx], float32 and finite; the patch radius r in [1, SIFT3D_AMD_MIND_MAX_RADIUS]; the dilation d
 * in [1, SIFT3D_AMD_MIND_MAX_DILATION]; the clamps 0 <= vlo <= vhi of the variance (vhi may be +inf).  Voxel units.
 *
 * Neighbours and pairs.  The six neighbours of a voxel are, in (x, y, z),
 *   n0 = (+d, 0, 0), n1 = (-d, 0, 0), n2 = (0, +d, 0), n3 = (0, -d, 0), n4 = (0, 0, +d), n5 = (0, 0, -d).
 * Channel k = 0 .. 11 is the pair (i, j) of this list, in this order:
 *   (0,2) (0,3) (0,4) (0,5) (1,2) (1,3) (1,4) (1,5) (2,4) (2,5) (3,4) (3,5)
 * the twelve pairs at distance sqrt(2) d; the three opposite pairs (distance 2 d) are left out.
 *
 * Per-voxel distances.  s_i(q) = I(clamp(q + n_i)), every coordinate clamped to the grid (replicated edges);
 * e_k(q) = ((double) s_i(q) - (double) s_j(q))^2, the difference and the square formed in double, unfused;
 * D_k(p) = box_r(e_k)(p) by the rule "Window sums" of "Local cross-correlation", word for word: windows clipped to the
 * grid, x then y then z, each ascending from +0.0, an off-grid position adding +0.0, additions unfused.
 *
 * Variance and clamp, in double, in this written order:
 *   S = D_0 + D_1 + ... + D_11 ascending from +0.0,  V = S / 12.0,  Vc = min(max(V, vlo), vhi),
 *   Dmin = min_k D_k,  t_k = (D_k - Dmin) / Vc, except that Vc == 0 gives t_k = 0
 * (a flat neighbourhood gives twelve exact ones).  Subtracting Dmin is the usual normalisation by the largest
 * channel: the largest channel of every voxel is exactly 1.0f.
 *
 * Descriptor.  out_k(p) = (float) cexp(t_k), where cexp(t) is the contract's exponential of -t, a fixed sequence of
 * double operations (multiplies and adds separate, nothing fused) that numpy reproduces bit for bit:
 *   t >= 104 gives +0.0 (exp(-104) is below half the smallest float);
 *   otherwise y = t * SIFT3D_AMD_MIND_LOG2E, n = floor(y), f = y - n (exact, 0 <= f < 1),
 *   p = c_10;  p = p * f + c_k for k = 9, 8, ..., 0  (Horner; 2^-f by its Taylor polynomial of degree 10),
 *   cexp = p * 2^-n (the exact power of two; n <= 150, so nothing leaves the normal doubles).
 * The coefficients c_k = (-ln 2)^k / k!, rounded to double:
 *   c_0  =  0x1.0000000000000p+0    c_1 = -0x1.62e42fefa39efp-1    c_2 =  0x1.ebfbdff82c58fp-3
 *   c_3  = -0x1.c6b08d704a0c0p-5    c_4 =  0x1.3b2ab6fba4e77p-7    c_5 = -0x1.5d87fe78a6731p-10
 *   c_6  =  0x1.430912f86c787p-13   c_7 = -0x1.ffcbfc588b0c7p-17   c_8 =  0x1.62c0223a5c824p-20
 *   c_9  = -0x1.b5253d395e7c4p-24   c_10 = 0x1.e4cf5158b8ecap-28
 * and SIFT3D_AMD_MIND_LOG2E = 0x1.71547652b82fep+0.  The series alternates, so its truncation error is below the first
 * term left out, (ln 2)^11 / 11! = 4.4e-10; with the roundings of the doubles (1e-15) and the one rounding to float
 * the result is within 1 ulp of the float nearest exp(-t).  cexp(0) = 1 exactly.
 *
 * Invariance.  The descriptor is unchanged under I -> a I + b for either sign of a, provided vlo and vhi are scaled
 * by a^2 (every D_k and V scale with a^2, t_k does not); it is EXACTLY unchanged, the same bytes, for a a power of two
 * and b = 0 while nothing under- or overflows.
 *
 * Outputs, each optional (NULL), at least one given: d_out, float [12][nz][ny][nx], the descriptor; d_D, double
 * [12][nz][ny][nx], the distances D_k; d_V, double [nz][ny][nx], the UNCLAMPED V; d_stats, 16 bytes with the layout
 * and reduction rule of SIFT3D_AMD_DEMONS_STATS_BYTES: bytes 0-7 the double sum of V over all voxels, bytes 8-15 the
 * uint64 voxel count; per-workgroup partials reduced in a fixed order, no float atomics; the order of that one sum
 * is not part of the contract.  (The mean of V is what the clamps are usually stated against: vlo = 1e-3 mean,
 * vhi = 1e3 mean.)
 *
 * d_work holds sift3d_amd_mind_work_bytes bytes (the partials).
 *
 * Refusals, -1 before any device call: NULL d_src or d_work, or all four outputs NULL; dims <= 0; radius or dilation
 * out of range; vlo negative or NaN, vhi < vlo or NaN; misalignment (doubles, d_stats and d_work 8 B, floats 4 B);
 * any output or the work buffer overlapping the input or another output.  The entry is asynchronous on `stream`,
 * allocates nothing, does no host synchronisation and uses 64-bit offsets.
 *
 * Out of scope: the plain six-channel MIND; Gaussian patch weights; radii above 2; physical or anisotropic spacing;
 * 4-D input; MIND together with the LNCC force, with mutual information, and in the affine stage; reorientation of
 * the neighbourhood under the deformation; multi-GPU. */
#define SIFT3D_AMD_MIND_CHANNELS 12
#define SIFT3D_AMD_MIND_MAX_RADIUS 2
#define SIFT3D_AMD_MIND_MAX_DILATION 4
#define SIFT3D_AMD_MIND_LOG2E 0x1.71547652b82fep+0
/* d_work of sift3d_hip_mind_ssc, in bytes: the per-workgroup partials (0 for bad dims) */
SIFT3D_AMD_API size_t sift3d_amd_mind_work_bytes(int nx, int ny, int nz);
/* d_src [nz][ny][nx]; d_out float [12][nz][ny][nx], d_D double [12][nz][ny][nx], d_V double [nz][ny][nx], d_stats
 * 16 B: each may be NULL, not all */
SIFT3D_AMD_API int
sift3d_hip_mind_ssc(const float *d_src, int nx, int ny, int nz, int radius, int dilation, double vlo, double vhi,
                    float *d_out /*NULL*/, double *d_D /*NULL*/, double *d_V /*NULL*/, void *d_stats /*NULL*/,
                    void *d_work, void *stream);

/* ------------------------------------------------------------------------ */
/* Block matching                                                            */
/* ------------------------------------------------------------------------ */
/* Rigid / affine registration by block matching with a trimmed least-squares fit (Ourselin et al. 2001, the scheme of
 * NiftyReg's reg_aladin): every 4^3 block of the fixed volume looks for its best-correlated position in the warped
 * moving volume inside a search cube, the matched point pairs go to a least-trimmed-squares (LTS) fit, and this is
 * repeated coarse to fine.  It needs no keypoints, tolerates a spatially varying gain (the score is a local
 * correlation) and trims outliers instead of averaging them in.  No upstream counterpart: PARITY UNPINNED, pinned to
 * this contract and its numpy restatement (tests/block_match_restatement.py); the device records bit for bit.
 *
 * Inputs (sift3d_hip_block_match).  F[nz][ny][nx], the fixed volume; W[nz][ny][nx], the moving volume already warped
 * onto the fixed grid; both finite float32, voxel units.  Optional float masks V_F and V_W on the same grid: a voxel
 * is in where w >= 0.5f (the rule of "Masks"); NULL is all in.  Radius R in [1, SIFT3D_AMD_BLOCK_MAX_RADIUS].
 *
 * Blocks.  Edge 4: block (bx, by, bz) covers voxels 4 b .. 4 b + 3 on every axis; nb_d = n_d / 4 (integer division),
 * trailing voxels belong to no block; -1 when any nb_d == 0.  The block's voxel i = x + 4 y + 16 z (local), 0 .. 63.
 * Candidates.  d = (dx, dy, dz) in [-R, R]^3, k = ((dz + R)(2R + 1) + (dy + R))(2R + 1) + (dx + R).
 *
 * Sums, all in double, each from +0.0 with i ascending and one add per term:
 *   sF = sum (double) F_i, sFF = sum (double) F_i (double) F_i; per candidate, with W_i the voxel of W at the block's
 *   voxel i + d:  sW, sWW, sFW = sum (double) F_i (double) W_i.
 * A product of two floats is exact in double, so the contract is the same with and without fused multiply-add.
 *   vF = sFF - (sF sF) / 64,  vW = sWW - (sW sW) / 64,  c = sFW - (sF sW) / 64,  cc = (c c) / (vF vW)  (that grouping)
 *
 * Validity.  A block is valid when all 64 voxels are in V_F and vF > sFF 2^-40 (a relative floor: below it the
 * variance of float data is rounding noise; an all-zero block fails it since 0 > 0 is false).  A candidate is valid
 * when the shifted block lies wholly inside the grid, all 64 of its W voxels are in V_W and vW > sWW 2^-40.  A valid
 * block without a valid candidate is invalid.
 * Choice.  The valid candidate of greatest cc (compared as doubles); equal cc: the smaller dx^2 + dy^2 + dz^2, then
 * the smaller k.
 * Sub-voxel step, in double.  Per axis a, c0 the winner's cc and c-, c+ those of its two neighbours along a: when both
 * neighbours lie in the search cube and are valid candidates and den = (c- - 2 c0) + c+ < 0, the offset is
 * o_a = 0.5 (c- - c+) / den clamped to [-0.5, 0.5]; otherwise o_a = 0.  (Without this step the driver below stalls
 * near 0.8 voxel: once most kept blocks report displacement 0 the trimmed fit keeps exactly those.)
 *
 * Outputs, planar over [nbz][nby][nbx]: d_disp float [3] (x, y, z) = (float) ((double) d_a + o_a), 0 for an invalid
 * block; d_cc float = (float) cc, -1.0f invalid; d_var DOUBLE = vF, the driver's selection key, 0.0 invalid (double:
 * vF of huge content leaves float's range).
 * Asynchronous on `stream`, allocates nothing, no host synchronisation, 64-bit offsets.  This implementation needs no
 * work buffer: sift3d_amd_block_match_work_bytes is 0 and d_work may be NULL; it is never read or written.
 * -1 before any device call on NULL pointers (the masks and d_work may be NULL), dims <= 0 or any dim < 4, R out of
 * range, misalignment (d_var 8 B, floats 4 B), an output overlapping an input, a mask or another output.
 *
 * Trimmed fit (sift3d_amd_fit_trimmed; host).  n point pairs src_i -> dst_i (n x 3 doubles each), a model
 * (TRANSLATION, RIGID, AFFINE) and per-axis scales S_src, S_dst (NULL = 1): with x = S_src src and y = S_dst dst the
 * model y ~ L x + t is fitted and returned as T = S_dst^-1 [L | t] S_src (3 x 4, row-major), so RIGID is rigid in
 * physical space for anisotropic voxels.  TRANSLATION: L = I, t the difference of the centroids.  RIGID: the
 * least-squares rotation about the centroids by Horn's unit quaternion (the dominant eigenvector of the 4 x 4 matrix
 * of the cross-covariance, cyclic Jacobi), so det L = +1 always, also for reflection-prone sets.  AFFINE: the normal
 * equations of the centred points, solved in double.  Sums run serially in index order (the result does not depend
 * on the thread count); only the residuals are computed in an OpenMP region.
 * LTS loop.  1. fit on all n; 2. r_i = |L x_i + t - y_i|^2; 3. keep the k = max(ceil(keep n), n_min) smallest, ties
 * to the lower index, n_min = 1 / 3 / 4; 4. stop when the kept set equals the set of the last fit or after max_iter
 * refits, else refit on the kept set and go to 2.  `used` marks the pairs the returned T was fitted to; *iterations
 * is the number of refits.
 * -1 on NULL pointers (scales, used may be NULL), n < n_min, an unknown model, keep outside (0, 1], max_iter < 0,
 * non-finite points, scales not positive and finite, or a degenerate set in any fit: with l1 >= l2 >= l3 the
 * eigenvalues of the scatter matrix of the fitted x about their centroid, RIGID refuses l2 <= 1e-10 l1 (collinear),
 * AFFINE l3 <= 1e-10 l1 (coplanar), both l1 == 0; RIGID checks the y likewise.  TRANSLATION has no degenerate set.
 *
 * Driver (sift3d_amd_block_register_device).  Fixed F (ox, oy, oz) and moving M (nx, ny, nz) on the device, optional
 * masks, the start pull map A (fixed voxel -> moving voxel, sift3d_hip_warp_affine's convention).  Levels follow
 * sift3d_amd_affine_refine_device word for word: volumes and FLOAT masks by sift3d_hip_restrict2 at scale 1, A[:][3]
 * halved going down a level and doubled going up, the coarsest level first.  Every level's fixed grid must be >= 8 on
 * every axis, else -1.  Per iteration on a level:
 *   1. W = warp_affine(M, A, LINEAR, fill 0);
 *   2. V_W = warp_affine(the level's moving mask, or a volume of ones, A, NEAREST, fill 0);
 *   3. sift3d_hip_block_match(F, W, V_F = the level's fixed mask or NULL, V_W, radius);
 *   4. the three records to the host and ONE wait for the stream (the trade of sift3d_amd_affine_refine_device);
 *   5. of the valid blocks (cc >= 0) the ceil(keep_blocks n_valid) of largest d_var, ties to the lower block index;
 *   6. pairs in block-index order: src_i = the block's centre (4 b + 1.5 per axis), dst_i = A (src_i + disp_i) in
 *      warp_affine's order of operations;
 *   7. A' = sift3d_amd_fit_trimmed(src, dst, model, keep_inliers, 20, spacing_fixed, spacing_moving) (the spacings
 *      of level 0 serve every level: both double per level, which leaves T unchanged);
 *   8. fewer than n_min valid blocks or a refused fit: FAILED, A stays, the level ends.  Else move = the largest
 *      distance |A' p - A p| over the 8 corners p of the level's fixed grid, A = A'; move < tol: CONVERGED; the
 *      level's `iterations` done: ITERATIONS; else 1.
 * The result holds the final A (also written to A_io), one trail entry per iteration in the order run (level, the A
 * it started from and the A it produced (the start again when FAILED), n_valid, n_selected, n_used, the mean cc over
 * the used pairs, the rms of their residuals |L x + t - y| in the fit's scaled units, the corner move; the last three
 * NaN when FAILED) and the stop reason of level 0.  params == NULL takes the defaults below.
 * d_work holds sift3d_amd_block_register_work_floats floats, 8-byte aligned: with n_l, m_l the voxels of the fixed and
 * moving grid on level l and b_0 the blocks of level 0,
 *   pad4(6 b_0) + 2 pad4(n_0) + [no moving mask: pad4(m_0)] + sum_{l >= 1} (pad4(n_l) + pad4(m_l)
 *   + [fixed mask: pad4(n_l)] + [moving mask: pad4(m_l)])
 * (the records: var, disp, cc; W; V_W; the ones; the level volumes and masks).  The host copies of the records are
 * allocated and freed by the call.
 * -1 before any device call on NULL pointers, dims <= 0, a level's fixed grid below 8, a non-finite A, an unknown
 * model, levels outside [1, SIFT3D_AMD_DEMONS_MAX_LEVELS], iterations outside [1, SIFT3D_AMD_BLOCK_MAX_ITERATIONS],
 * radius out of range, keep_blocks or keep_inliers outside (0, 1], tol < 0 or not finite, spacings not positive and
 * finite, misalignment (d_work 8 B, volumes 4 B), a work buffer that overlaps a volume or mask.
 *
 * Out of scope: block edges other than 4, overlapping blocks, search steps other than 1; skipping low-variance
 * blocks on the device; a similarity (7-parameter) model; non-affine start transforms; more than one channel;
 * multi-GPU; wiring into the keypoint and FFD registration pipelines. */
#define SIFT3D_AMD_BLOCK_MAX_RADIUS 6
#define SIFT3D_AMD_BLOCK_MAX_ITERATIONS 64          /* per level */
#define SIFT3D_AMD_BLOCK_MAX_TRAIL (6 * SIFT3D_AMD_BLOCK_MAX_ITERATIONS)       /* SIFT3D_AMD_DEMONS_MAX_LEVELS levels */
#define SIFT3D_AMD_MODEL_TRANSLATION 0
#define SIFT3D_AMD_MODEL_RIGID 1
#define SIFT3D_AMD_MODEL_AFFINE 2
#define SIFT3D_AMD_BLOCK_STOP_CONVERGED 0
#define SIFT3D_AMD_BLOCK_STOP_ITERATIONS 1
#define SIFT3D_AMD_BLOCK_STOP_FAILED 2
/* bytes of d_work for sift3d_hip_block_match: 0, this implementation needs none */
SIFT3D_AMD_API size_t sift3d_amd_block_match_work_bytes(int nx, int ny, int nz, int radius);
/* d_F, d_W [nz][ny][nx]; d_VF, d_VW masks or NULL; d_disp float [3][nbz][nby][nbx], d_cc float and d_var double
 * [nbz][nby][nbx]; d_work may be NULL */
SIFT3D_AMD_API int
sift3d_hip_block_match(const float *d_F, int nx, int ny, int nz, const float *d_W, const float *d_VF,
                       const float *d_VW, int radius, float *d_disp, float *d_cc, double *d_var, void *d_work,
                       void *stream);
/* host only */
SIFT3D_AMD_API int
sift3d_amd_fit_trimmed(const double *src, const double *dst, int n, int model, double keep, int max_iter,
                       const double *scale_src /*3 or NULL*/, const double *scale_dst /*3 or NULL*/, double *T /*12*/,
                       unsigned char *used /*n or NULL*/, int *iterations);
typedef struct {
    int model;                 /* SIFT3D_AMD_MODEL_RIGID */
    int levels;                /* 3 */
    int iterations;            /* 5, per level */
    int radius;                /* 3 */
    double keep_blocks;        /* 0.5 of the valid blocks, by variance */
    double keep_inliers;       /* 0.5 of the pairs, by residual */
    double tol;                /* 0.01 voxels */
    double spacing_fixed[3];   /* 1, 1, 1 (x, y, z) */
    double spacing_moving[3];  /* 1, 1, 1 */
} sift3d_amd_block_register_params;
typedef struct {
    int level, n_valid, n_selected, n_used;
    double A_in[12], A_out[12];
    double mean_cc, rms, move;
} sift3d_amd_block_iteration;
typedef struct {
    double A[12];
    int iterations, stop;
    sift3d_amd_block_iteration trail[SIFT3D_AMD_BLOCK_MAX_TRAIL];
} sift3d_amd_block_register_result;
SIFT3D_AMD_API void sift3d_amd_block_register_default_params(sift3d_amd_block_register_params *p);
/* for bindings that restate the layouts: sizeof the params (0), iteration (1) and result (2) structs, then
 * SIFT3D_AMD_BLOCK_MAX_ITERATIONS (3), SIFT3D_AMD_BLOCK_MAX_RADIUS (4); 0 otherwise */
SIFT3D_AMD_API size_t sift3d_amd_block_register_struct_bytes(int which);
/* device scratch of the driver in floats (0 for bad arguments, a level's fixed grid below 8 among them) */
SIFT3D_AMD_API size_t
sift3d_amd_block_register_work_floats(int ox, int oy, int oz, int nx, int ny, int nz, int levels, int mask_fixed,
                                      int mask_moving);
/* d_F [oz][oy][ox], d_M [nz][ny][nx], d_WF / d_WM masks on those grids or NULL; A_io [12] on the host, in / out;
 * waits for `stream` once per iteration */
SIFT3D_AMD_API int
sift3d_amd_block_register_device(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                 const float *d_WF, const float *d_WM, double *A_io,
                                 const sift3d_amd_block_register_params *params,
                                 sift3d_amd_block_register_result *result, float *d_work, void *stream);

/* ------------------------------------------------------------------------ */
/* Discrete displacement search                                              */
/* ------------------------------------------------------------------------ */
/* Deformable registration by discrete optimisation over a dense displacement label space (Heinrich et al., "MRF-based
 * deformable registration and ventilation estimation of lung CT", TMI 2013; Heinrich et al., "Non-parametric discrete
 * registration with convex optimisation", WBIR 2014): the matching cost of every block at every displacement of a
 * search cube is sampled into a cost volume, one displacement per block is picked under a quadratic coupling to a
 * smooth field, the field is smoothed, the coupling tightened, and this is repeated coarse to fine.  There is no
 * gradient and no dependence on the start inside the search range, so motions larger than the local structure's
 * period are found; the result is the start field that demons and FFD want.  No upstream counterpart: PARITY UNPINNED,
 * pinned to this contract and its numpy restatement (tests/discrete_restatement.py); the device reproduces every
 * output but the one order-free sum of the statistics record bit for bit.
 *
 * Blocks and labels.  Those of "Block matching", word for word.  Edge 4: block (bx, by, bz) covers voxels
 * 4 b .. 4 b + 3 on every axis; nb_d = n_d / 4 (integer division), trailing voxels belong to no block; -1 when any
 * nb_d == 0.  The block's voxel i = x + 4 y + 16 z (local), 0 .. 63.  Labels d = (dx, dy, dz) in [-R, R]^3,
 * k = ((dz + R)(2R + 1) + (dy + R))(2R + 1) + (dx + R), K = (2R + 1)^3, R in [1, SIFT3D_AMD_DISCRETE_MAX_RADIUS].
 *
 * Cost volume (sift3d_hip_cost_volume).  F[nc][nz][ny][nx], the fixed feature stack; W[nc][nz][ny][nx], the moving
 * stack already warped onto the fixed grid; both finite float32; nc in [1, SIFT3D_AMD_DISCRETE_MAX_CHANNELS].  Optional
 * float masks V_F, V_W on the grid: a voxel is in where w >= 0.5f (the rule of "Masks"); NULL is all in.
 * Per block b and label k, in double, from +0.0, channels c ascending outermost and voxels i ascending inside,
 * nothing fused:
 *   e = (double) F_c,i - (double) W_c,i+d  (exact),  s = e * e,  acc = acc + s;   cost = (float) (acc / (64.0 * nc)).
 * A label is valid when the shifted block lies wholly inside the grid and all its 64 voxels are in V_W; a block is
 * valid when all its 64 voxels are in V_F.  An invalid label, and every label of an invalid block, gets +inf.  A
 * finite sum that rounds past FLT_MAX gives +inf too: the two are indistinguishable on purpose, both mean "never
 * choose".  Output d_cost, float [nbz][nby][nbx][K], the label index fastest: sift3d_amd_cost_volume_bytes bytes (0
 * for bad arguments; 2.3 GB at 256^3 and R = 6).  This implementation needs no work buffer:
 * sift3d_amd_cost_volume_work_bytes is 0 and d_work may be NULL; it is never read or written.
 *
 * Coupled selection (sift3d_hip_cost_select).  u[3][nbz][nby][nbx], the block field the choice is coupled to (float
 * x, y, z, in voxels).  Per block and label, in double, unfused:
 *   ex = (double) dx - (double) u_x (ey, ez likewise),  q = (ex ex + ey ey) + ez ez,  val = (double) cost + theta q.
 * The choice is the smallest val; equal val: the smaller dx^2 + dy^2 + dz^2, then the smaller k.  Outputs: v[3], the
 * chosen label as float; d_data[nb], the chosen label's cost.  A block whose smallest val is +inf is empty: its v is
 * u's bytes and its d_data +inf.  d_stats: 16 bytes with the layout and reduction rule of
 * SIFT3D_AMD_DEMONS_STATS_BYTES: bytes 0-7 the double sum of (double) d_data over the non-empty blocks, bytes 8-15 the
 * uint64 count of the non-empty blocks; per-workgroup partials reduced in a fixed order, no float atomics; the order
 * of that one sum is not part of the contract.  theta >= 0 and finite; theta = 0 is the plain arg-min.  d_work holds
 * SIFT3D_AMD_COST_SELECT_WORK_BYTES bytes (the partials).
 *
 * Block-field smoothing (sift3d_hip_block_field_smooth).  Per channel the separable binomial with clamped indices,
 *   B_x(a)(i) = (0.25f a[max(i - 1, 0)] + 0.5f a[i]) + 0.25f a[min(i + 1, n - 1)],
 * along x, then y, then z, in float and unfused: one pass; `passes` in [0, SIFT3D_AMD_DISCRETE_MAX_PASSES] of them, 0
 * copies.  Its own rule rather than the detector's blur: it holds on grids of one block per axis.  d_work holds
 * sift3d_amd_block_field_smooth_work_bytes bytes: one more field with passes >= 2, else 0 (d_work may then be NULL).
 *
 * Expansion (sift3d_hip_block_field_expand).  The block field goes to a voxel field w[3][nz][ny][nx] by trilinear
 * interpolation between the block centres 4 b + 1.5.  Per axis, t = ((float) p - 1.5f) * 0.25f clamped to
 * [0, nb - 1], i0 = (int) floorf(t), i1 = min(i0 + 1, nb - 1), f = t - (float) i0; (1 - f) a[i0] + f a[i1] along x,
 * then y, then z, unfused.  Voxels past the last block centre take the edge value.  nb_d == n_d / 4 is required.
 *
 * Driver (sift3d_amd_discrete_register_device).  The levels are sift3d_amd_demons_level stacks exactly as
 * sift3d_amd_demons_multires_device takes them (level 0 the finest, every level the half of the one above, the caller
 * makes the stacks, levels in [1, SIFT3D_AMD_DEMONS_MAX_LEVELS]; `iterations` is not read).  u_0 = d_u; fields go down
 * by restrict2 at scale 0.5f, the masks d_VF (level 0's fixed grid) and d_VM (its moving grid) by restrict2 at scale
 * 1.  Per level l, the coarsest first:
 *   1. W = warp_field(M_l, u_l, LINEAR, fill 0), every channel;
 *   2. V_W = warp_field(the level's moving mask, or a volume of ones, u_l, NEAREST, fill 0);
 *   3. C = cost_volume(F_l, W, V_F = the level's fixed mask or NULL, V_W, radius);
 *   4. b = 0;
 *   5. for theta_j of params->theta[0 .. n_theta - 1], n_theta in [1, SIFT3D_AMD_DISCRETE_MAX_THETAS]:
 *   6.    v = cost_select(C, b, theta_j), its record to d_stats[next];
 *   7.    b = block_field_smooth(v, passes);
 *   8. (the first theta's selection runs against b = 0 with theta_0 like any other: it is not special-cased)
 *   9. w = block_field_expand(b); u_l = field_compose(u_l, w) = w(p) + u_l(p + w(p)) (SIFT3D_AMD_FIELD_COMPOSE);
 *      l > 0: u_(l-1) = field_prolong2(u_l).
 * d_stats receives one 16-byte record per (level, theta) in the order run.  A level whose fixed grid is below 4 on an
 * axis is refused.  Asynchronous on `stream`, no host synchronisation, allocates nothing.  d_work holds
 * sift3d_amd_discrete_register_work_floats floats, 8-byte aligned: with n_l, m_l the voxels of the fixed and moving
 * grid on level l, b_0 the blocks of level 0 and P = SIFT3D_AMD_COST_SELECT_WORK_BYTES / 4,
 *   pad4(P) + pad4(nc n_0) + pad4(n_0) + [no moving mask: pad4(m_0)] + pad4(b_0 K) + 3 pad4(3 b_0) + pad4(b_0)
 *   + 2 pad4(3 n_0) + sum_{l >= 1} (pad4(3 n_l) + [fixed mask: pad4(n_l)] + [moving mask: pad4(m_l)])
 * (the partials; W; V_W; the ones; C; v, b and the smoothing's second buffer; the chosen costs; w and the composed
 * field; the coarser fields and masks).  params == NULL takes the defaults below.
 *
 * Refusals, -1 before any device call: NULL pointers (the masks, and a work buffer of zero bytes, may be NULL);
 * dims <= 0 or a grid with nb_d == 0; nc, radius, passes or n_theta out of range; a theta that is negative or not
 * finite; dimensions off the halving chain; misalignment (statistics and work 8 B, the rest 4 B); any output or work
 * buffer overlapping an input or another output.  Every entry uses 64-bit offsets (nb K passes 2^31 early).
 *
 * Out of scope: label steps other than 1 voxel; sub-label refinement; block edges other than 4 and overlapping
 * blocks; MRF, tree or belief-propagation regularisers; symmetric (two-way) search; physical spacing; a cost other
 * than the channel SSD (LNCC and MI are out); multi-GPU; wiring into register_ffd / register_dense / refine_field. */
#define SIFT3D_AMD_DISCRETE_MAX_RADIUS 6
#define SIFT3D_AMD_DISCRETE_MAX_CHANNELS 16
#define SIFT3D_AMD_DISCRETE_MAX_PASSES 16
#define SIFT3D_AMD_DISCRETE_MAX_THETAS 16
#define SIFT3D_AMD_COST_SELECT_WORK_BYTES 16384     /* 1024 slots of a double and a uint64 */
/* the default schedule of the coupling: the six values of WBIR 2014, a factor ~3 apart, times 0.03: the mean squared
 * difference of MIND channels of matching blocks is near 0.05 and of unrelated ones near 0.15, not 1 */
#define SIFT3D_AMD_DISCRETE_DEFAULT_THETAS { 0.00009, 0.0003, 0.0009, 0.003, 0.009, 0.03 }
/* bytes of d_cost, float [nbz][nby][nbx][K]; 0 for bad arguments (a dimension below 4, radius out of range) */
SIFT3D_AMD_API size_t sift3d_amd_cost_volume_bytes(int nx, int ny, int nz, int radius);
/* bytes of d_work for sift3d_hip_cost_volume: 0, this implementation needs none */
SIFT3D_AMD_API size_t sift3d_amd_cost_volume_work_bytes(int nx, int ny, int nz, int nc, int radius);
/* d_F, d_W [nc][nz][ny][nx]; d_VF, d_VW masks [nz][ny][nx] or NULL; d_cost float [nbz][nby][nbx][K]; d_work may be
 * NULL */
SIFT3D_AMD_API int
sift3d_hip_cost_volume(const float *d_F, const float *d_W, int nc, int nx, int ny, int nz, const float *d_VF,
                       const float *d_VW, int radius, float *d_cost, void *d_work, void *stream);
/* bytes of d_work for sift3d_hip_cost_select: SIFT3D_AMD_COST_SELECT_WORK_BYTES (0 for bad dims) */
SIFT3D_AMD_API size_t sift3d_amd_cost_select_work_bytes(int nbx, int nby, int nbz);
/* d_cost [nbz][nby][nbx][K]; d_u, d_v float [3][nbz][nby][nbx]; d_data float [nbz][nby][nbx]; d_stats 16 B */
SIFT3D_AMD_API int
sift3d_hip_cost_select(const float *d_cost, int nbx, int nby, int nbz, int radius, const float *d_u, double theta,
                       float *d_v, float *d_data, void *d_stats, void *d_work, void *stream);
/* bytes of d_work for sift3d_hip_block_field_smooth: 12 nb with passes >= 2, else 0 (0 for bad arguments too) */
SIFT3D_AMD_API size_t sift3d_amd_block_field_smooth_work_bytes(int nbx, int nby, int nbz, int passes);
/* d_src, d_dst float [3][nbz][nby][nbx]; d_work may be NULL where the size above is 0 */
SIFT3D_AMD_API int
sift3d_hip_block_field_smooth(const float *d_src, float *d_dst, int nbx, int nby, int nbz, int passes, void *d_work,
                              void *stream);
/* d_b float [3][nbz][nby][nbx], nb_d == n_d / 4; d_w float [3][nz][ny][nx] */
SIFT3D_AMD_API int
sift3d_hip_block_field_expand(const float *d_b, int nbx, int nby, int nbz, float *d_w, int nx, int ny, int nz,
                              void *stream);
typedef struct {
    int radius;                /* 4 */
    int passes;                /* 2 */
    int n_theta;               /* 6 */
    double theta[SIFT3D_AMD_DISCRETE_MAX_THETAS];  /* SIFT3D_AMD_DISCRETE_DEFAULT_THETAS */
} sift3d_amd_discrete_register_params;
SIFT3D_AMD_API void sift3d_amd_discrete_register_default_params(sift3d_amd_discrete_register_params *p);
/* for bindings that restate the layouts: sizeof the params struct (0), then SIFT3D_AMD_DISCRETE_MAX_RADIUS (1),
 * _MAX_CHANNELS (2), _MAX_THETAS (3), _MAX_PASSES (4), SIFT3D_AMD_COST_SELECT_WORK_BYTES (5); 0 otherwise */
SIFT3D_AMD_API size_t sift3d_amd_discrete_register_struct_bytes(int which);
/* device scratch of the driver in floats, for level 0's fixed grid (nx, ny, nz) and moving grid (mx, my, mz); 0 for
 * bad arguments, a level's fixed grid below 4 among them */
SIFT3D_AMD_API size_t
sift3d_amd_discrete_register_work_floats(int nx, int ny, int nz, int mx, int my, int mz, int nc, int levels,
                                         int radius, int mask_fixed, int mask_moving);
/* level [levels] (level 0 the finest); d_VF, d_VM masks on level 0's fixed / moving grid or NULL; d_u float
 * [3][nz][ny][nx] on level 0's fixed grid, in / out; d_stats 16 B per (level, theta) */
SIFT3D_AMD_API int
sift3d_amd_discrete_register_device(const sift3d_amd_demons_level *level, int levels, int nc, const float *d_VF,
                                    const float *d_VM, float *d_u,
                                    const sift3d_amd_discrete_register_params *params, void *d_stats, float *d_work,
                                    void *stream);

/* ------------------------------------------------------------------------ */
/* Distance transforms and surface distances                                 */
/* ------------------------------------------------------------------------ */
/* The exact Euclidean distance transform (EDT) of a mask, the signed distance of a set, the six-neighbour surface of
 * a label and, from them, the distances between the surfaces of two segmentations: Hausdorff, HD95 and the average
 * symmetric surface distance, the measures reported beside Dice ("Similarity measures").  No upstream counterpart:
 * PARITY UNPINNED, pinned to this contract and its numpy restatement (tests/distance_restatement.py), every device
 * output bit for bit.  None of it uses the sampling core.
 *
 * Feature set.  A mask is a float32 volume [nz][ny][nx].  A voxel is IN when w >= 0.5f ("Masks": one float compare, so a
 * NaN is out).  The features are the voxels that are IN; with invert != 0, the voxels that are OUT.
 *
 * Weights.  spacing is three doubles (sx, sy, sz), the voxel's edge lengths; NULL: all 1.  Each must be finite and lie
 * in [1e-6, 1e6].  w_a = (float) (s_a * s_a): the product in double, rounded once to float.  Every dimension is at most
 * SIFT3D_AMD_DISTANCE_MAX_DIM = 4096, so every integer d * d below is exact in float32.
 *
 * Squared distance.  For an output voxel p and a feature voxel q with integer offsets dx, dy, dz:
 *     c(p, q) = ((w_x (*) (float) (dx dx)) (+) (w_y (*) (float) (dy dy))) (+) (w_z (*) (float) (dz dz))
 * where (*) and (+) are float32 multiply and add, unfused.  D2(p) = the minimum of c(p, q) over every feature voxel q,
 * +inf when there is no feature; D(p) = sqrtf(D2(p)), correctly rounded.
 * The device builds it in three per-axis passes, which reproduce that minimum bit for bit because (*) and (+) are
 * monotone: the x pass writes g1 = w_x (*) (float) (min dx dx) (+inf in a row without a feature), the y pass
 * g2(y) = min over y' of g1(y') (+) (w_y (*) (float) ((y - y') (y - y'))), the z pass the same along z, and each line
 * minimum is exact on the rounded values: the search walks outwards from y and stops where w (*) (float) (r r) alone
 * reaches the best value so far, beyond which no candidate can be smaller, ties included.  With unit spacing every
 * value is an integer: D2 is the integer squared distance rounded once to float (exact below 2^24).  A line without a
 * feature costs its whole length per voxel: O(n) per voxel per pass in the worst case.
 *
 * Signed distance of the set of IN voxels: +sqrtf(D2 to the set) at voxels outside it, -sqrtf(D2 to its complement) at
 * voxels inside it; +inf everywhere when the set is empty, -inf everywhere when it is the whole grid.
 *
 * Surface of a label.  S_k = {p : L(p) == (float) k} for a label volume L (float-valued integers, as label overlap
 * takes them).  p is on the surface dS_k when p is in S_k and at least one of its six face neighbours is not; a
 * neighbour beyond the grid is not.  The surface volume holds 1.0f there and 0.0f elsewhere, and *d_count their number.
 *
 * Surface distances for label k, both label volumes on one grid [nz][ny][nx]: d_fm is the multiset
 * {D to dM_k at p : p in dF_k}, d_mf the other direction.  sift3d_hip_surface_collect appends sqrtf(d2[p]) for every p
 * whose surface value is IN, in no particular order (the order in which the device collects is not part of the
 * contract; the sorted arrays are), adds their number to *d_count - also where it exceeds `capacity` - and writes
 * nothing at or past d_list[capacity].
 *
 * Measures (host, double), from the two lists sorted ascending, n_f and n_m their lengths:
 *   sum_fm, sum_mf = acc after: acc = 0.0; for each d in ascending order: acc = acc + (double) d
 *   max_fm, max_mf = the last elements; mean_fm = sum_fm / n_f, mean_mf = sum_mf / n_m
 *   hausdorff = max(max_fm, max_mf);  assd = (sum_fm + sum_mf) / (n_f + n_m)
 *   hd95: d[0 .. n-1] = both lists merged ascending, n = n_f + n_m; pos = 0.95 * (n - 1), i = floor(pos),
 *         hd95 = d[i] + (pos - i) * (d[min(i + 1, n - 1)] - d[i])   (the linear percentile of the pooled list)
 * When either surface is empty every measure is NaN; the counts are still reported.
 *
 * The sift3d_hip_ entries are asynchronous on `stream`, allocate nothing, use 64-bit offsets and check their arguments
 * before any device call: -1 on NULL pointers, dims <= 0 or > SIFT3D_AMD_DISTANCE_MAX_DIM (n_voxels == 0 or beyond its
 * cube, a capacity beyond it), a spacing that is not finite or outside [1e-6, 1e6], a buffer that is not 4-byte aligned
 * (8-byte: a counter, the driver's d_work), an output that overlaps an input, the work buffer or another output.
 * d_work of the three transform entries: sift3d_amd_distance_work_bytes() bytes = two volumes; sift3d_hip_distance_sq
 * and sift3d_hip_distance touch the first of them only (the ping-pong between the passes), the signed entry both. */
#define SIFT3D_AMD_DISTANCE_MAX_DIM 4096
typedef struct {
    uint64_t n_f, n_m;                          /* voxels on the fixed and the moving surface */
    double hausdorff, hd95, assd, mean_fm, mean_mf, max_fm, max_mf;
} sift3d_amd_surface_result;
/* bytes of d_work for the three transform entries (0 for bad dims) */
SIFT3D_AMD_API size_t sift3d_amd_distance_work_bytes(int nx, int ny, int nz);
/* d_out [nz][ny][nx] = D2 */
SIFT3D_AMD_API int
sift3d_hip_distance_sq(const float *d_mask, int nx, int ny, int nz, const double *spacing /*3 or NULL*/, int invert,
                       float *d_out, void *d_work, void *stream);
/* d_out = D = sqrtf(D2), the root taken by the last pass */
SIFT3D_AMD_API int
sift3d_hip_distance(const float *d_mask, int nx, int ny, int nz, const double *spacing /*3 or NULL*/, int invert,
                    float *d_out, void *d_work, void *stream);
/* d_out = the signed distance of the set of IN voxels */
SIFT3D_AMD_API int
sift3d_hip_distance_signed(const float *d_mask, int nx, int ny, int nz, const double *spacing /*3 or NULL*/,
                           float *d_out, void *d_work, void *stream);
/* d_surface [nz][ny][nx] float 0 / 1; *d_count (device, 8-byte aligned) = the number of surface voxels */
SIFT3D_AMD_API int
sift3d_hip_label_surface(const float *d_labels, int nx, int ny, int nz, int label, float *d_surface,
                         uint64_t *d_count, void *stream);
/* d_surface, d_d2 [n_voxels]; d_list [capacity]; *d_count (device, 8-byte aligned) = the number of surface voxels */
SIFT3D_AMD_API int
sift3d_hip_surface_collect(const float *d_surface, const float *d_d2, size_t n_voxels, float *d_list,
                           size_t capacity, uint64_t *d_count, void *stream);
/* host only: two lists sorted ascending on the host (a list may be NULL when its length is 0).  -1 on a NULL out or a
 * NULL list of non-zero length. */
SIFT3D_AMD_API int
sift3d_amd_surface_measures(const float *d_fm, uint64_t n_f, const float *d_mf, uint64_t n_m,
                            sift3d_amd_surface_result *out);
/* The driver: results[l] for labels[l], l = 0 .. n_labels - 1 (1 <= n_labels <= SIFT3D_AMD_SIMILARITY_MAX_BINS), of the
 * label volumes d_LF and d_LM on one grid; labels, spacing and results on the host.  Per label: the two surfaces, the
 * transform of each, the two lists, sorted on the host (the only host allocation), and the measures.  SYNCHRONOUS: it
 * waits for `stream` once per label to read the two surface counts - a label with an empty surface ends there - and
 * once more to receive the two lists.  d_work: sift3d_amd_surface_distances_work_bytes() bytes (0 for bad dims),
 * 8-byte aligned: five volumes and the counters. */
SIFT3D_AMD_API size_t sift3d_amd_surface_distances_work_bytes(int nx, int ny, int nz);
SIFT3D_AMD_API int
sift3d_amd_surface_distances_device(const float *d_LF, const float *d_LM, int nx, int ny, int nz, const int *labels,
                                    int n_labels, const double *spacing /*3 or NULL*/,
                                    sift3d_amd_surface_result *results, void *d_work, void *stream);

/* ------------------------------------------------------------------------ */
/* Multi-GPU: one process per GPU, the volume cut into Z-slabs               */
/* ------------------------------------------------------------------------ */

/* The three exchanges of the slab driver (sift3d_amd/csrc/sift3d_sharded.c).  All buffers are
 * DEVICE pointers; every call is enqueued on `stream` (stream-ordered, like RCCL) or completes
 * before returning.  A NULL send/recv pair of `halo` means "no neighbour on that side".  Return 0
 * on success. */
typedef struct {
    int rank, world;
    void *ctx;
    /* nearest neighbours: send send_lo to rank-1 / send_hi to rank+1, receive recv_lo from
     * rank-1 / recv_hi from rank+1, `bytes` each */
    int (*halo)(void *ctx, const void *d_send_lo, void *d_recv_lo, const void *d_send_hi,
                void *d_recv_hi, size_t bytes, void *stream);
    int (*allreduce_max)(void *ctx, float *d_buf, int n, void *stream);          /* in place */
    int (*allgather)(void *ctx, const void *d_send, void *d_recv, size_t bytes_per_rank,
                     void *stream);                     /* d_recv: world * bytes, rank order */
} sift3d_amd_transport;

/* RCCL over xGMI (librccl is loaded at run time).  Rank 0 makes the 128-byte unique id, the
 * application distributes it (any out-of-band channel), every rank builds its transport on its own
 * current HIP device. */
SIFT3D_AMD_API int sift3d_amd_rccl_unique_id(void *id128);
SIFT3D_AMD_API int sift3d_amd_rccl_transport(sift3d_amd_transport *out, int world, int rank,
                                             const void *id128);
SIFT3D_AMD_API void sift3d_amd_rccl_transport_free(sift3d_amd_transport *t);

/* Rehearsal / test transport: the `world` ranks are THREADS of one process (one slab driver each, on the
 * same device), exchanging device-to-device.  Stream-ordered with the completion semantics of
 * ncclSend / ncclRecv / ncclAllGather / ncclAllReduce and no host-side stream synchronisation
 * (sift3d_amd/csrc/sift3d_thread_transport.c): (pointer, event) pairs travel through a host mailbox, the
 * copies run on the receiver's stream behind the sender's `ready` event, the sender's stream waits for the
 * receiver's `consumed` event.  An error in the driver's event edges between its streams therefore shows
 * on one GPU as a wrong result, as it would over RCCL on eight.  _abort wakes every rank waiting in an
 * exchange (their calls fail) -- for a caller whose rank has given up. */
typedef struct sift3d_amd_thread_group sift3d_amd_thread_group;
SIFT3D_AMD_API sift3d_amd_thread_group *sift3d_amd_thread_group_create(int world);
SIFT3D_AMD_API void sift3d_amd_thread_group_free(sift3d_amd_thread_group *);
SIFT3D_AMD_API void sift3d_amd_thread_group_abort(sift3d_amd_thread_group *);
SIFT3D_AMD_API int sift3d_amd_thread_transport(sift3d_amd_transport *out, sift3d_amd_thread_group *,
                                               int rank);
SIFT3D_AMD_API void sift3d_amd_thread_transport_free(sift3d_amd_transport *t);

/* sift3d_detect_keypoints + sift3d_extract_descriptors (sift.c:1217-1249, 1615-1635) on ONE
 * nx*ny*nz volume cut into `world` Z-slabs; results equal the single-GPU ones bit for bit.
 * `params` supplies thresholds, scales, the number of keypoint levels per octave and the extrema
 * neighbourhood (NULL: defaults); every configuration the drop-in API accepts is supported.  This rank's raw planes [z0, z1) go to the device
 * buffer sift3d_amd_sharded_input() (x fastest, (z1 - z0) * ny * nx floats).  detect fills `kp`
 * with the GLOBAL keypoint list on every rank; describe computes the descriptors of the
 * keypoints this rank owns (their positions in `kp` go to own_idx, capacity kp's size).
 * Failures: detect and the descriptor gather are collective.  A failure that every rank sees (bad arguments,
 * a transport error, an exchange buffer that cannot be allocated) returns SIFT3D_FAILURE at once.  A rank whose
 * LOCAL work fails (a launch, an allocation) keeps issuing every exchange of the step in the common order, its
 * status word travels behind the blocks of both all-gathers, and EVERY rank returns SIFT3D_FAILURE at the same
 * point with the transport in step for the next call (the reference: every stage returns -1 to its caller,
 * immacros.h:27-32). */
typedef struct sift3d_amd_sharded sift3d_amd_sharded;
SIFT3D_AMD_API sift3d_amd_sharded *
sift3d_amd_sharded_create(int nx, int ny, int nz, const sift3d_amd_transport *t,
                          const sift3d_detector *params, double ux, double uy, double uz);
SIFT3D_AMD_API void sift3d_amd_sharded_free(sift3d_amd_sharded *);
SIFT3D_AMD_API int sift3d_amd_sharded_own_planes(const sift3d_amd_sharded *, int *z0, int *z1);
SIFT3D_AMD_API float *sift3d_amd_sharded_input(sift3d_amd_sharded *);
SIFT3D_AMD_API int sift3d_amd_sharded_synth(sift3d_amd_sharded *, uint64_t seed);
SIFT3D_AMD_API int sift3d_amd_sharded_detect(sift3d_amd_sharded *, sift3d_keypoint_store *kp);
SIFT3D_AMD_API int sift3d_amd_sharded_describe(sift3d_amd_sharded *, const sift3d_keypoint_store *kp,
                                               sift3d_descriptor_store *desc, int *own_idx,
                                               int *n_own);
/* The descriptors of ALL keypoints of `kp`, in its (global) order, from the rows every rank computed
 * (sift3d_amd_sharded_describe: desc_own / own_idx / n_own of THIS rank): one all-gather of the ranks' row
 * blocks, device to device.  root < 0: `all` is filled on every rank; else on rank `root` only (the others
 * take part in the exchange and leave `all` alone).  Collective; the status word behind every block makes a
 * rank-local failure return SIFT3D_FAILURE on every rank -- a rank whose sift3d_amd_sharded_describe failed
 * still calls this, with n_own = -1. */
SIFT3D_AMD_API int
sift3d_amd_sharded_gather_descriptors(sift3d_amd_sharded *, const sift3d_keypoint_store *kp,
                                      const sift3d_descriptor_store *desc_own, const int *own_idx, int n_own,
                                      sift3d_descriptor_store *all, int root);
/* test hook: the next detect (where = 1, 2, 3: before the pyramid, after the extrema, between the two
 * all-gathers) or descriptor gather (4) of this rank fails LOCALLY; 0 clears */
SIFT3D_AMD_API int sift3d_amd_sharded_inject_failure(sift3d_amd_sharded *, int where);
SIFT3D_AMD_API int sift3d_amd_sharded_num_candidates(const sift3d_amd_sharded *);
/* this rank's candidate list capacity (as sift3d_amd_detector_set_candidate_capacity / _candidate_capacity) */
SIFT3D_AMD_API int sift3d_amd_sharded_set_candidate_capacity(sift3d_amd_sharded *, int cap);
SIFT3D_AMD_API int sift3d_amd_sharded_candidate_capacity(const sift3d_amd_sharded *);
/* eight doubles of the last step: [0] Gaussian pyramid (device s, halo exchanges of the blurs inside)
 * [1] detect wall  [2] describe wall  [3] DoG maxima + extrema (device s, incl. the all-reduce)
 * [4] wait for the window halos + orientation (device s)  [5] gathers + global keypoint list (host s)
 * [6] input scaling (device s, incl. the all-reduce)  [7] unused */
SIFT3D_AMD_API const double *sift3d_amd_sharded_timings(const sift3d_amd_sharded *);
SIFT3D_AMD_API int sift3d_amd_sharded_info(const sift3d_amd_sharded *, int *num_octaves, int *o_shard,
                                           int *halo);

/* ------------------------------------------------------------------------ */
/* Device plumbing (so that the C host code needs no HIP headers)           */
/* ------------------------------------------------------------------------ */
SIFT3D_AMD_API int sift3d_hip_device_count(void);
SIFT3D_AMD_API int sift3d_hip_set_device(int dev);
SIFT3D_AMD_API int sift3d_hip_current_device(void);   /* -1 on error */
SIFT3D_AMD_API void *sift3d_hip_malloc(size_t bytes);
SIFT3D_AMD_API void sift3d_hip_free(void *d_ptr);
SIFT3D_AMD_API void *sift3d_hip_host_alloc(size_t bytes); /* pinned */
SIFT3D_AMD_API void sift3d_hip_host_free(void *h_ptr);
/* device-side address of a sift3d_hip_host_alloc block (kernels may write results into it) */
SIFT3D_AMD_API void *sift3d_hip_host_device_ptr(void *h_ptr);
SIFT3D_AMD_API int sift3d_hip_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes, void *stream);
SIFT3D_AMD_API int sift3d_hip_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes, void *stream);
SIFT3D_AMD_API int sift3d_hip_memcpy_d2d(void *d_dst, const void *d_src, size_t bytes, void *stream);
SIFT3D_AMD_API int sift3d_hip_memcpy2d_d2h(void *h_dst, size_t dst_pitch, const void *d_src,
                                           size_t src_pitch, size_t width, size_t height, void *stream);
SIFT3D_AMD_API int sift3d_hip_stream_wait_event(void *stream, void *ev);
/* descriptor rows (768 floats) out of the ranks' gathered blocks into the global order: row g = row
 * (d_map[g] & 0xffffff) of block (d_map[g] >> 24); blocks are blk_bytes apart.  The rows move as float4: d_dst,
 * d_all and blk_bytes are multiples of 16 bytes.  n == 0 is a success that touches nothing. */
SIFT3D_AMD_API int sift3d_hip_rows_scatter(float *d_dst, const void *d_all, size_t blk_bytes,
                                           const uint32_t *d_map, uint32_t n, void *stream);
/* d_dst[i] = max over r of d_rows[r * n + i] (the reduction step of the thread transport's all-reduce) */
SIFT3D_AMD_API int sift3d_hip_max_rows(float *d_dst, const float *d_rows, int nrows, int n, void *stream);
SIFT3D_AMD_API int sift3d_hip_memset(void *d_dst, int byte, size_t bytes, void *stream);
SIFT3D_AMD_API void *sift3d_hip_stream_create(void);
SIFT3D_AMD_API void *sift3d_hip_stream_create_high(void);   /* highest dispatch priority */
SIFT3D_AMD_API void sift3d_hip_stream_destroy(void *stream);
SIFT3D_AMD_API int sift3d_hip_stream_sync(void *stream);
/* HIP events, for device-side stage timing */
SIFT3D_AMD_API void *sift3d_hip_event_create(void);
SIFT3D_AMD_API void sift3d_hip_event_destroy(void *ev);
SIFT3D_AMD_API int sift3d_hip_event_record(void *ev, void *stream);
SIFT3D_AMD_API double sift3d_hip_event_elapsed_ms(void *ev_start, void *ev_stop); /* syncs on stop */

/* ------------------------------------------------------------------------ */
/* Stage kernels                                                            */
/* ------------------------------------------------------------------------ */

/* im_max_abs (imutil.c:681-695): *d_max = max(*d_max, max|src[i]|).  d_max is a
 * device float the caller zeroes first (max is order independent => exact). */
SIFT3D_AMD_API int
sift3d_hip_absmax(const float *d_src, size_t n, float *d_max, void *stream);

/* im_scale (imutil.c:699-713): dst = src / *d_max, a plain copy when *d_max == 0. */
SIFT3D_AMD_API int
sift3d_hip_scale(const float *d_src, float *d_dst, size_t n, const float *d_max,
                 void *stream);

#define SIFT3D_HIP_MAX_TAPS 65

/* One 1-D pass of convolve_sep_gen (imutil.c:742-861) along `axis`, applied directly
 * on the x-fastest volume (no im_permute copies, imutil.c:907-958).
 *
 *  unit_factor = (float)(unit / units[axis])             (imutil.c:754-755)
 *  z_lo, z_hi    local plane range [z_lo, z_hi) of outputs to produce
 *  n_glob, off   axis 2 only: the buffers hold planes [off, off + nz) of a global
 *                axis of n_glob planes; mirror rules use global coordinates and
 *                interior samples must be present locally (halo).  Unsharded:
 *                n_glob = nz, off = 0.
 *  variant       0 = pick the fastest specialised kernel, 1 = force the literal
 *                one-thread-per-voxel kernel (used by tests to A/B the fast paths) */
typedef struct {
    const float *src;
    float *dst;
    int nx, ny, nz;
    int axis;
    int width;
    const float *taps; /* host pointer */
    float unit_factor;
    int n_glob, off;
    int z_lo, z_hi;
    int variant;
} sift3d_hip_fir_args;

SIFT3D_AMD_API int
sift3d_hip_fir(const sift3d_hip_fir_args *args, void *stream);
/* The x pass of a unit-spaced blur applied to src / *d_max: im_scale (imutil.c:698-713; *d_max = max|src|
 * from sift3d_hip_absmax, 0: no scaling) folded into the first pass of the pyramid, so that the scaled image
 * is never stored.  Same result as sift3d_hip_scale followed by sift3d_hip_fir.  1: not covered (axis other
 * than x, tap spacing other than 1, more than 17 taps, the literal variant). */
SIFT3D_AMD_API int
sift3d_hip_fir_x_scaled(const sift3d_hip_fir_args *args, const float *d_max, void *stream);
SIFT3D_AMD_API int sift3d_hip_fir_x_scaled_covers(const sift3d_hip_fir_args *args);   /* 1: covered */

/* The y and z passes of one blur fused into one launch when both have tap spacing 1 (octave 0):
 * dst = FIR_z(FIR_y(src)), bit-identical to two sift3d_hip_fir calls, without the intermediate
 * volume touching HBM.  Slab arguments as for axis 2 of sift3d_hip_fir.  Returns SIFT3D_SUCCESS,
 * SIFT3D_FAILURE, or 1 when the configuration is not covered (width > 17, nx % 4 != 0, unaligned
 * buffers, an axis shorter than width + 1): the caller then issues the two passes itself. */
SIFT3D_AMD_API int
sift3d_hip_fir_yz_u1(const float *d_src, float *d_dst, int nx, int ny, int nz, const float *taps,
                     int width, int n_glob, int off, int z_lo, int z_hi, void *stream);
/* 1 when sift3d_hip_fir_yz_u1 covers the configuration (it returns 1 = "not covered" otherwise); for
 * callers that must know before they launch. */
SIFT3D_AMD_API int sift3d_hip_fir_yz_u1_covers(const float *d_src, const float *d_dst, int nx, int ny,
                                               int width, int n_glob);

/* A whole blur of a unit-spaced volume in one launch: dst = FIR_z(FIR_y(FIR_x(src))) over all planes,
 * bit-identical to sift3d_hip_fir (axis 0) followed by sift3d_hip_fir_yz_u1, without either intermediate
 * touching HBM.  d_scale_max (or NULL): the blur of src / *d_scale_max as sift3d_hip_fir_x_scaled forms it.
 * Returns SIFT3D_SUCCESS, SIFT3D_FAILURE, or 1 -- nothing done -- when the configuration is not covered. */
SIFT3D_AMD_API int
sift3d_hip_fir_xyz(const float *d_src, float *d_dst, int nx, int ny, int nz, const float *taps, int width,
                   const float *d_scale_max, void *stream);
/* 1 when sift3d_hip_fir_xyz covers the blur: tap spacing 1 on all three axes (uf_*: the passes' unit factors),
 * nx % 64 == 0, ny % 64 == 0, ny >= 128, an odd width <= 17, distinct 16-byte aligned volumes. */
SIFT3D_AMD_API int sift3d_hip_fir_xyz_covers(const float *d_src, const float *d_dst, int nx, int ny, int nz,
                                             int width, float uf_x, float uf_y, float uf_z);

/* im_subtract (imutil.c:719-739) fused with the dogmax scan of detect_extrema
 * (sift.c:821-826): dst = a - b and *d_absmax = max(*d_absmax, max|dst|).
 * d_absmax may be NULL. */
SIFT3D_AMD_API int
sift3d_hip_subtract_absmax(const float *d_a, const float *d_b, float *d_dst, size_t n,
                           float *d_absmax, void *stream);

/* build_dog (sift.c:713-732) for one octave in one pass: d_d[k] = d_g[k] - d_g[k+1] for
 * k < n_gauss-1 and d_absmax[k] = max(d_absmax[k], max|d_d[k]|).  Every Gaussian level is read
 * once.  Returns 1 (nothing done) when n_gauss > SIFT3D_HIP_MAX_DOG_STACK or a pointer is not
 * 16-byte aligned: the caller then uses sift3d_hip_subtract_absmax per level pair. */
#define SIFT3D_HIP_MAX_DOG_STACK 8
SIFT3D_AMD_API int sift3d_hip_dog_stack(const float *const *d_g, float *const *d_d, int n_gauss,
                                        size_t n, float *d_absmax, void *stream);

/* im_downsample_2x (imutil.c:591-617): dst(x,y,z) = src(2x,2y,2z) for the mx*my*mz
 * output box; src rows are nx long, planes nx*ny. */
SIFT3D_AMD_API int
sift3d_hip_downsample2(const float *d_src, int nx, int ny, float *d_dst, int mx, int my,
                       int mz, void *stream);

/* One DoG level for the extrema search */
typedef struct {
    const float *prev, *cur, *next; /* D[o,s-1], D[o,s], D[o,s+1]: same local dims */
    const float *d_absmax;          /* device float: max|D[o,s]| over the GLOBAL level */
    int z_lo, z_hi;                 /* local planes to test; planes z-1 and z+1 must exist */
    int tag;                        /* copied into every record (level id) */
} sift3d_hip_extrema_level;

typedef struct {
    uint32_t idx;   /* local linear index x + nx*(y + ny*z) */
    int32_t tag;
    float val;      /* |D| at the voxel = keypoint strength (sift.c:864) */
} sift3d_hip_cand;

/* detect_extrema (sift.c:735-871, default 8-neighbour build) for `nlevels` levels of
 * one octave (all nx*ny*nz).  Records are APPENDED to d_out starting at *d_count in
 * the reference's scan order (level, z, y, x); *d_count (device uint32) is advanced
 * by the number found, even past `cap` (records beyond cap are dropped, the caller
 * compares the final count with cap).  d_work: scratch of
 * sift3d_hip_extrema_work_bytes() bytes. */
SIFT3D_AMD_API size_t
sift3d_hip_extrema_work_bytes(int nx, int ny, int nz, int nlevels);
SIFT3D_AMD_API int
sift3d_hip_extrema(const sift3d_hip_extrema_level *levels, int nlevels, int nx, int ny,
                   int nz, double peak_thresh, sift3d_hip_cand *d_out, uint32_t cap,
                   uint32_t *d_count, void *d_work, size_t work_bytes, void *stream);

/* The same with the neighbourhood selectable: cuboid = 0 is the default build's 8-neighbour test
 * (sift.c:797-810), cuboid = 1 the reference's compile-time CUBOID_EXTREMA variant
 * (sift.c:24, 761-796: 27 + 26 + 27 samples). */
SIFT3D_AMD_API int
sift3d_hip_extrema_mode(const sift3d_hip_extrema_level *levels, int nlevels, int nx, int ny, int nz,
                        double peak_thresh, int cuboid, sift3d_hip_cand *d_out, uint32_t cap,
                        uint32_t *d_count, void *d_work, size_t work_bytes, void *stream);

/* build_dog + detect_extrema WITHOUT a stored DoG pyramid, default configuration (three keypoint
 * levels per octave = six Gaussian levels, 8-neighbour test):
 *   sift3d_hip_dogmax_stack    d_absmax[k] = max(d_absmax[k], max|d_g[k] - d_g[k+1]|), k < n_gauss-1
 *                              (the dogmax scan, sift.c:821-826, on differences formed on the fly);
 *   sift3d_hip_extrema_gauss6  detect_extrema for DoG levels 1..3 of the octave, the differences
 *                              (im_subtract, imutil.c:719-739) again formed when loaded; records as
 *                              sift3d_hip_extrema, tags tag0, tag0+1, tag0+2; d_absmax = the five
 *                              maxima of the octave (global over slabs).
 * Both return 1 (nothing done) when the configuration is not covered (nx % 4 != 0, unaligned
 * levels, more than SIFT3D_HIP_MAX_DOG_STACK levels): the caller then stores the DoG levels
 * (sift3d_hip_dog_stack) and calls sift3d_hip_extrema_mode. */
SIFT3D_AMD_API int sift3d_hip_dogmax_stack(const float *const *d_g, int n_gauss, size_t n,
                                           float *d_absmax, void *stream);
SIFT3D_AMD_API int
sift3d_hip_extrema_gauss6(const float *const *d_g, const float *d_absmax, int nx, int ny, int nz,
                          int z_lo, int z_hi, int tag0, double peak_thresh, sift3d_hip_cand *d_out,
                          uint32_t cap, uint32_t *d_count, void *d_work, size_t work_bytes,
                          void *stream);
/* The same in two phases, so that the sweeps of different octaves can run side by side on different
 * streams: phase 1 = the sweep (bit masks + block counts into d_work; touches nothing else), phase 2 =
 * scan + emission appending at *d_count -- to be issued in octave order once the sweeps are done --,
 * phase 0 = both.  d_work must keep its contents between the phases. */
SIFT3D_AMD_API int
sift3d_hip_extrema_gauss6_phase(const float *const *d_g, const float *d_absmax, int nx, int ny, int nz,
                                int z_lo, int z_hi, int tag0, double peak_thresh, sift3d_hip_cand *d_out,
                                uint32_t cap, uint32_t *d_count, void *d_work, size_t work_bytes,
                                void *stream, int phase);
/* The stage with ONE pass over the octave's Gaussian levels (the dogmax scan of sift.c:821-826 needs no
 * pass of its own).  sift3d_hip_dogmax_sub: maxima of the five |DoG| levels over the sub-lattice
 * z = 1, 6, 11, ..., y = 0, 3, 6, ... (one fifteenth of the bytes), atomically maxed into d_est[0..4] (zeroed by the
 * caller) -- LOWER bounds of the reference's maxima.  sift3d_hip_extrema_gauss6_est_phase: phases as above
 * on the whole volume (planes 1 .. nz - 2); the sweep marks every extremum above peak_thresh * d_est[level]
 * -- a superset of the reference's candidates --, gathers the EXACT maxima into d_exact[0..4] (zeroed by the
 * caller before phase 1) and the reference's threshold (sift.c:829, 842) is then applied to the marked
 * voxels: candidates and maxima are those of sift3d_hip_dogmax_stack + sift3d_hip_extrema_gauss6_phase.
 * Both return 1 when the configuration is not covered. */
SIFT3D_AMD_API int sift3d_hip_dogmax_sub(const float *const *d_g, int nx, int ny, int nz, float *d_est,
                                         void *stream);
/* Phase 2 (scan + emission) of the two entries above/below for ALL octaves of a call in two launches instead
 * of two per octave: octs[i] = what phase 1 of octave i was given.  Appends to d_out at *d_count in (octave,
 * level, z, y, x) order (sift.c:835-868).  Returns 1 when n_oct exceeds what one launch takes. */
typedef struct {
    const float *const *d_g;   /* the octave's six Gaussian levels */
    int nx, ny, nz;
    int tag0;
    void *d_work;
    size_t work_bytes;
} sift3d_hip_extrema_oct;
#define SIFT3D_HIP_EXTREMA_MAX_OCT 12   /* octaves one sift3d_hip_extrema_gauss6_finish call takes */
SIFT3D_AMD_API int
sift3d_hip_extrema_gauss6_finish(const sift3d_hip_extrema_oct *octs, int n_oct, double peak_thresh,
                                 sift3d_hip_cand *d_out, uint32_t cap, uint32_t *d_count, void *stream);
SIFT3D_AMD_API int
sift3d_hip_extrema_gauss6_est_phase(const float *const *d_g, const float *d_est, float *d_exact, int nx,
                                    int ny, int nz, int tag0, double peak_thresh, sift3d_hip_cand *d_out,
                                    uint32_t cap, uint32_t *d_count, void *d_work, size_t work_bytes,
                                    void *stream, int phase);

/* Geometry of one Gaussian level, as the window kernels see it (a table of these
 * lives in device memory, indexed by the `tag`/`level` of a record). */
typedef struct {
    const float *data;
    int nx, ny, nz;  /* local buffer dims */
    int z_off;       /* global z of local plane 0 */
    int nz_glob;     /* global number of planes (window clipping, sift.c:97-99) */
    float ux, uy, uz;/* (float) units of the level (sift.c:88-90) */
    int octave;
    double sd;       /* level scale (sift.c:860) */
} sift3d_hip_level;

/* assign_eig_ori + assign_orientation_thresh (sift.c:926-1102) for n candidates.
 * d_R: 9 floats per candidate (row-major), d_keep: 1 = kept, 0 = rejected. */
SIFT3D_AMD_API int
sift3d_hip_orient(const sift3d_hip_level *d_levels, const sift3d_hip_cand *d_cand,
                  uint32_t n, double corner_thresh, float *d_R, int32_t *d_keep,
                  void *stream);
/* The same with PARALLEL window sums.  Per level a table of the window's voxel offsets and weights is
 * built (a candidate sits on a voxel, so the reference's per-voxel window expressions depend on the
 * level alone); every lane keeps private double sums of its voxels, a fixed butterfly adds them;
 * every decision (sift.c:997, 1011-1015, 1100) and the float casts of the eigenvectors are accepted
 * only when they hold for every value the reference's serial sums can have, and the remaining
 * candidates (a few per cent) are re-run with the serial sums: keypoint lists and R are those of
 * sift3d_hip_orient bit for bit.  d_tab: device scratch of sift3d_hip_orient_tab_bytes(nlevels,
 * max_cand) bytes (tables, launch plan, ten double sums per candidate, list of the undecided).  The
 * caller ZEROES it once after allocating it: a level's table is kept from call to call while the
 * level's scale, units and strides stay the same (a validity mark + the parameters sit in its
 * header).  nlevels = entries of d_levels; a call with n > max_cand takes the serial path. */
SIFT3D_AMD_API size_t sift3d_hip_orient_tab_bytes(int nlevels, uint32_t max_cand);
SIFT3D_AMD_API int
sift3d_hip_orient_tab(const sift3d_hip_level *d_levels, int nlevels, const sift3d_hip_cand *d_cand,
                      uint32_t n, double corner_thresh, float *d_R, int32_t *d_keep, void *d_tab,
                      uint32_t max_cand, void *stream);
/* (d_tab = NULL: the serial sums for every candidate, = sift3d_hip_orient) */
/* A PART of the candidate list on its own: candidates first .. first + n - 1 (d_cand, d_R, d_keep are the
 * arrays of the WHOLE list), all of levels lv_lo .. lv_hi - 1.  Two parts with disjoint level ranges and
 * different slots (0 or 1: launch plan and undecided list of their own) may run at the same time on two
 * streams over one d_tab: the detector starts octave 0's candidates while the smaller octaves' extrema are
 * still being found.  Results: those of one call over the whole list. */
SIFT3D_AMD_API int
sift3d_hip_orient_tab_part(const sift3d_hip_level *d_levels, int nlevels, int lv_lo, int lv_hi,
                           const sift3d_hip_cand *d_cand, uint32_t first, uint32_t n, double corner_thresh,
                           float *d_R, int32_t *d_keep, void *d_tab, uint32_t max_cand, int slot, void *stream);
/* A LIMIT of all three entries: the serial sums queue a window's voxels with their window-relative x and y in 10
 * bits each, so the clipped window box -- max(floor(c - rad / u), 1) .. min(ceil(c + rad / u), n - 2) with rad =
 * 4.5 sd (sift.c:93-99, 936, 1125) -- may span at most 1024 voxels in x and in y; beyond that the orientations are
 * silently wrong, and from 2048 on the kernel can read outside the box.  The entries do not check it (they see
 * device memory only).  sift3d_hip_orient_window_fits() is the check on the level's numbers alone: 0 when
 * min(n - 2, 2 ceil(4.5 sd / u) + 1) exceeds 1023 on x or y, else 1.  The detector and the slab driver refuse such
 * a level with a message instead of orienting its candidates. */
SIFT3D_AMD_API int sift3d_hip_orient_window_fits(int nx, int ny, double ux, double uy, double sd);

typedef struct {
    float R[9];
    float cx, cy, cz; /* (float) keypoint voxel coordinates in its level, global z */
    int32_t level;
    uint32_t row1;    /* 0: the histogram goes to row i of d_hist (i = position in d_kp);
                       * r + 1: to row r -- lets the caller launch the widest windows first
                       * (longest-job-first keeps the kernel's tail short) */
    double sd;
} sift3d_hip_kp;

/* extract_descrip (sift.c:1442-1536): 768 floats per keypoint into d_hist. */
SIFT3D_AMD_API int
sift3d_hip_describe(const sift3d_hip_level *d_levels, const sift3d_hip_kp *d_kp,
                    uint32_t n, float *d_hist, void *stream);

/* The same with the Gaussian window weights tabulated per level (they are looked up by the
 * integer squared voxel distance instead of one division + expf per window voxel; exact for
 * levels whose spacing is one power of two on all axes, the others fall back).  d_wlut: device
 * scratch of sift3d_hip_describe_wlut_floats(nlevels) floats, rebuilt by every call; nlevels =
 * number of entries of d_levels. */
SIFT3D_AMD_API size_t sift3d_hip_describe_wlut_floats(int nlevels);
SIFT3D_AMD_API int
sift3d_hip_describe_wlut(const sift3d_hip_level *d_levels, int nlevels, const sift3d_hip_kp *d_kp,
                         uint32_t n, float *d_hist, float *d_wlut, void *stream);
/* The full entry: as sift3d_hip_describe_ex with the scratch of the split windows.  The fast kernel sums a window
 * in four parts (ranges of its planes: work items of a quarter of the size shorten the drain of the persistent
 * kernel from ~1 ms to ~0.3 at 512^3) and the wave that finishes a keypoint's last part adds the parts' histograms
 * in part order -- a function of the keypoint alone, so every entry of this family gives the same bits for the
 * same keypoint.  d_part: device scratch of sift3d_hip_describe_part_bytes(n - n_exact) bytes (3.2 KB per part,
 * 12.8 KB per keypoint) or NULL; the entries without the argument allocate it for the call and free it behind a
 * stream synchronisation. */
SIFT3D_AMD_API size_t sift3d_hip_describe_part_bytes(uint32_t n);
SIFT3D_AMD_API int
sift3d_hip_describe_parts(const sift3d_hip_level *d_levels, int nlevels, const sift3d_hip_kp *d_kp,
                          uint32_t n, uint32_t n_exact, float *d_hist, float *d_hist2, float *d_wlut,
                          void *d_part, void *stream);
/* The same with the lattice variant of the fast kernel for the LAST n_lattice records of the list (a launch of
 * its own behind the generic fast one).  The caller's contract for each of those records: it sits on a voxel
 * (cx, cy, cz integral), its sd has the bits of its level's sd, and sift3d_hip_describe_lattice_level() of that
 * level's units and sd is 1.  The variant computes the generic kernel's bits with fewer instructions per voxel;
 * records that do not qualify belong in front of the range. */
SIFT3D_AMD_API int sift3d_hip_describe_lattice_level(float ux, float uy, float uz, double sd);
SIFT3D_AMD_API int
sift3d_hip_describe_lattice(const sift3d_hip_level *d_levels, int nlevels, const sift3d_hip_kp *d_kp,
                            uint32_t n, uint32_t n_exact, uint32_t n_lattice, float *d_hist, float *d_hist2,
                            float *d_wlut, void *d_part, void *stream);
/* The form of the kernel's sample addresses.  A record whose window spans less than 2^31 bytes of its level may be
 * read at a scalar base plus one 32-bit offset per lane instead of 64-bit addresses per lane (same loads, same
 * bits): sift3d_hip_describe_addr32_level() decides for one level descriptor (host memory; no volume is touched)
 * and scale, sift3d_hip_describe_addr32_records() for a host-readable record list and level table.  The _a32 entry
 * is sift3d_hip_describe_lattice with that word (addr32 != 0: every record of the list qualifies); the entries
 * without it take 64-bit addresses.  sift3d_hip_describe_addr_mode() is for tests: 1 forces the 32-bit form on
 * every launch of the process (the caller vouches for the volumes), 2 the 64-bit one, 0 restores the guard; it
 * returns the previous mode. */
SIFT3D_AMD_API int sift3d_hip_describe_addr32_level(const sift3d_hip_level *level, double sd);
SIFT3D_AMD_API int sift3d_hip_describe_addr32_records(const sift3d_hip_level *levels, int nlevels,
                                                      const sift3d_hip_kp *kp, uint32_t n);
SIFT3D_AMD_API int sift3d_hip_describe_addr_mode(int mode);
SIFT3D_AMD_API int
sift3d_hip_describe_lattice_a32(const sift3d_hip_level *d_levels, int nlevels, const sift3d_hip_kp *d_kp,
                                uint32_t n, uint32_t n_exact, uint32_t n_lattice, float *d_hist, float *d_hist2,
                                float *d_wlut, void *d_part, void *stream, int addr32);
/* Test entry: the reciprocal the fast kernels take for the guessed face's determinant (v_rcp_f32 + one Newton
 * step) against 1.0f / x, on the device, for every float of both signs with biased exponent e_lo .. e_lo + n_exp
 * - 1: the number of values whose bits differ and the smallest such bit pattern (0xffffffff: none). */
SIFT3D_AMD_API int sift3d_hip_describe_rcp_check(uint32_t e_lo, uint32_t n_exp, uint64_t *mismatches,
                                                 uint32_t *first_bits, void *stream);
/* Clock probe of the last descriptor launch through d_wlut (the fast kernel -- its lattice launch when there
 * was one --; exact != 0: the reference-order one): shader cycles and ticks of the constant 100 MHz counter during which the launch's first -- persistent --
 * wave was alive.  cycles / (ticks / 1e8) = the clock the device held under the kernel.  Blocks on `stream`. */
SIFT3D_AMD_API int
sift3d_hip_describe_clock(const float *d_wlut, int nlevels, int exact, uint64_t *cycles, uint64_t *ticks,
                          void *stream);
/* The same with a second destination: d_hist2 (device memory, may be NULL) receives a copy of every
 * histogram -- the matcher's input stays in HBM (sift3d_amd_descriptor_store_keep_device). */
SIFT3D_AMD_API int
sift3d_hip_describe_wlut2(const sift3d_hip_level *d_levels, int nlevels, const sift3d_hip_kp *d_kp,
                          uint32_t n, float *d_hist, float *d_hist2, float *d_wlut, void *stream);
/* The same with the first n_exact records computed in the reference's accumulation ORDER and term
 * arithmetic (one histogram, voxels added in scan order, rounded products, sequential double norm): those
 * histograms are the reference's bit for bit, at ~1.5x the time per window voxel.  For windows so wide that
 * a bin receives enough terms for any other summation order to drift past 1e-5 relative of the reference's
 * own sequential float sums (sift.c:1371-1373); see sift3d_amd_detector_set_exact_descriptors. */
SIFT3D_AMD_API int
sift3d_hip_describe_ex(const sift3d_hip_level *d_levels, int nlevels, const sift3d_hip_kp *d_kp, uint32_t n,
                       uint32_t n_exact, float *d_hist, float *d_hist2, float *d_wlut, void *stream);

/* Device stages of the slab driver's keypoint exchange (sift3d_slab.hip): per-(octave, level) counts of a
 * rank's candidates; the rank's block of the all-gather (|DoG| of every candidate, then the kept candidates as
 * 56-byte records {o, s, x, y, z (global), R[9]} in order); the global list built from the gathered blocks
 * (64-byte records {.., strength, pad} behind a 64-byte header whose first int32 is the ranks' status).
 *
 * sift3d_hip_slab_count: d_cnt[2 key] = candidates, d_cnt[2 key + 1] = kept candidates (d_keep != 0) of key
 * (tag / ngl) * K + (tag % ngl - 1), 1 <= nkey <= 256 (else failure); d_cnt is zeroed first, also when n == 0.
 * Contract on the tags: a candidate's tag is the index of its Gaussian level in the level table, o * ngl + s + 1
 * with 0 <= o and 0 <= s < K (K <= ngl - 1), that is tag >= 0 and tag % ngl in 1 ... K, and its key lies below
 * nkey.  The extrema stage produces nothing else; what the kernels do with other tags is not defined.
 * sift3d_hip_slab_pack: n == 0 is a success that touches nothing; more than 256 * 64 * 1024 candidates are refused
 * before any launch.  d_scratch: sift3d_hip_slab_pack_scratch_bytes(n) bytes.  A level has fewer than 2^32 voxels
 * (idx is a uint32); the records' z is idx / (nx ny) + z_off of the candidate's level. */
SIFT3D_AMD_API int sift3d_hip_slab_count(const sift3d_hip_cand *d_cand, const int32_t *d_keep, uint32_t n,
                                         int ngl, int K, int nkey, int32_t *d_cnt, void *stream);
SIFT3D_AMD_API size_t sift3d_hip_slab_pack_scratch_bytes(uint32_t n);
SIFT3D_AMD_API int sift3d_hip_slab_pack(const sift3d_hip_level *d_levels, const sift3d_hip_cand *d_cand,
                                        const int32_t *d_keep, const float *d_R, uint32_t n, int ngl,
                                        float *d_vals, void *d_recs, void *d_scratch, void *stream);
SIFT3D_AMD_API int sift3d_hip_slab_build(const void *d_all, size_t blk_bytes, size_t roff, size_t toff,
                                         int world, int nkey, const uint32_t *d_tab, uint32_t tot_k,
                                         uint32_t tot_c, void *d_out, void *stream);
/* Host only, no device call: the table sift3d_hip_slab_build searches and the layout of a rank's block, from the
 * gathered count blocks (`world` blocks of 2 nkey int32 as sift3d_hip_slab_count writes them, cnt_stride bytes
 * apart).  tab: 2 (nkey world + 1) + 2 world (nkey + 1) words,
 *   [segk: nseg + 1][segc: nseg + 1][ck: world * (nkey + 1)][cc: world * (nkey + 1)],  nseg = nkey * world:
 * segk / segc[key * world + rank] = where segment (key, rank) starts in the global order of the kept / of all
 * candidates (keys major, ranks in slab order inside a key; the last entry is the total), ck / cc[rank * (nkey + 1)
 * + key] = where key starts in the rank's own records / values.  A rank's block is [values: 4 max(maxc, 1) bytes]
 * [records at roff: 56 max(maxk, 1) bytes][status word at toff], each part rounded up to 16 bytes, blk = toff + 16.
 * Failure (nothing promised about tab): NULL pointers, world < 1, nkey outside 1 ... 256, a stride shorter than a
 * block, a negative count, or a total of candidates or of kept candidates that does not fit a uint32_t. */
typedef struct {
    size_t tot_c, tot_k;            /* candidates / kept candidates of all ranks */
    size_t maxc, maxk;              /* the largest rank's */
    size_t roff, toff, blk;         /* byte offsets of the records and the status word in a block; block size */
} sift3d_amd_slab_layout;
SIFT3D_AMD_API int sift3d_amd_slab_table(const void *cnt, size_t cnt_stride, int world, int nkey, uint32_t *tab,
                                         sift3d_amd_slab_layout *lay);

/* Icosahedron face table for the descriptor kernel (init_geometry, sift.c:148-259;
 * per-face constants of cart2bary, sift.c:276-297).  20 records of
 * {v0[3], e1[3], e2[3], t[3], q[3], e2.q, idx[3] (as float)} = 19 floats each. */
#define SIFT3D_HIP_FACE_FLOATS 19
SIFT3D_AMD_API int
sift3d_hip_set_mesh(const float *faces /* 20 * SIFT3D_HIP_FACE_FLOATS */);

/* Order-independent synthetic volume (sift3d_amd/csrc/synth.c) generated on the
 * device: planes [z_off, z_off + nz) of a volume with nx*ny rows. */
SIFT3D_AMD_API int
sift3d_hip_synth_lattice(float *d_dst, int nx, int ny, int nz, int z_off, uint64_t seed,
                         void *stream);

/* Host evaluations of the device math (tests compare them with libm / LAPACK). */
SIFT3D_AMD_API void sift3d_amd_host_expf(const float *in, float *out, size_t n);
SIFT3D_AMD_API void sift3d_amd_host_eigen3(const double *A9, double *Q9, double *L3);
/* The same two routines evaluated ON the device (one thread per element). */
SIFT3D_AMD_API int sift3d_hip_test_expf(const float *d_in, float *d_out, size_t n, void *stream);
SIFT3D_AMD_API int sift3d_hip_test_eigen3(const double *d_A9, double *d_Q9, double *d_L3,
                                          size_t n, void *stream);

SIFT3D_AMD_API const char *sift3d_hip_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
