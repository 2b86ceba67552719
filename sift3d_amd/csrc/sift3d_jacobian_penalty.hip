// sift3d_jacobian_penalty.hip -- the volume (folding) penalty of a displacement field and its derivative with respect
// to the field.  Contract: include/sift3d_amd.h, "Jacobian penalty"; restated in numpy by
// tests/jacobian_penalty_restatement.py (tests/test_jacobian_penalty.py).  The host checks are in sift3d_ffd.c.
//
//   - k_jp_value: k_jacobian_det's walk (sift3d_warp.hip): a 256-lane workgroup is 64 x 4 (x, y) columns, a lane walks
//     JP_K planes of its column and carries u at z - 1, z, z + 1; a wave is 64 consecutive x of one row.  Per voxel the
//     float j, the double det, r = det / ref, phi and phi'.  The record's four statistics are reduced per workgroup
//     (workgroup_reduce) into one slot each of a grid of min(tiles, REDUCE_GRID) workgroups, then by k_jp_finish: no
//     atomics, so the bits of `sum` depend on the shapes only.
//   - the gradient, S_d(q) = sum_e sum_p K_de(p) D_e[p][q], K_de(p) = a(p) C_de(p), a = phi'(r) / ref.  Two designs
//     were on the table: keep the nine K_de of every voxel (72 B written by the value pass and read again by the
//     gather: 180 B per voxel over both passes with the field and S, and a work buffer of 72 B per voxel, 9.7 GB at
//     512^3), or recompute them from the float field with a halo of 2.  Column e of the cofactor matrix does not
//     contain the derivative ALONG e, so K_de(q -+ e) needs u only at q -+ e +- e', e' != e: the halo of 2 shrinks to the
//     12 edge neighbours of q (and its 6 face neighbours for the one-sided ends), all within the 3 x 3 x 3 cube around
//     q, and what is left of K's cost is a(p): a divide by ref, a divide in phi' and the det before them.  So the
//     kernels here do neither of the two as stated: with WITH_A the value pass keeps the ONE double a(p) per voxel
//     (8 B), and k_jp_grad recomputes the six (at an end seven) cofactor columns from the cube.  Algorithmic bytes per
//     voxel: value 12 B (+ 8 B with WITH_A), gradient 12 + 8 + 24 = 44 B, k_ffd_force's 44 B; the work buffer is 8 B
//     per voxel.  Every K_de is the same double in all three designs (a product of the same two doubles) and a lane
//     adds them in the contract's order, so the bits of S do not depend on the choice.  The 72 B design was not built:
//     its traffic alone is 3.0 ms at 512^3 at 8 TB/s (3.8 ms at the 6.3 TB/s that streams reach) against the 4.9 ms the
//     two kernels here take together, so it could be faster by a fifth at best, for nine times the work buffer.
//     No LDS tile either: the cube's rows are the coalesced rows of the neighbouring waves and come from L1 / L2.
//   - measured (profiles/microbench/jacobian_penalty_rate_mi355x.txt, 512^3, kernel trace, min of 5, one run):
//     k_jp_value 1.62 ms without and 1.79 ms with a(p), beside k_jacobian_det's 1.79 ms on the same field (the same
//     walk: bound by load latency, 8 x the 0.20 ms of its 12 B per voxel); k_jp_grad 3.08 ms, 4.2 x the 0.74 ms of its
//     44 B and 2.2 x k_ffd_force's 1.38 ms of the same run.  As one lane per voxel with the cube loaded afresh (57
//     loads; 114 VGPRs, four waves) k_jp_grad took 3.41 ms in an earlier run: the column walk's 27 loads per step buy a
//     tenth, so the loads are not what bounds it; what does (the seven dependent double loads of a(p), the f64 tail at
//     three waves per SIMD) was not separated.  An MSD evaluation with the penalty is 1.94 x one without (14.3 against
//     7.4 ms, HIP events), of which k_jp_grad is 3.1 ms, the value pass 1.8 ms and the second adjoint 2.0 ms.
#include "sift3d_resample.h"
#include "sift3d_ffd_eval.h"

namespace {

constexpr int JP_TX = 64, JP_TY = 4, JP_K = 8;   // a tile: 64 x 4 columns of 8 planes (k_jacobian_det's)
constexpr unsigned JP_GRID = REDUCE_GRID;

struct DMin {
    static __device__ __forceinline__ double op(double a, double b) { return fmin(a, b); }
};

struct JpArgs {
    const float *field;                          // [3][oz][oy][ox]
    double *part;                                // [4][JP_GRID]: sum, nonpos (uint64), rmin, rmax
    double *a;                                   // [oz][oy][ox]: phi'(r) / ref (WITH_A)
    double *S;                                   // [3][oz][oy][ox] (k_jp_grad)
    double ref;
    int ox, oy, oz;
    int tiles_x, tiles_y;
    unsigned ntiles;
};

// phi and phi' of the contract: (r + 1 / r) - 2 from 1/4 up, its second-order Taylor polynomial at 1/4 below (and for a
// NaN, which the polynomial hands on)
__device__ __forceinline__ void jp_phi(double r, double &phi, double &dphi)
{
    if (r >= 0.25) {
        phi = (r + 1.0 / r) - 2.0;
        dphi = 1.0 - 1.0 / (r * r);
    } else {
        const double t = r - 0.25;
        phi = (2.25 - 15.0 * t) + 64.0 * (t * t);
        dphi = -15.0 + 128.0 * t;
    }
}

// <false>: 70 VGPRs, seven waves per SIMD; <true>: 74 VGPRs, six waves; no AGPRs, no scratch
// (-Rpass-analysis=kernel-resource-usage, gfx950).
template <bool WITH_A>
__global__ __launch_bounds__(256) void k_jp_value(const JpArgs p)
{
    __shared__ double s_sum[4], s_min[4], s_max[4];
    __shared__ unsigned long long s_cnt[4];
    const float *__restrict__ field = p.field;
    const size_t sx = (size_t)p.ox, plane = (size_t)p.oy * (size_t)p.ox, vox = plane * (size_t)p.oz;
    unsigned long long cnt = 0;
    double sum = 0.0, rmin = INFINITY, rmax = -INFINITY;
    for (unsigned t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
        const unsigned tyz = t / (unsigned)p.tiles_x;
        const int x = (int)(t - tyz * (unsigned)p.tiles_x) * JP_TX + (int)(threadIdx.x & 63);
        const int y = (int)(tyz % (unsigned)p.tiles_y) * JP_TY + (int)(threadIdx.x >> 6);
        const int z0 = (int)(tyz / (unsigned)p.tiles_y) * JP_K;
        if (x >= p.ox || y >= p.oy)
            continue;
        const size_t col = (size_t)y * sx + (size_t)x;
        const size_t dxm = x > 0 ? 1 : 0, dxp = x + 1 < p.ox ? 1 : 0;          // neighbour offsets, clamped
        const size_t dym = y > 0 ? sx : 0, dyp = y + 1 < p.oy ? sx : 0;
        const int nk = min(JP_K, p.oz - z0);
        float lo[3], c[3], hi[3];                                            // u at z - 1, z, z + 1 of the column
#pragma unroll
        for (int d = 0; d < 3; d++) {
            const float *u = field + (size_t)d * vox + col;
            c[d] = u[(size_t)z0 * plane];
            lo[d] = z0 > 0 ? u[(size_t)(z0 - 1) * plane] : c[d];
        }
        for (int k = 0; k < nk; k++) {
            const int z = z0 + k;
            const size_t o = (size_t)z * plane + col;
            float j[3][3];
#pragma unroll
            for (int d = 0; d < 3; d++) {
                const float *u = field + (size_t)d * vox;
                hi[d] = z + 1 < p.oz ? u[o + plane] : c[d];
                j[d][0] = (d == 0 ? 1.0f : 0.0f) + grad(u[o - dxm], c[d], u[o + dxp], x, p.ox);
                j[d][1] = (d == 1 ? 1.0f : 0.0f) + grad(u[o - dym], c[d], u[o + dyp], y, p.oy);
                j[d][2] = (d == 2 ? 1.0f : 0.0f) + grad(lo[d], c[d], hi[d], z, p.oz);
            }
            const double j00 = j[0][0], j01 = j[0][1], j02 = j[0][2];
            const double j10 = j[1][0], j11 = j[1][1], j12 = j[1][2];
            const double j20 = j[2][0], j21 = j[2][1], j22 = j[2][2];
            const double det = j00 * (j11 * j22 - j12 * j21) - j01 * (j10 * j22 - j12 * j20) +
                               j02 * (j10 * j21 - j11 * j20);
            const double r = det / p.ref;
            double phi, dphi;
            jp_phi(r, phi, dphi);
            sum += phi;
            cnt += !(r > 0.0);
            rmin = fmin(rmin, r);                                            // fmin, fmax: a NaN is passed over
            rmax = fmax(rmax, r);
            if (WITH_A)
                p.a[o] = dphi / p.ref;
#pragma unroll
            for (int d = 0; d < 3; d++) {
                lo[d] = c[d];
                c[d] = hi[d];
            }
        }
    }
    sum = workgroup_reduce<Add>(sum, s_sum);
    cnt = workgroup_reduce<Add>(cnt, s_cnt);
    rmin = workgroup_reduce<DMin>(rmin, s_min);
    rmax = workgroup_reduce<Max>(rmax, s_max);
    if (threadIdx.x == 0) {
        p.part[blockIdx.x] = sum;
        reinterpret_cast<unsigned long long *>(p.part)[JP_GRID + blockIdx.x] = cnt;
        p.part[2 * JP_GRID + blockIdx.x] = rmin;
        p.part[3 * JP_GRID + blockIdx.x] = rmax;
    }
}

// one workgroup: the record {uint64 nonpos; double sum, rmin, rmax} from the n slots of each statistic
__global__ __launch_bounds__(256) void k_jp_finish(const double *part, unsigned n, double *rec)
{
    __shared__ double s_sum[256], s_min[4], s_max[4];
    __shared__ unsigned long long s_cnt[256];
    const double sum = finish_reduce<Add>(part, n, s_sum);
    const unsigned long long cnt =
        finish_reduce<Add>(reinterpret_cast<const unsigned long long *>(part) + JP_GRID, n, s_cnt);
    double rmin = INFINITY, rmax = -INFINITY;
    for (unsigned i = threadIdx.x; i < n; i += 256) {
        rmin = fmin(rmin, part[2 * JP_GRID + i]);
        rmax = fmax(rmax, part[3 * JP_GRID + i]);
    }
    rmin = workgroup_reduce<DMin>(rmin, s_min);
    rmax = workgroup_reduce<Max>(rmax, s_max);
    if (threadIdx.x == 0) {
        reinterpret_cast<unsigned long long *>(rec)[0] = cnt;
        rec[1] = sum;
        rec[2] = rmin;
        rec[3] = rmax;
    }
}

// j_{d e} of the voxel at offset (ax, ay, az) in {-1, 0, 1}^3 from the cube's centre, for the axis e: u[d] is the
// cube of channel d, [z][y][x], loaded at clamped coordinates (a clamped entry is one that grad() does not read)
template <int E>
__device__ __forceinline__ double jp_j(const float (&u)[3][3][3], int d, int ax, int ay, int az, int i, int n)
{
    const float lo = u[az + 1 - (E == 2)][ay + 1 - (E == 1)][ax + 1 - (E == 0)];
    const float c = u[az + 1][ay + 1][ax + 1];
    const float hi = u[az + 1 + (E == 2)][ay + 1 + (E == 1)][ax + 1 + (E == 0)];
    return (double)((d == E ? 1.0f : 0.0f) + grad(lo, c, hi, i, n));
}

// S_d += (a(p) * C_de(p)) * coef for d = 0, 1, 2, p = q + STEP along axis E: column E of the cofactor matrix of j(p), each
// entry the difference of two exact products, from the derivatives along the other two axes E1 < E2
template <int E, int STEP>
__device__ __forceinline__ void jp_term(const float (&u)[3][3][3][3], double a, double coef, const int (&q)[3],
                                        const int (&n)[3], double (&S)[3])
{
    constexpr int E1 = E == 0 ? 1 : 0, E2 = E == 2 ? 1 : 2;
    constexpr int ax = E == 0 ? STEP : 0, ay = E == 1 ? STEP : 0, az = E == 2 ? STEP : 0;
    double j1[3], j2[3];                                                     // j_{d E1}(p), j_{d E2}(p)
#pragma unroll
    for (int d = 0; d < 3; d++) {
        j1[d] = jp_j<E1>(u[d], d, ax, ay, az, q[E1], n[E1]);
        j2[d] = jp_j<E2>(u[d], d, ax, ay, az, q[E2], n[E2]);
    }
    // C_dE = (-1)^(d + E) * minor: rows d1 < d2 != d, columns E1 < E2; written as one difference with its sign
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const int d1 = d == 0 ? 1 : 0, d2 = d == 2 ? 1 : 2;
        const double m = ((d + E) & 1) ? j1[d2] * j2[d1] - j1[d1] * j2[d2] : j1[d1] * j2[d2] - j1[d2] * j2[d1];
        S[d] = S[d] + (a * m) * coef;
    }
}

// the (up to three) terms of axis E at the voxel whose coordinate along E is i of n: p = q - 1, q, q + 1 ascending, each
// with numpy.gradient's coefficient D_E[p][q]; a p with D_E[p][q] == 0 adds nothing (not even a zero)
template <int E>
__device__ __forceinline__ void jp_axis(const float (&u)[3][3][3][3], const double *a, size_t o, size_t stride,
                                        const int (&q)[3], const int (&n)[3], double (&S)[3])
{
    const int i = q[E], m = n[E];
    if (m == 1)
        return;
    if (i >= 1)
        jp_term<E, -1>(u, a[o - stride], i == 1 ? 1.0 : 0.5, q, n, S);
    if (i == 0 || i == m - 1)
        jp_term<E, 0>(u, a[o], i == 0 ? -1.0 : 1.0, q, n, S);
    if (i + 1 <= m - 1)
        jp_term<E, 1>(u, a[o + stride], i + 1 == m - 1 ? -1.0 : -0.5, q, n, S);
}

// One lane owns the three S_d of one voxel, and walks the JP_K voxels of its column in the value pass' tiling: the cube
// moves up with it, so a step loads one plane of it, 9 points of 3 channels (the plane's corners are not needed while
// it is the cube's top, but are once it is the middle), where a lane per voxel loads the 19 points it needs afresh.
// 146 VGPRs, no AGPRs, no scratch, three waves per SIMD (-Rpass-analysis=kernel-resource-usage, gfx950).
__global__ __launch_bounds__(256) void k_jp_grad(const JpArgs p)
{
    const float *__restrict__ field = p.field;
    const double *__restrict__ a = p.a;
    const size_t sx = (size_t)p.ox, plane = (size_t)p.oy * (size_t)p.ox, vox = plane * (size_t)p.oz;
    const int n[3] = {p.ox, p.oy, p.oz};
    for (unsigned t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
        const unsigned tyz = t / (unsigned)p.tiles_x;
        const int x = (int)(t - tyz * (unsigned)p.tiles_x) * JP_TX + (int)(threadIdx.x & 63);
        const int y = (int)(tyz % (unsigned)p.tiles_y) * JP_TY + (int)(threadIdx.x >> 6);
        const int z0 = (int)(tyz / (unsigned)p.tiles_y) * JP_K;
        if (x >= p.ox || y >= p.oy)
            continue;
        size_t col[3][3];                                                    // the 9 columns around (x, y), clamped
#pragma unroll
        for (int cy = 0; cy < 3; cy++)
#pragma unroll
            for (int cx = 0; cx < 3; cx++)
                col[cy][cx] = (size_t)clampi(y + cy - 1, 0, p.oy - 1) * sx + (size_t)clampi(x + cx - 1, 0, p.ox - 1);
        float u[3][3][3][3];                                                 // [d][z][y][x] around the lane's voxel
#pragma unroll
        for (int cz = 0; cz < 2; cz++) {
            const size_t at = (size_t)clampi(z0 + cz - 1, 0, p.oz - 1) * plane;
#pragma unroll
            for (int d = 0; d < 3; d++)
#pragma unroll
                for (int cy = 0; cy < 3; cy++)
#pragma unroll
                    for (int cx = 0; cx < 3; cx++)
                        u[d][cz][cy][cx] = field[(size_t)d * vox + at + col[cy][cx]];
        }
        const int nk = min(JP_K, p.oz - z0);
        for (int k = 0; k < nk; k++) {
            const int q[3] = {x, y, z0 + k};
            const size_t at = (size_t)clampi(q[2] + 1, 0, p.oz - 1) * plane;
#pragma unroll
            for (int d = 0; d < 3; d++)
#pragma unroll
                for (int cy = 0; cy < 3; cy++)
#pragma unroll
                    for (int cx = 0; cx < 3; cx++)
                        u[d][2][cy][cx] = field[(size_t)d * vox + at + col[cy][cx]];
            const size_t o = (size_t)q[2] * plane + col[1][1];
            double S[3] = {0.0, 0.0, 0.0};
            jp_axis<0>(u, a, o, 1, q, n, S);
            jp_axis<1>(u, a, o, sx, q, n, S);
            jp_axis<2>(u, a, o, plane, q, n, S);
#pragma unroll
            for (int d = 0; d < 3; d++) {
                p.S[(size_t)d * vox + o] = S[d];
#pragma unroll
                for (int cy = 0; cy < 3; cy++)
#pragma unroll
                    for (int cx = 0; cx < 3; cx++) {
                        u[d][0][cy][cx] = u[d][1][cy][cx];
                        u[d][1][cy][cx] = u[d][2][cy][cx];
                    }
            }
        }
    }
}

} // namespace

// For sift3d_ffd.c and sift3d_ffd.hip, which have checked every argument (not exported from the library).
// d_work: the partial slots [4][JP_GRID] doubles, then a [oz][oy][ox] doubles (written and read with d_S only).
// d_rec: {uint64 nonpos; double sum, rmin, rmax}.  d_S == NULL: the value alone.
extern "C" int sift3d_jacobian_penalty_launch(const char *fn, const float *d_field, int ox, int oy, int oz, double ref,
                                              double *d_rec, double *d_S, double *d_work, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    JpArgs p;
    p.field = d_field;
    p.part = d_work;
    p.a = d_work + 4 * (size_t)JP_GRID;
    p.S = d_S;
    p.ref = ref;
    p.ox = ox; p.oy = oy; p.oz = oz;
    p.tiles_x = (ox + JP_TX - 1) / JP_TX;
    p.tiles_y = (oy + JP_TY - 1) / JP_TY;
    const unsigned long long nt = (unsigned long long)p.tiles_x * p.tiles_y * ((oz + JP_K - 1) / JP_K);
    if (nt > 0xffffffffull - MAX_GRID)
        return launch_fail(fn, "grid too large");
    p.ntiles = (unsigned)nt;
    const unsigned grid = reduce_grid(p.ntiles);
    hipLaunchKernelGGL(d_S ? k_jp_value<true> : k_jp_value<false>, dim3(grid), dim3(256), 0, st, p);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_jp_finish, dim3(1), dim3(256), 0, st, (const double *)d_work, grid, d_rec);
    LAUNCH_CHECK();
    if (d_S) {
        hipLaunchKernelGGL(k_jp_grad, dim3(p.ntiles < MAX_GRID ? p.ntiles : MAX_GRID), dim3(256), 0, st, p);
        LAUNCH_CHECK();
    }
    return SIFT3D_SUCCESS;
}
