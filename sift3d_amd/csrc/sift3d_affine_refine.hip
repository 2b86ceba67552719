// sift3d_affine_refine.hip -- the Gauss-Newton normal equations of the mean squared difference over the 12 parameters
// of an affine pull map, in one gather-and-reduce pass over the fixed grid.
// Contract: include/sift3d_amd.h, "Intensity-driven affine refinement"; restated in numpy by
// tests/affine_refine_restatement.py (tests/test_affine_refine.py).
//
// The pass is k_similarity<LINEAR, affine> (sift3d_similarity.hip) with the histogram replaced by 73 double sums: the
// tiles, tile order, XCD grouping, pull map, inside test and sample are sift3d_resample.h's, so m is the warp's value
// bit for bit; the gradient of the sample comes from the eight corner values the gather holds (gather_grad).  Per
// voxel 8 B read, nothing written, a few hundred f64 operations: by the arithmetic of DESIGN.md 3.4.8 the pass is bound
// by f64 VALU work and registers, not by HBM.
//   - sums: with P = (X, Y, Z, 1) the centred position and G the gradient, H[4d+j][4e+k] = sum G_d G_e P_j P_k has 60
//     distinct values (6 pairs d <= e x 10 pairs j <= k) and b[4d+j] = sum G_d E P_j has 12; with S_ee, 73 doubles and
//     the count.  Statistic s = 10 * pair(d, e) + pair(j, k) for H, 60 + 4 d + j for b, 72 for S_ee, 73 the count;
//   - factored (the default): a lane's y and z are fixed within a tile and it visits 4 values of x, so per voxel it
//     adds w, w X and (w X) X for the 9 quantities w in {G_d G_e, G_d E} into tile sums (24 adds: b needs no X X),
//     and once per tile folds those into the 72 accumulators with the tile's Y, Z, Y Y, Y Z, Z Z.  A voxel that is
//     not counted enters with G = 0 and E = 0, so that the loop has no branches;
//   - direct (-DSIFT3D_AFFINE_REFINE_NAIVE, kept for profiles/microbench/affine_refine_rate.py): every accumulator
//     takes w * (P_j P_k) per voxel, 72 multiplies and 72 adds;
//   - grid: min(tiles, SIFT3D_AMD_SIMILARITY_GRID) workgroups walk the tiles; the size does not depend on the device,
//     so the bits of the sums depend on the shapes only.  Per-lane sums, the wave by butterfly, the four waves through
//     LDS as ((w0 + w1) + w2) + w3 into partial slot blockIdx.x, then one finish workgroup per statistic adds the
//     slots in finish_reduce's fixed order and writes every entry of the record that holds its value: H comes out
//     full and symmetric bit for bit.
//
// k_affine_ncc_normal (below) is the same pass for the fit under a linear intensity map (header, "Affine refinement
// under a linear intensity map (NCC)"): 101 double sums and the count, in two launches of 73 and 28 sums.
// k_parzen_hist and k_affine_mi_normal (at the end) are the two passes of the fit under an unknown intensity map
// (header, "Mutual-information affine refinement (Mattes)").
#include "sift3d_resample.h"
#include "sift3d_parzen.h"

namespace {

constexpr unsigned AFF_GRID = REDUCE_GRID;
constexpr int AFF_H = 60, AFF_B = 12;
constexpr int AFF_SUMS = AFF_H + AFF_B + 1;      // doubles: H's distinct values, b, S_ee
constexpr int AFF_STATS = AFF_SUMS + 1;          // and the count

struct AffArgs {
    double a[12];
    double cx, cy, cz;                           // the centre of the fixed grid
    GridArgs g;                                  // src = M; ox, oy, oz = F's grid; dst unused
    const float *F;
    double *part;                                // [AFF_STATS][AFF_GRID]; row 73 holds uint64
    MaskArgs w;                                  // MASKED == true: wf on F's grid, wm on M's; either may be null
};

__host__ __device__ constexpr int pair3(int d, int e) { return d == 0 ? e : d == 1 ? 2 + e : 5; }           // d <= e < 3
__host__ __device__ constexpr int pair4(int j, int k) { return j == 0 ? k : j == 1 ? 3 + k : j == 2 ? 5 + k : 9; }   // j <= k < 4

// ---- what the record kernels share -----------------------------------------------------------------------------------
// One tile's samples for a lane, the two-stage front-end (the one-stage form is sift3d_resample.h's tile_front): its
// four outputs' f, m and gradient, and whether each is counted (live, inside the moving grid and, MASKED, in both
// masks).
struct TileSamples {
    float f[4], m[4], gx[4], gy[4], gz[4];
    bool counted[4];
};

template <int LINEAR, bool MASKED>
__device__ __forceinline__ void tile_samples(const AffArgs &s, int xt, int y, int z, int lx, TileSamples &t)
{
    const GridArgs &p = s.g;
    const bool row = y < p.oy && z < p.oz;
    const size_t orow = ((size_t)z * (size_t)p.oy + (size_t)y) * (size_t)p.ox;
    const double yd = (double)y, zd = (double)z;
    const double rx = pull_row(s.a, yd, zd), ry = pull_row(s.a + 4, yd, zd), rz = pull_row(s.a + 8, yd, zd);
    // MASKED: the two mask values of the lane's four outputs first, all eight loads in flight together, kept as
    // four flags.  The accumulators leave no registers to hold them across the intensity gathers (it spills);
    // the stage costs one more round trip per tile (measured: DESIGN.md 3.4.10).  q is pull()'s three
    // multiply-adds per output, computed here and again in the taps loop rather than kept in 24 registers.
    bool ok[4] = {true, true, true, true};
    if (MASKED) {
        float wf[4], wm[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int x = xt + lx + 16 * k;
            const double xd = (double)x;
            const double qx = pull(s.a, xd, rx), qy = pull(s.a + 4, xd, ry), qz = pull(s.a + 8, xd, rz);
            wf[k] = s.w.wf && row && x < p.ox ? s.w.wf[orow + (size_t)x] : 1.0f;
            wm[k] = s.w.wm ? s.w.wm[mask_offset(p.nx, p.ny, p.nz, qx, qy, qz)] : 1.0f;
        }
#pragma unroll
        for (int k = 0; k < 4; k++)
            ok[k] = mask_in(wf[k]) && mask_in(wm[k]);
    }
    Taps tp[4];
    bool live[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int x = xt + lx + 16 * k;
        live[k] = row && x < p.ox;
        t.f[k] = live[k] ? s.F[orow + (size_t)x] : 0.0f;
        const double xd = (double)x;
        tp[k] = taps_at<LINEAR>(p.nx, p.ny, p.nz, pull(s.a, xd, rx), pull(s.a + 4, xd, ry), pull(s.a + 8, xd, rz));
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        t.m[k] = gather_grad<LINEAR>(p.src, tp[k], &t.gx[k], &t.gy[k], &t.gz[k]);
        t.counted[k] = MASKED ? live[k] && tp[k].in && ok[k] : live[k] && tp[k].in;
    }
}

// The per-tile factoring (top of the file).  A voxel adds w, w X (and, for H, (w X) X) into the tile's sums,
__device__ __forceinline__ void tile_add(double w, double X, double &s0, double &s1)
{
    s0 += w;
    s1 += w * X;
}

__device__ __forceinline__ void tile_add(double w, double X, double &s0, double &s1, double &s2)
{
    const double wx = w * X;
    s0 += w;
    s1 += wx;
    s2 += wx * X;
}

// once per tile the sums of a pair G_d G_e fold into its ten accumulators (P_j P_k, j <= k),
__device__ __forceinline__ void fold_pair(double *h, double s0, double s1, double s2, double Y, double Z, double YY,
                                          double YZ, double ZZ)
{
    h[0] += s2;                                                          // X X
    h[1] += s1 * Y;                                                      // X Y
    h[2] += s1 * Z;                                                      // X Z
    h[3] += s1;                                                          // X 1
    h[4] += s0 * YY;
    h[5] += s0 * YZ;
    h[6] += s0 * Y;
    h[7] += s0 * ZZ;
    h[8] += s0 * Z;
    h[9] += s0;
}

// and those of a quantity with one factor J (G_d E, G_d, G_d m, G_d f) into its four (P_j).
__device__ __forceinline__ void fold_row(double *b, double s0, double s1, double Y, double Z)
{
    b[0] += s1;
    b[1] += s0 * Y;
    b[2] += s0 * Z;
    b[3] += s0;
}

// a lane's value summed over its wave by butterfly (s = 32 .. 1)
template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1)
        v += __shfl_xor(v, sft);
    return v;
}

struct EverySum {
    __device__ constexpr bool operator()(int) const { return true; }
};

// The epilogue of the record kernels.  value(i), i = 0 .. NSUMS - 1, are the lane's sums and cnt its count (statistic
// NSUMS).  Each: the wave by butterfly (wave_sum), then the four waves' values through LDS as ((w0 + w1) + w2) + w3
// into partial slot blockIdx.x of row i of part [NSUMS + 1][AFF_GRID] (the count's row holds uint64).  in_part(i): the
// statistics this kernel writes (the NCC record is summed by two kernels).
template <int NSUMS, typename Value, typename InPart = EverySum>
__device__ __forceinline__ void record_slots(double *part, Value value, unsigned long long cnt,
                                             InPart in_part = InPart())
{
    __shared__ double slot[NSUMS * 4];
    __shared__ unsigned long long cslot[4];
    const int wave = threadIdx.x >> 6;
    const bool lead = (threadIdx.x & 63) == 0;
#pragma unroll
    for (int i = 0; i < NSUMS; i++) {
        if (!in_part(i))
            continue;
        const double v = wave_sum(value(i));
        if (lead)
            slot[4 * i + wave] = v;
    }
    cnt = wave_sum(cnt);
    if (lead)
        cslot[wave] = cnt;
    __syncthreads();
    if (!in_part((int)threadIdx.x))
        return;
    if (threadIdx.x < NSUMS) {
        const double *v = slot + 4 * threadIdx.x;
        part[(size_t)threadIdx.x * AFF_GRID + blockIdx.x] = ((v[0] + v[1]) + v[2]) + v[3];
    } else if (threadIdx.x == NSUMS) {
        reinterpret_cast<unsigned long long *>(part)[(size_t)NSUMS * AFF_GRID + blockIdx.x] =
            ((cslot[0] + cslot[1]) + cslot[2]) + cslot[3];
    }
}

// The head of the finish kernels: workgroup st = blockIdx.x adds the partial slots 0 .. n-1 of statistic st in a fixed
// order (finish_reduce).  The count (st == NSUMS) goes to rec[0] as uint64; true for the one lane that has a sum v to
// place in the record.
template <int NSUMS>
__device__ __forceinline__ bool finish_head(const double *part, unsigned n, double *rec, double &v)
{
    __shared__ double s_sum[256];
    __shared__ unsigned long long s_cnt[256];
    const int st = blockIdx.x;
    if (st == NSUMS) {
        const unsigned long long c =
            finish_reduce<Add>(reinterpret_cast<const unsigned long long *>(part) + (size_t)st * AFF_GRID, n, s_cnt);
        if (threadIdx.x == 0)
            reinterpret_cast<unsigned long long *>(rec)[0] = c;
        return false;
    }
    v = finish_reduce<Add>(part + (size_t)st * AFF_GRID, n, s_sum);
    return threadIdx.x == 0;
}

// (256, 2): the 72 accumulators are 144 VGPRs; the compiler reports 256 VGPRs (248 MASKED), two waves per SIMD and
// nothing spilled (-Rpass-analysis=kernel-resource-usage).  Measured
// (profiles/microbench/affine_refine_rate_mi355x.txt): 0.888 ms per pass at 512^3, 1.63 x k_similarity's on the same
// volumes; the direct formulation takes 1.086 ms.
// MASKED (header, "Masks"): a masked-out voxel enters with G = 0 and E = 0 like an outside one.
// This kernel alone is written out, front-end, tile sums, fold and epilogue, and not on the shared pieces above: its
// allocation sits on the 256-VGPR limit and every shared form spills, in bytes of scratch per lane over <1, false>,
// <1, true>, <2, false>, <2, true> (profiles/microbench/registration_front_end_mi355x.txt):
//   record_slots alone, the loop as it is                36,  0, 20,  0   (the same with the lambda's captures by
//     value, with an array in its place, with the LDS declared here, and with a scheduling barrier per statistic);
//   and fold_pair / fold_row                             36,  0, 20,  0;
//   tile_samples, tile_add, the folds and record_slots   44, 56, 20, 28   (this is k_affine_mi_normal's text with
//     E = e and G = g: the one template of the two kernels);
//   tile_samples and the folds, the epilogue inline      44, 56, 20, 24.
// So what changes in tile_samples, the tile sums or record_slots changes here too, by hand.
template <int LINEAR, bool MASKED>
__global__ __launch_bounds__(256, 2) void k_affine_normal(const AffArgs s)
{
    __shared__ double slot[AFF_SUMS * 4];
    __shared__ unsigned long long cslot[4];
    const GridArgs &p = s.g;
    const int lx = threadIdx.x & 15;
    unsigned long long cnt = 0;
    double see = 0.0;
    double acc[AFF_H + AFF_B];
#pragma unroll
    for (int i = 0; i < AFF_H + AFF_B; i++)
        acc[i] = 0.0;
    for (unsigned base = 0; base < p.ntiles; base += gridDim.x) {
        int xt, y, z;
        if (!tile_at(p, base, xt, y, z))
            break;
        const bool row = y < p.oy && z < p.oz;
        const size_t orow = ((size_t)z * (size_t)p.oy + (size_t)y) * (size_t)p.ox;
        const double yd = (double)y, zd = (double)z;
        const double rx = pull_row(s.a, yd, zd), ry = pull_row(s.a + 4, yd, zd), rz = pull_row(s.a + 8, yd, zd);
        // MASKED: the two mask values of the lane's four outputs first, all eight loads in flight together, kept as
        // four flags.  The 72 accumulators leave no registers to hold them across the intensity gathers (it spills);
        // the stage costs one more round trip per tile (measured: DESIGN.md 3.4.10).  q is pull()'s three
        // multiply-adds per output, computed here and again in the taps loop rather than kept in 24 registers.
        bool ok[4] = {true, true, true, true};
        if (MASKED) {
            float wf[4], wm[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int x = xt + lx + 16 * k;
                const double xd = (double)x;
                const double qx = pull(s.a, xd, rx), qy = pull(s.a + 4, xd, ry), qz = pull(s.a + 8, xd, rz);
                wf[k] = s.w.wf && row && x < p.ox ? s.w.wf[orow + (size_t)x] : 1.0f;
                wm[k] = s.w.wm ? s.w.wm[mask_offset(p.nx, p.ny, p.nz, qx, qy, qz)] : 1.0f;
            }
#pragma unroll
            for (int k = 0; k < 4; k++)
                ok[k] = mask_in(wf[k]) && mask_in(wm[k]);
        }
        Taps tp[4];
        float f[4];
        bool live[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int x = xt + lx + 16 * k;
            live[k] = row && x < p.ox;
            f[k] = live[k] ? s.F[orow + (size_t)x] : 0.0f;
            const double xd = (double)x;
            tp[k] = taps_at<LINEAR>(p.nx, p.ny, p.nz, pull(s.a, xd, rx), pull(s.a + 4, xd, ry), pull(s.a + 8, xd, rz));
        }
        float m[4], gx[4], gy[4], gz[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
            m[k] = gather_grad<LINEAR>(p.src, tp[k], &gx[k], &gy[k], &gz[k]);
        const double Y = yd - s.cy, Z = zd - s.cz;
#ifndef SIFT3D_AFFINE_REFINE_NAIVE
        double s0[9], s1[9], s2[6];
#pragma unroll
        for (int i = 0; i < 9; i++)
            s0[i] = s1[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 6; i++)
            s2[i] = 0.0;
#endif
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool counted = MASKED ? live[k] && tp[k].in && ok[k] : live[k] && tp[k].in;
            const float e = m[k] - f[k];
            const double E = counted ? (double)e : 0.0;
            const double G[3] = {counted ? (double)gx[k] : 0.0, counted ? (double)gy[k] : 0.0,
                                 counted ? (double)gz[k] : 0.0};
            const double X = (double)(xt + lx + 16 * k) - s.cx;
            cnt += counted ? 1u : 0u;
            see += E * E;
#ifndef SIFT3D_AFFINE_REFINE_NAIVE
#pragma unroll
            for (int d = 0; d < 3; d++) {
#pragma unroll
                for (int e2 = d; e2 < 3; e2++) {
                    const int i = pair3(d, e2);
                    const double w = G[d] * G[e2];                           // exact: two floats
                    const double wx = w * X;
                    s0[i] += w;
                    s1[i] += wx;
                    s2[i] += wx * X;
                }
                const double w = G[d] * E;
                s0[6 + d] += w;
                s1[6 + d] += w * X;
            }
#else
            const double P[4] = {X, Y, Z, 1.0};
#pragma unroll
            for (int d = 0; d < 3; d++) {
#pragma unroll
                for (int e2 = d; e2 < 3; e2++) {
                    const double w = G[d] * G[e2];
#pragma unroll
                    for (int j = 0; j < 4; j++)
#pragma unroll
                        for (int k2 = j; k2 < 4; k2++)
                            acc[10 * pair3(d, e2) + pair4(j, k2)] += w * (P[j] * P[k2]);
                }
                const double w = G[d] * E;
#pragma unroll
                for (int j = 0; j < 4; j++)
                    acc[AFF_H + 4 * d + j] += w * P[j];
            }
#endif
        }
#ifndef SIFT3D_AFFINE_REFINE_NAIVE
        const double YY = Y * Y, YZ = Y * Z, ZZ = Z * Z;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            double *h = acc + 10 * i;
            h[0] += s2[i];                                                   // X X
            h[1] += s1[i] * Y;                                               // X Y
            h[2] += s1[i] * Z;                                               // X Z
            h[3] += s1[i];                                                   // X 1
            h[4] += s0[i] * YY;
            h[5] += s0[i] * YZ;
            h[6] += s0[i] * Y;
            h[7] += s0[i] * ZZ;
            h[8] += s0[i] * Z;
            h[9] += s0[i];
        }
#pragma unroll
        for (int d = 0; d < 3; d++) {
            double *b = acc + AFF_H + 4 * d;
            b[0] += s1[6 + d];
            b[1] += s0[6 + d] * Y;
            b[2] += s0[6 + d] * Z;
            b[3] += s0[6 + d];
        }
#endif
    }
    // the wave by butterfly (s = 32 .. 1), then the four waves' values through LDS as ((w0 + w1) + w2) + w3
    const int wave = threadIdx.x >> 6;
    const bool lead = (threadIdx.x & 63) == 0;
#pragma unroll
    for (int i = 0; i < AFF_SUMS; i++) {
        double v = i < AFF_H + AFF_B ? acc[i] : see;
#pragma unroll
        for (int sft = 32; sft >= 1; sft >>= 1)
            v += __shfl_xor(v, sft);
        if (lead)
            slot[4 * i + wave] = v;
    }
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1)
        cnt += __shfl_xor(cnt, sft);
    if (lead)
        cslot[wave] = cnt;
    __syncthreads();
    if (threadIdx.x < AFF_SUMS) {
        const double *v = slot + 4 * threadIdx.x;
        s.part[(size_t)threadIdx.x * AFF_GRID + blockIdx.x] = ((v[0] + v[1]) + v[2]) + v[3];
    } else if (threadIdx.x == AFF_SUMS) {
        reinterpret_cast<unsigned long long *>(s.part)[(size_t)AFF_SUMS * AFF_GRID + blockIdx.x] =
            ((cslot[0] + cslot[1]) + cslot[2]) + cslot[3];
    }
}

// every entry of the full H[12][12] that holds the distinct value st = 10 * pair3(d, e) + pair4(j, k)
__device__ void scatter_h(double *H, int st, double v)
{
    for (int d = 0; d < 3; d++)
        for (int e = d; e < 3; e++)
            for (int j = 0; j < 4; j++)
                for (int k = j; k < 4; k++) {
                    if (10 * pair3(d, e) + pair4(j, k) != st)
                        continue;
                    H[(4 * d + j) * 12 + 4 * e + k] = v;
                    H[(4 * d + k) * 12 + 4 * e + j] = v;
                    H[(4 * e + j) * 12 + 4 * d + k] = v;
                    H[(4 * e + k) * 12 + 4 * d + j] = v;
                }
}

// Workgroup s adds the partial slots 0 .. n-1 of statistic s in a fixed order (finish_reduce) and writes every entry
// of the record {uint64 n; double S_ee; double b[12]; double H[12][12]} that holds it.
__global__ __launch_bounds__(256) void k_affine_normal_finish(const double *part, unsigned n, double *rec)
{
    const int st = blockIdx.x;
    double v;
    if (!finish_head<AFF_SUMS>(part, n, rec, v))
        return;
    double *b = rec + 2, *H = rec + 2 + AFF_B;
    if (st == AFF_SUMS - 1) {
        rec[1] = v;
    } else if (st >= AFF_H) {
        b[st - AFF_H] = v;
    } else {
        scatter_h(H, st, v);
    }
}

// ---- the fit under a linear intensity map (NCC) ----------------------------------------------------------------------
// Statistic s: H as above (0 .. 59), then v = sum J m (60 + 4 d + j), u = sum J (72 + ..), w = sum J f (84 + ..), the
// moments S_m, S_f, S_mm, S_fm, S_ff (96 .. 100) and the count (101).
constexpr int NCC_V = AFF_H, NCC_U = NCC_V + 12, NCC_W = NCC_U + 12, NCC_MOM = NCC_W + 12;
constexpr int NCC_SUMS = NCC_MOM + 5;            // doubles
constexpr int NCC_STATS = NCC_SUMS + 1;          // and the count

// The record is summed by two kernels: PART 1 holds H, v, S_mm and the count (k_affine_normal's 72 + 1 sums with m in
// the place of E), PART 2 the other 28 (u, w, S_m, S_f, S_fm, S_ff).  PART 0 is the whole record in one kernel, built with
// -DSIFT3D_AFFINE_NCC_ONE_KERNEL and kept for profiles/microbench/affine_refine_rate.py.  A statistic's chain of
// additions is the same in either, so the two builds write the same bytes.
__host__ __device__ constexpr bool ncc_in_part(int part, int st)
{
    return part == 0 || (part == 1) == (st < NCC_U || st == NCC_MOM + 2 || st == NCC_SUMS);
}

// The register budget decides the split.  The 96 accumulators and the 5 moments are 202 VGPRs and a tile's 36 sums 72
// more, past the 256 that two waves per SIMD leave a lane.  As reported by -Rpass-analysis=kernel-resource-usage:
//   PART 0, (256, 1): 256 VGPRs + 62 - 83 AGPRs, one wave per SIMD, no scratch (at (256, 2) it spills over a hundred
//                     VGPRs): half the waves are left to hide the gather's latency;
//   PART 1, (256, 2): 245 - 249 VGPRs, no AGPRs, two waves per SIMD, no scratch;
//   PART 2, (256, 2): 143 - 160 VGPRs, no AGPRs, three waves per SIMD, no scratch (bounded to four waves, 128 VGPRs, it
//                     spills 7 - 33 of them; not measured).
// Measured (profiles/microbench/affine_ncc_rate_mi355x.txt, 512^3, all in one run): k_affine_normal's pass 0.885 ms,
// the one kernel 2.790 ms (3.15 x), the two kernels together 1.722 ms (1.95 x): one wave per SIMD costs more than a
// second gather of the volumes does, so the two kernels are the default.
// The sums of H are tile_add's and fold_pair's on the same G_d G_e as k_affine_normal's (written out there), so H is
// that kernel's bit for bit.  A voxel that is not counted enters with G = 0, m = 0 and f = 0.
template <int LINEAR, bool MASKED, int PART>
__global__ __launch_bounds__(256, PART == 0 ? 1 : 2) void k_affine_ncc_normal(const AffArgs s)
{
    constexpr bool HV = PART != 2, UW = PART != 1;
    const GridArgs &p = s.g;
    const int lx = threadIdx.x & 15;
    unsigned long long cnt = 0;
    double acc[NCC_SUMS];                                                    // the part's own are live, the rest go
#pragma unroll
    for (int i = 0; i < NCC_SUMS; i++)
        acc[i] = 0.0;
    for (unsigned base = 0; base < p.ntiles; base += gridDim.x) {
        int xt, y, z;
        if (!tile_at(p, base, xt, y, z))
            break;
        TileSamples t;
        tile_samples<LINEAR, MASKED>(s, xt, y, z, lx, t);
        // tile sums: 0 .. 5 the pairs G_d G_e, 6 + d: G_d m, 9 + d: G_d, 12 + d: G_d f
        double s0[15], s1[15], s2[6];
#pragma unroll
        for (int i = 0; i < 15; i++)
            s0[i] = s1[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 6; i++)
            s2[i] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool counted = t.counted[k];
            const double m = counted ? (double)t.m[k] : 0.0, f = counted ? (double)t.f[k] : 0.0;
            const double G[3] = {counted ? (double)t.gx[k] : 0.0, counted ? (double)t.gy[k] : 0.0,
                                 counted ? (double)t.gz[k] : 0.0};
            const double X = (double)(xt + lx + 16 * k) - s.cx;
            cnt += counted ? 1u : 0u;
            acc[NCC_MOM + 0] += m;
            acc[NCC_MOM + 1] += f;
            acc[NCC_MOM + 2] += m * m;                                       // exact: two floats
            acc[NCC_MOM + 3] += f * m;
            acc[NCC_MOM + 4] += f * f;
#pragma unroll
            for (int d = 0; d < 3; d++) {
                if (HV) {
#pragma unroll
                    for (int e2 = d; e2 < 3; e2++) {
                        const int i = pair3(d, e2);
                        tile_add(G[d] * G[e2], X, s0[i], s1[i], s2[i]);
                    }
                    tile_add(G[d] * m, X, s0[6 + d], s1[6 + d]);
                }
                if (UW) {
                    tile_add(G[d], X, s0[9 + d], s1[9 + d]);
                    tile_add(G[d] * f, X, s0[12 + d], s1[12 + d]);
                }
            }
        }
        const double Y = (double)y - s.cy, Z = (double)z - s.cz;
        if (HV) {
            const double YY = Y * Y, YZ = Y * Z, ZZ = Z * Z;
#pragma unroll
            for (int i = 0; i < 6; i++)
                fold_pair(acc + 10 * i, s0[i], s1[i], s2[i], Y, Z, YY, YZ, ZZ);
#pragma unroll
            for (int d = 0; d < 3; d++)
                fold_row(acc + NCC_V + 4 * d, s0[6 + d], s1[6 + d], Y, Z);
        }
        if (UW) {
#pragma unroll
            for (int d = 0; d < 3; d++) {
                fold_row(acc + NCC_U + 4 * d, s0[9 + d], s1[9 + d], Y, Z);
                fold_row(acc + NCC_W + 4 * d, s0[12 + d], s1[12 + d], Y, Z);
            }
        }
    }
    record_slots<NCC_SUMS>(s.part, [&](int i) { return acc[i]; }, cnt, [](int st) { return ncc_in_part(PART, st); });
}

// Workgroup s adds the partial slots 0 .. n-1 of statistic s in a fixed order (finish_reduce) and writes every entry
// of the record {uint64 n; double S_m, S_f, S_mm, S_fm, S_ff, u[12], v[12], w[12], H[12][12]} that holds it.
__global__ __launch_bounds__(256) void k_affine_ncc_finish(const double *part, unsigned n, double *rec)
{
    const int st = blockIdx.x;
    double v;
    if (!finish_head<NCC_SUMS>(part, n, rec, v))
        return;
    double *mom = rec + 1, *u = mom + 5, *vv = u + 12, *w = vv + 12, *H = w + 12;
    if (st >= NCC_MOM)
        mom[st - NCC_MOM] = v;
    else if (st >= NCC_W)
        w[st - NCC_W] = v;
    else if (st >= NCC_U)
        u[st - NCC_U] = v;
    else if (st >= NCC_V)
        vv[st - NCC_V] = v;
    else
        scatter_h(H, st, v);
}

// ---- the fit under an unknown intensity map (Mattes mutual information) ----------------------------------------------
// Header, "Mutual-information affine refinement (Mattes)"; restated in numpy by tests/affine_mi_restatement.py.  Two
// passes over the fixed grid, the histogram with the one-stage front-end (tile_front's, written out in it) and the
// record on the two-stage one (tile_samples); the window of the moving value is sift3d_parzen.h's one function in both
// and on the host.
struct MiArgs {
    AffArgs a;                                   // part: the record pass's partial slots; the histogram pass's counts
    ParzenArgs z;                                // W: the record pass
    unsigned long long *hist;                    // histogram pass: [bins][bins], zeroed by the launcher
    const float *field;                          // histogram pass, FIELD == true: [3][oz][oy][ox]
};

// The Parzen joint histogram in fixed point.  k_similarity without the moments: per counted voxel four integer adds
// q[k] into the workgroup's LDS histogram at [b_f][k0 + k], then the workgroup's non-zero words into the global uint64
// histogram with integer atomics, and its count into partial slot blockIdx.x.  Every add is an integer add, so the bytes
// are a function of the inputs alone, whatever the order.
//   - counters: the LDS words are 64-bit (ds_add_u64, no return value; B * B * 8 bytes, 32 KiB at B = 64: four
//     workgroups fit a CU's 160 KiB, as many as the launch bound allows).  A workgroup visits at most
//     ceil(tiles / grid) * 1024 < 2^32 voxels and a voxel adds at most 43691 < 2^16 to a word, so a word stays below
//     2^48; the global words take at most 2^31 * 1024 voxels: below 2^57;
//   - contention: the four adds of a voxel go to four neighbouring words of one row, and on smooth volumes most lanes
//     of a wave share b_f and k0: the cost of that against k_similarity's single add is measured, not bounded
//     (profiles/microbench/affine_mi_rate_mi355x.txt, 512^3, one run): 0.847 ms on a lattice with a noise floor, 1.58 x
//     k_similarity's 0.537 ms; 1.46 ms (B = 32) and 1.29 ms (B = 64) on a sum of wide Gaussians.  A weight of 0
//     (r == 0: q[3]) is not added.
// The front-end is tile_front's, written out here with the field loaded before F: on tile_front one line of
// ffd_mi_rate.py (parzen_hist_affine, B = 32) came out 0.4 % slower than the parent's spread allows
// (profiles/microbench/registration_front_end_mi355x.txt), so the kernel kept its body.
// (256, 4): 111 - 126 VGPRs, four waves per SIMD, no scratch (-Rpass-analysis=kernel-resource-usage).
// FIELD (header, "Mutual-information free-form deformation (Mattes)"): q = p + u(p) with u read from s.field (three
// more coalesced loads per voxel in the place of pull()'s arithmetic; a lane past the grid reads nothing and takes
// u = 0); everything after q is the same code.  115 - 126 VGPRs, four waves per SIMD, no scratch, but <1, false, true>
// (unmasked, nx == 1), which spills 4 VGPRs there and is bounded to three waves instead (132 VGPRs, no scratch).  Measured
// (profiles/microbench/ffd_mi_rate_mi355x.txt, 512^3, kernel trace, min of 5, one run, the field being the export of
// the same affine map): 1.004 - 1.014 ms on the lattice with a noise floor, 1.16 x the affine kernel's 0.862 -
// 0.874 ms (12 B more read per voxel); 1.50 ms (B = 32) and 1.34 ms (B = 64) on the sum of wide Gaussians, 1.04 -
// 1.05 x: there the contended LDS adds set the time, not the loads.  (Spread of a kernel over its 5 calls: 1 - 3 %.)
template <int LINEAR, bool MASKED, bool FIELD = false>
__global__ __launch_bounds__(256, FIELD && LINEAR == 1 && !MASKED ? 3 : 4) void k_parzen_hist(const MiArgs s)
{
    extern __shared__ __align__(16) unsigned char mi_lds[];
    unsigned long long *h = reinterpret_cast<unsigned long long *>(mi_lds);
    __shared__ unsigned long long cslot[4];
    const GridArgs &p = s.a.g;
    const int B = s.z.bins, BB = B * B;
    for (int i = threadIdx.x; i < BB; i += 256)
        h[i] = 0ull;
    __syncthreads();
    const int lx = threadIdx.x & 15;
    const size_t ovox = (size_t)p.ox * (size_t)p.oy * (size_t)p.oz;             // FIELD only
    unsigned long long cnt = 0;
    for (unsigned base = 0; base < p.ntiles; base += gridDim.x) {
        int xt, y, z;
        if (!tile_at(p, base, xt, y, z))
            break;
        const bool row = y < p.oy && z < p.oz;
        const size_t orow = ((size_t)z * (size_t)p.oy + (size_t)y) * (size_t)p.ox;
        const double yd = (double)y, zd = (double)z;
        const double rx = FIELD ? 0.0 : pull_row(s.a.a, yd, zd), ry = FIELD ? 0.0 : pull_row(s.a.a + 4, yd, zd);
        const double rz = FIELD ? 0.0 : pull_row(s.a.a + 8, yd, zd);
        Taps tp[4];
        float f[4];
        bool live[4];
        float wf[4], wm[4];                                                  // MASKED only
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int x = xt + lx + 16 * k;
            live[k] = row && x < p.ox;
            float ux = 0.0f, uy = 0.0f, uz = 0.0f;                               // FIELD only
            f[k] = 0.0f;
            wf[k] = wm[k] = 1.0f;
            if (live[k]) {
                if (FIELD) {
                    const float *u = s.field + orow + (size_t)x;
                    ux = u[0];
                    uy = u[ovox];
                    uz = u[2 * ovox];
                }
                f[k] = s.a.F[orow + (size_t)x];
                if (MASKED && s.a.w.wf)
                    wf[k] = s.a.w.wf[orow + (size_t)x];
            }
            const double xd = (double)x;
            const double qx = FIELD ? xd + (double)ux : pull(s.a.a, xd, rx);
            const double qy = FIELD ? yd + (double)uy : pull(s.a.a + 4, xd, ry);
            const double qz = FIELD ? zd + (double)uz : pull(s.a.a + 8, xd, rz);
            tp[k] = taps_at<LINEAR>(p.nx, p.ny, p.nz, qx, qy, qz);
            if (MASKED && s.a.w.wm)
                wm[k] = s.a.w.wm[mask_offset(p.nx, p.ny, p.nz, qx, qy, qz)];
        }
        float m[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
            m[k] = gather<LINEAR>(p.src, tp[k], 0.0f);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool counted = MASKED ? live[k] && tp[k].in && mask_in(wf[k]) && mask_in(wm[k]) : live[k] && tp[k].in;
            int k0, out;
            uint32_t q[4];
            double dw[4];
            parzen_window(m[k], s.z.lo_m, s.z.s_m, B, &k0, q, dw, &out);
            unsigned long long *w = h + parzen_fixed_bin(f[k], s.z.lo_f, s.z.s_f, B) * B + k0;      // k0 + 3 <= B - 1
            if (counted) {
                cnt += 1;
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (q[j])
                        atomicAdd(w + j, (unsigned long long)q[j]);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < BB; i += 256) {
        const unsigned long long c = h[i];
        if (c)
            atomicAdd(s.hist + i, c);
    }
    cnt = workgroup_reduce<Add>(cnt, cslot);
    if (threadIdx.x == 0)
        reinterpret_cast<unsigned long long *>(s.a.part)[blockIdx.x] = cnt;
}

// the count's partial slots 0 .. n-1 in finish_reduce's order (integers: any order gives the same)
__global__ __launch_bounds__(256) void k_parzen_hist_finish(const unsigned long long *pcnt, unsigned n,
                                                            unsigned long long *count)
{
    __shared__ unsigned long long s_cnt[256];
    const unsigned long long c = finish_reduce<Add>(pcnt, n, s_cnt);
    if (threadIdx.x == 0)
        count[0] = c;
}

// The MI record: the MSD record's sums (tile_samples, tile_add, fold_pair / fold_row, record_slots) with
// G_d = psi * g_d and E = -1 (S_ee becomes S_pp = sum psi psi), so the partial slots, the finish kernel
// (k_affine_normal_finish) and the record's layout are k_affine_normal's.  W comes into LDS once per workgroup
// (parzen_table; dynamic: B * B * 8 bytes, 32 KiB at B = 64, beside the 2.3 KiB of slots: two workgroups per CU fit, as
// many as the registers allow).  psi of the lane's four outputs (parzen_psi) is formed right after the gathers, before
// the accumulation block, so the window's temporaries are dead when the tile sums are live; m and f are dead after it
// too.
// Registers, as reported by -Rpass-analysis=kernel-resource-usage: 255 - 256 VGPRs, two waves per SIMD and no scratch
// in <2, false>, <1, false> and <2, true>, with a scheduling barrier after each output's psi, so that the four windows'
// temporaries are not live together (without it the kernel spills).  <1, true> (masked, nx == 1: a moving volume one
// voxel wide) still spills there and is bounded to one wave per SIMD instead: 256 VGPRs + 7 AGPRs, no scratch.
// Measured (the same file): 1.15 ms per pass at 512^3 (B = 32; 1.17 ms at B = 64), 1.30 x k_affine_normal's 0.883 ms in
// the same run, on either content.
template <int LINEAR, bool MASKED>
__global__ __launch_bounds__(256, LINEAR == 1 && MASKED ? 1 : 2) void k_affine_mi_normal(const MiArgs sm)
{
    extern __shared__ __align__(16) unsigned char mi_lds[];
    const AffArgs &s = sm.a;
    const GridArgs &p = s.g;
    const double *W = parzen_table(sm.z, reinterpret_cast<double *>(mi_lds));
    const int lx = threadIdx.x & 15;
    unsigned long long cnt = 0;
    double see = 0.0;
    double acc[AFF_H + AFF_B];
#pragma unroll
    for (int i = 0; i < AFF_H + AFF_B; i++)
        acc[i] = 0.0;
    for (unsigned base = 0; base < p.ntiles; base += gridDim.x) {
        int xt, y, z;
        if (!tile_at(p, base, xt, y, z))
            break;
        TileSamples t;
        tile_samples<LINEAR, MASKED>(s, xt, y, z, lx, t);
        // psi (parzen_psi), 0 for a voxel outside the moving range or not counted
        double psi[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            int out;
            const double v = parzen_psi(sm.z, W, t.f[k], t.m[k], &out);
            psi[k] = t.counted[k] && !out ? v : 0.0;
            __builtin_amdgcn_sched_barrier(0);                               // one window's temporaries at a time
        }
        // tile sums: 0 .. 5 the pairs G_d G_e, 6 + d: G_d E
        double s0[9], s1[9], s2[6];
#pragma unroll
        for (int i = 0; i < 9; i++)
            s0[i] = s1[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 6; i++)
            s2[i] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool counted = t.counted[k];
            const double E = counted ? -1.0 : 0.0;
            const double G[3] = {psi[k] * (double)t.gx[k], psi[k] * (double)t.gy[k], psi[k] * (double)t.gz[k]};
            const double X = (double)(xt + lx + 16 * k) - s.cx;
            cnt += counted ? 1u : 0u;
            see += psi[k] * psi[k];
#pragma unroll
            for (int d = 0; d < 3; d++) {
#pragma unroll
                for (int e2 = d; e2 < 3; e2++) {
                    const int i = pair3(d, e2);
                    tile_add(G[d] * G[e2], X, s0[i], s1[i], s2[i]);
                }
                tile_add(G[d] * E, X, s0[6 + d], s1[6 + d]);
            }
        }
        const double Y = (double)y - s.cy, Z = (double)z - s.cz;
        const double YY = Y * Y, YZ = Y * Z, ZZ = Z * Z;
#pragma unroll
        for (int i = 0; i < 6; i++)
            fold_pair(acc + 10 * i, s0[i], s1[i], s2[i], Y, Z, YY, YZ, ZZ);
#pragma unroll
        for (int d = 0; d < 3; d++)
            fold_row(acc + AFF_H + 4 * d, s0[6 + d], s1[6 + d], Y, Z);
    }
    record_slots<AFF_SUMS>(s.part, [&](int i) { return i < AFF_H + AFF_B ? acc[i] : see; }, cnt);
}

} // namespace

// What the launchers below share: the grid of F over M, the map, F's centre, the partial slots and the masks.  false:
// the grid is too large.  A == NULL (the histogram through a field): the map is not read.
static bool aff_args(AffArgs &s, const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                     const double *A, void *d_work, const float *d_WF, const float *d_WM)
{
    if (!grid_args(s.g, d_M, nx, ny, nz, nullptr, ox, oy, oz, 0.0f))
        return false;
    for (int i = 0; i < 12; i++)
        s.a[i] = A ? A[i] : 0.0;
    s.cx = (double)(ox - 1) / 2.0;
    s.cy = (double)(oy - 1) / 2.0;
    s.cz = (double)(oz - 1) / 2.0;
    s.F = d_F;
    s.part = (double *)d_work;
    s.w = MaskArgs{d_WF, d_WM};
    return true;
}

// Launcher for sift3d_affine_refine.c, which has checked every argument (not exported from the library).  d_WF, d_WM:
// the masks or NULL; with both NULL the unmasked kernels run.
extern "C" int sift3d_affine_normal_launch(const char *fn, const float *d_F, int ox, int oy, int oz, const float *d_M,
                                           int nx, int ny, int nz, const double *A, void *d_record, void *d_work,
                                           void *stream, const float *d_WF, const float *d_WM)
{
    AffArgs s;
    if (!aff_args(s, d_F, ox, oy, oz, d_M, nx, ny, nz, A, d_work, d_WF, d_WM))
        return launch_fail(fn, "grid too large");
    const unsigned grid = reduce_grid(s.g.ntiles);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(PICK_LINEAR_MASKED(k_affine_normal, nx, d_WF || d_WM), dim3(grid), dim3(256), 0, st, s);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_affine_normal_finish, dim3(AFF_STATS), dim3(256), 0, st, (const double *)d_work, grid,
                       (double *)d_record);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

// one launch of k_affine_ncc_normal<., ., PART>
template <int PART>
static int ncc_pass(const AffArgs &s, unsigned grid, hipStream_t st)
{
    hipLaunchKernelGGL(PICK_LINEAR_MASKED(k_affine_ncc_normal, s.g.nx, s.w.wf || s.w.wm, PART), dim3(grid), dim3(256), 0,
                       st, s);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

// The same for sift3d_hip_affine_ncc_normal_eqs: d_record is the NCC record, d_work NCC_STATS rows of partial slots.
extern "C" int sift3d_affine_ncc_normal_launch(const char *fn, const float *d_F, int ox, int oy, int oz,
                                               const float *d_M, int nx, int ny, int nz, const double *A,
                                               void *d_record, void *d_work, void *stream, const float *d_WF,
                                               const float *d_WM)
{
    AffArgs s;
    if (!aff_args(s, d_F, ox, oy, oz, d_M, nx, ny, nz, A, d_work, d_WF, d_WM))
        return launch_fail(fn, "grid too large");
    const unsigned grid = reduce_grid(s.g.ntiles);
    hipStream_t st = (hipStream_t)stream;
#ifndef SIFT3D_AFFINE_NCC_ONE_KERNEL
    if (ncc_pass<1>(s, grid, st) || ncc_pass<2>(s, grid, st))
        return SIFT3D_FAILURE;
#else
    if (ncc_pass<0>(s, grid, st))
        return SIFT3D_FAILURE;
#endif
    hipLaunchKernelGGL(k_affine_ncc_finish, dim3(NCC_STATS), dim3(256), 0, st, (const double *)d_work, grid,
                       (double *)d_record);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

// ---- Mattes mutual information: the launchers of sift3d_hip_parzen_hist_affine and sift3d_hip_affine_mi_normal_eqs ----
// d_hist [bins][bins] and d_count are zeroed / written on the stream; d_work: SIFT3D_AMD_SIMILARITY_GRID counts.
// The pull map is A, or with A == NULL the field d_field [3][oz][oy][ox] (sift3d_hip_parzen_hist_field, the MI FFD
// driver).
extern "C" int sift3d_parzen_hist_launch(const char *fn, const float *d_F, int ox, int oy, int oz, const float *d_M,
                                         int nx, int ny, int nz, const double *A, const float *d_field, int bins,
                                         float lo_f, float s_f,
                                         float lo_m, float hi_m, unsigned long long *d_hist,
                                         unsigned long long *d_count, void *d_work, void *stream, const float *d_WF,
                                         const float *d_WM)
{
    MiArgs m;
    if (!aff_args(m.a, d_F, ox, oy, oz, d_M, nx, ny, nz, A, d_work, d_WF, d_WM))
        return launch_fail(fn, "grid too large");
    m.z = parzen_args(bins, lo_f, s_f, lo_m, hi_m, nullptr);
    m.hist = d_hist;
    m.field = d_field;
    const unsigned grid = reduce_grid(m.a.g.ntiles);
    const bool masked = d_WF || d_WM;
    void (*k)(const MiArgs) = A ? PICK_LINEAR_MASKED(k_parzen_hist, nx, masked, false)
                                : PICK_LINEAR_MASKED(k_parzen_hist, nx, masked, true);
    const size_t hb = (size_t)bins * bins * sizeof(unsigned long long);
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(d_hist, 0, hb, st));
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), hb, st, m);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_parzen_hist_finish, dim3(1), dim3(256), 0, st, (const unsigned long long *)d_work, grid,
                       d_count);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

// d_record is the MSD record's layout, d_work k_affine_normal's partial slots, d_W [bins][bins] doubles on the device
extern "C" int sift3d_affine_mi_normal_launch(const char *fn, const float *d_F, int ox, int oy, int oz,
                                              const float *d_M, int nx, int ny, int nz, const double *A, int bins,
                                              float lo_f, float s_f, float lo_m, float hi_m, const double *d_W,
                                              void *d_record, void *d_work, void *stream, const float *d_WF,
                                              const float *d_WM)
{
    MiArgs m;
    if (!aff_args(m.a, d_F, ox, oy, oz, d_M, nx, ny, nz, A, d_work, d_WF, d_WM))
        return launch_fail(fn, "grid too large");
    m.z = parzen_args(bins, lo_f, s_f, lo_m, hi_m, d_W);
    m.hist = nullptr;
    m.field = nullptr;
    const unsigned grid = reduce_grid(m.a.g.ntiles);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(PICK_LINEAR_MASKED(k_affine_mi_normal, nx, d_WF || d_WM), dim3(grid), dim3(256),
                       (size_t)bins * bins * sizeof(double), st, m);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_affine_normal_finish, dim3(AFF_STATS), dim3(256), 0, st, (const double *)d_work, grid,
                       (double *)d_record);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}
