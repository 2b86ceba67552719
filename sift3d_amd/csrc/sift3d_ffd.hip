// sift3d_ffd.hip -- cubic B-spline free-form deformation: the field of a control lattice, the mean squared difference
// through it with its gradient over the control points, the bending energy with its gradient, the steepest-descent
// update and the lattice subdivision.
// Contract: include/sift3d_amd.h, "B-spline free-form deformation"; restated in numpy by tests/ffd_restatement.py
// (tests/test_ffd.py).  The host checks and the driver are in sift3d_ffd.c.
//
//   - k_ffd_field: 64 x 4 x 4 tiles in sift3d_resample.h's order.  Nothing is gathered from a volume, so a wave is 64
//     CONSECUTIVE x of one row (not the warp's 4 x that are 16 apart) and a lane walks the tile's 4 planes: every
//     plane and channel leaves with one coalesced 256-byte store, no exchange through LDS.  The contract's sum (64
//     terms of 3 multiplies and an add, per channel, unfused) is 768 VALU operations per voxel against 12 B written:
//     the kernel is bound by VALU work and by the 192 lattice loads per voxel (L1 hits), not by HBM.
//   - evaluation: k_ffd_force is k_similarity's walk through a field (the field is read, not the spline; the
//     front-end is written out in it, k_ffd_mi_force calls sift3d_resample.h's tile_front):
//     per counted voxel e = m - f and the gradient (gather_grad), n and S_ee reduced as the affine pass does, and the
//     force E G_d (exact in double) stored, three doubles per voxel.  The adjoint of the spline is SEPARABLE:
//     k_ffd_adjoint sums one axis, sum_x w(x, i) v(x) in ascending x, one lane per output, and is launched for z, then
//     y, then x -- z first because its lanes run along the contiguous y x plane, and every pass shrinks the array by
//     the spacing, so the y and x passes cost next to nothing.  The force is read once from HBM (each value by 4
//     neighbouring control planes, 3 of them from cache); a direct gather per control point would read every voxel 64
//     times.  No atomics anywhere: a lane owns its output and adds in a fixed order, so the bits depend on the
//     shapes only;
//   - bending energy: one lane per control point that has all 26 neighbours computes the six second derivatives of
//     each channel from the 27 values (double), keeps them (k_ffd_bend_value), and k_ffd_bend_grad gathers the exact
//     adjoint per control point from the kept derivatives of its up to 27 neighbours;
//   - reductions: workgroup_reduce into one partial slot per workgroup of a grid that depends on the shapes only, then
//     finish_reduce.
#include "sift3d_resample.h"
#include "sift3d_parzen.h"
#include "sift3d_ffd_eval.h"

namespace {

constexpr unsigned FFD_GRID = REDUCE_GRID;

struct FfdLattice {
    const float *c;                              // [3][gz][gy][gx]
    const float *w;                              // weight tables [dx + dy + dz][4]: x, then y, then z
    int gx, gy, gz, dx, dy, dz;
};

// s = sum_c sum_b sum_a wz[c] * (wy[b] * (wx[a] * c[k0 + c][j0 + b][i0 + a])), float, unfused, x innermost, from +0
__device__ __forceinline__ float ffd_value(const float *c, int gx, int gy, int i0, int j0, int k0, const float4 wx,
                                           const float4 wy, const float4 wz)
{
    const float ax[4] = {wx.x, wx.y, wx.z, wx.w}, ay[4] = {wy.x, wy.y, wy.z, wy.w}, az[4] = {wz.x, wz.y, wz.z, wz.w};
    float s = 0.0f;
#pragma unroll
    for (int cc = 0; cc < 4; cc++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const float *row = c + ((size_t)(k0 + cc) * (size_t)gy + (size_t)(j0 + b)) * (size_t)gx + (size_t)i0;
#pragma unroll
            for (int a = 0; a < 4; a++)
                s = s + az[cc] * (ay[b] * (ax[a] * row[a]));
        }
    return s;
}

struct FfdFieldArgs {
    double a[12];
    FfdLattice l;
    GridArgs g;                                  // dst = the field; src unused
};

// A lane is one (x, y) column of the tile and walks its 4 planes; the channels and planes are NOT unrolled, so that one
// value's 64 lattice loads are in flight at a time and nothing spills (-Rpass-analysis=kernel-resource-usage).  A wave
// is 64 consecutive x of one row: each plane and channel leaves with one coalesced 256-byte store.
template <bool AFFINE>
__global__ __launch_bounds__(256) void k_ffd_field(const FfdFieldArgs s)
{
    const GridArgs &p = s.g;
    const FfdLattice &l = s.l;
    const float4 *w = reinterpret_cast<const float4 *>(l.w);
    const size_t ovox = (size_t)p.ox * (size_t)p.oy * (size_t)p.oz, cvox = (size_t)l.gx * (size_t)l.gy * (size_t)l.gz;
    for (unsigned base = 0; base < p.ntiles; base += gridDim.x) {
        int xt, ty, tz;
        if (!tile_at(p, base, xt, ty, tz))
            return;
        // tile_at's row is the warp's lane layout; this kernel's is x = lane of the wave, y = the wave
        const int x = xt + (int)(threadIdx.x & 63);
        const int y = ty - (int)((threadIdx.x >> 4) & 3) + (int)(threadIdx.x >> 6);
        const int z0 = tz - (int)(threadIdx.x >> 6);
        if (x >= p.ox || y >= p.oy)
            continue;
        const int i0 = x / l.dx, j0 = y / l.dy;
        const float4 wx = w[x - i0 * l.dx], wy = w[l.dx + (y - j0 * l.dy)];
        const double xd = (double)x, yd = (double)y;
        float *out = p.dst + ((size_t)z0 * (size_t)p.oy + (size_t)y) * (size_t)p.ox + (size_t)x;
        const int nk = min(TZ, p.oz - z0);
#pragma unroll 1
        for (int k = 0; k < nk; k++) {
            const int z = z0 + k, k0 = z / l.dz;
            const float4 wz = w[l.dx + l.dy + (z - k0 * l.dz)];
            const double zd = (double)z;
#pragma unroll 1
            for (int d = 0; d < 3; d++) {
                float v = ffd_value(l.c + (size_t)d * cvox, l.gx, l.gy, i0, j0, k0, wx, wy, wz);
                if (AFFINE) {
                    const double pd = d == 0 ? xd : d == 1 ? yd : zd;
                    const double q = pull(s.a + 4 * d, xd, pull_row(s.a + 4 * d, yd, zd));
                    v = (float)(q - pd) + v;
                }
                out[(size_t)d * ovox + (size_t)k * (size_t)p.oy * (size_t)p.ox] = v;
            }
        }
    }
}

struct FfdForceArgs {
    GridArgs g;                                  // src = M; ox, oy, oz = F's grid; dst unused
    const float *F, *field;
    double *force;                               // [3][oz][oy][ox]
    double *part;                                // [2][FFD_GRID]: S_ee, then the count as uint64
    MaskArgs w;                                  // MASKED == true: wf on F's grid, wm on M's; either may be null
};

// MASKED (header, "Masks"): the force at a masked-out voxel is 0 like an outside one's.
// This kernel keeps its own front-end (tile_front's with the field loaded before F): on tile_front it compiled to
// fewer registers (k_ffd_force<2, true>: 132 -> 123 VGPRs, 3 -> 4 waves per SIMD) and ran 3 % slower on the masked
// evaluation of mask_rate.py (profiles/microbench/registration_front_end_mi355x.txt).
// As reported by -Rpass-analysis=kernel-resource-usage: 120 - 132 VGPRs with nx >= 2 (four waves per SIMD unmasked,
// three masked), 129 - 158 and three waves with nx == 1; no scratch.
template <int LINEAR, bool MASKED>
__global__ __launch_bounds__(256) void k_ffd_force(const FfdForceArgs s)
{
    __shared__ double s_see[4];
    __shared__ unsigned long long s_cnt[4];
    const GridArgs &p = s.g;
    const int lx = threadIdx.x & 15;
    const size_t ovox = (size_t)p.ox * (size_t)p.oy * (size_t)p.oz;
    unsigned long long cnt = 0;
    double see = 0.0;
    for (unsigned base = 0; base < p.ntiles; base += gridDim.x) {
        int xt, y, z;
        if (!tile_at(p, base, xt, y, z))
            break;
        const bool row = y < p.oy && z < p.oz;
        const size_t orow = ((size_t)z * (size_t)p.oy + (size_t)y) * (size_t)p.ox;
        Taps tp[4];
        float f[4];
        bool live[4];
        float wf[4], wm[4];                                                  // MASKED only
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int x = xt + lx + 16 * k;
            live[k] = row && x < p.ox;
            float ux = 0.0f, uy = 0.0f, uz = 0.0f;
            f[k] = 0.0f;
            wf[k] = wm[k] = 1.0f;
            if (live[k]) {
                const float *u = s.field + orow + (size_t)x;
                ux = u[0];
                uy = u[ovox];
                uz = u[2 * ovox];
                f[k] = s.F[orow + (size_t)x];
                if (MASKED && s.w.wf)
                    wf[k] = s.w.wf[orow + (size_t)x];
            }
            const double qx = (double)x + (double)ux, qy = (double)y + (double)uy, qz = (double)z + (double)uz;
            tp[k] = taps_at<LINEAR>(p.nx, p.ny, p.nz, qx, qy, qz);
            if (MASKED && s.w.wm)
                wm[k] = s.w.wm[mask_offset(p.nx, p.ny, p.nz, qx, qy, qz)];
        }
        float m[4], gx[4], gy[4], gz[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
            m[k] = gather_grad<LINEAR>(p.src, tp[k], &gx[k], &gy[k], &gz[k]);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool counted = MASKED ? live[k] && tp[k].in && mask_in(wf[k]) && mask_in(wm[k]) : live[k] && tp[k].in;
            const float e = m[k] - f[k];
            const double E = counted ? (double)e : 0.0;
            cnt += counted ? 1u : 0u;
            see += E * E;
            if (live[k]) {
                double *o = s.force + orow + (size_t)(xt + lx + 16 * k);
                o[0] = counted ? E * (double)gx[k] : 0.0;                    // exact: two floats
                o[ovox] = counted ? E * (double)gy[k] : 0.0;
                o[2 * ovox] = counted ? E * (double)gz[k] : 0.0;
            }
        }
    }
    const double vs = workgroup_reduce<Add>(see, s_see);
    const unsigned long long vc = workgroup_reduce<Add>(cnt, s_cnt);
    if (threadIdx.x == 0) {
        s.part[blockIdx.x] = vs;
        reinterpret_cast<unsigned long long *>(s.part)[FFD_GRID + blockIdx.x] = vc;
    }
}

// ---- the force of a channel stack (header, "Multi-channel free-form deformation") ---------------------------------
#ifndef FFD_CHANNELS_UNROLL
#define FFD_CHANNELS_UNROLL 2                    // channels per iteration of the sweep (FFDDEF=-DFFD_CHANNELS_UNROLL=n)
#endif

struct FfdChannelsArgs {
    FfdForceArgs f;                              // F [nc][oz][oy][ox], g.src = M [nc][nz][ny][nx]; one field, one mask pair
    int nc;
};

// One channel of a lane's four outputs: e = m - f (float), E = e widened, S_d = E g_d (FIRST: channel 0) or
// S_d + E g_d, and S_ee += E E in the order k = 0 .. 3.  An output that is not counted has E = 0; what it leaves in S
// is replaced by +0 at the store.  The F reads of outputs past the grid go to the channel's voxel 0: no branch.
template <int LINEAR, bool FIRST>
__device__ __forceinline__ void ffd_channel_terms(const float *Fc, const float *Mc, const Taps (&tp)[4],
                                                  const size_t (&foff)[4], const bool (&counted)[4], double (&S)[4][3],
                                                  double &see)
{
    float f[4], m[4], gx[4], gy[4], gz[4];
#pragma unroll
    for (int k = 0; k < 4; k++)
        f[k] = Fc[foff[k]];
#pragma unroll
    for (int k = 0; k < 4; k++)
        m[k] = gather_grad<LINEAR>(Mc, tp[k], &gx[k], &gy[k], &gz[k]);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float e = m[k] - f[k];
        const double E = counted[k] ? (double)e : 0.0;
        see += E * E;
        const double px = E * (double)gx[k], py = E * (double)gy[k], pz = E * (double)gz[k];   // exact: two floats
        S[k][0] = FIRST ? px : S[k][0] + px;
        S[k][1] = FIRST ? py : S[k][1] + py;
        S[k][2] = FIRST ? pz : S[k][2] + pz;
    }
}

// k_ffd_force over nc channels in one pass: the tile geometry, the partial slots and the front-end (field before F,
// masks, taps) are k_ffd_force's and run once per voxel; then the channels are swept with F advancing by ovox and M by
// mvox (64-bit), the twelve double accumulators of the lane's four outputs staying in registers, and the force is
// stored once after the last channel.  Channel 0 is peeled so that S starts from its product, not from +0 (with nc == 1
// the stores are k_ffd_force's, signed zeros included); the other channels run two to an iteration, so that the eight
// 8-byte gathers of two channels' outputs are in flight together.  S_ee adds E_c E_c in the order (c, k), which with
// nc == 1 is k_ffd_force's order.
// As reported by -Rpass-analysis=kernel-resource-usage: 234 - 236 VGPRs and two waves per SIMD with nx >= 2 (two
// channels' gathers of four outputs beside the twelve accumulators and the taps), 256 VGPRs + 48 - 50 AGPRs and one wave
// with nx == 1; no scratch.
// Measured (profiles/microbench/ffd_channels_rate_mi355x.txt, kernel trace, min of 5, spread of a kernel under 2 %): at
// 512^3 1.44 / 2.37 / 6.21 ms at nc = 1 / 3 / 12 against 1.35 / 4.08 / 16.23 ms for nc launches of k_ffd_force in the same
// run, 1.07 / 0.58 / 0.38 x (256^3: 1.17 / 0.62 / 0.39 x), and 1.95 / 2.35 / 2.80 x the (36 + 8 nc) B per voxel of the
// bytes model at 8 TB/s.  A further channel costs 0.43 ms, 8 B per voxel at 2.5 TB/s: the sweep is bound by the latency
// of its gathers at two waves per SIMD, not by HBM.  One channel per iteration (FFD_CHANNELS_UNROLL=1: 158 - 160 VGPRs,
// three waves) took 1.31 / 2.29 / 6.98 ms in a run where this build took 1.44 / 2.34 / 6.19 and 1.48 / 2.44 / 6.29; three
// per iteration (256 VGPRs + 14 AGPRs, one wave) 2.69 / 3.98 / 8.97 ms.  Two is kept for the twelve channels of the
// descriptors; with one channel k_ffd_force itself is 7 - 17 % faster than this kernel.
template <int LINEAR, bool MASKED>
__global__ __launch_bounds__(256) void k_ffd_force_channels(const FfdChannelsArgs sc)
{
    __shared__ double s_see[4];
    __shared__ unsigned long long s_cnt[4];
    const FfdForceArgs &s = sc.f;
    const GridArgs &p = s.g;
    const int lx = threadIdx.x & 15;
    const size_t ovox = (size_t)p.ox * (size_t)p.oy * (size_t)p.oz;
    const size_t mvox = (size_t)p.nx * (size_t)p.ny * (size_t)p.nz;
    unsigned long long cnt = 0;
    double see = 0.0;
    for (unsigned base = 0; base < p.ntiles; base += gridDim.x) {
        int xt, y, z;
        if (!tile_at(p, base, xt, y, z))
            break;
        const bool row = y < p.oy && z < p.oz;
        const size_t orow = ((size_t)z * (size_t)p.oy + (size_t)y) * (size_t)p.ox;
        Taps tp[4];
        size_t foff[4];
        bool live[4], counted[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int x = xt + lx + 16 * k;
            live[k] = row && x < p.ox;
            foff[k] = live[k] ? orow + (size_t)x : 0;
            float ux = 0.0f, uy = 0.0f, uz = 0.0f;
            float wf = 1.0f, wm = 1.0f;                                      // MASKED only
            if (live[k]) {
                const float *u = s.field + orow + (size_t)x;
                ux = u[0];
                uy = u[ovox];
                uz = u[2 * ovox];
                if (MASKED && s.w.wf)
                    wf = s.w.wf[orow + (size_t)x];
            }
            const double qx = (double)x + (double)ux, qy = (double)y + (double)uy, qz = (double)z + (double)uz;
            tp[k] = taps_at<LINEAR>(p.nx, p.ny, p.nz, qx, qy, qz);
            if (MASKED && s.w.wm)
                wm = s.w.wm[mask_offset(p.nx, p.ny, p.nz, qx, qy, qz)];
            counted[k] = MASKED ? live[k] && tp[k].in && mask_in(wf) && mask_in(wm) : live[k] && tp[k].in;
            cnt += counted[k] ? 1u : 0u;
        }
        double S[4][3];
        const float *Fc = s.F, *Mc = p.src;
        ffd_channel_terms<LINEAR, true>(Fc, Mc, tp, foff, counted, S, see);
#pragma unroll FFD_CHANNELS_UNROLL
        for (int c = 1; c < sc.nc; c++) {
            Fc += ovox;
            Mc += mvox;
            ffd_channel_terms<LINEAR, false>(Fc, Mc, tp, foff, counted, S, see);
        }
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (live[k]) {
                double *o = s.force + orow + (size_t)(xt + lx + 16 * k);
                o[0] = counted[k] ? S[k][0] : 0.0;
                o[ovox] = counted[k] ? S[k][1] : 0.0;
                o[2 * ovox] = counted[k] ? S[k][2] : 0.0;
            }
    }
    const double vs = workgroup_reduce<Add>(see, s_see);
    const unsigned long long vc = workgroup_reduce<Add>(cnt, s_cnt);
    if (threadIdx.x == 0) {
        s.part[blockIdx.x] = vs;
        reinterpret_cast<unsigned long long *>(s.part)[FFD_GRID + blockIdx.x] = vc;
    }
}

// ---- the force of the mutual information (header, "Mutual-information free-form deformation (Mattes)") ------------
struct FfdMiForceArgs {
    FfdForceArgs f;                              // part: S_pp, then the count
    ParzenArgs z;
};

// k_ffd_force's sums and stores on tile_front, with the force E G'_d = -(psi * g_d) in the place of E G_d, psi being
// sift3d_parzen.h's parzen_psi (W from LDS), and S_pp = sum psi psi in the slot of S_ee.  W comes into dynamic LDS once
// per workgroup: B * B * 8 bytes, 32 KiB at B = 64, so five workgroups fit a CU's 160 KiB.  A voxel that is not
// counted, and a counted one outside the moving range (psi = 0), store +0.
// (256, 4): 124 - 128 VGPRs, no AGPRs, four waves per SIMD and no scratch in all four instantiations
// (-Rpass-analysis=kernel-resource-usage): there are no 72 accumulators here, so the window's temporaries and the four
// outputs' taps fit where k_affine_mi_normal needs two waves and scheduling barriers.
// Measured (profiles/microbench/ffd_mi_rate_mi355x.txt, 512^3, kernel trace, min of 5, one run): 1.29 - 1.35 ms at
// B = 32 and 64 on either content, 0.996 - 1.001 x k_ffd_force's 1.30 - 1.35 ms in the same run (spread of a kernel
// 1 %; an earlier run of the same script gave 1.42 - 1.44 ms for both kernels, the same quotients); both are 1.75 -
// 1.83 x the 0.74 ms that their 44 B per voxel take at 8 TB/s: the window and the four LDS reads hide behind the
// stores of three doubles per voxel.
template <int LINEAR, bool MASKED>
__global__ __launch_bounds__(256, 4) void k_ffd_mi_force(const FfdMiForceArgs sm)
{
    extern __shared__ __align__(16) unsigned char ffd_lds[];
    __shared__ double s_spp[4];
    __shared__ unsigned long long s_cnt[4];
    const FfdForceArgs &s = sm.f;
    const GridArgs &p = s.g;
    const double *W = parzen_table(sm.z, reinterpret_cast<double *>(ffd_lds));
    const int lx = threadIdx.x & 15;
    const size_t ovox = (size_t)p.ox * (size_t)p.oy * (size_t)p.oz;
    unsigned long long cnt = 0;
    double spp = 0.0;
    for (unsigned base = 0; base < p.ntiles; base += gridDim.x) {
        int xt, y, z;
        if (!tile_at(p, base, xt, y, z))
            break;
        TileFront t;
        tile_front<LINEAR, true, MASKED>(p, nullptr, s.field, s.F, s.w, xt, y, z, t);
        float m[4], gx[4], gy[4], gz[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
            m[k] = gather_grad<LINEAR>(p.src, t.tp[k], &gx[k], &gy[k], &gz[k]);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool counted = tile_counted<MASKED>(t, k);
            int out;
            const double v = parzen_psi(sm.z, W, t.f[k], m[k], &out);
            const bool on = counted && !out;
            const double psi = on ? v : 0.0;
            cnt += counted ? 1u : 0u;
            spp += psi * psi;
            if (t.live[k]) {
                double *o = s.force + t.orow + (size_t)(xt + lx + 16 * k);
                o[0] = on ? -(psi * (double)gx[k]) : 0.0;                    // one rounding; the sign is exact
                o[ovox] = on ? -(psi * (double)gy[k]) : 0.0;
                o[2 * ovox] = on ? -(psi * (double)gz[k]) : 0.0;
            }
        }
    }
    const double vs = workgroup_reduce<Add>(spp, s_spp);
    const unsigned long long vc = workgroup_reduce<Add>(cnt, s_cnt);
    if (threadIdx.x == 0) {
        s.part[blockIdx.x] = vs;
        reinterpret_cast<unsigned long long *>(s.part)[FFD_GRID + blockIdx.x] = vc;
    }
}

// one workgroup: dst[0] = the slots of a statistic in finish_reduce's order, times scale (1.0 is exact)
template <typename Op>
__global__ __launch_bounds__(256) void k_ffd_finish(const double *part, unsigned n, double *dst, double scale)
{
    __shared__ double s_sum[256];
    const double v = finish_reduce<Op>(part, n, s_sum);
    if (threadIdx.x == 0)
        dst[0] = v * scale;
}

__global__ __launch_bounds__(256) void k_ffd_finish_count(const unsigned long long *part, unsigned n,
                                                          unsigned long long *dst)
{
    __shared__ unsigned long long s_cnt[256];
    const unsigned long long v = finish_reduce<Add>(part, n, s_cnt);
    if (threadIdx.x == 0)
        dst[0] = v;
}

// One axis of the adjoint: src [outer][n][inner] -> dst [outer][g][inner],
//   dst[o][i][q] = sum over x = max(0, (i - 3) delta) .. min(n - 1, (i + 1) delta - 1), ascending, of
//                  (double) w[x % delta][i - x / delta] * src[o][x][q]                (from +0; double, unfused)
struct FfdAdjArgs {
    const double *src;
    double *dst;
    const float *w;                              // this axis' table [delta][4]
    size_t inner, total;                         // total = outer * g * inner
    int n, g, delta;
};

__global__ __launch_bounds__(256) void k_ffd_adjoint(const FfdAdjArgs s)
{
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < s.total; idx += (size_t)gridDim.x * 256) {
        const size_t t = idx / s.inner, q = idx - t * s.inner;
        const size_t o = t / (size_t)s.g;
        const int i = (int)(t - o * (size_t)s.g);
        const int lo = max(0, (i - 3) * s.delta), hi = min(s.n - 1, (i + 1) * s.delta - 1);
        int cell = lo / s.delta, r = lo - cell * s.delta;
        const double *v = s.src + (o * (size_t)s.n + (size_t)lo) * s.inner + q;
        double sum = 0.0;
        for (int x = lo; x <= hi; x++) {
            sum += (double)s.w[4 * r + (i - cell)] * *v;
            v += s.inner;
            if (++r == s.delta) {
                r = 0;
                cell++;
            }
        }
        s.dst[idx] = sum;
    }
}

// ---- bending energy ----------------------------------------------------------------------------------------------
// st[axis][order][tap]: the value (1/6, 4/6, 1/6), first ((-1/2, 0, 1/2) / delta) and second ((1, -2, 1) / delta^2)
// derivative stencils of each axis, made on the host.  Derivative t = xx, yy, zz, xy, xz, yz has the orders
// bend_order(t, axis) along x, y, z and the weight 1 (t < 3) or 2 in the energy; it is evaluated axis by axis,
// sum_c sz[c] * (sum_b sy[b] * (sum_a sx[a] * v[c][b][a])), every sum ascending from +0, and its coefficient at the
// neighbour (a, b, c) in the adjoint is (sz[c] * sy[b]) * sx[a].
struct FfdBendArgs {
    double st[3][3][3];
    const float *c;
    double *D;                                   // [3][6][N], N = (gx - 2)(gy - 2)(gz - 2)
    double *part;                                // [FFD_GRID] (value); unused (grad)
    double *dR;                                  // [3][gz][gy][gx] (grad)
    int gx, gy, gz;
};

__device__ __forceinline__ int bend_order(int t, int axis)
{
    // xx, yy, zz, xy, xz, yz
    return t < 3 ? (t == axis ? 2 : 0) : (t == 3 ? (axis < 2) : t == 4 ? (axis != 1) : (axis > 0));
}

__device__ __forceinline__ double bend_coef(const FfdBendArgs &s, int t, int a, int b, int c)
{
    return (s.st[2][bend_order(t, 2)][c] * s.st[1][bend_order(t, 1)][b]) * s.st[0][bend_order(t, 0)][a];
}

__global__ __launch_bounds__(256) void k_ffd_bend_value(const FfdBendArgs s)
{
    __shared__ double slot[4];
    const int mx = s.gx - 2, my = s.gy - 2, mz = s.gz - 2;
    const size_t N = (size_t)mx * my * mz, cvox = (size_t)s.gx * s.gy * s.gz;
    double acc = 0.0;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < N; p += (size_t)gridDim.x * 256) {
        const int i = (int)(p % (size_t)mx) + 1, j = (int)(p / (size_t)mx % (size_t)my) + 1;
        const int k = (int)(p / ((size_t)mx * my)) + 1;
        for (int ch = 0; ch < 3; ch++) {
            double v[3][3][3];
#pragma unroll
            for (int c = 0; c < 3; c++)
#pragma unroll
                for (int b = 0; b < 3; b++)
#pragma unroll
                    for (int a = 0; a < 3; a++)
                        v[c][b][a] = (double)s.c[(size_t)ch * cvox +
                                                 ((size_t)(k + c - 1) * s.gy + (size_t)(j + b - 1)) * s.gx +
                                                 (size_t)(i + a - 1)];
#pragma unroll
            for (int t = 0; t < 6; t++) {
                const double *sx = s.st[0][bend_order(t, 0)], *sy = s.st[1][bend_order(t, 1)];
                const double *sz = s.st[2][bend_order(t, 2)];
                double d = 0.0;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    double ry = 0.0;
#pragma unroll
                    for (int b = 0; b < 3; b++) {
                        double rx = 0.0;
#pragma unroll
                        for (int a = 0; a < 3; a++)
                            rx += sx[a] * v[c][b][a];
                        ry += sy[b] * rx;
                    }
                    d += sz[c] * ry;
                }
                s.D[((size_t)ch * 6 + t) * N + p] = d;
                acc += (t < 3 ? 1.0 : 2.0) * (d * d);
            }
        }
    }
    const double r = workgroup_reduce<Add>(acc, slot);
    if (threadIdx.x == 0)
        s.part[blockIdx.x] = r;
}

// dR[ch][q] = (2 / N) * sum over the neighbours p = q - (a, b, c) - that have all 26 neighbours themselves - in
// ascending (c, b, a), and t = 0 .. 5, of m_t * (coef_t(a, b, c) * D_t[ch][p])
__global__ __launch_bounds__(256) void k_ffd_bend_grad(const FfdBendArgs s)
{
    const int mx = s.gx - 2, my = s.gy - 2, mz = s.gz - 2;
    const size_t N = (size_t)mx * my * mz, cvox = (size_t)s.gx * s.gy * s.gz;
    const double scale = 2.0 / (double)N;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < 3 * cvox; idx += (size_t)gridDim.x * 256) {
        const size_t ch = idx / cvox, q = idx - ch * cvox;
        const int i = (int)(q % (size_t)s.gx), j = (int)(q / (size_t)s.gx % (size_t)s.gy);
        const int k = (int)(q / ((size_t)s.gx * s.gy));
        double sum = 0.0;
        for (int c = 0; c < 3; c++)
            for (int b = 0; b < 3; b++)
                for (int a = 0; a < 3; a++) {
                    // q is neighbour (a, b, c) of p = q - (a - 1, b - 1, c - 1)
                    const int pi = i - (a - 1), pj = j - (b - 1), pk = k - (c - 1);
                    if (pi < 1 || pi > mx || pj < 1 || pj > my || pk < 1 || pk > mz)
                        continue;
                    const size_t p = ((size_t)(pk - 1) * my + (size_t)(pj - 1)) * mx + (size_t)(pi - 1);
                    for (int t = 0; t < 6; t++)
                        sum += (t < 3 ? 1.0 : 2.0) * (bend_coef(s, t, a, b, c) * s.D[(ch * 6 + t) * N + p]);
                }
        s.dR[idx] = scale * sum;
    }
}

// grad = (float)(b) and the largest |grad| (as stored) into one partial slot per workgroup, with
//   b = (scale / n) * Gc + bending * dR; scale: 2.0 for the MSD (Gc / n is half its derivative), 1.0 for the MI;
//   JAC (header, "Jacobian penalty"): b = b + jn * GJ, jn = jacobian / N made on the host;
//   LM (header, "FFD landmarks"): b = b + (lk / Omega) * GL, lk = lambda * (2 * 4^l) made on the host and Omega read
//   from the landmark record; Omega == 0 adds no term.
// The terms are added in this order, each product rounded before its sum.
struct FfdCombineArgs {
    const double *rec;                           // rec[0] = n as uint64
    const double *Gc, *dR;
    float *grad;
    double *part;
    double bending, scale;
    size_t total;
    const double *GJ;                            // JAC only
    double jn;
    const double *GL, *lrec;                     // LM only
    double lk;
};

template <bool JAC, bool LM>
__global__ __launch_bounds__(256) void k_ffd_combine(const FfdCombineArgs s)
{
    __shared__ double slot[4];
    const double n = (double)reinterpret_cast<const unsigned long long *>(s.rec)[0];
    const double two_n = s.scale / n;
    const double omega = LM ? s.lrec[2] : 0.0, f = s.lk / omega;             // LM only
    double mx = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < s.total; i += (size_t)gridDim.x * 256) {
        double b = two_n * s.Gc[i] + s.bending * s.dR[i];
        if (JAC)
            b = b + s.jn * s.GJ[i];
        const float g = (float)(!LM || omega == 0.0 ? b : b + f * s.GL[i]);
        s.grad[i] = g;
        mx = fmax(mx, (double)fabsf(g));
    }
    const double r = workgroup_reduce<Max>(mx, slot);
    if (threadIdx.x == 0)
        s.part[blockIdx.x] = r;
}

__global__ __launch_bounds__(256) void k_ffd_step(const float *c, const float *grad, float a, float *out, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        out[i] = c[i] - a * grad[i];
}

// ---- subdivision: the lattice over (o + 1) / 2 voxels -> the lattice over o voxels, same spacing, times 2 ------------
// Per axis, fine j odd (= 2 i - 1): ((c[i - 1] + 6 c[i]) + c[i + 1]) * 0.125; j even (= 2 i): (c[i] + c[i + 1]) * 0.5;
// x first, then y, then z, then * 2, all float.  The largest coarse index needed is floor(floor((o - 1) / delta) / 2)
// + 3 = g_coarse - 1 (o_coarse - 1 = floor((o - 1) / 2)), so every read is inside the coarse lattice.
struct FfdRefineArgs {
    const float *c;
    float *f;
    int cx, cy, cz, fx, fy, fz;
};

__device__ __forceinline__ int sub_taps(int j, int &first)
{
    first = (j & 1) ? (j + 1) / 2 - 1 : j / 2;
    return (j & 1) ? 3 : 2;
}

__device__ __forceinline__ float sub_mix(const float v[3], int n)
{
    return n == 3 ? ((v[0] + 6.0f * v[1]) + v[2]) * 0.125f : (v[0] + v[1]) * 0.5f;
}

__global__ __launch_bounds__(256) void k_ffd_refine2(const FfdRefineArgs s)
{
    const size_t fvox = (size_t)s.fx * s.fy * s.fz, cvox = (size_t)s.cx * s.cy * s.cz;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < 3 * fvox; idx += (size_t)gridDim.x * 256) {
        const size_t ch = idx / fvox, q = idx - ch * fvox;
        const int i = (int)(q % (size_t)s.fx), j = (int)(q / (size_t)s.fx % (size_t)s.fy);
        const int k = (int)(q / ((size_t)s.fx * s.fy));
        int ai, aj, ak;
        const int ni = sub_taps(i, ai), nj = sub_taps(j, aj), nk = sub_taps(k, ak);
        const float *c = s.c + ch * cvox;
        float vz[3] = {0.0f, 0.0f, 0.0f};
        for (int cc = 0; cc < nk; cc++) {
            float vy[3] = {0.0f, 0.0f, 0.0f};
            for (int b = 0; b < nj; b++) {
                float vx[3] = {0.0f, 0.0f, 0.0f};
                const int zz = min(ak + cc, s.cz - 1), yy = min(aj + b, s.cy - 1);      // never binding (see above)
                for (int a = 0; a < ni; a++)
                    vx[a] = c[((size_t)zz * s.cy + (size_t)yy) * s.cx + (size_t)min(ai + a, s.cx - 1)];
                vy[b] = sub_mix(vx, ni);
            }
            vz[cc] = sub_mix(vy, nj);
        }
        s.f[idx] = sub_mix(vz, nk) * 2.0f;
    }
}

unsigned flat_grid(size_t total, unsigned cap)
{
    const size_t b = (total + 255) / 256;
    return (unsigned)(b < 1 ? 1 : b < cap ? b : cap);
}

} // namespace

// Launchers for sift3d_ffd.c, which has checked every argument (not exported from the library).
extern "C" int sift3d_ffd_field_launch(const char *fn, const float *d_lat, int gx, int gy, int gz, int dx, int dy,
                                       int dz, const float *d_w, const double *A, int ox, int oy, int oz,
                                       float *d_field, void *stream)
{
    FfdFieldArgs s;
    if (!grid_args(s.g, nullptr, 1, 1, 1, d_field, ox, oy, oz, 0.0f))
        return launch_fail(fn, "grid too large");
    s.l = FfdLattice{d_lat, d_w, gx, gy, gz, dx, dy, dz};
    for (int i = 0; i < 12; i++)
        s.a[i] = A ? A[i] : 0.0;
    const unsigned grid = s.g.ntiles < MAX_GRID ? s.g.ntiles : MAX_GRID;
    void (*k)(const FfdFieldArgs) = A ? k_ffd_field<true> : k_ffd_field<false>;
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, (hipStream_t)stream, s);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

// the adjoint of the spline on src [3][oz][oy][ox] -> dst [3][gz][gy][gx]: z, y, x
static int ffd_adjoint_passes(const double *src, double *t1, double *t2, double *dst, const float *d_w, int ox, int oy,
                              int oz, int gx, int gy, int gz, int dx, int dy, int dz, hipStream_t st)
{
    const FfdAdjArgs az = {src, t1, d_w + 4 * (size_t)(dx + dy), (size_t)oy * ox, 3 * (size_t)gz * oy * ox, oz, gz, dz};
    const FfdAdjArgs ay = {t1, t2, d_w + 4 * (size_t)dx, (size_t)ox, 3 * (size_t)gz * gy * ox, oy, gy, dy};
    const FfdAdjArgs ax = {t2, dst, d_w, 1, 3 * (size_t)gx * gy * gz, ox, gx, dx};
    const FfdAdjArgs *pass[3] = {&az, &ay, &ax};
    for (int i = 0; i < 3; i++) {
        hipLaunchKernelGGL(k_ffd_adjoint, dim3(flat_grid(pass[i]->total, MAX_GRID)), dim3(256), 0, st, *pass[i]);
        LAUNCH_CHECK();
    }
    return SIFT3D_SUCCESS;
}

// The parts `parts` (sift3d_ffd_eval.h) of the evaluation e.  e->d_work: partial slots [2][FFD_GRID] doubles, then the
// force [3][oz][oy][ox], t1 [3][gz][oy][ox], t2 [3][gz][gy][ox], D [18][N] doubles.  FFD_BEND_GRAD reads the D that the
// last FFD_BEND_VALUE on this d_work left, FFD_COMBINE the n that the last FFD_IMAGE left in d_rec.
extern "C" int sift3d_ffd_evaluate_launch(const char *fn, unsigned parts, const sift3d_ffd_eval *e)
{
    hipStream_t st = (hipStream_t)e->stream;
    const sift3d_ffd_jac *jac = e->jac;
    const sift3d_ffd_lm *lm = e->lm;
    const int ox = e->ox, oy = e->oy, oz = e->oz, gx = e->gx, gy = e->gy, gz = e->gz;
    const size_t vox = (size_t)ox * oy * oz, cvox = (size_t)gx * gy * gz;
    const size_t N = (size_t)(gx - 2) * (gy - 2) * (gz - 2);
    double *part = e->d_work, *force = part + 2 * FFD_GRID, *t1 = force + 3 * vox;
    double *t2 = t1 + 3 * (size_t)gz * oy * ox, *D = t2 + 3 * (size_t)gz * gy * ox;
    double *d_rec = e->d_rec, *Gc = d_rec + 4, *dR = Gc + 3 * cvox;
    if (parts & FFD_IMAGE) {
        FfdMiForceArgs fm;
        FfdForceArgs &f = fm.f;
        if (!grid_args(f.g, e->d_M, e->nx, e->ny, e->nz, nullptr, ox, oy, oz, 0.0f))
            return launch_fail(fn, "grid too large");
        f.F = e->d_F;
        f.field = e->d_field;
        f.force = force;
        f.part = part;
        const unsigned grid = reduce_grid(f.g.ntiles);
        f.w = MaskArgs{e->d_WF, e->d_WM};
        const bool masked = e->d_WF || e->d_WM;
        if (e->mi) {
            const sift3d_ffd_mi &m = *e->mi;
            fm.z = parzen_args(m.bins, m.lo_f, m.s_f, m.lo_m, m.hi_m, m.d_W);
            hipLaunchKernelGGL(PICK_LINEAR_MASKED(k_ffd_mi_force, e->nx, masked), dim3(grid), dim3(256),
                               (size_t)m.bins * m.bins * sizeof(double), st, fm);
        } else if (e->nc >= 1) {
            FfdChannelsArgs fc;
            fc.f = f;
            fc.nc = e->nc;
            hipLaunchKernelGGL(PICK_LINEAR_MASKED(k_ffd_force_channels, e->nx, masked), dim3(grid), dim3(256), 0, st, fc);
        } else {
            hipLaunchKernelGGL(PICK_LINEAR_MASKED(k_ffd_force, e->nx, masked), dim3(grid), dim3(256), 0, st, f);
        }
        LAUNCH_CHECK();
        hipLaunchKernelGGL(k_ffd_finish_count, dim3(1), dim3(256), 0, st, (const unsigned long long *)part + FFD_GRID, grid,
                           (unsigned long long *)d_rec);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(k_ffd_finish<Add>, dim3(1), dim3(256), 0, st, (const double *)part, grid, d_rec + 1, 1.0);
        LAUNCH_CHECK();
        if (ffd_adjoint_passes(force, t1, t2, Gc, e->d_w, ox, oy, oz, gx, gy, gz, e->dx, e->dy, e->dz, st))
            return SIFT3D_FAILURE;
    }
    if (jac && (parts & (FFD_JAC_VALUE | FFD_JAC_GRAD))) {
        const bool with_grad = parts & FFD_JAC_GRAD;
        if (sift3d_jacobian_penalty_launch(fn, e->d_field, ox, oy, oz, jac->ref, jac->d_rec, with_grad ? force : nullptr,
                                           jac->d_work, e->stream) ||
            (with_grad &&
             ffd_adjoint_passes(force, t1, t2, jac->d_GJ, e->d_w, ox, oy, oz, gx, gy, gz, e->dx, e->dy, e->dz, st)))
            return SIFT3D_FAILURE;
    }
    if (lm && (parts & (FFD_LM_VALUE | FFD_LM_GRAD)) &&
        sift3d_ffd_landmarks_launch(fn, e->d_lat, gx, gy, gz, e->dx, e->dy, e->dz, lm, (parts & FFD_LM_GRAD) != 0, nullptr,
                                    e->stream))
        return SIFT3D_FAILURE;
    // the bending energy and its gradient
    FfdBendArgs b;
    for (int i = 0; i < 27; i++)
        (&b.st[0][0][0])[i] = e->stencils[i];
    b.c = e->d_lat;
    b.D = D;
    b.part = part;
    b.dR = dR;
    b.gx = gx; b.gy = gy; b.gz = gz;
    if (parts & FFD_BEND_VALUE) {
        const unsigned bgrid = flat_grid(N, FFD_GRID);
        hipLaunchKernelGGL(k_ffd_bend_value, dim3(bgrid), dim3(256), 0, st, b);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(k_ffd_finish<Add>, dim3(1), dim3(256), 0, st, (const double *)part, bgrid, d_rec + 2,
                           1.0 / (double)N);
        LAUNCH_CHECK();
    }
    if (parts & FFD_BEND_GRAD) {
        hipLaunchKernelGGL(k_ffd_bend_grad, dim3(flat_grid(3 * cvox, MAX_GRID)), dim3(256), 0, st, b);
        LAUNCH_CHECK();
    }
    if (parts & FFD_COMBINE) {
        const bool with_jac = jac && jac->weight > 0.0, with_lm = lm && lm->weight > 0.0;
        const FfdCombineArgs c = {d_rec, Gc, dR, e->d_grad, part, e->bending, e->mi ? 1.0 : 2.0, 3 * cvox,
                                  with_jac ? jac->d_GJ : nullptr, with_jac ? jac->weight / (double)vox : 0.0,
                                  with_lm ? lm->d_GL : nullptr, with_lm ? lm->d_rec : nullptr,
                                  with_lm ? lm->weight * lm->scale : 0.0};
        const unsigned cgrid = flat_grid(3 * cvox, FFD_GRID);
        void (*k)(const FfdCombineArgs) = with_lm ? (with_jac ? k_ffd_combine<true, true> : k_ffd_combine<false, true>)
                                                  : (with_jac ? k_ffd_combine<true, false> : k_ffd_combine<false, false>);
        hipLaunchKernelGGL(k, dim3(cgrid), dim3(256), 0, st, c);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(k_ffd_finish<Max>, dim3(1), dim3(256), 0, st, (const double *)part, cgrid, d_rec + 3, 1.0);
        LAUNCH_CHECK();
    }
    return SIFT3D_SUCCESS;
}

// The penalty of a field and its gradient over the lattice of that grid: the record, S and its adjoint GJ.  d_work: S
// [3][oz][oy][ox], t1 [3][gz][oy][ox], t2 [3][gz][gy][ox] doubles, then the penalty's work.
extern "C" int sift3d_ffd_jacobian_gradient_launch(const char *fn, const float *d_field, int ox, int oy, int oz, int gx,
                                                   int gy, int gz, int dx, int dy, int dz, const float *d_w, double ref,
                                                   double *d_rec, double *d_GJ, double *d_work, void *stream)
{
    const size_t vox = (size_t)ox * oy * oz;
    double *S = d_work, *t1 = S + 3 * vox, *t2 = t1 + 3 * (size_t)gz * oy * ox, *jwork = t2 + 3 * (size_t)gz * gy * ox;
    if (sift3d_jacobian_penalty_launch(fn, d_field, ox, oy, oz, ref, d_rec, S, jwork, stream))
        return SIFT3D_FAILURE;
    return ffd_adjoint_passes(S, t1, t2, d_GJ, d_w, ox, oy, oz, gx, gy, gz, dx, dy, dz, (hipStream_t)stream);
}

extern "C" int sift3d_ffd_step_launch(const float *d_c, const float *d_grad, float a, float *d_out, size_t n,
                                      void *stream)
{
    hipLaunchKernelGGL(k_ffd_step, dim3(flat_grid(n, MAX_GRID)), dim3(256), 0, (hipStream_t)stream, d_c, d_grad, a,
                       d_out, n);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

extern "C" int sift3d_ffd_refine2_launch(const float *d_c, int cx, int cy, int cz, float *d_f, int fx, int fy, int fz,
                                         void *stream)
{
    const FfdRefineArgs s = {d_c, d_f, cx, cy, cz, fx, fy, fz};
    hipLaunchKernelGGL(k_ffd_refine2, dim3(flat_grid(3 * (size_t)fx * fy * fz, MAX_GRID)), dim3(256), 0,
                       (hipStream_t)stream, s);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}
