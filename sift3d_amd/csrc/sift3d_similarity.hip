// sift3d_similarity.hip -- similarity of a fixed volume and a moving volume seen through a pull map: the joint
// intensity histogram and the moments behind MSD and NCC in one gather-and-reduce pass over the fixed grid.
// Contract: include/sift3d_amd.h, "Similarity measures"; restated in numpy by tests/similarity_restatement.py
// (histogram and count bit for bit, tests/test_similarity.py).
//
// The pass is k_warp_affine / k_warp_field (sift3d_warp.hip) with the store replaced by a reduction: the tiles (64 x 4
// x 4 outputs per 256-lane workgroup, a lane gathers for 4 x outputs 16 apart), tile order, XCD grouping, pull map,
// inside test and sample of sift3d_resample.h, so m is the warp's value bit for bit; F comes in as the field does
// there (16 lanes of a row read 64 consecutive bytes).  Per voxel 8 B read (+ 12 B of field), nothing written.
//   - grid: min(tiles, SIM_GRID) workgroups walk the tiles (tile_at); the size does not depend on the device, so the
//     bits of the moments depend on the shapes only;
//   - histogram: private to the workgroup in LDS, uint32 [B][B] (dynamic: B * B * 4 bytes, 64 KiB at B = 128 -- two
//     workgroups per CU there, 160 KiB of LDS per CU; at B <= 64 the registers bound the occupancy, not the LDS),
//     committed with ds_add_u32 (no return value).  A workgroup visits at most ceil(tiles / grid) * 1024 < 2^32
//     voxels, so no counter wraps (header);
//   - contention: distinct words cost 4.55 cycles per wave instruction, all 64 lanes on one word 128
//     (profiles/microbench/lds_atomic_mi355x.txt), and a masked volume puts most waves wholly into bin (0, 0): when
//     every counted lane of the wave holds the same bin (one ballot against the first counted lane's), one lane adds
//     the popcount.  Measured at 512^3 (profiles/microbench/similarity_rate_mi355x.txt), masked and spread contents
//     time alike with and without it: the commit hides behind the gathers;
//   - flush: at the end of the walk the workgroup adds its non-zero words to the global uint64 histogram with
//     integer atomics (order-independent: exact).  Per-workgroup partial histograms would need SIM_GRID * B * B * 4 B
//     = 128 MiB of work buffer at B = 128 and a finish pass over all of it; the atomics touch at most grid * B * B
//     words, in practice the populated band of the joint histogram, once per workgroup;
//   - moments: per-lane doubles over the walk, workgroup_reduce<Add> into partial slot blockIdx.x, finish_reduce in a
//     one-workgroup finish kernel (as k_demons_finish).  The reduction slots reuse the histogram's LDS after the flush.
#include "sift3d_resample.h"

#include <cmath>

namespace {

constexpr unsigned SIM_GRID = REDUCE_GRID;
constexpr int SIM_STATS = 7;                     // count, sum f, m, ff, mm, fm, dd
constexpr size_t SIM_SLOT_BYTES = SIM_STATS * 4 * sizeof(double);    // workgroup_reduce: 4 slots per statistic

struct SimArgs {
    double a[12];                                // the affine pull map (FIELD == false)
    GridArgs g;                                  // src = M; ox, oy, oz = F's grid; dst unused
    const float *F;
    const float *field;                          // FIELD == true
    int bins;
    float lo_f, s_f, lo_m, s_m;
    unsigned long long *hist;                    // [bins][bins]
    unsigned long long *pcnt;                    // [SIM_GRID]
    double *psum;                                // [6][SIM_GRID]
    MaskArgs w;                                  // MASKED == true: wf on F's grid, wm on M's; either may be null
};

// b = t < 0 ? 0 : t >= B ? B - 1 : (int) t of the contract (the first test written so that a NaN, which finite
// volumes do not produce, takes bin 0 and converts nothing)
__device__ __forceinline__ int bin_of(float v, float lo, float s, int B)
{
    const float t = (v - lo) * s;
    return !(t >= 0.0f) ? 0 : t >= (float)B ? B - 1 : (int)t;
}

// one wave instruction's worth of commits: lanes with `counted` add 1 to h[idx]
__device__ __forceinline__ void commit(unsigned *h, int idx, bool counted)
{
    const unsigned long long live = __ballot(counted);
    if (!live)
        return;                                                              // wave-uniform
#ifndef SIFT3D_SIMILARITY_NO_UNIFORM
    const int lead = __ffsll((long long)live) - 1;
    const int first = __builtin_amdgcn_readlane(idx, lead);
    if (__ballot(counted && idx != first) == 0) {                            // wave-uniform: every counted lane in one bin
        if ((int)(threadIdx.x & 63) == lead)
            atomicAdd(h + first, (unsigned)__popcll(live));
        return;
    }
#endif
    if (counted)
        atomicAdd(h + idx, 1u);
}

// The front-end written out below is the text of sift3d_resample.h's tile_front (this kernel's was taken for it).  On
// tile_front the kernel compiled to the same registers and occupancy and wrote the same bytes, and one of its twenty
// timing lines came out 0.0002 ms beyond the parent's spread (profiles/microbench/registration_front_end_mi355x.txt),
// so it kept its body: what changes in tile_front changes here too, by hand.
// (256, 4): 116 - 128 VGPRs (LINEAR; 56 - 70 nearest), 4 waves per SIMD, nothing spilled
// (-Rpass-analysis=kernel-resource-usage); left to itself the compiler takes 131 (LINEAR) and fits 3.
// MASKED (header, "Masks"): W_F comes in beside F and W_M by one nearest gather per output, issued with the intensity
// gathers; a voxel whose mask value is below 0.5 is treated as one whose q is outside.
template <int LINEAR, bool FIELD, bool MASKED>
__global__ __launch_bounds__(256, 4) void k_similarity(const SimArgs s)
{
    extern __shared__ __align__(16) unsigned char sim_lds[];
    unsigned *h = reinterpret_cast<unsigned *>(sim_lds);
    const GridArgs &p = s.g;
    const int B = s.bins, BB = B * B;
    for (int i = threadIdx.x; i < BB; i += 256)
        h[i] = 0u;
    __syncthreads();
    const int lx = threadIdx.x & 15;
    const size_t ovox = (size_t)p.ox * (size_t)p.oy * (size_t)p.oz;
    unsigned long long cnt = 0;
    double sf = 0.0, sm = 0.0, sff = 0.0, smm = 0.0, sfm = 0.0, sdd = 0.0;
    for (unsigned base = 0; base < p.ntiles; base += gridDim.x) {
        int xt, y, z;
        if (!tile_at(p, base, xt, y, z))
            break;
        const bool row = y < p.oy && z < p.oz;
        const size_t orow = ((size_t)z * (size_t)p.oy + (size_t)y) * (size_t)p.ox;
        // outputs past the grid read neither F nor the field (f = 0, u = 0), sample inside M and are not counted
        const double yd = (double)y, zd = (double)z;
        double rx = 0.0, ry = 0.0, rz = 0.0;
        if (!FIELD) {
            rx = pull_row(s.a, yd, zd);
            ry = pull_row(s.a + 4, yd, zd);
            rz = pull_row(s.a + 8, yd, zd);
        }
        Taps tp[4];
        float f[4];
        bool live[4];
        float wf[4], wm[4];                                                  // MASKED only
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int x = xt + lx + 16 * k;
            live[k] = row && x < p.ox;
            f[k] = 0.0f;
            wf[k] = wm[k] = 1.0f;
            float ux = 0.0f, uy = 0.0f, uz = 0.0f;
            if (live[k]) {
                f[k] = s.F[orow + (size_t)x];
                if (MASKED && s.w.wf)
                    wf[k] = s.w.wf[orow + (size_t)x];
                if (FIELD) {
                    const float *u = s.field + orow + (size_t)x;
                    ux = u[0];
                    uy = u[ovox];
                    uz = u[2 * ovox];
                }
            }
            const double xd = (double)x;
            const double qx = FIELD ? xd + (double)ux : pull(s.a, xd, rx);
            const double qy = FIELD ? yd + (double)uy : pull(s.a + 4, xd, ry);
            const double qz = FIELD ? zd + (double)uz : pull(s.a + 8, xd, rz);
            tp[k] = taps_at<LINEAR>(p.nx, p.ny, p.nz, qx, qy, qz);
            if (MASKED && s.w.wm)
                wm[k] = s.w.wm[mask_offset(p.nx, p.ny, p.nz, qx, qy, qz)];
        }
        float m[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
            m[k] = gather<LINEAR>(p.src, tp[k], 0.0f);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool counted = MASKED ? live[k] && tp[k].in && mask_in(wf[k]) && mask_in(wm[k]) : live[k] && tp[k].in;
            const int idx = bin_of(f[k], s.lo_f, s.s_f, B) * B + bin_of(m[k], s.lo_m, s.s_m, B);
            commit(h, idx, counted);
            if (counted) {
                const double fd = (double)f[k], md = (double)m[k], dd = (double)(f[k] - m[k]);
                cnt += 1;
                sf += fd;
                sm += md;
                sff += fd * fd;
                smm += md * md;
                sfm += fd * md;
                sdd += dd * dd;
            }
        }
    }
    // flush: this workgroup's non-zero words into the global histogram, consecutive lanes on consecutive words
    __syncthreads();
    for (int i = threadIdx.x; i < BB; i += 256) {
        const unsigned c = h[i];
        if (c)
            atomicAdd(s.hist + i, (unsigned long long)c);
    }
    __syncthreads();                                                         // the histogram's LDS is free
    double *slot = reinterpret_cast<double *>(sim_lds);
    unsigned long long *cslot = reinterpret_cast<unsigned long long *>(sim_lds) + 6 * 4;
    cnt = workgroup_reduce<Add>(cnt, cslot);
    sf = workgroup_reduce<Add>(sf, slot);
    sm = workgroup_reduce<Add>(sm, slot + 4);
    sff = workgroup_reduce<Add>(sff, slot + 8);
    smm = workgroup_reduce<Add>(smm, slot + 12);
    sfm = workgroup_reduce<Add>(sfm, slot + 16);
    sdd = workgroup_reduce<Add>(sdd, slot + 20);
    if (threadIdx.x == 0) {
        s.pcnt[blockIdx.x] = cnt;
        s.psum[blockIdx.x] = sf;
        s.psum[SIM_GRID + blockIdx.x] = sm;
        s.psum[2 * SIM_GRID + blockIdx.x] = sff;
        s.psum[3 * SIM_GRID + blockIdx.x] = smm;
        s.psum[4 * SIM_GRID + blockIdx.x] = sfm;
        s.psum[5 * SIM_GRID + blockIdx.x] = sdd;
    }
}

// the partial slots 0 .. n-1 in a fixed order (finish_reduce) into the stats record {count, six sums}
__global__ __launch_bounds__(256) void k_similarity_finish(const unsigned long long *pcnt, const double *psum,
                                                           unsigned n, unsigned long long *stats)
{
    __shared__ unsigned long long s_cnt[256];
    __shared__ double s_sum[256];
    const unsigned long long c = finish_reduce<Add>(pcnt, n, s_cnt);
    if (threadIdx.x == 0)
        stats[0] = c;
    double *out = reinterpret_cast<double *>(stats + 1);
    for (int k = 0; k < 6; k++) {
        __syncthreads();                                                     // s_sum's last read (s[0]) is done
        const double a = finish_reduce<Add>(psum + (size_t)k * SIM_GRID, n, s_sum);
        if (threadIdx.x == 0)
            out[k] = a;
    }
}

template <bool FIELD, bool MASKED>
int run(const char *fn, SimArgs &s, int interp, void *d_stats, void *stream)
{
    const GridArgs &p = s.g;
    const unsigned grid = reduce_grid(p.ntiles);
    // uint32 counters: passes * 1024 voxels per workgroup (true for every ntiles grid_args accepts; kept as a check)
    const unsigned long long passes = ((unsigned long long)p.ntiles + grid - 1) / grid;
    if (passes * (unsigned long long)(TX * TY * TZ) > 0xffffffffull)
        return launch_fail(fn, "grid too large");
    void (*k)(const SimArgs) = interp == SIFT3D_AMD_INTERP_NEAREST ? k_similarity<0, FIELD, MASKED>
                               : p.nx >= 2                         ? k_similarity<2, FIELD, MASKED>
                                                                   : k_similarity<1, FIELD, MASKED>;
    const size_t hb = (size_t)s.bins * s.bins * sizeof(unsigned);
    const size_t lds = hb > SIM_SLOT_BYTES ? hb : SIM_SLOT_BYTES;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(s.hist, 0, (size_t)s.bins * s.bins * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), lds, st, s);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_similarity_finish, dim3(1), dim3(256), 0, st, s.pcnt, s.psum, grid,
                       (unsigned long long *)d_stats);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

} // namespace

// Launcher for sift3d_similarity.c, which has checked every argument (not exported from the library).  A == NULL:
// through d_field.  s_f, s_m: the bin scales (float) B / (hi - lo).  d_WF, d_WM: the masks or NULL; with both NULL the
// unmasked kernels run.
extern "C" int sift3d_similarity_launch(const char *fn, const float *d_F, int ox, int oy, int oz, const float *d_M,
                                        int nx, int ny, int nz, const double *A, const float *d_field, int interp,
                                        int bins, float lo_f, float s_f, float lo_m, float s_m,
                                        unsigned long long *d_hist, void *d_stats, void *d_work, void *stream,
                                        const float *d_WF, const float *d_WM)
{
    SimArgs s;
    if (!grid_args(s.g, d_M, nx, ny, nz, nullptr, ox, oy, oz, 0.0f))
        return launch_fail(fn, "grid too large");
    for (int i = 0; i < 12; i++)
        s.a[i] = A ? A[i] : 0.0;
    s.F = d_F;
    s.field = d_field;
    s.bins = bins;
    s.lo_f = lo_f; s.s_f = s_f;
    s.lo_m = lo_m; s.s_m = s_m;
    s.hist = d_hist;
    s.pcnt = (unsigned long long *)d_work;
    s.psum = (double *)d_work + SIM_GRID;
    s.w = MaskArgs{d_WF, d_WM};
    if (d_WF || d_WM)
        return A ? run<false, true>(fn, s, interp, d_stats, stream) : run<true, true>(fn, s, interp, d_stats, stream);
    return A ? run<false, false>(fn, s, interp, d_stats, stream) : run<true, false>(fn, s, interp, d_stats, stream);
}
