// sift3d_init.hip -- the device passes behind an initial transform: the moments of a volume (count, mass, first and
// second moments about the grid's centre) and the similarity of a fixed and a moving volume through K candidate affine
// pull maps in one call.  Contract: include/sift3d_amd.h, "Initial transforms: moments and candidate search"; restated
// in numpy by tests/affine_init_restatement.py.  The checked entries are in sift3d_init.c.
//
// Both passes walk their grid as the sum kernels of this library do: 64 x 4 x 4 tiles per 256-lane workgroup, a lane
// holds 4 x outputs 16 apart (the 16 lanes of a row read 64 consecutive bytes), min(tiles, SIFT3D_AMD_SIMILARITY_GRID)
// workgroups walk the tiles (tile_at, reduce_grid), sums per lane in double, workgroup_reduce<Add> into the
// workgroup's partial slot, finish_reduce over the slots by one workgroup.  The bytes depend on the shapes only.
#include "sift3d_resample.h"

#include <cmath>

namespace {

// ---- moments ---------------------------------------------------------------------------------------------------------
constexpr int MOM_SUMS = 10;                     // S0, S1[3], S2[6]

struct MomArgs {
    GridArgs g;                                  // ox, oy, oz = V's grid; src, dst, nx, ny, nz unused
    const float *V;
    const float *W;                              // MASKED == true
    float floor;
    int binary;
    double cx, cy, cz;                           // (n - 1) / 2, exact
    unsigned long long *pcnt;                    // [REDUCE_GRID]
    double *psum;                                // [MOM_SUMS][REDUCE_GRID]
};

// Read-bound: 4 B per voxel (8 with a mask) against 3 subtractions, 9 products and 10 adds in double, all four loads
// (eight) of a lane's tile issued before the first use.  Measured (the same file): 0.211 ms at 512^3, 3.1 x the
// read-bound time; 17.5 us at 32^3, where it runs in the driver, which is the two launches.
// (256, 4) asks for no more than the compiler takes by itself: 52 VGPRs without a mask, 56 with one, 8 waves per SIMD
// by the registers, 352 bytes of LDS (the reduction's slots), nothing spilled (-Rpass-analysis=kernel-resource-usage).
template <bool MASKED>
__global__ __launch_bounds__(256, 4) void k_moments(const MomArgs s)
{
    __shared__ double slot[MOM_SUMS * 4];
    __shared__ unsigned long long cslot[4];
    const GridArgs &p = s.g;
    const int lx = threadIdx.x & 15;
    unsigned long long cnt = 0;
    double s0 = 0.0, sx = 0.0, sy = 0.0, sz = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
    for (unsigned base = 0; base < p.ntiles; base += gridDim.x) {
        int xt, y, z;
        if (!tile_at(p, base, xt, y, z))
            break;
        const bool row = y < p.oy && z < p.oz;
        const size_t orow = ((size_t)z * (size_t)p.oy + (size_t)y) * (size_t)p.ox;
        const double py = (double)y - s.cy, pz = (double)z - s.cz;
        float v[4], m[4];
        bool live[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int x = xt + lx + 16 * k;
            live[k] = row && x < p.ox;
            v[k] = 0.0f;
            m[k] = 1.0f;
            if (live[k]) {
                v[k] = s.V[orow + (size_t)x];
                if (MASKED)
                    m[k] = s.W[orow + (size_t)x];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float w = v[k] - s.floor;
            const bool counted = live[k] && w > 0.0f && (!MASKED || mask_in(m[k]));    // a NaN fails w > 0
            if (counted) {
                const double W = s.binary ? 1.0 : (double)w;
                const double px = (double)(xt + lx + 16 * k) - s.cx;
                const double wx = W * px, wy = W * py, wz = W * pz;
                cnt += 1;
                s0 += W;
                sx += wx;
                sy += wy;
                sz += wz;
                sxx += wx * px;
                sxy += wx * py;
                sxz += wx * pz;
                syy += wy * py;
                syz += wy * pz;
                szz += wz * pz;
            }
        }
    }
    const double sums[MOM_SUMS] = {s0, sx, sy, sz, sxx, sxy, sxz, syy, syz, szz};
    cnt = workgroup_reduce<Add>(cnt, cslot);
    if (threadIdx.x == 0)
        s.pcnt[blockIdx.x] = cnt;
#pragma unroll
    for (int i = 0; i < MOM_SUMS; i++) {
        const double a = workgroup_reduce<Add>(sums[i], slot + 4 * i);
        if (threadIdx.x == 0)
            s.psum[(size_t)i * REDUCE_GRID + blockIdx.x] = a;
    }
}

// the partial slots 0 .. n-1 in a fixed order (finish_reduce) into the record {n, S0, S1[3], S2[6]}
__global__ __launch_bounds__(256) void k_moments_finish(const unsigned long long *pcnt, const double *psum, unsigned n,
                                                        unsigned long long *record)
{
    __shared__ unsigned long long s_cnt[256];
    __shared__ double s_sum[256];
    const unsigned long long c = finish_reduce<Add>(pcnt, n, s_cnt);
    if (threadIdx.x == 0)
        record[0] = c;
    double *out = reinterpret_cast<double *>(record + 1);
    for (int k = 0; k < MOM_SUMS; k++) {
        __syncthreads();                                                     // s_sum's last read (s[0]) is done
        const double a = finish_reduce<Add>(psum + (size_t)k * REDUCE_GRID, n, s_sum);
        if (threadIdx.x == 0)
            out[k] = a;
    }
}

// ---- batched similarity ------------------------------------------------------------------------------------------------
// Candidate k's histogram and stats record are the bytes sift3d_hip_similarity_affine (_masked) writes for A_k, so the
// body below is k_similarity's (sift3d_similarity.hip) for FIELD == false, restated: tiles, lane-to-voxel assignment,
// per-lane order, workgroup_reduce into the workgroup's slot, finish_reduce over the slots.  bin_of and commit are
// restated too: moving them into a header would touch sift3d_similarity.hip, whose object code stays as it is.  What
// changes there changes here, by hand; tests/test_affine_init.py compares the two byte for byte.
//
// Mapping: one candidate per workgroup (blockIdx.y), BATCH_PER_LAUNCH candidates per launch, whose maps travel as
// kernel arguments (wave-uniform: scalar loads): the caller's host array is read when the entry is called, nothing is
// staged and the host waits for nothing.  A 32^3 level has 64 tiles, so a single call fills a quarter of the device's
// 256 CUs with one workgroup each; 343 candidates make 21952 workgroups in 11 launches.  Several candidates per workgroup
// sharing the tile's F loads were not built: F is 4 of the ~36 bytes a voxel gathers (8 corner values of M), a 32^3
// F stays in L2 (128 KiB), and at 121 - 128 VGPRs per candidate a second candidate's taps do not fit beside the first
// at 4 waves per SIMD.  Measured against the loop of single calls with their read-backs, 343 candidates, 32 bins
// (profiles/microbench/affine_init_rate_mi355x.txt): 0.340 ms against 20.7 at 32^3, 1.03 against 21.1 at 64^3, 5.55
// against 33.2 at 128^3.
constexpr int SIM_STATS = 7;                     // count, sum f, m, ff, mm, fm, dd
constexpr size_t SIM_SLOT_BYTES = SIM_STATS * 4 * sizeof(double);

constexpr int BATCH_PER_LAUNCH = 32;             // 32 x 96 bytes of the 4 KiB a kernel's arguments may take

struct BatchArgs {
    double A[BATCH_PER_LAUNCH][12];              // the maps of this launch's candidates, blockIdx.y = 0 .. gridDim.y - 1
    GridArgs g;                                  // src = M; ox, oy, oz = F's grid; dst unused
    const float *F;
    int bins;
    float lo_f, s_f, lo_m, s_m;
    unsigned long long *hist;                    // [gridDim.y][bins][bins]; HIST == true (this launch's candidates':
    unsigned long long *pcnt;                    // [gridDim.y][gridDim.x]               the launcher moves the three on)
    double *psum;                                // [gridDim.y][6][gridDim.x]
    MaskArgs w;
};

__device__ __forceinline__ int bin_of(float v, float lo, float s, int B)
{
    const float t = (v - lo) * s;
    return !(t >= 0.0f) ? 0 : t >= (float)B ? B - 1 : (int)t;
}

__device__ __forceinline__ void commit(unsigned *h, int idx, bool counted)
{
    const unsigned long long live = __ballot(counted);
    if (!live)
        return;                                                              // wave-uniform
    const int lead = __ffsll((long long)live) - 1;
    const int first = __builtin_amdgcn_readlane(idx, lead);
    if (__ballot(counted && idx != first) == 0) {                            // wave-uniform: every counted lane in one bin
        if ((int)(threadIdx.x & 63) == lead)
            atomicAdd(h + first, (unsigned)__popcll(live));
        return;
    }
    if (counted)
        atomicAdd(h + idx, 1u);
}

// Waves per SIMD asked of the compiler.  Four, as k_similarity, wherever the body fits 128 VGPRs without spilling; it
// does not with a moving mask beside the LDS histogram in linear mode (10 - 20 VGPRs spilled at four), nor on a moving
// grid one voxel wide (LINEAR == 1), so those take three.
constexpr int batch_waves(int linear, int masks, bool hist)
{
    return linear == 1 || (linear == 2 && (masks & 2) && hist) ? 3 : 4;
}

// -Rpass-analysis=kernel-resource-usage, nothing spilled in any of the 24 instantiations:
//   LINEAR 2 (the search's):  121 - 128 VGPRs, 4 waves per SIMD; with a moving mask and a histogram 134 - 136, 3 waves
//   LINEAR 1 (nx == 1):       128 - 162 VGPRs, 3 - 4 waves
//   nearest:                  56 VGPRs, 7 - 8 waves (7: 102 SGPRs)
// MASKS: bit 0 the fixed mask is given, bit 1 the moving one: k_similarity tests the two pointers in the kernel; a
// template argument spares the branch and the registers of a mask that is not there.
// HIST == false (bins == 0): no histogram, in LDS or in memory.
template <int LINEAR, int MASKS, bool HIST>
__global__ __launch_bounds__(256, batch_waves(LINEAR, MASKS, HIST)) void k_similarity_batch(const BatchArgs s)
{
    constexpr bool MASKED = MASKS != 0;
    extern __shared__ __align__(16) unsigned char sim_lds[];
    unsigned *h = reinterpret_cast<unsigned *>(sim_lds);
    const GridArgs &p = s.g;
    const int B = s.bins, BB = B * B;
    const unsigned cand = blockIdx.y;
    const double *a = s.A[cand];
    if (HIST) {
        for (int i = threadIdx.x; i < BB; i += 256)
            h[i] = 0u;
        __syncthreads();
    }
    const int lx = threadIdx.x & 15;
    unsigned long long cnt = 0;
    double sf = 0.0, sm = 0.0, sff = 0.0, smm = 0.0, sfm = 0.0, sdd = 0.0;
    for (unsigned base = 0; base < p.ntiles; base += gridDim.x) {
        int xt, y, z;
        if (!tile_at(p, base, xt, y, z))
            break;
        const bool row = y < p.oy && z < p.oz;
        const size_t orow = ((size_t)z * (size_t)p.oy + (size_t)y) * (size_t)p.ox;
        const double yd = (double)y, zd = (double)z;
        const double rx = pull_row(a, yd, zd), ry = pull_row(a + 4, yd, zd), rz = pull_row(a + 8, yd, zd);
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
            if (live[k]) {
                f[k] = s.F[orow + (size_t)x];
                if (MASKS & 1)
                    wf[k] = s.w.wf[orow + (size_t)x];
            }
            const double xd = (double)x;
            const double qx = pull(a, xd, rx), qy = pull(a + 4, xd, ry), qz = pull(a + 8, xd, rz);
            tp[k] = taps_at<LINEAR>(p.nx, p.ny, p.nz, qx, qy, qz);
            if (MASKS & 2)
                wm[k] = s.w.wm[mask_offset(p.nx, p.ny, p.nz, qx, qy, qz)];
        }
        float m[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
            m[k] = gather<LINEAR>(p.src, tp[k], 0.0f);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool counted = MASKED ? live[k] && tp[k].in && mask_in(wf[k]) && mask_in(wm[k]) : live[k] && tp[k].in;
            if (HIST) {
                const int idx = bin_of(f[k], s.lo_f, s.s_f, B) * B + bin_of(m[k], s.lo_m, s.s_m, B);
                commit(h, idx, counted);
            }
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
    if (HIST) {
        // flush: this workgroup's non-zero words into the candidate's histogram (integer atomics: exact)
        unsigned long long *hist = s.hist + (size_t)cand * (size_t)BB;
        __syncthreads();
        for (int i = threadIdx.x; i < BB; i += 256) {
            const unsigned c = h[i];
            if (c)
                atomicAdd(hist + i, (unsigned long long)c);
        }
        __syncthreads();                                                     // the histogram's LDS is free
    }
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
        const size_t G = gridDim.x;
        double *ps = s.psum + (size_t)cand * 6 * G;
        s.pcnt[(size_t)cand * G + blockIdx.x] = cnt;
        ps[blockIdx.x] = sf;
        ps[G + blockIdx.x] = sm;
        ps[2 * G + blockIdx.x] = sff;
        ps[3 * G + blockIdx.x] = smm;
        ps[4 * G + blockIdx.x] = sfm;
        ps[5 * G + blockIdx.x] = sdd;
    }
}

// workgroup k: candidate k's partial slots 0 .. n-1 in k_similarity_finish's order into record k (56 bytes)
__global__ __launch_bounds__(256) void k_similarity_batch_finish(const unsigned long long *pcnt, const double *psum,
                                                                 unsigned n, unsigned long long *stats)
{
    __shared__ unsigned long long s_cnt[256];
    __shared__ double s_sum[256];
    const size_t cand = blockIdx.x;
    unsigned long long *rec = stats + cand * SIM_STATS;
    const unsigned long long c = finish_reduce<Add>(pcnt + cand * n, n, s_cnt);
    if (threadIdx.x == 0)
        rec[0] = c;
    double *out = reinterpret_cast<double *>(rec + 1);
    for (int k = 0; k < 6; k++) {
        __syncthreads();                                                     // s_sum's last read (s[0]) is done
        const double a = finish_reduce<Add>(psum + (cand * 6 + k) * n, n, s_sum);
        if (threadIdx.x == 0)
            out[k] = a;
    }
}

template <int MASKS, bool HIST>
void (*pick_interp(int interp, int nx))(const BatchArgs)
{
    return interp == SIFT3D_AMD_INTERP_NEAREST ? k_similarity_batch<0, MASKS, HIST>
           : nx >= 2                           ? k_similarity_batch<2, MASKS, HIST>
                                               : k_similarity_batch<1, MASKS, HIST>;
}

// masks: bit 0 the fixed mask is given, bit 1 the moving one (k_similarity tests the two pointers in the kernel)
template <bool HIST>
void (*pick_batch(int masks, int interp, int nx))(const BatchArgs)
{
    return masks == 3   ? pick_interp<3, HIST>(interp, nx)
           : masks == 2 ? pick_interp<2, HIST>(interp, nx)
           : masks == 1 ? pick_interp<1, HIST>(interp, nx)
                        : pick_interp<0, HIST>(interp, nx);
}

} // namespace

// Launchers for sift3d_init.c, which has checked every argument (not exported from the library).

extern "C" int sift3d_moments_launch(const char *fn, const float *d_V, int nx, int ny, int nz, const float *d_W,
                                     int binary, float floor, void *d_record, void *d_work, void *stream)
{
    MomArgs s;
    if (!grid_args(s.g, nullptr, 1, 1, 1, nullptr, nx, ny, nz, 0.0f))
        return launch_fail(fn, "grid too large");
    s.V = d_V;
    s.W = d_W;
    s.floor = floor;
    s.binary = binary;
    s.cx = (double)(nx - 1) / 2.0;
    s.cy = (double)(ny - 1) / 2.0;
    s.cz = (double)(nz - 1) / 2.0;
    s.pcnt = (unsigned long long *)d_work;
    s.psum = (double *)d_work + REDUCE_GRID;
    const unsigned grid = reduce_grid(s.g.ntiles);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(d_W ? k_moments<true> : k_moments<false>, dim3(grid), dim3(256), 0, st, s);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_moments_finish, dim3(1), dim3(256), 0, st, s.pcnt, s.psum, grid,
                       (unsigned long long *)d_record);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

// the workgroups (and partial slots) per candidate of a batch on this fixed grid; 0 when it has too many tiles
extern "C" unsigned sift3d_similarity_batch_grid(int ox, int oy, int oz)
{
    GridArgs g;
    if (!grid_args(g, nullptr, 1, 1, 1, nullptr, ox, oy, oz, 0.0f))
        return 0;
    return reduce_grid(g.ntiles);
}

// d_work: pcnt [K][grid] uint64, then psum [K][6][grid] double.  A: the K maps on the host, read here (the caller's
// array is free when the call returns).  bins == 0: no histogram (d_hist NULL).
extern "C" int sift3d_similarity_batch_launch(const char *fn, const float *d_F, int ox, int oy, int oz,
                                              const float *d_M, int nx, int ny, int nz, const double *A, int K,
                                              int interp, int bins, float lo_f, float s_f, float lo_m, float s_m,
                                              unsigned long long *d_hist, void *d_stats, void *d_work, void *stream,
                                              const float *d_WF, const float *d_WM)
{
    BatchArgs s;
    if (!grid_args(s.g, d_M, nx, ny, nz, nullptr, ox, oy, oz, 0.0f))
        return launch_fail(fn, "grid too large");
    const GridArgs &p = s.g;
    const unsigned grid = reduce_grid(p.ntiles);
    const unsigned long long passes = ((unsigned long long)p.ntiles + grid - 1) / grid;
    if (passes * (unsigned long long)(TX * TY * TZ) > 0xffffffffull)
        return launch_fail(fn, "grid too large");
    s.F = d_F;
    s.bins = bins;
    s.lo_f = lo_f; s.s_f = s_f;
    s.lo_m = lo_m; s.s_m = s_m;
    s.hist = d_hist;
    unsigned long long *const pcnt = (unsigned long long *)d_work;
    double *const psum = (double *)(pcnt + (size_t)K * grid);
    s.w = MaskArgs{d_WF, d_WM};
    const int masks = (d_WF ? 1 : 0) | (d_WM ? 2 : 0);
    void (*k)(const BatchArgs) = bins ? pick_batch<true>(masks, interp, nx) : pick_batch<false>(masks, interp, nx);
    const size_t hb = (size_t)bins * bins * sizeof(unsigned);
    const size_t lds = hb > SIM_SLOT_BYTES ? hb : SIM_SLOT_BYTES;
    hipStream_t st = (hipStream_t)stream;
    if (bins)
        HIPCHK(hipMemsetAsync(d_hist, 0, (size_t)K * bins * bins * sizeof(unsigned long long), st));
    for (int k0 = 0; k0 < K; k0 += BATCH_PER_LAUNCH) {
        const int nk = K - k0 < BATCH_PER_LAUNCH ? K - k0 : BATCH_PER_LAUNCH;
        memcpy(s.A, A + (size_t)k0 * 12, (size_t)nk * 12 * sizeof(double));
        s.hist = d_hist + (size_t)k0 * bins * bins;
        s.pcnt = pcnt + (size_t)k0 * grid;
        s.psum = psum + (size_t)k0 * 6 * grid;
        hipLaunchKernelGGL(k, dim3(grid, (unsigned)nk), dim3(256), lds, st, s);
        LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_similarity_batch_finish, dim3((unsigned)K), dim3(256), 0, st, pcnt, psum, grid,
                       (unsigned long long *)d_stats);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}
