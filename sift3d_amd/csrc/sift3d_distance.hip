// sift3d_distance.hip -- exact Euclidean distance transform of a mask in three per-axis passes, the signed distance,
// the six-neighbour surface of a label and the list of distances at surface voxels.
// Contract: include/sift3d_amd.h, "Distance transforms and surface distances"; restated in numpy by
// tests/distance_restatement.py (every output bit for bit, tests/test_distance.py).
//
// The three passes move 8 B per voxel each (4 read, 4 written) and do next to no arithmetic, so what matters is that a
// wave always touches a contiguous row segment:
//   - k_edt_x: one wave per row.  A row has at most 4096 / 64 = 64 chunks of 64 voxels, so the wave reads the row once,
//     chunk by chunk, and lane c keeps chunk c's feature ballot: the whole row's feature set sits in one 64-bit
//     register per lane.  The nearest feature to the left (right) of a voxel is then the highest (lowest) set bit of
//     its chunk's ballot at or below (above) its lane -- the wave-level max / min scan of feature indices, done with
//     one clz / ffs on the ballot -- and, where the chunk holds none on that side, the last (first) feature of the
//     nearest non-empty chunk before (after) it, found the same way on the ballot of (ballot != 0) over the lanes: the
//     carry between chunks, from both ends, without reading the row a second time.  The second loop only writes.
//   - k_edt_line<AXIS>: lanes along x, one output voxel per lane, a wave per (x chunk, y, z).  best = g(i), then
//     outwards r = 1, 2, ... on both sides at once: t(r) = w * (float) (r r) is the same on both, so one test
//     t(r) >= best ends both (g >= 0 and + is monotone: nothing further out can be smaller, ties included), and the
//     grid's two edges end a side each.  Every step reads one contiguous row segment per side.  Waves that follow one
//     another in a workgroup are neighbours ALONG the line, so the segments they read are the same lines of the cache.
//     The search costs a voxel as many steps as its distance along the axis, in voxels; the worst case is O(n): a line
//     (or a whole plane) without a feature, best = +inf, walks to both edges.  The walk is a chain of dependent loads
//     and tests, so the kernel takes EDT_STEP = 8 radii per test with their 16 loads in flight together (every value
//     taken is a candidate of the minimum, so the few radii past the stop change nothing): at 512^3, 46 ms with one
//     radius per test, 33 with 4, 31 with 8, 30 with 16 on a ball of radius n / 4.  Measured and not kept
//     (profiles/microbench/distance_mi355x.txt): several consecutive outputs per wave (slower: fewer waves in flight
//     hide less latency) and a contiguous run of lines per XCD (the lines far from the features cost most, and then
//     sit behind one XCD).  No LDS staging.  What would change the order of the cost is a lower-envelope line solver.
//   - k_signed_combine, k_label_surface, k_surface_collect: one pass each.  Counts are ballots added per wave; the
//     label surface adds one 64-bit atomic per workgroup, the collector reserves a wave's slots with one.
#include "sift3d_kernels_common.h"

#include <cmath>

namespace {

typedef unsigned long long u64;

constexpr int EDT_MAX_DIM = SIFT3D_AMD_DISTANCE_MAX_DIM;
constexpr unsigned EDT_MAX_BLOCKS = 1u << 20;                 // grid-stride beyond that
#ifndef EDT_STEP
#define EDT_STEP 8                                            // radii per step of the outward search
#endif
static_assert(EDT_MAX_DIM <= 64 * 64, "k_edt_x keeps one chunk ballot per lane");

__device__ __forceinline__ bool mask_in(float w) { return w >= 0.5f; }          // header, "Masks": a NaN is out

__device__ __forceinline__ int high_bit(u64 b) { return 63 - __clzll((long long)b); }   // b != 0
__device__ __forceinline__ int low_bit(u64 b) { return __ffsll((long long)b) - 1; }     // b != 0

// the wave's index in its workgroup as the scalar it is (the compiler takes threadIdx.x >> 6 for a per-lane value):
// the split of a wave's number into line, segment and position is then scalar arithmetic, once per wave
__device__ __forceinline__ unsigned wave_index() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }

static inline unsigned blocks_for(size_t waves)
{
    const size_t b = (waves + 3) / 4;
    return (unsigned)(b < 1 ? 1 : b > EDT_MAX_BLOCKS ? EDT_MAX_BLOCKS : b);
}

// out = w_x * (float) (dx dx) to the nearest feature of the row, +inf for a row without one
__global__ __launch_bounds__(256) void k_edt_x(const float *__restrict__ mask, float *__restrict__ out, int nx,
                                               size_t rows, float wx, int invert)
{
    const int lane = threadIdx.x & 63;
    const int nchunks = (nx + 63) >> 6;                                          // <= 64
    const size_t nwaves = (size_t)gridDim.x * 4;
    for (size_t r = (size_t)blockIdx.x * 4 + wave_index(); r < rows; r += nwaves) {         // wave-uniform
        const float *m = mask + r * (size_t)nx;
        float *o = out + r * (size_t)nx;
        u64 mine = 0;                                                            // lane c: the ballot of chunk c
        for (int c = 0; c < nchunks; c++) {
            const int x = c * 64 + lane;
            bool f = false;
            if (x < nx)
                f = mask_in(m[x]) != (invert != 0);
            const u64 b = __ballot(f);
            if (lane == c)
                mine = b;
        }
        const u64 nonempty = __ballot(mine != 0);                                // bit c: chunk c holds a feature
        for (int c = 0; c < nchunks; c++) {
            // the carries, wave-uniform and outside any divergent code (a shuffle reads live lanes only)
            const u64 before = nonempty & ((1ull << c) - 1);
            const u64 after = c < 63 ? nonempty & (~0ull << (c + 1)) : 0;
            const int pc = before ? high_bit(before) : 0;
            const int nc = after ? low_bit(after) : 0;
            const u64 b = __shfl(mine, c, 64), pb = __shfl(mine, pc, 64), nb = __shfl(mine, nc, 64);
            const int carry_l = before ? pc * 64 + high_bit(pb) : -1;
            const int carry_r = after ? nc * 64 + low_bit(nb) : -1;
            const int x = c * 64 + lane;
            const u64 lm = b & (~0ull >> (63 - lane));                           // features at lanes <= this one
            const u64 rm = b & (~0ull << lane);                                  // at lanes >= this one
            const int L = lm ? c * 64 + high_bit(lm) : carry_l;
            const int R = rm ? c * 64 + low_bit(rm) : carry_r;
            int d = -1;
            if (L >= 0)
                d = x - L;
            if (R >= 0 && (d < 0 || R - x < d))
                d = R - x;
            if (x < nx)
                o[x] = d < 0 ? INFINITY : wx * (float)(d * d);                   // d <= 4095: d d is exact
        }
    }
}

// out(i) = min over i' of g(i') + w * (float) ((i - i') (i - i')) along AXIS (1: y, 2: z); ROOT: its sqrtf
template <int AXIS, bool ROOT>
__global__ __launch_bounds__(256) void k_edt_line(const float *__restrict__ g, float *__restrict__ out, int nx, int ny,
                                                  int nz, float w)
{
    const int lane = threadIdx.x & 63;
    const int n = AXIS == 1 ? ny : nz, other = AXIS == 1 ? nz : ny;
    const size_t stride = AXIS == 1 ? (size_t)nx : (size_t)nx * (size_t)ny;      // along the line
    const size_t ostride = AXIS == 1 ? (size_t)nx * (size_t)ny : (size_t)nx;     // between lines
    const size_t xchunks = (size_t)((nx + 63) >> 6);
    const size_t total = (size_t)other * xchunks * (size_t)n;
    const size_t nwaves = (size_t)gridDim.x * 4;
    for (size_t wid = (size_t)blockIdx.x * 4 + wave_index(); wid < total; wid += nwaves) {
        // wave-uniform, in scalar registers: every row below is a scalar base plus the lane
        const int i = (int)(wid % (size_t)n);                                    // fastest: neighbours share rows
        const size_t t0 = wid / (size_t)n;
        const int x0 = (int)(t0 % xchunks) * 64;
        const size_t o = t0 / xchunks;
        if (x0 + lane >= nx)
            continue;
        const float *line = g + o * ostride + (size_t)x0;
        float best = (line + (size_t)i * stride)[lane];
        for (int r = 1; r < n; r += EDT_STEP) {
            if (w * (float)(r * r) >= best || (i - r < 0 && i + r >= n))         // r <= 4095: r r is exact
                break;
            // EDT_STEP radii at once, their loads in flight together.  Every value taken is a candidate of the
            // minimum, so looking past the radius at which the next test would have stopped changes nothing; a radius
            // with both ends beyond the grid (only there can r r leave the exact integers) takes none.
            float c[2 * EDT_STEP];
#pragma unroll
            for (int k = 0; k < EDT_STEP; k++) {
                const int rr = r + k, a = i - rr, b = i + rr;
                const float t = w * (float)(rr * rr);
                c[2 * k] = a >= 0 ? (line + (size_t)a * stride)[lane] + t : INFINITY;
                c[2 * k + 1] = b < n ? (line + (size_t)b * stride)[lane] + t : INFINITY;
            }
#pragma unroll
            for (int k = 0; k < 2 * EDT_STEP; k++)
                best = c[k] < best ? c[k] : best;
        }
        (out + o * ostride + (size_t)x0 + (size_t)i * stride)[lane] = ROOT ? sqrtf(best) : best;
    }
}

// io holds D2 to the complement; io = in the set ? -sqrtf(io) : +sqrtf(D2 to the set)
__global__ __launch_bounds__(256) void k_signed_combine(const float *__restrict__ mask, const float *__restrict__ d2set,
                                                        float *__restrict__ io, size_t n)
{
    const size_t step = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step)
        io[i] = mask_in(mask[i]) ? -sqrtf(io[i]) : sqrtf(d2set[i]);
}

// surface = 1 where L == k and a face neighbour (one beyond the grid included) is not, else 0; *count += their number
__global__ __launch_bounds__(256) void k_label_surface(const float *__restrict__ L, float *__restrict__ surface, int nx,
                                                       int ny, int nz, float k, u64 *count)
{
    __shared__ u64 s_cnt[4];
    const int lane = threadIdx.x & 63;
    const size_t sy = (size_t)nx, sz = (size_t)nx * (size_t)ny;
    const size_t xchunks = (size_t)((nx + 63) >> 6);
    const size_t total = xchunks * (size_t)ny * (size_t)nz;
    const size_t nwaves = (size_t)gridDim.x * 4;
    u64 cnt = 0;                                                                 // wave-uniform
    for (size_t wid = (size_t)blockIdx.x * 4 + wave_index(); wid < total; wid += nwaves) {
        const int x = (int)(wid % xchunks) * 64 + lane;
        const size_t t0 = wid / xchunks;
        const int y = (int)(t0 % (size_t)ny), z = (int)(t0 / (size_t)ny);
        bool s = false;
        if (x < nx) {
            const size_t at = (size_t)z * sz + (size_t)y * sy + (size_t)x;
            if (L[at] == k)
                s = x == 0 || x == nx - 1 || y == 0 || y == ny - 1 || z == 0 || z == nz - 1 ||
                    !(L[at - 1] == k) || !(L[at + 1] == k) || !(L[at - sy] == k) || !(L[at + sy] == k) ||
                    !(L[at - sz] == k) || !(L[at + sz] == k);
            surface[at] = s ? 1.0f : 0.0f;
        }
        cnt += (u64)__popcll(__ballot(s));
    }
    if (lane == 0)
        s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 c = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
        if (c)
            atomicAdd(count, c);
    }
}

// appends sqrtf(d2[i]) for every i with surface[i] in; *count += their number, nothing is written at or past capacity
__global__ __launch_bounds__(256) void k_surface_collect(const float *__restrict__ surface,
                                                         const float *__restrict__ d2, size_t n,
                                                         float *__restrict__ list, u64 capacity, u64 *count)
{
    const int lane = threadIdx.x & 63;
    const size_t step = (size_t)gridDim.x * 256;
    for (size_t base = (size_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < n; base += step) {   // wave-uniform
        const size_t i = base + (size_t)lane;
        const bool s = i < n && mask_in(surface[i]);
        const u64 b = __ballot(s);
        if (!b)
            continue;
        u64 first = 0;
        if (lane == 0)
            first = atomicAdd(count, (u64)__popcll(b));
        first = __shfl(first, 0, 64);
        if (s) {
            const u64 pos = first + (u64)__popcll(b & ((1ull << lane) - 1));
            if (pos < capacity)
                list[pos] = sqrtf(d2[i]);
        }
    }
}

} // namespace

// Launchers for sift3d_distance.c, which has checked every argument (not exported from the library).

// the three passes: mask -> d_out (x), d_out -> d_work (y), d_work -> d_out (z; root != 0: its square root)
extern "C" int sift3d_distance_launch(const char *fn, const float *d_mask, int nx, int ny, int nz, float wx, float wy,
                                      float wz, int invert, int root, float *d_out, float *d_work, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const size_t rows = (size_t)ny * (size_t)nz, xchunks = (size_t)((nx + 63) >> 6);
    const size_t waves = rows * xchunks;                                         // of a line pass: one per row segment
    (void)fn;
    hipLaunchKernelGGL(k_edt_x, dim3(blocks_for(rows)), dim3(256), 0, st, d_mask, d_out, nx, rows, wx, invert);
    LAUNCH_CHECK();
    hipLaunchKernelGGL((k_edt_line<1, false>), dim3(blocks_for(waves)), dim3(256), 0, st, (const float *)d_out, d_work,
                       nx, ny, nz, wy);
    LAUNCH_CHECK();
    if (root)
        hipLaunchKernelGGL((k_edt_line<2, true>), dim3(blocks_for(waves)), dim3(256), 0, st, (const float *)d_work,
                           d_out, nx, ny, nz, wz);
    else
        hipLaunchKernelGGL((k_edt_line<2, false>), dim3(blocks_for(waves)), dim3(256), 0, st, (const float *)d_work,
                           d_out, nx, ny, nz, wz);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

extern "C" int sift3d_signed_combine_launch(const char *fn, const float *d_mask, const float *d_d2set, float *d_io,
                                            size_t n, void *stream)
{
    (void)fn;
    hipLaunchKernelGGL(k_signed_combine, dim3(grid_for(n, 4)), dim3(256), 0, (hipStream_t)stream, d_mask, d_d2set, d_io,
                       n);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

extern "C" int sift3d_label_surface_launch(const char *fn, const float *d_labels, int nx, int ny, int nz, int label,
                                           float *d_surface, uint64_t *d_count, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const size_t waves = (size_t)ny * (size_t)nz * (size_t)((nx + 63) >> 6);
    (void)fn;
    HIPCHK(hipMemsetAsync(d_count, 0, sizeof(uint64_t), st));
    hipLaunchKernelGGL(k_label_surface, dim3(blocks_for(waves)), dim3(256), 0, st, d_labels, d_surface, nx, ny, nz,
                       (float)label, (u64 *)d_count);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

extern "C" int sift3d_surface_collect_launch(const char *fn, const float *d_surface, const float *d_d2, size_t n,
                                             float *d_list, size_t capacity, uint64_t *d_count, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    (void)fn;
    HIPCHK(hipMemsetAsync(d_count, 0, sizeof(uint64_t), st));
    hipLaunchKernelGGL(k_surface_collect, dim3(grid_for(n, 4)), dim3(256), 0, st, d_surface, d_d2, n, d_list,
                       (u64)capacity, (u64 *)d_count);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}
