// sift3d_discrete.hip -- discrete displacement search: the multi-channel cost volume of every 4^3 block over a
// (2R+1)^3 label cube, the coupled selection of one label per block, the binomial smoothing of a block field and its
// expansion to a voxel field (contract: include/sift3d_amd.h, "Discrete displacement search").
//
// k_cost_volume<R>.  k_block_match<R>'s mapping with a channel loop around it.  One workgroup (4 waves) takes a tile
// of TBX x TBY x TBZ adjacent blocks and stages the W neighbourhood of the tile in LDS, ONE CHANNEL AT A TIME:
// (4 TBX + 2R) x (4 TBY + 2R) x (4 TBZ + 2R) floats.  A voxel that is off the grid or out of V_W is staged as NaN: the
// inputs are finite, so a NaN sum means exactly "a voxel of the shifted block is off the grid or masked out", and it
// leaves as +inf with no validity array.
// A wave owns BPW = TILE_BLOCKS / 4 blocks of the tile for the whole channel loop and ONE LANE PER LABEL: lane l holds
// the double accumulators of labels k = l, l + 64, ... (NL = ceil(K / 64) of them) of each of its blocks in registers,
// BPW x NL doubles, carried across the channels.  The sums therefore run in the contract's order (channels outermost,
// voxels i = 0 .. 63 inside) and no cross-lane reduction touches one.  The block's 64 F values of the channel are
// fetched one per lane and read back by v_readlane (wave-uniform), promoted to double once per voxel and shared by JC
// independent chains of the lane (NL in chunks of JC <= 7: more chains in flight only cost registers).  Per term: one ds_read_b32 at an immediate offset, one f32 -> f64 convert, a
// double subtract, multiply and add.  Lanes of consecutive k have consecutive dx: they read consecutive LDS words and
// write consecutive floats of d_cost.
// The tile shrinks as R grows so that BPW x NL stays within the register file (see CvGeo): LDS is never the limit
// (25.6 KB at R = 6), the accumulators are.
//
// k_cost_select<R>: one wave per block streams its K floats once (lane l: k = l, l + 64, ...), reduces with the
// contract's total order (val, then |d|^2, then k) and writes v, the chosen cost and the workgroup's partial of the
// statistics; k_cost_select_finish adds the partials in a fixed order.
// k_block_field_smooth: one launch per pass, the x, y and z binomials evaluated in place of three sweeps (27 reads per
// output, the same float operations in the same order).  k_block_field_expand: one lane per voxel.
#include "sift3d_resample.h"

#include <climits>

// the labels a lane sums at once are fixed by R; the blocks a wave owns (tile / 4) are a build option for
// profiles/microbench/cost_volume_rate.py: 0 takes the table in CvGeo
#ifndef SIFT3D_CV_TILE
#define SIFT3D_CV_TILE 0
#endif

namespace {

constexpr int WAVES = 4;
constexpr unsigned SELECT_GRID = SIFT3D_AMD_COST_SELECT_WORK_BYTES / 16;   // partial slots: a double and a uint64 each

struct CvArgs {
    const float *F, *W, *VF, *VW;
    int nc;
    int nx, ny, nz;
    int nbx, nby, nbz;
    int tiles_x, tiles_y;
    float *cost;
};

// The tile of blocks per R.  BPW x NL doubles per lane: 4 / 8 / 12 / 24 / 21 / 35 for R = 1 .. 6.
template <int R> struct CvGeo {
    static constexpr int D = 2 * R + 1, K = D * D * D, NL = (K + 63) / 64;
    // the labels of a lane that share one trip through the block's 64 voxels (the chains in flight): NL in chunks of JC
    static constexpr int JC = NL % 7 == 0 ? 7 : (NL % 6 == 0 ? 6 : NL);
#if SIFT3D_CV_TILE == 16
    static constexpr int TBX = 4, TBY = 2, TBZ = 2;
#elif SIFT3D_CV_TILE == 8
    static constexpr int TBX = 2, TBY = 2, TBZ = 2;
#elif SIFT3D_CV_TILE == 4
    static constexpr int TBX = 2, TBY = 2, TBZ = 1;
#else
    static constexpr int TBX = R <= 2 ? 4 : 2, TBY = 2, TBZ = R <= 4 ? 2 : 1;
#endif
    static constexpr int TILE_BLOCKS = TBX * TBY * TBZ, BPW = TILE_BLOCKS / WAVES;
    static constexpr int SX = 4 * TBX + 2 * R, SY = 4 * TBY + 2 * R, SZ = 4 * TBZ + 2 * R;
    static constexpr int STAGED = SX * SY * SZ;
    static_assert(TILE_BLOCKS % WAVES == 0, "a wave owns a whole number of blocks");
    static_assert(STAGED * sizeof(float) <= 65536, "the staged tile does not fit the static LDS limit");
};

template <int R>
__global__ __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(2))) void k_cost_volume(const CvArgs p)
{
    using G = CvGeo<R>;
    constexpr int D = G::D, K = G::K, NL = G::NL, JC = G::JC, BPW = G::BPW, SX = G::SX, SY = G::SY;
    __shared__ __attribute__((aligned(16))) float s_w[G::STAGED];

    const int tile = blockIdx.x;
    const int tx = tile % p.tiles_x, ty = (tile / p.tiles_x) % p.tiles_y, tz = tile / (p.tiles_x * p.tiles_y);
    const int bx0 = tx * G::TBX, by0 = ty * G::TBY, bz0 = tz * G::TBZ;
    const size_t sx = (size_t)p.nx, plane = sx * (size_t)p.ny, vox = plane * (size_t)p.nz;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    // the label's first voxel relative to the block's own position in the staged tile; a lane past the last label
    // repeats it and stores nothing
    int rel[NL];
#pragma unroll
    for (int j = 0; j < NL; j++) {
        const int k = lane + 64 * j < K ? lane + 64 * j : K - 1;
        rel[j] = ((k / (D * D) - R) * SY + ((k / D) % D - R)) * SX + (k % D - R);
    }

    // the wave's blocks: b = wave + WAVES * m (all wave-uniform)
    bool on[BPW], ok[BPW];
    size_t g0[BPW];                                              // lane's F voxel of the block, channel 0
    int own[BPW];                                                // the block's own first voxel in the staged tile
    double acc[BPW][NL];
#pragma unroll
    for (int m = 0; m < BPW; m++) {
        const int b = wave + WAVES * m;
        const int lx = b % G::TBX, ly = (b / G::TBX) % G::TBY, lz = b / (G::TBX * G::TBY);
        const int bx = bx0 + lx, by = by0 + ly, bz = bz0 + lz;
        on[m] = bx < p.nbx && by < p.nby && bz < p.nbz;
        own[m] = ((4 * lz + R) * SY + (4 * ly + R)) * SX + (4 * lx + R);
        g0[m] = 0;
        ok[m] = false;
        if (on[m]) {
            g0[m] = (size_t)(4 * bz + (lane >> 4)) * plane + (size_t)(4 * by + ((lane >> 2) & 3)) * sx +
                    (size_t)(4 * bx + (lane & 3));
            const bool in_mask = !p.VF || p.VF[g0[m]] >= 0.5f;
            ok[m] = __ballot(in_mask) == ~0ull;
        }
#pragma unroll
        for (int j = 0; j < NL; j++)
            acc[m][j] = 0.0;
    }

    const int ox = 4 * bx0 - R, oy = 4 * by0 - R, oz = 4 * bz0 - R;
    for (int c = 0; c < p.nc; c++) {
        const float *Wc = p.W + (size_t)c * vox;
        const float *Fc = p.F + (size_t)c * vox;
        __syncthreads();                                         // the last channel's reads are done
        for (int i = threadIdx.x; i < G::STAGED; i += 64 * WAVES) {
            const int x = i % SX, y = (i / SX) % SY, z = i / (SX * SY);
            const int gx = ox + x, gy = oy + y, gz = oz + z;
            float v = __builtin_nanf("");
            if (gx >= 0 && gx < p.nx && gy >= 0 && gy < p.ny && gz >= 0 && gz < p.nz) {
                const size_t g = (size_t)gz * plane + (size_t)gy * sx + (size_t)gx;
                if (!p.VW || p.VW[g] >= 0.5f)
                    v = Wc[g];
            }
            s_w[i] = v;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < BPW; m++) {
            if (!ok[m])
                continue;                                        // wave-uniform; no barrier below
            const float f = Fc[g0[m]];
            const float *w0 = s_w + own[m];
#pragma unroll
            for (int j0 = 0; j0 < NL; j0 += JC) {
#pragma unroll 1
                for (int z = 0; z < 4; z++) {
#pragma unroll
                    for (int y = 0; y < 4; y++)
#pragma unroll
                        for (int x = 0; x < 4; x++) {
                            const double fd = (double)__int_as_float(
                                __builtin_amdgcn_readlane(__float_as_int(f), (z * 4 + y) * 4 + x));
#pragma unroll
                            for (int j = j0; j < j0 + JC; j++) {
                                const double e = fd - (double)w0[rel[j] + (z * SY + y) * SX + x];
                                const double s = e * e;
                                acc[m][j] = acc[m][j] + s;
                            }
                        }
                }
            }
        }
    }

    const double den = 64.0 * (double)p.nc;
    const float inf = __builtin_inff();
#pragma unroll
    for (int m = 0; m < BPW; m++) {
        if (!on[m])
            continue;
        const int b = wave + WAVES * m;
        const int lx = b % G::TBX, ly = (b / G::TBX) % G::TBY, lz = b / (G::TBX * G::TBY);
        const size_t blk = ((size_t)(bz0 + lz) * p.nby + (size_t)(by0 + ly)) * p.nbx + (size_t)(bx0 + lx);
        float *out = p.cost + blk * (size_t)K;
#pragma unroll
        for (int j = 0; j < NL; j++) {
            const int k = lane + 64 * j;
            if (k < K) {
                const float cst = (float)(acc[m][j] / den);
                out[k] = ok[m] && cst < inf ? cst : inf;         // a NaN sum (off the grid, masked) fails the compare
            }
        }
    }
}

// ---- coupled selection ----

struct Pick {
    double val;
    int d2, k;
};

// the contract's choice: smaller val, then smaller |d|^2, then smaller k
__device__ __forceinline__ bool pick_better(const Pick &a, const Pick &b)
{
    return a.val < b.val || (a.val == b.val && (a.d2 < b.d2 || (a.d2 == b.d2 && a.k < b.k)));
}

template <int R>
__global__ __launch_bounds__(64 * WAVES) void k_cost_select(const float *__restrict__ cost, size_t nb,
                                                            const float *__restrict__ u, double theta,
                                                            float *__restrict__ v, float *__restrict__ data,
                                                            double *__restrict__ psum,
                                                            unsigned long long *__restrict__ pcnt)
{
    constexpr int D = 2 * R + 1, K = D * D * D;
    __shared__ double s_sum[4];
    __shared__ unsigned long long s_cnt[4];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float inf = __builtin_inff();
    double lsum = 0.0;
    unsigned long long lcnt = 0;
    for (size_t b = (size_t)blockIdx.x * WAVES + wave; b < nb; b += (size_t)gridDim.x * WAVES) {
        const float *cb = cost + b * (size_t)K;
        const float ux = u[b], uy = u[nb + b], uz = u[2 * nb + b];
        Pick best = { (double)inf, INT_MAX, INT_MAX };
        for (int k = lane; k < K; k += 64) {
            const int dx = k % D - R, dy = (k / D) % D - R, dz = k / (D * D) - R;
            const double ex = (double)dx - (double)ux, ey = (double)dy - (double)uy, ez = (double)dz - (double)uz;
            const double q = (ex * ex + ey * ey) + ez * ez;
            const double tq = theta * q;
            const Pick c = { (double)cb[k] + tq, dx * dx + dy * dy + dz * dz, k };
            if (pick_better(c, best))
                best = c;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const Pick other = { __shfl_xor(best.val, o, 64), __shfl_xor(best.d2, o, 64), __shfl_xor(best.k, o, 64) };
            if (pick_better(other, best))
                best = other;
        }
        if (lane == 0) {
            if (best.val < (double)inf) {
                const float c = cb[best.k];
                v[b] = (float)(best.k % D - R);
                v[nb + b] = (float)((best.k / D) % D - R);
                v[2 * nb + b] = (float)(best.k / (D * D) - R);
                data[b] = c;
                lsum += (double)c;
                lcnt += 1;
            } else {                                             // an empty block keeps u's bytes
                v[b] = ux;
                v[nb + b] = uy;
                v[2 * nb + b] = uz;
                data[b] = inf;
            }
        }
    }
    lsum = workgroup_reduce<Add>(lsum, s_sum);
    lcnt = workgroup_reduce<Add>(lcnt, s_cnt);
    if (threadIdx.x == 0) {
        psum[blockIdx.x] = lsum;
        pcnt[blockIdx.x] = lcnt;
    }
}

// the partial slots 0 .. n-1 in a fixed order (finish_reduce)
__global__ __launch_bounds__(256) void k_cost_select_finish(const double *psum, const unsigned long long *pcnt,
                                                            unsigned n, double *sum, unsigned long long *cnt)
{
    __shared__ double s_sum[256];
    __shared__ unsigned long long s_cnt[256];
    const double a = finish_reduce<Add>(psum, n, s_sum);
    const unsigned long long b = finish_reduce<Add>(pcnt, n, s_cnt);
    if (threadIdx.x == 0) {
        *sum = a;
        *cnt = b;
    }
}

// ---- block-field smoothing and expansion ----

__device__ __forceinline__ float binomial(float lo, float mid, float hi)
{
    return (0.25f * lo + 0.5f * mid) + 0.25f * hi;
}

// one pass: B_z(B_y(B_x(src))) per channel; the intermediate values are recomputed per output, in the sweeps' order
__global__ __launch_bounds__(256) void k_block_field_smooth(const float *__restrict__ src, float *__restrict__ dst,
                                                            int nbx, int nby, int nbz)
{
    const size_t nb = (size_t)nbx * nby * nbz, total = 3 * nb;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t ch = i / nb, r = i - ch * nb;
        const int x = (int)(r % (size_t)nbx), y = (int)((r / (size_t)nbx) % (size_t)nby),
                  z = (int)(r / ((size_t)nbx * nby));
        const float *a = src + ch * nb;
        const int xs[3] = { max(x - 1, 0), x, min(x + 1, nbx - 1) };
        const int ys[3] = { max(y - 1, 0), y, min(y + 1, nby - 1) };
        const int zs[3] = { max(z - 1, 0), z, min(z + 1, nbz - 1) };
        float bz[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float by[3];
#pragma unroll
            for (int bq = 0; bq < 3; bq++) {
                const float *row = a + ((size_t)zs[c] * nby + (size_t)ys[bq]) * nbx;
                by[bq] = binomial(row[xs[0]], row[xs[1]], row[xs[2]]);
            }
            bz[c] = binomial(by[0], by[1], by[2]);
        }
        dst[i] = binomial(bz[0], bz[1], bz[2]);
    }
}

struct Lerp {
    int i0, i1;
    float f;
};

__device__ __forceinline__ Lerp lerp_of(int p, int nb)
{
    float t = ((float)p - 1.5f) * 0.25f;
    t = t < 0.0f ? 0.0f : t;
    t = t > (float)(nb - 1) ? (float)(nb - 1) : t;
    Lerp l;
    l.i0 = (int)floorf(t);
    l.i1 = min(l.i0 + 1, nb - 1);
    l.f = t - (float)l.i0;
    return l;
}

__device__ __forceinline__ float lerp(float f, float a, float b)
{
    return (1.0f - f) * a + f * b;
}

__global__ __launch_bounds__(256) void k_block_field_expand(const float *__restrict__ b, int nbx, int nby, int nbz,
                                                            float *__restrict__ w, int nx, int ny, int nz)
{
    const size_t nb = (size_t)nbx * nby * nbz, n = (size_t)nx * ny * nz, total = 3 * n;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t ch = i / n, r = i - ch * n;
        const int x = (int)(r % (size_t)nx), y = (int)((r / (size_t)nx) % (size_t)ny), z = (int)(r / ((size_t)nx * ny));
        const Lerp lx = lerp_of(x, nbx), ly = lerp_of(y, nby), lz = lerp_of(z, nbz);
        const float *a = b + ch * nb;
        const float *r00 = a + ((size_t)lz.i0 * nby + (size_t)ly.i0) * nbx;
        const float *r01 = a + ((size_t)lz.i0 * nby + (size_t)ly.i1) * nbx;
        const float *r10 = a + ((size_t)lz.i1 * nby + (size_t)ly.i0) * nbx;
        const float *r11 = a + ((size_t)lz.i1 * nby + (size_t)ly.i1) * nbx;
        const float x00 = lerp(lx.f, r00[lx.i0], r00[lx.i1]), x01 = lerp(lx.f, r01[lx.i0], r01[lx.i1]);
        const float x10 = lerp(lx.f, r10[lx.i0], r10[lx.i1]), x11 = lerp(lx.f, r11[lx.i0], r11[lx.i1]);
        const float y0 = lerp(ly.f, x00, x01), y1 = lerp(ly.f, x10, x11);
        w[i] = lerp(lz.f, y0, y1);
    }
}

} // namespace

// Launchers for sift3d_discrete.c, which has checked every argument (not exported from the library).

extern "C" int sift3d_cost_volume_launch(const float *d_F, const float *d_W, int nc, int nx, int ny, int nz,
                                         const float *d_VF, const float *d_VW, int radius, float *d_cost,
                                         void *stream)
{
    static const char fn[] = "sift3d_hip_cost_volume";
    CvArgs p;
    p.F = d_F; p.W = d_W; p.VF = d_VF; p.VW = d_VW;
    p.nc = nc;
    p.nx = nx; p.ny = ny; p.nz = nz;
    p.nbx = nx / 4; p.nby = ny / 4; p.nbz = nz / 4;
    p.cost = d_cost;
    if (!dispatch_int<1, SIFT3D_AMD_DISCRETE_MAX_RADIUS>(radius, [&](auto r) {
            using G = CvGeo<decltype(r)::value>;
            p.tiles_x = (p.nbx + G::TBX - 1) / G::TBX;
            p.tiles_y = (p.nby + G::TBY - 1) / G::TBY;
            const size_t tiles = (size_t)p.tiles_x * p.tiles_y * (size_t)((p.nbz + G::TBZ - 1) / G::TBZ);
            if (tiles > (size_t)INT_MAX) {
                p.tiles_x = 0;
                return;
            }
            hipLaunchKernelGGL(k_cost_volume<decltype(r)::value>, dim3((unsigned)tiles), dim3(64 * WAVES), 0,
                               (hipStream_t)stream, p);
        }))
        return launch_fail(fn, "radius out of range");
    if (!p.tiles_x)
        return launch_fail(fn, "the grid has too many blocks for one launch");
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

// d_work: SIFT3D_AMD_COST_SELECT_WORK_BYTES (the partials)
extern "C" int sift3d_cost_select_launch(const float *d_cost, int nbx, int nby, int nbz, int radius, const float *d_u,
                                         double theta, float *d_v, float *d_data, void *d_stats, void *d_work,
                                         void *stream)
{
    static const char fn[] = "sift3d_hip_cost_select";
    const size_t nb = (size_t)nbx * nby * nbz;
    const size_t groups = (nb + WAVES - 1) / WAVES;
    const unsigned grid = groups < SELECT_GRID ? (unsigned)groups : SELECT_GRID;
    double *psum = (double *)d_work;
    unsigned long long *pcnt = (unsigned long long *)((char *)d_work + SELECT_GRID * sizeof(double));
    hipStream_t st = (hipStream_t)stream;
    if (!dispatch_int<1, SIFT3D_AMD_DISCRETE_MAX_RADIUS>(radius, [&](auto r) {
            hipLaunchKernelGGL(k_cost_select<decltype(r)::value>, dim3(grid), dim3(64 * WAVES), 0, st, d_cost, nb, d_u,
                               theta, d_v, d_data, psum, pcnt);
        }))
        return launch_fail(fn, "radius out of range");
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cost_select_finish, dim3(1), dim3(256), 0, st, psum, pcnt, grid, (double *)d_stats,
                       (unsigned long long *)((char *)d_stats + 8));
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

extern "C" int sift3d_block_field_smooth_launch(const float *d_src, float *d_dst, int nbx, int nby, int nbz,
                                                void *stream)
{
    const size_t total = 3 * (size_t)nbx * nby * nbz;
    hipLaunchKernelGGL(k_block_field_smooth, dim3(grid_for(total, 1)), dim3(256), 0, (hipStream_t)stream, d_src, d_dst,
                       nbx, nby, nbz);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

extern "C" int sift3d_block_field_expand_launch(const float *d_b, int nbx, int nby, int nbz, float *d_w, int nx,
                                                int ny, int nz, void *stream)
{
    const size_t total = 3 * (size_t)nx * ny * nz;
    hipLaunchKernelGGL(k_block_field_expand, dim3(grid_for(total, 1)), dim3(256), 0, (hipStream_t)stream, d_b, nbx,
                       nby, nbz, d_w, nx, ny, nz);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}
