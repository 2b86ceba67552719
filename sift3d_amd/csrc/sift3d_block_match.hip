// sift3d_block_match.hip -- block matching: every 4^3 block of the fixed volume finds its best-correlated position
// in the warped moving volume inside a (2R+1)^3 search cube (contract: include/sift3d_amd.h, "Block matching").
//
// Mapping.  One workgroup (4 waves) takes a tile of TBX x TBY x TBZ adjacent blocks and stages the W neighbourhood
// of the whole tile in LDS once: (4 TBX + 2R) x (4 TBY + 2R) x (4 TBZ + 2R) floats, 44.8 KB at R = 6 for the default
// 4 x 2 x 2 tile.  A voxel that is off the grid or out of V_W is staged as NaN: the contract's inputs are finite, so a
// NaN in a candidate's sums means exactly "a voxel of the shifted block is off the grid or masked out", and the
// candidate then fails vW > sWW 2^-40 with no validity array and no extra LDS read.
// A wave takes one block at a time.  Its 64 F values are fetched one per lane, spread by v_readlane (wave-uniform,
// so they live in scalar registers) and promoted to double once.  Then ONE LANE PER CANDIDATE: lane l walks candidates
// k = l, l + 64, ... and sums the block's 64 voxels in the contract's order i = 0 .. 63, so no cross-lane reduction
// touches a sum and the bits are the restatement's.  Per voxel: one ds_read_b32 at an immediate offset (R is a
// template parameter, the LDS strides are constants), one f32 -> f64 convert, one double add and two double FMAs.  The
// FMAs are written as fma(): both products are of two floats and exact in double, so fused or not gives the same
// bits (the unit is compiled with contraction off like every other).  Lanes with consecutive k have consecutive dx
// and read consecutive LDS words.
// The winner is reduced across the wave with the contract's total order (cc, then |d|^2, then k).  The six
// neighbours of the winner are then RECOMPUTED by lanes 0 .. 5 (one more trip through the 64 voxels) instead of
// keeping (2R+1)^3 doubles per wave in LDS: 70 KB at R = 6 for four waves, which would leave one workgroup per CU.
#include "sift3d_kernels_common.h"

#include <climits>

// the tile of blocks per workgroup: a build option for profiles/microbench/block_match_rate.py
#ifndef SIFT3D_BM_TBX
#define SIFT3D_BM_TBX 4
#endif
#ifndef SIFT3D_BM_TBY
#define SIFT3D_BM_TBY 2
#endif
#ifndef SIFT3D_BM_TBZ
#define SIFT3D_BM_TBZ 2
#endif
// candidates a lane sums at once (independent chains that share the promotion of F): also a build option
#ifndef SIFT3D_BM_J
#define SIFT3D_BM_J 1
#endif
// 0: let the compiler hoist the promotion of the block's 64 F values out of the candidate loop (128 VGPRs)
#ifndef SIFT3D_BM_OPAQUE
#define SIFT3D_BM_OPAQUE 1
#endif

namespace {

constexpr int TBX = SIFT3D_BM_TBX, TBY = SIFT3D_BM_TBY, TBZ = SIFT3D_BM_TBZ;
constexpr int TILE_BLOCKS = TBX * TBY * TBZ;
constexpr int WAVES = 4;

struct BmArgs {
    const float *F, *W, *VF, *VW;
    int nx, ny, nz;
    int nbx, nby, nbz;
    int tiles_x, tiles_y;
    float *disp, *cc;
    double *var;
};

template <int R> struct BmGeo {
    static constexpr int D = 2 * R + 1, NCAND = D * D * D;
    static constexpr int SX = 4 * TBX + 2 * R, SY = 4 * TBY + 2 * R, SZ = 4 * TBZ + 2 * R;
    static constexpr int STAGED = SX * SY * SZ;
};

// the three sums of J candidates at once over the block's 64 voxels, i ascending, from 0; w[j]: the first voxel of
// candidate j's shifted block.  ff: the block's F, wave-uniform (scalar registers); its promotion to double is shared
// by the J candidates, whose chains are independent of one another.
template <int R, int J>
__device__ __forceinline__ void bm_sums(const float *const (&w)[J], const float (&ff)[64], double (&sW)[J],
                                        double (&sWW)[J], double (&sFW)[J])
{
    constexpr int SX = BmGeo<R>::SX, SY = BmGeo<R>::SY;
#pragma unroll
    for (int j = 0; j < J; j++)
        sW[j] = sWW[j] = sFW[j] = 0.0;
#pragma unroll
    for (int z = 0; z < 4; z++)
#pragma unroll
        for (int y = 0; y < 4; y++)
#pragma unroll
            for (int x = 0; x < 4; x++) {
                // the empty asm keeps the scalar float opaque, so that the compiler does not hoist 64 promoted doubles
                // (128 VGPRs) out of the candidate loop; the convert is shared by the J candidates instead
                float fs = ff[(z * 4 + y) * 4 + x];
#if SIFT3D_BM_OPAQUE
                asm volatile("" : "+s"(fs));
#endif
                const double f = (double)fs;
#pragma unroll
                for (int j = 0; j < J; j++) {
                    const double v = (double)w[j][(z * SY + y) * SX + x];
                    sW[j] = sW[j] + v;
                    sWW[j] = fma(v, v, sWW[j]);              // v * v is exact: fused == unfused
                    sFW[j] = fma(f, v, sFW[j]);              // so is a product of two floats
                }
            }
}

// cc of a candidate from its sums, or -1 where it is not valid (a NaN sum: off the grid or masked; flat W)
__device__ __forceinline__ double bm_score(double sF, double vF, double sW, double sWW, double sFW)
{
    const double vW = sWW - (sW * sW) / 64.0;
    if (!(vW > sWW * 0x1p-40))
        return -1.0;
    const double c = sFW - (sF * sW) / 64.0;
    return (c * c) / (vF * vW);
}

struct Best {
    double cc;
    int d2, k;
};

// the contract's choice: greater cc, then smaller |d|^2, then smaller k; an invalid entry is (-1, INT_MAX, INT_MAX)
__device__ __forceinline__ bool bm_better(const Best &a, const Best &b)
{
    return a.cc > b.cc || (a.cc == b.cc && (a.d2 < b.d2 || (a.d2 == b.d2 && a.k < b.k)));
}

template <int R> __global__ __launch_bounds__(64 * WAVES) void k_block_match(const BmArgs p)
{
    using G = BmGeo<R>;
    constexpr int D = G::D, SX = G::SX, SY = G::SY;
    // candidates per lane and pass: no more than the cube gives 64 lanes to do
    constexpr int J = G::NCAND >= 64 * SIFT3D_BM_J ? SIFT3D_BM_J : (G::NCAND >= 128 ? 2 : 1);
    __shared__ __attribute__((aligned(16))) float s_w[G::STAGED];

    const int tile = blockIdx.x;
    const int tx = tile % p.tiles_x, ty = (tile / p.tiles_x) % p.tiles_y, tz = tile / (p.tiles_x * p.tiles_y);
    const int bx0 = tx * TBX, by0 = ty * TBY, bz0 = tz * TBZ;
    const size_t sx = (size_t)p.nx, plane = sx * (size_t)p.ny;

    // stage W for the tile: voxel (4 bx0 - R + x, ...) at s_w[(z SY + y) SX + x]
    {
        const int ox = 4 * bx0 - R, oy = 4 * by0 - R, oz = 4 * bz0 - R;
        for (int i = threadIdx.x; i < G::STAGED; i += 64 * WAVES) {
            const int x = i % SX, y = (i / SX) % SY, z = i / (SX * SY);
            const int gx = ox + x, gy = oy + y, gz = oz + z;
            float v = __builtin_nanf("");
            if (gx >= 0 && gx < p.nx && gy >= 0 && gy < p.ny && gz >= 0 && gz < p.nz) {
                const size_t g = (size_t)gz * plane + (size_t)gy * sx + (size_t)gx;
                if (!p.VW || p.VW[g] >= 0.5f)
                    v = p.W[g];
            }
            s_w[i] = v;
        }
    }
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int b = wave; b < TILE_BLOCKS; b += WAVES) {
        const int lx = b % TBX, ly = (b / TBX) % TBY, lz = b / (TBX * TBY);
        const int bx = bx0 + lx, by = by0 + ly, bz = bz0 + lz;
        if (bx >= p.nbx || by >= p.nby || bz >= p.nbz)
            continue;                                        // wave-uniform
        const size_t out = ((size_t)bz * p.nby + (size_t)by) * p.nbx + (size_t)bx;
        const size_t nb = (size_t)p.nbx * p.nby * p.nbz;

        // the block's F: lane i holds voxel i = x + 4 y + 16 z
        float ff[64];
        bool in_mask;
        {
            const size_t g = (size_t)(4 * bz + (lane >> 4)) * plane + (size_t)(4 * by + ((lane >> 2) & 3)) * sx +
                             (size_t)(4 * bx + (lane & 3));
            const float f = p.F[g];
            in_mask = !p.VF || p.VF[g] >= 0.5f;
#pragma unroll
            for (int i = 0; i < 64; i++)
                ff[i] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(f), i));
        }
        double sF = 0.0, sFF = 0.0;
#pragma unroll
        for (int i = 0; i < 64; i++) {
            const double fi = (double)ff[i];
            sF = sF + fi;
            sFF = fma(fi, fi, sFF);
        }
        const double vF = sFF - (sF * sF) / 64.0;
        const bool block_ok = __ballot(in_mask) == ~0ull && vF > sFF * 0x1p-40;

        Best best = { -1.0, INT_MAX, INT_MAX };
        // the block's own position in the staged tile, at displacement 0
        const float *w0 = s_w + ((4 * lz + R) * SY + (4 * ly + R)) * SX + (4 * lx + R);
        if (block_ok) {
            for (int k0 = lane; k0 < G::NCAND; k0 += 64 * J) {
                const float *w[J];
                int kk[J];
#pragma unroll
                for (int j = 0; j < J; j++) {                // a lane past the last candidate repeats it
                    kk[j] = k0 + 64 * j < G::NCAND ? k0 + 64 * j : G::NCAND - 1;
                    w[j] = w0 + ((kk[j] / (D * D) - R) * SY + ((kk[j] / D) % D - R)) * SX + (kk[j] % D - R);
                }
                double sW[J], sWW[J], sFW[J];
                bm_sums<R, J>(w, ff, sW, sWW, sFW);
#pragma unroll
                for (int j = 0; j < J; j++) {
                    const int dx = kk[j] % D - R, dy = (kk[j] / D) % D - R, dz = kk[j] / (D * D) - R;
                    const Best c = { bm_score(sF, vF, sW[j], sWW[j], sFW[j]), dx * dx + dy * dy + dz * dz, kk[j] };
                    if (c.cc >= 0.0 && bm_better(c, best))
                        best = c;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const Best other = { __shfl_xor(best.cc, o, 64), __shfl_xor(best.d2, o, 64),
                                     __shfl_xor(best.k, o, 64) };
                if (bm_better(other, best))
                    best = other;
            }
        }
        if (!(best.cc >= 0.0)) {                             // invalid block (wave-uniform)
            if (lane == 0) {
                p.disp[out] = 0.0f;
                p.disp[nb + out] = 0.0f;
                p.disp[2 * nb + out] = 0.0f;
                p.cc[out] = -1.0f;
                p.var[out] = 0.0;
            }
            continue;
        }
        const int d[3] = { best.k % D - R, (best.k / D) % D - R, best.k / (D * D) - R };

        // the winner's six neighbours, lanes 0 .. 5: axis lane >> 1, side -1 (even lane) or +1 (odd)
        double ncc = -1.0;
        if (lane < 6) {
            int e[3] = { d[0], d[1], d[2] };
            const int a = lane >> 1;
            e[a] += (lane & 1) ? 1 : -1;
            if (e[a] >= -R && e[a] <= R) {
                const float *const w[1] = { w0 + (e[2] * SY + e[1]) * SX + e[0] };
                double sW[1], sWW[1], sFW[1];
                bm_sums<R, 1>(w, ff, sW, sWW, sFW);
                ncc = bm_score(sF, vF, sW[0], sWW[0], sFW[0]);
            }
        }
        float disp[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double cm = __shfl(ncc, 2 * a, 64), cp = __shfl(ncc, 2 * a + 1, 64);
            double o = 0.0;
            if (cm >= 0.0 && cp >= 0.0) {
                const double den = (cm - 2.0 * best.cc) + cp;
                if (den < 0.0) {
                    o = 0.5 * (cm - cp) / den;
                    o = o < -0.5 ? -0.5 : (o > 0.5 ? 0.5 : o);
                }
            }
            disp[a] = (float)((double)d[a] + o);
        }
        if (lane == 0) {
            p.disp[out] = disp[0];
            p.disp[nb + out] = disp[1];
            p.disp[2 * nb + out] = disp[2];
            p.cc[out] = (float)best.cc;
            p.var[out] = vF;
        }
    }
}

__global__ __launch_bounds__(256) void k_block_fill(float *__restrict__ dst, size_t n, float v)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        dst[i] = v;
}

} // namespace

// unchecked (sift3d_hip_block_match in sift3d_block_fit.c checks): dims >= 4, 1 <= radius <= 6
extern "C" int sift3d_block_match_launch(const float *d_F, int nx, int ny, int nz, const float *d_W,
                                         const float *d_VF, const float *d_VW, int radius, float *d_disp,
                                         float *d_cc, double *d_var, void *stream)
{
    static const char fn[] = "sift3d_hip_block_match";
    BmArgs p;
    p.F = d_F; p.W = d_W; p.VF = d_VF; p.VW = d_VW;
    p.nx = nx; p.ny = ny; p.nz = nz;
    p.nbx = nx / 4; p.nby = ny / 4; p.nbz = nz / 4;
    p.tiles_x = (p.nbx + TBX - 1) / TBX;
    p.tiles_y = (p.nby + TBY - 1) / TBY;
    p.disp = d_disp; p.cc = d_cc; p.var = d_var;
    const size_t tiles = (size_t)p.tiles_x * p.tiles_y * (size_t)((p.nbz + TBZ - 1) / TBZ);
    if (tiles > (size_t)INT_MAX)
        return launch_fail(fn, "the grid has too many blocks for one launch");
    if (!dispatch_int<1, SIFT3D_AMD_BLOCK_MAX_RADIUS>(radius, [&](auto r) {
            constexpr int R = decltype(r)::value;
            hipLaunchKernelGGL(k_block_match<R>, dim3((unsigned)tiles), dim3(64 * WAVES), 0, (hipStream_t)stream, p);
        }))
        return launch_fail(fn, "radius out of range");
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

extern "C" int sift3d_block_fill_launch(float *d_dst, size_t n, float value, void *stream)
{
    if (n == 0)
        return SIFT3D_SUCCESS;
    hipLaunchKernelGGL(k_block_fill, dim3(grid_for(n, 4)), dim3(256), 0, (hipStream_t)stream, d_dst, n, value);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}
