// sift3d_warp.hip -- affine resampling of a volume (the last step of registration).
//
// Upstream SIFT3D's registration tool resamples the moving image into the fixed image's grid once
// the affine is known.  This is that step on the device.  The arithmetic is fixed so that a
// restatement in numpy reproduces it bit for bit (tests/test_warp.py):
//
//   A (3 x 4, row-major) is a PULL map: output voxel (x, y, z) reads the source at
//     q_d = A[d][0]*x + ((A[d][1]*y + A[d][2]*z) + A[d][3])      (double, this order, no contraction)
//   inside  : 0 <= q_d <= n_d - 1 on every axis (a NaN is outside); outside voxels get `fill`;
//   linear  : i = floor(q), f = (float)(q - i), j = min(i + 1, n - 1), lerp(a, b, f) = a + f*(b - a)
//             in float, along x for the four (y, z) corner rows, then along y, then along z;
//   nearest : the value at floor(q + 0.5).
//
// 4 B read + 4 B written per output voxel algorithmically; in fact 4 gathered 8-byte loads (linear: one per
// (y, z) corner row, the x pair) or 1 dword load (nearest) per voxel, most of them L1 / L2 hits.  The time
// follows the gather instructions and how many distinct addresses each carries, not HBM bytes
// (profiles/microbench/warp_rate_mi355x.txt).  Layout:
//   - a lane gathers for 4 x outputs 16 apart, so that neighbouring lanes read neighbouring source
//     addresses, and after an exchange through LDS writes 4 consecutive x outputs with one 16-byte store
//     (scalar stores for the row tail when ox % 4 != 0, where the rows are not 16-byte aligned);
//   - a 256-lane workgroup makes a 64 x 4 x 4 tile, compact in 3-D so that the source footprint of a
//     rotated tile is small and stays in L1 / L2 (a long x-row tile rotated about z or y would sweep
//     a long diagonal of the source);
//   - tiles are numbered x fastest, and blocks are remapped so that each XCD (blocks b, b + 8, ...
//     share one) works on a contiguous run of tile numbers -- neighbouring tiles, overlapping source
//     footprints, the same L2.
#include "sift3d_kernels_common.h"

#include <cmath>

namespace {

constexpr int TX = 64, TY = 4, TZ = 4;          // outputs per tile: 16 lanes x 4 in x, 4 rows, 4 planes
constexpr int NXCD = 8;
constexpr unsigned MAX_GRID = 1u << 20;          // blocks per pass over the tiles

struct WarpArgs {
    double a[12];
    const float *src;
    float *dst;
    int nx, ny, nz, ox, oy, oz;
    int tiles_x, tiles_y;
    unsigned ntiles;                             // < 2^32 (checked at launch)
    float fill;
    int vec;                                     // 16-byte stores (ox % 4 == 0, dst 16-byte aligned)
};

// block b of a pass of n blocks -> tile number within the pass: the blocks of one XCD (b % 8) get
// a contiguous run of tile numbers (bijective for any n; cdna_hip_programming T1)
__device__ __forceinline__ unsigned xcd_swizzle(unsigned b, unsigned n)
{
    const unsigned g = b % NXCD, k = b / NXCD, q = n / NXCD, r = n % NXCD;
    return g * q + (g < r ? g : r) + k;
}

__device__ __forceinline__ float lerp(float a, float b, float f) { return a + f * (b - a); }

// two neighbouring source elements with one 8-byte load (4-byte aligned: global_load_dwordx2)
typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));

// Branch-free: an outside sample reads voxel 0 and is replaced by `fill` at the end, so that the loads of
// all four outputs of a lane are in flight together instead of one output's behind each branch.
// LINEAR == 2 is linear mode for nx >= 2: each (y, z) corner row gives the pair (ix, jx) with one 8-byte load
// at min(ix, nx - 2) -- the same two values as two single loads, half the load instructions.  LINEAR == 1
// (nx == 1) loads them singly.
template <int LINEAR>
__device__ __forceinline__ float sample(const WarpArgs &p, double qx, double qy, double qz)
{
    // `&`, not `&&`: six compares and one mask, no branches (a NaN fails every compare)
    const bool in = (qx >= 0.0) & (qx <= (double)(p.nx - 1)) & (qy >= 0.0) & (qy <= (double)(p.ny - 1)) &
                    (qz >= 0.0) & (qz <= (double)(p.nz - 1));
    qx = in ? qx : 0.0;
    qy = in ? qy : 0.0;
    qz = in ? qz : 0.0;
    const size_t sx = (size_t)p.nx, sxy = (size_t)p.nx * (size_t)p.ny;
    const float *s = p.src;
    float v;
    if (!LINEAR) {
        const int ix = (int)floor(qx + 0.5), iy = (int)floor(qy + 0.5), iz = (int)floor(qz + 0.5);
        v = s[(size_t)iz * sxy + (size_t)iy * sx + (size_t)ix];
    } else {
        const double fx0 = floor(qx), fy0 = floor(qy), fz0 = floor(qz);
        const int ix = (int)fx0, iy = (int)fy0, iz = (int)fz0;
        const float fx = (float)(qx - fx0), fy = (float)(qy - fy0), fz = (float)(qz - fz0);
        const int jy = min(iy + 1, p.ny - 1), jz = min(iz + 1, p.nz - 1);
        const size_t r00 = (size_t)iz * sxy + (size_t)iy * sx, r10 = (size_t)iz * sxy + (size_t)jy * sx;
        const size_t r01 = (size_t)jz * sxy + (size_t)iy * sx, r11 = (size_t)jz * sxy + (size_t)jy * sx;
        float a00, b00, a10, b10, a01, b01, a11, b11;                       // values at (ix, jx) per corner row
        if (LINEAR == 2) {
            const int bx = min(ix, p.nx - 2);                                // ix == nx - 1: jx == ix, both = .y
            const bool hi = ix != bx;
            const f32x2u w00 = *reinterpret_cast<const f32x2u *>(s + r00 + bx);
            const f32x2u w10 = *reinterpret_cast<const f32x2u *>(s + r10 + bx);
            const f32x2u w01 = *reinterpret_cast<const f32x2u *>(s + r01 + bx);
            const f32x2u w11 = *reinterpret_cast<const f32x2u *>(s + r11 + bx);
            a00 = hi ? w00.y : w00.x; b00 = w00.y;
            a10 = hi ? w10.y : w10.x; b10 = w10.y;
            a01 = hi ? w01.y : w01.x; b01 = w01.y;
            a11 = hi ? w11.y : w11.x; b11 = w11.y;
        } else {
            const int jx = min(ix + 1, p.nx - 1);
            a00 = s[r00 + ix]; b00 = s[r00 + jx];
            a10 = s[r10 + ix]; b10 = s[r10 + jx];
            a01 = s[r01 + ix]; b01 = s[r01 + jx];
            a11 = s[r11 + ix]; b11 = s[r11 + jx];
        }
        const float c00 = lerp(a00, b00, fx), c10 = lerp(a10, b10, fx);
        const float c01 = lerp(a01, b01, fx), c11 = lerp(a11, b11, fx);
        v = lerp(lerp(c00, c10, fy), lerp(c01, c11, fy), fz);
    }
    return in ? v : p.fill;
}

template <int LINEAR>
__global__ __launch_bounds__(256) void k_warp_affine(const WarpArgs p)
{
    // A lane computes x = x_tile + lx + 16 k (k = 0..3): the 16 lanes of a row gather from neighbouring source
    // addresses in each load instruction (lanes 4 x apart would make every lane a request of its own).  The
    // values are then regrouped through LDS so that the lane stores x_tile + 4 lx .. + 3 with one 16-byte store.
    __shared__ float4 xch[256];
    float *xs = reinterpret_cast<float *>(xch) + (threadIdx.x & ~15) * 4;    // this row's 64 outputs
    const int lx = threadIdx.x & 15, ly = (threadIdx.x >> 4) & 3, lz = threadIdx.x >> 6;
    for (unsigned base = 0; base < p.ntiles; base += gridDim.x) {
        const unsigned n = min(p.ntiles - base, gridDim.x);
        if (blockIdx.x >= n)
            return;                                                          // uniform over the block
        const unsigned t = base + xcd_swizzle(blockIdx.x, n);
        const unsigned tyz = t / (unsigned)p.tiles_x;
        const int tx = (int)(t - tyz * (unsigned)p.tiles_x);
        const int ty = (int)(tyz % (unsigned)p.tiles_y), tz = (int)(tyz / (unsigned)p.tiles_y);
        const int xt = tx * TX, y = ty * TY + ly, z = tz * TZ + lz;
        // once per row: r_d = (A[d][1] y + A[d][2] z) + A[d][3]  (rows past the grid are computed and not
        // stored: every lane takes part in the exchange; sampling is branch-free and reads inside the source)
        const double yd = (double)y, zd = (double)z;
        const double rx = (p.a[1] * yd + p.a[2] * zd) + p.a[3];
        const double ry = (p.a[5] * yd + p.a[6] * zd) + p.a[7];
        const double rz = (p.a[9] * yd + p.a[10] * zd) + p.a[11];
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double xd = (double)(xt + lx + 16 * k);
            v[k] = sample<LINEAR>(p, p.a[0] * xd + rx, p.a[4] * xd + ry, p.a[8] * xd + rz);
        }
        __syncthreads();                                                     // previous tile's reads done
#pragma unroll
        for (int k = 0; k < 4; k++)
            xs[lx + 16 * k] = v[k];
        __syncthreads();
        const float4 w = xch[threadIdx.x];
        const int x0 = xt + 4 * lx;
        if (x0 >= p.ox || y >= p.oy || z >= p.oz)
            continue;
        float *out = p.dst + ((size_t)z * (size_t)p.oy + (size_t)y) * (size_t)p.ox + (size_t)x0;
        if (p.vec) {
            st4(out, w);
        } else {
            const float o[4] = {w.x, w.y, w.z, w.w};
            const int m = min(4, p.ox - x0);
#pragma nounroll
            for (int k = 0; k < m; k++)
                out[k] = o[k];
        }
    }
}

int warp_fail(const char *why)
{
    snprintf(g_err, sizeof(g_err), "sift3d_hip_warp_affine: %s", why);
    fprintf(stderr, "sift3d_amd: %s\n", g_err);
    return SIFT3D_FAILURE;
}

// ---- thin-plate spline: q(p) = affine(p) + (double) s(p), s = sum_i w_i phi(|p - c_i|) ------------------------
// (contract: include/sift3d_amd.h, "Thin-plate spline").  The radial sum is compute-bound: per voxel-point
// 3 differences, 3 squares, 2 adds, a correctly rounded sqrt and 3 multiply-adds, all float, unfused.
//   - a lane keeps TPS_K voxels of one (x, y) column in flight (z = z_tile .. + TPS_K - 1): dx, dy and
//     dx*dx + dy*dy are the same for all of them, so each point costs 5 instructions per lane plus per voxel
//     dz, dz*dz, the add, the sqrt and the 3 multiply-adds; the per-voxel part runs on pairs of voxels with
//     packed f32 arithmetic (v_pk_add_f32 / v_pk_mul_f32), everything but the sqrt;
//   - the points are wave-uniform: the loop reads them through the constant address space, so they come
//     in by scalar loads (one 32-byte record per point) and every lane uses the same c_i, w_i;
//   - a wave is 64 consecutive x of one row, so that the gathers of neighbouring lanes touch neighbouring
//     source addresses and each plane's results leave with one coalesced 256-byte store;
//   - a 256-lane workgroup makes a 64 x 4 x TPS_K tile.  Tiles are numbered x fastest, then y, then z, and a
//     launch covers a contiguous range of them: whole z-slabs (z-ranges) whenever one slab fits the launch
//     budget (tps_tiles_per_launch).
// The device layout (sift3d_amd_tps_pack) holds per point {cx, cy, cz, 0, -wx, -wy, -wz, 0}: the sign of
// phi(r) = -r is folded into the weights, and s + (-w) * r is w * (-r) added to s, bit for bit.
constexpr int TPS_K = 8;                          // voxels per lane, along z
constexpr int TPS_TX = 64, TPS_TY = 4;            // a wave per row, 4 rows per workgroup
constexpr int TPS_TILE = TPS_TX * TPS_TY * TPS_K;
constexpr unsigned TPS_MAX_GRID = 1u << 24;       // blocks per launch
// launch budget: no launch is estimated above TPS_BUDGET_S at TPS_S_PER_VOXEL_POINT machine-wide (measured on an
// MI355X at 512^3: 0.54 ps for m = 256 .. 4096, profiles/microbench/tps_rate_mi355x.txt; rounded up)
constexpr double TPS_BUDGET_S = 50e-3;
constexpr double TPS_S_PER_VOXEL_POINT = 0.60e-12;

struct TpsArgs {
    WarpArgs w;                                  // the affine, the source, the grids, fill (w.vec unused)
    const float *tps;                            // 8 floats per point (sift3d_amd_tps_pack)
    int m;
    int tiles_x, tiles_y;
    unsigned t0;                                 // this launch: tiles t0 .. t0 + gridDim.x - 1
};

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(4))) float *tps_cptr;    // constant address space: scalar loads

template <int LINEAR>
__global__ __launch_bounds__(256) void k_warp_tps(const TpsArgs p)
{
    const unsigned t = p.t0 + blockIdx.x;
    const unsigned tyz = t / (unsigned)p.tiles_x;
    const int tx = (int)(t - tyz * (unsigned)p.tiles_x);
    const int ty = (int)(tyz % (unsigned)p.tiles_y), tz = (int)(tyz / (unsigned)p.tiles_y);
    const int x = tx * TPS_TX + (int)(threadIdx.x & 63), y = ty * TPS_TY + (int)(threadIdx.x >> 6);
    const int z0 = tz * TPS_K;
    // lanes past the grid compute (the source reads stay inside it: sample<> is branch-free) and do not store
    const float xf = (float)x, yf = (float)y;
    f32x2 zf[TPS_K / 2], sx[TPS_K / 2], sy[TPS_K / 2], sz[TPS_K / 2];
#pragma unroll
    for (int k = 0; k < TPS_K / 2; k++) {
        zf[k] = f32x2{(float)(z0 + 2 * k), (float)(z0 + 2 * k + 1)};
        sx[k] = sy[k] = sz[k] = f32x2{0.0f, 0.0f};
    }
    const tps_cptr pt = (tps_cptr)p.tps;
#pragma unroll 2
    for (int i = 0; i < p.m; i++) {
        const tps_cptr q = pt + SIFT3D_AMD_TPS_FLOATS * i;
        const float cx = q[0], cy = q[1], cz = q[2];
        const float wx = q[4], wy = q[5], wz = q[6];                    // -w_i: the sign of phi folded in
        const float dx = xf - cx, dy = yf - cy;
        const float hxy = dx * dx + dy * dy;
#pragma unroll
        for (int k = 0; k < TPS_K / 2; k++) {
            const f32x2 dz = zf[k] - cz;
            const f32x2 r2 = hxy + dz * dz;
            const f32x2 r = f32x2{sqrtf(r2.x), sqrtf(r2.y)};           // correctly rounded (no -ffast-math)
            sx[k] = sx[k] + wx * r;
            sy[k] = sy[k] + wy * r;
            sz[k] = sz[k] + wz * r;
        }
    }
    // affine part once per column: r_d = (A[d][1] y + A[d][2] z) + A[d][3] depends on z, so it is per voxel
    const double xd = (double)x, yd = (double)y;
    const bool col = x < p.w.ox && y < p.w.oy;
    float *out = p.w.dst + ((size_t)z0 * (size_t)p.w.oy + (size_t)y) * (size_t)p.w.ox + (size_t)x;
    const size_t plane = (size_t)p.w.oy * (size_t)p.w.ox;
#pragma unroll
    for (int k = 0; k < TPS_K; k++) {
        const double zd = (double)(z0 + k);
        const float rx = (k & 1) ? sx[k / 2].y : sx[k / 2].x;
        const float ry = (k & 1) ? sy[k / 2].y : sy[k / 2].x;
        const float rz = (k & 1) ? sz[k / 2].y : sz[k / 2].x;
        const double qx = p.w.a[0] * xd + ((p.w.a[1] * yd + p.w.a[2] * zd) + p.w.a[3]) + (double)rx;
        const double qy = p.w.a[4] * xd + ((p.w.a[5] * yd + p.w.a[6] * zd) + p.w.a[7]) + (double)ry;
        const double qz = p.w.a[8] * xd + ((p.w.a[9] * yd + p.w.a[10] * zd) + p.w.a[11]) + (double)rz;
        const float v = sample<LINEAR>(p.w, qx, qy, qz);
        if (col && z0 + k < p.w.oz)
            out[(size_t)k * plane] = v;
    }
}

int tps_fail(const char *why)
{
    snprintf(g_err, sizeof(g_err), "sift3d_hip_warp_tps: %s", why);
    fprintf(stderr, "sift3d_amd: %s\n", g_err);
    return SIFT3D_FAILURE;
}

// tiles per launch: as many as the budget allows (at least one), rounded down to whole z-slabs when a slab fits
unsigned long long tps_tiles_per_launch(int ox, int oy, int m)
{
    const unsigned long long slab = (unsigned long long)((ox + TPS_TX - 1) / TPS_TX) * ((oy + TPS_TY - 1) / TPS_TY);
    const double per_tile = (double)TPS_TILE * (double)m * TPS_S_PER_VOXEL_POINT;
    double n = floor(TPS_BUDGET_S / per_tile);
    if (n > (double)TPS_MAX_GRID)
        n = (double)TPS_MAX_GRID;
    unsigned long long c = n < 1.0 ? 1ull : (unsigned long long)n;
    if (c >= slab)
        c -= c % slab;
    return c;
}

} // namespace

extern "C" {

int sift3d_hip_warp_affine(const float *d_src, int nx, int ny, int nz, float *d_dst, int ox, int oy, int oz,
                           const double *A, int interp, float fill, void *stream)
{
    if (!d_src || !d_dst || !A)
        return warp_fail("NULL argument");
    if (nx <= 0 || ny <= 0 || nz <= 0 || ox <= 0 || oy <= 0 || oz <= 0)
        return warp_fail("dimensions must be positive");
    if (interp != SIFT3D_AMD_INTERP_NEAREST && interp != SIFT3D_AMD_INTERP_LINEAR)
        return warp_fail("unknown interpolation mode");
    for (int i = 0; i < 12; i++)
        if (!std::isfinite(A[i]))
            return warp_fail("the affine map is not finite");
    {
        const uintptr_t s0 = (uintptr_t)d_src, d0 = (uintptr_t)d_dst;
        const uintptr_t s1 = s0 + (size_t)nx * ny * nz * sizeof(float), d1 = d0 + (size_t)ox * oy * oz * sizeof(float);
        if (s0 < d1 && d0 < s1)
            return warp_fail("source and destination overlap");
    }
    WarpArgs p;
    for (int i = 0; i < 12; i++)
        p.a[i] = A[i];
    p.src = d_src;
    p.dst = d_dst;
    p.nx = nx; p.ny = ny; p.nz = nz;
    p.ox = ox; p.oy = oy; p.oz = oz;
    p.tiles_x = (ox + TX - 1) / TX;
    p.tiles_y = (oy + TY - 1) / TY;
    {
        const unsigned long long nt = (unsigned long long)p.tiles_x * p.tiles_y * ((oz + TZ - 1) / TZ);
        if (nt > 0xffffffffull - MAX_GRID)
            return warp_fail("output grid too large");
        p.ntiles = (unsigned)nt;
    }
    p.fill = fill;
    p.vec = (ox % 4 == 0) && !((uintptr_t)d_dst & 15);
    const unsigned grid = p.ntiles < MAX_GRID ? (unsigned)p.ntiles : MAX_GRID;
    hipStream_t st = (hipStream_t)stream;
    const dim3 g(grid), b(256);
    void (*k)(const WarpArgs) = interp == SIFT3D_AMD_INTERP_NEAREST ? k_warp_affine<0>
                                : nx >= 2                          ? k_warp_affine<2>
                                                                   : k_warp_affine<1>;
    hipLaunchKernelGGL(k, g, b, 0, st, p);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

int sift3d_hip_warp_tps_launches(int ox, int oy, int oz, int m)
{
    if (ox <= 0 || oy <= 0 || oz <= 0 || m < 1 || m > SIFT3D_AMD_TPS_MAX_POINTS)
        return -1;
    const unsigned long long nt = (unsigned long long)((ox + TPS_TX - 1) / TPS_TX) * ((oy + TPS_TY - 1) / TPS_TY) *
                                  ((oz + TPS_K - 1) / TPS_K);
    const unsigned long long c = tps_tiles_per_launch(ox, oy, m);
    const unsigned long long n = (nt + c - 1) / c;
    return n > 0x7fffffffull ? -1 : (int)n;
}

int sift3d_hip_warp_tps(const float *d_src, int nx, int ny, int nz, float *d_dst, int ox, int oy, int oz,
                        const double *A, const float *d_tps, int m, int interp, float fill, void *stream)
{
    if (!d_src || !d_dst || !A || !d_tps)
        return tps_fail("NULL argument");
    if (nx <= 0 || ny <= 0 || nz <= 0 || ox <= 0 || oy <= 0 || oz <= 0)
        return tps_fail("dimensions must be positive");
    if (m < 1 || m > SIFT3D_AMD_TPS_MAX_POINTS)
        return tps_fail("the number of control points must be in [1, SIFT3D_AMD_TPS_MAX_POINTS]");
    if (interp != SIFT3D_AMD_INTERP_NEAREST && interp != SIFT3D_AMD_INTERP_LINEAR)
        return tps_fail("unknown interpolation mode");
    for (int i = 0; i < 12; i++)
        if (!std::isfinite(A[i]))
            return tps_fail("the affine map is not finite");
    if ((uintptr_t)d_tps & 15)
        return tps_fail("the control point records are not 16-byte aligned");
    {
        const uintptr_t s0 = (uintptr_t)d_src, d0 = (uintptr_t)d_dst, c0 = (uintptr_t)d_tps;
        const uintptr_t s1 = s0 + (size_t)nx * ny * nz * sizeof(float), d1 = d0 + (size_t)ox * oy * oz * sizeof(float);
        const uintptr_t c1 = c0 + (size_t)m * SIFT3D_AMD_TPS_FLOATS * sizeof(float);
        if ((s0 < d1 && d0 < s1) || (c0 < d1 && d0 < c1))
            return tps_fail("the destination overlaps the source or the control points");
    }
    TpsArgs p;
    for (int i = 0; i < 12; i++)
        p.w.a[i] = A[i];
    p.w.src = d_src;
    p.w.dst = d_dst;
    p.w.nx = nx; p.w.ny = ny; p.w.nz = nz;
    p.w.ox = ox; p.w.oy = oy; p.w.oz = oz;
    p.w.fill = fill;
    p.w.tiles_x = p.w.tiles_y = 0;              // k_warp_affine's tiling, unused here
    p.w.ntiles = 0;
    p.w.vec = 0;
    p.tps = d_tps;
    p.m = m;
    p.tiles_x = (ox + TPS_TX - 1) / TPS_TX;
    p.tiles_y = (oy + TPS_TY - 1) / TPS_TY;
    const unsigned long long nt = (unsigned long long)p.tiles_x * p.tiles_y * ((oz + TPS_K - 1) / TPS_K);
    if (nt > 0xffffffffull)
        return tps_fail("output grid too large");
    const unsigned long long chunk = tps_tiles_per_launch(ox, oy, m);
    hipStream_t st = (hipStream_t)stream;
    void (*k)(const TpsArgs) = interp == SIFT3D_AMD_INTERP_NEAREST ? k_warp_tps<0>
                               : nx >= 2                          ? k_warp_tps<2>
                                                                  : k_warp_tps<1>;
    for (unsigned long long t0 = 0; t0 < nt; t0 += chunk) {
        p.t0 = (unsigned)t0;
        hipLaunchKernelGGL(k, dim3((unsigned)(nt - t0 < chunk ? nt - t0 : chunk)), dim3(256), 0, st, p);
        LAUNCH_CHECK();
    }
    return SIFT3D_SUCCESS;
}

} // extern "C"
