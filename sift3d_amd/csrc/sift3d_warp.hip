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

// ---- displacement fields (contract: include/sift3d_amd.h, "Displacement fields") ------------------------------
// A field is u[3][oz][oy][ox] float, planar (x, y, z), in source voxels: output voxel p reads the source at p + u(p).
//
// Export (k_affine_field) and the Jacobian (k_jacobian_det) share one tiling: a 256-lane workgroup is 64 x 4 (x, y)
// columns, a lane walks FLD_K planes of its column; a wave is 64 consecutive x of one row, so every plane's load or
// store of a channel is one coalesced 256-byte access.  The TPS export (k_tps_field) is k_warp_tps's tiling and
// radial loop with the sampling replaced by three plane stores.
constexpr int FLD_TX = 64, FLD_TY = 4, FLD_K = 8;
constexpr int JAC_K = 8;                           // k_jacobian_det: planes per lane (1, 2, 4 measured slower)

struct FieldTiles {
    int ox, oy, oz;
    int tiles_x, tiles_y, k;                     // k: planes per tile
    unsigned ntiles;                             // < 2^32 - MAX_GRID (checked at launch)
};

// tile t -> the lane's column (x, y) and first plane z0
__device__ __forceinline__ void field_tile(const FieldTiles &g, unsigned t, int &x, int &y, int &z0)
{
    const unsigned tyz = t / (unsigned)g.tiles_x;
    const int tx = (int)(t - tyz * (unsigned)g.tiles_x);
    const int ty = (int)(tyz % (unsigned)g.tiles_y), tz = (int)(tyz / (unsigned)g.tiles_y);
    x = tx * FLD_TX + (int)(threadIdx.x & 63);
    y = ty * FLD_TY + (int)(threadIdx.x >> 6);
    z0 = tz * g.k;
}

struct AffineFieldArgs {
    double a[12];
    float *field;
    FieldTiles g;
};

// u_d = (float)(q_d - (double)p_d), q_d warp_affine's expression: 12 B written per voxel, nothing read
__global__ __launch_bounds__(256) void k_affine_field(const AffineFieldArgs p)
{
    const size_t plane = (size_t)p.g.oy * (size_t)p.g.ox, vox = plane * (size_t)p.g.oz;
    for (unsigned t = blockIdx.x; t < p.g.ntiles; t += gridDim.x) {
        int x, y, z0;
        field_tile(p.g, t, x, y, z0);
        if (x >= p.g.ox || y >= p.g.oy)
            continue;
        const double xd = (double)x, yd = (double)y;
        float *out = p.field + ((size_t)z0 * (size_t)p.g.oy + (size_t)y) * (size_t)p.g.ox + (size_t)x;
        const int nk = min(FLD_K, p.g.oz - z0);
        for (int k = 0; k < nk; k++) {
            const double zd = (double)(z0 + k);
            const double qx = p.a[0] * xd + ((p.a[1] * yd + p.a[2] * zd) + p.a[3]);
            const double qy = p.a[4] * xd + ((p.a[5] * yd + p.a[6] * zd) + p.a[7]);
            const double qz = p.a[8] * xd + ((p.a[9] * yd + p.a[10] * zd) + p.a[11]);
            float *o = out + (size_t)k * plane;
            o[0] = (float)(qx - xd);
            o[vox] = (float)(qy - yd);
            o[2 * vox] = (float)(qz - zd);
        }
    }
}

// u_d = (float)((affine_d(p) + (double)s_d(p)) - (double)p_d): k_warp_tps's radial loop, word for word, without the
// sampling; the three channels of a plane leave with one coalesced store each
__global__ __launch_bounds__(256) void k_tps_field(const TpsArgs p)
{
    const unsigned t = p.t0 + blockIdx.x;
    const unsigned tyz = t / (unsigned)p.tiles_x;
    const int tx = (int)(t - tyz * (unsigned)p.tiles_x);
    const int ty = (int)(tyz % (unsigned)p.tiles_y), tz = (int)(tyz / (unsigned)p.tiles_y);
    const int x = tx * TPS_TX + (int)(threadIdx.x & 63), y = ty * TPS_TY + (int)(threadIdx.x >> 6);
    const int z0 = tz * TPS_K;
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
        const float wx = q[4], wy = q[5], wz = q[6];
        const float dx = xf - cx, dy = yf - cy;
        const float hxy = dx * dx + dy * dy;
#pragma unroll
        for (int k = 0; k < TPS_K / 2; k++) {
            const f32x2 dz = zf[k] - cz;
            const f32x2 r2 = hxy + dz * dz;
            const f32x2 r = f32x2{sqrtf(r2.x), sqrtf(r2.y)};
            sx[k] = sx[k] + wx * r;
            sy[k] = sy[k] + wy * r;
            sz[k] = sz[k] + wz * r;
        }
    }
    if (x >= p.w.ox || y >= p.w.oy)
        return;
    const double xd = (double)x, yd = (double)y;
    const size_t plane = (size_t)p.w.oy * (size_t)p.w.ox, vox = plane * (size_t)p.w.oz;
    float *out = p.w.dst + ((size_t)z0 * (size_t)p.w.oy + (size_t)y) * (size_t)p.w.ox + (size_t)x;
#pragma unroll
    for (int k = 0; k < TPS_K; k++) {
        const double zd = (double)(z0 + k);
        const float rx = (k & 1) ? sx[k / 2].y : sx[k / 2].x;
        const float ry = (k & 1) ? sy[k / 2].y : sy[k / 2].x;
        const float rz = (k & 1) ? sz[k / 2].y : sz[k / 2].x;
        const double qx = p.w.a[0] * xd + ((p.w.a[1] * yd + p.w.a[2] * zd) + p.w.a[3]) + (double)rx;
        const double qy = p.w.a[4] * xd + ((p.w.a[5] * yd + p.w.a[6] * zd) + p.w.a[7]) + (double)ry;
        const double qz = p.w.a[8] * xd + ((p.w.a[9] * yd + p.w.a[10] * zd) + p.w.a[11]) + (double)rz;
        if (z0 + k < p.w.oz) {
            float *o = out + (size_t)k * plane;
            o[0] = (float)(qx - xd);
            o[vox] = (float)(qy - yd);
            o[2 * vox] = (float)(qz - zd);
        }
    }
}

// ---- resampling through a field: sample<>'s arithmetic, split into where to read (once per voxel) and the reads
// (once per channel).  taps_at<> is sample<>'s inside test, index and fraction code word for word; gather<> is its
// loads and lerps, then the fill.
struct Taps {
    size_t r00, r10, r01, r11;                   // row offsets of the four (y, z) corner rows (NEAREST: r00 + ix)
    int ix, jx, bx;
    bool hi, in;
    float fx, fy, fz;
};

template <int LINEAR>
__device__ __forceinline__ Taps taps_at(const WarpArgs &p, double qx, double qy, double qz)
{
    Taps t;
    const bool in = (qx >= 0.0) & (qx <= (double)(p.nx - 1)) & (qy >= 0.0) & (qy <= (double)(p.ny - 1)) &
                    (qz >= 0.0) & (qz <= (double)(p.nz - 1));
    qx = in ? qx : 0.0;
    qy = in ? qy : 0.0;
    qz = in ? qz : 0.0;
    t.in = in;
    const size_t sx = (size_t)p.nx, sxy = (size_t)p.nx * (size_t)p.ny;
    if (!LINEAR) {
        const int ix = (int)floor(qx + 0.5), iy = (int)floor(qy + 0.5), iz = (int)floor(qz + 0.5);
        t.r00 = (size_t)iz * sxy + (size_t)iy * sx + (size_t)ix;
    } else {
        const double fx0 = floor(qx), fy0 = floor(qy), fz0 = floor(qz);
        const int ix = (int)fx0, iy = (int)fy0, iz = (int)fz0;
        t.fx = (float)(qx - fx0); t.fy = (float)(qy - fy0); t.fz = (float)(qz - fz0);
        const int jy = min(iy + 1, p.ny - 1), jz = min(iz + 1, p.nz - 1);
        t.r00 = (size_t)iz * sxy + (size_t)iy * sx; t.r10 = (size_t)iz * sxy + (size_t)jy * sx;
        t.r01 = (size_t)jz * sxy + (size_t)iy * sx; t.r11 = (size_t)jz * sxy + (size_t)jy * sx;
        if (LINEAR == 2) {
            t.bx = min(ix, p.nx - 2);
            t.hi = ix != t.bx;
        } else {
            t.ix = ix;
            t.jx = min(ix + 1, p.nx - 1);
        }
    }
    return t;
}

template <int LINEAR>
__device__ __forceinline__ float gather(const float *s, const Taps &t, float fill)
{
    float v;
    if (!LINEAR) {
        v = s[t.r00];
    } else {
        float a00, b00, a10, b10, a01, b01, a11, b11;
        if (LINEAR == 2) {
            const f32x2u w00 = *reinterpret_cast<const f32x2u *>(s + t.r00 + t.bx);
            const f32x2u w10 = *reinterpret_cast<const f32x2u *>(s + t.r10 + t.bx);
            const f32x2u w01 = *reinterpret_cast<const f32x2u *>(s + t.r01 + t.bx);
            const f32x2u w11 = *reinterpret_cast<const f32x2u *>(s + t.r11 + t.bx);
            a00 = t.hi ? w00.y : w00.x; b00 = w00.y;
            a10 = t.hi ? w10.y : w10.x; b10 = w10.y;
            a01 = t.hi ? w01.y : w01.x; b01 = w01.y;
            a11 = t.hi ? w11.y : w11.x; b11 = w11.y;
        } else {
            a00 = s[t.r00 + t.ix]; b00 = s[t.r00 + t.jx];
            a10 = s[t.r10 + t.ix]; b10 = s[t.r10 + t.jx];
            a01 = s[t.r01 + t.ix]; b01 = s[t.r01 + t.jx];
            a11 = s[t.r11 + t.ix]; b11 = s[t.r11 + t.jx];
        }
        const float c00 = lerp(a00, b00, t.fx), c10 = lerp(a10, b10, t.fx);
        const float c01 = lerp(a01, b01, t.fx), c11 = lerp(a11, b11, t.fx);
        v = lerp(lerp(c00, c10, t.fy), lerp(c01, c11, t.fy), t.fz);
    }
    return t.in ? v : fill;
}

struct FieldWarpArgs {
    WarpArgs w;                                  // source, destination, grids, tiles, fill, vec (w.a unused)
    const float *field;
    int nc;
};

// k_warp_affine's tiles, tile order and store exchange; the lane's 4 outputs read their u (16 lanes of a row read 64
// consecutive bytes of each plane), place their taps once and gather every channel with them
template <int LINEAR>
__global__ __launch_bounds__(256) void k_warp_field(const FieldWarpArgs f)
{
    const WarpArgs &p = f.w;
    __shared__ float4 xch[256];
    float *xs = reinterpret_cast<float *>(xch) + (threadIdx.x & ~15) * 4;
    const int lx = threadIdx.x & 15, ly = (threadIdx.x >> 4) & 3, lz = threadIdx.x >> 6;
    const size_t svox = (size_t)p.nx * (size_t)p.ny * (size_t)p.nz;
    const size_t ovox = (size_t)p.ox * (size_t)p.oy * (size_t)p.oz;
    for (unsigned base = 0; base < p.ntiles; base += gridDim.x) {
        const unsigned n = min(p.ntiles - base, gridDim.x);
        if (blockIdx.x >= n)
            return;                                                          // uniform over the block
        const unsigned t = base + xcd_swizzle(blockIdx.x, n);
        const unsigned tyz = t / (unsigned)p.tiles_x;
        const int tx = (int)(t - tyz * (unsigned)p.tiles_x);
        const int ty = (int)(tyz % (unsigned)p.tiles_y), tz = (int)(tyz / (unsigned)p.tiles_y);
        const int xt = tx * TX, y = ty * TY + ly, z = tz * TZ + lz;
        const bool row = y < p.oy && z < p.oz;
        const size_t orow = ((size_t)z * (size_t)p.oy + (size_t)y) * (size_t)p.ox;
        // outputs past the grid read no field (u = 0) and sample inside the source; they are not stored
        Taps tp[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int x = xt + lx + 16 * k;
            float ux = 0.0f, uy = 0.0f, uz = 0.0f;
            if (row && x < p.ox) {
                const float *u = f.field + orow + (size_t)x;
                ux = u[0];
                uy = u[ovox];
                uz = u[2 * ovox];
            }
            tp[k] = taps_at<LINEAR>(p, (double)x + (double)ux, (double)y + (double)uy, (double)z + (double)uz);
        }
        const int x0 = xt + 4 * lx;
        const bool st = row && x0 < p.ox;
        for (int c = 0; c < f.nc; c++) {
            const float *s = p.src + (size_t)c * svox;
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; k++)
                v[k] = gather<LINEAR>(s, tp[k], p.fill);
            __syncthreads();                                                 // previous exchange's reads done
#pragma unroll
            for (int k = 0; k < 4; k++)
                xs[lx + 16 * k] = v[k];
            __syncthreads();
            const float4 w = xch[threadIdx.x];
            if (!st)
                continue;
            float *out = p.dst + (size_t)c * ovox + orow + (size_t)x0;
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
}

// ---- Jacobian determinant of q(p) = p + u(p) ------------------------------------------------------------------
// Per voxel 12 B read (the centre of the lane's z column arrives once, as the next plane; the x and y neighbours are
// loads of the neighbouring lanes' words, 0.71 of all requests hit L1) and 4 B written.  Bound by load latency: a wave
// has one plane's 15 loads in flight before its f64 tail.  Stats: a folded count and min / max keys, reduced per
// wave by shuffles and per workgroup through LDS, then one atomic per workgroup and statistic.
struct JacArgs {
    const float *field;
    float *det;                                  // may be NULL
    unsigned long long *folded;                  // d_stats + 0
    int *kmin, *kmax;                            // d_stats + 8, + 12: keys while the kernel runs, floats after
    FieldTiles g;
};

// a monotone map float -> int (for non-NaN values: a < b  <=>  key(a) < key(b), -0 just below +0)
__device__ __forceinline__ int fkey(float f)
{
    const int b = __float_as_int(f);
    return b >= 0 ? b : b ^ 0x7fffffff;
}

__device__ __forceinline__ float grad(float lo, float c, float hi, int i, int n)
{
    // numpy.gradient: central difference inside, one-sided at the ends; an axis of length 1 has none
    return n == 1 ? 0.0f : i == 0 ? hi - c : i == n - 1 ? c - lo : (hi - lo) * 0.5f;
}

__global__ void k_jacobian_init(JacArgs p)
{
    if (threadIdx.x == 0) {
        *p.folded = 0ull;
        *p.kmin = 0x7f800000;                                                // key(+inf)
        *p.kmax = (int)(0xff800000u ^ 0x7fffffffu);                          // key(-inf)
    }
}

__global__ void k_jacobian_finish(JacArgs p)
{
    if (threadIdx.x == 0) {
        const int a = *p.kmin, b = *p.kmax;
        *reinterpret_cast<float *>(p.kmin) = __int_as_float(a >= 0 ? a : a ^ 0x7fffffff);
        *reinterpret_cast<float *>(p.kmax) = __int_as_float(b >= 0 ? b : b ^ 0x7fffffff);
    }
}

__global__ __launch_bounds__(256) void k_jacobian_det(const JacArgs p)
{
    __shared__ unsigned long long s_cnt[4];
    __shared__ int s_min[4], s_max[4];
    const FieldTiles &g = p.g;
    const float *__restrict__ field = p.field;
    float *__restrict__ dst = p.det;
    const size_t sx = (size_t)g.ox, plane = (size_t)g.oy * (size_t)g.ox, vox = plane * (size_t)g.oz;
    unsigned long long cnt = 0;
    int kmn = 0x7f800000, kmx = (int)(0xff800000u ^ 0x7fffffffu);
    for (unsigned t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
        int x, y, z0;
        field_tile(g, t, x, y, z0);
        if (x < g.ox && y < g.oy) {
            const size_t col = (size_t)y * sx + (size_t)x;
            const size_t dxm = x > 0 ? 1 : 0, dxp = x + 1 < g.ox ? 1 : 0;      // neighbour offsets, clamped
            const size_t dym = y > 0 ? sx : 0, dyp = y + 1 < g.oy ? sx : 0;
            const int nk = min(JAC_K, g.oz - z0);
            float lo[3], c[3], hi[3];                                        // u at z - 1, z, z + 1 of the column
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
                    hi[d] = z + 1 < g.oz ? u[o + plane] : c[d];
                    const float gx = grad(u[o - dxm], c[d], u[o + dxp], x, g.ox);
                    const float gy = grad(u[o - dym], c[d], u[o + dyp], y, g.oy);
                    const float gz = grad(lo[d], c[d], hi[d], z, g.oz);
                    j[d][0] = (d == 0 ? 1.0f : 0.0f) + gx;
                    j[d][1] = (d == 1 ? 1.0f : 0.0f) + gy;
                    j[d][2] = (d == 2 ? 1.0f : 0.0f) + gz;
                }
                const double j00 = j[0][0], j01 = j[0][1], j02 = j[0][2];
                const double j10 = j[1][0], j11 = j[1][1], j12 = j[1][2];
                const double j20 = j[2][0], j21 = j[2][1], j22 = j[2][2];
                const double dd = j00 * (j11 * j22 - j12 * j21) - j01 * (j10 * j22 - j12 * j20) +
                                  j02 * (j10 * j21 - j11 * j20);
                const float det = (float)dd;
                if (dst)
                    dst[o] = det;
                cnt += !(det > 0.0f);
                if (det == det) {
                    const int kk = fkey(det);
                    kmn = min(kmn, kk);
                    kmx = max(kmx, kk);
                }
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    lo[d] = c[d];
                    c[d] = hi[d];
                }
            }
        }
    }
    // once per workgroup, after all its tiles: one wave by butterfly, the workgroup through LDS, the device by one
    // atomic per statistic (a persistent grid keeps that to one set per resident workgroup)
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        cnt += __shfl_xor(cnt, s);
        kmn = min(kmn, __shfl_xor(kmn, s));
        kmx = max(kmx, __shfl_xor(kmx, s));
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_cnt[wv] = cnt;
        s_min[wv] = kmn;
        s_max[wv] = kmx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long n = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        const int a = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
        const int b = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
        if (n)
            atomicAdd(p.folded, n);
        if (a != 0x7f800000)
            atomicMin(p.kmin, a);
        if (b != (int)(0xff800000u ^ 0x7fffffffu))
            atomicMax(p.kmax, b);
    }
}

int field_fail(const char *fn, const char *why)
{
    snprintf(g_err, sizeof(g_err), "%s: %s", fn, why);
    fprintf(stderr, "sift3d_amd: %s\n", g_err);
    return SIFT3D_FAILURE;
}

// the export / Jacobian tiling of an output grid; false when it has 2^32 - MAX_GRID tiles or more
bool field_tiles(int ox, int oy, int oz, int k, FieldTiles &g)
{
    g.ox = ox; g.oy = oy; g.oz = oz;
    g.k = k;
    g.tiles_x = (ox + FLD_TX - 1) / FLD_TX;
    g.tiles_y = (oy + FLD_TY - 1) / FLD_TY;
    const unsigned long long nt = (unsigned long long)g.tiles_x * g.tiles_y * ((oz + k - 1) / k);
    if (nt > 0xffffffffull - MAX_GRID)
        return false;
    g.ntiles = (unsigned)nt;
    return true;
}

bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

// ---- field composition (contract: include/sift3d_amd.h, "Field composition, exponential and inverse") -----------
// k_warp_field with the source u (3 channels) and the field v: the lane's 4 outputs read v (which also gives the
// add's operand: no extra read), place one set of taps each -- clamped onto u's grid only when outside -- and gather
// the three channels of u with them; the results leave through the same LDS exchange.  Statistics: per lane, per
// wave by butterfly, per workgroup through LDS into partial slot blockIdx.x; k_compose_finish combines the slots in a
// fixed order.  With statistics the grid is min(tiles, CMP_GRID) whatever the device, so the bits of the sum depend on
// the shapes; without, it is k_warp_field's.
constexpr unsigned CMP_GRID = SIFT3D_AMD_FIELD_WORK_BYTES / 32;    // slots: sum, max (double), two uint64 counts

struct ComposeArgs {
    WarpArgs w;                                  // src = u, dst = out (may be null), grids, tiles, vec
    const float *v;
    double *psum, *pmax;                         // [CMP_GRID] each
    unsigned long long *pcnt, *pins;             // [CMP_GRID] each
};

template <int MODE, int LINEAR, bool STATS>
__global__ __launch_bounds__(256) void k_field_compose(const ComposeArgs f)
{
    const WarpArgs &p = f.w;
    __shared__ float4 xch[256];
    __shared__ double s_sum[4], s_max[4];
    __shared__ unsigned long long s_cnt[4], s_ins[4];
    float *xs = reinterpret_cast<float *>(xch) + (threadIdx.x & ~15) * 4;
    const int lx = threadIdx.x & 15, ly = (threadIdx.x >> 4) & 3, lz = threadIdx.x >> 6;
    const size_t svox = (size_t)p.nx * (size_t)p.ny * (size_t)p.nz;
    const size_t ovox = (size_t)p.ox * (size_t)p.oy * (size_t)p.oz;
    const double hx = (double)(p.nx - 1), hy = (double)(p.ny - 1), hz = (double)(p.nz - 1);
    double lsum = 0.0, lmax = 0.0;
    unsigned long long lcnt = 0, lins = 0;
    for (unsigned base = 0; base < p.ntiles; base += gridDim.x) {
        const unsigned n = min(p.ntiles - base, gridDim.x);
        if (blockIdx.x >= n)
            break;                                                           // uniform over the block
        const unsigned t = base + xcd_swizzle(blockIdx.x, n);
        const unsigned tyz = t / (unsigned)p.tiles_x;
        const int tx = (int)(t - tyz * (unsigned)p.tiles_x);
        const int ty = (int)(tyz % (unsigned)p.tiles_y), tz = (int)(tyz / (unsigned)p.tiles_y);
        const int xt = tx * TX, y = ty * TY + ly, z = tz * TZ + lz;
        const bool row = y < p.oy && z < p.oz;
        const size_t orow = ((size_t)z * (size_t)p.oy + (size_t)y) * (size_t)p.ox;
        // outputs past the grid read no field (v = 0), sample inside u and are neither stored nor counted
        Taps tp[4];
        float v[4][3];
        bool live[4], in[4], nan[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int x = xt + lx + 16 * k;
            v[k][0] = v[k][1] = v[k][2] = 0.0f;
            live[k] = row && x < p.ox;
            if (live[k]) {
                const float *src = f.v + orow + (size_t)x;
                v[k][0] = src[0];
                v[k][1] = src[ovox];
                v[k][2] = src[2 * ovox];
            }
            double qx = (double)x + (double)v[k][0], qy = (double)y + (double)v[k][1];
            double qz = (double)z + (double)v[k][2];
            in[k] = (qx >= 0.0) & (qx <= hx) & (qy >= 0.0) & (qy <= hy) & (qz >= 0.0) & (qz <= hz);
            nan[k] = (qx != qx) | (qy != qy) | (qz != qz);
            if (!in[k]) {
                // nearest-edge extension; a NaN stays NaN and taps_at sends it to voxel 0 (the output is NaN)
                qx = qx < 0.0 ? 0.0 : qx > hx ? hx : qx;
                qy = qy < 0.0 ? 0.0 : qy > hy ? hy : qy;
                qz = qz < 0.0 ? 0.0 : qz > hz ? hz : qz;
            }
            tp[k] = taps_at<LINEAR>(p, qx, qy, qz);
        }
        float o[3][4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float r[3];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float s = gather<LINEAR>(p.src + (size_t)c * svox, tp[k], 0.0f);
                r[c] = v[k][c] + s;
                o[c][k] = nan[k] ? __int_as_float(0x7fc00000) : MODE == SIFT3D_AMD_FIELD_COMPOSE ? r[c] : -s;
            }
            if (STATS && live[k] && !nan[k]) {
                const double m = sqrt(((double)r[0] * r[0] + (double)r[1] * r[1]) + (double)r[2] * r[2]);
                lsum += m;
                lmax = fmax(lmax, m);
                lcnt += 1;
                lins += in[k] ? 1 : 0;
            }
        }
        if (!p.dst)
            continue;                                                        // uniform: statistics only
        const int x0 = xt + 4 * lx;
        const bool st = row && x0 < p.ox;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            __syncthreads();                                                 // previous exchange's reads done
#pragma unroll
            for (int k = 0; k < 4; k++)
                xs[lx + 16 * k] = o[c][k];
            __syncthreads();
            const float4 w = xch[threadIdx.x];
            if (!st)
                continue;
            float *out = p.dst + (size_t)c * ovox + orow + (size_t)x0;
            if (p.vec) {
                st4(out, w);
            } else {
                const float ov[4] = {w.x, w.y, w.z, w.w};
                const int m = min(4, p.ox - x0);
#pragma nounroll
                for (int k = 0; k < m; k++)
                    out[k] = ov[k];
            }
        }
    }
    if (!STATS)
        return;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        lsum += __shfl_xor(lsum, s);
        lmax = fmax(lmax, __shfl_xor(lmax, s));
        lcnt += __shfl_xor(lcnt, s);
        lins += __shfl_xor(lins, s);
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_sum[wv] = lsum;
        s_max[wv] = lmax;
        s_cnt[wv] = lcnt;
        s_ins[wv] = lins;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        f.psum[blockIdx.x] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
        f.pmax[blockIdx.x] = fmax(fmax(s_max[0], s_max[1]), fmax(s_max[2], s_max[3]));
        f.pcnt[blockIdx.x] = ((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3];
        f.pins[blockIdx.x] = ((s_ins[0] + s_ins[1]) + s_ins[2]) + s_ins[3];
    }
}

// the partial slots 0 .. n-1 in a fixed order (k_demons_finish's): lane t takes slots t, t + 256, ... in turn, then
// a fixed tree; the record is {sum, max, count, inside}
__global__ __launch_bounds__(256) void k_compose_finish(const ComposeArgs f, unsigned n, double *rec)
{
    __shared__ double s_sum[256], s_max[256];
    __shared__ unsigned long long s_cnt[256], s_ins[256];
    double a = 0.0, m = 0.0;
    unsigned long long b = 0, c = 0;
    for (unsigned i = threadIdx.x; i < n; i += 256) {
        a += f.psum[i];
        m = fmax(m, f.pmax[i]);
        b += f.pcnt[i];
        c += f.pins[i];
    }
    s_sum[threadIdx.x] = a;
    s_max[threadIdx.x] = m;
    s_cnt[threadIdx.x] = b;
    s_ins[threadIdx.x] = c;
    __syncthreads();
    for (unsigned s = 128; s >= 1; s >>= 1) {
        if (threadIdx.x < s) {
            s_sum[threadIdx.x] = s_sum[threadIdx.x] + s_sum[threadIdx.x + s];
            s_max[threadIdx.x] = fmax(s_max[threadIdx.x], s_max[threadIdx.x + s]);
            s_cnt[threadIdx.x] = s_cnt[threadIdx.x] + s_cnt[threadIdx.x + s];
            s_ins[threadIdx.x] = s_ins[threadIdx.x] + s_ins[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        rec[0] = s_sum[0];
        rec[1] = s_max[0];
        reinterpret_cast<unsigned long long *>(rec)[2] = s_cnt[0];
        reinterpret_cast<unsigned long long *>(rec)[3] = s_ins[0];
    }
}

// dst = src * s per element (the exponential's w_0 = v * 2^-K); dst may be src
__global__ __launch_bounds__(256) void k_field_scale(float *dst, const float *src, size_t n, float s)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        dst[i] = src[i] * s;
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

// ---- displacement fields ---------------------------------------------------------------------------------------
int sift3d_hip_affine_field(float *d_field, int ox, int oy, int oz, const double *A, void *stream)
{
    static const char fn[] = "sift3d_hip_affine_field";
    if (!d_field || !A)
        return field_fail(fn, "NULL argument");
    if (ox <= 0 || oy <= 0 || oz <= 0)
        return field_fail(fn, "dimensions must be positive");
    for (int i = 0; i < 12; i++)
        if (!std::isfinite(A[i]))
            return field_fail(fn, "the affine map is not finite");
    AffineFieldArgs p;
    if (!field_tiles(ox, oy, oz, FLD_K, p.g))
        return field_fail(fn, "output grid too large");
    for (int i = 0; i < 12; i++)
        p.a[i] = A[i];
    p.field = d_field;
    const unsigned grid = p.g.ntiles < MAX_GRID ? p.g.ntiles : MAX_GRID;
    hipLaunchKernelGGL(k_affine_field, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

int sift3d_hip_tps_field_launches(int ox, int oy, int oz, int m)
{
    return sift3d_hip_warp_tps_launches(ox, oy, oz, m);    // the same tiles and launch budget
}

int sift3d_hip_tps_field(float *d_field, int ox, int oy, int oz, const double *A, const float *d_tps, int m,
                         void *stream)
{
    static const char fn[] = "sift3d_hip_tps_field";
    if (!d_field || !A || !d_tps)
        return field_fail(fn, "NULL argument");
    if (ox <= 0 || oy <= 0 || oz <= 0)
        return field_fail(fn, "dimensions must be positive");
    if (m < 1 || m > SIFT3D_AMD_TPS_MAX_POINTS)
        return field_fail(fn, "the number of control points must be in [1, SIFT3D_AMD_TPS_MAX_POINTS]");
    for (int i = 0; i < 12; i++)
        if (!std::isfinite(A[i]))
            return field_fail(fn, "the affine map is not finite");
    if ((uintptr_t)d_tps & 15)
        return field_fail(fn, "the control point records are not 16-byte aligned");
    if (overlap(d_field, 3 * sizeof(float) * (size_t)ox * oy * oz, d_tps, sizeof(float) * SIFT3D_AMD_TPS_FLOATS * (size_t)m))
        return field_fail(fn, "the field overlaps the control points");
    TpsArgs p;
    for (int i = 0; i < 12; i++)
        p.w.a[i] = A[i];
    p.w.src = nullptr;
    p.w.dst = d_field;
    p.w.nx = p.w.ny = p.w.nz = 0;
    p.w.ox = ox; p.w.oy = oy; p.w.oz = oz;
    p.w.fill = 0.0f;
    p.w.tiles_x = p.w.tiles_y = 0;
    p.w.ntiles = 0;
    p.w.vec = 0;
    p.tps = d_tps;
    p.m = m;
    p.tiles_x = (ox + TPS_TX - 1) / TPS_TX;
    p.tiles_y = (oy + TPS_TY - 1) / TPS_TY;
    const unsigned long long nt = (unsigned long long)p.tiles_x * p.tiles_y * ((oz + TPS_K - 1) / TPS_K);
    if (nt > 0xffffffffull)
        return field_fail(fn, "output grid too large");
    const unsigned long long chunk = tps_tiles_per_launch(ox, oy, m);
    for (unsigned long long t0 = 0; t0 < nt; t0 += chunk) {
        p.t0 = (unsigned)t0;
        hipLaunchKernelGGL(k_tps_field, dim3((unsigned)(nt - t0 < chunk ? nt - t0 : chunk)), dim3(256), 0,
                           (hipStream_t)stream, p);
        LAUNCH_CHECK();
    }
    return SIFT3D_SUCCESS;
}

int sift3d_hip_warp_field(const float *d_src, int nx, int ny, int nz, int nc, const float *d_field, int ox, int oy,
                          int oz, float *d_dst, int interp, float fill, void *stream)
{
    static const char fn[] = "sift3d_hip_warp_field";
    if (!d_src || !d_field || !d_dst)
        return field_fail(fn, "NULL argument");
    if (nx <= 0 || ny <= 0 || nz <= 0 || ox <= 0 || oy <= 0 || oz <= 0)
        return field_fail(fn, "dimensions must be positive");
    if (nc < 1)
        return field_fail(fn, "the number of channels must be positive");
    if (interp != SIFT3D_AMD_INTERP_NEAREST && interp != SIFT3D_AMD_INTERP_LINEAR)
        return field_fail(fn, "unknown interpolation mode");
    if (((uintptr_t)d_src | (uintptr_t)d_field | (uintptr_t)d_dst) & 3)
        return field_fail(fn, "a buffer is not 4-byte aligned");
    {
        const size_t ns = sizeof(float) * (size_t)nc * nx * ny * nz, no = sizeof(float) * (size_t)ox * oy * oz;
        if (overlap(d_dst, (size_t)nc * no, d_src, ns) || overlap(d_dst, (size_t)nc * no, d_field, 3 * no))
            return field_fail(fn, "the destination overlaps the source or the field");
    }
    FieldWarpArgs f;
    WarpArgs &p = f.w;
    for (int i = 0; i < 12; i++)
        p.a[i] = 0.0;
    p.src = d_src;
    p.dst = d_dst;
    p.nx = nx; p.ny = ny; p.nz = nz;
    p.ox = ox; p.oy = oy; p.oz = oz;
    p.tiles_x = (ox + TX - 1) / TX;
    p.tiles_y = (oy + TY - 1) / TY;
    {
        const unsigned long long nt = (unsigned long long)p.tiles_x * p.tiles_y * ((oz + TZ - 1) / TZ);
        if (nt > 0xffffffffull - MAX_GRID)
            return field_fail(fn, "output grid too large");
        p.ntiles = (unsigned)nt;
    }
    p.fill = fill;
    p.vec = (ox % 4 == 0) && !((uintptr_t)d_dst & 15);
    f.field = d_field;
    f.nc = nc;
    const unsigned grid = p.ntiles < MAX_GRID ? p.ntiles : MAX_GRID;
    void (*k)(const FieldWarpArgs) = interp == SIFT3D_AMD_INTERP_NEAREST ? k_warp_field<0>
                                     : nx >= 2                          ? k_warp_field<2>
                                                                        : k_warp_field<1>;
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, (hipStream_t)stream, f);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

int sift3d_hip_jacobian_det(const float *d_field, int ox, int oy, int oz, float *d_det, void *d_stats, void *stream)
{
    static const char fn[] = "sift3d_hip_jacobian_det";
    if (!d_field || !d_stats)
        return field_fail(fn, "NULL argument");
    if (ox <= 0 || oy <= 0 || oz <= 0)
        return field_fail(fn, "dimensions must be positive");
    if ((uintptr_t)d_stats & 7)
        return field_fail(fn, "the stats buffer is not 8-byte aligned");
    if (((uintptr_t)d_field | (uintptr_t)d_det) & 3)
        return field_fail(fn, "a buffer is not 4-byte aligned");
    {
        const size_t no = sizeof(float) * (size_t)ox * oy * oz;
        if (overlap(d_stats, SIFT3D_AMD_JACOBIAN_STATS_BYTES, d_field, 3 * no) ||
            (d_det && (overlap(d_det, no, d_field, 3 * no) || overlap(d_det, no, d_stats, SIFT3D_AMD_JACOBIAN_STATS_BYTES))))
            return field_fail(fn, "the outputs overlap the field or each other");
    }
    JacArgs p;
    if (!field_tiles(ox, oy, oz, JAC_K, p.g))
        return field_fail(fn, "output grid too large");
    p.field = d_field;
    p.det = d_det;
    p.folded = (unsigned long long *)d_stats;
    p.kmin = (int *)((char *)d_stats + 8);
    p.kmax = (int *)((char *)d_stats + 12);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_jacobian_init, dim3(1), dim3(64), 0, st, p);
    LAUNCH_CHECK();
    // persistent: as many workgroups as are resident at once (the registers decide), each reducing its stats once
    int dev = 0, cus = 0, per_cu = 0;
    HIPCHK(hipGetDevice(&dev));
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_jacobian_det, 256, 0));
    const unsigned long long res = (unsigned long long)(cus > 0 ? cus : 1) * (per_cu > 0 ? per_cu : 1);
    const unsigned grid = p.g.ntiles < res ? p.g.ntiles : (unsigned)res;
    hipLaunchKernelGGL(k_jacobian_det, dim3(grid), dim3(256), 0, st, p);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_jacobian_finish, dim3(1), dim3(64), 0, st, p);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

// Launchers for sift3d_field_ops.c, which has checked every argument (not exported from the library).
int sift3d_field_compose_launch(const float *d_u, int ux, int uy, int uz, const float *d_v, int ox, int oy, int oz,
                                float *d_out, int mode, void *d_stats, void *d_work, void *stream)
{
    static const char fn[] = "sift3d_hip_field_compose";
    ComposeArgs f;
    WarpArgs &p = f.w;
    for (int i = 0; i < 12; i++)
        p.a[i] = 0.0;
    p.src = d_u;
    p.dst = d_out;
    p.nx = ux; p.ny = uy; p.nz = uz;
    p.ox = ox; p.oy = oy; p.oz = oz;
    p.tiles_x = (ox + TX - 1) / TX;
    p.tiles_y = (oy + TY - 1) / TY;
    {
        const unsigned long long nt = (unsigned long long)p.tiles_x * p.tiles_y * ((oz + TZ - 1) / TZ);
        if (nt > 0xffffffffull - MAX_GRID)
            return field_fail(fn, "output grid too large");
        p.ntiles = (unsigned)nt;
    }
    p.fill = 0.0f;
    p.vec = (ox % 4 == 0) && !((uintptr_t)d_out & 15);
    f.v = d_v;
    f.psum = (double *)d_work;
    f.pmax = f.psum + CMP_GRID;
    f.pcnt = (unsigned long long *)(f.pmax + CMP_GRID);
    f.pins = f.pcnt + CMP_GRID;
    // with statistics a fixed grid of partial slots; without, k_warp_field's grid (one tile per workgroup up to
    // MAX_GRID): a persistent grid of CMP_GRID workgroups is not resident at once and ends in a tail of its own
    const bool stats = d_stats != nullptr;
    const unsigned cap = stats ? CMP_GRID : MAX_GRID;
    const unsigned grid = p.ntiles < cap ? p.ntiles : cap;
    void (*k)(const ComposeArgs);
    if (mode == SIFT3D_AMD_FIELD_COMPOSE)
        k = ux >= 2 ? (stats ? k_field_compose<SIFT3D_AMD_FIELD_COMPOSE, 2, true> : k_field_compose<SIFT3D_AMD_FIELD_COMPOSE, 2, false>)
                    : (stats ? k_field_compose<SIFT3D_AMD_FIELD_COMPOSE, 1, true> : k_field_compose<SIFT3D_AMD_FIELD_COMPOSE, 1, false>);
    else
        k = ux >= 2 ? (stats ? k_field_compose<SIFT3D_AMD_FIELD_INVERT, 2, true> : k_field_compose<SIFT3D_AMD_FIELD_INVERT, 2, false>)
                    : (stats ? k_field_compose<SIFT3D_AMD_FIELD_INVERT, 1, true> : k_field_compose<SIFT3D_AMD_FIELD_INVERT, 1, false>);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, st, f);
    LAUNCH_CHECK();
    if (stats) {
        hipLaunchKernelGGL(k_compose_finish, dim3(1), dim3(256), 0, st, f, grid, (double *)d_stats);
        LAUNCH_CHECK();
    }
    return SIFT3D_SUCCESS;
}

int sift3d_field_scale_launch(float *d_dst, const float *d_src, size_t n, float s, void *stream)
{
    size_t blocks = (n + 255) / 256;
    if (blocks > 8192)
        blocks = 8192;
    if (blocks < 1)
        blocks = 1;
    hipLaunchKernelGGL(k_field_scale, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_dst, d_src, n, s);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

} // extern "C"
