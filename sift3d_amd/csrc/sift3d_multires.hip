// sift3d_multires.hip -- the two grid transfers of multi-resolution demons (contract: include/sift3d_amd.h,
// "Multi-resolution demons"): k_restrict2 halves a multi-channel image with the separable binomial (1/4, 1/2, 1/4),
// k_field_prolong2 carries a displacement field to the grid twice as fine.  The pyramid driver that chains them with
// the demons loop is host code (sift3d_multires.c), which checks every argument before it calls a launcher here.
//
// Both follow k_affine_field / k_field_add in layout: a 256-lane workgroup is 64 x 4 (x, y) columns, a wave one
// row, a lane walks a run of planes of its column; 64-bit offsets.  On the fine side a lane owns four consecutive x
// (one 16-byte access when the rows are 16-byte aligned: nx % 4 == 0 and an aligned base), so a wave's access is
// 1 KiB contiguous; on the coarse side the same lane owns the two or three voxels under them.
//
// k_restrict2 reads 4 B per fine voxel and writes 1/8 of that: HBM-bound by its reads.  The x pass is done in
// registers on each fine row as it is loaded (a 16-byte load and the voxel left of it), the y pass on the three x-passed
// rows of a coarse row, the z pass on a rolling window of three xy-passed planes of which the odd one is shared by
// two coarse planes: every fine voxel comes from HBM once; odd rows are loaded by two waves and a tile's first plane
// by the tile below, both from cache.
//
// k_field_prolong2 writes 12 B per fine voxel and reads 1/8 of that.  p / 2 is an integer or a half, so every
// output is 0.5f * (a + b) of two coarse neighbours per axis (a == b where p is even or clamped): a lane loads
// three coarse x of two coarse rows per coarse plane and stores the 4 (x) x 2 (y) x 2 (z) fine voxels between them, so
// here a wave is one coarse row (two fine rows) and a workgroup eight fine rows.
#include "sift3d_kernels_common.h"

namespace {

constexpr int MR_TX = 64, MR_TY = 4;
constexpr int RES_K = 16;                        // k_restrict2: coarse planes per tile (2 RES_K + 1 fine planes read)
constexpr int PRO_K = 8;                         // k_field_prolong2: fine planes per tile (even)
constexpr unsigned MR_MAX_GRID = 1u << 20;       // workgroups per launch; the tiles beyond are strided over

struct MultiresTiles {
    int tiles_x, tiles_y, tiles_z;               // per channel
    unsigned ntiles;                             // tiles_x * tiles_y * tiles_z * channels, < 2^32 - MR_MAX_GRID
};

// tile t -> the lane's quad of x (xq), its row y, the tile's plane run tz and the channel: x fastest, channel slowest
__device__ __forceinline__ void mr_tile(const MultiresTiles &g, unsigned t, int &xq, int &y, int &tz, int &c)
{
    const unsigned a = t / (unsigned)g.tiles_x;
    const int tx = (int)(t - a * (unsigned)g.tiles_x);
    const unsigned b = a / (unsigned)g.tiles_y;
    const int ty = (int)(a - b * (unsigned)g.tiles_y);
    c = (int)(b / (unsigned)g.tiles_z);
    tz = (int)(b - (unsigned)c * (unsigned)g.tiles_z);
    xq = tx * MR_TX + (int)(threadIdx.x & 63);
    y = ty * MR_TY + (int)(threadIdx.x >> 6);
}

struct RestrictArgs {
    const float *src;
    float *dst;
    int nx, ny, nz, cx, cy, cz;
    float scale;
    MultiresTiles g;
};

// the x pass of one fine row for the coarse voxels 2 xq and 2 xq + 1: fine x = 4 xq - 1 .. 4 xq + 3, clamped
template <bool VEC>
__device__ __forceinline__ void restrict_row(const float *__restrict__ row, int xf, int nx, float &r0, float &r1)
{
    float a, b, c, d, e;
    if (VEC) {                                   // nx % 4 == 0: xf + 3 <= nx - 1
        const float4 v = ld4(row + xf);
        a = row[xf > 0 ? xf - 1 : 0];
        b = v.x; c = v.y; d = v.z; e = v.w;
    } else {
        const int hi = nx - 1;
        a = row[xf > 0 ? xf - 1 : 0];
        b = row[xf];
        c = row[min(xf + 1, hi)];
        d = row[min(xf + 2, hi)];
        e = row[min(xf + 3, hi)];
    }
    r0 = (0.25f * a + 0.5f * b) + 0.25f * c;
    r1 = (0.25f * c + 0.5f * d) + 0.25f * e;
}

// the x and y passes of fine plane `pl` for one coarse row: the fine rows at the offsets ym, y0, yp
template <bool VEC>
__device__ __forceinline__ void restrict_plane(const float *__restrict__ pl, size_t ym, size_t y0, size_t yp, int xf,
                                               int nx, float &p0, float &p1)
{
    float m0, m1, c0, c1, q0, q1;
    restrict_row<VEC>(pl + ym, xf, nx, m0, m1);
    restrict_row<VEC>(pl + y0, xf, nx, c0, c1);
    restrict_row<VEC>(pl + yp, xf, nx, q0, q1);
    p0 = (0.25f * m0 + 0.5f * c0) + 0.25f * q0;
    p1 = (0.25f * m1 + 0.5f * c1) + 0.25f * q1;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_restrict2(const RestrictArgs p)
{
    const size_t sx = (size_t)p.nx, plane = (size_t)p.ny * sx, vox = plane * (size_t)p.nz;
    const size_t cplane = (size_t)p.cy * (size_t)p.cx, cvox = cplane * (size_t)p.cz;
    for (unsigned t = blockIdx.x; t < p.g.ntiles; t += gridDim.x) {
        int xq, yc, tz, c;
        mr_tile(p.g, t, xq, yc, tz, c);
        const int xc = 2 * xq, xf = 4 * xq;
        if (xc >= p.cx || yc >= p.cy)
            continue;
        const bool two = xc + 1 < p.cx;
        const int yf = 2 * yc;
        const size_t y0 = (size_t)yf * sx, ym = (size_t)(yf > 0 ? yf - 1 : 0) * sx;
        const size_t yp = (size_t)min(yf + 1, p.ny - 1) * sx;
        const float *__restrict__ src = p.src + (size_t)c * vox;
        float *__restrict__ out = p.dst + (size_t)c * cvox + (size_t)yc * (size_t)p.cx + (size_t)xc;
        const int k0 = tz * RES_K, k1 = min(k0 + RES_K, p.cz);
        float lo0, lo1;
        restrict_plane<VEC>(src + (size_t)(k0 > 0 ? 2 * k0 - 1 : 0) * plane, ym, y0, yp, xf, p.nx, lo0, lo1);
        for (int k = k0; k < k1; k++) {
            float mid0, mid1, hi0, hi1;
            restrict_plane<VEC>(src + (size_t)(2 * k) * plane, ym, y0, yp, xf, p.nx, mid0, mid1);
            hi0 = mid0;
            hi1 = mid1;
            if (2 * k + 1 < p.nz)
                restrict_plane<VEC>(src + (size_t)(2 * k + 1) * plane, ym, y0, yp, xf, p.nx, hi0, hi1);
            const float r0 = ((0.25f * lo0 + 0.5f * mid0) + 0.25f * hi0) * p.scale;
            const float r1 = ((0.25f * lo1 + 0.5f * mid1) + 0.25f * hi1) * p.scale;
            float *o = out + (size_t)k * cplane;
            if (VEC) {                           // cx even, dst 8-byte aligned
                *reinterpret_cast<float2 *>(o) = make_float2(r0, r1);
            } else {
                o[0] = r0;
                if (two)
                    o[1] = r1;
            }
            lo0 = hi0;
            lo1 = hi1;
        }
    }
}

struct ProlongArgs {
    const float *coarse;
    float *fine;
    int nx, ny, nz, cx, cy, cz;
    MultiresTiles g;
};

// the x pass of one coarse row for the fine voxels 4 xq .. 4 xq + 3: h_j = 0.5f * (c[i0] + c[i1]), i0 = x / 2,
// i1 = min(i0 + (x & 1), cx - 1)
__device__ __forceinline__ float4 prolong_row(const float *__restrict__ row, int xq, int cx)
{
    const int hi = cx - 1;
    const float a = row[min(2 * xq, hi)], b = row[min(2 * xq + 1, hi)], c = row[min(2 * xq + 2, hi)];
    return make_float4(0.5f * (a + a), 0.5f * (a + b), 0.5f * (b + b), 0.5f * (b + c));
}

__device__ __forceinline__ float4 half_sum(const float4 &a, const float4 &b)
{
    return make_float4(0.5f * (a.x + b.x), 0.5f * (a.y + b.y), 0.5f * (a.z + b.z), 0.5f * (a.w + b.w));
}

template <bool VEC>
__device__ __forceinline__ void prolong_store(float *o, int xf, int nx, const float4 &a, const float4 &b)
{
    const float4 h = half_sum(a, b);
    const float4 v = make_float4(2.0f * h.x, 2.0f * h.y, 2.0f * h.z, 2.0f * h.w);
    if (VEC) {                                   // nx % 4 == 0, fine 16-byte aligned
        st4(o, v);
    } else {
        o[0] = v.x;
        if (xf + 1 < nx)
            o[1] = v.y;
        if (xf + 2 < nx)
            o[2] = v.z;
        if (xf + 3 < nx)
            o[3] = v.w;
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_field_prolong2(const ProlongArgs p)
{
    const size_t sx = (size_t)p.nx, plane = (size_t)p.ny * sx, vox = plane * (size_t)p.nz;
    const size_t cplane = (size_t)p.cy * (size_t)p.cx, cvox = cplane * (size_t)p.cz;
    for (unsigned t = blockIdx.x; t < p.g.ntiles; t += gridDim.x) {
        int xq, y, tz, c;
        mr_tile(p.g, t, xq, y, tz, c);                                  // y: the lane's coarse row
        const int xf = 4 * xq, yf = 2 * y;
        if (xf >= p.nx || y >= p.cy)
            continue;
        const bool odd_row = yf + 1 < p.ny;
        const size_t j0 = (size_t)y * (size_t)p.cx, j1 = (size_t)min(y + 1, p.cy - 1) * (size_t)p.cx;
        const float *__restrict__ src = p.coarse + (size_t)c * cvox;
        float *__restrict__ out = p.fine + (size_t)c * vox + (size_t)yf * sx + (size_t)xf;
        const int z0 = tz * PRO_K, k0 = z0 >> 1;                        // z0 is even
        // The tile's PRO_K / 2 + 1 coarse planes (past the grid: the last one again, which the clamp wants or nothing
        // reads), two coarse rows of each, x-passed: e[j] is the fine row 2 y after the y pass, o[j] the row 2 y + 1.
        float4 e[PRO_K / 2 + 1], o[PRO_K / 2 + 1];
#pragma unroll
        for (int j = 0; j <= PRO_K / 2; j++) {
            const float *pl = src + (size_t)min(k0 + j, p.cz - 1) * cplane;
            const float4 ra = prolong_row(pl + j0, xq, p.cx), rb = prolong_row(pl + j1, xq, p.cx);
            e[j] = half_sum(ra, ra);
            o[j] = half_sum(ra, rb);
        }
#pragma unroll
        for (int j = 0; j < PRO_K / 2; j++) {
            const int z = z0 + 2 * j;
            if (z < p.nz) {
                prolong_store<VEC>(out + (size_t)z * plane, xf, p.nx, e[j], e[j]);
                if (odd_row)
                    prolong_store<VEC>(out + (size_t)z * plane + sx, xf, p.nx, o[j], o[j]);
            }
            if (z + 1 < p.nz) {
                prolong_store<VEC>(out + (size_t)(z + 1) * plane, xf, p.nx, e[j], e[j + 1]);
                if (odd_row)
                    prolong_store<VEC>(out + (size_t)(z + 1) * plane + sx, xf, p.nx, o[j], o[j + 1]);
            }
        }
    }
}

// lanes own `per_lane` x each on the tiled grid (x, y, z) of `chans` channels, `k` planes per tile
bool mr_tiles(int x, int y, int z, int per_lane, int k, int chans, MultiresTiles &g)
{
    const int lanes_x = (x + per_lane - 1) / per_lane;
    g.tiles_x = (lanes_x + MR_TX - 1) / MR_TX;
    g.tiles_y = (y + MR_TY - 1) / MR_TY;
    g.tiles_z = (z + k - 1) / k;
    const unsigned long long nt = (unsigned long long)g.tiles_x * g.tiles_y * g.tiles_z * (unsigned long long)chans;
    if (nt > 0xffffffffull - MR_MAX_GRID)
        return false;
    g.ntiles = (unsigned)nt;
    return true;
}

} // namespace

// Launchers for sift3d_multires.c, which has checked every argument (not exported from the library).
extern "C" int sift3d_restrict2_launch(const float *d_src, int nx, int ny, int nz, int nc, float *d_dst, float scale,
                                       void *stream)
{
    RestrictArgs p;
    p.src = d_src; p.dst = d_dst;
    p.nx = nx; p.ny = ny; p.nz = nz;
    p.cx = (nx + 1) / 2; p.cy = (ny + 1) / 2; p.cz = (nz + 1) / 2;
    p.scale = scale;
    if (!mr_tiles(p.cx, p.cy, p.cz, 2, RES_K, nc, p.g))
        return launch_fail("sift3d_hip_restrict2", "grid too large");
    // 16-byte loads and 8-byte stores: every fine row 16-byte aligned, every coarse row 8-byte aligned
    const bool vec = nx % 4 == 0 && !((uintptr_t)d_src & 15) && !((uintptr_t)d_dst & 7);
    const unsigned grid = p.g.ntiles < MR_MAX_GRID ? p.g.ntiles : MR_MAX_GRID;
    if (vec)
        hipLaunchKernelGGL(k_restrict2<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(k_restrict2<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

extern "C" int sift3d_field_prolong2_launch(const float *d_coarse, float *d_fine, int nx, int ny, int nz, void *stream)
{
    ProlongArgs p;
    p.coarse = d_coarse; p.fine = d_fine;
    p.nx = nx; p.ny = ny; p.nz = nz;
    p.cx = (nx + 1) / 2; p.cy = (ny + 1) / 2; p.cz = (nz + 1) / 2;
    if (!mr_tiles(nx, p.cy, nz, 4, PRO_K, 3, p.g))                 // a lane owns 4 x of two fine rows
        return launch_fail("sift3d_hip_field_prolong2", "grid too large");
    const bool vec = nx % 4 == 0 && !((uintptr_t)d_fine & 15);
    const unsigned grid = p.g.ntiles < MR_MAX_GRID ? p.g.ntiles : MR_MAX_GRID;
    if (vec)
        hipLaunchKernelGGL(k_field_prolong2<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(k_field_prolong2<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}
