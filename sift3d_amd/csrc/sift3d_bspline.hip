// sift3d_bspline.hip -- cubic B-spline resampling: the prefilter (samples -> coefficients) and the 64-tap gathers
// through an affine pull map and through a displacement field.  Contract: include/sift3d_amd.h, "Cubic B-spline
// resampling"; restated in numpy by tests/bspline_restatement.py and reproduced bit for bit (tests/test_bspline.py).
//
// Prefilter.  Per axis a 33-tap symmetric FIR on the whole-sample mirror extension (the truncated two-sided
// exponential), every output a fixed expression of its line, so that no tiling shows in the result.  Three passes
// over HBM per channel (x: src -> coef, y: coef -> work, z: work -> coef), 8 B per voxel and pass algorithmically:
//   - k_bspline_x: a workgroup takes 64 x of 4 rows; a wave loads its row segment and the 16-sample halo on either
//     side (mirrored indices) into LDS, and a lane reads its 33 taps from there (consecutive lanes, consecutive words);
//   - k_bspline_s, the y and the z pass: lines `stride` apart, 64 of them side by side per workgroup, so that every
//     load and store is a coalesced 256-byte row; a tile is 32 outputs along the axis plus the halo in LDS (64 x 64
//     words), and a lane slides a 40-word register window over its 8 outputs.  The z pass sees the volume as nx*ny
//     lines side by side, the y pass as nz groups of nx.
// Gathers.  The tiles (64 x 4 x 4 outputs per 256-lane workgroup, a lane gathers for 4 x outputs 16 apart), tile
// order, XCD grouping, pull map and inside test of sift3d_resample.h.  The four x taps of a (y, z) tap row are one
// 16-byte load (4-byte aligned: global_load_dwordx4) whenever they are not mirrored (1 <= ix <= nx - 3), four dword
// loads otherwise.
#include "sift3d_resample.h"

#include <cmath>

namespace {

constexpr int H = SIFT3D_AMD_BSPLINE_H;
__constant__ float c_taps[H + 1] = SIFT3D_AMD_BSPLINE_TAPS;

// whole-sample mirror of any int j into [0, n)
__device__ __forceinline__ int mirror(int j, int n)
{
    if ((unsigned)j < (unsigned)n)
        return j;
    if (n == 1)
        return 0;
    const int P = 2 * n - 2;
    j %= P;
    if (j < 0)
        j += P;
    return j < n ? j : P - j;
}

// c[i] of the contract from the window w, w[H] = s[i], w[H -+ k] = s[m(i -+ k)]
template <typename W>
__device__ __forceinline__ float fir33(const W &w, int c)
{
    float acc = 0.0f;
#pragma unroll
    for (int k = H; k >= 1; k--)
        acc = acc + c_taps[k] * (w[c - k] + w[c + k]);
    return acc + c_taps[0] * w[c];
}

// ---- x pass ---------------------------------------------------------------------------------------------------
constexpr int PX = 64, PR = 4;

__global__ __launch_bounds__(256) void k_bspline_x(const float *__restrict__ src, float *__restrict__ dst, int nx,
                                                   unsigned long long nrows, unsigned tiles_x,
                                                   unsigned long long ntiles)
{
    __shared__ float line[PR][PX + 2 * H];
    const int lx = threadIdx.x & 63, lr = threadIdx.x >> 6;
    for (unsigned long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const unsigned long long tr = t / tiles_x;
        const int x0 = (int)(t - tr * tiles_x) * PX;
        const unsigned long long row = tr * PR + lr;
        __syncthreads();                                                     // previous tile's reads done
        if (row < nrows) {
            const float *s = src + (size_t)row * (size_t)nx;
            for (int j = lx; j < PX + 2 * H; j += 64)
                line[lr][j] = s[mirror(x0 - H + j, nx)];
        }
        __syncthreads();
        const int x = x0 + lx;
        if (row < nrows && x < nx)
            dst[(size_t)row * (size_t)nx + (size_t)x] = fir33(line[lr], lx + H);
    }
}

// ---- y / z pass -----------------------------------------------------------------------------------------------
constexpr int SA = 32, SK = 8;                   // outputs along the axis per tile / per lane

struct StrideArgs {
    const float *src;
    float *dst;
    size_t inner, stride, ostride;               // lines side by side; samples of a line / groups of lines apart
    int n;                                       // samples per line
    unsigned long long tiles_i, tiles_a, ntiles;
};

__global__ __launch_bounds__(256) void k_bspline_s(const StrideArgs p)
{
    __shared__ float tile[SA + 2 * H][64];
    const int li = threadIdx.x & 63, g = threadIdx.x >> 6;
    for (unsigned long long t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
        const unsigned long long rest = t / p.tiles_i;
        const size_t i = (size_t)(t - rest * p.tiles_i) * 64 + (size_t)li;
        const unsigned long long o = rest / p.tiles_a;
        const int a0 = (int)(rest - o * p.tiles_a) * SA;
        const size_t base = (size_t)o * p.ostride + i;
        __syncthreads();                                                     // previous tile's reads done
        if (i < p.inner) {
#pragma unroll 4
            for (int j = g; j < SA + 2 * H; j += 4)
                tile[j][li] = p.src[base + (size_t)mirror(a0 - H + j, p.n) * p.stride];
        }
        __syncthreads();
        if (i >= p.inner)
            continue;
        float w[SK + 2 * H];
#pragma unroll
        for (int j = 0; j < SK + 2 * H; j++)
            w[j] = tile[g * SK + j][li];
#pragma unroll
        for (int u = 0; u < SK; u++) {
            const int a = a0 + g * SK + u;
            const float v = fir33(w, u + H);
            if (a < p.n)
                p.dst[base + (size_t)a * p.stride] = v;
        }
    }
}

// ---- sampling ---------------------------------------------------------------------------------------------------
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

constexpr float C6 = 0x1.555556p-3f, C23 = 0x1.555556p-1f;

__device__ __forceinline__ void weights(float f, float w[4])
{
    const float g = 1.0f - f;
    w[0] = ((g * g) * g) * C6;
    w[1] = C23 - (0.5f * (f * f)) * (2.0f - f);
    w[2] = C23 - (0.5f * (g * g)) * (2.0f - g);
    w[3] = ((f * f) * f) * C6;
}

__device__ __forceinline__ float dot4(const float w[4], float a0, float a1, float a2, float a3)
{
    return ((w[0] * a0 + w[1] * a1) + w[2] * a2) + w[3] * a3;
}

// where to read and with which weights: once per output voxel (p.src holds the coefficients)
struct CubicTaps {
    size_t ry[4], rz[4];                         // offsets of the four tap rows / planes
    int xt[4];                                   // the four x taps; xt[0] = ix - 1 on the fast path
    float wx[4], wy[4], wz[4];
    bool fast, in;
};

__device__ __forceinline__ CubicTaps cubic_taps_at(const GridArgs &p, double qx, double qy, double qz)
{
    CubicTaps t;
    const bool in = inside(qx, qy, qz, p.nx, p.ny, p.nz);                    // an outside sample reads around voxel 0
    qx = in ? qx : 0.0;
    qy = in ? qy : 0.0;
    qz = in ? qz : 0.0;
    t.in = in;
    const double fx0 = floor(qx), fy0 = floor(qy), fz0 = floor(qz);
    const int ix = (int)fx0, iy = (int)fy0, iz = (int)fz0;
    weights((float)(qx - fx0), t.wx);
    weights((float)(qy - fy0), t.wy);
    weights((float)(qz - fz0), t.wz);
    const size_t sx = (size_t)p.nx, sxy = (size_t)p.nx * (size_t)p.ny;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        t.xt[j] = mirror(ix - 1 + j, p.nx);
        t.ry[j] = (size_t)mirror(iy - 1 + j, p.ny) * sx;
        t.rz[j] = (size_t)mirror(iz - 1 + j, p.nz) * sxy;
    }
    t.fast = (ix >= 1) & (ix <= p.nx - 3);       // ix - 1 .. ix + 2 inside the row: no tap is mirrored
    return t;
}

__device__ __forceinline__ float cubic_gather(const float *__restrict__ s, const CubicTaps &t, float fill)
{
    float r[4][4];
    if (t.fast) {
#pragma unroll
        for (int jz = 0; jz < 4; jz++)
#pragma unroll
            for (int jy = 0; jy < 4; jy++) {
                const f32x4u a = *reinterpret_cast<const f32x4u *>(s + t.rz[jz] + t.ry[jy] + (size_t)t.xt[0]);
                r[jz][jy] = dot4(t.wx, a.x, a.y, a.z, a.w);
            }
    } else {
#pragma unroll
        for (int jz = 0; jz < 4; jz++)
#pragma unroll
            for (int jy = 0; jy < 4; jy++) {
                const float *row = s + t.rz[jz] + t.ry[jy];
                r[jz][jy] = dot4(t.wx, row[t.xt[0]], row[t.xt[1]], row[t.xt[2]], row[t.xt[3]]);
            }
    }
    float sz[4];
#pragma unroll
    for (int jz = 0; jz < 4; jz++)
        sz[jz] = dot4(t.wy, r[jz][0], r[jz][1], r[jz][2], r[jz][3]);
    const float v = dot4(t.wz, sz[0], sz[1], sz[2], sz[3]);
    return t.in ? v : fill;
}

// k_warp_affine (sift3d_warp.hip) with the cubic sample
__global__ __launch_bounds__(256) void k_bspline_warp_affine(const AffineArgs q)
{
    const GridArgs &p = q.g;
    __shared__ float4 xch[256];
    const int lx = threadIdx.x & 15;
    for (unsigned base = 0; base < p.ntiles; base += gridDim.x) {
        int xt, y, z;
        if (!tile_at(p, base, xt, y, z))
            return;
        // rows past the grid are computed and not stored: every lane takes part in the exchange, and every sample
        // reads inside the source
        const double yd = (double)y, zd = (double)z;
        const double rx = pull_row(q.a, yd, zd), ry = pull_row(q.a + 4, yd, zd), rz = pull_row(q.a + 8, yd, zd);
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double xd = (double)(xt + lx + 16 * k);
            const CubicTaps tp = cubic_taps_at(p, pull(q.a, xd, rx), pull(q.a + 4, xd, ry), pull(q.a + 8, xd, rz));
            v[k] = cubic_gather(p.src, tp, p.fill);
        }
        const int x0 = xt + 4 * lx;
        exchange_store(xch, v, p.dst + ((size_t)z * (size_t)p.oy + (size_t)y) * (size_t)p.ox, x0,
                       x0 < p.ox && y < p.oy && z < p.oz, p.vec, p.ox);
    }
}

// The same tiles and tile order.  A lane places the taps and weights of one output (44 registers) and gathers every
// channel with them before it turns to its next output; the values leave as dword stores, 16 lanes of a row writing
// 64 consecutive bytes (holding the taps of all 4 outputs for a 16-byte store would cost 4 x 44 registers, and the
// stores are 1 in 17 of the memory instructions).
__global__ __launch_bounds__(256) void k_bspline_warp_field(const FieldArgs f)
{
    const GridArgs &p = f.g;
    const int lx = threadIdx.x & 15;
    const size_t svox = (size_t)p.nx * (size_t)p.ny * (size_t)p.nz;
    const size_t ovox = (size_t)p.ox * (size_t)p.oy * (size_t)p.oz;
    for (unsigned base = 0; base < p.ntiles; base += gridDim.x) {
        int xt, y, z;
        if (!tile_at(p, base, xt, y, z))
            return;
        if (y >= p.oy || z >= p.oz)
            continue;
        const size_t orow = ((size_t)z * (size_t)p.oy + (size_t)y) * (size_t)p.ox;
#pragma nounroll
        for (int k = 0; k < 4; k++) {
            const int x = xt + lx + 16 * k;
            if (x >= p.ox)
                break;
            const float *u = f.field + orow + (size_t)x;
            const float ux = u[0], uy = u[ovox], uz = u[2 * ovox];
            const CubicTaps tp = cubic_taps_at(p, (double)x + (double)ux, (double)y + (double)uy, (double)z + (double)uz);
            float *out = p.dst + orow + (size_t)x;
            for (int c = 0; c < f.nc; c++)
                out[(size_t)c * ovox] = cubic_gather(p.src + (size_t)c * svox, tp, p.fill);
        }
    }
}

int pass_x(const float *src, float *dst, int nx, int ny, int nz, hipStream_t st)
{
    const unsigned long long nrows = (unsigned long long)ny * nz;
    const unsigned tiles_x = (unsigned)((nx + PX - 1) / PX);
    const unsigned long long ntiles = (unsigned long long)tiles_x * ((nrows + PR - 1) / PR);
    const unsigned grid = ntiles < MAX_GRID ? (unsigned)ntiles : MAX_GRID;
    hipLaunchKernelGGL(k_bspline_x, dim3(grid), dim3(256), 0, st, src, dst, nx, nrows, tiles_x, ntiles);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

int pass_s(const float *src, float *dst, size_t inner, int n, size_t outer, hipStream_t st)
{
    StrideArgs p;
    p.src = src;
    p.dst = dst;
    p.inner = inner;
    p.stride = inner;
    p.ostride = inner * (size_t)n;
    p.n = n;
    p.tiles_i = (inner + 63) / 64;
    p.tiles_a = (unsigned long long)((n + SA - 1) / SA);
    p.ntiles = p.tiles_i * p.tiles_a * outer;
    const unsigned grid = p.ntiles < MAX_GRID ? (unsigned)p.ntiles : MAX_GRID;
    hipLaunchKernelGGL(k_bspline_s, dim3(grid), dim3(256), 0, st, p);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

} // namespace

// Launchers for sift3d_bspline.c, which has checked every argument (not exported from the library).
extern "C" {

int sift3d_bspline_prefilter_launch(const float *d_src, int nx, int ny, int nz, int nc, float *d_coef, float *d_work,
                                    void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)nx * ny * nz;
    const int passes = (nx > 1) + (ny > 1) + (nz > 1);
    for (int c = 0; c < nc; c++) {
        const float *s = d_src + (size_t)c * n;
        float *d = d_coef + (size_t)c * n;
        if (passes == 0) {
            HIPCHK(hipMemcpyAsync(d, s, n * sizeof(float), hipMemcpyDeviceToDevice, st));
            continue;
        }
        // the last pass writes d: with two passes the first goes through the work buffer, with three the second
        float *to[3] = {d, d, d};
        if (passes == 2)
            to[0] = d_work;
        if (passes == 3)
            to[1] = d_work;
        const float *from = s;
        int k = 0;
        if (nx > 1) {
            if (pass_x(from, to[k], nx, ny, nz, st))
                return SIFT3D_FAILURE;
            from = to[k++];
        }
        if (ny > 1) {
            if (pass_s(from, to[k], (size_t)nx, ny, (size_t)nz, st))
                return SIFT3D_FAILURE;
            from = to[k++];
        }
        if (nz > 1) {
            if (pass_s(from, to[k], (size_t)nx * ny, nz, 1, st))
                return SIFT3D_FAILURE;
        }
    }
    return SIFT3D_SUCCESS;
}

int sift3d_bspline_warp_affine_launch(const float *d_coef, int nx, int ny, int nz, float *d_dst, int ox, int oy, int oz,
                                      const double *A, float fill, void *stream)
{
    AffineArgs q;
    if (!grid_args(q.g, d_coef, nx, ny, nz, d_dst, ox, oy, oz, fill))
        return launch_fail("sift3d_hip_bspline_warp_affine", "output grid too large");
    for (int i = 0; i < 12; i++)
        q.a[i] = A[i];
    const unsigned grid = q.g.ntiles < MAX_GRID ? q.g.ntiles : MAX_GRID;
    hipLaunchKernelGGL(k_bspline_warp_affine, dim3(grid), dim3(256), 0, (hipStream_t)stream, q);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

int sift3d_bspline_warp_field_launch(const float *d_coef, int nx, int ny, int nz, int nc, const float *d_field, int ox,
                                     int oy, int oz, float *d_dst, float fill, void *stream)
{
    FieldArgs f;
    if (!grid_args(f.g, d_coef, nx, ny, nz, d_dst, ox, oy, oz, fill))
        return launch_fail("sift3d_hip_bspline_warp_field", "output grid too large");
    f.field = d_field;
    f.nc = nc;
    const unsigned grid = f.g.ntiles < MAX_GRID ? f.g.ntiles : MAX_GRID;
    hipLaunchKernelGGL(k_bspline_warp_field, dim3(grid), dim3(256), 0, (hipStream_t)stream, f);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

} // extern "C"
