// sift3d_warp.hip -- resampling of a volume through an affine map, a thin-plate spline or a displacement field
// (the last step of registration), and the field kernels that go with it: export, Jacobian, composition.
//
// Upstream SIFT3D's registration tool resamples the moving image into the fixed image's grid once the affine is
// known.  This is that step on the device.  The arithmetic of the pull map and of the sample, the tiling and the
// reductions are sift3d_resample.h's, fixed so that a restatement in numpy reproduces every kernel here bit for bit
// (tests/test_warp.py and its neighbours).
//
// 4 B read + 4 B written per output voxel algorithmically; in fact 4 gathered 8-byte loads (linear: one per
// (y, z) corner row, the x pair) or 1 dword load (nearest) per voxel, most of them L1 / L2 hits.  The time
// follows the gather instructions and how many distinct addresses each carries, not HBM bytes
// (profiles/microbench/warp_rate_mi355x.txt).
#include "sift3d_resample.h"

#include <cmath>

namespace {

template <int LINEAR>
__global__ __launch_bounds__(256) void k_warp_affine(const AffineArgs q)
{
    const GridArgs &p = q.g;
    __shared__ float4 xch[256];
    const int lx = threadIdx.x & 15;
    for (unsigned base = 0; base < p.ntiles; base += gridDim.x) {
        int xt, y, z;
        if (!tile_at(p, base, xt, y, z))
            return;
        // the row part of q once per row (rows past the grid are computed and not stored: every lane takes part in
        // the exchange; sampling is branch-free and reads inside the source)
        const double yd = (double)y, zd = (double)z;
        const double rx = pull_row(q.a, yd, zd), ry = pull_row(q.a + 4, yd, zd), rz = pull_row(q.a + 8, yd, zd);
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double xd = (double)(xt + lx + 16 * k);
            v[k] = sample<LINEAR>(p, pull(q.a, xd, rx), pull(q.a + 4, xd, ry), pull(q.a + 8, xd, rz));
        }
        const int x0 = xt + 4 * lx;
        exchange_store(xch, v, p.dst + ((size_t)z * (size_t)p.oy + (size_t)y) * (size_t)p.ox, x0,
                       x0 < p.ox && y < p.oy && z < p.oz, p.vec, p.ox);
    }
}

// ---- thin-plate spline (sift3d_resample.h: tps_column, tps_pull) -----------------------------------------------
// A launch covers a contiguous range of tiles: whole z-slabs (z-ranges) whenever one slab fits the launch budget
// (tps_tiles_per_launch).
constexpr int TPS_TILE = TPS_TX * TPS_TY * TPS_K;
constexpr unsigned TPS_MAX_GRID = 1u << 24;       // blocks per launch
// launch budget: no launch is estimated above TPS_BUDGET_S at TPS_S_PER_VOXEL_POINT machine-wide (measured on an
// MI355X at 512^3: 0.54 ps for m = 256 .. 4096, profiles/microbench/tps_rate_mi355x.txt; rounded up)
constexpr double TPS_BUDGET_S = 50e-3;
constexpr double TPS_S_PER_VOXEL_POINT = 0.60e-12;

struct TpsWarpArgs : TpsArgs {
    const float *src;
    int nx, ny, nz;
    float fill;
};

template <int LINEAR>
__global__ __launch_bounds__(256) void k_warp_tps(const TpsWarpArgs p)
{
    // lanes past the grid compute (the source reads stay inside it: the sample is branch-free) and do not store
    int x, y, z0;
    TpsSum s;
    tps_column(p, x, y, z0, s);
    const double xd = (double)x, yd = (double)y;
    const bool col = x < p.ox && y < p.oy;
    float *out = p.dst + ((size_t)z0 * (size_t)p.oy + (size_t)y) * (size_t)p.ox + (size_t)x;
    const size_t plane = (size_t)p.oy * (size_t)p.ox;
#pragma unroll
    for (int k = 0; k < TPS_K; k++) {
        double qx, qy, qz;
        tps_pull(p, s, xd, yd, (double)(z0 + k), k, qx, qy, qz);
        const float v = gather<LINEAR>(p.src, taps_at<LINEAR>(p.nx, p.ny, p.nz, qx, qy, qz), p.fill);
        if (col && z0 + k < p.oz)
            out[(size_t)k * plane] = v;
    }
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
// store of a channel is one coalesced 256-byte access.  The TPS export (k_tps_field) is k_warp_tps with the sampling
// replaced by three plane stores.
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
            const double qx = pull(p.a, xd, pull_row(p.a, yd, zd));
            const double qy = pull(p.a + 4, xd, pull_row(p.a + 4, yd, zd));
            const double qz = pull(p.a + 8, xd, pull_row(p.a + 8, yd, zd));
            float *o = out + (size_t)k * plane;
            o[0] = (float)(qx - xd);
            o[vox] = (float)(qy - yd);
            o[2 * vox] = (float)(qz - zd);
        }
    }
}

// u_d = (float)((affine_d(p) + (double)s_d(p)) - (double)p_d); the three channels of a plane leave with one
// coalesced store each
__global__ __launch_bounds__(256) void k_tps_field(const TpsArgs p)
{
    int x, y, z0;
    TpsSum s;
    tps_column(p, x, y, z0, s);
    if (x >= p.ox || y >= p.oy)
        return;
    const double xd = (double)x, yd = (double)y;
    const size_t plane = (size_t)p.oy * (size_t)p.ox, vox = plane * (size_t)p.oz;
    float *out = p.dst + ((size_t)z0 * (size_t)p.oy + (size_t)y) * (size_t)p.ox + (size_t)x;
#pragma unroll
    for (int k = 0; k < TPS_K; k++) {
        const double zd = (double)(z0 + k);
        double qx, qy, qz;
        tps_pull(p, s, xd, yd, zd, k, qx, qy, qz);
        if (z0 + k < p.oz) {
            float *o = out + (size_t)k * plane;
            o[0] = (float)(qx - xd);
            o[vox] = (float)(qy - yd);
            o[2 * vox] = (float)(qz - zd);
        }
    }
}

// ---- resampling through a field ---------------------------------------------------------------------------------
// The lane's 4 outputs read their u (16 lanes of a row read 64 consecutive bytes of each plane), place their taps
// once and gather every channel with them
template <int LINEAR>
__global__ __launch_bounds__(256) void k_warp_field(const FieldArgs f)
{
    const GridArgs &p = f.g;
    __shared__ float4 xch[256];
    const int lx = threadIdx.x & 15;
    const size_t svox = (size_t)p.nx * (size_t)p.ny * (size_t)p.nz;
    const size_t ovox = (size_t)p.ox * (size_t)p.oy * (size_t)p.oz;
    for (unsigned base = 0; base < p.ntiles; base += gridDim.x) {
        int xt, y, z;
        if (!tile_at(p, base, xt, y, z))
            return;
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
            tp[k] = taps_at<LINEAR>(p.nx, p.ny, p.nz, (double)x + (double)ux, (double)y + (double)uy,
                                    (double)z + (double)uz);
        }
        const int x0 = xt + 4 * lx;
        for (int c = 0; c < f.nc; c++) {
            const float *s = p.src + (size_t)c * svox;
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; k++)
                v[k] = gather<LINEAR>(s, tp[k], p.fill);
            exchange_store(xch, v, p.dst + (size_t)c * ovox + orow, x0, row && x0 < p.ox, p.vec, p.ox);
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
    cnt = workgroup_reduce<Add>(cnt, s_cnt);
    kmn = workgroup_reduce<Min>(kmn, s_min);
    kmx = workgroup_reduce<Max>(kmx, s_max);
    if (threadIdx.x == 0) {
        if (cnt)
            atomicAdd(p.folded, cnt);
        if (kmn != 0x7f800000)
            atomicMin(p.kmin, kmn);
        if (kmx != (int)(0xff800000u ^ 0x7fffffffu))
            atomicMax(p.kmax, kmx);
    }
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

// ---- field composition (contract: include/sift3d_amd.h, "Field composition, exponential and inverse") -----------
// k_warp_field with the source u (3 channels) and the field v: the lane's 4 outputs read v (which also gives the
// add's operand: no extra read), place one set of taps each -- clamped onto u's grid only when outside -- and gather
// the three channels of u with them; the results leave through the same LDS exchange.  Statistics: per lane, per
// wave by butterfly, per workgroup through LDS into partial slot blockIdx.x; k_compose_finish combines the slots in a
// fixed order.  With statistics the grid is min(tiles, CMP_GRID) whatever the device, so the bits of the sum depend on
// the shapes; without, it is k_warp_field's.
constexpr unsigned CMP_GRID = SIFT3D_AMD_FIELD_WORK_BYTES / 32;    // slots: sum, max (double), two uint64 counts

struct ComposeArgs {
    GridArgs g;                                  // src = u, dst = out (may be null), grids, tiles, vec
    const float *v;
    double *psum, *pmax;                         // [CMP_GRID] each
    unsigned long long *pcnt, *pins;             // [CMP_GRID] each
};

template <int MODE, int LINEAR, bool STATS>
__global__ __launch_bounds__(256) void k_field_compose(const ComposeArgs f)
{
    const GridArgs &p = f.g;
    __shared__ float4 xch[256];
    __shared__ double s_sum[4], s_max[4];
    __shared__ unsigned long long s_cnt[4], s_ins[4];
    const int lx = threadIdx.x & 15;
    const size_t svox = (size_t)p.nx * (size_t)p.ny * (size_t)p.nz;
    const size_t ovox = (size_t)p.ox * (size_t)p.oy * (size_t)p.oz;
    const double hx = (double)(p.nx - 1), hy = (double)(p.ny - 1), hz = (double)(p.nz - 1);
    double lsum = 0.0, lmax = 0.0;
    unsigned long long lcnt = 0, lins = 0;
    for (unsigned base = 0; base < p.ntiles; base += gridDim.x) {
        int xt, y, z;
        if (!tile_at(p, base, xt, y, z))
            break;
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
            in[k] = inside(qx, qy, qz, p.nx, p.ny, p.nz);
            nan[k] = (qx != qx) | (qy != qy) | (qz != qz);
            if (!in[k]) {
                // nearest-edge extension; a NaN stays NaN and taps_at sends it to voxel 0 (the output is NaN)
                qx = qx < 0.0 ? 0.0 : qx > hx ? hx : qx;
                qy = qy < 0.0 ? 0.0 : qy > hy ? hy : qy;
                qz = qz < 0.0 ? 0.0 : qz > hz ? hz : qz;
            }
            tp[k] = taps_at<LINEAR>(p.nx, p.ny, p.nz, qx, qy, qz);
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
#pragma unroll
        for (int c = 0; c < 3; c++)
            exchange_store(xch, o[c], p.dst + (size_t)c * ovox + orow, x0, row && x0 < p.ox, p.vec, p.ox);
    }
    if (!STATS)
        return;
    lsum = workgroup_reduce<Add>(lsum, s_sum);
    lmax = workgroup_reduce<Max>(lmax, s_max);
    lcnt = workgroup_reduce<Add>(lcnt, s_cnt);
    lins = workgroup_reduce<Add>(lins, s_ins);
    if (threadIdx.x == 0) {
        f.psum[blockIdx.x] = lsum;
        f.pmax[blockIdx.x] = lmax;
        f.pcnt[blockIdx.x] = lcnt;
        f.pins[blockIdx.x] = lins;
    }
}

// the partial slots 0 .. n-1 in a fixed order (finish_reduce); the record is {sum, max, count, inside}
__global__ __launch_bounds__(256) void k_compose_finish(const ComposeArgs f, unsigned n, double *rec)
{
    __shared__ double s_sum[256], s_max[256];
    __shared__ unsigned long long s_cnt[256], s_ins[256];
    const double a = finish_reduce<Add>(f.psum, n, s_sum), m = finish_reduce<Max>(f.pmax, n, s_max);
    const unsigned long long b = finish_reduce<Add>(f.pcnt, n, s_cnt), c = finish_reduce<Add>(f.pins, n, s_ins);
    if (threadIdx.x == 0) {
        rec[0] = a;
        rec[1] = m;
        reinterpret_cast<unsigned long long *>(rec)[2] = b;
        reinterpret_cast<unsigned long long *>(rec)[3] = c;
    }
}

// dst = src * s per element (the exponential's w_0 = v * 2^-K); dst may be src
__global__ __launch_bounds__(256) void k_field_scale(float *dst, const float *src, size_t n, float s)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        dst[i] = src[i] * s;
}

// fills the TpsArgs of p and launches k over the tiles, in as many launches as the budget asks for
template <typename Args>
int tps_run(const char *fn, void (*k)(const Args), Args &p, float *d_dst, int ox, int oy, int oz, const double *A,
            const float *d_tps, int m, void *stream)
{
    for (int i = 0; i < 12; i++)
        p.a[i] = A[i];
    p.tps = d_tps;
    p.dst = d_dst;
    p.m = m;
    p.ox = ox; p.oy = oy; p.oz = oz;
    p.tiles_x = (ox + TPS_TX - 1) / TPS_TX;
    p.tiles_y = (oy + TPS_TY - 1) / TPS_TY;
    const unsigned long long nt = (unsigned long long)p.tiles_x * p.tiles_y * ((oz + TPS_K - 1) / TPS_K);
    if (nt > 0xffffffffull)
        return launch_fail(fn, "output grid too large");
    const unsigned long long chunk = tps_tiles_per_launch(ox, oy, m);
    for (unsigned long long t0 = 0; t0 < nt; t0 += chunk) {
        p.t0 = (unsigned)t0;
        hipLaunchKernelGGL(k, dim3((unsigned)(nt - t0 < chunk ? nt - t0 : chunk)), dim3(256), 0, (hipStream_t)stream, p);
        LAUNCH_CHECK();
    }
    return SIFT3D_SUCCESS;
}

} // namespace

extern "C" {

int sift3d_hip_warp_affine(const float *d_src, int nx, int ny, int nz, float *d_dst, int ox, int oy, int oz,
                           const double *A, int interp, float fill, void *stream)
{
    static const char fn[] = "sift3d_hip_warp_affine";
    if (!d_src || !d_dst || !A)
        return launch_fail(fn, "NULL argument");
    if (check_dims(fn, nx, ny, nz) || check_dims(fn, ox, oy, oz) || check_interp(fn, interp) || check_affine(fn, A))
        return SIFT3D_FAILURE;
    if (overlap(d_src, sizeof(float) * (size_t)nx * ny * nz, d_dst, sizeof(float) * (size_t)ox * oy * oz))
        return launch_fail(fn, "source and destination overlap");
    AffineArgs q;
    if (!grid_args(q.g, d_src, nx, ny, nz, d_dst, ox, oy, oz, fill))
        return launch_fail(fn, "output grid too large");
    for (int i = 0; i < 12; i++)
        q.a[i] = A[i];
    const unsigned grid = q.g.ntiles < MAX_GRID ? q.g.ntiles : MAX_GRID;
    void (*k)(const AffineArgs) = interp == SIFT3D_AMD_INTERP_NEAREST ? k_warp_affine<0>
                                  : nx >= 2                          ? k_warp_affine<2>
                                                                     : k_warp_affine<1>;
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, (hipStream_t)stream, q);
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
    static const char fn[] = "sift3d_hip_warp_tps";
    if (!d_src || !d_dst || !A || !d_tps)
        return launch_fail(fn, "NULL argument");
    if (check_dims(fn, nx, ny, nz) || check_dims(fn, ox, oy, oz))
        return SIFT3D_FAILURE;
    if (m < 1 || m > SIFT3D_AMD_TPS_MAX_POINTS)
        return launch_fail(fn, "the number of control points must be in [1, SIFT3D_AMD_TPS_MAX_POINTS]");
    if (check_interp(fn, interp) || check_affine(fn, A))
        return SIFT3D_FAILURE;
    if ((uintptr_t)d_tps & 15)
        return launch_fail(fn, "the control point records are not 16-byte aligned");
    {
        const size_t nd = sizeof(float) * (size_t)ox * oy * oz;
        if (overlap(d_src, sizeof(float) * (size_t)nx * ny * nz, d_dst, nd) ||
            overlap(d_tps, sizeof(float) * SIFT3D_AMD_TPS_FLOATS * (size_t)m, d_dst, nd))
            return launch_fail(fn, "the destination overlaps the source or the control points");
    }
    TpsWarpArgs p;
    p.src = d_src;
    p.nx = nx; p.ny = ny; p.nz = nz;
    p.fill = fill;
    void (*k)(const TpsWarpArgs) = interp == SIFT3D_AMD_INTERP_NEAREST ? k_warp_tps<0>
                                   : nx >= 2                          ? k_warp_tps<2>
                                                                      : k_warp_tps<1>;
    return tps_run(fn, k, p, d_dst, ox, oy, oz, A, d_tps, m, stream);
}

// ---- displacement fields ---------------------------------------------------------------------------------------
int sift3d_hip_affine_field(float *d_field, int ox, int oy, int oz, const double *A, void *stream)
{
    static const char fn[] = "sift3d_hip_affine_field";
    if (!d_field || !A)
        return launch_fail(fn, "NULL argument");
    if (check_dims(fn, ox, oy, oz) || check_affine(fn, A))
        return SIFT3D_FAILURE;
    AffineFieldArgs p;
    if (!field_tiles(ox, oy, oz, FLD_K, p.g))
        return launch_fail(fn, "output grid too large");
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
        return launch_fail(fn, "NULL argument");
    if (check_dims(fn, ox, oy, oz))
        return SIFT3D_FAILURE;
    if (m < 1 || m > SIFT3D_AMD_TPS_MAX_POINTS)
        return launch_fail(fn, "the number of control points must be in [1, SIFT3D_AMD_TPS_MAX_POINTS]");
    if (check_affine(fn, A))
        return SIFT3D_FAILURE;
    if ((uintptr_t)d_tps & 15)
        return launch_fail(fn, "the control point records are not 16-byte aligned");
    if (overlap(d_field, 3 * sizeof(float) * (size_t)ox * oy * oz, d_tps, sizeof(float) * SIFT3D_AMD_TPS_FLOATS * (size_t)m))
        return launch_fail(fn, "the field overlaps the control points");
    TpsArgs p;
    return tps_run(fn, k_tps_field, p, d_field, ox, oy, oz, A, d_tps, m, stream);
}

int sift3d_hip_warp_field(const float *d_src, int nx, int ny, int nz, int nc, const float *d_field, int ox, int oy,
                          int oz, float *d_dst, int interp, float fill, void *stream)
{
    static const char fn[] = "sift3d_hip_warp_field";
    if (!d_src || !d_field || !d_dst)
        return launch_fail(fn, "NULL argument");
    if (check_dims(fn, nx, ny, nz) || check_dims(fn, ox, oy, oz))
        return SIFT3D_FAILURE;
    if (nc < 1)
        return launch_fail(fn, "the number of channels must be positive");
    if (check_interp(fn, interp))
        return SIFT3D_FAILURE;
    if (((uintptr_t)d_src | (uintptr_t)d_field | (uintptr_t)d_dst) & 3)
        return launch_fail(fn, "a buffer is not 4-byte aligned");
    {
        const size_t ns = sizeof(float) * (size_t)nc * nx * ny * nz, no = sizeof(float) * (size_t)ox * oy * oz;
        if (overlap(d_dst, (size_t)nc * no, d_src, ns) || overlap(d_dst, (size_t)nc * no, d_field, 3 * no))
            return launch_fail(fn, "the destination overlaps the source or the field");
    }
    FieldArgs f;
    if (!grid_args(f.g, d_src, nx, ny, nz, d_dst, ox, oy, oz, fill))
        return launch_fail(fn, "output grid too large");
    f.field = d_field;
    f.nc = nc;
    const unsigned grid = f.g.ntiles < MAX_GRID ? f.g.ntiles : MAX_GRID;
    void (*k)(const FieldArgs) = interp == SIFT3D_AMD_INTERP_NEAREST ? k_warp_field<0>
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
        return launch_fail(fn, "NULL argument");
    if (check_dims(fn, ox, oy, oz))
        return SIFT3D_FAILURE;
    if ((uintptr_t)d_stats & 7)
        return launch_fail(fn, "the stats buffer is not 8-byte aligned");
    if (((uintptr_t)d_field | (uintptr_t)d_det) & 3)
        return launch_fail(fn, "a buffer is not 4-byte aligned");
    {
        const size_t no = sizeof(float) * (size_t)ox * oy * oz;
        if (overlap(d_stats, SIFT3D_AMD_JACOBIAN_STATS_BYTES, d_field, 3 * no) ||
            (d_det && (overlap(d_det, no, d_field, 3 * no) || overlap(d_det, no, d_stats, SIFT3D_AMD_JACOBIAN_STATS_BYTES))))
            return launch_fail(fn, "the outputs overlap the field or each other");
    }
    JacArgs p;
    if (!field_tiles(ox, oy, oz, JAC_K, p.g))
        return launch_fail(fn, "output grid too large");
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
    if (!grid_args(f.g, d_u, ux, uy, uz, d_out, ox, oy, oz, 0.0f))
        return launch_fail(fn, "output grid too large");
    const GridArgs &p = f.g;
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
