// sift3d_resample.h -- the sampling and tiling core of the resampling kernels (sift3d_warp.hip, sift3d_bspline.hip,
// sift3d_demons.hip) and of the registration sum kernels (sift3d_similarity.hip, sift3d_affine_refine.hip,
// sift3d_ffd.hip).  Every kernel built from these pieces is reproduced bit for bit by a numpy restatement, so
// the order of the arithmetic below is part of the library's contract, and this is the one place that states it:
//
//   A (3 x 4, row-major) is a PULL map: output voxel (x, y, z) reads the source at
//     q_d = A[d][0]*x + ((A[d][1]*y + A[d][2]*z) + A[d][3])      (double, this order, no contraction)
//   inside  : 0 <= q_d <= n_d - 1 on every axis (a NaN is outside); outside voxels get `fill`;
//   linear  : i = floor(q), f = (float)(q - i), j = min(i + 1, n - 1), lerp(a, b, f) = a + f*(b - a)
//             in float, along x for the four (y, z) corner rows, then along y, then along z;
//   nearest : the value at floor(q + 0.5).
//
// Everything here is __device__ __forceinline__ or a plain inline host helper.  What the compiler made of each kernel
// before and after a piece moved here is on record: profiles/microbench/resample_refactor_mi355x.txt (the resampling
// kernels) and registration_front_end_mi355x.txt (the sum kernels).
#ifndef SIFT3D_RESAMPLE_H
#define SIFT3D_RESAMPLE_H

#include "sift3d_kernels_common.h"

// ---- grid and tile geometry -----------------------------------------------------------------------------------
//   - a lane gathers for 4 x outputs 16 apart, so that neighbouring lanes read neighbouring source addresses, and
//     after an exchange through LDS writes 4 consecutive x outputs with one 16-byte store (exchange_store);
//   - a 256-lane workgroup makes a 64 x 4 x 4 tile, compact in 3-D so that the source footprint of a rotated tile is
//     small and stays in L1 / L2 (a long x-row tile rotated about z or y would sweep a long diagonal of the source);
//   - tiles are numbered x fastest, and blocks are remapped so that each XCD (blocks b, b + 8, ... share one) works
//     on a contiguous run of tile numbers -- neighbouring tiles, overlapping source footprints, the same L2.
constexpr int TX = 64, TY = 4, TZ = 4;           // outputs per tile: 16 lanes x 4 in x, 4 rows, 4 planes
constexpr int NXCD = 8;
constexpr unsigned MAX_GRID = 1u << 20;          // blocks per pass over the tiles

struct GridArgs {
    const float *src;
    float *dst;
    int nx, ny, nz, ox, oy, oz;
    int tiles_x, tiles_y;
    unsigned ntiles;                             // < 2^32 - MAX_GRID (checked at launch)
    float fill;
    int vec;                                     // 16-byte stores (ox % 4 == 0, dst 16-byte aligned)
};

struct AffineArgs {                              // resampling through an affine pull map
    double a[12];
    GridArgs g;
};

struct FieldArgs {                               // resampling nc channels through a displacement field
    GridArgs g;
    const float *field;
    int nc;
};

// the tiling of an output grid; false when it has 2^32 - MAX_GRID tiles or more
static inline bool grid_args(GridArgs &p, const float *d_src, int nx, int ny, int nz, float *d_dst, int ox, int oy,
                             int oz, float fill)
{
    p.src = d_src;
    p.dst = d_dst;
    p.nx = nx; p.ny = ny; p.nz = nz;
    p.ox = ox; p.oy = oy; p.oz = oz;
    p.tiles_x = (ox + TX - 1) / TX;
    p.tiles_y = (oy + TY - 1) / TY;
    const unsigned long long nt = (unsigned long long)p.tiles_x * p.tiles_y * ((oz + TZ - 1) / TZ);
    if (nt > 0xffffffffull - MAX_GRID)
        return false;
    p.ntiles = (unsigned)nt;
    p.fill = fill;
    p.vec = (ox % 4 == 0) && !((uintptr_t)d_dst & 15);
    return true;
}

// block b of a pass of n blocks -> tile number within the pass: the blocks of one XCD (b % 8) get
// a contiguous run of tile numbers (bijective for any n; cdna_hip_programming T1)
__device__ __forceinline__ unsigned xcd_swizzle(unsigned b, unsigned n)
{
    const unsigned g = b % NXCD, k = b / NXCD, q = n / NXCD, r = n % NXCD;
    return g * q + (g < r ? g : r) + k;
}

// The walk over the tiles is `for (base = 0; base < p.ntiles; base += gridDim.x)`.  This block's tile of the pass
// at `base`: its x origin and the lane's row (y, z), which may lie past the grid; false when the pass has no tile
// for this block (uniform over the block, and so is every later pass).
__device__ __forceinline__ bool tile_at(const GridArgs &p, unsigned base, int &xt, int &y, int &z)
{
    const unsigned n = min(p.ntiles - base, gridDim.x);
    if (blockIdx.x >= n)
        return false;
    const unsigned t = base + xcd_swizzle(blockIdx.x, n);
    const unsigned tyz = t / (unsigned)p.tiles_x;
    const int tx = (int)(t - tyz * (unsigned)p.tiles_x);
    const int ty = (int)(tyz % (unsigned)p.tiles_y), tz = (int)(tyz / (unsigned)p.tiles_y);
    xt = tx * TX;
    y = ty * TY + (int)((threadIdx.x >> 4) & 3);
    z = tz * TZ + (int)(threadIdx.x >> 6);
    return true;
}

// A lane computed v[k] for x = xt + lx + 16 k (k = 0 .. 3, lx = lane & 15): the 16 lanes of a row gather from
// neighbouring source addresses in each load instruction (lanes 4 x apart would make every lane a request of its
// own).  The values are regrouped through LDS (xch: 256 float4 of the workgroup) so that the lane stores
// x0 = xt + 4 lx .. + 3 of its row with one 16-byte store, or one by one for the row tail when ox % 4 != 0, where the
// rows are not 16-byte aligned.  Every lane of the workgroup takes part; only `live` lanes store.
__device__ __forceinline__ void exchange_store(float4 *xch, const float v[4], float *out_row, int x0, bool live,
                                               int vec, int ox)
{
    float *xs = reinterpret_cast<float *>(xch) + (threadIdx.x & ~15) * 4;    // this row's 64 outputs
    const int lx = threadIdx.x & 15;
    __syncthreads();                                                         // previous exchange's reads done
#pragma unroll
    for (int k = 0; k < 4; k++)
        xs[lx + 16 * k] = v[k];
    __syncthreads();
    const float4 w = xch[threadIdx.x];
    if (!live)
        return;
    float *out = out_row + (size_t)x0;
    if (vec) {
        st4(out, w);
    } else {
        const float o[4] = {w.x, w.y, w.z, w.w};
        const int m = min(4, ox - x0);
#pragma nounroll
        for (int k = 0; k < m; k++)
            out[k] = o[k];
    }
}

// ---- the affine pull map: q_d = a[0]*x + ((a[1]*y + a[2]*z) + a[3]) for the row a = A + 4 d ----------------------
__device__ __forceinline__ double pull_row(const double *a, double y, double z) { return (a[1] * y + a[2] * z) + a[3]; }
__device__ __forceinline__ double pull(const double *a, double x, double row) { return a[0] * x + row; }

// ---- the trilinear (or nearest) sample, split into where to read (once per voxel) and the reads (once per channel)
// `&`, not `&&`: six compares and one mask, no branches (a NaN fails every compare)
__device__ __forceinline__ bool inside(double qx, double qy, double qz, int nx, int ny, int nz)
{
    return (qx >= 0.0) & (qx <= (double)(nx - 1)) & (qy >= 0.0) & (qy <= (double)(ny - 1)) & (qz >= 0.0) &
           (qz <= (double)(nz - 1));
}

__device__ __forceinline__ float lerp(float a, float b, float f) { return a + f * (b - a); }

// two neighbouring source elements with one 8-byte load (4-byte aligned: global_load_dwordx2)
typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));

struct Taps {
    size_t r00, r10, r01, r11;                   // row offsets of the four (y, z) corner rows (NEAREST: r00 + ix)
    int ix, jx, bx;
    bool hi, in;
    float fx, fy, fz;
};

// Branch-free: an outside sample reads voxel 0 and is replaced by `fill` at the end, so that the loads of all four
// outputs of a lane are in flight together instead of one output's behind each branch.  LINEAR == 0 is nearest.
// LINEAR == 2 is linear mode for nx >= 2: each (y, z) corner row gives the pair (ix, jx) with one 8-byte load at
// min(ix, nx - 2) -- the same two values as two single loads, half the load instructions.  LINEAR == 1 (nx == 1)
// loads them singly.
template <int LINEAR>
__device__ __forceinline__ Taps taps_at(int nx, int ny, int nz, double qx, double qy, double qz)
{
    Taps t;
    const bool in = inside(qx, qy, qz, nx, ny, nz);
    qx = in ? qx : 0.0;
    qy = in ? qy : 0.0;
    qz = in ? qz : 0.0;
    t.in = in;
    const size_t sx = (size_t)nx, sxy = (size_t)nx * (size_t)ny;
    if (!LINEAR) {
        const int ix = (int)floor(qx + 0.5), iy = (int)floor(qy + 0.5), iz = (int)floor(qz + 0.5);
        t.r00 = (size_t)iz * sxy + (size_t)iy * sx + (size_t)ix;
    } else {
        const double fx0 = floor(qx), fy0 = floor(qy), fz0 = floor(qz);
        const int ix = (int)fx0, iy = (int)fy0, iz = (int)fz0;
        t.fx = (float)(qx - fx0); t.fy = (float)(qy - fy0); t.fz = (float)(qz - fz0);
        const int jy = min(iy + 1, ny - 1), jz = min(iz + 1, nz - 1);
        t.r00 = (size_t)iz * sxy + (size_t)iy * sx; t.r10 = (size_t)iz * sxy + (size_t)jy * sx;
        t.r01 = (size_t)jz * sxy + (size_t)iy * sx; t.r11 = (size_t)jz * sxy + (size_t)jy * sx;
        if (LINEAR == 2) {
            t.bx = min(ix, nx - 2);                                          // ix == nx - 1: jx == ix, both = .y
            t.hi = ix != t.bx;
        } else {
            t.ix = ix;
            t.jx = min(ix + 1, nx - 1);
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
        float a00, b00, a10, b10, a01, b01, a11, b11;                       // values at (ix, jx) per corner row
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

// gather<LINEAR>'s value bit for bit (LINEAR 1 and 2 only; no fill: the caller tests t.in) and the derivative of the
// trilinear interpolant from the same eight corner values, no further loads.  Float, unfused, in gather's names:
//   gx = lerp(lerp(b00 - a00, b10 - a10, fy), lerp(b01 - a01, b11 - a11, fy), fz)
//   gy = lerp(c10 - c00, c11 - c01, fz)
//   gz = lerp(c01, c11, fy) - lerp(c00, c10, fy)
// On a clamped last plane (j == i: q on the grid's high face, or an axis of 1) both corners are one voxel and the
// difference along that axis is 0.  (gather itself is not built on this: its kernels compile as they did.)
template <int LINEAR>
__device__ __forceinline__ float gather_grad(const float *s, const Taps &t, float *gx, float *gy, float *gz)
{
    static_assert(LINEAR == 1 || LINEAR == 2, "gather_grad: linear modes only");
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
    const float c0 = lerp(c00, c10, t.fy), c1 = lerp(c01, c11, t.fy);
    *gx = lerp(lerp(b00 - a00, b10 - a10, t.fy), lerp(b01 - a01, b11 - a11, t.fy), t.fz);
    *gy = lerp(c10 - c00, c11 - c01, t.fz);
    *gz = c1 - c0;
    return lerp(c0, c1, t.fz);
}

template <int LINEAR>
__device__ __forceinline__ float sample(const GridArgs &p, double qx, double qy, double qz)
{
    return gather<LINEAR>(p.src, taps_at<LINEAR>(p.nx, p.ny, p.nz, qx, qy, qz), p.fill);
}

// ---- region-of-interest masks (contract: include/sift3d_amd.h, "Masks") ------------------------------------------
// A mask is a float volume on its grid; a voxel is in when w >= 0.5f (one compare: a NaN is out).  wf lies on the
// output grid and is read beside F; wm lies on the source grid and is read at the NEAREST voxel of the q that the
// intensity sample uses, whatever that sample's interpolation.  Either pointer may be null: all in.
struct MaskArgs {
    const float *wf, *wm;
};

__device__ __forceinline__ bool mask_in(float w) { return w >= 0.5f; }

// The offset of the source-grid mask voxel for a sample at q: the NEAREST taps of the same q, whatever the
// interpolation of the intensity sample, with taps_at's own clamp (the compiler keeps one copy of the inside test and
// the selects), so an outside q reads voxel 0 branch-free and needs no test before the load.
__device__ __forceinline__ size_t mask_offset(int nx, int ny, int nz, double qx, double qy, double qz)
{
    return taps_at<0>(nx, ny, nz, qx, qy, qz).r00;
}

// ---- the one-stage tile front-end of the registration sum kernels ---------------------------------------------------
// k_similarity, k_parzen_hist, k_ffd_force and k_ffd_mi_force walk the fixed grid F as the warps walk their output
// (tile_at) and reduce instead of storing.  For the lane's four outputs x = xt + lx + 16 k of row (y, z): F, W_F beside
// it, the sample point q (the affine pull map `a`, or FIELD: p + u(p) with u read from field [3][oz][oy][ox]), the
// taps of q on the moving grid and W_M at q's nearest voxel, every load issued before the caller's gathers.  An output
// past the grid reads neither F, nor the field, nor W_F (f = 0, u = 0, w = 1), samples inside M and is not counted.
// k_ffd_mi_force calls tile_front.  k_similarity, k_parzen_hist and k_ffd_force restate it in their own bodies (the
// last two with the field loaded before F): each compiled and wrote the same bytes on tile_front, and each had a timing
// line beyond the parent's spread there (profiles/microbench/registration_front_end_mi355x.txt; their comments).
// (The record kernels of sift3d_affine_refine.hip have no registers for the masks beside the gathers: tile_samples
// there is the two-stage form.)
struct TileFront {
    Taps tp[4];
    float f[4];
    float wf[4], wm[4];                          // MASKED only
    bool live[4];
    size_t orow;                                 // the row's offset on the fixed grid
};

template <int LINEAR, bool FIELD, bool MASKED>
__device__ __forceinline__ void tile_front(const GridArgs &p, const double *a, const float *field, const float *F,
                                           const MaskArgs &w, int xt, int y, int z, TileFront &t)
{
    const int lx = threadIdx.x & 15;
    const size_t ovox = (size_t)p.ox * (size_t)p.oy * (size_t)p.oz;             // FIELD only
    const bool row = y < p.oy && z < p.oz;
    const size_t orow = ((size_t)z * (size_t)p.oy + (size_t)y) * (size_t)p.ox;
    const double yd = (double)y, zd = (double)z;
    double rx = 0.0, ry = 0.0, rz = 0.0;
    if (!FIELD) {
        rx = pull_row(a, yd, zd);
        ry = pull_row(a + 4, yd, zd);
        rz = pull_row(a + 8, yd, zd);
    }
    t.orow = orow;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int x = xt + lx + 16 * k;
        t.live[k] = row && x < p.ox;
        t.f[k] = 0.0f;
        t.wf[k] = t.wm[k] = 1.0f;
        float ux = 0.0f, uy = 0.0f, uz = 0.0f;
        if (t.live[k]) {
            t.f[k] = F[orow + (size_t)x];
            if (MASKED && w.wf)
                t.wf[k] = w.wf[orow + (size_t)x];
            if (FIELD) {
                const float *u = field + orow + (size_t)x;
                ux = u[0];
                uy = u[ovox];
                uz = u[2 * ovox];
            }
        }
        const double xd = (double)x;
        const double qx = FIELD ? xd + (double)ux : pull(a, xd, rx);
        const double qy = FIELD ? yd + (double)uy : pull(a + 4, xd, ry);
        const double qz = FIELD ? zd + (double)uz : pull(a + 8, xd, rz);
        t.tp[k] = taps_at<LINEAR>(p.nx, p.ny, p.nz, qx, qy, qz);
        if (MASKED && w.wm)
            t.wm[k] = w.wm[mask_offset(p.nx, p.ny, p.nz, qx, qy, qz)];
    }
}

// output k of the tile enters the sums: on the grid, q inside the moving grid and, MASKED, in both masks
template <bool MASKED>
__device__ __forceinline__ bool tile_counted(const TileFront &t, int k)
{
    return MASKED ? t.live[k] && t.tp[k].in && mask_in(t.wf[k]) && mask_in(t.wm[k]) : t.live[k] && t.tp[k].in;
}

// ---- launch helpers of those kernels ----------------------------------------------------------------------------------
// min(tiles, SIFT3D_AMD_SIMILARITY_GRID) workgroups walk the tiles: the size does not depend on the device, so the bits
// of the sums depend on the shapes only
constexpr unsigned REDUCE_GRID = SIFT3D_AMD_SIMILARITY_GRID;
static inline unsigned reduce_grid(unsigned ntiles) { return ntiles < REDUCE_GRID ? ntiles : REDUCE_GRID; }

// K<LINEAR, MASKED, ...> for a linear sample of a moving grid nx wide (2: nx >= 2, 1: nx == 1), with masks or without
#define PICK_LINEAR_MASKED(K, nx, masked, ...)                                                                         \
    ((masked) ? ((nx) >= 2 ? K<2, true, ##__VA_ARGS__> : K<1, true, ##__VA_ARGS__>)                                    \
              : ((nx) >= 2 ? K<2, false, ##__VA_ARGS__> : K<1, false, ##__VA_ARGS__>))

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
//     launch covers a contiguous range of them.
// The device layout (sift3d_amd_tps_pack) holds per point {cx, cy, cz, 0, -wx, -wy, -wz, 0}: the sign of
// phi(r) = -r is folded into the weights, and s + (-w) * r is w * (-r) added to s, bit for bit.
constexpr int TPS_K = 8;                          // voxels per lane, along z
constexpr int TPS_TX = 64, TPS_TY = 4;            // a wave per row, 4 rows per workgroup

struct TpsArgs {
    double a[12];
    const float *tps;                            // 8 floats per point (sift3d_amd_tps_pack)
    float *dst;
    int m;
    int ox, oy, oz;
    int tiles_x, tiles_y;
    unsigned t0;                                 // this launch: tiles t0 .. t0 + gridDim.x - 1
};

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(4))) float *tps_cptr;    // constant address space: scalar loads

struct TpsSum {
    f32x2 sx[TPS_K / 2], sy[TPS_K / 2], sz[TPS_K / 2];    // s of the voxel pairs (z0 + 2 k, z0 + 2 k + 1)
};

// the lane's column (x, y), first plane z0 (lanes past the grid compute too) and the radial sums of its TPS_K voxels
__device__ __forceinline__ void tps_column(const TpsArgs &p, int &x, int &y, int &z0, TpsSum &s)
{
    const unsigned t = p.t0 + blockIdx.x;
    const unsigned tyz = t / (unsigned)p.tiles_x;
    const int tx = (int)(t - tyz * (unsigned)p.tiles_x);
    const int ty = (int)(tyz % (unsigned)p.tiles_y), tz = (int)(tyz / (unsigned)p.tiles_y);
    x = tx * TPS_TX + (int)(threadIdx.x & 63);
    y = ty * TPS_TY + (int)(threadIdx.x >> 6);
    z0 = tz * TPS_K;
    const float xf = (float)x, yf = (float)y;
    f32x2 zf[TPS_K / 2];
#pragma unroll
    for (int k = 0; k < TPS_K / 2; k++) {
        zf[k] = f32x2{(float)(z0 + 2 * k), (float)(z0 + 2 * k + 1)};
        s.sx[k] = s.sy[k] = s.sz[k] = f32x2{0.0f, 0.0f};
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
            s.sx[k] = s.sx[k] + wx * r;
            s.sy[k] = s.sy[k] + wy * r;
            s.sz[k] = s.sz[k] + wz * r;
        }
    }
}

// q of the column's voxel k (plane z0 + k): the affine part depends on z, so it is per voxel
__device__ __forceinline__ void tps_pull(const TpsArgs &p, const TpsSum &s, double xd, double yd, double zd, int k,
                                         double &qx, double &qy, double &qz)
{
    const float rx = (k & 1) ? s.sx[k / 2].y : s.sx[k / 2].x;
    const float ry = (k & 1) ? s.sy[k / 2].y : s.sy[k / 2].x;
    const float rz = (k & 1) ? s.sz[k / 2].y : s.sz[k / 2].x;
    qx = pull(p.a, xd, pull_row(p.a, yd, zd)) + (double)rx;
    qy = pull(p.a + 4, xd, pull_row(p.a + 4, yd, zd)) + (double)ry;
    qz = pull(p.a + 8, xd, pull_row(p.a + 8, yd, zd)) + (double)rz;
}

// ---- gradients and reductions ---------------------------------------------------------------------------------
__device__ __forceinline__ float grad(float lo, float c, float hi, int i, int n)
{
    // numpy.gradient: central difference inside, one-sided at the ends; an axis of length 1 has none
    return n == 1 ? 0.0f : i == 0 ? hi - c : i == n - 1 ? c - lo : (hi - lo) * 0.5f;
}

struct Add {
    template <typename T> static __device__ __forceinline__ T op(T a, T b) { return a + b; }
};
struct Min {
    static __device__ __forceinline__ int op(int a, int b) { return min(a, b); }
};
struct Max {
    static __device__ __forceinline__ int op(int a, int b) { return max(a, b); }
    static __device__ __forceinline__ double op(double a, double b) { return fmax(a, b); }
};

// One statistic of a 256-lane workgroup, in a fixed order: the wave by butterfly (s = 32 .. 1), then the four waves'
// values through slot[4] (LDS, one array per statistic) as ((s0 op s1) op s2) op s3.  Every lane calls it and gets
// the result.
template <typename Op, typename T>
__device__ __forceinline__ T workgroup_reduce(T v, T *slot)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1)
        v = Op::op(v, __shfl_xor(v, s));
    if ((threadIdx.x & 63) == 0)
        slot[threadIdx.x >> 6] = v;
    __syncthreads();
    return Op::op(Op::op(Op::op(slot[0], slot[1]), slot[2]), slot[3]);
}

// The partial slots part[0 .. n-1] of a grid, by one 256-lane workgroup in a fixed order: lane t takes slots
// t, t + 256, ... in turn, then the tree 128 .. 1 through s[256] (LDS, one array per statistic); lane 0 gets the result.
template <typename Op, typename T>
__device__ __forceinline__ T finish_reduce(const T *part, unsigned n, T *s)
{
    T a = 0;
    for (unsigned i = threadIdx.x; i < n; i += 256)
        a = Op::op(a, part[i]);
    s[threadIdx.x] = a;
    __syncthreads();
    for (unsigned h = 128; h >= 1; h >>= 1) {
        if (threadIdx.x < h)
            s[threadIdx.x] = Op::op(s[threadIdx.x], s[threadIdx.x + h]);
        __syncthreads();
    }
    return s[0];
}

#endif
