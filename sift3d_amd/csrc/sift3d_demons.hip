// sift3d_demons.hip -- the per-voxel force of the dense demons refinement and the field update (contract:
// include/sift3d_amd.h, "Dense demons refinement").  The iteration that chains them with warp_field and the
// detector's blur is host code (sift3d_demons.c), which checks every argument before it calls a launcher here.
//
// k_demons_force reads F and W (nc channels each) in a 7-point stencil, u once, and writes delta: at nc = 12,
// 48 + 48 + 12 B read and 12 B written per voxel.  A 256-lane workgroup is 64 x 4 (x, y) columns, a wave 64
// consecutive x of one row, a lane DEM_K planes of its column.  Channels are the outer loop and the lane's planes the
// inner, unrolled: the planes z0 - 1 .. z0 + DEM_K of a channel are loaded once and serve as centres and z
// neighbours; the x neighbours come from the neighbouring lanes by DPP shifts (the wave's end lanes load theirs);
// so a channel costs 3 + 3 DEM_K loads per DEM_K planes instead of 14 per plane.  The channel loop is
// software-pipelined: channel c + 1's loads issue before channel c's f64 sums, whose five accumulators per plane stay
// in registers across the channels.  Tiles are numbered z fastest and each workgroup takes a contiguous run, so
// the planes a tile shares with the tile below come from cache.  Statistics: per lane in double, per wave by
// butterfly, per workgroup through LDS into partial slot blockIdx.x; k_demons_finish adds the slots in a fixed
// order.  The grid is min(tiles, DEM_GRID) workgroups whatever the device, so the bits of the sum depend on the
// shape alone.
//
// k_demons_force<true> is the masked force (contract: "Masks in demons"): W_F is read beside u, W_M gathered at q's
// nearest voxel (mask_offset: an outside q reads voxel 0, no branch), and a plane is counted when it is inside and in
// both masks.  The tile loop has no barrier and a wave's DPP neighbours are its own lanes, so a wave none of whose
// lanes has a counted plane in the tile writes its zeros and skips the channel loop: it reads u and W_F (and W_M) only.
// The flags are needed before the first channel's loads for that, so <true> waits for u where <false> does not.  For
// the skipped work to shorten the kernel, <true> also deals the runs of tiles to the XCDs in rotation (below).
// <false> is the unmasked kernel's code unchanged.
#include "sift3d_resample.h"

namespace {

constexpr int DEM_TX = 64, DEM_TY = 4, DEM_K = 2;    // planes per lane: 2 beat 4
constexpr unsigned DEM_GRID = SIFT3D_AMD_DEMONS_FORCE_WORK_BYTES / 16;    // partial slots: double + uint64
// the masked kernel's wave-uniform skip: 2 (the default) with the runs of tiles dealt to the XCDs in rotation, 1
// without the rotation, 0 compiles the skip out (-DSIFT3D_DEMONS_MASK_SKIP=n; profiles/microbench/demons_mask_rate.py)
#ifndef SIFT3D_DEMONS_MASK_SKIP
#define SIFT3D_DEMONS_MASK_SKIP 2
#endif

struct ForceArgs {
    const float *F, *W, *u;
    float *step;
    double *psum;                                // [DEM_GRID]
    unsigned long long *pcnt;                    // [DEM_GRID]
    double a2;
    int nx, ny, nz, mx, my, mz, nc;
    int tiles_x, tiles_z;
    unsigned ntiles;
    const float *wf, *wm;                        // <true> only: the masks, either may be null (all in)
};

// the value of lane - 1 (SR) or lane + 1 (SL) of the wave; the wave's first (last) lane gets `edge`
__device__ __forceinline__ float from_left(float v, float edge)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float from_right(float v, float edge)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x130, 0xf, 0xf, false));
}

// One channel's loads for a lane's DEM_K planes.  f[j], w[j]: the centre at plane z0 - 1 + j (j = 0 .. DEM_K + 1;
// planes off the grid or past the lane's last are not loaded and hold 0, which no derivative reads: numpy.gradient's
// one-sided ends do not look past the grid).  fym .. wyp: the y neighbours (clamped) per plane; ef, ew: one load per
// plane in which lane 0 reads its x - 1 and lane 63 its x + 1 (the x neighbours across the wave's ends; the other
// lanes read their own centre, which is not used).
struct ChanLoads {
    float f[DEM_K + 2], w[DEM_K + 2];
    float fym[DEM_K], fyp[DEM_K], wym[DEM_K], wyp[DEM_K];
    float ef[DEM_K], ew[DEM_K];
};

__device__ __forceinline__ void load_channel(const ForceArgs &p, const float *__restrict__ Fb,
                                             const float *__restrict__ Wb, int c, size_t col, int z0, int nk,
                                             ptrdiff_t dxe, ptrdiff_t dym, ptrdiff_t dyp, size_t plane,
                                             size_t vox, ChanLoads &L)
{
    const float *f = Fb + (size_t)c * vox + col + (size_t)z0 * plane;
    const float *w = Wb + (size_t)c * vox + col + (size_t)z0 * plane;
#pragma unroll
    for (int j = 0; j < DEM_K + 2; j++) {
        const int z = z0 - 1 + j;
        L.f[j] = L.w[j] = 0.0f;
        if (j <= nk + 1 && z >= 0 && z < p.nz) {
            const ptrdiff_t o = (ptrdiff_t)(j - 1) * (ptrdiff_t)plane;
            L.f[j] = f[o];
            L.w[j] = w[o];
        }
    }
#pragma unroll
    for (int k = 0; k < DEM_K; k++) {
        L.fym[k] = L.fyp[k] = L.wym[k] = L.wyp[k] = 0.0f;
        L.ef[k] = L.ew[k] = 0.0f;
        if (k < nk) {
            const ptrdiff_t o = (ptrdiff_t)k * (ptrdiff_t)plane;
            L.fym[k] = f[o - dym];
            L.fyp[k] = f[o + dyp];
            L.wym[k] = w[o - dym];
            L.wyp[k] = w[o + dyp];
            L.ef[k] = f[o + dxe];
            L.ew[k] = w[o + dxe];
        }
    }
}

template <bool MASKED>
__global__ __launch_bounds__(256) void k_demons_force(const ForceArgs p)
{
    __shared__ double s_sum[4];
    __shared__ unsigned long long s_cnt[4];
    const float *__restrict__ Fb = p.F;
    const float *__restrict__ Wb = p.W;
    const float *__restrict__ ub = p.u;
    float *__restrict__ out = p.step;
    const size_t sx = (size_t)p.nx, plane = (size_t)p.ny * sx, vox = plane * (size_t)p.nz;
    double lsum = 0.0;
    unsigned long long lcnt = 0;
    // tiles numbered z fastest, each workgroup a contiguous run of them: it walks its columns up in z, so the
    // planes a tile shares with the one below (its z - 1 and z0 planes) were read by the same workgroup just before
    // and come from cache, not HBM (numbered x fastest, as k_jacobian_det's, they were read twice from HBM)
    const unsigned per = (p.ntiles + gridDim.x - 1) / gridDim.x;
    // The run of tiles, and the partial slot, of this workgroup.  <true>: consecutive workgroups go to consecutive XCDs
    // (8) and consecutive runs are z stretches of one column, so XCD k would get the same stretches of every column,
    // and under a compact region of interest the XCDs of the middle stretches would do all the work while the others skip
    // theirs (measured at 256^3: a mask in for z < nz / 2 saved nothing).  Rotating each aligned group of 8 runs deals
    // every stretch to every XCD.  The rotation steps once per band of 4 tile rows (16 y): rotating by the group's own
    // index also balanced, but put the runs of neighbouring tile rows, which share their edge rows in L2, on different
    // XCDs and cost the all-in mask 6 %.  A permutation of the runs: each slot still holds its own run's sums, so the
    // 8 XCDs and their round-robin dispatch are an assumption about time only, never about the bytes.
    unsigned blk = blockIdx.x;
    if (MASKED && SIFT3D_DEMONS_MASK_SKIP == 2 && (blk | 7u) < gridDim.x) {
        const unsigned ty_g = ((blk & ~7u) * per) / ((unsigned)p.tiles_z * (unsigned)p.tiles_x);
        blk = (blk & ~7u) | ((blk + (ty_g >> 2)) & 7u);
    }
    const unsigned t_end = min(p.ntiles, blk * per + per);
    for (unsigned t = blk * per; t < t_end; t++) {
        const unsigned txy = t / (unsigned)p.tiles_z;
        const int tz = (int)(t - txy * (unsigned)p.tiles_z);
        const int tx = (int)(txy % (unsigned)p.tiles_x), ty = (int)(txy / (unsigned)p.tiles_x);
        const int x = tx * DEM_TX + (int)(threadIdx.x & 63);
        const int y = ty * DEM_TY + (int)(threadIdx.x >> 6);
        const int z0 = tz * DEM_K;
        const int lane = (int)(threadIdx.x & 63);
        if (x >= p.nx || y >= p.ny)
            continue;
        const size_t col = (size_t)y * sx + (size_t)x;
        // the x neighbour a wave's end lane loads (clamped; 0 elsewhere), the y neighbour offsets (clamped)
        const ptrdiff_t dxe = lane == 0 ? (x > 0 ? -1 : 0) : lane == 63 ? (x + 1 < p.nx ? 1 : 0) : 0;
        const ptrdiff_t dym = y > 0 ? (ptrdiff_t)sx : 0, dyp = y + 1 < p.ny ? (ptrdiff_t)sx : 0;
        const int nk = min(DEM_K, p.nz - z0);                                // uniform over the workgroup
        bool in[DEM_K];
        double n0[DEM_K], n1[DEM_K], n2[DEM_K], sg[DEM_K], sd[DEM_K];
#pragma unroll
        for (int k = 0; k < DEM_K; k++) {
            in[k] = false;
            n0[k] = n1[k] = n2[k] = sg[k] = sd[k] = 0.0;
            if (k < nk) {
                const int z = z0 + k;
                const size_t o = (size_t)z * plane + col;
                const float ux = ub[o], uy = ub[o + vox], uz = ub[o + 2 * vox];
                const double qx = (double)x + (double)ux, qy = (double)y + (double)uy;
                const double qz = (double)z + (double)uz;
                in[k] = inside(qx, qy, qz, p.mx, p.my, p.mz);                // warp_field's (a NaN is outside)
                if (MASKED) {
                    // W_F beside u; W_M at q's nearest voxel (voxel 0 for an outside q: the inside test decides)
                    const float wf = p.wf ? p.wf[o] : 1.0f;
                    const float wm = p.wm ? p.wm[mask_offset(p.mx, p.my, p.mz, qx, qy, qz)] : 1.0f;
                    in[k] = in[k] && mask_in(wf) && mask_in(wm);
                }
            }
        }
        // <true>, wave-uniform: when no lane of the wave counts a plane of this tile, nothing of the channel loop is
        // used: no channel is run, the sums stay 0.0 and the stores below write the zeros
        int ncr = p.nc;
        if (MASKED && SIFT3D_DEMONS_MASK_SKIP) {
            bool any = false;
#pragma unroll
            for (int k = 0; k < DEM_K; k++)
                any = any || in[k];
            if (__ballot(any) == 0ull)
                ncr = 0;
        }
        // Channels outer, the lane's planes inner: the planes z0 - 1 .. z0 + DEM_K of a channel are loaded once and
        // serve as centres and z neighbours.  Software-pipelined over the channels: channel c + 1's loads are issued
        // before channel c's f64 sums, so a wave has two channels' loads in flight.  Voxels outside are computed too
        // (every address is on the fixed grid) and masked at the end.
        ChanLoads cur, nxt;
        if (!MASKED || ncr > 0)
            load_channel(p, Fb, Wb, 0, col, z0, nk, dxe, dym, dyp, plane, vox, cur);
        for (int c = 0; c < ncr; c++) {
            if (c + 1 < ncr)
                load_channel(p, Fb, Wb, c + 1, col, z0, nk, dxe, dym, dyp, plane, vox, nxt);
#pragma unroll
            for (int k = 0; k < DEM_K; k++) {
                if (k < nk) {
                    const int z = z0 + k;
                    const float fl = cur.f[k], fc = cur.f[k + 1], fh = cur.f[k + 2];
                    const float wl = cur.w[k], wc = cur.w[k + 1], wh = cur.w[k + 2];
                    // x neighbours from the neighbouring lanes (a wave is 64 consecutive x of one row); the
                    // wave's end lanes loaded theirs.  A lane past the grid's end feeds only the last voxel of the
                    // row, whose derivative does not read it.
                    const float fxm = from_left(fc, cur.ef[k]), fxp = from_right(fc, cur.ef[k]);
                    const float wxm = from_left(wc, cur.ew[k]), wxp = from_right(wc, cur.ew[k]);
                    const float d = fc - wc;
                    const float g0 = 0.5f * (grad(fxm, fc, fxp, x, p.nx) + grad(wxm, wc, wxp, x, p.nx));
                    const float g1 = 0.5f * (grad(cur.fym[k], fc, cur.fyp[k], y, p.ny) +
                                             grad(cur.wym[k], wc, cur.wyp[k], y, p.ny));
                    const float g2 = 0.5f * (grad(fl, fc, fh, z, p.nz) + grad(wl, wc, wh, z, p.nz));
                    const double dd = (double)d;
                    n0[k] = n0[k] + dd * (double)g0;
                    n1[k] = n1[k] + dd * (double)g1;
                    n2[k] = n2[k] + dd * (double)g2;
                    sg[k] = sg[k] + (((double)g0 * g0 + (double)g1 * g1) + (double)g2 * g2);
                    sd[k] = sd[k] + dd * d;
                }
            }
            cur = nxt;
        }
#pragma unroll
        for (int k = 0; k < DEM_K; k++) {
            if (k < nk) {
                const size_t o = (size_t)(z0 + k) * plane + col;
                float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
                const double den = sg[k] + p.a2 * sd[k];
                if (in[k] && den > 0.0) {
                    r0 = (float)(n0[k] / den);
                    r1 = (float)(n1[k] / den);
                    r2 = (float)(n2[k] / den);
                }
                if (in[k]) {
                    lsum += sd[k];
                    lcnt += 1;
                }
                out[o] = r0;
                out[o + vox] = r1;
                out[o + 2 * vox] = r2;
            }
        }
    }
    lsum = workgroup_reduce<Add>(lsum, s_sum);
    lcnt = workgroup_reduce<Add>(lcnt, s_cnt);
    if (threadIdx.x == 0) {
        p.psum[blk] = lsum;
        p.pcnt[blk] = lcnt;
    }
}

// the partial slots 0 .. n-1 in a fixed order (finish_reduce)
__global__ __launch_bounds__(256) void k_demons_finish(const double *psum, const unsigned long long *pcnt, unsigned n,
                                                       double *sum, unsigned long long *cnt)
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

// u += delta, element by element: 16-byte accesses when both are 16-byte aligned, the tail one by one
__global__ __launch_bounds__(256) void k_field_add(float *__restrict__ u, const float *__restrict__ d, size_t n, int vec)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (vec) {
        const size_t n4 = n / 4;
        for (size_t j = i; j < n4; j += stride) {
            float4 a = ld4(u + 4 * j);
            const float4 b = ld4(d + 4 * j);
            a.x = a.x + b.x; a.y = a.y + b.y; a.z = a.z + b.z; a.w = a.w + b.w;
            st4(u + 4 * j, a);
        }
        i += 4 * n4;
    }
    for (; i < n; i += stride)
        u[i] = u[i] + d[i];
}

} // namespace

// Launchers for sift3d_demons.c, which has checked every argument (not exported from the library).
// d_WF, d_WM: the masks or NULL; with both NULL the unmasked kernel runs.
extern "C" int sift3d_demons_force_launch(const float *d_F, int nx, int ny, int nz, const float *d_W, const float *d_u,
                                          int mx, int my, int mz, int nc, double alpha, float *d_step, void *d_stats,
                                          void *d_work, void *stream, const float *d_WF, const float *d_WM)
{
    ForceArgs p;
    p.F = d_F; p.W = d_W; p.u = d_u;
    p.step = d_step;
    p.psum = (double *)d_work;
    p.pcnt = (unsigned long long *)((char *)d_work + DEM_GRID * sizeof(double));
    p.a2 = alpha * alpha;
    p.nx = nx; p.ny = ny; p.nz = nz;
    p.mx = mx; p.my = my; p.mz = mz;
    p.nc = nc;
    p.wf = d_WF; p.wm = d_WM;
    p.tiles_x = (nx + DEM_TX - 1) / DEM_TX;
    p.tiles_z = (nz + DEM_K - 1) / DEM_K;
    const unsigned long long nt = (unsigned long long)p.tiles_x * ((ny + DEM_TY - 1) / DEM_TY) * p.tiles_z;
    if (nt > 0xffffffffull - DEM_GRID)
        return launch_fail("sift3d_hip_demons_force", "grid too large");
    p.ntiles = (unsigned)nt;
    const unsigned grid = p.ntiles < DEM_GRID ? p.ntiles : DEM_GRID;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL((d_WF || d_WM ? k_demons_force<true> : k_demons_force<false>), dim3(grid), dim3(256), 0, st, p);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_demons_finish, dim3(1), dim3(256), 0, st, p.psum, p.pcnt, grid, (double *)d_stats,
                       (unsigned long long *)((char *)d_stats + 8));
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

extern "C" int sift3d_demons_field_add_launch(float *d_u, const float *d_step, size_t n, void *stream)
{
    const int vec = !(((uintptr_t)d_u | (uintptr_t)d_step) & 15);
    const size_t per = vec ? 4 * 256 : 256;
    size_t blocks = (n + per - 1) / per;
    if (blocks > 8192)
        blocks = 8192;
    if (blocks < 1)
        blocks = 1;
    hipLaunchKernelGGL(k_field_add, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_u, d_step, n, vec);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}
