// sift3d_lncc.hip -- local (windowed) cross-correlation of a fixed and a warped volume, its exact derivative as a
// demons-style force, and the normalisation of a field to a step length (contract: include/sift3d_amd.h, "Local
// cross-correlation").  The iteration that chains them with warp_field, the blur and the update is host code
// (sift3d_lncc.c), which checks every argument before it calls a launcher here.
//
// k_lncc_valid writes v(p) (1.0f / 0.0f: k_demons_force<true>'s rule) once, so that the two windowed passes read one
// float per halo voxel instead of u and two masks.  k_lncc_stats<R> box-sums the six quantities of the statistic
// (sift3d_boxsum.h, NQ = 6; raw form v, F, W) and writes cc, the four coefficient volumes and the per-workgroup
// partials of (sum cc, count); k_lncc_finish adds the partials in a fixed order.  k_lncc_force<R> box-sums the four
// coefficient volumes (NQ = 4; raw form: the doubles themselves) and writes phi.  Both walk tiles numbered z
// fastest, a contiguous run per workgroup, in stretches of LNCC_ZC planes: a stretch re-reads the 2R planes under and
// over it (2R / LNCC_ZC more planes), and gives a 256^3 volume 2048 stretches instead of 256 columns.  The grid is
// min(tiles, LNCC_GRID) workgroups whatever the device, so the bits of the sum depend on the shape alone.
// k_field_maxnorm / k_field_maxnorm_finish / k_field_scale: the max of |phi|^2 in double (exact, order-free), the
// scale (float)(step / sqrt(m2)) left in device memory, and the multiply by it, which reads it there.
#include "sift3d_boxsum.h"
#include "sift3d_resample.h"

namespace {

// output planes per stretch (-DSIFT3D_LNCC_ZC=n; profiles/microbench/lncc_rate.py)
#ifndef SIFT3D_LNCC_ZC
#define SIFT3D_LNCC_ZC 32
#endif
constexpr int LNCC_ZC = SIFT3D_LNCC_ZC;
// rows per lane: the tile is 64 x 4 LNCC_RY (-DSIFT3D_LNCC_RY=2: the 64 x 8 tile, for the passes whose LDS still fits
// the 64 KiB static limit with it; the force pass at r = 4 needs 68 KiB and keeps 64 x 4)
#ifndef SIFT3D_LNCC_RY
#define SIFT3D_LNCC_RY 1
#endif
template <class P, int R> constexpr int rows_per_lane()
{
    return sizeof(BoxLds<P, R, SIFT3D_LNCC_RY>) <= 65536 - 256 ? SIFT3D_LNCC_RY : 1;
}
constexpr unsigned LNCC_GRID = SIFT3D_AMD_LNCC_PARTIAL_BYTES / 16;    // partial slots: double + uint64
constexpr unsigned NORM_GRID = (SIFT3D_AMD_FIELD_NORMALIZE_WORK_BYTES - 16) / 8;    // partial maxima, then m2 and s
constexpr double LNCC_TAU = 9.313225746154785e-10;            // 2^-30

struct ValidArgs {
    const float *u, *wf, *wm;
    float *v;
    int nx, ny, nz, mx, my, mz;
};

// v(p): p samples inside the moving grid and is in both masks (either may be null: all in)
__global__ __launch_bounds__(256) void k_lncc_valid(const ValidArgs p)
{
    const size_t sx = (size_t)p.nx, plane = (size_t)p.ny * sx, vox = plane * (size_t)p.nz;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < vox; o += stride) {
        const size_t zy = o / sx;
        const int x = (int)(o - zy * sx), y = (int)(zy % (size_t)p.ny), z = (int)(zy / (size_t)p.ny);
        const double qx = (double)x + (double)p.u[o], qy = (double)y + (double)p.u[o + vox];
        const double qz = (double)z + (double)p.u[o + 2 * vox];
        bool in = inside(qx, qy, qz, p.mx, p.my, p.mz);
        const float wf = p.wf ? p.wf[o] : 1.0f;
        const float wm = p.wm ? p.wm[mask_offset(p.mx, p.my, p.mz, qx, qy, qz)] : 1.0f;
        in = in && mask_in(wf) && mask_in(wm);
        p.v[o] = in ? 1.0f : 0.0f;
    }
}

struct TileWalk {
    int nx, ny, nz;
    int ty;                                      // the tile's rows: 4 x the kernel's rows per lane
    int tiles_x, tiles_z;
    unsigned ntiles;
};

struct StatsArgs {
    const float *F, *W, *v;
    float *cc;                                   // or null
    double *coef;                                // or null
    double *psum;                                // [LNCC_GRID]
    unsigned long long *pcnt;                    // [LNCC_GRID]
    TileWalk t;
};

struct ForceArgs {
    const float *F, *W, *v;
    const double *coef;
    float *phi;
    TileWalk t;
};

// the statistic's six quantities v, vF, vW, vFF, vWW, vFW from the raw (v, F, W): the floats promoted first, so every
// product is exact; a voxel with v = 0 gives +0.0 six times whatever F and W hold there (a select, not a multiply)
struct StatsPolicy {
    static constexpr int NQ = 6, NRAW = 3;
    typedef float raw_t;
    const float *F, *W, *v;
    size_t sx, plane;
    __device__ __forceinline__ void load(int x, int y, int z, float *r) const
    {
        const size_t o = (size_t)z * plane + (size_t)y * sx + (size_t)x;
        r[0] = v[o];
        r[1] = F[o];
        r[2] = W[o];
    }
    __device__ __forceinline__ void expand(const float *r, double *q) const
    {
        const bool in = r[0] != 0.0f;
        const double f = in ? (double)r[1] : 0.0, w = in ? (double)r[2] : 0.0;
        q[0] = in ? 1.0 : 0.0;
        q[1] = f;
        q[2] = w;
        q[3] = f * f;
        q[4] = w * w;
        q[5] = f * w;
    }
};

// the force's four quantities a, a mf, b, b mw: the coefficient volumes themselves
struct ForcePolicy {
    static constexpr int NQ = 4, NRAW = 4;
    typedef double raw_t;
    const double *coef;
    size_t sx, plane, vox;
    __device__ __forceinline__ void load(int x, int y, int z, double *r) const
    {
        const size_t o = (size_t)z * plane + (size_t)y * sx + (size_t)x;
#pragma unroll
        for (int k = 0; k < 4; k++)
            r[k] = coef[(size_t)k * vox + o];
    }
    __device__ __forceinline__ void expand(const double *r, double *q) const
    {
#pragma unroll
        for (int k = 0; k < 4; k++)
            q[k] = r[k];
    }
};

// tile t of the walk: the tile's (x, y) origin and its stretch of output planes
__device__ __forceinline__ void tile_of(const TileWalk &w, unsigned t, int &x0, int &y0, int &zlo, int &zhi)
{
    const unsigned txy = t / (unsigned)w.tiles_z;
    const int tz = (int)(t - txy * (unsigned)w.tiles_z);
    x0 = (int)(txy % (unsigned)w.tiles_x) * BOX_TX;
    y0 = (int)(txy / (unsigned)w.tiles_x) * w.ty;
    zlo = tz * LNCC_ZC;
    zhi = min(w.nz, zlo + LNCC_ZC);
}

template <int R>
__global__ __launch_bounds__(256) void k_lncc_stats(const StatsArgs p)
{
    constexpr int RY = rows_per_lane<StatsPolicy, R>();
    __shared__ BoxLds<StatsPolicy, R, RY> s_box;
    __shared__ double s_sum[4];
    __shared__ unsigned long long s_cnt[4];
    const size_t sx = (size_t)p.t.nx, plane = (size_t)p.t.ny * sx, vox = plane * (size_t)p.t.nz;
    const StatsPolicy pol = { p.F, p.W, p.v, sx, plane };
    double lsum = 0.0;
    unsigned long long lcnt = 0;
    const unsigned per = (p.t.ntiles + gridDim.x - 1) / gridDim.x;
    const unsigned t_end = min(p.t.ntiles, blockIdx.x * per + per);
    for (unsigned t = blockIdx.x * per; t < t_end; t++) {
        int x0, y0, zlo, zhi;
        tile_of(p.t, t, x0, y0, zlo, zhi);
        box_march<StatsPolicy, R, RY>(pol, x0, y0, zlo, zhi, p.t.nx, p.t.ny, p.t.nz, s_box,
                                  [&](int x, int y, int z, bool on, const double *q) {
            if (!on)
                return;
            const size_t o = (size_t)z * plane + (size_t)y * sx + (size_t)x;
            const double n = q[0], sf = q[1], sw = q[2], sff = q[3], sww = q[4], sfw = q[5];
            double cc = 0.0, a = 0.0, am = 0.0, b = 0.0, bm = 0.0;
            if (p.v[o] != 0.0f && n >= 2.0) {
                const double A = sfw - (sf * sw) / n;
                const double B = sff - (sf * sf) / n;
                const double C = sww - (sw * sw) / n;
                if (B > LNCC_TAU * sff && C > LNCC_TAU * sww) {
                    cc = (A * A) / (B * C);
                    a = (2.0 * A) / (B * C);
                    b = (2.0 * cc) / C;
                    am = a * (sf / n);
                    bm = b * (sw / n);
                    lsum += cc;
                    lcnt += 1;
                }
            }
            if (p.cc)
                p.cc[o] = (float)cc;
            if (p.coef) {
                p.coef[o] = a;
                p.coef[o + vox] = am;
                p.coef[o + 2 * vox] = b;
                p.coef[o + 3 * vox] = bm;
            }
        });
    }
    lsum = workgroup_reduce<Add>(lsum, s_sum);
    lcnt = workgroup_reduce<Add>(lcnt, s_cnt);
    if (threadIdx.x == 0) {
        p.psum[blockIdx.x] = lsum;
        p.pcnt[blockIdx.x] = lcnt;
    }
}

// the partial slots 0 .. n-1 in a fixed order (finish_reduce)
__global__ __launch_bounds__(256) void k_lncc_finish(const double *psum, const unsigned long long *pcnt, unsigned n,
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

template <int R>
__global__ __launch_bounds__(256) void k_lncc_force(const ForceArgs p)
{
    constexpr int RY = rows_per_lane<ForcePolicy, R>();
    __shared__ BoxLds<ForcePolicy, R, RY> s_box;
    const int nx = p.t.nx, ny = p.t.ny, nz = p.t.nz;
    const size_t sx = (size_t)nx, plane = (size_t)ny * sx, vox = plane * (size_t)nz;
    const ForcePolicy pol = { p.coef, sx, plane, vox };
    const float *__restrict__ Fb = p.F;
    const float *__restrict__ Wb = p.W;
    const unsigned per = (p.t.ntiles + gridDim.x - 1) / gridDim.x;
    const unsigned t_end = min(p.t.ntiles, blockIdx.x * per + per);
    for (unsigned t = blockIdx.x * per; t < t_end; t++) {
        int x0, y0, zlo, zhi;
        tile_of(p.t, t, x0, y0, zlo, zhi);
        box_march<ForcePolicy, R, RY>(pol, x0, y0, zlo, zhi, nx, ny, nz, s_box,
                                  [&](int x, int y, int z, bool on, const double *q) {
            if (!on)
                return;
            const size_t o = (size_t)z * plane + (size_t)y * sx + (size_t)x;
            float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
            if (p.v[o] != 0.0f) {
                // the neighbours of W, clamped onto the grid (numpy.gradient's ends do not read past it)
                const float wc = Wb[o];
                const float wxm = Wb[o - (x > 0 ? 1 : 0)], wxp = Wb[o + (x + 1 < nx ? 1 : 0)];
                const float wym = Wb[o - (y > 0 ? sx : 0)], wyp = Wb[o + (y + 1 < ny ? sx : 0)];
                const float wzm = Wb[o - (z > 0 ? plane : 0)], wzp = Wb[o + (z + 1 < nz ? plane : 0)];
                const double g = ((double)Fb[o] * q[0] - q[1]) - ((double)wc * q[2] - q[3]);
                r0 = (float)(g * (double)grad(wxm, wc, wxp, x, nx));
                r1 = (float)(g * (double)grad(wym, wc, wyp, y, ny));
                r2 = (float)(g * (double)grad(wzm, wc, wzp, z, nz));
            }
            p.phi[o] = r0;
            p.phi[o + vox] = r1;
            p.phi[o + 2 * vox] = r2;
        });
    }
}

// ---- normalisation of a field to a step length --------------------------------------------------------------------
// max over a stretch of voxels of ((double) x^2 + (double) y^2) + (double) z^2: exact whatever the order
__global__ __launch_bounds__(256) void k_field_maxnorm(const float *__restrict__ f, size_t n, double *part)
{
    __shared__ double s_max[4];
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    double m = 0.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double x = (double)f[i], y = (double)f[i + n], z = (double)f[i + 2 * n];
        m = fmax(m, (x * x + y * y) + z * z);
    }
    m = workgroup_reduce<Max>(m, s_max);
    if (threadIdx.x == 0)
        part[blockIdx.x] = m;
}

// rec[0] (double): m2; the float at byte 8 of rec: s = (float)(step / sqrt(m2)) (not read when m2 == 0)
__global__ __launch_bounds__(256) void k_field_maxnorm_finish(const double *part, unsigned n, double step, double *rec)
{
    __shared__ double s_max[256];
    const double m2 = finish_reduce<Max>(part, n, s_max);
    if (threadIdx.x == 0) {
        rec[0] = m2;
        *reinterpret_cast<float *>(rec + 1) = m2 > 0.0 ? (float)(step / sqrt(m2)) : 1.0f;
    }
}

// every component times s (a float multiply); m2 == 0 leaves the field as it is
__global__ __launch_bounds__(256) void k_field_scale_by(float *__restrict__ f, size_t n3, const double *rec)
{
    if (!(rec[0] > 0.0))
        return;
    const float s = *reinterpret_cast<const float *>(rec + 1);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n3; i += stride)
        f[i] = s * f[i];
}

// the tile walk of a grid; false when it has too many tiles for 32 bits
bool tile_walk(TileWalk &t, int nx, int ny, int nz, int ry)
{
    t.nx = nx; t.ny = ny; t.nz = nz;
    t.ty = 4 * ry;
    t.tiles_x = (nx + BOX_TX - 1) / BOX_TX;
    t.tiles_z = (nz + LNCC_ZC - 1) / LNCC_ZC;
    const unsigned long long nt = (unsigned long long)t.tiles_x * ((ny + t.ty - 1) / t.ty) * t.tiles_z;
    if (nt > 0xffffffffull - LNCC_GRID)
        return false;
    t.ntiles = (unsigned)nt;
    return true;
}

unsigned stream_grid(size_t n, unsigned cap)
{
    size_t b = (n + 255) / 256;
    if (b > cap)
        b = cap;
    return (unsigned)(b < 1 ? 1 : b);
}

} // namespace

// Launchers for sift3d_lncc.c, which has checked every argument (not exported from the library).
extern "C" int sift3d_lncc_valid_launch(const float *d_u, int nx, int ny, int nz, int mx, int my, int mz,
                                        const float *d_WF, const float *d_WM, float *d_v, void *stream)
{
    ValidArgs p;
    p.u = d_u; p.wf = d_WF; p.wm = d_WM; p.v = d_v;
    p.nx = nx; p.ny = ny; p.nz = nz; p.mx = mx; p.my = my; p.mz = mz;
    const size_t n = (size_t)nx * ny * nz;
    hipLaunchKernelGGL(k_lncc_valid, dim3(stream_grid(n, 8192)), dim3(256), 0, (hipStream_t)stream, p);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

// d_part: SIFT3D_AMD_LNCC_PARTIAL_BYTES; d_cc, d_coef: either may be NULL
extern "C" int sift3d_lncc_stats_launch(const float *d_F, const float *d_W, const float *d_v, int nx, int ny, int nz,
                                        int radius, float *d_cc, double *d_coef, void *d_stats, void *d_part,
                                        void *stream)
{
    StatsArgs p;
    p.F = d_F; p.W = d_W; p.v = d_v;
    p.cc = d_cc; p.coef = d_coef;
    p.psum = (double *)d_part;
    p.pcnt = (unsigned long long *)((char *)d_part + LNCC_GRID * sizeof(double));
    hipStream_t st = (hipStream_t)stream;
    unsigned grid = 0;
    bool fits = true;
    // (the tile's rows depend on the radius where SIFT3D_LNCC_RY asks for more than one per lane)
    if (!dispatch_int<1, SIFT3D_AMD_LNCC_MAX_RADIUS>(radius, [&](auto r) {
            constexpr int R = decltype(r)::value;
            fits = tile_walk(p.t, nx, ny, nz, rows_per_lane<StatsPolicy, R>());
            if (!fits)
                return;
            grid = p.t.ntiles < LNCC_GRID ? p.t.ntiles : LNCC_GRID;
            hipLaunchKernelGGL(k_lncc_stats<R>, dim3(grid), dim3(256), 0, st, p);
        }))
        return launch_fail("sift3d_hip_lncc", "radius out of range");
    if (!fits)
        return launch_fail("sift3d_hip_lncc", "grid too large");
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_lncc_finish, dim3(1), dim3(256), 0, st, p.psum, p.pcnt, grid, (double *)d_stats,
                       (unsigned long long *)((char *)d_stats + 8));
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

extern "C" int sift3d_lncc_force_launch(const float *d_F, const float *d_W, const float *d_v, int nx, int ny, int nz,
                                        int radius, const double *d_coef, float *d_force, void *stream)
{
    ForceArgs p;
    p.F = d_F; p.W = d_W; p.v = d_v;
    p.coef = d_coef;
    p.phi = d_force;
    bool fits = true;
    if (!dispatch_int<1, SIFT3D_AMD_LNCC_MAX_RADIUS>(radius, [&](auto r) {
            constexpr int R = decltype(r)::value;
            fits = tile_walk(p.t, nx, ny, nz, rows_per_lane<ForcePolicy, R>());
            if (!fits)
                return;
            const unsigned grid = p.t.ntiles < LNCC_GRID ? p.t.ntiles : LNCC_GRID;
            hipLaunchKernelGGL(k_lncc_force<R>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
        }))
        return launch_fail("sift3d_hip_lncc_force", "radius out of range");
    if (!fits)
        return launch_fail("sift3d_hip_lncc_force", "grid too large");
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

// d_work: SIFT3D_AMD_FIELD_NORMALIZE_WORK_BYTES (the partial maxima, then m2 and s)
extern "C" int sift3d_field_normalize_launch(float *d_field, size_t n, double step, void *d_work, void *stream)
{
    double *part = (double *)d_work, *rec = part + NORM_GRID;
    const unsigned grid = stream_grid(n, NORM_GRID);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_field_maxnorm, dim3(grid), dim3(256), 0, st, d_field, n, part);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_field_maxnorm_finish, dim3(1), dim3(256), 0, st, part, grid, step, rec);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_field_scale_by, dim3(stream_grid(3 * n, 8192)), dim3(256), 0, st, d_field, 3 * n, rec);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}
