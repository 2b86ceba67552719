// sift3d_mind.hip -- the MIND-SSC self-similarity descriptor of a volume (contract: include/sift3d_amd.h, "MIND
// self-similarity descriptors").  The arguments are checked by host code (sift3d_mind.c) before the launcher here.
//
// k_mind<R> is a policy over box_march (sift3d_boxsum.h, NQ = 12): the raw form of a halo voxel is its six shifted
// samples I(clamp(q + n_i)) as floats, and the expansion forms the twelve squared differences in double, so the
// twelve box sums D_k come out in the contract's order.  emit forms S, V, Dmin and the twelve cexp values, stores
// whichever outputs were asked for and adds V to the workgroup's partial; k_mind_finish adds the partials in a fixed
// order.  The tile walk is sift3d_lncc.hip's: tiles of 64 x 4 numbered z fastest, a contiguous run per workgroup, in
// stretches of MIND_ZC planes, on min(tiles, MIND_GRID) workgroups whatever the device, so that the bits of the one
// sum depend on the shape alone.  LDS (256 lanes, one row per lane): 46,368 B at r = 1 and 62,208 B at r = 2.
#include "sift3d_boxsum.h"
#include "sift3d_resample.h"

namespace {

constexpr int MIND_ZC = 32;                                   // output planes per stretch
constexpr unsigned MIND_PARTIAL_BYTES = 32768;                // sift3d_amd_mind_work_bytes
constexpr unsigned MIND_GRID = MIND_PARTIAL_BYTES / 16;       // partial slots: double + uint64
constexpr int NCH = SIFT3D_AMD_MIND_CHANNELS;

struct TileWalk {
    int nx, ny, nz;
    int tiles_x, tiles_z;
    unsigned ntiles;
};

struct MindArgs {
    const float *src;
    float *out;                                  // or null
    double *D, *V;                               // or null
    double *psum;                                // [MIND_GRID]
    unsigned long long *pcnt;                    // [MIND_GRID]
    double vlo, vhi;
    int d;
    TileWalk t;
};

// the six shifted samples of an on-grid voxel, and from them the twelve e_k; six zeros (an off-grid halo voxel)
// give twelve times +0.0
struct MindPolicy {
    static constexpr int NQ = NCH, NRAW = 6;
    typedef float raw_t;
    const float *src;
    int nx, ny, nz, d;
    size_t sx, plane;
    __device__ __forceinline__ void load(int x, int y, int z, float *r) const
    {
        const size_t o = (size_t)z * plane + (size_t)y * sx;
        const size_t row = o + (size_t)x;
        r[0] = src[o + (size_t)min(x + d, nx - 1)];
        r[1] = src[o + (size_t)max(x - d, 0)];
        r[2] = src[row + (size_t)(min(y + d, ny - 1) - y) * sx];
        r[3] = src[row - (size_t)(y - max(y - d, 0)) * sx];
        r[4] = src[row + (size_t)(min(z + d, nz - 1) - z) * plane];
        r[5] = src[row - (size_t)(z - max(z - d, 0)) * plane];
    }
    __device__ __forceinline__ void expand(const float *r, double *q) const
    {
        double s[6];
#pragma unroll
        for (int i = 0; i < 6; i++)
            s[i] = (double)r[i];
        // the pairs (0,2) (0,3) (0,4) (0,5) (1,2) (1,3) (1,4) (1,5) (2,4) (2,5) (3,4) (3,5)
        int k = 0;
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = (i < 2 ? 2 : 4); j < 6; j++) {
                const double e = s[i] - s[j];
                q[k++] = e * e;
            }
    }
};

// the contract's exponential of -t: 2^-f by the Taylor polynomial of degree 10 in Horner form, times the exact 2^-n
__device__ __forceinline__ double cexp(double t)
{
    if (t >= 104.0)
        return 0.0;
    const double y = t * SIFT3D_AMD_MIND_LOG2E;
    const double n = floor(y);
    const double f = y - n;
    double p = 0x1.e4cf5158b8ecap-28;
    p = p * f + -0x1.b5253d395e7c4p-24;
    p = p * f + 0x1.62c0223a5c824p-20;
    p = p * f + -0x1.ffcbfc588b0c7p-17;
    p = p * f + 0x1.430912f86c787p-13;
    p = p * f + -0x1.5d87fe78a6731p-10;
    p = p * f + 0x1.3b2ab6fba4e77p-7;
    p = p * f + -0x1.c6b08d704a0c0p-5;
    p = p * f + 0x1.ebfbdff82c58fp-3;
    p = p * f + -0x1.62e42fefa39efp-1;
    p = p * f + 1.0;
    // 2^-n, 0 <= n <= 150: a normal double written by its exponent field
    const double s = __longlong_as_double((long long)(1023 - (int)n) << 52);
    return p * s;
}

// tile t of the walk: the tile's (x, y) origin and its stretch of output planes (sift3d_lncc.hip's tile_of)
__device__ __forceinline__ void tile_of(const TileWalk &w, unsigned t, int &x0, int &y0, int &zlo, int &zhi)
{
    const unsigned txy = t / (unsigned)w.tiles_z;
    const int tz = (int)(t - txy * (unsigned)w.tiles_z);
    x0 = (int)(txy % (unsigned)w.tiles_x) * BOX_TX;
    y0 = (int)(txy / (unsigned)w.tiles_x) * 4;
    zlo = tz * MIND_ZC;
    zhi = min(w.nz, zlo + MIND_ZC);
}

template <int R>
__global__ __launch_bounds__(256) void k_mind(const MindArgs p)
{
    __shared__ BoxLds<MindPolicy, R, 1> s_box;
    __shared__ double s_sum[4];
    __shared__ unsigned long long s_cnt[4];
    static_assert(sizeof(BoxLds<MindPolicy, R, 1>) <= 65536 - 256, "the tile does not fit the static LDS limit");
    const size_t sx = (size_t)p.t.nx, plane = (size_t)p.t.ny * sx, vox = plane * (size_t)p.t.nz;
    const MindPolicy pol = { p.src, p.t.nx, p.t.ny, p.t.nz, p.d, sx, plane };
    double lsum = 0.0;
    unsigned long long lcnt = 0;
    const unsigned per = (p.t.ntiles + gridDim.x - 1) / gridDim.x;
    const unsigned t_end = min(p.t.ntiles, blockIdx.x * per + per);
    for (unsigned t = blockIdx.x * per; t < t_end; t++) {
        int x0, y0, zlo, zhi;
        tile_of(p.t, t, x0, y0, zlo, zhi);
        box_march<MindPolicy, R, 1>(pol, x0, y0, zlo, zhi, p.t.nx, p.t.ny, p.t.nz, s_box,
                                    [&](int x, int y, int z, bool on, const double *D) {
            if (!on)
                return;
            const size_t o = (size_t)z * plane + (size_t)y * sx + (size_t)x;
            double S = 0.0, dmin = D[0];
#pragma unroll
            for (int k = 0; k < NCH; k++) {
                S = S + D[k];
                dmin = D[k] < dmin ? D[k] : dmin;
            }
            const double V = S / 12.0;
            lsum += V;
            lcnt += 1;
            if (p.V)
                p.V[o] = V;
            if (p.D) {
#pragma unroll
                for (int k = 0; k < NCH; k++)
                    p.D[(size_t)k * vox + o] = D[k];
            }
            if (p.out) {
                double vc = V < p.vlo ? p.vlo : V;
                vc = vc > p.vhi ? p.vhi : vc;
#pragma unroll
                for (int k = 0; k < NCH; k++) {
                    const double tk = vc == 0.0 ? 0.0 : (D[k] - dmin) / vc;
                    p.out[(size_t)k * vox + o] = (float)cexp(tk);
                }
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
__global__ __launch_bounds__(256) void k_mind_finish(const double *psum, const unsigned long long *pcnt, unsigned n,
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

// the tile walk of a grid; false when it has too many tiles for 32 bits
bool tile_walk(TileWalk &t, int nx, int ny, int nz)
{
    t.nx = nx; t.ny = ny; t.nz = nz;
    t.tiles_x = (nx + BOX_TX - 1) / BOX_TX;
    t.tiles_z = (nz + MIND_ZC - 1) / MIND_ZC;
    const unsigned long long nt = (unsigned long long)t.tiles_x * ((ny + 3) / 4) * t.tiles_z;
    if (nt > 0xffffffffull - MIND_GRID)
        return false;
    t.ntiles = (unsigned)nt;
    return true;
}

} // namespace

// Launcher for sift3d_mind.c, which has checked every argument (not exported from the library).  d_work:
// sift3d_amd_mind_work_bytes; d_out, d_D, d_V, d_stats: any may be NULL.
extern "C" int sift3d_mind_launch(const float *d_src, int nx, int ny, int nz, int radius, int dilation, double vlo,
                                  double vhi, float *d_out, double *d_D, double *d_V, void *d_stats, void *d_work,
                                  void *stream)
{
    static_assert(MIND_PARTIAL_BYTES == MIND_GRID * (sizeof(double) + sizeof(unsigned long long)), "partial slots");
    MindArgs p;
    p.src = d_src; p.out = d_out; p.D = d_D; p.V = d_V;
    p.psum = (double *)d_work;
    p.pcnt = (unsigned long long *)((char *)d_work + MIND_GRID * sizeof(double));
    p.vlo = vlo; p.vhi = vhi; p.d = dilation;
    if (!tile_walk(p.t, nx, ny, nz))
        return launch_fail("sift3d_hip_mind_ssc", "grid too large");
    const unsigned grid = p.t.ntiles < MIND_GRID ? p.t.ntiles : MIND_GRID;
    hipStream_t st = (hipStream_t)stream;
    if (!dispatch_int<1, SIFT3D_AMD_MIND_MAX_RADIUS>(radius, [&](auto r) {
            hipLaunchKernelGGL(k_mind<decltype(r)::value>, dim3(grid), dim3(256), 0, st, p);
        }))
        return launch_fail("sift3d_hip_mind_ssc", "radius out of range");
    LAUNCH_CHECK();
    if (d_stats) {
        hipLaunchKernelGGL(k_mind_finish, dim3(1), dim3(256), 0, st, p.psum, p.pcnt, grid, (double *)d_stats,
                           (unsigned long long *)((char *)d_stats + 8));
        LAUNCH_CHECK();
    }
    return SIFT3D_SUCCESS;
}
