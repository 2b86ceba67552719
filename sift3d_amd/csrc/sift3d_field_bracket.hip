// sift3d_field_bracket.hip -- the Lie bracket of two vector fields and the first-order BCH update, and the
// symmetric velocity update of log-domain demons (contract: include/sift3d_amd.h, "Log-domain demons").
//
// k_field_bracket shares k_jacobian_det's walk (sift3d_warp.hip): a 256-lane workgroup is 64 x 4 (x, y) columns, a
// lane walks BRK_K planes of its column, a wave is 64 consecutive x of one row, so every plane's load or store of a
// channel is one coalesced 256-byte access.  Six channels are live: a lane keeps prev / cur / next along z of all
// six in registers (18 words), so the centre of a column arrives once, as the next plane; the x and y neighbours are
// loads of the neighbouring lanes' and rows' words (words that those lanes load as their own centre).
// Algorithmically 24 B read and 12 B written per voxel; 30 load and 3 store instructions per lane and plane
// (profiles/microbench/logdemons_rate_mi355x.txt).  Float arithmetic in the contract's order, no
// contraction (the unit is built with -ffp-contract=off like the rest).
#include "sift3d_resample.h"

namespace {

constexpr int BRK_TX = 64, BRK_TY = 4, BRK_K = 8;

struct BracketArgs {
    const float *a, *b;
    float *out;
    int ox, oy, oz;
    int tiles_x, tiles_y;
    unsigned ntiles;                             // < 2^32 - MAX_GRID (checked at launch)
};

template <int MODE>
__global__ __launch_bounds__(256) void k_field_bracket(const BracketArgs p)
{
    const float *__restrict__ fa = p.a;
    const float *__restrict__ fb = p.b;
    float *__restrict__ dst = p.out;
    const size_t sx = (size_t)p.ox, plane = (size_t)p.oy * (size_t)p.ox, vox = plane * (size_t)p.oz;
    for (unsigned t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
        const unsigned tyz = t / (unsigned)p.tiles_x;
        const int tx = (int)(t - tyz * (unsigned)p.tiles_x);
        const int ty = (int)(tyz % (unsigned)p.tiles_y), tz = (int)(tyz / (unsigned)p.tiles_y);
        const int x = tx * BRK_TX + (int)(threadIdx.x & 63), y = ty * BRK_TY + (int)(threadIdx.x >> 6);
        const int z0 = tz * BRK_K;
        if (x >= p.ox || y >= p.oy)
            continue;
        const size_t col = (size_t)y * sx + (size_t)x;
        const size_t dxm = x > 0 ? 1 : 0, dxp = x + 1 < p.ox ? 1 : 0;          // neighbour offsets, clamped
        const size_t dym = y > 0 ? sx : 0, dyp = y + 1 < p.oy ? sx : 0;
        const int nk = min(BRK_K, p.oz - z0);
        // channel c < 3: a_c, else b_(c-3); the field at z - 1, z, z + 1 of the column
        float lo[6], c[6], hi[6];
#pragma unroll
        for (int q = 0; q < 6; q++) {
            const float *u = (q < 3 ? fa + (size_t)q * vox : fb + (size_t)(q - 3) * vox) + col;
            c[q] = u[(size_t)z0 * plane];
            lo[q] = z0 > 0 ? u[(size_t)(z0 - 1) * plane] : c[q];
        }
        for (int k = 0; k < nk; k++) {
            const int z = z0 + k;
            const size_t o = (size_t)z * plane + col;
            float g[6][3];
#pragma unroll
            for (int q = 0; q < 6; q++) {
                const float *u = q < 3 ? fa + (size_t)q * vox : fb + (size_t)(q - 3) * vox;
                hi[q] = z + 1 < p.oz ? u[o + plane] : c[q];
                g[q][0] = grad(u[o - dxm], c[q], u[o + dxp], x, p.ox);
                g[q][1] = grad(u[o - dym], c[q], u[o + dyp], y, p.oy);
                g[q][2] = grad(lo[q], c[q], hi[q], z, p.oz);
            }
#pragma unroll
            for (int d = 0; d < 3; d++) {
                const float td = (g[d][0] * c[3] + g[d][1] * c[4]) + g[d][2] * c[5];          // (J_a b)_d
                const float sd = (g[3 + d][0] * c[0] + g[3 + d][1] * c[1]) + g[3 + d][2] * c[2];    // (J_b a)_d
                const float br = td - sd;
                dst[(size_t)d * vox + o] = MODE == SIFT3D_AMD_FIELD_BRACKET ? br : (c[d] + c[3 + d]) + 0.5f * br;
            }
#pragma unroll
            for (int q = 0; q < 6; q++) {
                lo[q] = c[q];
                c[q] = hi[q];
            }
        }
    }
}

// v = 0.5f * (Z_f - Z_b).  BCH 0: Z_f = v + df, Z_b = (-v) + db, formed here; BCH 1: zf and zb hold them.
template <int BCH>
__global__ __launch_bounds__(256) void k_velocity_symmetrize(float *__restrict__ v, const float *__restrict__ zf,
                                                             const float *__restrict__ zb, size_t n)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float w = v[i];
        const float f = BCH ? zf[i] : w + zf[i];
        const float b = BCH ? zb[i] : (-w) + zb[i];
        v[i] = 0.5f * (f - b);
    }
}

} // namespace

// Launchers for sift3d_field_ops.c and sift3d_demons.c, which have checked every argument (not exported).
extern "C" int sift3d_field_bracket_launch(const float *d_a, const float *d_b, int ox, int oy, int oz, float *d_out,
                                           int mode, void *stream)
{
    static const char fn[] = "sift3d_hip_field_bracket";
    BracketArgs p;
    p.a = d_a; p.b = d_b;
    p.out = d_out;
    p.ox = ox; p.oy = oy; p.oz = oz;
    p.tiles_x = (ox + BRK_TX - 1) / BRK_TX;
    p.tiles_y = (oy + BRK_TY - 1) / BRK_TY;
    const unsigned long long nt = (unsigned long long)p.tiles_x * p.tiles_y * ((oz + BRK_K - 1) / BRK_K);
    if (nt > 0xffffffffull - MAX_GRID)
        return launch_fail(fn, "output grid too large");
    p.ntiles = (unsigned)nt;
    const unsigned grid = p.ntiles < MAX_GRID ? p.ntiles : MAX_GRID;
    void (*k)(const BracketArgs) = mode == SIFT3D_AMD_FIELD_BRACKET ? k_field_bracket<SIFT3D_AMD_FIELD_BRACKET>
                                                                     : k_field_bracket<SIFT3D_AMD_FIELD_BCH1>;
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

extern "C" int sift3d_velocity_symmetrize_launch(float *d_v, const float *d_zf, const float *d_zb, size_t n, int bch,
                                                 void *stream)
{
    size_t blocks = (n + 255) / 256;
    if (blocks > 8192)
        blocks = 8192;
    if (blocks < 1)
        blocks = 1;
    hipLaunchKernelGGL(bch ? k_velocity_symmetrize<1> : k_velocity_symmetrize<0>, dim3((unsigned)blocks), dim3(256), 0,
                       (hipStream_t)stream, d_v, d_zf, d_zb, n);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}
