// sift3d_fir_xyz.hip -- a whole octave-0 blur (x, y and z passes) in ONE launch and its C entry: XyzGeom and the
// staging geometry of k_fir_xyz_dma, its per-request filter (scale, x edges, x phase, y taps), its z ring and the
// dynamic-LDS launcher.  The LDS-DMA pipeline it shares with k_fir_yz_dma is in sift3d_fir_dma.h, explained there.
//
// Compiled with -fno-slp-vectorize like sift3d_fir_yz.hip.  Numerical contract and citations as in
// sift3d_kernels.hip.
#include "sift3d_fir_dma.h"

#include <atomic>

// ---- fused x + y + z passes, unit tap spacing -----------------------------------------------------
// dst = FIR_z(FIR_y(FIR_x(src))) where neither the x-pass nor the y-pass result reaches HBM: the pair
// k_fir_x_u1f + k_fir_yz_dma writes the x-filtered volume to scratch and reads it back (8 of its ~16.3
// B/voxel).  A workgroup owns a 64(x) x TY(y) column and sweeps a segment along z as k_fir_yz_dma does.  What
// differs from that kernel:
//   * The staged rows are rows of the blur's SOURCE, 64 + 2 * 8 floats wide (HALO = 8 as in k_fir_x_u1f: every
//     DMA piece stays 16-byte aligned): SQ = 20 quads per row.  A DMA piece is 64 consecutive quads of the
//     tile (3.2 rows); lane -> (row, quad) = (f / 20, f % 20) of its flat quad index f.  Source addresses are
//     clamped at the volume's x edges as they are for y.
//   * An x phase per request: after the barrier that opens request t its TY + 2 HW rows are filtered along x
//     into the tile `xf` (16 quads per row), with k_fir_x_u1f's arithmetic and tap order; the y filter reads
//     `xf` as k_fir_yz_dma reads its staged tile.  One more barrier per request.
//   * x edges as ext_sample forms them, in LDS after the DMA, by the workgroups of the first and the last tile
//     column only: the low face's mirror images E[-i] = src[i], the high face's virtual samples E[nx - 1 + m]
//     from Ex.lo / w0 / w1 (imutil.c:846-848).  (k_fir_x_u1f forms a mirrored sample as 1 * a + 0 * b, which
//     differs from a by the sign of a zero at most; a sum that starts from +0 cannot show it.)
//   * SCALED (the first blur of the pyramid): every staged sample is divided by *scale_max once, in LDS, before
//     the edge samples are formed (im_scale, imutil.c:698-713; a maximum of 0 leaves the image alone).
//   * The virtual rows of the high y face are formed from x-FILTERED rows (in `xf`): the y edge rules act on
//     the x pass's output, as in the reference (apply_Sep_FIR_filter, imutil.c:1165-1188).
// Per-voxel arithmetic and tap order are those of the separate passes: bit-identical results.
// LDS (dynamic, above the 64 KB of a static allocation): 4 staged tiles of NP KB + xf + seq --
//   HW = 8, TY = 32: 4 x 15 KB + 12 KB + 1.3 KB = 73.3 KB, two 512-thread workgroups per CU;
//   HW = 2, TY = 64: 4 x 22 KB + 17 KB + 1.3 KB = 106.3 KB, one 1024-thread workgroup per CU;
// 4 waves per SIMD either way, as k_fir_yz_dma.
template <int HW, int TY> struct XyzGeom {
    static constexpr int TXQ = DMA_TXQ, SQ = 20, HALO = 8, W = 2 * HW + 1, ROWS = TY + 2 * HW, NB = DMA_NB;
    static constexpr int NT = 16 * TY, NWAVE = NT / 64;
    static constexpr int NQ = ROWS * SQ;               // quads of a staged tile
    static constexpr int NP = (NQ + 63) / 64;          // its DMA pieces (1 KB each; the last one padded)
    static constexpr int TILEQ = NP * 64;
    static constexpr size_t LDS_BYTES = (size_t)(NB * TILEQ + ROWS * TXQ) * 16 + (DMA_SEQ + 1) * 4;
    static_assert((NP + NWAVE - 1) / NWAVE == 2, "two pieces per wave and request");
    static_assert(HW <= HALO, "halo too small");
};

template <int HW, int TY, bool SCALED>
__global__ __launch_bounds__(16 * TY) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_fir_xyz_dma(
    FirParams P, FirTaps T, EdgeTab Ex, EdgeTab Ey, EdgeTab Ez)
{
    typedef XyzGeom<HW, TY> G;
    constexpr int TXQ = G::TXQ, SQ = G::SQ, HALO = G::HALO, W = G::W, ROWS = G::ROWS, NB = G::NB, NT = G::NT;
    constexpr int NWAVE = G::NWAVE, NQ = G::NQ, NP = G::NP, TILEQ = G::TILEQ;
    extern __shared__ float4 smem[];
    float4 *const stg = smem;                          // [NB][TILEQ]: staged source rows, SQ quads each
    float4 *const xf = smem + NB * TILEQ;              // [ROWS][TXQ]: the x-filtered rows of the open request
    int *const seq = reinterpret_cast<int *>(xf + ROWS * TXQ);
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int qx = tid % TXQ, ty = tid / TXQ;
    const int x0 = blockIdx.x * (4 * TXQ);
    const int x = x0 + qx * 4;
    const int y0 = blockIdx.y * TY;
    const int y = y0 + ty;
    const int nx = P.nx, ny = P.ny;
    const size_t plane = (size_t)nx * ny;
    const int nl1 = P.nz - 1;
    const int endz = nl1, endy = ny - 1, endx = nx - 1;
    const int p0 = blockIdx.z * P.ts;
    const int p1 = min(p0 + P.ts, P.nz);

    // DMA pieces of this wave: piece pc = NWAVE k + wave (beyond the tile: the last piece once more -- the same
    // bytes to the same place -- so that every wave has two pieces per request in flight); lane -> flat quad
    // f = 64 pc + lane -> (tile row f / SQ, quad f % SQ); the source row of tile row j is extended-y index
    // y0 - HW + j (virtual and unused rows and the padding of the last piece: any valid row), its source column
    // x0 - HALO + 4 (f % SQ), clamped into the row
    size_t srcoff[2];
    uint32_t pcoff[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int pc = min(NWAVE * k + wave, NP - 1);
        const int f = 64 * pc + lane;
        const int j = min(f / SQ, ROWS - 1);
        const int i = y0 - HW + j;
        const int sr = i < 0 ? min(-i, endy) : min(i, endy);
        const int xq = clampi(x0 - HALO + 4 * (f % SQ), 0, nx - 4);
        srcoff[k] = (size_t)sr * nx + xq;
        pcoff[k] = (uint32_t)__builtin_amdgcn_readfirstlane(pc * 1024);
    }
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float4 *)stg;
    auto issue = [&](int pl, int b) {
        const float *src = P.src + (size_t)pl * plane;
        const uint32_t tb = lds0 + (uint32_t)(b * (TILEQ * 16));
#pragma unroll
        for (int k = 0; k < 2; k++)
            dma_load_lds_16(src + srcoff[k], (uint32_t)__builtin_amdgcn_readfirstlane((int)(tb + pcoff[k])));
    };
    // x edges (block-uniform): the first tile column mirrors E[-e] = src[e], e = 1 .. HALO; the last one forms
    // E[endx + m], m = 0 .. HW.  Thread -> (row tid / 16 [+ TY], sample tid % 16); positions in floats from the
    // row's start, source sample s at HALO + s - x0
    const bool xlo = blockIdx.x == 0, xhi = blockIdx.x == gridDim.x - 1;
    const int xe = tid & 15;
    int xpos = 0;
    float xw0 = 0.0f, xw1 = 0.0f;
#pragma unroll
    for (int mm = 0; mm <= HW; mm++)
        if (mm == xe) {
            xpos = clampi(Ex.lo[mm], 0, endx - 1) - x0 + HALO;
            xw0 = Ex.w0[mm];
            xw1 = Ex.w1[mm];
        }
    xpos = clampi(xpos, 0, 4 * SQ - 2);
    const DmaYEdge<HW, ROWS> ye(Ey, y0, TY, endy, ty, qx);
    float smax = 1.0f;
    if (SCALED) {
        smax = *P.scale_max;
        smax = smax != 0.0f ? smax : 1.0f;                     // imutil.c:706-707 (then every sample is 0)
    }
    // x- and y-filtered value of this thread's column from staged tile b
    auto filter = [&](int b) -> float4 {
        float4 *const tile = stg + b * TILEQ;
        if (SCALED) {
            for (int f = tid; f < NQ; f += NT) {
                float4 q = tile[f];
                q.x = q.x / smax; q.y = q.y / smax; q.z = q.z / smax; q.w = q.w / smax;   // imutil.c:711
                tile[f] = q;
            }
            dma_lds_barrier();
        }
        if (xlo || xhi) {
            for (int r = tid >> 4; r < ROWS; r += TY) {
                float *const row = reinterpret_cast<float *>(tile + r * SQ);
                if (xlo && xe < HALO)
                    row[HALO - 1 - xe] = row[HALO + 1 + xe];
                if (xhi && xe <= HW) {
                    const float a = row[xpos], c = row[xpos + 1];
                    row[HALO + 4 * TXQ - 1 + xe] = xw0 * a + xw1 * c;
                }
            }
            dma_lds_barrier();
        }
        // x phase: row-quad (r, qx) of the tile, r = ty and (the first 2 HW rows of threads) ty + TY
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int r = ty + k * TY;
            if (r < ROWS) {
                float w[4 + 2 * HALO];
#pragma unroll
                for (int i = 0; i < (4 + 2 * HALO) / 4; i++) {
                    const float4 q = tile[r * SQ + qx + i];
                    w[4 * i] = q.x; w[4 * i + 1] = q.y; w[4 * i + 2] = q.z; w[4 * i + 3] = q.w;
                }
                float o[4];
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    float acc = 0.0f;
#pragma unroll
                    for (int dd = -HW; dd <= HW; dd++)
                        acc += T.k[dd + HW] * w[HALO + c - dd];   // E[x - d], d ascending
                    o[c] = acc;
                }
                xf[r * TXQ + qx] = make_float4(o[0], o[1], o[2], o[3]);
            }
        }
        dma_lds_barrier();
        return dma_filter_y<HW>(T, ye, xf, qx);
    };
    DmaSweep s = dma_begin<HW>(seq, Ez, 2, p0, p1, 0, endz, P.nz - 1, issue);
    // extended-z plane r; the one-request path up to 11 taps (see dma_ext_z)
    auto ext_z = [&](int r, bool stores) -> float4 { return dma_ext_z<HW, 5>(s, Ez, r, endz, stores, issue, filter); };
    // the z ring, as in k_fir_yz_dma (every wave of a whole tile stores)
    float4 ring[W];
#pragma unroll
    for (int i = 0; i < W; i++)
        ring[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    // warm-up: planes p0 - HW .. p0 + HW - 1 into ring[0 .. 2*HW - 1] (static positions)
#pragma unroll
    for (int i = 0; i < 2 * HW; i++)
        ring[i] = ext_z(p0 - HW + i, false);
    float *__restrict__ d = P.dst + (size_t)y * nx + x;
#pragma unroll 1
    for (int q0 = p0; q0 < p1; q0 += W) {
#pragma unroll
        for (int j = 0; j < W; j++) {
            const int q = q0 + j;
            if (q < p1) {                              // block-uniform
                ring[(j + 2 * HW) % W] = ext_z(q + HW, true);
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int dd = -HW; dd <= HW; dd++)
                    Vec<4>::mac(acc, T.k[dd + HW], ring[(j + HW - dd) % W]);   // E[q - d], d ascending
                st4(d + (size_t)q * plane, acc);
            }
        }
    }
    dma_drain();
}

template <int HW, int TY, bool SCALED>
static hipError_t launch_fir_xyz_t(const FirParams &P, const FirTaps &T, const EdgeTab &Ex, const EdgeTab &Ey,
                                   const EdgeTab &Ez, int nseg, hipStream_t st)
{
    typedef XyzGeom<HW, TY> G;
    auto kern = k_fir_xyz_dma<HW, TY, SCALED>;
    // more than 64 KB of dynamic LDS has to be allowed once per instance and device (bit = device ordinal)
    static std::atomic<unsigned long long> allowed{0};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess)
        return e;
    if (dev < 0 || dev >= 64 || !((allowed.load(std::memory_order_relaxed) >> dev) & 1)) {
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)G::LDS_BYTES);
        if (e != hipSuccess)
            return e;
        if (dev >= 0 && dev < 64)
            allowed.fetch_or(1ull << dev, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(kern, dim3(P.nx / 64, P.ny / TY, nseg), dim3(G::NT), G::LDS_BYTES, st, P, T, Ex, Ey, Ez);
    return hipSuccess;
}

// tile height per half width: k_fir_yz_dma's choice (64 rows at 3 and 5 taps, 32 above)
template <int HW>
static hipError_t launch_fir_xyz(const FirParams &P, const FirTaps &T, const EdgeTab &Ex, const EdgeTab &Ey,
                                 const EdgeTab &Ez, int nseg, hipStream_t st)
{
    constexpr int DTY = HW <= 2 ? 64 : 32;
    return P.scale_max ? launch_fir_xyz_t<HW, DTY, true>(P, T, Ex, Ey, Ez, nseg, st)
                       : launch_fir_xyz_t<HW, DTY, false>(P, T, Ex, Ey, Ez, nseg, st);
}

extern "C" {

// does sift3d_hip_fir_xyz cover this blur?  Unit tap spacing on all three axes, whole 64 x 64 tiles of at
// least two tile rows, at most 17 taps, distinct 16-byte aligned volumes.
int sift3d_hip_fir_xyz_covers(const float *d_src, const float *d_dst, int nx, int ny, int nz, int width,
                              float uf_x, float uf_y, float uf_z)
{
    const int hw = width / 2;
    return d_src && d_dst && d_src != d_dst && (width & 1) && hw >= 1 && hw <= 8 && uf_x == 1.0f && uf_y == 1.0f &&
           uf_z == 1.0f && nx >= 64 && (nx & 63) == 0 && (ny & 63) == 0 && ny >= 128 && nz >= 1 && nz < (1 << 22) &&
           ny < (1 << 22) && nx < (1 << 22) && ((((uintptr_t)d_src | (uintptr_t)d_dst) & 15) == 0);
}

// One blur of a unit-spaced volume, all of its planes: dst = FIR_z(FIR_y(FIR_x(src))), or of src / *d_scale_max
// where d_scale_max is not null.  Returns 1 without doing anything when the configuration is not covered.
int sift3d_hip_fir_xyz(const float *d_src, float *d_dst, int nx, int ny, int nz, const float *taps, int width,
                       const float *d_scale_max, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const int hw = width / 2;
    if (!d_src || !d_dst || !taps || nx < 1 || ny < 1 || nz < 1 || width < 1)
        return launch_fail("sift3d_hip_fir_xyz", "invalid arguments");
    if (!sift3d_hip_fir_xyz_covers(d_src, d_dst, nx, ny, nz, width, 1.0f, 1.0f, 1.0f))
        return 1;
    if (overlap(d_src, sizeof(float) * (size_t)nx * ny * nz, d_dst, sizeof(float) * (size_t)nx * ny * nz))
        return launch_fail("sift3d_hip_fir_xyz", "source and destination overlap");
    FirParams P;
    FirTaps T;
    fir_dma_fill(&P, &T, d_src, d_dst, nx, ny, nz, taps, width);
    P.scale_max = d_scale_max;
    int nseg;
    fir_dma_segments((long)(nx / 64) * (ny / 32), nz, &P.ts, &nseg);
    const EdgeTab Ex = edge_table(nx, hw), Ey = edge_table(ny, hw), Ez = edge_table(nz, hw);
    hipError_t e = hipSuccess;
    dispatch_int_or<1, 8, 8>(hw, [&](auto H) { e = launch_fir_xyz<decltype(H)::value>(P, T, Ex, Ey, Ez, nseg, st); });
    HIPCHK(e);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

} // extern "C"
