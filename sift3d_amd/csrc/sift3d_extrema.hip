// sift3d_extrema.hip -- the extrema stage of the detect path: the DoG kernels (differences of the Gaussian
// levels and their max |DoG|) and detect_extrema (sift.c:735-871) as mask -> count -> scan -> emit, with the
// three generations of the mask step: k_extrema_mask (any configuration), k_extrema_sweep3 (five stored DoG
// levels) and k_extrema_sweep3g (straight from the six Gaussian levels: the default).  Numerical contract and
// citations as in sift3d_kernels.hip.
#include "sift3d_kernels_common.h"
#include <cstdlib>

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// ---------------------------------------------------------------------------------------
// im_subtract + dogmax  (imutil.c:719-739, sift.c:821-826)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sub_absmax(const float *__restrict__ a,
                                                    const float *__restrict__ b,
                                                    float *__restrict__ dst, size_t n,
                                                    unsigned *__restrict__ out)
{
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nthr = (size_t)gridDim.x * blockDim.x;
    const size_t n4 = n >> 2;
    float m = 0.0f;
    // four independent 16-byte load pairs in flight per thread and iteration
    size_t i = tid;
    for (; i + 3 * nthr < n4; i += 4 * nthr) {
        float4 u[4], v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            u[k] = ld4(a + 4 * (i + k * nthr));
            v[k] = ld4(b + 4 * (i + k * nthr));
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float4 r;
            r.x = u[k].x - v[k].x; r.y = u[k].y - v[k].y; r.z = u[k].z - v[k].z; r.w = u[k].w - v[k].w;
            st4(dst + 4 * (i + k * nthr), r);
            m = fmaxf(m, fmaxf(fmaxf(fabsf(r.x), fabsf(r.y)), fmaxf(fabsf(r.z), fabsf(r.w))));
        }
    }
    for (; i < n4; i += nthr) {
        const float4 u = ld4(a + 4 * i), v = ld4(b + 4 * i);
        float4 r;
        r.x = u.x - v.x; r.y = u.y - v.y; r.z = u.z - v.z; r.w = u.w - v.w;
        st4(dst + 4 * i, r);
        m = fmaxf(m, fmaxf(fmaxf(fabsf(r.x), fabsf(r.y)), fmaxf(fabsf(r.z), fabsf(r.w))));
    }
    for (size_t j = 4 * n4 + tid; j < n; j += nthr) {
        const float r = a[j] - b[j];
        dst[j] = r;
        m = fmaxf(m, fabsf(r));
    }
    if (out)                                   // kernel argument: uniform
        block_max_atomic<1>(&m, out);
}

// All DoG levels of one octave in one pass: NL Gaussian levels are read once (4*NL B/voxel) and
// NL-1 differences written, instead of 12 B/voxel per level pair.  Same arithmetic and the same
// order-free max as k_sub_absmax.
struct DogStack {
    const float *g[SIFT3D_HIP_MAX_DOG_STACK];
    float *d[SIFT3D_HIP_MAX_DOG_STACK - 1];
    unsigned *out; // NL-1 consecutive maxima (float bits)
};

template <int NL>
__global__ __launch_bounds__(256) void k_dog_stack(DogStack S, size_t n)
{
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nthr = (size_t)gridDim.x * blockDim.x;
    const size_t n4 = n >> 2;
    float m[NL - 1];
#pragma unroll
    for (int k = 0; k < NL - 1; k++)
        m[k] = 0.0f;
    for (size_t i = tid; i < n4; i += nthr) {
        float4 v[NL];
#pragma unroll
        for (int k = 0; k < NL; k++)
            v[k] = ld4(S.g[k] + 4 * i);
#pragma unroll
        for (int k = 0; k < NL - 1; k++) {
            float4 r;
            r.x = v[k].x - v[k + 1].x; r.y = v[k].y - v[k + 1].y;
            r.z = v[k].z - v[k + 1].z; r.w = v[k].w - v[k + 1].w;
            st4(S.d[k] + 4 * i, r);
            m[k] = fmaxf(m[k], fmaxf(fmaxf(fabsf(r.x), fabsf(r.y)), fmaxf(fabsf(r.z), fabsf(r.w))));
        }
    }
    for (size_t j = 4 * n4 + tid; j < n; j += nthr) {
        float prev = S.g[0][j];
#pragma unroll
        for (int k = 0; k < NL - 1; k++) {
            const float cur = S.g[k + 1][j];
            const float r = prev - cur;
            S.d[k][j] = r;
            m[k] = fmaxf(m[k], fabsf(r));
            prev = cur;
        }
    }
    block_max_atomic<NL - 1>(m, S.out);
}

// The same maxima without the DoG levels themselves: the extrema sweep below forms the
// differences on the fly from the Gaussian levels, so the DoG pyramid is never stored
// (24 B/voxel read here instead of 24 B read + 20 B written, and 5/11 of the pyramid memory).
template <int NL>
__global__ __launch_bounds__(256) void k_dogmax_stack(DogStack S, size_t n)
{
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nthr = (size_t)gridDim.x * blockDim.x;
    const size_t n4 = n >> 2;
    float m[NL - 1];
#pragma unroll
    for (int k = 0; k < NL - 1; k++)
        m[k] = 0.0f;
    for (size_t i = tid; i < n4; i += nthr) {
        float4 v[NL];
#pragma unroll
        for (int k = 0; k < NL; k++)
            v[k] = ld4(S.g[k] + 4 * i);
#pragma unroll
        for (int k = 0; k < NL - 1; k++) {
            float4 r;
            r.x = v[k].x - v[k + 1].x; r.y = v[k].y - v[k + 1].y;
            r.z = v[k].z - v[k + 1].z; r.w = v[k].w - v[k + 1].w;
            m[k] = fmaxf(m[k], fmaxf(fmaxf(fabsf(r.x), fabsf(r.y)), fmaxf(fabsf(r.z), fabsf(r.w))));
        }
    }
    for (size_t j = 4 * n4 + tid; j < n; j += nthr) {
        float prev = S.g[0][j];
#pragma unroll
        for (int k = 0; k < NL - 1; k++) {
            const float cur = S.g[k + 1][j];
            m[k] = fmaxf(m[k], fabsf(prev - cur));
            prev = cur;
        }
    }
    block_max_atomic<NL - 1>(m, S.out);
}

// ---------------------------------------------------------------------------------------
// detect_extrema  (sift.c:735-871): mask -> scan -> emit, output in scan order
// ---------------------------------------------------------------------------------------
constexpr int EX_WPB = 128; // 64-voxel words per block (32 per wave)

struct ExLevels {
    sift3d_hip_extrema_level lv[8];
};

struct ExGeom {
    int nx, ny, nz;
    int wpr;        // words per row = ceil(nx / 64)
    uint32_t nwords;// nz * ny * wpr
    uint32_t nblk;  // ceil(nwords / EX_WPB)
    double peak_thresh;
    int cuboid;     // 1: the reference's CUBOID_EXTREMA build (80 neighbours, sift.c:761-796)
};

// CMP_CUBE of the CUBOID_EXTREMA build (sift.c:761-796): strictly above (or strictly below) all
// 27 samples of the previous and next DoG level and the 26 neighbours in the current one
__device__ __forceinline__ bool cuboid_extremum(const float *__restrict__ prev,
                                                const float *__restrict__ cur,
                                                const float *__restrict__ next, size_t q, size_t ys,
                                                size_t zs, float c)
{
    bool gt = true, lt = true;
#pragma unroll
    for (int dz = -1; dz <= 1; dz++)
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const size_t r = q + dx + ys * dy + zs * dz;
                const float a = prev[r], b = next[r];
                gt = gt && c > a && c > b;
                lt = lt && c < a && c < b;
                if (dx || dy || dz) {
                    const float m = cur[r];
                    gt = gt && c > m;
                    lt = lt && c < m;
                }
            }
    return gt || lt;
}

template <bool CUBOID>
__global__ __launch_bounds__(256) void k_extrema_mask(ExLevels LV, ExGeom E,
                                                      unsigned long long *__restrict__ masks,
                                                      uint32_t *__restrict__ blk_counts)
{
    __shared__ uint32_t wc[4];
    constexpr int WPW = EX_WPB / 4; // words per wave
    const int level = blockIdx.y;
    const sift3d_hip_extrema_level L = LV.lv[level];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // thr = (float)(peak_thresh * dogmax), sift.c:829
    const float thr = (float)(E.peak_thresh * (double)(*L.d_absmax));
    const size_t ys = E.nx, zs = (size_t)E.nx * E.ny;
    const uint32_t wbase = blockIdx.x * EX_WPB + wave * WPW;
    uint32_t cnt = 0;
    if (wbase < E.nwords) {
        // (z, y, word-in-row) of the wave's first word; advanced without divisions afterwards
        const uint32_t row0 = wbase / E.wpr;
        int xw = (int)(wbase - row0 * E.wpr);
        int z = (int)(row0 / E.ny), y = (int)(row0 - (uint32_t)z * E.ny);
        const uint32_t wend = min(wbase + WPW, E.nwords);
        for (uint32_t word = wbase; word < wend; word += 4) {
            // four words per iteration: their centre samples are loaded together
            float v[4];
            size_t p[4];
            bool ok[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int x = xw * 64 + lane;
                ok[k] = word + k < wend && z >= L.z_lo && z < L.z_hi && y >= 1 && y <= E.ny - 2 &&
                        x >= 1 && x <= E.nx - 2;
                p[k] = (size_t)x + ys * y + zs * z;
                v[k] = ok[k] ? L.cur[p[k]] : 0.0f;
                if (++xw == E.wpr) {
                    xw = 0;
                    if (++y == E.ny) {
                        y = 0;
                        ++z;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                bool hit = false;
                if (CUBOID) {
                    if (ok[k] && (v[k] > thr || v[k] < -thr))            // sift.c:842
                        hit = cuboid_extremum(L.prev, L.cur, L.next, p[k], ys, zs, v[k]);
                } else if (ok[k] && (v[k] > thr || v[k] < -thr)) {       // sift.c:842
                    const size_t q = p[k];
                    const float c = v[k];
                    const float n0 = L.prev[q], n1 = L.cur[q + 1], n2 = L.cur[q - 1],
                                n3 = L.cur[q + ys], n4 = L.cur[q - ys], n5 = L.cur[q - zs],
                                n6 = L.cur[q + zs], n7 = L.next[q];
                    hit = (c > n0 && c > n1 && c > n2 && c > n3 && c > n4 && c > n5 && c > n6 &&
                           c > n7) ||
                          (c < n0 && c < n1 && c < n2 && c < n3 && c < n4 && c < n5 && c < n6 &&
                           c < n7);                                      // sift.c:844-849
                }
                const unsigned long long m = __ballot(hit);
                if (word + k < wend) {
                    if (lane == 0)
                        masks[(size_t)level * E.nwords + word + k] = m;
                    cnt += (uint32_t)__popcll(m);
                }
            }
        }
    }
    if (lane == 0)
        wc[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0)
        blk_counts[(size_t)level * E.nblk + blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// ---- three keypoint levels in one z sweep (default 8-neighbour test) -----------------------
// The three keypoint levels of an octave share their DoG levels (next of level i = centre of
// level i+1), and the scattered neighbour lines of k_extrema_mask cost ~4x the centre samples.
// Here a workgroup owns a 64(x) x 16(y) column and walks z: every thread keeps three planes
// (z-1, z, z+1) of the three centre levels in registers, so each of the five DoG levels is read
// once along z; the y neighbours are two more (cache-resident) row loads, the x neighbours come
// from the adjacent lanes (DPP row shift; one scalar load at the tile's ends).  Output: the same
// 64-voxel mask words as k_extrema_mask, assembled with a DPP OR-reduction over the 16 lanes of
// a row, so the scan and emit kernels (and with them the reference's scan order) are unchanged.
struct ExSweep {
    const float *d[6];        // DoG levels s-1 .. s+3 of the three keypoint levels (k_extrema_sweep3) or
                              // the SIX Gaussian levels they are differences of (k_extrema_sweep3g)
    const float *absmax[3];
    double peak_thresh;
    int nx, ny, nz;           // local dims
    int z_lo, z_hi, ts;       // output planes [z_lo, z_hi), segment length
    int wpr;
    uint32_t nwords;
    uint32_t *masks32;        // [3][nwords] 64-bit words as uint32 pairs
    unsigned *exact;          // k_extrema_sweep3g<.., true>: the five max|DoG| of the octave are gathered here
};

// v_max3_f32 / v_min3_f32 (operands that are not NaN: the result is the exact maximum / minimum)
__device__ __forceinline__ float max3f(float a, float b, float c)
{
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float min3f(float a, float b, float c)
{
    float r;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

__device__ __forceinline__ float max2f(float a, float b)
{
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float min2f(float a, float b)
{
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

template <int CTRL> __device__ __forceinline__ int dpp_i(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);   // out-of-row lanes read 0
}

// (Stored DoG levels; the default configuration has none and runs k_extrema_sweep3g below.)
__global__ __launch_bounds__(256) void k_extrema_sweep3(ExSweep S)
{
    auto ldd4 = [&](int k, size_t o) -> float4 { return ld4(S.d[k] + o); };
    auto ldd1 = [&](int k, size_t o) -> float { return S.d[k][o]; };
    constexpr int TY = 16;
    const int qx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int x = (blockIdx.x * 16 + qx) * 4, y = blockIdx.y * TY + ty;
    const int nx = S.nx, ny = S.ny;
    const size_t ys = nx, zs = (size_t)nx * ny;
    const bool col = x < nx && y < ny;                 // (nx % 4 == 0: whole quads)
    const int yc = min(y, ny - 1), xc = min(x, nx - 4);
    const int yu = max(yc - 1, 0), yd = min(yc + 1, ny - 1);
    const size_t oc = (size_t)yc * ys + xc, ou = (size_t)yu * ys + xc, od = (size_t)yd * ys + xc;
    const int p0 = S.z_lo + blockIdx.z * S.ts, p1 = min(p0 + S.ts, S.z_hi);
    if (p0 >= p1)
        return;
    float thr[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
        thr[i] = (float)(S.peak_thresh * (double)(*S.absmax[i]));        // sift.c:829
    // which of the quad's four voxels may be extrema at all (sift.c:833-838: 1 .. n-2)
    bool okx[4];
#pragma unroll
    for (int e = 0; e < 4; e++)
        okx[e] = col && y >= 1 && y <= ny - 2 && x + e >= 1 && x + e <= nx - 2;
    float4 m[3], c[3], p[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        m[i] = ldd4(i + 1, (size_t)(p0 - 1) * zs + oc);
        c[i] = ldd4(i + 1, (size_t)p0 * zs + oc);
    }
#pragma unroll 1
    for (int z = p0; z < p1; z++) {
        const size_t zo = (size_t)z * zs;
        float4 up[3], dn[3];
        float lf[3], rt[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            p[i] = ldd4(i + 1, zo + zs + oc);
            up[i] = ldd4(i + 1, zo + ou);
            dn[i] = ldd4(i + 1, zo + od);
            // x neighbours of the quad's ends: adjacent lanes of the 16-lane row, or memory at
            // the ends of the 64-voxel tile
            lf[i] = __int_as_float(dpp_i<0x111>(__float_as_int(c[i].w)));   // row_shr:1
            rt[i] = __int_as_float(dpp_i<0x101>(__float_as_int(c[i].x)));   // row_shl:1
            if (qx == 0 && col && x > 0)
                lf[i] = ldd1(i + 1, zo + oc - 1);
            if (qx == 15 && col && x + 4 < nx)
                rt[i] = ldd1(i + 1, zo + oc + 4);
        }
        const float4 d0c = ldd4(0, zo + oc), d4c = ldd4(4, zo + oc);
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const float4 pv = i == 0 ? d0c : c[i - 1], nv = i == 2 ? d4c : c[i + 1];
            const float cv[4] = { c[i].x, c[i].y, c[i].z, c[i].w };
            const float pr[4] = { pv.x, pv.y, pv.z, pv.w }, ne[4] = { nv.x, nv.y, nv.z, nv.w };
            const float uu[4] = { up[i].x, up[i].y, up[i].z, up[i].w };
            const float dd[4] = { dn[i].x, dn[i].y, dn[i].z, dn[i].w };
            const float zm[4] = { m[i].x, m[i].y, m[i].z, m[i].w };
            const float zp[4] = { p[i].x, p[i].y, p[i].z, p[i].w };
            int nib = 0;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const float v = cv[e];
                const float xm = e > 0 ? cv[e - 1] : lf[i], xp = e < 3 ? cv[e + 1] : rt[i];
                const bool hit =
                    okx[e] && (v > thr[i] || v < -thr[i]) &&                           // sift.c:842
                    ((v > pr[e] && v > xp && v > xm && v > dd[e] && v > uu[e] && v > zm[e] &&
                      v > zp[e] && v > ne[e]) ||
                     (v < pr[e] && v < xp && v < xm && v < dd[e] && v < uu[e] && v < zm[e] &&
                      v < zp[e] && v < ne[e]));                                        // sift.c:844-849
                nib |= hit ? (1 << e) : 0;
            }
            // 64-bit word of the row: voxel 4*qx + e -> bit 4*qx + e; OR over the 16 lanes
            int lo = qx < 8 ? nib << (4 * qx) : 0, hi = qx >= 8 ? nib << (4 * (qx - 8)) : 0;
            lo |= dpp_i<0x111>(lo); hi |= dpp_i<0x111>(hi);
            lo |= dpp_i<0x112>(lo); hi |= dpp_i<0x112>(hi);
            lo |= dpp_i<0x114>(lo); hi |= dpp_i<0x114>(hi);
            lo |= dpp_i<0x118>(lo); hi |= dpp_i<0x118>(hi);
            if (qx == 15 && y < ny) {
                const size_t w = (size_t)i * S.nwords + ((size_t)z * ny + y) * S.wpr + blockIdx.x;
                *reinterpret_cast<uint2 *>(S.masks32 + 2 * w) = make_uint2((unsigned)lo, (unsigned)hi);
            }
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            m[i] = c[i];
            c[i] = p[i];
        }
    }
}

// ---- the same sweep straight from the SIX Gaussian levels, every sample loaded once ----------
// Forming the differences inside k_extrema_sweep3's loads would ask the memory system for ~26 KB
// per wave and plane (the y neighbours and both Gaussian levels of every difference loaded again by
// every thread that needs them): 5x the bytes of the levels, and the L2 -> L1 path, not HBM, then
// sets the time (round 2 started that way).  Here a thread loads
// exactly its own quad of each Gaussian level once per plane (G1..G4 one plane ahead, G0 and G5 at
// the centre plane), keeps what the next step needs in registers, and the workgroup trades the
// centre-plane differences through an LDS tile (64 x 16 voxels + one halo row above and below,
// loaded by 32 of the 256 threads) for the y neighbours.  One barrier per plane (the tile is
// double-buffered).  Arithmetic, order of the tests and output are those of k_extrema_sweep3.
// EST: S.absmax[] hold LOWER BOUNDS of the three maxima (k_dogmax_sub's maxima over a sub-lattice), so the
// masks are a SUPERSET of the reference's; the sweep gathers the exact maxima of all five DoG levels over
// its centre planes on the way (it forms every difference of those planes anyway) and
// k_extrema_refilter then applies the reference's threshold (sift.c:829, 842) to the marked voxels.  The
// octave's Gaussian levels are read once instead of twice.
template <int TXQ, bool EST = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_extrema_sweep3g(ExSweep S)
{
    constexpr int TY = 256 / TXQ;          // tile: 4 * TXQ voxels along x, TY rows
    __shared__ float4 tile[2][3][TY + 2][TXQ];
    const int qx = threadIdx.x % TXQ, ty = threadIdx.x / TXQ;
    const int q16 = qx & 15;               // position in the 16-lane row = the 64-voxel mask word
    // Workgroups go to the eight XCDs round robin in launch order, and an XCD's L2 is its own: tiles that share
    // halo rows (y neighbours) should meet in ONE L2.  XCD k takes the k-th eighth of the tiles in (x, y, z
    // segment) order -- at 512^3 exactly one z segment --, in that order.
    int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
    {
        const unsigned gx = gridDim.x, gy = gridDim.y, T = gx * gy * gridDim.z;
        const unsigned L = bx + gx * (by + gy * bz), xcd = L & 7u, j = L >> 3;
        const unsigned q = T >> 3, r = T & 7u;
        const unsigned t = xcd * q + (xcd < r ? xcd : r) + j;
        bx = (int)(t % gx);
        by = (int)((t / gx) % gy);
        bz = (int)(t / (gx * gy));
    }
    const int x = (bx * TXQ + qx) * 4, y0 = by * TY, y = y0 + ty;
    const int nx = S.nx, ny = S.ny;
    const size_t ys = nx, zs = (size_t)nx * ny;
    const bool col = x < nx && y < ny;                 // (nx % 4 == 0: whole quads)
    const int yc = min(y, ny - 1), xc = min(x, nx - 4);
    const size_t oc = (size_t)yc * ys + xc;
    // halo rows of the tile (rows y0 - 1 and y0 + TY, clamped like the y neighbours of the
    // reference loop's border voxels, which are never extrema): threads 0..31
    const bool halo = threadIdx.x < 2 * TXQ;
    const int hr = threadIdx.x / TXQ;                  // 0: row above, 1: row below (halo threads)
    const int yh = hr == 0 ? max(y0 - 1, 0) : min(y0 + TY, ny - 1);
    const size_t oh = (size_t)yh * ys + xc;
    const int p0 = S.z_lo + bz * S.ts, p1 = min(p0 + S.ts, S.z_hi);
    if (p0 >= p1)
        return;
    float thr[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
        thr[i] = (float)(S.peak_thresh * (double)(*S.absmax[i]));        // sift.c:829
    bool okx[4];
#pragma unroll
    for (int e = 0; e < 4; e++)
        okx[e] = col && y >= 1 && y <= ny - 2 && x + e >= 1 && x + e <= nx - 2;
    auto sub4 = [](const float4 &a, const float4 &b) {
        return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);   // im_subtract, imutil.c:719-739
    };
    float mx[5] = { 0.f, 0.f, 0.f, 0.f, 0.f };
    auto amax4 = [](float mm, const float4 &v) {
        float r;
        asm("v_max3_f32 %0, %1, |%2|, |%3|" : "=v"(r) : "v"(mm), "v"(v.x), "v"(v.y));
        asm("v_max3_f32 %0, %1, |%2|, |%3|" : "=v"(r) : "v"(r), "v"(v.z), "v"(v.w));
        return r;
    };
    // differences 1..3 at planes z-1 (m), z (c), z+1 (p); Gaussian levels 1 and 4 at plane z
    float4 m[3], c[3], p[3], g1c, g4c;
    {
        float4 a[4], b[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            a[k] = ld4(S.d[k + 1] + (size_t)(p0 - 1) * zs + oc);
            b[k] = ld4(S.d[k + 1] + (size_t)p0 * zs + oc);
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            m[i] = sub4(a[i], a[i + 1]);
            c[i] = sub4(b[i], b[i + 1]);
        }
        g1c = b[0];
        g4c = b[3];
        // (the halo rows' differences go straight into the tile the plane will use: the buffer of the NEXT
        // plane was last read two planes ago, behind a barrier; nothing of them is carried in registers)
        if (halo) {
            float4 h[4];
#pragma unroll
            for (int k = 0; k < 4; k++)
                h[k] = ld4(S.d[k + 1] + (size_t)p0 * zs + oh);
#pragma unroll
            for (int i = 0; i < 3; i++)
                tile[0][i][hr * (TY + 1)][qx] = sub4(h[i], h[i + 1]);
        }
    }
    // The x neighbours of a row segment's two end quads come from memory (every other one from the adjacent
    // lane): Gaussian levels 1..4 at x - 1 (lane qx == 0) or x + 4 (lane qx == TXQ - 1) of the centre plane.
    // They are requested ONE PLANE AHEAD, like every other sample of the sweep: requested where they are
    // needed, each of the six differences cost the wave a full memory round trip per plane -- s_waitcnt
    // vmcnt(0) six times, draining the plane's 16-byte loads with it -- and every wave of a 256-voxel row
    // segment holds both end lanes (measured: 6.8 us per plane and workgroup, 2.7 TB/s).
    const bool edge = col && ((qx == 0 && x > 0) || (qx == TXQ - 1 && x + 4 < nx));
    const size_t oe = oc + (qx == 0 ? (size_t)-1 : (size_t)4);
    float ed[3] = { 0.f, 0.f, 0.f };          // centre plane's differences (beyond the volume: 0, as before)
    if (edge) {
        float e0[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
            e0[k] = S.d[k + 1][(size_t)p0 * zs + oe];
#pragma unroll
        for (int i = 0; i < 3; i++)
            ed[i] = e0[i] - e0[i + 1];
    }
    int buf = 0;
#pragma unroll 1
    for (int z = p0; z < p1; z++) {
        const size_t zo = (size_t)z * zs;
        // centre-plane differences into the tile (known since the previous step)
#pragma unroll
        for (int i = 0; i < 3; i++)
            tile[buf][i][ty + 1][qx] = c[i];
        // this step's loads: every Gaussian level once
        float4 n[4], hn[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
            n[k] = ld4(S.d[k + 1] + zo + zs + oc);
        const float4 g0 = ld4(S.d[0] + zo + oc), g5 = ld4(S.d[5] + zo + oc);
        if (halo) {
#pragma unroll
            for (int k = 0; k < 4; k++)
                hn[k] = ld4(S.d[k + 1] + zo + zs + oh);
        }
        float en[4] = { 0.f, 0.f, 0.f, 0.f };     // the end quads' outer neighbours of the NEXT centre plane
        if (edge) {
#pragma unroll
            for (int k = 0; k < 4; k++)
                en[k] = S.d[k + 1][zo + zs + oe];
        }
        float lf[3], rt[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            // the neighbours come from the adjacent lanes of the WAVE (DPP wave shift; a wave holds
            // 64 / TXQ whole row segments), memory (ec, requested a plane ago) only at the two ends of a
            // row segment
            lf[i] = __int_as_float(dpp_i<0x138>(__float_as_int(c[i].w)));   // wave_shr:1
            rt[i] = __int_as_float(dpp_i<0x130>(__float_as_int(c[i].x)));   // wave_shl:1
            lf[i] = qx == 0 ? ed[i] : lf[i];
            rt[i] = qx == TXQ - 1 ? ed[i] : rt[i];
        }
        __syncthreads();
        float4 up[3], dn[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            up[i] = tile[buf][i][ty][qx];
            dn[i] = tile[buf][i][ty + 2][qx];
        }
        buf ^= 1;
#pragma unroll
        for (int i = 0; i < 3; i++)
            p[i] = sub4(n[i], n[i + 1]);
        const float4 d0c = sub4(g0, g1c), d4c = sub4(g4c, g5);
        if (EST && col) {
            // (clamped duplicates of the last column / row would not matter to a maximum either)
            mx[0] = amax4(mx[0], d0c);
            mx[1] = amax4(mx[1], c[0]);
            mx[2] = amax4(mx[2], c[1]);
            mx[3] = amax4(mx[3], c[2]);
            mx[4] = amax4(mx[4], d4c);
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const float4 pv = i == 0 ? d0c : c[i - 1], nv = i == 2 ? d4c : c[i + 1];
            const float cv[4] = { c[i].x, c[i].y, c[i].z, c[i].w };
            const float pr[4] = { pv.x, pv.y, pv.z, pv.w }, ne[4] = { nv.x, nv.y, nv.z, nv.w };
            const float uu[4] = { up[i].x, up[i].y, up[i].z, up[i].w };
            const float dd[4] = { dn[i].x, dn[i].y, dn[i].z, dn[i].w };
            const float zm[4] = { m[i].x, m[i].y, m[i].z, m[i].w };
            const float zp[4] = { p[i].x, p[i].y, p[i].z, p[i].w };
            int nib = 0;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const float v = cv[e];
                const float xm = e > 0 ? cv[e - 1] : lf[i], xp = e < 3 ? cv[e + 1] : rt[i];
                // "greater than each of the eight" = greater than their maximum (sift.c:844-849; the differences
                // of finite samples are never NaN): 3 x v_max3 + v_max and the same for the minimum instead of
                // sixteen compares and as many scalar ANDs -- the sweep's arithmetic, not its loads, is what a
                // plane costs beyond the copy rate.  (No short circuit: in a wave some lane nearly always passes
                // the threshold, so branches only cost.)
                const float hi8 = max2f(max3f(max3f(max3f(uu[e], dd[e], zm[e]), zp[e], pr[e]), ne[e], xm), xp);
                const float lo8 = min2f(min3f(min3f(min3f(uu[e], dd[e], zm[e]), zp[e], pr[e]), ne[e], xm), xp);
                const bool hit = okx[e] & (fabsf(v) > thr[i]) &                       // sift.c:842
                                 ((v > hi8) | (v < lo8));
                nib |= hit ? (1 << e) : 0;
            }
            // 64-bit word of the row: voxel 4*qx + e -> bit 4*qx + e; OR over the 16 lanes
            int lo = q16 < 8 ? nib << (4 * q16) : 0, hi = q16 >= 8 ? nib << (4 * (q16 - 8)) : 0;
            lo |= dpp_i<0x111>(lo); hi |= dpp_i<0x111>(hi);
            lo |= dpp_i<0x112>(lo); hi |= dpp_i<0x112>(hi);
            lo |= dpp_i<0x114>(lo); hi |= dpp_i<0x114>(hi);
            lo |= dpp_i<0x118>(lo); hi |= dpp_i<0x118>(hi);
            const int wcol = bx * (TXQ / 16) + (qx >> 4);     // 64-voxel word of the row
            if (q16 == 15 && wcol < S.wpr && y < ny) {
                const size_t w = (size_t)i * S.nwords + ((size_t)z * ny + y) * S.wpr + wcol;
                *reinterpret_cast<uint2 *>(S.masks32 + 2 * w) = make_uint2((unsigned)lo, (unsigned)hi);
            }
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            m[i] = c[i];
            c[i] = p[i];
        }
        g1c = n[0];
        g4c = n[3];
#pragma unroll
        for (int i = 0; i < 3; i++)
            ed[i] = en[i] - en[i + 1];
        if (halo) {
#pragma unroll
            for (int i = 0; i < 3; i++)
                tile[buf][i][hr * (TY + 1)][qx] = sub4(hn[i], hn[i + 1]);   // (buf: the next plane's)
        }
    }
    if (EST) {
        __syncthreads();                   // (block_max_atomic has a shared array of its own; the tile is done)
        block_max_atomic<5>(mx, S.exact);
    }
}

// max|DoG| of an octave's levels over the sub-lattice z = 1, 6, 11, ..., y = 0, 3, 6, ...: LOWER bounds of the
// maxima (k_extrema_sweep3g<.., true> wants nothing more of them), one fifteenth of the octave's bytes.  (Strides
// 5 and 3: a lattice point within (2, 1) voxels of every voxel, and no common factor with power-of-two
// structure in the data.)
constexpr int SUB_Z = 5, SUB_Y = 3;
template <int NL>
__global__ __launch_bounds__(256) void k_dogmax_sub(DogStack S, int nx, int ny, int nz)
{
    const uint32_t q = (uint32_t)nx >> 2, rpp = ((uint32_t)ny + SUB_Y - 1) / SUB_Y;
    const uint32_t npl = nz >= 2 ? ((uint32_t)nz - 2) / SUB_Z + 1 : 1;      // planes 1, 6, ... (plane 0 if nz < 2)
    const uint64_t items = (uint64_t)q * rpp * npl;
    const uint64_t nthr = (uint64_t)gridDim.x * blockDim.x;
    float m[NL - 1];
#pragma unroll
    for (int k = 0; k < NL - 1; k++)
        m[k] = 0.0f;
    for (uint64_t it = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += nthr) {
        const uint32_t r = (uint32_t)(it / q), qq = (uint32_t)(it - (uint64_t)r * q);
        const uint32_t pl = r / rpp, row = r - pl * rpp;
        const uint32_t z = nz >= 2 ? 1 + SUB_Z * pl : 0, y = SUB_Y * row;
        const size_t off = ((size_t)z * ny + y) * nx + 4 * qq;
        float4 v[NL];
#pragma unroll
        for (int k = 0; k < NL; k++)
            v[k] = ld4(S.g[k] + off);
#pragma unroll
        for (int k = 0; k < NL - 1; k++) {
            float4 r4;
            r4.x = v[k].x - v[k + 1].x; r4.y = v[k].y - v[k + 1].y;
            r4.z = v[k].z - v[k + 1].z; r4.w = v[k].w - v[k + 1].w;
            m[k] = fmaxf(m[k], fmaxf(fmaxf(fabsf(r4.x), fabsf(r4.y)), fmaxf(fabsf(r4.z), fabsf(r4.w))));
        }
    }
    block_max_atomic<NL - 1>(m, S.out);
}

// The masks of k_extrema_sweep3g<.., true> hold every extremum above a LOWER bound of the threshold; with
// the exact maxima known, the reference's test (sift.c:829, 842) is applied to the marked voxels: one
// thread per 64-voxel mask word, nearly all of them zero.
__global__ __launch_bounds__(256) void k_extrema_refilter(ExSweep S)
{
    const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= (uint64_t)3 * S.nwords)
        return;
    unsigned long long *word = reinterpret_cast<unsigned long long *>(S.masks32) + w;
    unsigned long long bits = *word;
    if (!bits)
        return;
    const int i = (int)(w / S.nwords);
    const uint32_t r = (uint32_t)(w - (uint64_t)i * S.nwords);
    const uint32_t rowi = r / (uint32_t)S.wpr, wc = r - rowi * (uint32_t)S.wpr;   // rowi = z * ny + y
    const size_t base = (size_t)rowi * S.nx + 64u * wc;
    const float thr = (float)(S.peak_thresh * (double)__uint_as_float(S.exact[1 + i]));    // sift.c:829
    const float *ga = S.d[i + 1], *gb = S.d[i + 2];
    unsigned long long keep = bits;
    while (bits) {
        const int b = __ffsll((long long)bits) - 1;
        bits &= bits - 1;
        const float v = ga[base + b] - gb[base + b];                               // im_subtract
        if (!((v > thr) | (v < -thr)))                                             // sift.c:842
            keep &= ~(1ull << b);
    }
    *word = keep;
}

// candidates per block of EX_WPB mask words (what k_extrema_mask counts itself)
__global__ __launch_bounds__(256) void k_extrema_count(const unsigned long long *__restrict__ masks,
                                                       uint32_t nwords, uint32_t nblk,
                                                       uint32_t *__restrict__ blk_counts)
{
    __shared__ uint32_t wc[4];
    const int level = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t cnt = 0;
    for (uint32_t w = blockIdx.x * EX_WPB + threadIdx.x; w < min((blockIdx.x + 1) * (uint32_t)EX_WPB, nwords);
         w += 256)
        cnt += (uint32_t)__popcll(masks[(size_t)level * nwords + w]);
    cnt = wave_sum_u32(cnt);
    if (lane == 0)
        wc[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0)
        blk_counts[(size_t)level * nblk + blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// exclusive scan of the block counts (all levels of the launch), continuing from *d_count.  One workgroup
// walks the array in chunks of 8192 entries: a thread loads eight consecutive entries (two 16-byte loads,
// coalesced), scans them, the thread sums are scanned by wave shifts and the sixteen wave totals by the
// first wave -- two barriers per chunk (49 152 entries at 512^3: 6 chunks; the chunked Hillis-Steele scan
// this replaces took 480 barriers and 85 us there).
__device__ __forceinline__ uint32_t ex_scan_range(uint32_t *__restrict__ blk, uint32_t n, uint32_t carry,
                                                  uint32_t *wtot, uint32_t &wsum)
{
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    for (uint32_t base = 0; base < n; base += 8192) {
        const uint32_t i0 = base + 8u * (uint32_t)t;
        uint32_t v[8];
        if (i0 + 8 <= n && (((uintptr_t)(blk + i0)) & 15) == 0) {
            const uint4 a = *reinterpret_cast<const uint4 *>(blk + i0), b = *reinterpret_cast<const uint4 *>(blk + i0 + 4);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++)
                v[k] = i0 + k < n ? blk[i0 + k] : 0;
        }
        uint32_t sum = 0;
#pragma unroll
        for (int k = 0; k < 8; k++)
            sum += v[k];
        uint32_t inc = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(inc, o, 64);
            inc += lane >= o ? u : 0;
        }
        if (lane == 63)
            wtot[wave] = inc;
        __syncthreads();
        if (wave == 0) {
            uint32_t w = lane < 16 ? wtot[lane] : 0, winc = w;
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                const uint32_t u = __shfl_up(winc, o, 64);
                winc += lane >= o ? u : 0;
            }
            if (lane < 16)
                wtot[lane] = winc - w;                 // exclusive
            if (lane == 15)
                wsum = winc;
        }
        __syncthreads();
        uint32_t run = carry + wtot[wave] + inc - sum;
        carry += wsum;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t x = v[k];
            v[k] = run;
            run += x;
        }
        if (i0 + 8 <= n && (((uintptr_t)(blk + i0)) & 15) == 0) {
            *reinterpret_cast<uint4 *>(blk + i0) = make_uint4(v[0], v[1], v[2], v[3]);
            *reinterpret_cast<uint4 *>(blk + i0 + 4) = make_uint4(v[4], v[5], v[6], v[7]);
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++)
                if (i0 + k < n)
                    blk[i0 + k] = v[k];
        }
        __syncthreads();                   // wtot / wsum are rewritten by the next chunk
    }
    return carry;
}

__global__ __launch_bounds__(1024) void k_extrema_scan(uint32_t *__restrict__ blk, uint32_t n,
                                                       uint32_t *__restrict__ d_count)
{
    __shared__ uint32_t wtot[16];
    __shared__ uint32_t wsum;
    const uint32_t carry = ex_scan_range(blk, n, *d_count, wtot, wsum);
    if (threadIdx.x == 0)
        *d_count = carry;
}

// Scan + emission of ALL octaves of a detect call in two launches (round 5; before: a scan and an emission
// launch per octave, fourteen dependent short launches at 512^3): the octaves' block-count arrays are scanned
// one after the other by the one workgroup (the running total carries over: octave order), and the emission
// grid covers every octave's blocks -- a workgroup finds its octave in a table of first-block numbers.
constexpr int EX_MAX_OCT = SIFT3D_HIP_EXTREMA_MAX_OCT;
struct ExOct {
    const float *g[4];                    // Gaussian levels 1..4: keypoint DoG level i = g[i] - g[i + 1]
    const unsigned long long *masks;      // [3][nwords]
    uint32_t *blk;                        // [3][nblk] block counts -> offsets
    int nx, ny, wpr;
    uint32_t nwords, nblk;
    int tag0;
    uint32_t blk_first;                   // first workgroup (x) of this octave in the emission grid
};
struct ExMulti {
    int n;
    ExOct o[EX_MAX_OCT];
};

__global__ __launch_bounds__(1024) void k_extrema_scan_multi(ExMulti M, uint32_t *__restrict__ d_count)
{
    __shared__ uint32_t wtot[16];
    __shared__ uint32_t wsum;
    uint32_t carry = *d_count;
    for (int i = 0; i < M.n; i++)
        carry = ex_scan_range(M.o[i].blk, M.o[i].nblk * 3u, carry, wtot, wsum);
    if (threadIdx.x == 0)
        *d_count = carry;
}

// FROM_G: `cur` and `next` of a level hold the two Gaussian levels whose difference is the DoG
// level (the DoG pyramid is not stored)
// one emission workgroup: block `bx` of a level (masks / blk_off: that level's own arrays)
template <bool FROM_G>
__device__ __forceinline__ void ex_emit_block(const float *__restrict__ cur, const float *__restrict__ next,
                                              int tag, int nx, int ny, int wpr, uint32_t nwords, uint32_t bx,
                                              const unsigned long long *__restrict__ masks,
                                              const uint32_t *__restrict__ blk_off,
                                              sift3d_hip_cand *__restrict__ out, uint32_t cap)
{
    __shared__ uint32_t pre[EX_WPB + 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t w0 = bx * EX_WPB;
    // pre[i] = candidates in the block's words before word i: the first EX_WPB / 64 waves hold one word per
    // lane, scan their counts by wave shifts and add the totals of the waves before them
    static_assert(EX_WPB % 64 == 0 && EX_WPB <= 256, "one word per thread of the first waves");
    __shared__ uint32_t wtot[EX_WPB / 64];
    {
        const uint32_t word = w0 + threadIdx.x;
        uint32_t inc = threadIdx.x < EX_WPB && word < nwords ? (uint32_t)__popcll(masks[word]) : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = __shfl_up(inc, o, 64);
            inc += lane >= o ? v : 0;
        }
        if (threadIdx.x < EX_WPB) {
            pre[threadIdx.x + 1] = inc;
            if (lane == 63)
                wtot[wave] = inc;
        }
        if (threadIdx.x == 0)
            pre[0] = 0;
        __syncthreads();
        if (threadIdx.x >= 64 && threadIdx.x < EX_WPB) {
            uint32_t add = 0;
            for (int u = 0; u < wave; u++)
                add += wtot[u];
            pre[threadIdx.x + 1] += add;
        }
        __syncthreads();
    }
    if (pre[EX_WPB] == 0)
        return;
    const uint32_t base = blk_off[bx];
    const size_t ys = nx, zs = (size_t)nx * ny;
    // the wave's EX_WPB / 4 (<= 64) mask words: one load, lane i holds word i
    static_assert(EX_WPB / 4 <= 64, "one word per lane");
    unsigned long long mine = 0ull;
    if (lane < EX_WPB / 4 && w0 + wave * (EX_WPB / 4) + lane < nwords)
        mine = masks[w0 + wave * (EX_WPB / 4) + lane];
    // only the words that hold a candidate (a few per cent of them) are visited
    unsigned long long todo = __ballot(mine != 0ull);
    while (todo) {
        const int w = __ffsll((long long)todo) - 1;          // wave-uniform
        todo &= todo - 1ull;
        const int wi = wave * (EX_WPB / 4) + w;
        const uint32_t word = w0 + wi;
        const unsigned long long m =
            ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(mine >> 32), w) << 32) |
            (unsigned)__builtin_amdgcn_readlane((int)mine, w);
        if (!((m >> lane) & 1ull))
            continue;
        const uint32_t pos = base + pre[wi] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (pos >= cap)
            continue;
        const uint32_t row = word / wpr;
        const int x = (int)(word % wpr) * 64 + lane;
        const size_t p = (size_t)x + ys * (row % ny) + zs * (row / ny);
        sift3d_hip_cand c;
        c.idx = (uint32_t)p;
        c.tag = tag;
        c.val = fabsf(FROM_G ? cur[p] - next[p] : cur[p]);     // sift.c:864
        out[pos] = c;
    }
}

template <bool FROM_G>
__global__ __launch_bounds__(256) void k_extrema_emit(ExLevels LV, ExGeom E,
                                                      const unsigned long long *__restrict__ masks,
                                                      const uint32_t *__restrict__ blk_off,
                                                      sift3d_hip_cand *__restrict__ out,
                                                      uint32_t cap)
{
    const int level = blockIdx.y;
    const sift3d_hip_extrema_level L = LV.lv[level];
    ex_emit_block<FROM_G>(L.cur, L.next, L.tag, E.nx, E.ny, E.wpr, E.nwords, blockIdx.x,
                          masks + (size_t)level * E.nwords, blk_off + (size_t)level * E.nblk, out, cap);
}

__global__ __launch_bounds__(256) void k_extrema_emit_multi(ExMulti M, sift3d_hip_cand *__restrict__ out,
                                                            uint32_t cap)
{
    int i = 0;                            // (wave-uniform: blockIdx only)
    while (i + 1 < M.n && blockIdx.x >= M.o[i + 1].blk_first)
        i++;
    const ExOct &O = M.o[i];
    const int level = blockIdx.y;
    ex_emit_block<true>(O.g[level], O.g[level + 1], O.tag0 + level, O.nx, O.ny, O.wpr, O.nwords,
                        blockIdx.x - O.blk_first, O.masks + (size_t)level * O.nwords,
                        O.blk + (size_t)level * O.nblk, out, cap);
}

extern "C" {

int sift3d_hip_subtract_absmax(const float *d_a, const float *d_b, float *d_dst, size_t n,
                               float *d_absmax, void *stream)
{
    if (!n)
        return SIFT3D_SUCCESS;
    hipLaunchKernelGGL(k_sub_absmax, dim3(grid_reduce(n)), dim3(256), 0, (hipStream_t)stream, d_a,
                       d_b, d_dst, n, reinterpret_cast<unsigned *>(d_absmax));
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

int sift3d_hip_dog_stack(const float *const *d_g, float *const *d_d, int n_gauss, size_t n,
                         float *d_absmax, void *stream)
{
    if (n_gauss < 2 || n_gauss > SIFT3D_HIP_MAX_DOG_STACK)
        return 1; // not covered: the caller subtracts level pairs
    if (!n)
        return SIFT3D_SUCCESS;
    DogStack S;
    memset(&S, 0, sizeof(S));
    for (int k = 0; k < n_gauss; k++) {
        S.g[k] = d_g[k];
        if (((uintptr_t)d_g[k] & 15) || (k < n_gauss - 1 && ((uintptr_t)d_d[k] & 15)))
            return 1;
        if (k < n_gauss - 1)
            S.d[k] = d_d[k];
    }
    S.out = reinterpret_cast<unsigned *>(d_absmax);
    dispatch_int_or<2, 7, 8>(n_gauss, [&](auto nl) {
        hipLaunchKernelGGL((k_dog_stack<nl>), dim3(grid_reduce(n)), dim3(256), 0, (hipStream_t)stream, S, n);
    });
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

// The sweeps write EVERY mask word of the planes they test (z_lo <= z < z_hi), zeros included: only the
// words of the planes outside that range (the first and the last plane of a volume, the halo planes of a
// slab) have to be cleared -- not the whole mask (50 MB at 512^3: a 0.28 ms fill per step).
__global__ __launch_bounds__(256) void k_zero_mask_planes(unsigned long long *__restrict__ masks, uint32_t nwords,
                                                          uint32_t wpp, int z_lo, int z_hi, int nz)
{
    const uint32_t nout = (uint32_t)(z_lo + (nz - z_hi)) * wpp;       // words per level outside the range
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < nout; i += gridDim.x * 256) {
        const uint32_t pl = i / wpp, w = i - pl * wpp;
        const uint32_t z = pl < (uint32_t)z_lo ? pl : (uint32_t)z_hi + (pl - (uint32_t)z_lo);
        masks[(size_t)blockIdx.y * nwords + (size_t)z * wpp + w] = 0ull;
    }
}

static ExGeom ex_geom(int nx, int ny, int nz, double peak, int cuboid = 0)
{
    ExGeom E;
    E.cuboid = cuboid;
    E.nx = nx; E.ny = ny; E.nz = nz;
    E.wpr = (nx + 63) / 64;
    E.nwords = (uint32_t)((size_t)nz * ny * E.wpr);
    E.nblk = (E.nwords + EX_WPB - 1) / EX_WPB;
    E.peak_thresh = peak;
    return E;
}

// Before a sweep over the planes z_lo <= z < z_hi: clear the mask words it will not write (all of the three
// levels' masks where it tests no plane at all).
static int clear_unswept_masks(unsigned long long *masks, const ExGeom &E, int z_lo, int z_hi, hipStream_t st)
{
    if (z_hi <= z_lo) {
        HIPCHK(hipMemsetAsync(masks, 0, (size_t)3 * E.nwords * 8, st));
        return SIFT3D_SUCCESS;
    }
    if (z_lo < 0 || z_hi > E.nz)
        return SIFT3D_FAILURE;
    const uint32_t wpp = (uint32_t)E.ny * (uint32_t)E.wpr;
    const long nout = (long)(z_lo + (E.nz - z_hi)) * wpp;
    if (nout > 0) {
        const long nb = (nout + 255) / 256;
        hipLaunchKernelGGL(k_zero_mask_planes, dim3((unsigned)(nb < 512 ? nb : 512), 3), dim3(256), 0, st, masks,
                           E.nwords, wpp, z_lo, z_hi, E.nz);
        LAUNCH_CHECK();
    }
    return SIFT3D_SUCCESS;
}

// Length of the z segments of a sweep over n_out planes with bxy workgroups per segment: about 2048 workgroups
// in all, in segments of 16 planes or more
static int sweep_segments(int n_out, long bxy)
{
    long nseg = (2048 + bxy - 1) / bxy;
    const long cap_seg = n_out / 16 > 1 ? n_out / 16 : 1;
    nseg = nseg < cap_seg ? nseg : cap_seg;
    return (int)((n_out + nseg - 1) / nseg);
}

size_t sift3d_hip_extrema_work_bytes(int nx, int ny, int nz, int nlevels)
{
    const ExGeom E = ex_geom(nx, ny, nz, 0.0);
    return (size_t)nlevels * ((size_t)E.nwords * 8 + (size_t)E.nblk * 4) + 256;
}

int sift3d_hip_extrema(const sift3d_hip_extrema_level *levels, int nlevels, int nx, int ny, int nz,
                       double peak_thresh, sift3d_hip_cand *d_out, uint32_t cap, uint32_t *d_count,
                       void *d_work, size_t work_bytes, void *stream)
{
    return sift3d_hip_extrema_mode(levels, nlevels, nx, ny, nz, peak_thresh, 0, d_out, cap, d_count,
                                   d_work, work_bytes, stream);
}

int sift3d_hip_extrema_mode(const sift3d_hip_extrema_level *levels, int nlevels, int nx, int ny,
                            int nz, double peak_thresh, int cuboid, sift3d_hip_cand *d_out,
                            uint32_t cap, uint32_t *d_count, void *d_work, size_t work_bytes,
                            void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (nlevels < 1 || nlevels > 8 || (size_t)nx * ny * nz >= (1ull << 32) ||
        work_bytes < sift3d_hip_extrema_work_bytes(nx, ny, nz, nlevels))
        return launch_fail("sift3d_hip_extrema", "invalid arguments");
    const ExGeom E = ex_geom(nx, ny, nz, peak_thresh, cuboid ? 1 : 0);
    ExLevels LV;
    memset(&LV, 0, sizeof(LV));
    for (int i = 0; i < nlevels; i++)
        LV.lv[i] = levels[i];
    unsigned long long *masks = reinterpret_cast<unsigned long long *>(d_work);
    uint32_t *blk = reinterpret_cast<uint32_t *>(masks + (size_t)nlevels * E.nwords);
    // default configuration (three keypoint levels sharing their DoG levels, whole quads): one z
    // sweep over the five DoG levels instead of three scattered-neighbour passes
#ifdef SIFT3D_AMD_DIAG
    static const bool no_sweep = getenv("SIFT3D_AMD_NO_EXSWEEP") != nullptr;   // A/B of the sweep kernel
#else
    const bool no_sweep = false;
#endif
    bool sweep = !E.cuboid && !no_sweep && nlevels == 3 && (nx & 3) == 0 && nz >= 3;
    if (sweep) {
        const float *ptrs[5] = { levels[0].prev, levels[0].cur, levels[1].cur, levels[2].cur, levels[2].next };
        sweep = levels[0].next == levels[1].cur && levels[1].prev == levels[0].cur &&
                levels[1].next == levels[2].cur && levels[2].prev == levels[1].cur &&
                levels[0].z_lo == levels[1].z_lo && levels[1].z_lo == levels[2].z_lo &&
                levels[0].z_hi == levels[1].z_hi && levels[1].z_hi == levels[2].z_hi &&
                levels[0].z_lo >= 1 && levels[0].z_hi <= nz - 1;
        for (int i = 0; i < 5; i++)
            sweep = sweep && (((uintptr_t)ptrs[i]) & 15) == 0;
        if (sweep) {
            ExSweep S;
            memset(&S, 0, sizeof(S));
            for (int i = 0; i < 5; i++)
                S.d[i] = ptrs[i];
            for (int i = 0; i < 3; i++)
                S.absmax[i] = levels[i].d_absmax;
            S.peak_thresh = peak_thresh;
            S.nx = nx; S.ny = ny; S.nz = nz;
            S.z_lo = levels[0].z_lo; S.z_hi = levels[0].z_hi;
            S.wpr = E.wpr; S.nwords = E.nwords;
            S.masks32 = reinterpret_cast<uint32_t *>(masks);
            const int n_out = S.z_hi - S.z_lo;
            if (clear_unswept_masks(masks, E, S.z_lo, S.z_hi, st))
                return SIFT3D_FAILURE;
            if (n_out > 0) {
                S.ts = sweep_segments(n_out, (long)((nx + 63) / 64) * ((ny + 15) / 16));
                dim3 grid((nx + 63) / 64, (ny + 15) / 16, (n_out + S.ts - 1) / S.ts);
                hipLaunchKernelGGL(k_extrema_sweep3, grid, dim3(256), 0, st, S);
            }
            hipLaunchKernelGGL(k_extrema_count, dim3(E.nblk, 3), dim3(256), 0, st, masks, E.nwords,
                               E.nblk, blk);
        }
    }
    if (sweep)
        ;
    else if (E.cuboid)
        hipLaunchKernelGGL(k_extrema_mask<true>, dim3(E.nblk, nlevels), dim3(256), 0, st, LV, E, masks,
                           blk);
    else
        hipLaunchKernelGGL(k_extrema_mask<false>, dim3(E.nblk, nlevels), dim3(256), 0, st, LV, E, masks,
                           blk);
    hipLaunchKernelGGL(k_extrema_scan, dim3(1), dim3(1024), 0, st, blk, E.nblk * (uint32_t)nlevels,
                       d_count);
    hipLaunchKernelGGL(k_extrema_emit<false>, dim3(E.nblk, nlevels), dim3(256), 0, st, LV, E, masks, blk,
                       d_out, cap);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

int sift3d_hip_dogmax_stack(const float *const *d_g, int n_gauss, size_t n, float *d_absmax, void *stream)
{
    if (n_gauss < 2 || n_gauss > SIFT3D_HIP_MAX_DOG_STACK)
        return 1; // not covered
    if (!n)
        return SIFT3D_SUCCESS;
    DogStack S;
    memset(&S, 0, sizeof(S));
    for (int k = 0; k < n_gauss; k++) {
        S.g[k] = d_g[k];
        if ((uintptr_t)d_g[k] & 15)
            return 1;
    }
    S.out = reinterpret_cast<unsigned *>(d_absmax);
    dispatch_int_or<2, 7, 8>(n_gauss, [&](auto nl) {
        hipLaunchKernelGGL((k_dogmax_stack<nl>), dim3(grid_reduce(n)), dim3(256), 0, (hipStream_t)stream, S, n);
    });
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

int sift3d_hip_extrema_gauss6(const float *const *d_g, const float *d_absmax, int nx, int ny, int nz,
                              int z_lo, int z_hi, int tag0, double peak_thresh, sift3d_hip_cand *d_out,
                              uint32_t cap, uint32_t *d_count, void *d_work, size_t work_bytes,
                              void *stream)
{
    return sift3d_hip_extrema_gauss6_phase(d_g, d_absmax, nx, ny, nz, z_lo, z_hi, tag0, peak_thresh, d_out,
                                           cap, d_count, d_work, work_bytes, stream, 0);
}

// Lower bounds of an octave's five max|DoG| from a sub-lattice of its six Gaussian levels (one fifteenth of the
// bytes), atomically maxed into d_est[0..4] (zeroed by the caller): what sift3d_hip_extrema_gauss6_est_phase
// thresholds its sweep with.  1: not covered.
int sift3d_hip_dogmax_sub(const float *const *d_g, int nx, int ny, int nz, float *d_est, void *stream)
{
    if ((nx & 3) || nx < 4 || ny < 1 || nz < 1)
        return 1;
    DogStack S;
    memset(&S, 0, sizeof(S));
    for (int k = 0; k < 6; k++) {
        S.g[k] = d_g[k];
        if ((uintptr_t)d_g[k] & 15)
            return 1;
    }
    S.out = reinterpret_cast<unsigned *>(d_est);
    const size_t items = (size_t)(nx / 4) * ((ny + SUB_Y - 1) / SUB_Y) * (nz >= 2 ? (nz - 2) / SUB_Z + 1 : 1);
    hipLaunchKernelGGL((k_dogmax_sub<6>), dim3(grid_reduce(4 * items)), dim3(256), 0, (hipStream_t)stream, S, nx,
                       ny, nz);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

static int extrema_gauss6_impl(const float *const *d_g, const float *d_absmax, const float *d_est,
                               float *d_exact, int nx, int ny, int nz, int z_lo, int z_hi, int tag0,
                               double peak_thresh, sift3d_hip_cand *d_out, uint32_t cap, uint32_t *d_count,
                               void *d_work, size_t work_bytes, void *stream, int phase);

// phase 1: the sweep (masks + per-block counts in d_work; independent of every other octave);
// phase 2: scan + emission, which appends to d_out at *d_count (so: in octave order); 0: both
int sift3d_hip_extrema_gauss6_phase(const float *const *d_g, const float *d_absmax, int nx, int ny, int nz,
                                    int z_lo, int z_hi, int tag0, double peak_thresh,
                                    sift3d_hip_cand *d_out, uint32_t cap, uint32_t *d_count, void *d_work,
                                    size_t work_bytes, void *stream, int phase)
{
    return extrema_gauss6_impl(d_g, d_absmax, nullptr, nullptr, nx, ny, nz, z_lo, z_hi, tag0, peak_thresh, d_out,
                               cap, d_count, d_work, work_bytes, stream, phase);
}

// The same stage WITHOUT a separate pass for the maxima: d_est[0..4] are lower bounds of the octave's
// max|DoG| (sift3d_hip_dogmax_sub), the sweep marks every extremum above peak_thresh * bound and gathers the
// exact maxima into d_exact[0..4] (zeroed by the caller before phase 1; the two planes the sweep has no
// centre on are added by two one-plane launches), and the reference's threshold is then applied to the
// marked voxels.  Whole volumes only (z_lo = 1, z_hi = nz - 1: the maxima are those of the planes swept).
int sift3d_hip_extrema_gauss6_est_phase(const float *const *d_g, const float *d_est, float *d_exact, int nx,
                                        int ny, int nz, int tag0, double peak_thresh, sift3d_hip_cand *d_out,
                                        uint32_t cap, uint32_t *d_count, void *d_work, size_t work_bytes,
                                        void *stream, int phase)
{
    if (!d_est || !d_exact)
        return SIFT3D_FAILURE;
    return extrema_gauss6_impl(d_g, d_exact, d_est, d_exact, nx, ny, nz, 1, nz - 1, tag0, peak_thresh, d_out, cap,
                               d_count, d_work, work_bytes, stream, phase);
}

static int extrema_gauss6_impl(const float *const *d_g, const float *d_absmax, const float *d_est,
                               float *d_exact, int nx, int ny, int nz, int z_lo, int z_hi, int tag0,
                               double peak_thresh, sift3d_hip_cand *d_out, uint32_t cap, uint32_t *d_count,
                               void *d_work, size_t work_bytes, void *stream, int phase)
{
    hipStream_t st = (hipStream_t)stream;
    if ((size_t)nx * ny * nz >= (1ull << 32) || work_bytes < sift3d_hip_extrema_work_bytes(nx, ny, nz, 3))
        return launch_fail("sift3d_hip_extrema_gauss6", "invalid arguments");
    // covered: whole quads, aligned levels, at least one interior plane
    if ((nx & 3) || nz < 3 || z_lo < 1 || z_hi > nz - 1)
        return 1;
    for (int i = 0; i < 6; i++)
        if ((uintptr_t)d_g[i] & 15)
            return 1;
    const ExGeom E = ex_geom(nx, ny, nz, peak_thresh, 0);
    unsigned long long *masks = reinterpret_cast<unsigned long long *>(d_work);
    uint32_t *blk = reinterpret_cast<uint32_t *>(masks + (size_t)3 * E.nwords);
    ExSweep S;
    memset(&S, 0, sizeof(S));
    for (int i = 0; i < 6; i++)
        S.d[i] = d_g[i];
    for (int i = 0; i < 3; i++)
        S.absmax[i] = (d_est ? d_est : d_absmax) + 1 + i;       // DoG levels 1..3 are the keypoint levels
    S.exact = reinterpret_cast<unsigned *>(d_exact);
    S.peak_thresh = peak_thresh;
    S.nx = nx; S.ny = ny; S.nz = nz;
    S.z_lo = z_lo; S.z_hi = z_hi;
    S.wpr = E.wpr; S.nwords = E.nwords;
    S.masks32 = reinterpret_cast<uint32_t *>(masks);
    const int n_out = z_hi - z_lo;
    if (phase != 2 && clear_unswept_masks(masks, E, z_lo, z_hi, st))
        return SIFT3D_FAILURE;
    if (n_out > 0 && phase != 2) {
        // tile width: a whole wave per row where the rows are long enough -- 1 KB row segments
        // (measured at 512^3, the sweep alone: 0.58 ms against 0.66 / 0.80 with 512 / 256-byte segments,
        // although the 4-row tiles re-read more halo rows)
        const int txq = nx >= 256 ? 64 : nx >= 128 ? 32 : 16, tyy = 256 / txq;
        S.ts = sweep_segments(n_out, (long)((nx + 4 * txq - 1) / (4 * txq)) * ((ny + tyy - 1) / tyy));
        dim3 grid((nx + 4 * txq - 1) / (4 * txq), (ny + tyy - 1) / tyy, (n_out + S.ts - 1) / S.ts);
        if (d_est) {
            if (txq == 32)
                hipLaunchKernelGGL((k_extrema_sweep3g<32, true>), grid, dim3(256), 0, st, S);
            else if (txq == 64)
                hipLaunchKernelGGL((k_extrema_sweep3g<64, true>), grid, dim3(256), 0, st, S);
            else
                hipLaunchKernelGGL((k_extrema_sweep3g<16, true>), grid, dim3(256), 0, st, S);
        } else if (txq == 32)
            hipLaunchKernelGGL((k_extrema_sweep3g<32>), grid, dim3(256), 0, st, S);
        else if (txq == 64)
            hipLaunchKernelGGL((k_extrema_sweep3g<64>), grid, dim3(256), 0, st, S);
        else
            hipLaunchKernelGGL((k_extrema_sweep3g<16>), grid, dim3(256), 0, st, S);
    }
    if (d_est && phase != 2) {
        // the first and the last plane, then the reference's threshold on the marked voxels
        const size_t plane = (size_t)nx * ny;
        const float *g0[6], *g1[6];
        for (int i = 0; i < 6; i++) {
            g0[i] = d_g[i];
            g1[i] = d_g[i] + (size_t)(nz - 1) * plane;
        }
        if (sift3d_hip_dogmax_stack(g0, 6, plane, d_exact, stream) != SIFT3D_SUCCESS ||
            sift3d_hip_dogmax_stack(g1, 6, plane, d_exact, stream) != SIFT3D_SUCCESS)
            return SIFT3D_FAILURE;
        hipLaunchKernelGGL(k_extrema_refilter, dim3((unsigned)(((size_t)3 * E.nwords + 255) / 256)), dim3(256), 0,
                           st, S);
    }
    if (phase != 2)
        hipLaunchKernelGGL(k_extrema_count, dim3(E.nblk, 3), dim3(256), 0, st, masks, E.nwords, E.nblk, blk);
    if (phase == 1) {
        LAUNCH_CHECK();
        return SIFT3D_SUCCESS;
    }
    hipLaunchKernelGGL(k_extrema_scan, dim3(1), dim3(1024), 0, st, blk, E.nblk * 3u, d_count);
    ExLevels LV;
    memset(&LV, 0, sizeof(LV));
    for (int i = 0; i < 3; i++) {
        LV.lv[i].cur = d_g[i + 1];            // DoG level i + 1 = G[i + 1] - G[i + 2]
        LV.lv[i].next = d_g[i + 2];
        LV.lv[i].tag = tag0 + i;
    }
    hipLaunchKernelGGL(k_extrema_emit<true>, dim3(E.nblk, 3), dim3(256), 0, st, LV, E, masks, blk, d_out,
                       cap);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

// Phase 2 of sift3d_hip_extrema_gauss6_[est_]phase for ALL octaves of a call at once: one scan launch over the
// octaves' block counts in order, one emission launch over every octave's blocks; appends at *d_count in
// (octave, level, z, y, x) order -- the reference's (sift.c:835-868).  1: more octaves than one launch takes
// (the caller then issues phase 2 per octave).
int sift3d_hip_extrema_gauss6_finish(const sift3d_hip_extrema_oct *octs, int n_oct, double peak_thresh,
                                     sift3d_hip_cand *d_out, uint32_t cap, uint32_t *d_count, void *stream)
{
    if (n_oct < 1 || n_oct > EX_MAX_OCT)
        return 1;
    ExMulti M;
    memset(&M, 0, sizeof(M));
    M.n = n_oct;
    uint32_t nb = 0;
    for (int i = 0; i < n_oct; i++) {
        const sift3d_hip_extrema_oct &q = octs[i];
        if ((size_t)q.nx * q.ny * q.nz >= (1ull << 32) ||
            q.work_bytes < sift3d_hip_extrema_work_bytes(q.nx, q.ny, q.nz, 3))
            return launch_fail("sift3d_hip_extrema_gauss6_finish", "invalid arguments");
        const ExGeom E = ex_geom(q.nx, q.ny, q.nz, peak_thresh, 0);
        ExOct &O = M.o[i];
        for (int k = 0; k < 4; k++)
            O.g[k] = q.d_g[k + 1];
        unsigned long long *masks = reinterpret_cast<unsigned long long *>(q.d_work);
        O.masks = masks;
        O.blk = reinterpret_cast<uint32_t *>(masks + (size_t)3 * E.nwords);
        O.nx = q.nx; O.ny = q.ny; O.wpr = E.wpr;
        O.nwords = E.nwords; O.nblk = E.nblk;
        O.tag0 = q.tag0;
        O.blk_first = nb;
        nb += E.nblk;
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_extrema_scan_multi, dim3(1), dim3(1024), 0, st, M, d_count);
    hipLaunchKernelGGL(k_extrema_emit_multi, dim3(nb, 3), dim3(256), 0, st, M, d_out, cap);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

} // extern "C"
