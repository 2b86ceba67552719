// sift3d_kernels.hip -- hand-written gfx950 (CDNA4, MI355X) kernels of the pyramid stage of the SIFT3D
// detect path and their C-ABI launchers (include/sift3d_amd.h): input scaling, the 1-D Gaussian passes and
// the 2x downsampling; plus the synthetic-volume kernel and two test kernels.  The stages after it have units
// of their own (sift3d_extrema.hip, sift3d_orient.hip, sift3d_describe.hip), the HIP runtime wrappers are in
// sift3d_device.hip.
//
// All stages are memory-bound stencils or per-keypoint window reductions: no MFMA.
// Design rules that matter here (cdna_hip_programming.md / MI355X_MICROARCH.md):
//   * wave = 64 lanes; coalesced 16 B/lane accesses along the unit-stride x axis
//   * the three 1-D Gaussian passes never transpose the volume in HBM: the x pass stages
//     row segments in LDS and slides a register window, the y/z passes sweep along the
//     strided axis with a register ring so every input is loaded once per thread
//   * bit-exact float32 results vs the reference CPU path: tap order d = -hw..+hw,
//     `tap * ((1-frac)*lo + frac*hi)` then `+=`, NO fused multiply-add (every unit is
//     compiled with -ffp-contract=off and carries the pragma of sift3d_kernels_common.h)
//   * window reductions (orientation tensor, descriptor histogram) accumulate in the
//     reference's voxel scan order, so sums are bit-identical, not just close
//
// Reference citations are file:line under /root/reference/sift3d/.
#include "sift3d_kernels_common.h"
#include "sift3d_math.h"
#include "synth.h"

// ---------------------------------------------------------------------------------------
// im_max_abs / im_scale  (imutil.c:681-713)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_absmax(const float *__restrict__ src, size_t n,
                                                unsigned *__restrict__ out)
{
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nthr = (size_t)gridDim.x * blockDim.x;
    const size_t n4 = n >> 2;
    float m = 0.0f;
    // four independent 16-byte loads in flight per thread and iteration
    size_t i = tid;
    for (; i + 3 * nthr < n4; i += 4 * nthr) {
        float4 v[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
            v[k] = ld4(src + 4 * (i + k * nthr));
#pragma unroll
        for (int k = 0; k < 4; k++)
            m = fmaxf(m, fmaxf(fmaxf(fabsf(v[k].x), fabsf(v[k].y)), fmaxf(fabsf(v[k].z), fabsf(v[k].w))));
    }
    for (; i < n4; i += nthr) {
        const float4 v = ld4(src + 4 * i);
        m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
    for (size_t j = 4 * n4 + tid; j < n; j += nthr)
        m = fmaxf(m, fabsf(src[j]));
    block_max_atomic<1>(&m, out);
}

__global__ __launch_bounds__(256) void k_scale(const float *__restrict__ src,
                                               float *__restrict__ dst, size_t n,
                                               const float *__restrict__ d_max)
{
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nthr = (size_t)gridDim.x * blockDim.x;
    const size_t n4 = n >> 2;
    const float mx = *d_max;
    if (mx == 0.0f) { // imutil.c:706-707
        for (size_t i = tid; i < n4; i += nthr)
            st4(dst + 4 * i, ld4(src + 4 * i));
        for (size_t i = 4 * n4 + tid; i < n; i += nthr)
            dst[i] = src[i];
        return;
    }
    for (size_t i = tid; i < n4; i += nthr) {
        float4 v = ld4(src + 4 * i);
        v.x = v.x / mx; // imutil.c:711, IEEE division
        v.y = v.y / mx;
        v.z = v.z / mx;
        v.w = v.w / mx;
        st4(dst + 4 * i, v);
    }
    for (size_t i = 4 * n4 + tid; i < n; i += nthr)
        dst[i] = src[i] / mx;
}

// ---------------------------------------------------------------------------------------
// 1-D interpolating FIR  (convolve_sep_gen, imutil.c:742-861)
// ---------------------------------------------------------------------------------------
// One output sample, the literal arithmetic of the reference.  `line` points at the
// LOCAL index 0 of the 1-D line; g is the GLOBAL coordinate of the output.  Samples are
// clamped into the local buffer for memory safety only (a correct call never needs it,
// except for the weight-0 `hi` read one past the row -- SURVEY.md A.2).
template <int HWT>
__device__ __forceinline__ float fir_literal_t(const float *__restrict__ line, size_t stride,
                                               int g, int n_glob, int off, int n_loc,
                                               const float *__restrict__ taps, int hw_rt,
                                               float uf, int uhw)
{
    // HWT > 0: compile-time half width -> the tap loop is fully unrolled and its 2*(2*HWT+1)
    // loads are issued back to back (a rolled loop serialises one memory latency per tap)
    const int hw = HWT > 0 ? HWT : hw_rt;
    const int dim_end = n_glob - 1;                               // :753
    const bool interior = g >= uhw && g <= n_glob - 2 - uhw;      // :762-763, :829
    float acc = 0.0f;                                             // im_zero, :777
    float coord = (float)g;
#pragma unroll
    for (int d = -hw; d <= hw; d++) {
        const float tap = taps[d + hw];
        const float step = (float)d * uf;                         // :808 / :837
        float c;
        if (interior) {
            coord -= step;                                        // :811
            c = coord;
        } else {
            c = (float)g - step;                                  // :835,:840
            if ((int)c < 0)                                       // :843
                c = -c;
            else if ((int)c >= dim_end)                           // :846
                c = 2.0f * (float)dim_end - c - 0.1f;             // :847-848
        }
        const int lo = (int)c;                                    // trunc, :783
        const float frac = c - (float)lo;                         // :788
        const int llo = clampi(lo - off, 0, n_loc - 1);
        const int lhi = clampi(lo + 1 - off, 0, n_loc - 1);
        const float a = line[(size_t)llo * stride];
        const float b = line[(size_t)lhi * stride];
        acc += tap * ((1.0f - frac) * a + frac * b);              // :791-795
        if (interior)
            coord += step;                                        // :817
    }
    return acc;
}

__device__ __forceinline__ float fir_literal(const float *__restrict__ line, size_t stride,
                                             int g, int n_glob, int off, int n_loc,
                                             const float *__restrict__ taps, int hw,
                                             float uf, int uhw)
{
    return fir_literal_t<0>(line, stride, g, n_glob, off, n_loc, taps, hw, uf, uhw);
}

// literal kernel: one thread per output voxel, any axis, any unit factor
__global__ __launch_bounds__(256) void k_fir_literal(FirParams P, FirTaps T)
{
    const size_t plane = (size_t)P.nx * P.ny;
    const size_t total = plane * (size_t)(P.z_hi - P.z_lo);
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total)
        return;
    const int z = P.z_lo + (int)(i / plane);
    const size_t r = i % plane;
    const int y = (int)(r / P.nx);
    const int x = (int)(r % P.nx);
    const size_t idx = (size_t)z * plane + r;
    // per-axis geometry by selects (no control flow): coordinate along the axis, stride,
    // local extent; n_glob / off were resolved by the launcher
    const int p = P.axis == 0 ? x : (P.axis == 1 ? y : z);
    const size_t stride = P.axis == 0 ? (size_t)1 : (P.axis == 1 ? (size_t)P.nx : plane);
    const int n_loc = P.axis == 0 ? P.nx : (P.axis == 1 ? P.ny : P.nz);
    const float *line = P.src + (idx - (size_t)p * stride);
    P.dst[idx] = fir_literal(line, stride, p + P.off, P.n_glob, P.off, n_loc, T.k, P.hw, P.uf,
                             P.uhw);
}

// Filters WIDER than the kernarg tap table (SIFT3D_HIP_MAX_TAPS; the reference accepts any sigma0 >= 0,
// sift.c:553-565 -- half width ceil(3 sigma), imutil.c:1275-1277): the literal kernel in chunks of taps.  A
// launch adds taps d in [d_lo, d_hi) to the running sum of every output voxel, which travels between the
// launches in dst (first chunk: 0); the reference adds the taps of a voxel in ascending d into one float
// accumulator (imutil.c:791-795), so the chunks reproduce its sum bit for bit.  The interior branch's
// coordinate round trip (imutil.c:811-817: coord -= step ... coord += step, a state carried from tap to tap)
// is replayed from d = -hw in every launch -- arithmetic only -- so that its state at a chunk's first tap is
// the reference's.
__global__ __launch_bounds__(256) void k_fir_literal_chunk(FirParams P, FirTaps T, int d_lo, int d_hi)
{
    const size_t plane = (size_t)P.nx * P.ny;
    const size_t total = plane * (size_t)(P.z_hi - P.z_lo);
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total)
        return;
    const int z = P.z_lo + (int)(i / plane);
    const size_t r = i % plane;
    const int y = (int)(r / P.nx);
    const int x = (int)(r % P.nx);
    const size_t idx = (size_t)z * plane + r;
    const int p = P.axis == 0 ? x : (P.axis == 1 ? y : z);
    const size_t stride = P.axis == 0 ? (size_t)1 : (P.axis == 1 ? (size_t)P.nx : plane);
    const int n_loc = P.axis == 0 ? P.nx : (P.axis == 1 ? P.ny : P.nz);
    const float *__restrict__ line = P.src + (idx - (size_t)p * stride);
    const int g = p + P.off, hw = P.hw;
    const int dim_end = P.n_glob - 1;                             // :753
    const bool interior = g >= P.uhw && g <= P.n_glob - 2 - P.uhw;  // :762-763, :829
    float acc = d_lo > -hw ? P.dst[idx] : 0.0f;                   // im_zero, :777
    float coord = (float)g;
    for (int d = -hw; d < d_hi; d++) {
        const float step = (float)d * P.uf;                       // :808 / :837
        float c;
        if (interior) {
            coord -= step;                                        // :811
            c = coord;
        } else {
            c = (float)g - step;                                  // :835,:840
            if ((int)c < 0)                                       // :843
                c = -c;
            else if ((int)c >= dim_end)                           // :846
                c = 2.0f * (float)dim_end - c - 0.1f;             // :847-848
        }
        if (d >= d_lo) {
            const int lo = (int)c;                                // trunc, :783
            const float frac = c - (float)lo;                     // :788
            const int llo = clampi(lo - P.off, 0, n_loc - 1);
            const int lhi = clampi(lo + 1 - P.off, 0, n_loc - 1);
            const float a = line[(size_t)llo * stride];
            const float b = line[(size_t)lhi * stride];
            acc += T.k[d - d_lo] * ((1.0f - frac) * a + frac * b);    // :791-795
        }
        if (interior)
            coord += step;                                        // :817
    }
    P.dst[idx] = acc;
}

// ---- unit factor 1 (octave 0): edges as a staging transformation ----------------------------
// With uf == 1 every sample coordinate is an integer, and the reference's edge rules
// (imutil.c:842-850) depend only on that integer i = x - d, not on (x, d) separately:
//     i < 0          -> sample src[-i]                       (frac == 0)
//     0 <= i < end   -> sample src[i]                        (frac == 0)
//     i >= end = n-1 -> c' = 2*end - i - 0.1f, a fixed lerp of two samples near the end
//                       (including i == end itself, quirk Q4)
// and interior outputs never reach i >= end.  So the whole pass is  out[x] = sum_d k[d]*E[x-d]
// over an EXTENDED line E with reflected samples on the low side and pre-interpolated
// "virtual" samples v_m = w0_m*src[lo_m] + w1_m*src[lo_m+1] (m = i - end) on the high side.
// tap*((1-frac)*lo + frac*hi) is evaluated exactly as written -- the inner expression is
// v_m -- and for frac == 0 it equals tap*lo for finite data.  Requires n >= 2*hw + 2 (no
// double mirroring); shorter axes take the literal kernel.  The (lo_m, w0_m, w1_m) table is
// computed on the host with the reference's float expressions.
// E[i] for one line; i and the table are GLOBAL coordinates, the line pointer addresses local
// index 0 and holds global indices [off, off + n_loc).
__device__ __forceinline__ float ext_sample(const float *__restrict__ line, size_t stride, int i,
                                            int end, int off, int n_loc, int hw,
                                            const EdgeTab &E)
{
    if (i < 0) {
        return -i <= hw ? line[(size_t)clampi(-i - off, 0, n_loc - 1) * stride] : 0.0f;
    } else if (i >= end) {
        const int m = i - end;
        if (m > hw)
            return 0.0f;
        const int lo = E.lo[m];
        const float a = line[(size_t)clampi(lo - off, 0, n_loc - 1) * stride];
        const float b = line[(size_t)clampi(lo + 1 - off, 0, n_loc - 1) * stride];
        return E.w0[m] * a + E.w1[m] * b;
    }
    return line[(size_t)clampi(i - off, 0, n_loc - 1) * stride];
}

// x pass: each wave walks XROWS consecutive rows of one 512-output segment, software
// pipelined: the 16-byte global loads of row r+1 are in flight while row r is computed from
// LDS (double-buffered, wave-private, so no workgroup barrier).  The extended segment
// (+8-float halos) is staged with coalesced loads; each lane pulls two 20-float windows into
// registers (lane stride 16 B: conflict-free ds_read_b128) and emits 2 x 4 outputs with fully
// coalesced 16-byte stores, in the reference's tap order.  No edge code in the FIR itself.
constexpr int XROWS = 4;

template <int HW>
__global__ __launch_bounds__(256) void k_fir_x_u1(FirParams P, FirTaps T, EdgeTab E)
{
    constexpr int SEG = 512, HALO = 8, L = SEG + 2 * HALO, NV = (L / 4 + 63) / 64; // NV = 3
    static_assert(HW <= HALO, "halo too small");
    __shared__ __attribute__((aligned(16))) float lds[4][2][L];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nrows = P.ny * (P.z_hi - P.z_lo);
    // Blocks walk the volume from its LAST rows to its first: the producer of `src` (the
    // previous blur's z sweep) finished there, so those planes are still in the 256 MB
    // Infinity Cache; the consumer of `dst` starts at plane 0, where this kernel ends.
    const int row0 = ((gridDim.y - 1 - blockIdx.y) * 4 + wave) * XROWS;
    if (row0 >= nrows)
        return;
    const int nr = min(XROWS, nrows - row0);
    const int x0 = blockIdx.x * SEG;
    const int nx = P.nx, end = nx - 1;
    const bool vec_ok = (nx & 3) == 0 && ((((uintptr_t)P.src | (uintptr_t)P.dst) & 15) == 0);
    // rows of the plane range are contiguous in memory: row r starts at base + r*nx
    const size_t base = (size_t)P.z_lo * P.ny * nx;
    const int egi = lane < 8 ? -1 - lane : end + (lane - 8);   // edge sample this lane provides
    const int epos = egi - (x0 - HALO);
    const bool has_edge = lane < 17 && epos >= 0 && epos < L;

    // im_scale folded in (P.scale_max): the quotient v / max of imutil.c:711 is formed when a row is committed
    // to LDS -- not when it is requested: nothing may depend on a load in flight -- and the edge samples
    // are built from scaled samples, as the reference builds them from the scaled image
    const float smax = P.scale_max ? *P.scale_max : 0.0f;
    const bool scaled = smax != 0.0f;                          // (max == 0: im_scale leaves the image alone)
    float4 v[NV];
    float ve = 0.0f, ve2 = 0.0f, ew0 = 1.0f, ew1 = 0.0f;
    auto fetch = [&](int r) {
        const float *__restrict__ s = P.src + base + (size_t)(row0 + r) * nx;
#pragma unroll
        for (int k = 0; k < NV; k++) {
            const int i = lane + 64 * k;
            const int gx = x0 - HALO + 4 * i;
            if (i < L / 4) {
                if (vec_ok && gx >= 0 && gx + 3 < nx) {
                    v[k] = ld4(s + gx);
                } else {
                    v[k].x = (gx >= 0 && gx < nx) ? s[gx] : 0.0f;
                    v[k].y = (gx + 1 >= 0 && gx + 1 < nx) ? s[gx + 1] : 0.0f;
                    v[k].z = (gx + 2 >= 0 && gx + 2 < nx) ? s[gx + 2] : 0.0f;
                    v[k].w = (gx + 3 >= 0 && gx + 3 < nx) ? s[gx + 3] : 0.0f;
                }
            }
        }
        // edge samples of the extended line, one per lane: E[-1..-8] and E[end..end+8] (the two samples and
        // weights of ext_sample's cases; combined in commit)
        if (has_edge) {
            ve = ve2 = 0.0f;
            ew0 = 1.0f;
            ew1 = 0.0f;
            if (egi < 0) {
                if (-egi <= HW)
                    ve = s[clampi(-egi, 0, nx - 1)];
            } else if (egi - end <= HW) {
                const int m = egi - end, lo = E.lo[m];
                ve = s[clampi(lo, 0, nx - 1)];
                ve2 = s[clampi(lo + 1, 0, nx - 1)];
                ew0 = E.w0[m];
                ew1 = E.w1[m];
            }
        }
    };
    auto commit = [&](int buf) {
#pragma unroll
        for (int k = 0; k < NV; k++) {
            const int i = lane + 64 * k;
            if (i < L / 4) {
                float4 q = v[k];
                if (scaled) {
                    q.x = q.x / smax; q.y = q.y / smax; q.z = q.z / smax; q.w = q.w / smax;   // imutil.c:711
                }
                *reinterpret_cast<float4 *>(&lds[wave][buf][4 * i]) = q;
            }
        }
        // DS writes of a wave retire in order: the edge samples overwrite the bulk values
        if (has_edge) {
            const float a = scaled ? ve / smax : ve, b = scaled ? ve2 / smax : ve2;
            // (ext_sample's cases: a lone sample is 1 * a + 0 * b = a exactly; beyond the taps' reach 0)
            lds[wave][buf][epos] = egi >= end ? ew0 * a + ew1 * b : a;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
    };

    fetch(0);
    commit(0);
    for (int r = 0; r < nr; r++) {
        const int buf = r & 1;
        if (r + 1 < nr)
            fetch(r + 1);                     // in flight during the FIR below
        float *__restrict__ d = P.dst + base + (size_t)(row0 + r) * nx;
#pragma unroll
        for (int grp = 0; grp < 2; grp++) {
            const int lb = grp * 256 + lane * 4;   // first output of this lane in the segment
            const int xb = x0 + lb;
            if (xb < nx) {
                float w[4 + 2 * HALO];
#pragma unroll
                for (int i = 0; i < (4 + 2 * HALO) / 4; i++) {
                    const float4 q = *reinterpret_cast<const float4 *>(&lds[wave][buf][lb + 4 * i]);
                    w[4 * i] = q.x; w[4 * i + 1] = q.y; w[4 * i + 2] = q.z; w[4 * i + 3] = q.w;
                }
                float o[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    float acc = 0.0f;
#pragma unroll
                    for (int dd = -HW; dd <= HW; dd++)
                        acc += T.k[dd + HW] * w[HALO + k - dd];   // E[x - d], d ascending
                    o[k] = acc;
                }
                if (vec_ok && xb + 4 <= nx) {
                    st4(d + xb, make_float4(o[0], o[1], o[2], o[3]));
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (xb + k < nx)
                            d[xb + k] = o[k];
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        if (r + 1 < nr)
            commit(buf ^ 1);
    }
}

// The same pass for rows of whole 512-float segments (nx % 512 == 0, 16-byte aligned: every volume of the
// BASELINE configurations), with TWO rows in flight per wave.  k_fir_x_u1 above is bound by latency x
// occupancy, not by bytes (measured: 0.228-0.236 ms at 6 waves per SIMD, 0.275-0.280 ms at 5, for the same
// 8 B/voxel; one row = 2 KB in flight per wave): here the loads of rows r + 1 AND r + 2 fly while row r is
// filtered.  All vector-memory instructions of the loop body are issued unconditionally (clamped addresses,
// values masked when they are committed to LDS; the tail re-requests the last row), so the body is
// straight-line code and the compiler's s_waitcnt vmcnt counts are exact -- a load or store behind a
// lane- or wave-dependent branch would make it wait for the younger row as well.
constexpr int XROWS_F = 8;

template <int HW, bool SCALED>
__global__ __launch_bounds__(256) void k_fir_x_u1f(FirParams P, FirTaps T, EdgeTab E)
{
    constexpr int SEG = 512, HALO = 8, L = SEG + 2 * HALO;
    static_assert(HW <= HALO, "halo too small");
    __shared__ __attribute__((aligned(16))) float lds[4][2][L];
    // where the lanes that have no third quad / no edge sample to commit put theirs: every commit is then
    // free of branches, and no load is left "maybe consumed" at the loop's back edge
    __shared__ __attribute__((aligned(16))) float lds_sink[4][64 * 4];
    // (wave-uniform by construction; said so, or the row loop's exits become lane-divergent control flow)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int nrows = P.ny * (P.z_hi - P.z_lo);
    // (back to front, as k_fir_x_u1: the producer of `src` ended at the last planes)
    const int row0 = ((gridDim.y - 1 - blockIdx.y) * 4 + wave) * XROWS_F;
    if (row0 >= nrows)
        return;
    const int nr = min(XROWS_F, nrows - row0);
    const int x0 = blockIdx.x * SEG;
    const int nx = P.nx, end = nx - 1;
    const size_t base = (size_t)P.z_lo * P.ny * nx;
    // quads of the extended segment this lane stages: i = lane, lane + 64, lane + 128 (< L / 4 = 132)
    const int g0 = x0 - HALO + 4 * lane, g1 = g0 + 256, g2 = g0 + 512;
    const bool in0 = g0 >= 0, use2 = lane < 4, in2 = use2 && g2 + 3 < nx;
    const int c0 = in0 ? g0 : 0, c2 = in2 ? g2 : nx - 4;
    // edge samples of the extended line, one per lane (ext_sample's cases)
    const int egi = lane < 8 ? -1 - lane : end + (lane - 8);
    const int epos = egi - (x0 - HALO);
    const bool has_edge = lane < 17 && epos >= 0 && epos < L;
    int eo0 = 0, eo1 = 0;
    float ew0 = 0.0f, ew1 = 0.0f;                 // (beyond the taps' reach: 0)
    if (lane < 17) {
        if (egi < 0) {
            if (-egi <= HW) {
                eo0 = clampi(-egi, 0, nx - 1);
                ew0 = 1.0f;
            }
        } else if (egi - end <= HW) {
            // (selects, not E.lo[m]: a lane-dependent index into a kernel argument would go through scratch)
            const int m = egi - end;
            int lo = 0;
#pragma unroll
            for (int mm = 0; mm <= HW; mm++)
                if (mm == m) {
                    lo = E.lo[mm];
                    ew0 = E.w0[mm];
                    ew1 = E.w1[mm];
                }
            eo0 = clampi(lo, 0, nx - 1);
            eo1 = clampi(lo + 1, 0, nx - 1);
        }
    }
    // SCALED: im_scale folded in (imutil.c:698-713); a maximum of 0 leaves the image alone (imutil.c:706-707):
    // every sample is then 0 and 0 / 1 = 0 exactly
    float smax = 1.0f;
    if (SCALED) {
        smax = *P.scale_max;
        smax = smax != 0.0f ? smax : 1.0f;
    }

    struct RowRegs {
        float4 v0, v1, v2;
        float e0, e1;
    };
    auto fetch = [&](RowRegs &R, int r) {
        const float *__restrict__ s = P.src + base + (size_t)(row0 + min(r, nr - 1)) * nx;
        R.v0 = ld4(s + c0);
        R.v1 = ld4(s + g1);
        R.v2 = ld4(s + c2);
        R.e0 = s[eo0];
        R.e1 = s[eo1];
    };
    auto commit = [&](const RowRegs &R, int buf) {
        float4 q0 = R.v0, q1 = R.v1, q2 = R.v2;
        float a = R.e0, b = R.e1;
        if (SCALED) {                                           // imutil.c:711, formed when committed
            q0.x = q0.x / smax; q0.y = q0.y / smax; q0.z = q0.z / smax; q0.w = q0.w / smax;
            q1.x = q1.x / smax; q1.y = q1.y / smax; q1.z = q1.z / smax; q1.w = q1.w / smax;
            q2.x = q2.x / smax; q2.y = q2.y / smax; q2.z = q2.z / smax; q2.w = q2.w / smax;
            a = a / smax;
            b = b / smax;
        }
        // (component selects: a select between two float4 objects would go through scratch)
        q0.x = in0 ? q0.x : 0.0f; q0.y = in0 ? q0.y : 0.0f; q0.z = in0 ? q0.z : 0.0f; q0.w = in0 ? q0.w : 0.0f;
        q2.x = in2 ? q2.x : 0.0f; q2.y = in2 ? q2.y : 0.0f; q2.z = in2 ? q2.z : 0.0f; q2.w = in2 ? q2.w : 0.0f;
        float *const row = lds[wave][buf], *const sink = &lds_sink[wave][4 * lane];
        *reinterpret_cast<float4 *>(row + 4 * lane) = q0;
        *reinterpret_cast<float4 *>(row + 4 * (lane + 64)) = q1;
        *reinterpret_cast<float4 *>(use2 ? row + 4 * (lane + 128) : sink) = q2;
        // DS writes of a wave retire in order: the edge samples overwrite the bulk values
        // (ext_sample's three cases in one expression, so that nothing here branches: a lone sample has
        // weights (1, 0): 1 * a + 0 * b = a for finite data -- up to the sign of a zero, which no later
        // comparison or non-zero sum can see --, a sample beyond the taps' reach (0, 0))
        *(has_edge ? row + epos : sink) = ew0 * a + ew1 * b;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
    };
    auto compute = [&](int r, int buf) {
        float *__restrict__ d = P.dst + base + (size_t)(row0 + r) * nx;
#pragma unroll
        for (int grp = 0; grp < 2; grp++) {
            const int lb = grp * 256 + lane * 4;   // first output of this lane in the segment
            float w[4 + 2 * HALO];
#pragma unroll
            for (int i = 0; i < (4 + 2 * HALO) / 4; i++) {
                const float4 q = *reinterpret_cast<const float4 *>(&lds[wave][buf][lb + 4 * i]);
                w[4 * i] = q.x; w[4 * i + 1] = q.y; w[4 * i + 2] = q.z; w[4 * i + 3] = q.w;
            }
            float o[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                float acc = 0.0f;
#pragma unroll
                for (int dd = -HW; dd <= HW; dd++)
                    acc += T.k[dd + HW] * w[HALO + k - dd];   // E[x - d], d ascending
                o[k] = acc;
            }
            st4(d + x0 + lb, make_float4(o[0], o[1], o[2], o[3]));
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        __builtin_amdgcn_wave_barrier();
    };

    // The rows of this wave.  Called with the constant XROWS_F (all but the volume's last rows) the loop is
    // unrolled completely: one basic block, in which the compiler's vmcnt counts are exact (at a loop header
    // it merges the states of the entry and the back edge and waits for the younger row too).
    auto rows = [&](const int n) __attribute__((always_inline)) {
        RowRegs A, B;
        fetch(A, 0);
        fetch(B, 1);
        commit(A, 0);
#pragma unroll
        for (int r = 0; r < XROWS_F; r += 2) {
            fetch(A, r + 2);                  // rows r + 1 (B) and r + 2 (A) in flight during the FIR below
            compute(r, 0);
            if (r + 1 >= n)
                break;
            commit(B, 1);
            fetch(B, r + 3);
            compute(r + 1, 1);
            if (r + 2 >= n)
                break;
            commit(A, 0);
        }
    };
    if (nr == XROWS_F)
        rows(XROWS_F);
    else
        rows(nr);
}

// ---- y / z pass, unit factor 1 ----------------------------------------------------------
// Each thread owns V adjacent x (one 16-byte quad for V=4) and sweeps `ts` outputs along
// the strided axis, keeping the 2*HW+1 most recent rows of the EXTENDED line in a register
// ring: every input is loaded once per thread, loads are coalesced along x, nothing is
// transposed.  Whether a ring row is plain, reflected or virtual depends only on the sweep
// coordinate, which is wave-uniform, so the edge rows cost no divergence.
struct SweepGeom {
    int ncols;          // number of V-wide columns
    int cols_inner;     // columns per contiguous run (row for the y pass, plane for z)
    size_t outer_stride;// floats between runs (plane for the y pass)
    int outer_lo;       // first run (z_lo for the y pass)
    size_t stride;      // floats between consecutive samples along the sweep axis
    int n_loc;          // local extent of the sweep axis
    int out_lo, out_hi; // local output range along the sweep axis
};

// row r (LOCAL index, may be outside [0, n_loc)) of the extended line
template <int V>
__device__ __forceinline__ typename Vec<V>::T ext_row(const float *__restrict__ s, size_t stride,
                                                      int r, int off, int end, int nl1, int hw,
                                                      const EdgeTab &E)
{
    const int i = r + off; // global, wave-uniform
    if (i < 0) {
        return Vec<V>::ld(s + (size_t)clampi(-i - off, 0, nl1) * stride);
    } else if (i >= end) {
        const int m = i - end;
        if (m > hw)
            return Vec<V>::zero();
        const int lo = E.lo[m] - off;
        return Vec<V>::lerp(E.w0[m], Vec<V>::ld(s + (size_t)clampi(lo, 0, nl1) * stride), E.w1[m],
                            Vec<V>::ld(s + (size_t)clampi(lo + 1, 0, nl1) * stride));
    }
    return Vec<V>::ld(s + (size_t)clampi(r, 0, nl1) * stride);
}

template <int HW, int V>
__global__ __launch_bounds__(256) void k_fir_sweep_u1(FirParams P, SweepGeom G, FirTaps T, EdgeTab E)
{
    typedef typename Vec<V>::T vec;
    constexpr int W = 2 * HW + 1;
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= G.ncols)
        return;
    const int p0 = G.out_lo + blockIdx.y * P.ts;
    const int p1 = min(p0 + P.ts, G.out_hi);
    const size_t base = (size_t)(G.outer_lo + col / G.cols_inner) * G.outer_stride +
                        (size_t)(col % G.cols_inner) * V;
    const float *__restrict__ s = P.src + base;
    float *__restrict__ d = P.dst + base;
    const int nl1 = G.n_loc - 1;
    const int off = P.off, end = P.n_glob - 1;

    vec ring[W];
#pragma unroll
    for (int i = 0; i < 2 * HW; i++)
        ring[i] = ext_row<V>(s, G.stride, p0 - HW + i, off, end, nl1, HW, E);

#pragma unroll 1
    for (int p = p0; p < p1; p += W) {
#pragma unroll
        for (int j = 0; j < W; j++) {
            const int q = p + j;
            ring[(j + 2 * HW) % W] = ext_row<V>(s, G.stride, q + HW, off, end, nl1, HW, E);
            if (q < p1) {
                vec acc = Vec<V>::zero();
#pragma unroll
                for (int dd = -HW; dd <= HW; dd++)
                    Vec<V>::mac(acc, T.k[dd + HW], ring[(j + HW - dd) % W]);
                Vec<V>::st(d + (size_t)q * G.stride, acc);
            }
        }
    }
}

// ---- dyadic unit factors (octaves >= 1): per-tap constant (offset, frac) -------------------
// For uf = 2^-k the sample coordinate g - d*uf is exact in float, so every interior output
// uses the same per-tap integer offset and interpolation weights (computed on the host with
// the reference's float expressions).  One thread per V-wide column and output row; the
// arithmetic per tap is the literal tap*((1-frac)*lo + frac*hi).
struct DyadTaps {
    float k[SIFT3D_HIP_MAX_TAPS];
    float w0[SIFT3D_HIP_MAX_TAPS]; // 1 - frac
    float w1[SIFT3D_HIP_MAX_TAPS]; // frac
    int off[SIFT3D_HIP_MAX_TAPS];  // lo - g
};

template <int HW, int V>
__global__ __launch_bounds__(256) void k_fir_sweep_dyad(FirParams P, SweepGeom G, DyadTaps T)
{
    typedef typename Vec<V>::T vec;
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= G.ncols)
        return;
    const int q = G.out_lo + blockIdx.y;
    const size_t base = (size_t)(G.outer_lo + col / G.cols_inner) * G.outer_stride +
                        (size_t)(col % G.cols_inner) * V;
    const float *__restrict__ s = P.src + base;
    float *__restrict__ d = P.dst + base;
    const int g = q + P.off;
    const int nl1 = G.n_loc - 1;
    const int W = HW > 0 ? 2 * HW + 1 : 2 * P.hw + 1;   // HW == 0: run-time width
    vec acc = Vec<V>::zero();
    if (g >= P.uhw && g <= P.n_glob - 2 - P.uhw) {
#pragma unroll
        for (int t = 0; t < W; t++) {
            const int lo = clampi(q + T.off[t], 0, nl1);
            const int hi = clampi(q + T.off[t] + 1, 0, nl1);
            const vec a = Vec<V>::ld(s + (size_t)lo * G.stride);
            const vec b = Vec<V>::ld(s + (size_t)hi * G.stride);
            const float tap = T.k[t], w0 = T.w0[t], w1 = T.w1[t];
            const float *af = reinterpret_cast<const float *>(&a);
            const float *bf = reinterpret_cast<const float *>(&b);
            float *cf = reinterpret_cast<float *>(&acc);
#pragma unroll
            for (int v = 0; v < V; v++)
                cf[v] += tap * (w0 * af[v] + w1 * bf[v]);
        }
    } else {
        float *cf = reinterpret_cast<float *>(&acc);
#pragma unroll
        for (int v = 0; v < V; v++)
            cf[v] = fir_literal_t<HW>(s + v, G.stride, g, P.n_glob, P.off, G.n_loc, T.k, P.hw, P.uf,
                                      P.uhw);
    }
    Vec<V>::st(d + (size_t)q * G.stride, acc);
}

// x pass for dyadic unit factors: one thread per output voxel
template <int HW>
__global__ __launch_bounds__(256) void k_fir_x_dyad(FirParams P, DyadTaps T)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= P.nx)
        return;
    const int row = blockIdx.y; // (y, z) pair inside the plane range
    const size_t rowoff = ((size_t)(P.z_lo + row / P.ny) * P.ny + (row % P.ny)) * P.nx;
    const float *__restrict__ s = P.src + rowoff;
    const int nl1 = P.nx - 1;
    const int W = HW > 0 ? 2 * HW + 1 : 2 * P.hw + 1;
    float acc = 0.0f;
    if (x >= P.uhw && x <= P.nx - 2 - P.uhw) {
#pragma unroll
        for (int t = 0; t < W; t++) {
            const float a = s[clampi(x + T.off[t], 0, nl1)];
            const float b = s[clampi(x + T.off[t] + 1, 0, nl1)];
            acc += T.k[t] * (T.w0[t] * a + T.w1[t] * b);
        }
    } else {
        acc = fir_literal_t<HW>(s, 1, x, P.nx, 0, P.nx, T.k, P.hw, P.uf, P.uhw);
    }
    P.dst[rowoff + x] = acc;
}

// ---- tap spacings 1/2 and 1/4 (octaves 1 and 2): register-resident source window -----------
// For uf = 2^-S the interior sample of tap d sits at g + off_d + frac_d with the COMPILE-TIME
// constants off_d = floor(-d / 2^S) and frac_d = (-d mod 2^S) / 2^S (exactly what the
// reference's float expressions give, imutil.c:783-788, since g - d*uf is exact).  Source rows
// g-R .. g+R+1 (R = ceil(HW / 2^S)) are kept in a register ring (y/z sweeps) or a register
// window filled from LDS (x), so each input is loaded once per thread, and every term is the
// literal tap*((1-frac)*lo + frac*hi) (tap*lo when frac == 0).  Outputs classified "boundary"
// by the reference (g < uhw or g > n-2-uhw) take the literal mirror arithmetic: wave-uniform
// rows in the sweeps; for the x pass a separate edge kernel overwrites the few columns.
template <int S> __host__ __device__ constexpr int dy_off(int d) { return (-d) >> S; }
template <int S> __host__ __device__ constexpr int dy_num(int d) { return (-d) - (((-d) >> S) << S); }

template <int S, int V>
__device__ __forceinline__ void dy_term(typename Vec<V>::T &acc, float k, int d,
                                        const typename Vec<V>::T &a, const typename Vec<V>::T &b)
{
    const int num = (-d) - (((-d) >> S) << S);
    if (num == 0) {
        Vec<V>::mac(acc, k, a);
    } else {
        const float w1 = (float)num / (float)(1 << S), w0 = 1.0f - w1;
        Vec<V>::mac(acc, k, Vec<V>::lerp(w0, a, w1, b));
    }
}

template <int HW, int S, int V>
__global__ __launch_bounds__(256) void k_fir_sweep_dy(FirParams P, SweepGeom G, FirTaps T)
{
    typedef typename Vec<V>::T vec;
    constexpr int R = (HW + (1 << S) - 1) >> S;   // ceil(HW / 2^S)
    constexpr int RW = 2 * R + 2;
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= G.ncols)
        return;
    const int p0 = G.out_lo + blockIdx.y * P.ts;
    const int p1 = min(p0 + P.ts, G.out_hi);
    const size_t base = (size_t)(G.outer_lo + col / G.cols_inner) * G.outer_stride +
                        (size_t)(col % G.cols_inner) * V;
    const float *__restrict__ s = P.src + base;
    float *__restrict__ d = P.dst + base;
    const int nl1 = G.n_loc - 1;
    const int off = P.off, n_glob = P.n_glob, uhw = P.uhw;

    vec ring[RW];
#pragma unroll
    for (int i = 0; i < RW - 1; i++)
        ring[i] = Vec<V>::ld(s + (size_t)clampi(p0 - R + i, 0, nl1) * G.stride);

#pragma unroll 1
    for (int p = p0; p < p1; p += RW) {
#pragma unroll
        for (int j = 0; j < RW; j++) {
            const int q = p + j;
            ring[(j + RW - 1) % RW] = Vec<V>::ld(s + (size_t)clampi(q + R + 1, 0, nl1) * G.stride);
            if (q < p1) {
                const int g = q + off;
                vec acc = Vec<V>::zero();
                if (g >= uhw && g <= n_glob - 2 - uhw) {
#pragma unroll
                    for (int dd = -HW; dd <= HW; dd++) {
                        const int o = ((-dd) >> S);          // floor(-d / 2^S), compile time
                        dy_term<S, V>(acc, T.k[dd + HW], dd, ring[(j + o + R + RW) % RW],
                                      ring[(j + o + R + 1 + RW) % RW]);
                    }
                } else {
                    float *a = reinterpret_cast<float *>(&acc);
#pragma unroll
                    for (int v = 0; v < V; v++)
                        a[v] = fir_literal_t<HW>(s + v, G.stride, g, n_glob, off, G.n_loc, T.k, HW,
                                                 P.uf, uhw);
                }
                Vec<V>::st(d + (size_t)q * G.stride, acc);
            }
        }
    }
}

// RX outputs per lane: 8, or 4 for rows of at most 256 voxels (all 64 lanes busy from octave 1 of a
// 512^3 volume on)
template <int HW, int S, int RX>
__global__ __launch_bounds__(256) void k_fir_x_dy(FirParams P, FirTaps T)
{
    constexpr int SEG = 64 * RX, HALO = 8, L = SEG + 2 * HALO;
    constexpr int R = (HW + (1 << S) - 1) >> S;
    static_assert(R + 1 <= HALO, "halo too small");
    __shared__ __attribute__((aligned(16))) float lds[4][L];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nrows = P.ny * (P.z_hi - P.z_lo);
    const int nx = P.nx;
    const int nmain = (nrows + 3) / 4;             // blockIdx.y >= nmain: boundary-column blocks
    if ((int)blockIdx.y >= nmain) {
        // The uhw low and uhw + 1 high columns of every row take the reference's boundary
        // path (imutil.c:829-850): one thread per such output, the literal arithmetic.  They
        // ride in the same launch; the interior blocks below do not store those columns.
        const int nedge = 2 * P.uhw + 1;
        const size_t i = ((size_t)(blockIdx.y - nmain) * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        if (i >= (size_t)nrows * nedge)
            return;
        const size_t erow = i / nedge;
        const int e = (int)(i % nedge);
        const int x = e < P.uhw ? e : nx - 1 - P.uhw + (e - P.uhw);
        if (x < 0 || x >= nx || (x >= P.uhw && x <= nx - 2 - P.uhw))
            return;
        const size_t eoff = ((size_t)P.z_lo * P.ny + erow) * nx;
        P.dst[eoff + x] = fir_literal_t<HW>(P.src + eoff, 1, x, nx, 0, nx, T.k, P.hw, P.uf, P.uhw);
        return;
    }
    const int row = blockIdx.y * 4 + wave;
    const bool active = row < nrows;
    const int x0 = blockIdx.x * SEG;
    const size_t rowoff = active ? ((size_t)(P.z_lo + row / P.ny) * P.ny + (row % P.ny)) * nx : 0;
    const float *__restrict__ s = P.src + rowoff;
    float *__restrict__ d = P.dst + rowoff;
    const bool vec_ok = (nx & 3) == 0 && ((((uintptr_t)P.src | (uintptr_t)P.dst) & 15) == 0);
    if (active) {
        for (int i = lane; i < L / 4; i += 64) {
            const int gx = x0 - HALO + 4 * i;
            float4 v;
            if (vec_ok && gx >= 0 && gx + 3 < nx) {
                v = ld4(s + gx);
            } else {
                v.x = (gx >= 0 && gx < nx) ? s[gx] : 0.0f;
                v.y = (gx + 1 >= 0 && gx + 1 < nx) ? s[gx + 1] : 0.0f;
                v.z = (gx + 2 >= 0 && gx + 2 < nx) ? s[gx + 2] : 0.0f;
                v.w = (gx + 3 >= 0 && gx + 3 < nx) ? s[gx + 3] : 0.0f;
            }
            *reinterpret_cast<float4 *>(&lds[wave][4 * i]) = v;
        }
    }
    __syncthreads();
    if (!active)
        return;
    const int xb = x0 + lane * RX;
    if (xb >= nx)
        return;
    float w[RX + 2 * HALO];
#pragma unroll
    for (int i = 0; i < (RX + 2 * HALO) / 4; i++) {
        const float4 v = *reinterpret_cast<const float4 *>(&lds[wave][lane * RX + 4 * i]);
        w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
    float o[RX];
#pragma unroll
    for (int r = 0; r < RX; r++) {
        float acc = 0.0f;
#pragma unroll
        for (int dd = -HW; dd <= HW; dd++) {
            const int of = ((-dd) >> S);
            dy_term<S, 1>(acc, T.k[dd + HW], dd, w[HALO + r + of], w[HALO + r + of + 1]);
        }
        o[r] = acc;
    }
    // boundary columns belong to the edge blocks of this launch
    const bool has_edge = xb < P.uhw || xb + RX - 1 > nx - 2 - P.uhw;
    if (has_edge) {
#pragma unroll
        for (int r = 0; r < RX; r++)
            if (xb + r < nx && xb + r >= P.uhw && xb + r <= nx - 2 - P.uhw)
                d[xb + r] = o[r];
    } else if (vec_ok && xb + RX <= nx) {
#pragma unroll
        for (int r = 0; r < RX; r += 4)
            st4(d + xb + r, make_float4(o[r], o[r + 1], o[r + 2], o[r + 3]));
    } else {
#pragma unroll
        for (int r = 0; r < RX; r++)
            if (xb + r < nx)
                d[xb + r] = o[r];
    }
}

// ---------------------------------------------------------------------------------------
// im_downsample_2x  (imutil.c:591-617)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_downsample2(const float *__restrict__ src, int nx, int ny,
                                                     float *__restrict__ dst, int mx, int my,
                                                     int mz)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y;
    const int z = blockIdx.z;
    if (x >= mx)
        return;
    dst[(size_t)x + (size_t)mx * ((size_t)y + (size_t)my * z)] =
        src[(size_t)(2 * x) + (size_t)nx * ((size_t)(2 * y) + (size_t)ny * (2 * z))];
}

// the same for rows of whole quads on both sides (mx % 4 == 0, nx >= 2 mx, 16-byte aligned): a thread reads
// two 16-byte quads and writes one; a workgroup covers 4 output rows of up to 256 voxels.  (One dword per
// thread and 1 KB per workgroup made the first link of the smaller octaves' chain -- 512^3 -> 256^3 -- a
// 65 536-workgroup launch.)
__global__ __launch_bounds__(256) void k_downsample2_q(const float *__restrict__ src, int nx, int ny,
                                                       float *__restrict__ dst, int mxq, int my, int mz)
{
    const int qx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int z = blockIdx.z;
    if (qx >= mxq || y >= my)
        return;
    const float *s = src + (size_t)(8 * qx) + (size_t)nx * ((size_t)(2 * y) + (size_t)ny * (2 * z));
    const float4 a = ld4(s), b = ld4(s + 4);
    st4(dst + (size_t)(4 * qx) + (size_t)(4 * mxq) * ((size_t)y + (size_t)my * z), make_float4(a.x, a.z, b.x, b.z));
}

// ---------------------------------------------------------------------------------------
// synthetic lattice volume (twin of synth.c:sift3d_amd_synth_lattice_voxel)
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t mix64(uint64_t v)
{
    v += 0x9E3779B97F4A7C15ull;
    v = (v ^ (v >> 30)) * 0xBF58476D1CE4E5B9ull;
    v = (v ^ (v >> 27)) * 0x94D049BB133111EBull;
    return v ^ (v >> 31);
}

__device__ __forceinline__ float unit_f(uint64_t h, int k)
{
    return (float)((h >> (16 * k)) & 0xFFFF) * (1.0f / 65536.0f);
}

__global__ __launch_bounds__(256) void k_synth_lattice(float *__restrict__ dst, int nx, int ny,
                                                       int nz, int z_off, uint64_t seed)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y, zl = blockIdx.z, z = zl + z_off;
    if (x >= nx)
        return;
    const int cell = SIFT3D_AMD_SYNTH_CELL;
    const uint64_t hv = mix64(seed ^ mix64(((uint64_t)(uint32_t)x) | ((uint64_t)(uint32_t)y << 21) |
                                           ((uint64_t)(uint32_t)z << 42)));
    float v = 0.05f * unit_f(hv, 0);
    const int gx = x / cell, gy = y / cell, gz = z / cell;
    for (int iz = gz - 1; iz <= gz + 1; iz++)
        for (int iy = gy - 1; iy <= gy + 1; iy++)
            for (int ix = gx - 1; ix <= gx + 1; ix++) {
                if (ix < 0 || iy < 0 || iz < 0)
                    continue;
                const uint64_t h1 = mix64(seed + 0x51ED270B1ull +
                                          mix64(((uint64_t)ix) | ((uint64_t)iy << 21) |
                                                ((uint64_t)iz << 42)));
                const uint64_t h2 = mix64(h1);
                const float cx = ((float)ix + unit_f(h1, 0)) * (float)cell;
                const float cy = ((float)iy + unit_f(h1, 1)) * (float)cell;
                const float cz = ((float)iz + unit_f(h1, 2)) * (float)cell;
                const float sg = 1.5f + 2.5f * unit_f(h1, 3);
                const float a = 2.0f * unit_f(h2, 0) - 1.0f;
                const float dx = (float)x - cx, dy = (float)y - cy, dz = (float)z - cz;
                const float q = dx * dx + 1.3f * dy * dy + 0.7f * dz * dz;
                if (q > 18.0f * sg * sg)
                    continue;
                v += a * s3d_expf(-q / (2.0f * sg * sg));   // == the host twin's libm expf, bit for bit
            }
    dst[(size_t)x + (size_t)nx * ((size_t)y + (size_t)ny * zl)] = v;
}

// device evaluation of the shared math, for tests
__global__ void k_test_expf(const float *in, float *out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        out[i] = s3d_expf(in[i]);
}

__global__ void k_test_eigen3(const double *A, double *Q, double *L, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        s3d_eigen3(A + 9 * i, Q + 9 * i, L + 3 * i);
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
template <int HW>
static void launch_fir_x_u1(const FirParams &P, const FirTaps &T, const EdgeTab &E, hipStream_t st)
{
    const int nrows = P.ny * (P.z_hi - P.z_lo);
    if ((P.nx & 511) == 0 && ((((uintptr_t)P.src | (uintptr_t)P.dst) & 15) == 0)) {
        // rows of whole segments: two rows in flight per wave
        dim3 grid(P.nx / 512, (nrows + 4 * XROWS_F - 1) / (4 * XROWS_F));
        if (P.scale_max)
            hipLaunchKernelGGL((k_fir_x_u1f<HW, true>), grid, dim3(256), 0, st, P, T, E);
        else
            hipLaunchKernelGGL((k_fir_x_u1f<HW, false>), grid, dim3(256), 0, st, P, T, E);
        return;
    }
    dim3 grid((P.nx + 511) / 512, (nrows + 4 * XROWS - 1) / (4 * XROWS));
    hipLaunchKernelGGL(k_fir_x_u1<HW>, grid, dim3(256), 0, st, P, T, E);
}

template <int HW>
static void launch_fir_sweep_u1(const FirParams &P, const SweepGeom &G, const FirTaps &T,
                                const EdgeTab &E, int V, hipStream_t st)
{
    const int nseg = (G.out_hi - G.out_lo + P.ts - 1) / P.ts;
    dim3 grid((G.ncols + 255) / 256, nseg);
    if (V == 4)
        hipLaunchKernelGGL((k_fir_sweep_u1<HW, 4>), grid, dim3(256), 0, st, P, G, T, E);
    else
        hipLaunchKernelGGL((k_fir_sweep_u1<HW, 1>), grid, dim3(256), 0, st, P, G, T, E);
}

// per-tap (offset, 1-frac, frac) of a dyadic unit factor: the reference's float expressions
// (imutil.c:783-788) evaluated at an index where g -+ hw*uf is exact
static void dyad_table(DyadTaps &D, const float *taps, int width, float uf)
{
    const int hw = width / 2;
    memset(&D, 0, sizeof(D));
    for (int d = -hw; d <= hw; d++) {
        const int g0 = 1 << 10;
        const float c = (float)g0 - (float)d * uf;
        const int lo = (int)c;
        const float frac = c - (float)lo;
        D.k[d + hw] = taps[d + hw];
        D.w0[d + hw] = 1.0f - frac;
        D.w1[d + hw] = frac;
        D.off[d + hw] = lo - g0;
    }
}

template <int HW, int S>
static void launch_fir_dy(const FirParams &P, const SweepGeom &G, const FirTaps &T, int V,
                          hipStream_t st)
{
    if (P.axis == 0) {
        const int nrows = P.ny * (P.z_hi - P.z_lo);
        const bool narrow = P.nx <= 256;
        const unsigned gx = narrow ? (P.nx + 255) / 256 : (P.nx + 511) / 512;
        const size_t nedge = (size_t)nrows * (2 * P.uhw + 1);
        const unsigned eblocks = (unsigned)((nedge + (size_t)256 * gx - 1) / ((size_t)256 * gx));
        dim3 grid(gx, (nrows + 3) / 4 + eblocks);   // interior blocks, then boundary-column blocks
        if (narrow)
            hipLaunchKernelGGL((k_fir_x_dy<HW, S, 4>), grid, dim3(256), 0, st, P, T);
        else
            hipLaunchKernelGGL((k_fir_x_dy<HW, S, 8>), grid, dim3(256), 0, st, P, T);
    } else {
        const int nseg = (G.out_hi - G.out_lo + P.ts - 1) / P.ts;
        dim3 grid((G.ncols + 255) / 256, nseg);
        hipLaunchKernelGGL((k_fir_sweep_dy<HW, S, 4>), grid, dim3(256), 0, st, P, G, T);
    }
}

template <int HW>
static void launch_fir_dyad_hw(const FirParams &P, const SweepGeom &G, const DyadTaps &dt, int V,
                               hipStream_t st)
{
    if (P.axis == 0) {
        dim3 grid((P.nx + 255) / 256, P.ny * (P.z_hi - P.z_lo));
        hipLaunchKernelGGL(k_fir_x_dyad<HW>, grid, dim3(256), 0, st, P, dt);
    } else {
        dim3 grid((G.ncols + 255) / 256, G.out_hi - G.out_lo);
        if (V == 4)
            hipLaunchKernelGGL((k_fir_sweep_dyad<HW, 4>), grid, dim3(256), 0, st, P, G, dt);
        else
            hipLaunchKernelGGL((k_fir_sweep_dyad<HW, 1>), grid, dim3(256), 0, st, P, G, dt);
    }
}

static void launch_fir_dyad_generic(const FirParams &P, const SweepGeom &G, const DyadTaps &dt,
                                    int V, hipStream_t st)
{
    dispatch_int_or<1, 8, 0>(P.hw, [&](auto hw) { launch_fir_dyad_hw<hw>(P, G, dt, V, st); });
}

template <int S>
static bool launch_fir_dy_hw(const FirParams &P, const SweepGeom &G, const FirTaps &T, int V,
                             hipStream_t st)
{
    return dispatch_int<1, 8>(P.hw, [&](auto hw) { launch_fir_dy<hw, S>(P, G, T, V, st); });
}

static bool is_dyadic(float uf, int *shift)
{
    int e;
    const float m = frexpf(uf, &e);
    if (m != 0.5f || e > 1)
        return false;
    *shift = 1 - e;
    return true;
}

extern "C" {

int sift3d_hip_absmax(const float *d_src, size_t n, float *d_max, void *stream)
{
    if (!n)
        return SIFT3D_SUCCESS;
    hipLaunchKernelGGL(k_absmax, dim3(grid_reduce(n)), dim3(256), 0, (hipStream_t)stream, d_src, n,
                       reinterpret_cast<unsigned *>(d_max));
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

int sift3d_hip_scale(const float *d_src, float *d_dst, size_t n, const float *d_max, void *stream)
{
    if (!n)
        return SIFT3D_SUCCESS;
    hipLaunchKernelGGL(k_scale, dim3(grid_for(n, 16)), dim3(256), 0, (hipStream_t)stream, d_src,
                       d_dst, n, d_max);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

static int fir_impl(const sift3d_hip_fir_args *a, const float *d_scale_max, void *stream);

int sift3d_hip_fir(const sift3d_hip_fir_args *a, void *stream) { return fir_impl(a, nullptr, stream); }

// The x pass of a unit-spaced blur on src / *d_max (im_scale, imutil.c:698-713, folded into the pass: the
// scaled image is never stored).  1: not covered (the caller scales first, then calls sift3d_hip_fir).
// (one predicate for the entry's own check and for callers that must know BEFORE they launch: the slab
// driver's ranks have to agree on the path whatever happens to one of them)
int sift3d_hip_fir_x_scaled_covers(const sift3d_hip_fir_args *a)
{
    if (!a)
        return 0;
    const int hw = a->width / 2;
    return !(a->axis != 0 || a->variant == 1 || a->unit_factor != 1.0f || hw < 1 || hw > 8 ||
             a->nx < 2 * hw + 2 || a->nx >= (1 << 22));
}

int sift3d_hip_fir_x_scaled(const sift3d_hip_fir_args *a, const float *d_max, void *stream)
{
    if (!a || !d_max)
        return SIFT3D_FAILURE;
    if (!sift3d_hip_fir_x_scaled_covers(a))
        return 1;
    return fir_impl(a, d_max, stream);
}

static int fir_impl(const sift3d_hip_fir_args *a, const float *d_scale_max, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!a || !a->src || !a->dst || a->nx < 1 || a->ny < 1 || a->nz < 1 || a->axis < 0 ||
        a->axis > 2 || a->width < 1 || !(a->width & 1) || a->width > (1 << 20) ||
        a->z_lo < 0 || a->z_hi > a->nz || a->src == a->dst)
        return launch_fail("sift3d_hip_fir", "invalid arguments");
    if (a->z_hi <= a->z_lo)
        return SIFT3D_SUCCESS;
    FirParams P;
    FirTaps T;
    memset(&T, 0, sizeof(T));
    memcpy(T.k, a->taps, sizeof(float) * (a->width < SIFT3D_HIP_MAX_TAPS ? a->width : SIFT3D_HIP_MAX_TAPS));
    P.src = a->src; P.dst = a->dst;
    P.nx = a->nx; P.ny = a->ny; P.nz = a->nz;
    P.axis = a->axis;
    P.hw = a->width / 2;
    P.uf = a->unit_factor;
    P.uhw = (int)ceilf((float)P.hw * P.uf);           // imutil.c:756-757
    const int dims[3] = { a->nx, a->ny, a->nz };
    P.n_glob = a->axis == 2 ? a->n_glob : dims[a->axis];
    P.off = a->axis == 2 ? a->off : 0;
    P.z_lo = a->z_lo; P.z_hi = a->z_hi;
    P.ts = 64;
    P.scale_max = d_scale_max;
    if (a->axis == 2 && (P.off < 0 || P.off + a->nz > P.n_glob))
        return launch_fail("sift3d_hip_fir", "slab outside the global axis");
    const size_t plane = (size_t)a->nx * a->ny;
    if (a->width > SIFT3D_HIP_MAX_TAPS) {
        // wider than the tap tables of the fast kernels: the literal kernel, SIFT3D_HIP_MAX_TAPS taps per launch
        const size_t total = plane * (size_t)(a->z_hi - a->z_lo);
        for (int d_lo = -P.hw; d_lo <= P.hw; d_lo += SIFT3D_HIP_MAX_TAPS) {
            const int d_hi = d_lo + SIFT3D_HIP_MAX_TAPS < P.hw + 1 ? d_lo + SIFT3D_HIP_MAX_TAPS : P.hw + 1;
            memcpy(T.k, a->taps + (d_lo + P.hw), sizeof(float) * (size_t)(d_hi - d_lo));
            hipLaunchKernelGGL(k_fir_literal_chunk, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, P, T,
                               d_lo, d_hi);
        }
        LAUNCH_CHECK();
        return SIFT3D_SUCCESS;
    }
    int shift = 0;
    const bool dyadic = is_dyadic(P.uf, &shift) && shift <= 12 && P.n_glob < (1 << (23 - shift));
    const bool aligned = (((uintptr_t)a->src | (uintptr_t)a->dst) & 15) == 0;

    // geometry of the strided sweeps (y and z passes)
    SweepGeom G;
    int V = 1;
    if (a->axis == 1) {
        V = (aligned && (a->nx & 3) == 0) ? 4 : 1;
        G.cols_inner = a->nx / V;
        G.ncols = G.cols_inner * (a->z_hi - a->z_lo);
        G.outer_stride = plane;
        G.outer_lo = a->z_lo;
        G.stride = a->nx;
        G.n_loc = a->ny;
        G.out_lo = 0; G.out_hi = a->ny;
    } else if (a->axis == 2) {
        V = (aligned && (plane & 3) == 0) ? 4 : 1;
        G.cols_inner = (int)(plane / V);
        G.ncols = G.cols_inner;
        G.outer_stride = 0;
        G.outer_lo = 0;
        G.stride = plane;
        G.n_loc = a->nz;
        G.out_lo = a->z_lo; G.out_hi = a->z_hi;
    }

    if (a->axis != 0) {
        // sweep segmentation: aim at >= 8 waves per SIMD (8192 waves) without letting the ring
        // warm-up (2*hw extra rows per segment) dominate
        const int n_out = G.out_hi - G.out_lo;
        long want = (8192L * 64 + G.ncols - 1) / (G.ncols > 0 ? G.ncols : 1);
        long cap = n_out / 16 > 1 ? n_out / 16 : 1;
        long nseg = want < cap ? want : cap;
        if (nseg < 1)
            nseg = 1;
        P.ts = (int)((n_out + nseg - 1) / nseg);
        if (P.ts < 1)
            P.ts = 1;
    }
    if (a->variant != 1 && P.uf == 1.0f && P.hw >= 1 && P.hw <= 8 &&
        P.n_glob >= 2 * P.hw + 2 && P.n_glob < (1 << 22)) {
        // unit-spaced taps (octave 0): extended-line register-window kernels
        const EdgeTab E = edge_table(P.n_glob, P.hw);
        if (a->axis == 0)
            dispatch_int_or<1, 7, 8>(P.hw, [&](auto hw) { launch_fir_x_u1<hw>(P, T, E, st); });
        else
            dispatch_int_or<1, 7, 8>(P.hw, [&](auto hw) { launch_fir_sweep_u1<hw>(P, G, T, E, V, st); });
    } else if (a->variant != 1 && dyadic && (shift == 1 || shift == 2) && P.hw <= 8 &&
               (a->axis == 0 || V == 4) &&
               (shift == 1 ? launch_fir_dy_hw<1>(P, G, T, V, st) : launch_fir_dy_hw<2>(P, G, T, V, st))) {
        // octaves 1 and 2: compile-time tap spacing, register-resident source window
    } else if (a->variant != 1 && dyadic && P.hw < 1024) {
        DyadTaps dt;
        dyad_table(dt, a->taps, a->width, P.uf);
        launch_fir_dyad_generic(P, G, dt, V, st);
    } else {
        const size_t total = plane * (size_t)(a->z_hi - a->z_lo);
        hipLaunchKernelGGL(k_fir_literal, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, P, T);
    }
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

int sift3d_hip_downsample2(const float *d_src, int nx, int ny, float *d_dst, int mx, int my, int mz,
                           void *stream)
{
    if (mx < 1 || my < 1 || mz < 1)
        return SIFT3D_SUCCESS;
    if ((mx & 3) == 0 && (nx & 3) == 0 && nx >= 2 * mx && ((((uintptr_t)d_src | (uintptr_t)d_dst) & 15) == 0))
        hipLaunchKernelGGL(k_downsample2_q, dim3((mx / 4 + 63) / 64, (my + 3) / 4, mz), dim3(256), 0,
                           (hipStream_t)stream, d_src, nx, ny, d_dst, mx / 4, my, mz);
    else
        hipLaunchKernelGGL(k_downsample2, dim3((mx + 255) / 256, my, mz), dim3(256), 0,
                           (hipStream_t)stream, d_src, nx, ny, d_dst, mx, my, mz);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

int sift3d_hip_synth_lattice(float *d_dst, int nx, int ny, int nz, int z_off, uint64_t seed,
                             void *stream)
{
    hipLaunchKernelGGL(k_synth_lattice, dim3((nx + 255) / 256, ny, nz), dim3(256), 0,
                       (hipStream_t)stream, d_dst, nx, ny, nz, z_off, seed);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

void sift3d_amd_host_expf(const float *in, float *out, size_t n)
{
    for (size_t i = 0; i < n; i++)
        out[i] = s3d_expf(in[i]);
}

void sift3d_amd_host_eigen3(const double *A9, double *Q9, double *L3) { s3d_eigen3(A9, Q9, L3); }

int sift3d_hip_test_expf(const float *d_in, float *d_out, size_t n, void *stream)
{
    hipLaunchKernelGGL(k_test_expf, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, d_in, d_out, n);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

int sift3d_hip_test_eigen3(const double *d_A9, double *d_Q9, double *d_L3, size_t n, void *stream)
{
    hipLaunchKernelGGL(k_test_eigen3, dim3((unsigned)((n + 63) / 64)), dim3(64), 0,
                       (hipStream_t)stream, d_A9, d_Q9, d_L3, n);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

} // extern "C"
