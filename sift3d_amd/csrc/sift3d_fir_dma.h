// sift3d_fir_dma.h -- the LDS-DMA pipeline of k_fir_yz_dma (sift3d_fir_yz.hip) and k_fir_xyz_dma
// (sift3d_fir_xyz.hip) and the host helpers of their C entries: request list, DMA issue, counted waits, virtual
// y rows, and the extended z planes with the state that the wait count depends on.  Only the z register ring
// stays in the kernels, in the same form in both: as a function template of this header it costs k_fir_xyz_dma
// 1-6 VGPRs at every width below 17 taps (profiles/microbench/fir_dma_core_mi355x.txt).
//
// Both kernels blur a 64(x) x TY(y) column of the volume along a segment of z.  k_fir_yz_u1 does the same with
// rows loaded through registers and is bound by latency, not by bytes or arithmetic: one workgroup per CU, one
// barrier per plane, and the rows of plane p + 1 are requested only while plane p is filtered: 17-20 KB in flight
// per CU against the ~50 KB that 6 TB/s need at ~2 us of loaded latency.  Here the rows of a plane go from HBM
// straight into one of FOUR LDS tiles (global_load_lds_dwordx4: no staging registers, no ds_write), three requests
// ahead of the one being filtered:
//   * the REQUEST LIST `seq` holds the source planes of the workgroup in the order the sweep consumes them;
//   * request t + 3 is issued right after the barrier that opens request t -- the tile it overwrites was last
//     read before that barrier;
//   * each wave waits for its own pieces of request t with a COUNTED s_waitcnt vmcnt(N) before that barrier, never
//     vmcnt(0): N = the wave's younger vector-memory operations = the pieces of requests t + 1 and t + 2 and the
//     output stores of the last three iterations (`shist`).  The DMA is inline assembly, so the compiler neither
//     counts it nor drains it; the output stores are the only vector-memory operations it sees;
//   * beyond the end of the list the last request is issued again (the same bytes to a tile nobody reads), so
//     that the count of pieces in flight -- and with it N -- stays what it is everywhere else.
// The count, the clamp and the store history are correct only TOGETHER: a mistake does not fault, it filters a
// tile before its rows have landed.  Hence one copy of them, here.
//
// A kernel supplies what differs: `issue(pl, b)`, the DMA pieces of ITS wave for source plane pl into tile b (the
// staging geometry; the same number of pieces for every request), and `filter(b)`, the y-filtered float4 of its
// thread's column from tile b (called by the whole workgroup right after the barrier that opens the request).
// Edges: mirrored rows and planes are source ADDRESSES; the virtual rows of the high y face are formed in LDS
// (DmaYEdge); the virtual planes of the high z face from two y-filtered planes, i.e. the z edge rules act on the y
// pass's OUTPUT as in the reference (apply_Sep_FIR_filter runs the passes one after the other, imutil.c:1165-1188).
#pragma once
#include "sift3d_kernels_common.h"

constexpr int DMA_NB = 4;         // LDS tiles of a workgroup: the open request and three in flight
constexpr int DMA_TXQ = 16;       // quads of a row that the y filter reads (a workgroup is 64 voxels wide)
constexpr int DMA_SEQ = 320;      // capacity of the request list: seq[DMA_SEQ] holds its length
constexpr int DMA_MAX_TS = 256;   // longest z segment a launcher may ask for: 256 + 2 * 8 planes + 9 second requests

// One 16-byte DMA piece per lane: global address g -> LDS, lane l at lds + 16 l (lds: wave-uniform byte address,
// through m0, which the compiler owns otherwise: saved and restored)
__device__ __forceinline__ void dma_load_lds_16(const float *g, uint32_t lds)
{
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(g), "s"(lds) : "memory");
}

// wait until at most n of this wave's vector-memory operations are outstanding, then the barrier
__device__ __forceinline__ void dma_wait_vm_barrier(int n)
{
    switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(1)\n\ts_barrier" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)\n\ts_barrier" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)\n\ts_barrier" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)\n\ts_barrier" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)\n\ts_barrier" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(7)\n\ts_barrier" ::: "memory"); break;
    }
}

// the barrier between two phases that hand data over in LDS
__device__ __forceinline__ void dma_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// The re-requests beyond the list are still in flight when the sweep ends: they write LDS only, and a wave's
// vector-memory operations complete before its program ends.
__device__ __forceinline__ void dma_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// The y-filter requests of a workgroup in the order its sweep consumes them, as LOCAL plane indices: for every
// extended plane r = p0 - HW .. p1 - 1 + HW (global index r + off) its mirror image at the low face, the two
// planes a virtual plane interpolates at the high face (global index >= endz), none beyond the taps' reach.
// Returns the length of the list (wave-uniform); nl1 = the last local plane.
template <int HW>
__device__ __forceinline__ int dma_build_requests(int *seq, const EdgeTab &Ez, int p0, int p1, int off, int endz, int nl1)
{
    if (threadIdx.x == 0) {
        int n = 0;
        for (int r = p0 - HW; r < p1 + HW && n + 2 <= DMA_SEQ; r++) {
            const int i = r + off;
            if (i < 0) {
                seq[n++] = clampi(-i - off, 0, nl1);
            } else if (i >= endz) {
                const int m = i - endz;
                if (m <= HW) {
                    int lo = 0;
                    for (int mm = 0; mm <= HW; mm++)
                        lo = mm == m ? Ez.lo[mm] : lo;
                    seq[n++] = clampi(lo - off, 0, nl1);
                    seq[n++] = clampi(lo + 1 - off, 0, nl1);
                }
            } else {
                seq[n++] = clampi(r, 0, nl1);
            }
        }
        seq[DMA_SEQ] = n;
    }
    __syncthreads();
    return __builtin_amdgcn_readfirstlane(seq[DMA_SEQ]);
}

// source plane of request t (clamped: beyond the list a harmless re-request keeps the count of pieces in flight)
__device__ __forceinline__ int dma_request(const int *seq, int nreq, int t)
{
    return __builtin_amdgcn_readfirstlane(seq[min(t, nreq - 1)]);
}

// Virtual rows E[endy + m], m = 0 .. HW, of the high y face (imutil.c:846-848), formed in LDS from the two rows
// they interpolate, by the workgroups of the last tile row only (one more barrier there).  `rows` holds ROWS rows
// of DMA_TXQ quads, row j = extended-y index y0 - HW + j, and the row of a virtual sample holds anything before.
// Thread -> (m, quad) = (tid / 16, tid % 16).
template <int HW, int ROWS> struct DmaYEdge {
    bool yedge, efix;      // block-uniform: the tile has such rows; this thread forms one
    int ej, elo;           // its tile row; the lower of the two rows it interpolates
    float ew0, ew1;
    int col;               // quad (ty, qx) of `rows`: formed once (left to the compiler it costs the y+z kernel a VGPR)

    __device__ __forceinline__ DmaYEdge(const EdgeTab &Ey, int y0, int TY, int endy, int ty, int qx)
    {
        col = ty * DMA_TXQ + qx;
        const int em = threadIdx.x >> 4;
        yedge = y0 + TY + HW > endy;
        ej = endy + em - (y0 - HW);
        efix = yedge && em <= HW && ej < ROWS;
        elo = 0;
        ew0 = ew1 = 0.0f;
#pragma unroll
        for (int mm = 0; mm <= HW; mm++)
            if (mm == em) {
                // (through readfirstlane: the table's entries stay scalar loads selected by value.  Selected by
                // address they become per-lane loads, whose wait -- a vmcnt(0) -- lands in the filter)
                elo = __builtin_amdgcn_readfirstlane(Ey.lo[mm]) - (y0 - HW);
                ew0 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(Ey.w0[mm])));
                ew1 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(Ey.w1[mm])));
            }
    }
};

// the y taps of a thread (quad qx of its row) from `rows` (as above), the tile's virtual rows formed first
template <int HW, int ROWS>
__device__ __forceinline__ float4 dma_filter_y(const FirTaps &T, const DmaYEdge<HW, ROWS> &ye, float4 *rows, int qx)
{
    if (ye.yedge) {
        if (ye.efix) {
            const float4 a = rows[clampi(ye.elo, 0, ROWS - 1) * DMA_TXQ + qx];
            const float4 c = rows[clampi(ye.elo + 1, 0, ROWS - 1) * DMA_TXQ + qx];
            rows[ye.ej * DMA_TXQ + qx] = Vec<4>::lerp(ye.ew0, a, ye.ew1, c);
        }
        dma_lds_barrier();
    }
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int dd = -HW; dd <= HW; dd++)
        Vec<4>::mac(acc, T.k[dd + HW], rows[ye.col + (HW - dd) * DMA_TXQ]);
    return acc;
}

// the pipeline's state: all of it wave-uniform
struct DmaSweep {
    const int *seq;     // the request list and its length
    int nreq;
    int pieces;         // DMA pieces of this wave per request
    int t;              // next request to be consumed
    int shist;          // output stores of this wave in the last three iterations (bits 0..2)
};

// issue request t into its tile
template <class Issue> __device__ __forceinline__ void dma_stage(const DmaSweep &s, int t, Issue &&issue)
{
    issue(dma_request(s.seq, s.nreq, t), t & (DMA_NB - 1));
}

// open the next request of the list, y-filtered; `stored`: an output store of this wave follows it
template <class Issue, class Filter>
__device__ __forceinline__ float4 dma_next(DmaSweep &s, bool stored, Issue &&issue, Filter &&filter)
{
    // younger than the pieces of request t: those of t + 1 and t + 2, and this wave's recent stores
    dma_wait_vm_barrier(2 * s.pieces + __builtin_popcount(s.shist));
    dma_stage(s, s.t + DMA_NB - 1, issue);
    const float4 v = filter(s.t & (DMA_NB - 1));
    s.t++;
    s.shist = ((s.shist << 1) | (int)stored) & 7;
    return v;
}

// Extended-z plane with global index i (beyond the volume at its faces): one or two requests.  `stores`: this
// wave stores an output plane after it.
template <int HW, int HW1, class Issue, class Filter>
__device__ __forceinline__ float4 dma_ext_z(DmaSweep &s, const EdgeTab &Ez, int i, int endz, bool stores, Issue &&issue,
                                            Filter &&filter)
{
    // Every plane but the high face's virtual ones (block-uniform) takes ONE request and nothing else: as a path of
    // its own it frees the plane loop of the selects and copies that merged it with the two-request case (~65 of
    // ~340 vector instructions per plane at 13 taps of the y+z kernel, and the wide instances are bound by their
    // vector instructions).  Up to half width HW1 only: a second inlined copy of the filter per ring position costs
    // the register allocator scratch at 17 taps (y+z: 72 dwords) and from 13 taps on where the filter has an x
    // phase (x+y+z: 960 and 992 bytes per lane at 13 and 15 taps).
    if (HW <= HW1 && i < endz)
        return dma_next(s, stores, issue, filter);
    int np = 1;
    float w0 = 1.0f, w1 = 0.0f;
    if (i >= endz) {
        const int m = i - endz;
        np = m > HW ? 0 : 2;
#pragma unroll
        for (int mm = 0; mm <= HW; mm++)
            if (mm == m) {
                w0 = Ez.w0[mm];
                w1 = Ez.w1[mm];
            }
    }
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
    for (int k = 0; k < np; k++) {
        // (the store that follows this plane belongs to the LAST of its requests)
        const float4 yv = dma_next(s, stores && k + 1 == np, issue, filter);
        // (block-uniform; the second request of a virtual plane interpolates in place: w0 * first + w1 * second)
        if (k == 0)
            a = yv;
        else
            a = Vec<4>::lerp(w0, a, w1, yv);
    }
    if (np == 0)
        s.shist = ((s.shist << 1) | (int)stores) & 7;   // (a store without a request)
    return a;
}

// Start a workgroup's pipeline for output planes p0 .. p1 - 1 (local indices; global = local + off; endz = the
// last GLOBAL plane, nl1 the last local one): build the request list in `seq` (DMA_SEQ + 1 ints of LDS) and put
// the first DMA_NB - 1 requests in flight.  `pieces`: DMA pieces per request that issue() issues for this wave.
template <int HW, class Issue>
__device__ __forceinline__ DmaSweep dma_begin(int *seq, const EdgeTab &Ez, int pieces, int p0, int p1, int off, int endz,
                                              int nl1, Issue &&issue)
{
    DmaSweep s;
    s.seq = seq;
    s.nreq = dma_build_requests<HW>(seq, Ez, p0, p1, off, endz, nl1);
    s.pieces = pieces;
    s.t = 0;
    s.shist = 0;
#pragma unroll
    for (int t = 0; t < DMA_NB - 1; t++)
        dma_stage(s, t, issue);
    return s;
}

// ---- host side ----------------------------------------------------------------------------------------------
// z segmentation of n_out output planes where the tiles give blocks_xy workgroups per segment: at least 512
// workgroups (4096 waves in flight), segments of at least 32 planes and at most DMA_MAX_TS (the request list).
static inline void fir_dma_segments(long blocks_xy, int n_out, int *ts, int *nseg)
{
    if (blocks_xy < 1)
        blocks_xy = 1;
    const long want = (512 + blocks_xy - 1) / blocks_xy;
    const long cap = n_out / 32 > 1 ? n_out / 32 : 1;
    long n = want < cap ? want : cap;
    if ((n_out + n - 1) / n > DMA_MAX_TS)
        n = (n_out + DMA_MAX_TS - 1) / DMA_MAX_TS;
    *ts = (int)((n_out + n - 1) / n);
    *nseg = (n_out + *ts - 1) / *ts;
}

// parameters and taps of a unit-spaced pass over all nz planes of a volume (a slab entry sets n_glob, off, z_lo
// and z_hi afterwards)
static inline void fir_dma_fill(FirParams *P, FirTaps *T, const float *d_src, float *d_dst, int nx, int ny, int nz,
                                const float *taps, int width)
{
    memset(T, 0, sizeof(*T));
    memcpy(T->k, taps, sizeof(float) * width);
    memset(P, 0, sizeof(*P));
    P->src = d_src; P->dst = d_dst;
    P->nx = nx; P->ny = ny; P->nz = nz;
    P->axis = 2; P->hw = width / 2; P->uf = 1.0f; P->uhw = width / 2;
    P->n_glob = nz; P->z_hi = nz;
}
