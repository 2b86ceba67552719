// sift3d_match.hip -- brute-force nearest / second-nearest neighbour of 768-float descriptors.
//
// BASELINE config 5 ("two volumes: detect + describe both, NN match, RANSAC affine").  The
// matcher and the RANSAC fit were REMOVED from the reference fork (CHANGES.md:99-103; upstream
// description README-OLD.md:5), so there is no reference code, no oracle and no fixture for this
// stage: parity with upstream cannot be pinned.  What is built is the textbook form of what
// upstream describes -- for every descriptor of set A the nearest and second nearest descriptor
// of set B under the L2 distance, accepted by Lowe's ratio test.  Every value it returns is pinned
// bit for bit to a numpy restatement of the arithmetic below (tests/match_restatement.py,
// tests/test_match.py): the row norms' lane order, the fma chain in group()'s k order, the
// lexicographic top-2 and the clamp.
//
// This is the one dense contraction of the project: |a - b|^2 = |a|^2 + |b|^2 - 2 a.b, an
// (nA x 768) x (768 x nB) matrix product, done on the matrix cores with
// v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate: bit-for-bit an ordered f32 fma chain, at the
// f32 vector peak rate but with one operand register per lane, leaving the VALU to the top-2
// bookkeeping).  A workgroup owns 128 descriptors of A, walks a run of B in blocks of 128 and
// keeps, per lane and row, the two smallest distances seen; the 128 x 128 distance block is
// never stored.  B is cut into up to 16 runs per row block of A (enough workgroups to fill the
// device several times over); k_nn2_merge combines the per-run top-2.
//
// sift3d_hip_nn2_gated is the same search over the candidates inside a spatial gate (guided matching, once a
// first transform predicts where a keypoint lies in the other volume): k_nn2_gated shares k_nn2's body, gates the
// epilogue's pushes and skips the blocks of B whose box lies beyond the radius (tests/match_guided_restatement.py).
#include "sift3d_kernels_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int MT = 128, NT = 128, KC = 32;      // block of A rows, of B rows, K chunk
constexpr int LDK = KC + 4;                      // LDS row stride in floats (see k_nn2)

// squared norms of the rows
__global__ __launch_bounds__(256) void k_row_norms(const float *__restrict__ a, int n, int dim,
                                                   float *__restrict__ out)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n)
        return;
    float s = 0.0f;
    for (int k = lane; k < dim; k += 64) {
        const float v = a[(size_t)row * dim + k];
        s += v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        s += __shfl_xor(s, o, 64);
    if (lane == 0)
        out[row] = s;
}

struct Top2 {
    float d1, d2;
    int j1;
};

// (distance, index) pairs compare lexicographically: ties go to the smaller index, so the result
// does not depend on the order in which candidates arrive
__device__ __forceinline__ void top2_push(Top2 &t, float d, int j)
{
    const bool first = d < t.d1 || (d == t.d1 && j < t.j1);
    const float nd2 = first ? t.d1 : fminf(t.d2, d);
    t.d1 = first ? d : t.d1;
    t.j1 = first ? j : t.j1;
    t.d2 = nd2;
}

__device__ __forceinline__ void top2_merge(Top2 &t, float d1, float d2, int j1)
{
    top2_push(t, d1, j1);
    t.d2 = fminf(t.d2, d2);
}

// What the gated search (sift3d_hip_nn2_gated) adds to a workgroup of k_nn2: the two position arrays, the
// row orders, the boxes of the 128-row blocks and the block-pair counters, and its own LDS (the ungated
// kernel declares none of it and passes NULL).
struct Nn2Gate {
    const float4 *posA, *posB;          // n x (x, y, z, ignored), indexed by ORIGINAL row
    const int *permA, *permB;           // block row r is original row perm[r] (NULL: the identity)
    const float *boxA, *boxB;           // per 128-row block, in block order: lo x, y, z, -, hi x, y, z, -
    unsigned long long *visited;        // NULL or {block pairs visited, block pairs in all}
    float r2;
    float4 *posAs;                      // LDS: [MT] positions of the A block's rows
    int *idxA, *idxB;                   // LDS: [MT], [2][NT] original (clamped) rows of the block rows
};

// gate(i, j) of include/sift3d_amd.h: f32 differences, (dx dx + dy dy) + dz dz (this unit is built without
// contraction), <= r2; a NaN makes it false.  Swapping a and b only negates the differences: the backward search
// computes the same d2 bit for bit.
__device__ __forceinline__ bool nn2_gate(const float4 &a, const float4 &b, float r2)
{
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return (dx * dx + dy * dy) + dz * dz <= r2;
}

// A: nA x dim, B: nB x dim (row-major, dim % KC == 0).  out: for each row of A the index of the
// nearest row of B, the squared distance to it and to the second nearest (+inf if nB < 2).
// GATED: only the rows of B inside the gate of the row of A are candidates, blocks of B whose box lies
// farther than the radius from the A block's box are not computed at all, and rows are walked in the order
// of the permutations.  Everything gated is compiled out of the ungated instantiation, which is k_nn2 as it
// was (same registers, same LDS).
template <bool GATED>
__device__ __forceinline__ void nn2_block(const float *__restrict__ A, int nA, const float *__restrict__ B,
                                          int nB, int dim, const float *__restrict__ normB, int jb_per_split,
                                          int *__restrict__ out_j, float *__restrict__ out_d1,
                                          float *__restrict__ out_d2, const Nn2Gate &g)
{
    // blockIdx.y: which run of jb_per_split 128-row blocks of B this workgroup scans; its top-2 go to
    // slice blockIdx.y of the outputs (merged by k_nn2_merge when there is more than one)
    const int jlo = blockIdx.y * jb_per_split * NT, jhi = min(nB, jlo + jb_per_split * NT);
    out_j += (size_t)blockIdx.y * nA;
    out_d1 += (size_t)blockIdx.y * nA;
    out_d2 += (size_t)blockIdx.y * nA;
    // Row-major tiles As[row][k] (as the rows lie in memory: the staging stores are 16-byte stores of what
    // the 16-byte global loads delivered, no transposition), rows LDK = KC + 4 floats apart.  A lane of an
    // MFMA operand (row = lane & 31, half h = lane >> 5) takes FOUR k at a time with one 16-byte read,
    // k = 8 g + 4 h + {0, 1, 2, 3}: the j-th of the four v_mfma_f32_32x32x2_f32 of group g then multiplies the
    // k pair (8 g + j, 8 g + 4 + j).  A and B must use the same pairing; the pairing also fixes the order of
    // the fma chain, k = 0, 4, 1, 5, 2, 6, 3, 7 per group, which tests/match_restatement.py restates bit for
    // bit (another pairing changes the last bits of the distances).  Eight consecutive lanes read rows 36 floats
    // apart: 4-float slots at 0, 4, ..., 28 modulo the 32 banks -- conflict-free; a chunk needs 16
    // 16-byte reads and 8 16-byte stores per lane where the k-major layout needed 64 + 32 4-byte ones.
    // Double-buffered: the global loads of chunk c + 1 are in flight during the 64 MFMAs of chunk c and go
    // to the other buffer afterwards -- one barrier per chunk of KC = 32 (two tiles of 2 x 18 KB per
    // workgroup, two workgroups per CU).
    __shared__ __attribute__((aligned(16))) float As[2][MT][LDK];
    __shared__ __attribute__((aligned(16))) float Bs[2][NT][LDK];
    __shared__ float red_d1[MT][2], red_d2[MT][2];
    __shared__ int red_j[MT][2];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wr = wave >> 1, wc = wave & 1;            // 2 x 2 waves, 64 x 64 outputs each
    const int i0 = blockIdx.x * MT;
    const int lr = lane & 31, lh = lane >> 5;
    // staging role: thread t copies the 16-byte pieces (row (t >> 3) + 32 i, columns 4 (t & 7) ..) of both
    // tiles, i = 0..3: eight consecutive lanes cover the 128 contiguous bytes of a row's chunk
    const int srow = tid >> 3, sc4 = (tid & 7) * 4;
    const int nk = dim / KC;

    Top2 best[2][16];
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            best[t][r].d1 = best[t][r].d2 = __builtin_inff();
            best[t][r].j1 = 0x7fffffff;
        }
    // (row addresses are recomputed per load rather than kept in 16 registers: the kernel lives at the edge
    // of its 256)
    const uint32_t udim = (uint32_t)dim;
    // GATED: the A block's original rows and positions go to LDS once (the first barrier of the first visited
    // block publishes them); its box stays in scalar registers
    float alo[3] = { 0.0f, 0.0f, 0.0f }, ahi[3] = { 0.0f, 0.0f, 0.0f };
    int nvis = 0;
    if constexpr (GATED) {
        if (tid < MT) {
            const int r = min(i0 + tid, nA - 1), o = g.permA ? g.permA[r] : r;
            g.idxA[tid] = o;
            g.posAs[tid] = g.posA[o];
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            alo[k] = g.boxA[8 * blockIdx.x + k];
            ahi[k] = g.boxA[8 * blockIdx.x + 4 + k];
        }
    }
    for (int j0 = jlo; j0 < jhi; j0 += NT) {
        int pb = 0;                         // GATED: which half of idxB holds this block's rows
        if constexpr (GATED) {
            // Skip the block when the two boxes are farther apart than the radius.  Per axis the gap is
            // g = max(0, loA - hiB, loB - hiA) in f32, gap2 in the gate's association.  For every row pair of the
            // two blocks |pa - pb| >= g on that axis in the reals, and f32 subtraction, multiplication and
            // addition round monotonically, so the gate's computed d2 >= gap2: gap2 > r2 implies d2 > r2 for
            // every pair, and the skip is exact with no epsilon.  fmaxf drops a NaN (inf - inf of an unbounded
            // box): the block is then visited.  The test is uniform over the workgroup (scalar loads and
            // arithmetic), so the barriers below stay matched.
            const float *bb = g.boxB + 8 * (size_t)(j0 / NT);
            const float gx = fmaxf(0.0f, fmaxf(alo[0] - bb[4], bb[0] - ahi[0]));
            const float gy = fmaxf(0.0f, fmaxf(alo[1] - bb[5], bb[1] - ahi[1]));
            const float gz = fmaxf(0.0f, fmaxf(alo[2] - bb[6], bb[2] - ahi[2]));
            if ((gx * gx + gy * gy) + gz * gz > g.r2)
                continue;
            // original rows of this block: the halves of idxB alternate, since the previous visited block's
            // epilogue may still be reading its half (two barriers separate a half's readers from its next writer)
            pb = nvis & 1;
            nvis++;
            if (tid < NT) {
                const int c = min(j0 + tid, nB - 1);
                g.idxB[pb * NT + tid] = g.permB ? g.permB[c] : c;
            }
        }
        f32x16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 2; b++)
#pragma unroll
                for (int r = 0; r < 16; r++)
                    acc[a][b][r] = 0.0f;
        float4 vs[4];                       // staging registers: the A pieces of a chunk, then its B pieces
        auto fetch = [&](const float *__restrict__ M, int r0, int nrows, const int *idx, int c) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int rr = r0 + srow + 32 * i;
                // rows beyond the end repeat the last row: their distances are never used (the epilogue skips
                // columns >= nB, the final store rows >= nA) -- and nothing may depend on the loaded value
                // here, or the load could not stay in flight during the MFMAs
                // (GATED: the clamped, permuted row comes from LDS -- one 4-byte read per 16-byte load)
                const int row = GATED ? idx[srow + 32 * i] : min(rr, nrows - 1);
                vs[i] = ld4(M + ((size_t)((uint32_t)row) * udim + (uint32_t)(sc4 + c * KC)));
            }
        };
        const int *ixa = GATED ? g.idxA : nullptr, *ixb = GATED ? g.idxB + pb * NT : nullptr;
        auto commit = [&](float (*T)[LDK]) {
#pragma unroll
            for (int i = 0; i < 4; i++)
                *reinterpret_cast<float4 *>(&T[srow + 32 * i][sc4]) = vs[i];
        };
        // eight k of the chunk: two halves of four, each with 8-byte operand reads (16-byte reads would
        // hold 16 operand registers where 8 do, and the kernel has none to spare)
        auto group = [&](int buf, int g) {
#pragma unroll
            for (int hf = 0; hf < 2; hf++) {
                float2 fa[2], fb[2];
#pragma unroll
                for (int t = 0; t < 2; t++) {
                    fa[t] = *reinterpret_cast<const float2 *>(&As[buf][wr * 64 + t * 32 + lr][8 * g + 4 * lh + 2 * hf]);
                    fb[t] = *reinterpret_cast<const float2 *>(&Bs[buf][wc * 64 + t * 32 + lr][8 * g + 4 * lh + 2 * hf]);
                }
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const float xa[2] = { j == 0 ? fa[0].x : fa[0].y, j == 0 ? fa[1].x : fa[1].y };
                    const float xb[2] = { j == 0 ? fb[0].x : fb[0].y, j == 0 ? fb[1].x : fb[1].y };
#pragma unroll
                    for (int a = 0; a < 2; a++)
#pragma unroll
                        for (int b = 0; b < 2; b++)
                            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[a], xb[b], acc[a][b], 0, 0, 0);
                }
            }
        };
        __syncthreads();                    // the previous block's last MFMAs have read buffer (nk - 1) & 1
        fetch(A, i0, nA, ixa, 0);
        commit(As[0]);
        fetch(B, j0, nB, ixb, 0);
        commit(Bs[0]);
        __syncthreads();
        static_assert(KC == 32, "four groups of eight k per chunk");
        for (int c = 0; c < nk; c++) {
            const int buf = c & 1;
            const bool more = c + 1 < nk;
            // the next chunk's pieces travel through ONE set of staging registers: A's are requested before
            // the first group of MFMAs and stored after the second, B's requested then and stored after the
            // fourth (the other buffer's last readers passed the barrier of chunk c - 1)
            if (more)
                fetch(A, i0, nA, ixa, c + 1);
            group(buf, 0);
            group(buf, 1);
            if (more) {
                commit(As[buf ^ 1]);
                fetch(B, j0, nB, ixb, c + 1);
            }
            group(buf, 2);
            group(buf, 3);
            if (more)
                commit(Bs[buf ^ 1]);
            __syncthreads();
        }
        // distances of this block: element r of lane l of tile (a, b) is
        // (row = 32 a + (r & 3) + 8 (r >> 2) + 4 (l >> 5), col = 32 b + (l & 31)).
        // |a - b|^2 = |a|^2 + (|b|^2 - 2 a.b): for a fixed row the first term is a constant, so the top-2
        // bookkeeping runs on e = |b|^2 - 2 a.b and k_nn2_merge adds |a|^2 (and clamps at 0) at the very end --
        // the row norms stay out of this loop (read here, 32 per lane and block, each load was waited for
        // before the next could be issued: as long as the block's MFMAs).
        if constexpr (GATED) {
            // The lane's two columns keep their original row, norm and position in registers; a row's position is
            // one 16-byte LDS read (two addresses per wave: a broadcast), 32 per lane and block.  A candidate is
            // pushed under its ORIGINAL index, so ties do not depend on the row order.
            int cj[2];
            float cn[2];
            float4 cp[2];
            bool cin[2];
#pragma unroll
            for (int b = 0; b < 2; b++) {
                const int c = wc * 64 + b * 32 + lr;
                cj[b] = g.idxB[pb * NT + c];
                cin[b] = j0 + c < nB;
                cn[b] = normB[cj[b]];
                cp[b] = g.posB[cj[b]];
            }
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const float4 pa = g.posAs[wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh];
#pragma unroll
                    for (int b = 0; b < 2; b++) {
                        const float e = cn[b] - 2.0f * acc[a][b][r];
                        if (cin[b] && nn2_gate(pa, cp[b], g.r2))
                            top2_push(best[a][r], e, cj[b]);
                    }
                }
        } else {
#pragma unroll
            for (int b = 0; b < 2; b++) {
                const int col = j0 + wc * 64 + b * 32 + lr;
                const float nb = col < nB ? normB[col] : 0.0f;
#pragma unroll
                for (int a = 0; a < 2; a++)
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const float e = nb - 2.0f * acc[a][b][r];
                        if (col < nB)
                            top2_push(best[a][r], e, col);
                    }
            }
        }
    }
    // merge over the 32 lanes that hold the same row (same lane >> 5), then over the two waves
    // that cover the two column halves
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            Top2 t = best[a][r];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) {
                const float d1 = __shfl_xor(t.d1, o, 64), d2 = __shfl_xor(t.d2, o, 64);
                const int j1 = __shfl_xor(t.j1, o, 64);
                top2_merge(t, d1, d2, j1);
            }
            if (lr == 0) {
                const int row = wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                red_d1[row][wc] = t.d1;
                red_d2[row][wc] = t.d2;
                red_j[row][wc] = t.j1;
            }
        }
    __syncthreads();
    if (tid < MT && i0 + tid < nA) {
        Top2 t;
        t.d1 = red_d1[tid][0]; t.d2 = red_d2[tid][0]; t.j1 = red_j[tid][0];
        top2_merge(t, red_d1[tid][1], red_d2[tid][1], red_j[tid][1]);
        const int o = GATED ? g.idxA[tid] : i0 + tid;       // (GATED: block row -> original row)
        out_j[o] = t.j1;                    // (0x7fffffff: none; k_nn2_merge / the launcher's final pass turn it into -1)
        out_d1[o] = t.d1;
        out_d2[o] = t.d2;
    }
    if constexpr (GATED) {
        // (ordinary vector atomics; a run past the end of B holds no block)
        if (tid == 0 && g.visited) {
            atomicAdd(&g.visited[0], (unsigned long long)nvis);
            atomicAdd(&g.visited[1], (unsigned long long)(jhi > jlo ? (jhi - jlo + NT - 1) / NT : 0));
        }
    }
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_nn2(const float *__restrict__ A, int nA, const float *__restrict__ B,
                                             int nB, int dim, const float *__restrict__ normA,
                                             const float *__restrict__ normB, int jb_per_split,
                                             int *__restrict__ out_j, float *__restrict__ out_d1,
                                             float *__restrict__ out_d2)
{
    nn2_block<false>(A, nA, B, nB, dim, normB, jb_per_split, out_j, out_d1, out_d2, Nn2Gate{});
}

// The gated search's workgroup: k_nn2's plus 3.5 KB of LDS (80 384 B: two workgroups still share a CU's 160 KiB).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_nn2_gated(const float *__restrict__ A, int nA, const float *__restrict__ B,
                                             int nB, int dim, const float *__restrict__ normB, int jb_per_split,
                                             int *__restrict__ out_j, float *__restrict__ out_d1,
                                             float *__restrict__ out_d2, Nn2Gate g)
{
    __shared__ float4 posAs[MT];
    __shared__ int idxA[MT], idxB[2 * NT];
    g.posAs = posAs;
    g.idxA = idxA;
    g.idxB = idxB;
    nn2_block<true>(A, nA, B, nB, dim, normB, jb_per_split, out_j, out_d1, out_d2, g);
}

// Box of every 128-row block of a set in its row order: block b covers rows perm[128 b ..].  fminf / fmaxf drop
// NaNs, and a point with a NaN coordinate stays out altogether (its gate is false against everything); a block
// without a finite point gets lo = +inf, hi = -inf, which is farther than any finite radius from every box.
__global__ __launch_bounds__(128) void k_block_boxes(const float4 *__restrict__ pos, const int *__restrict__ perm,
                                                     int n, float *__restrict__ box)
{
    __shared__ float red[2][6];
    const int tid = threadIdx.x, r = blockIdx.x * 128 + tid;
    float v[6] = { __builtin_inff(), __builtin_inff(), __builtin_inff(),
                   -__builtin_inff(), -__builtin_inff(), -__builtin_inff() };
    if (r < n) {
        const float4 p = pos[perm ? perm[r] : r];
        if (p.x == p.x && p.y == p.y && p.z == p.z) {
            v[0] = v[3] = p.x;
            v[1] = v[4] = p.y;
            v[2] = v[5] = p.z;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            v[k] = fminf(v[k], __shfl_xor(v[k], o, 64));
            v[3 + k] = fmaxf(v[3 + k], __shfl_xor(v[3 + k], o, 64));
        }
    if ((tid & 63) == 0)
#pragma unroll
        for (int k = 0; k < 6; k++)
            red[tid >> 6][k] = v[k];
    __syncthreads();
    if (tid < 3) {
        box[8 * (size_t)blockIdx.x + tid] = fminf(red[0][tid], red[1][tid]);
        box[8 * (size_t)blockIdx.x + 4 + tid] = fmaxf(red[0][3 + tid], red[1][3 + tid]);
    } else if (tid == 3) {
        box[8 * (size_t)blockIdx.x + 3] = box[8 * (size_t)blockIdx.x + 7] = 0.0f;
    }
}

// Top-2 of a row = merge of its top-2 over the runs of B (lexicographic ties: the result does not
// depend on how B was cut), then e -> |a - b|^2 = max(|a|^2 + e, 0) (clamped: cancellation for near-identical
// descriptors).
__global__ __launch_bounds__(256) void k_nn2_merge(const int *__restrict__ pj, const float *__restrict__ pd1,
                                                   const float *__restrict__ pd2, int nsplit, int nA,
                                                   const float *__restrict__ normA, int *__restrict__ out_j,
                                                   float *__restrict__ out_d1, float *__restrict__ out_d2)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nA)
        return;
    Top2 t;
    t.d1 = pd1[i]; t.d2 = pd2[i]; t.j1 = pj[i];
    for (int s = 1; s < nsplit; s++)
        top2_merge(t, pd1[(size_t)s * nA + i], pd2[(size_t)s * nA + i], pj[(size_t)s * nA + i]);
    const float na = normA[i];
    out_j[i] = t.j1 == 0x7fffffff ? -1 : t.j1;
    out_d1[i] = fmaxf(na + t.d1, 0.0f);
    out_d2[i] = fmaxf(na + t.d2, 0.0f);
}

// runs of B per row block of A: enough workgroups to fill the device several times over (a 128-row
// block of A against ALL of B is one long workgroup, and 40 000 descriptors are only 317 of them)
static int nn2_splits(int nA, int nB)
{
    const int nblkA = (nA + MT - 1) / MT, nblkB = (nB + NT - 1) / NT;
    int s = nblkA > 0 ? (2048 + nblkA - 1) / nblkA : 1;
    if (s > 16) s = 16;
    if (s > nblkB) s = nblkB;
    return s < 1 ? 1 : s;
}

extern "C" {

size_t sift3d_hip_nn2_work_floats(int nA, int nB)
{
    const size_t a = (size_t)(nA > 0 ? nA : 0), b = (size_t)(nB > 0 ? nB : 0);
    return a + b + 8 + 3 * a * (size_t)nn2_splits(nA, nB);
}

int sift3d_hip_nn2(const float *d_A, int nA, const float *d_B, int nB, int dim, int *d_j1, float *d_d1,
                   float *d_d2, float *d_work, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!d_A || !d_B || !d_j1 || !d_d1 || !d_d2 || !d_work || nA < 0 || nB < 0 || dim < KC || (dim % KC) ||
        (((uintptr_t)d_A | (uintptr_t)d_B) & 15))
        return launch_fail("sift3d_hip_nn2", "invalid arguments");
    if (!nA)
        return SIFT3D_SUCCESS;
    float *nrmA = d_work, *nrmB = d_work + nA;
    hipLaunchKernelGGL(k_row_norms, dim3((nA + 3) / 4), dim3(256), 0, st, d_A, nA, dim, nrmA);
    if (nB)
        hipLaunchKernelGGL(k_row_norms, dim3((nB + 3) / 4), dim3(256), 0, st, d_B, nB, dim, nrmB);
    {
        const int ns = nn2_splits(nA, nB), nblkB = (nB + NT - 1) / NT;
        const int per = ns > 0 ? (nblkB + ns - 1) / ns : 0;
        // partial results: three slices of ns * nA after the norms (the index slice holds ints)
        float *part = d_work + nA + nB + 8;
        int *pj = reinterpret_cast<int *>(part);
        float *pd1 = part + (size_t)ns * nA, *pd2 = part + 2 * (size_t)ns * nA;
        hipLaunchKernelGGL(k_nn2, dim3((nA + MT - 1) / MT, ns), dim3(256), 0, st, d_A, nA, d_B, nB, dim, nrmA,
                           nrmB, per > 0 ? per : 1, pj, pd1, pd2);
        hipLaunchKernelGGL(k_nn2_merge, dim3((nA + 255) / 256), dim3(256), 0, st, pj, pd1, pd2, ns, nA, nrmA, d_j1,
                           d_d1, d_d2);
    }
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

// the norms and partial slices of sift3d_hip_nn2, then the boxes: 8 floats per 128-row block of A and of B
size_t sift3d_hip_nn2_gated_work_floats(int nA, int nB)
{
    const size_t a = (size_t)(nA > 0 ? nA : 0), b = (size_t)(nB > 0 ? nB : 0);
    return sift3d_hip_nn2_work_floats(nA, nB) + 8 * ((a + MT - 1) / MT + (b + NT - 1) / NT);
}

int sift3d_hip_nn2_gated(const float *d_A, int nA, const float *d_B, int nB, int dim, const float *d_posA,
                         const float *d_posB, float r2, const int *d_permA, const int *d_permB, int *d_j1,
                         float *d_d1, float *d_d2, unsigned long long *d_visited, float *d_work, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!d_A || !d_B || !d_j1 || !d_d1 || !d_d2 || !d_work || nA < 0 || nB < 0 || dim < KC || (dim % KC) ||
        (((uintptr_t)d_A | (uintptr_t)d_B) & 15) || !d_posA || !d_posB ||
        (((uintptr_t)d_posA | (uintptr_t)d_posB) & 15) || !(r2 >= 0.0f))
        return launch_fail("sift3d_hip_nn2_gated", "invalid arguments");
    if (d_visited && hipMemsetAsync(d_visited, 0, 2 * sizeof(unsigned long long), st) != hipSuccess)
        return launch_fail("sift3d_hip_nn2_gated", "hipMemsetAsync failed");
    if (!nA)
        return SIFT3D_SUCCESS;
    {
        const int ns = nn2_splits(nA, nB), nblkA = (nA + MT - 1) / MT, nblkB = (nB + NT - 1) / NT;
        const int per = ns > 0 ? (nblkB + ns - 1) / ns : 0;
        float *nrmA = d_work, *nrmB = d_work + nA, *part = d_work + nA + nB + 8;
        int *pj = reinterpret_cast<int *>(part);
        float *pd1 = part + (size_t)ns * nA, *pd2 = part + 2 * (size_t)ns * nA;
        float *boxA = part + 3 * (size_t)ns * nA, *boxB = boxA + 8 * (size_t)nblkA;
        Nn2Gate g = {};
        g.posA = reinterpret_cast<const float4 *>(d_posA);
        g.posB = reinterpret_cast<const float4 *>(d_posB);
        g.permA = d_permA;
        g.permB = d_permB;
        g.boxA = boxA;
        g.boxB = boxB;
        g.visited = d_visited;
        g.r2 = r2;
        hipLaunchKernelGGL(k_row_norms, dim3((nA + 3) / 4), dim3(256), 0, st, d_A, nA, dim, nrmA);
        hipLaunchKernelGGL(k_block_boxes, dim3(nblkA), dim3(128), 0, st, g.posA, d_permA, nA, boxA);
        if (nB) {
            hipLaunchKernelGGL(k_row_norms, dim3((nB + 3) / 4), dim3(256), 0, st, d_B, nB, dim, nrmB);
            hipLaunchKernelGGL(k_block_boxes, dim3(nblkB), dim3(128), 0, st, g.posB, d_permB, nB, boxB);
        }
        // (every workgroup writes its slice, whether or not it visits a block: the merge reads all of them)
        hipLaunchKernelGGL(k_nn2_gated, dim3(nblkA, ns), dim3(256), 0, st, d_A, nA, d_B, nB, dim, nrmB,
                           per > 0 ? per : 1, pj, pd1, pd2, g);
        hipLaunchKernelGGL(k_nn2_merge, dim3((nA + 255) / 256), dim3(256), 0, st, pj, pd1, pd2, ns, nA, nrmA, d_j1,
                           d_d1, d_d2);
    }
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

} // extern "C"
