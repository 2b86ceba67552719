// lds_commit_forward.hip -- go / no-go for two changes to k_describe's commit, at the REAL bin
// addresses of 48 windows of the 128^3 lattice volume (desc_trace.py, as lds_f64_atomic.hip):
//   python3 profiles/microbench/desc_trace.py /tmp/desc_trace.bin
//   hipcc --offload-arch=gfx950 -O3 -o lds_commit_forward lds_commit_forward.hip && ./lds_commit_forward /tmp/desc_trace.bin
//
// Every wave takes one 64-voxel batch of the trace and commits it `iters` times into its two private
// histograms, 16 waves per CU, the kernel's rounds: round u of pass p adds voxel 32 p + u (half-wave 0) and
// 32 p + 16 + u (half-wave 1); commit lane = (cell corner, face vertex) in quads, as in the kernel.
//   RMW     the shipped dependent rounds: ds_read_b32, wait, add, ds_write_b32, the next read behind the write
//   FWD     the same with register forwarding: in a round in which BOTH half-waves' voxels have the bins of
//           their predecessors (every lane addresses the bin it addressed the round before) the previous
//           round's write and this round's read are skipped as one unit and the register carries the sum;
//           no carry across batches.  BRANCH: one scalar bit test and one branch per round; EXEC: no branch,
//           the pair is issued with EXEC = 0 in the skipped rounds
//   REC     the dependent rounds plus the 14 record-row stores of a batch (7 before each pass), as
//           ds_write_b32 (an address register each) or as ds_write_addtid_b32 (M0 + offset + 4 * lane)
// Reported as lds_f64_atomic.hip reports: shader cycles per 64 window voxels per CU.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define CHK(x) do{hipError_t e=(x); if(e!=hipSuccess){printf("err %s line %d\n", hipGetErrorString(e), __LINE__); exit(1);} }while(0)

__constant__ int c_boff[12];        // word offset of each vertex's 64-cell block

struct Rec { unsigned char cell, v0, v1, v2; };

constexpr int HIST = 832, RECW = 7 * 68;   // floats: one histogram; the record block (7 super-rows, 68 apart)

// MODE 0 RMW, 1 FWD by branch, 2 FWD by EXEC; REC 0 no record stores, 1 ds_write_b32, 2 ds_write_addtid_b32
template <int MODE, int REC_>
__global__ __launch_bounds__(256) void k_commit(const Rec *__restrict__ trace, int nbatch, int iters,
                                                float *__restrict__ out, long long *__restrict__ clk,
                                                unsigned *__restrict__ skipped)
{
    __shared__ float hist_[4][2 * HIST];
    __shared__ float rec_[4][RECW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *hist = hist_[wave];
    for (int i = lane; i < 2 * HIST; i += 64)
        hist[i] = 0.0f;
    __syncthreads();
    const int gw = blockIdx.x * 4 + wave;
    const Rec *b = trace + (size_t)((gw * 7919) % nbatch) * 64;
    const int half = lane >> 5, l5 = lane & 31;
    const int pc = l5 >> 2, pt = l5 & 3, pj = pt < 3 ? pt : 0;
    const int corner = ((pc >> 2) & 1) + 4 * ((pc >> 1) & 1) + 16 * (pc & 1);
    int addr[32];
    unsigned m = 0;
#pragma unroll
    for (int u = 0; u < 32; u++) {
        const Rec r = b[(u >> 4) * 32 + (u & 15) + 16 * half];
        const int vert = pj == 0 ? r.v0 : pj == 1 ? r.v1 : r.v2;
        addr[u] = (int)(size_t)(hist + half * HIST + c_boff[vert] + r.cell + corner);
        // every lane addresses the bin of the round before <=> both voxels repeat their predecessors' bins
        if (u > 0 && __ballot(addr[u] == addr[u - 1]) == ~0ull)
            m |= 1u << u;
    }
    m = (unsigned)__builtin_amdgcn_readfirstlane((int)m);
    const unsigned rec_m0 = (unsigned)__builtin_amdgcn_readfirstlane((int)(size_t)(rec_[wave]));
    const int rec_a = (int)rec_m0 + 4 * lane;
    const float val = 1.0f + lane;
    const long long t0 = clock64(), w0 = wall_clock64();
    for (int it = 0; it < iters; it++) {
        float x = 0.0f;
#pragma unroll
        for (int u = 0; u < 32; u++) {
            if (REC_ == 1 && (u & 15) == 0)
                asm volatile("ds_write_b32 %0, %1\n\tds_write_b32 %0, %1 offset:272\n\tds_write_b32 %0, %1 offset:544\n\t"
                             "ds_write_b32 %0, %1 offset:816\n\tds_write_b32 %0, %1 offset:1088\n\t"
                             "ds_write_b32 %0, %1 offset:1360\n\tds_write_b32 %0, %1 offset:1632" ::"v"(rec_a), "v"(val) : "memory");
            if (REC_ == 2 && (u & 15) == 0)
                asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tds_write_addtid_b32 %0\n\tds_write_addtid_b32 %0 offset:272\n\t"
                             "ds_write_addtid_b32 %0 offset:544\n\tds_write_addtid_b32 %0 offset:816\n\t"
                             "ds_write_addtid_b32 %0 offset:1088\n\tds_write_addtid_b32 %0 offset:1360\n\t"
                             "ds_write_addtid_b32 %0 offset:1632" ::"v"(val), "s"(rec_m0) : "m0", "memory");
            if (MODE == 0) {
                asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(x) : "v"(addr[u]) : "memory");
                x += val;
                asm volatile("ds_write_b32 %0, %1" ::"v"(addr[u]), "v"(x) : "memory");
            } else if (MODE == 1) {
                if (u == 0)
                    asm volatile("ds_read_b32 %0, %1" : "=v"(x) : "v"(addr[0]) : "memory");
                asm volatile("s_waitcnt lgkmcnt(0)\n\tv_add_f32 %0, %0, %1" : "+v"(x) : "v"(val) : "memory");
                if (u == 31)
                    asm volatile("ds_write_b32 %0, %1" ::"v"(addr[u]), "v"(x) : "memory");
                else if (!((m >> (u + 1)) & 1u))
                    asm volatile("ds_write_b32 %1, %0\n\tds_read_b32 %0, %2" : "+v"(x) : "v"(addr[u]), "v"(addr[(u + 1) & 31]) : "memory");
            } else {
                if (u == 0)
                    asm volatile("ds_read_b32 %0, %1" : "=v"(x) : "v"(addr[0]) : "memory");
                const unsigned long long em = (unsigned long long)(long long)((int)(u == 31 ? 0u : (m >> ((u + 1) & 31)) & 1u) - 1);
                if (u == 31)
                    asm volatile("s_waitcnt lgkmcnt(0)\n\tv_add_f32 %0, %0, %1\n\tds_write_b32 %2, %0" : "+v"(x) : "v"(val), "v"(addr[u]) : "memory");
                else
                    asm volatile("s_waitcnt lgkmcnt(0)\n\tv_add_f32 %0, %0, %1\n\ts_mov_b64 exec, %4\n\tds_write_b32 %2, %0\n\t"
                                 "ds_read_b32 %0, %3\n\ts_mov_b64 exec, -1"
                                 : "+v"(x) : "v"(val), "v"(addr[u]), "v"(addr[(u + 1) & 31]), "s"(em) : "memory");
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    const long long t1 = clock64(), w1 = wall_clock64();
    __syncthreads();
    float s = 0;
    for (int i = lane; i < 2 * HIST; i += 64)
        s += hist[i];
    for (int i = lane; i < RECW; i += 64)
        s += rec_[wave][i];
    out[blockIdx.x * 256 + threadIdx.x] = s;
    if (lane == 0) {
        clk[2 * gw] = t1 - t0;
        clk[2 * gw + 1] = w1 - w0;
        skipped[gw] = (unsigned)__popc(m);
    }
}

static int g_cus = 256;

template <typename F>
static double report(const char *name, F launch, long long *d_clk, int nblk, int iters)
{
    hipEvent_t e0, e1; CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
    float ms = 0;
    for (int rep = 0; rep < 2; rep++) {
        CHK(hipEventRecord(e0));
        launch();
        CHK(hipEventRecord(e1)); CHK(hipEventSynchronize(e1));
        CHK(hipEventElapsedTime(&ms, e0, e1));
    }
    std::vector<long long> clk(2 * nblk * 4);
    CHK(hipMemcpy(clk.data(), d_clk, clk.size() * sizeof(long long), hipMemcpyDeviceToHost));
    double sc = 0, wc = 0;
    for (int i = 0; i < nblk * 4; i++) { sc += (double)clk[2 * i]; wc += (double)clk[2 * i + 1]; }
    sc /= nblk * 4; wc /= nblk * 4;
    const double ghz = sc / (wc / 100e6) / 1e9;
    const double cyc = sc / iters / ((double)nblk * 4 / g_cus);
    printf("%-72s %8.3f ms  %7.1f cycles / 64 voxels / CU   clock %.3f GHz\n", name, ms, cyc, ghz);
    return cyc;
}

int main(int argc, char **argv)
{
    const char *path = argc > 1 ? argv[1] : "desc_trace.bin";
    FILE *f = fopen(path, "rb");
    if (!f) { printf("cannot open %s (run desc_trace.py first)\n", path); return 1; }
    int hdr[2];
    if (fread(hdr, 4, 2, f) != 2) return 1;
    std::vector<Rec> recs(hdr[0]);
    if (fread(recs.data(), 4, hdr[0], f) != (size_t)hdr[0]) return 1;
    fclose(f);
    const int nbatch = hdr[0] / 64;
    hipDeviceProp_t prop; CHK(hipGetDeviceProperties(&prop, 0)); g_cus = prop.multiProcessorCount;
    Rec *d_tr; CHK(hipMalloc(&d_tr, recs.size() * 4));
    CHK(hipMemcpy(d_tr, recs.data(), recs.size() * 4, hipMemcpyHostToDevice));
    const int nblk = g_cus * 4, iters = 500;      // 4 blocks of 4 waves per CU = 16 waves per CU
    float *d_o; CHK(hipMalloc(&d_o, (size_t)nblk * 256 * 4));
    long long *d_clk; CHK(hipMalloc(&d_clk, (size_t)nblk * 4 * 2 * 8));
    unsigned *d_sk; CHK(hipMalloc(&d_sk, (size_t)nblk * 4 * 4));
    static const int colour[12] = { 0, 1, 2, 3, 1, 0, 3, 2, 2, 3, 0, 1 };
    static const int shift[4] = { 0, 8, 18, 26 };
    int boff[12], rank = 0;
    for (int c = 0; c < 4; c++)
        for (int u = 0; u < 12; u++)
            if (colour[u] == c)
                boff[u] = 64 * rank++ + shift[c];
    CHK(hipMemcpyToSymbol(HIP_SYMBOL(c_boff), boff, sizeof(boff)));
#define RUN(M, R, name) report(name, [&] { hipLaunchKernelGGL((k_commit<M, R>), dim3(nblk), dim3(256), 0, 0, d_tr, nbatch, iters, d_o, d_clk, d_sk); }, d_clk, nblk, iters)
    printf("trace: %d window voxels, %d batches; 16 waves per CU, %d batches per wave\n", hdr[0], nbatch, iters);
    for (int rep = 0; rep < 2; rep++) {
        RUN(0, 0, "1  dependent rounds (shipped)");
        RUN(1, 0, "2a forwarding, one branch per round");
        RUN(2, 0, "2b forwarding, EXEC = 0 in skipped rounds");
        RUN(0, 1, "3a dependent rounds + 14 ds_write_b32 record stores");
        RUN(0, 2, "3b dependent rounds + 14 ds_write_addtid_b32 record stores");
    }
    std::vector<unsigned> sk(nblk * 4);
    CHK(hipMemcpy(sk.data(), d_sk, sk.size() * 4, hipMemcpyDeviceToHost));
    double tot = 0;
    for (unsigned v : sk) tot += v;
    printf("skipped rounds: %.1f %% of the rounds of the batches the waves took\n", 100.0 * tot / (32.0 * sk.size()));
    return 0;
}
