// sift3d_ffd_landmarks.hip -- the cubic B-spline free-form deformation at POINTS: the map of a list of points through a
// control lattice, and the landmark (matched-point) term of the FFD drivers: the residuals T(P) - Q with their weighted
// sum of squares, and the adjoint of the point evaluation over the control points.
// Contract: include/sift3d_amd.h, "FFD landmarks"; restated in numpy by tests/ffd_landmarks_restatement.py
// (tests/test_ffd_landmarks.py).  The host checks, the ordering of the landmarks and the driver are in sift3d_ffd.c.
//
//   - nothing is sampled from a volume: sift3d_resample.h is included for pull / pull_row (the header's q) and for
//     workgroup_reduce / finish_reduce only;
//   - k_ffd_points, k_ffd_lm_value: one lane per point.  Per axis the cell and the four weights in double, then per
//     channel the contract's 64 terms one by one (3 multiplies and an add each, unfused): 576 double operations and 192
//     lattice loads (L1 / L2 hits: neighbouring landmarks are neighbours in cell order) per point.  The value pass keeps
//     the weights and the residual of every landmark for the adjoint, [row][m] so that a wave's stores are contiguous,
//     and reduces S, Omega and rmax as the other sum kernels do: workgroup_reduce into one slot per workgroup of a grid
//     that depends on the number of counted landmarks only, then finish_reduce (k_ffd_lm_finish);
//   - k_ffd_lm_adjoint GATHERS: one lane per control point visits the at most 64 cells whose points it weighs, in
//     ascending (k0, j0, i0), and each cell's run of landmarks in ascending order (the host's stable counting sort), and
//     carries the three channels' sums in registers: per landmark three multiplies for the coefficient and a multiply
//     and an add per channel, seven loads that the lanes of neighbouring controls share.  No atomics and nothing staged
//     through LDS; the order is a function of the points and the lattice shape only.
#include "sift3d_resample.h"
#include "sift3d_ffd_eval.h"

namespace {

struct LmLattice {
    const float *c;                              // [3][gz][gy][gx]
    int gx, gy, gz, dx, dy, dz;
};

// One axis of a point: v = x / delta, i0 = floor(v), t = v - i0 and the four weights of sift3d_amd_ffd_weights at t,
// left in double.  false (and i0 = 0) where the coordinate is not finite or i0 is outside [0, g - 4].
__device__ __forceinline__ bool lm_axis(double x, int delta, int g, int &i0, double (&w)[4])
{
    const double v = x / (double)delta, f = floor(v);
    const bool in = f >= 0.0 && f <= (double)(g - 4);                   // a NaN or an infinity fails one of the two
    i0 = in ? (int)f : 0;
    const double t = in ? v - (double)i0 : 0.0;
    const double u = 1.0 - t, t2 = t * t, t3 = t2 * t;
    w[0] = ((u * u) * u) / 6.0;
    w[1] = ((3.0 * t3 - 6.0 * t2) + 4.0) / 6.0;
    w[2] = (((-3.0 * t3 + 3.0 * t2) + 3.0 * t) + 1.0) / 6.0;
    w[3] = t3 / 6.0;
    return in;
}

// s = sum_c sum_b sum_a wz[c] * (wy[b] * (wx[a] * (double) c[k0 + c][j0 + b][i0 + a])), x innermost, from +0
__device__ __forceinline__ double lm_spline(const float *c, int gx, int gy, int i0, int j0, int k0, const double (&wx)[4],
                                            const double (&wy)[4], const double (&wz)[4])
{
    double s = 0.0;
#pragma unroll
    for (int cc = 0; cc < 4; cc++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const float *row = c + ((size_t)(k0 + cc) * (size_t)gy + (size_t)(j0 + b)) * (size_t)gx + (size_t)i0;
#pragma unroll
            for (int a = 0; a < 4; a++)
                s = s + wz[cc] * (wy[b] * (wx[a] * (double)row[a]));
        }
    return s;
}

template <bool AFFINE>
__device__ __forceinline__ double lm_pull(const double *a, int d, double x, double y, double z)
{
    return AFFINE ? pull(a + 4 * d, x, pull_row(a + 4 * d, y, z)) : d == 0 ? x : d == 1 ? y : z;
}

struct LmPointsArgs {
    double a[12];
    LmLattice l;
    const double *P;                             // [m][3]
    double *T;                                   // [m][3]
    int m;
};

template <bool AFFINE>
__global__ __launch_bounds__(256) void k_ffd_points(const LmPointsArgs s)
{
    const LmLattice &l = s.l;
    const size_t cvox = (size_t)l.gx * (size_t)l.gy * (size_t)l.gz;
    for (int i = (int)(blockIdx.x * 256 + threadIdx.x); i < s.m; i += (int)(gridDim.x * 256)) {
        const double x = s.P[3 * (size_t)i], y = s.P[3 * (size_t)i + 1], z = s.P[3 * (size_t)i + 2];
        double wx[4], wy[4], wz[4];
        int i0, j0, k0;
        const bool ix = lm_axis(x, l.dx, l.gx, i0, wx), iy = lm_axis(y, l.dy, l.gy, j0, wy);
        const bool in = lm_axis(z, l.dz, l.gz, k0, wz) && ix && iy;
#pragma unroll 1
        for (int d = 0; d < 3; d++) {
            const double t = lm_pull<AFFINE>(s.a, d, x, y, z) + lm_spline(l.c + (size_t)d * cvox, l.gx, l.gy, i0, j0, k0,
                                                                          wx, wy, wz);
            s.T[3 * (size_t)i + d] = in ? t : __builtin_nan("");
        }
    }
}

struct LmValueArgs {
    double a[12];
    LmLattice l;
    const double *lm;                            // [7][m]: Px, Py, Pz, Qx, Qy, Qz, w
    double *wt;                                  // [12][m]
    double *r;                                   // [3][m]
    const unsigned *orig;                        // [m]
    double *d_r;                                 // [m][3] in the caller's order, cleared by the host; or null
    double *part;                                // [3][SIFT3D_FFD_LM_GRID]
    int n, m;
};

// Every landmark here is inside (the host's test is lm_axis' on the same doubles).
template <bool AFFINE>
__global__ __launch_bounds__(256) void k_ffd_lm_value(const LmValueArgs s)
{
    __shared__ double slot_s[4], slot_o[4], slot_m[4];
    const LmLattice &l = s.l;
    const size_t cvox = (size_t)l.gx * (size_t)l.gy * (size_t)l.gz, m = (size_t)s.m;
    double S = 0.0, Om = 0.0, mx = 0.0;
    for (int i = (int)(blockIdx.x * 256 + threadIdx.x); i < s.n; i += (int)(gridDim.x * 256)) {
        const double x = s.lm[i], y = s.lm[m + i], z = s.lm[2 * m + i], om = s.lm[6 * m + i];
        double wx[4], wy[4], wz[4], r[3];
        int i0, j0, k0;
        lm_axis(x, l.dx, l.gx, i0, wx);
        lm_axis(y, l.dy, l.gy, j0, wy);
        lm_axis(z, l.dz, l.gz, k0, wz);
#pragma unroll
        for (int a = 0; a < 4; a++) {
            s.wt[(size_t)a * m + i] = wx[a];
            s.wt[(size_t)(4 + a) * m + i] = wy[a];
            s.wt[(size_t)(8 + a) * m + i] = wz[a];
        }
#pragma unroll
        for (int d = 0; d < 3; d++) {
            const double t = lm_pull<AFFINE>(s.a, d, x, y, z) + lm_spline(l.c + (size_t)d * cvox, l.gx, l.gy, i0, j0, k0,
                                                                          wx, wy, wz);
            r[d] = t - s.lm[(size_t)(3 + d) * m + i];
            s.r[(size_t)d * m + i] = r[d];
        }
        if (s.d_r) {
            double *o = s.d_r + 3 * (size_t)s.orig[i];
            o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
        }
        const double ss = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
        S = S + om * ss;
        Om = Om + om;
        mx = fmax(mx, sqrt(ss));
    }
    const double rs = workgroup_reduce<Add>(S, slot_s), ro = workgroup_reduce<Add>(Om, slot_o);
    const double rm = workgroup_reduce<Max>(mx, slot_m);
    if (threadIdx.x == 0) {
        s.part[blockIdx.x] = rs;
        s.part[SIFT3D_FFD_LM_GRID + blockIdx.x] = ro;
        s.part[2 * SIFT3D_FFD_LM_GRID + blockIdx.x] = rm;
    }
}

// one workgroup: the record {uint64 counted; double S, Omega, rmax} from the n slots of each statistic
__global__ __launch_bounds__(256) void k_ffd_lm_finish(const double *part, unsigned n, unsigned long long counted,
                                                       double *rec)
{
    __shared__ double s_red[256];
    const double S = finish_reduce<Add>(part, n, s_red);
    __syncthreads();
    const double Om = finish_reduce<Add>(part + SIFT3D_FFD_LM_GRID, n, s_red);
    __syncthreads();
    const double mx = finish_reduce<Max>(part + 2 * SIFT3D_FFD_LM_GRID, n, s_red);
    if (threadIdx.x == 0) {
        reinterpret_cast<unsigned long long *>(rec)[0] = counted;
        rec[1] = S;
        rec[2] = Om;
        rec[3] = mx;
    }
}

struct LmAdjArgs {
    const double *om;                            // [m]: the weights of the landmarks, in cell order
    const double *wt;                            // [12][m]
    const double *r;                             // [3][m]
    const unsigned *start;                       // [cells + 1]
    double *GL;                                  // [3][gz][gy][gx]
    int gx, gy, gz, m;
};

// GL_d[k][j][i] = sum over the cells (k0, j0, i0), k - 3 <= k0 <= k and so on, inside the lattice's support, ascending,
// and over each cell's landmarks, ascending, of (om * ((wz[k - k0] * wy[j - j0]) * wx[i - i0])) * r_d, from +0
__global__ __launch_bounds__(256) void k_ffd_lm_adjoint(const LmAdjArgs s)
{
    const size_t cvox = (size_t)s.gx * (size_t)s.gy * (size_t)s.gz, m = (size_t)s.m;
    const int cx = s.gx - 3, cy = s.gy - 3, cz = s.gz - 3;
    const double *r0 = s.r, *r1 = s.r + m, *r2 = s.r + 2 * m;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < cvox; idx += (size_t)gridDim.x * 256) {
        const int i = (int)(idx % (size_t)s.gx), j = (int)(idx / (size_t)s.gx % (size_t)s.gy);
        const int k = (int)(idx / ((size_t)s.gx * (size_t)s.gy));
        double g0 = 0.0, g1 = 0.0, g2 = 0.0;
        for (int k0 = max(0, k - 3); k0 <= min(k, cz - 1); k0++) {
            const double *wz = s.wt + (size_t)(8 + k - k0) * m;
            for (int j0 = max(0, j - 3); j0 <= min(j, cy - 1); j0++) {
                const double *wy = s.wt + (size_t)(4 + j - j0) * m;
                for (int i0 = max(0, i - 3); i0 <= min(i, cx - 1); i0++) {
                    const double *wx = s.wt + (size_t)(i - i0) * m;
                    const size_t cell = ((size_t)k0 * (size_t)cy + (size_t)j0) * (size_t)cx + (size_t)i0;
                    const unsigned end = s.start[cell + 1];
                    for (unsigned q = s.start[cell]; q < end; q++) {
                        const double coef = s.om[q] * ((wz[q] * wy[q]) * wx[q]);
                        g0 = g0 + coef * r0[q];
                        g1 = g1 + coef * r1[q];
                        g2 = g2 + coef * r2[q];
                    }
                }
            }
        }
        s.GL[idx] = g0;
        s.GL[cvox + idx] = g1;
        s.GL[2 * cvox + idx] = g2;
    }
}

unsigned lm_grid(size_t total, unsigned cap)
{
    const size_t b = (total + 255) / 256;
    return (unsigned)(b < 1 ? 1 : b < cap ? b : cap);
}

} // namespace

// Launchers for sift3d_ffd.c, which has checked every argument (not exported from the library).
extern "C" int sift3d_ffd_points_launch(const char *fn, const float *d_lat, int gx, int gy, int gz, int dx, int dy,
                                        int dz, const double *A, const double *d_P, int m, double *d_T, void *stream)
{
    LmPointsArgs s;
    for (int i = 0; i < 12; i++)
        s.a[i] = A ? A[i] : 0.0;
    s.l = LmLattice{d_lat, gx, gy, gz, dx, dy, dz};
    s.P = d_P;
    s.T = d_T;
    s.m = m;
    void (*k)(const LmPointsArgs) = A ? k_ffd_points<true> : k_ffd_points<false>;
    hipLaunchKernelGGL(k, dim3(lm_grid((size_t)m, SIFT3D_FFD_LM_GRID)), dim3(256), 0, (hipStream_t)stream, s);
    LAUNCH_CHECK();
    return SIFT3D_SUCCESS;
}

// The value pass of the level's landmarks at d_lat into lm->d_rec (and d_r, cleared by the caller, when given); with
// `adjoint` GL into lm->d_GL from the weights and residuals the value pass has just left in lm->d_work.
extern "C" int sift3d_ffd_landmarks_launch(const char *fn, const float *d_lat, int gx, int gy, int gz, int dx, int dy,
                                           int dz, const sift3d_ffd_lm *lm, int adjoint, double *d_r, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const size_t m = (size_t)lm->m;
    double *part = (double *)lm->d_work, *rows = part + 3 * SIFT3D_FFD_LM_GRID;
    double *wt = rows + 7 * m, *r = wt + 12 * m;
    const unsigned *orig = (const unsigned *)(r + 3 * m), *start = orig + m;
    unsigned slots = 0;
    if (lm->n > 0) {
        LmValueArgs s;
        for (int i = 0; i < 12; i++)
            s.a[i] = lm->A ? lm->A[i] : 0.0;
        s.l = LmLattice{d_lat, gx, gy, gz, dx, dy, dz};
        s.lm = rows;
        s.wt = wt;
        s.r = r;
        s.orig = orig;
        s.d_r = d_r;
        s.part = part;
        s.n = lm->n;
        s.m = lm->m;
        slots = lm_grid((size_t)lm->n, SIFT3D_FFD_LM_GRID);
        void (*k)(const LmValueArgs) = lm->A ? k_ffd_lm_value<true> : k_ffd_lm_value<false>;
        hipLaunchKernelGGL(k, dim3(slots), dim3(256), 0, st, s);
        LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_ffd_lm_finish, dim3(1), dim3(256), 0, st, (const double *)part, slots,
                       (unsigned long long)lm->n, lm->d_rec);
    LAUNCH_CHECK();
    if (adjoint) {
        const LmAdjArgs a = {rows + 6 * m, wt, r, start, lm->d_GL, gx, gy, gz, lm->m};
        hipLaunchKernelGGL(k_ffd_lm_adjoint, dim3(lm_grid((size_t)gx * gy * gz, MAX_GRID)), dim3(256), 0, st, a);
        LAUNCH_CHECK();
    }
    return SIFT3D_SUCCESS;
}
