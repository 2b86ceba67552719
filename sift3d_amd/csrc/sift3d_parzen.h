/* sift3d_parzen.h -- the Parzen window of "Mutual-information affine refinement (Mattes)" (include/sift3d_amd.h): the
 * one statement of its arithmetic, compiled into the kernels (k_parzen_hist and k_affine_mi_normal in
 * sift3d_affine_refine.hip, k_ffd_mi_force in sift3d_ffd.hip) and into the host (sift3d_amd_parzen_window in
 * sift3d_affine_refine.c), so that they cannot drift apart.  Plain C and HIP; every operation in double, in the
 * header's order, unfused (both builds compile with -ffp-contract=off).  The kernels' arguments, the table in LDS and
 * psi, which the record kernel and the FFD's force share, are at the end (HIP only). */
#ifndef SIFT3D_PARZEN_H
#define SIFT3D_PARZEN_H

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define PARZEN_FN __host__ __device__ __forceinline__
#else
#define PARZEN_FN static inline
#endif

#define PARZEN_Q 65536.0                         /* 2^16: the fixed point of the histogram's weights */

/* the fixed volume's bin: "Similarity measures"' rule on (lo, s = (float) B / (hi - lo), B), float (written so that a
 * NaN, which finite volumes do not produce, takes bin 0 and converts nothing) */
PARZEN_FN int parzen_fixed_bin(float v, float lo, float s, int B)
{
    const float t = (v - lo) * s;
    return !(t >= 0.0f) ? 0 : t >= (float)B ? B - 1 : (int)t;
}

/* s_m = (double)(B - 3) / ((double) hi - (double) lo), once per call */
PARZEN_FN double parzen_scale(float lo, float hi, int B)
{
    return (double)(B - 3) / ((double)hi - (double)lo);
}

/* The window of the moving value m: the first of its four bins k0, the weights in fixed point q, the derivatives of the
 * weights by the bin coordinate dw, and whether m lies outside its range.  (A NaN clamps to t = 1 and is `out`.) */
PARZEN_FN void parzen_window(float m, float lo, double s, int B, int *k0, uint32_t q[4], double dw[4], int *out)
{
    const double top = (double)(B - 2);
    double t = 1.0 + ((double)m - (double)lo) * s;
    *out = !(t >= 1.0) || t > top;
    t = !(t >= 1.0) ? 1.0 : t > top ? top : t;
    {
        const int f = (int)floor(t) - 1;
        const int k = f < B - 4 ? f : B - 4;
        const double r = t - (double)(k + 1);
        const double u = 1.0 - r, t2 = r * r, t3 = t2 * r;
        const double w0 = ((u * u) * u) / 6.0;
        const double w1 = ((3.0 * t3 - 6.0 * t2) + 4.0) / 6.0;
        const double w2 = (((-3.0 * t3 + 3.0 * t2) + 3.0 * r) + 1.0) / 6.0;
        const double w3 = t3 / 6.0;
        *k0 = k;
        q[0] = (uint32_t)llrint(w0 * PARZEN_Q);
        q[1] = (uint32_t)llrint(w1 * PARZEN_Q);
        q[2] = (uint32_t)llrint(w2 * PARZEN_Q);
        q[3] = (uint32_t)llrint(w3 * PARZEN_Q);
        dw[0] = -(u * u) / 2.0;
        dw[1] = (3.0 * t2 - 4.0 * r) / 2.0;
        dw[2] = ((-3.0 * t2 + 2.0 * r) + 1.0) / 2.0;
        dw[3] = t2 / 2.0;
    }
}

#ifdef __HIPCC__
/* what a kernel needs of the two histograms' binning, and the table of the record pass and of the FFD's force */
struct ParzenArgs {
    int bins;
    float lo_f, s_f, lo_m;                       /* s_f: "Similarity measures"' float scale of the fixed bin */
    double s_m;                                  /* parzen_scale(lo_m, hi_m, bins) */
    const double *W;                             /* [bins][bins] on the device; the histogram pass does not read it */
};

static inline ParzenArgs parzen_args(int bins, float lo_f, float s_f, float lo_m, float hi_m, const double *d_W)
{
    return ParzenArgs{bins, lo_f, s_f, lo_m, parzen_scale(lo_m, hi_m, bins), d_W};
}

/* W into the workgroup's LDS (bins * bins doubles), once per workgroup; every lane calls it */
__device__ __forceinline__ const double *parzen_table(const ParzenArgs &z, double *lds)
{
    for (int i = threadIdx.x; i < z.bins * z.bins; i += 256)
        lds[i] = z.W[i];
    __syncthreads();
    return lds;
}

/* psi = s_m * sum_k dw[k] W[b_f][k0 + k] for the fixed value f and the moving value m, W being parzen_table's; *out:
 * m lies outside the moving range (the caller takes psi = counted && !out ? value : 0) */
__device__ __forceinline__ double parzen_psi(const ParzenArgs &z, const double *W, float f, float m, int *out)
{
    int k0;
    uint32_t q[4];
    double dw[4];
    parzen_window(m, z.lo_m, z.s_m, z.bins, &k0, q, dw, out);
    const double *w = W + parzen_fixed_bin(f, z.lo_f, z.s_f, z.bins) * z.bins + k0;             /* k0 + 3 <= B - 1 */
    return z.s_m * (((dw[0] * w[0] + dw[1] * w[1]) + dw[2] * w[2]) + dw[3] * w[3]);
}
#endif

#endif
