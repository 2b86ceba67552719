/* sift3d_parzen.h -- the Parzen window of "Mutual-information affine refinement (Mattes)" (include/sift3d_amd.h): the
 * one statement of its arithmetic, compiled into the two kernels (sift3d_affine_refine.hip) and into the host
 * (sift3d_amd_parzen_window in sift3d_affine_refine.c), so that the three cannot drift apart.  Plain C and HIP; every
 * operation in double, in the header's order, unfused (both builds compile with -ffp-contract=off). */
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

#endif
