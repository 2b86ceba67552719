/* sift3d_ffd_landmarks.h -- the landmark term's share of an FFD evaluation (include/sift3d_amd.h, "FFD landmarks"), as
 * sift3d_ffd.c hands it to the launchers of sift3d_ffd.hip and sift3d_ffd_landmarks.hip, and the layout of its work
 * buffer, which the host fills and the kernels read.  NULL in its place: an evaluation without landmarks. */
#ifndef SIFT3D_FFD_LANDMARKS_H
#define SIFT3D_FFD_LANDMARKS_H

#include <stddef.h>

/* workgroups (and partial slots per statistic) of the value pass, at most: a function of nothing, so that the order of
 * the sums depends on the number of counted landmarks only */
#define SIFT3D_FFD_LM_GRID 128

/* d_work, doubles first:
 *   part [3][SIFT3D_FFD_LM_GRID]   the value pass' partial S, Omega, rmax
 *   lm   [7][m]                    Px, Py, Pz, Qx, Qy, Qz, w of the counted landmarks in cell order (host)
 *   wt   [12][m]                   their point weights wx[4], wy[4], wz[4] (value pass)
 *   r    [3][m]                    their residuals (value pass)
 * then 32-bit words:
 *   orig  [m]                      the caller's index of each counted landmark (host)
 *   start [cells + 1]              the first landmark of each cell (k0, j0, i0), i0 fastest; cells = (gx - 3)(gy - 3)
 *                                  (gz - 3) (host)
 * Only the first n entries of each row of m are used. */
static inline size_t sift3d_ffd_lm_doubles(size_t m)
{
    return 3 * (size_t)SIFT3D_FFD_LM_GRID + 22 * m;
}

typedef struct {
    double weight;                               /* lambda; > 0: the third (fourth) term of the gradient is formed */
    double scale;                                /* 2 * 4^l on level l: the gradient's factor is (weight * scale) / Omega */
    const double *A;                             /* the level's pull map (host, 12 doubles) or NULL */
    int n;                                       /* the landmarks inside the level's lattice */
    int m;                                       /* the caller's m: the rows of the work buffer */
    double *d_rec;                               /* SIFT3D_AMD_FFD_LANDMARKS_RECORD_BYTES */
    double *d_GL;                                /* [3][gz][gy][gx] of the level */
    void *d_work;                                /* sift3d_amd_ffd_landmarks_work_bytes() of the finest level */
} sift3d_ffd_lm;

#endif
