/* sift3d_ffd_jac.h -- the Jacobian penalty's share of an FFD evaluation (include/sift3d_amd.h, "Jacobian penalty"), as
 * sift3d_ffd.c hands it to the launchers of sift3d_ffd.hip.  NULL in its place: an evaluation without the penalty. */
#ifndef SIFT3D_FFD_JAC_H
#define SIFT3D_FFD_JAC_H

typedef struct {
    double weight;                               /* > 0: the third term of the gradient is formed; 0: the record alone */
    double ref;
    double *d_rec;                               /* SIFT3D_AMD_JACOBIAN_PENALTY_RECORD_BYTES */
    double *d_GJ;                                /* [3][gz][gy][gx] of the finest level */
    double *d_work;                              /* sift3d_amd_jacobian_penalty_work_bytes() of the finest level */
} sift3d_ffd_jac;

#endif
