/* sift3d_ffd_eval.h -- what sift3d_ffd.c hands to the launchers of sift3d_ffd.hip, sift3d_ffd_landmarks.hip and
 * sift3d_jacobian_penalty.hip: the descriptor of one FFD evaluation, the parts of it that a call runs, and every
 * launcher's prototype.  The host and the kernel units compile against these declarations, so a launcher and its caller
 * cannot disagree.  The launchers are not exported from the library; the host has checked every argument. */
#ifndef SIFT3D_FFD_EVAL_H
#define SIFT3D_FFD_EVAL_H

#include <stddef.h>

#include "sift3d_ffd_jac.h"
#include "sift3d_ffd_landmarks.h"

/* The parts of an evaluation, in the order they run.  The MSD entries run FFD_ALL (the bending entry only the two
 * bending parts); the MI driver runs FFD_BEND_VALUE per evaluation and the other three only where a step starts.
 * FFD_JAC_VALUE, FFD_JAC_GRAD (with a penalty only; one of the two): the penalty's record from the field, alone or with
 * S and its adjoint GJ.  They run after the image term, whose force buffer S takes over once Gc is formed.
 * FFD_LM_VALUE, FFD_LM_GRAD (with landmarks only; one of the two): the landmark record from the lattice, alone or with
 * the adjoint GL. */
enum { FFD_IMAGE = 1, FFD_BEND_VALUE = 2, FFD_BEND_GRAD = 4, FFD_COMBINE = 8, FFD_ALL = 15, FFD_JAC_VALUE = 16,
       FFD_JAC_GRAD = 32, FFD_LM_VALUE = 64, FFD_LM_GRAD = 128 };

/* what the MI force needs beside the MSD force's arguments (header, "Mutual-information free-form deformation") */
typedef struct {
    int bins;
    float lo_f, s_f, lo_m, hi_m;                 /* s_f: the fixed bin's scale (parzen_check) */
    const double *d_W;                           /* [bins][bins] */
} sift3d_ffd_mi;

typedef struct {
    const float *d_F, *d_M;                      /* nc >= 1: stacks of nc channels; not read without FFD_IMAGE */
    int ox, oy, oz, nx, ny, nz;
    int nc;                                      /* 0: single volumes (k_ffd_force, k_ffd_mi_force); >= 1:
                                                    k_ffd_force_channels (mi == NULL) */
    const float *d_WF, *d_WM;                    /* the masks or NULL; both NULL: the unmasked force kernels */
    const float *d_field;
    const float *d_lat;
    int gx, gy, gz, dx, dy, dz;
    const float *d_w;                            /* the weight tables [dx + dy + dz][4] */
    const double *stencils;                      /* [3][3][3] (host) */
    double bending;
    const sift3d_ffd_mi *mi;                     /* NULL: the MSD, whose combine has the factor 2 / n, not 1 / n */
    const sift3d_ffd_jac *jac;                   /* NULL: no penalty; the combine takes its term when weight > 0 */
    const sift3d_ffd_lm *lm;                     /* NULL: no landmarks; the combine takes their term when weight > 0 */
    double *d_rec;                               /* {uint64 n; double S_ee, R, gmax}, Gc, dR [3][gz][gy][gx] each */
    float *d_grad;
    double *d_work;                              /* behind the weight tables: see sift3d_ffd_evaluate_launch */
    void *stream;
} sift3d_ffd_eval;

#ifdef __cplusplus
extern "C" {
#endif

/* sift3d_ffd.hip */
int sift3d_ffd_field_launch(const char *fn, const float *d_lat, int gx, int gy, int gz, int dx, int dy, int dz,
                            const float *d_w, const double *A, int ox, int oy, int oz, float *d_field, void *stream);
int sift3d_ffd_evaluate_launch(const char *fn, unsigned parts, const sift3d_ffd_eval *e);
int sift3d_ffd_jacobian_gradient_launch(const char *fn, const float *d_field, int ox, int oy, int oz, int gx, int gy,
                                        int gz, int dx, int dy, int dz, const float *d_w, double ref, double *d_rec,
                                        double *d_GJ, double *d_work, void *stream);
int sift3d_ffd_step_launch(const float *d_c, const float *d_grad, float a, float *d_out, size_t n, void *stream);
int sift3d_ffd_refine2_launch(const float *d_c, int cx, int cy, int cz, float *d_f, int fx, int fy, int fz,
                              void *stream);
/* sift3d_ffd_landmarks.hip */
int sift3d_ffd_points_launch(const char *fn, const float *d_lat, int gx, int gy, int gz, int dx, int dy, int dz,
                             const double *A, const double *d_P, int m, double *d_T, void *stream);
int sift3d_ffd_landmarks_launch(const char *fn, const float *d_lat, int gx, int gy, int gz, int dx, int dy, int dz,
                                const sift3d_ffd_lm *lm, int adjoint, double *d_r, void *stream);
/* sift3d_jacobian_penalty.hip */
int sift3d_jacobian_penalty_launch(const char *fn, const float *d_field, int ox, int oy, int oz, double ref,
                                   double *d_rec, double *d_S, double *d_work, void *stream);

#ifdef __cplusplus
}
#endif

#endif
