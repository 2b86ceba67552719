/* sift3d_ffd.c -- cubic B-spline free-form deformation: the weight table and the stencils on the host, the checked
 * device entries (field export, evaluation with gradient, bending energy, subdivision) and the steepest-descent driver
 * (included at the end of sift3d_host.c, after sift3d_affine_refine.c).
 *
 * The contract is in include/sift3d_amd.h, "B-spline free-form deformation" (the MSD) and "Mutual-information free-form
 * deformation (Mattes)": two metrics, one evaluation entry body and one driver loop over either.  The kernels are in
 * sift3d_ffd.hip (the histogram pass in sift3d_affine_refine.hip), reached through the launchers of sift3d_ffd_eval.h
 * after the checks here.  Arguments are checked before the device is touched, so bad input is refused on a machine
 * without a GPU too.
 *
 * The Jacobian penalty (header, "Jacobian penalty"; kernels in sift3d_jacobian_penalty.hip) has its checked entry here
 * and is the optional third term of the driver's cost.
 *
 * "Multi-channel free-form deformation": the same entry body and the same driver loop over stacks of nc channels, the
 * driver's levels supplied by the caller instead of restricted here.
 *
 * "FFD landmarks" (kernels in sift3d_ffd_landmarks.hip): the spline at points, the landmark record with its residuals
 * and adjoint, whose landmarks the host puts in cell order, and the optional last term of the driver's cost. */
#include <stddef.h>

#include "sift3d_ffd_eval.h"

int sift3d_amd_ffd_lattice_dim(int o, int delta)
{
    return o <= 0 || delta <= 0 ? 0 : (o - 1) / delta + 4;
}

int sift3d_amd_ffd_weights(int delta, float *w)
{
    int r;
    if (!w || delta <= 0 || delta > SIFT3D_AMD_FFD_MAX_SPACING)
        return refuse("sift3d_amd_ffd_weights", "NULL table or spacing outside [1, SIFT3D_AMD_FFD_MAX_SPACING]");
    for (r = 0; r < delta; r++) {
        const double t = (double)r / (double)delta, u = 1.0 - t, t2 = t * t, t3 = t2 * t;
        w[4 * r + 0] = (float)(((u * u) * u) / 6.0);
        w[4 * r + 1] = (float)(((3.0 * t3 - 6.0 * t2) + 4.0) / 6.0);
        w[4 * r + 2] = (float)((((-3.0 * t3 + 3.0 * t2) + 3.0 * t) + 1.0) / 6.0);
        w[4 * r + 3] = (float)(t3 / 6.0);
    }
    return SIFT3D_SUCCESS;
}

/* st[axis][order][tap] of the bending energy */
static void ffd_stencils(const int *delta, double *st)
{
    int a;
    for (a = 0; a < 3; a++) {
        const double d = (double)delta[a];
        double *s = st + 9 * a;
        s[0] = 1.0 / 6.0; s[1] = 4.0 / 6.0; s[2] = 1.0 / 6.0;
        s[3] = -0.5 / d; s[4] = 0.0; s[5] = 0.5 / d;
        s[6] = 1.0 / (d * d); s[7] = -2.0 / (d * d); s[8] = 1.0 / (d * d);
    }
}

static int ffd_spacing_ok(int dx, int dy, int dz)
{
    return dx >= 1 && dy >= 1 && dz >= 1 && dx <= SIFT3D_AMD_FFD_MAX_SPACING && dy <= SIFT3D_AMD_FFD_MAX_SPACING &&
           dz <= SIFT3D_AMD_FFD_MAX_SPACING;
}

static int check_ffd_lattice(const char *what, int ox, int oy, int oz, int gx, int gy, int gz, int dx, int dy, int dz)
{
    if (check_dims(what, ox, oy, oz))
        return SIFT3D_FAILURE;
    if (!ffd_spacing_ok(dx, dy, dz))
        return refuse(what, "the spacing must be in [1, SIFT3D_AMD_FFD_MAX_SPACING]");
    if (gx != sift3d_amd_ffd_lattice_dim(ox, dx) || gy != sift3d_amd_ffd_lattice_dim(oy, dy) ||
        gz != sift3d_amd_ffd_lattice_dim(oz, dz))
        return refuse(what, "the lattice is not (o - 1) / spacing + 4 along every axis");
    return SIFT3D_SUCCESS;
}

static size_t ffd_weights_bytes(int dx, int dy, int dz)
{
    return ((size_t)dx + dy + dz) * 4 * sizeof(float);
}

/* the three tables to d_w, x then y then z (the copy is staged by the runtime before the call returns) */
static int ffd_upload_weights(int dx, int dy, int dz, float *d_w, void *stream)
{
    float w[3 * 4 * SIFT3D_AMD_FFD_MAX_SPACING];
    sift3d_amd_ffd_weights(dx, w);
    sift3d_amd_ffd_weights(dy, w + 4 * dx);
    sift3d_amd_ffd_weights(dz, w + 4 * (dx + dy));
    return sift3d_hip_memcpy_h2d(d_w, w, ffd_weights_bytes(dx, dy, dz), stream);
}

size_t sift3d_amd_ffd_field_work_bytes(int dx, int dy, int dz)
{
    return ffd_spacing_ok(dx, dy, dz) ? ffd_weights_bytes(dx, dy, dz) : 0;
}

int sift3d_hip_ffd_field(const float *d_lattice, int gx, int gy, int gz, int dx, int dy, int dz, const double *A,
                         int ox, int oy, int oz, float *d_field, void *d_work, void *stream)
{
    static const char what[] = "sift3d_hip_ffd_field";
    if (!d_lattice || !d_field || !d_work)
        return refuse(what, "NULL argument");
    if (check_ffd_lattice(what, ox, oy, oz, gx, gy, gz, dx, dy, dz) || (A && check_affine(what, A)) ||
        check_aligned(what, 0, ADDR(d_lattice) | ADDR(d_field) | ADDR(d_work)))
        return SIFT3D_FAILURE;
    if (ADDR(d_work) & 15)
        return refuse(what, "a buffer is misaligned");
    {
        const range_t in[] = { { d_lattice, image_bytes(gx, gy, gz, 3) } };
        const range_t out[] = { { d_field, field_bytes(ox, oy, oz) }, { d_work, ffd_weights_bytes(dx, dy, dz) } };
        if (ranges_aliased(out, 2, in, 1))
            return refuse(what, ALIASED);
    }
    if (ffd_upload_weights(dx, dy, dz, (float *)d_work, stream))
        return SIFT3D_FAILURE;
    return sift3d_ffd_field_launch(what, d_lattice, gx, gy, gz, dx, dy, dz, (const float *)d_work, A, ox, oy, oz,
                                   d_field, stream);
}

/* ---- evaluation ---- */

static size_t pad16(size_t bytes)
{
    return (bytes + 15) & ~(size_t)15;
}

size_t sift3d_amd_ffd_record_bytes(int gx, int gy, int gz)
{
    if (gx < 4 || gy < 4 || gz < 4)
        return 0;
    return SIFT3D_AMD_FFD_RECORD_HEAD_BYTES + 2 * 3 * grid_voxels(gx, gy, gz) * sizeof(double);
}

/* doubles of the evaluation's scratch behind the weight tables: partial slots, force, the two intermediate arrays of
 * the adjoint, the second derivatives */
static size_t ffd_eval_doubles(int ox, int oy, int oz, int gx, int gy, int gz)
{
    return 2 * (size_t)SIFT3D_AMD_SIMILARITY_GRID + 3 * grid_voxels(ox, oy, oz) + 3 * grid_voxels(ox, oy, gz) +
           3 * grid_voxels(ox, gy, gz) + 18 * grid_voxels(gx - 2, gy - 2, gz - 2);
}

size_t sift3d_amd_ffd_evaluate_work_bytes(int ox, int oy, int oz, int dx, int dy, int dz)
{
    if (ox <= 0 || oy <= 0 || oz <= 0 || !ffd_spacing_ok(dx, dy, dz))
        return 0;
    return pad16(ffd_weights_bytes(dx, dy, dz)) +
           ffd_eval_doubles(ox, oy, oz, sift3d_amd_ffd_lattice_dim(ox, dx), sift3d_amd_ffd_lattice_dim(oy, dy),
                            sift3d_amd_ffd_lattice_dim(oz, dz)) * sizeof(double);
}

/* the landmarks of an evaluation (defined with the landmark entries below) */
struct ffd_lm_host_s;
static int ffd_lm_prepare(struct ffd_lm_host_s *h, sift3d_ffd_lm *lm, int gx, int gy, int gz, const int *d, double scale,
                          void *stream);

/* bins, the two ranges and the table of an MI evaluation */
typedef struct {
    int bins;
    float lo_f, hi_f, lo_m, hi_m;
    const double *d_W;
} ffd_mi_args;

/* The parts (sift3d_ffd_eval.h) of the evaluation e.  value: the bending value; gradient: the image term, the bending
 * gradient and the combined gradient.  The MSD evaluates with both; the MI driver with the value per evaluation and the
 * gradient where a step starts.  A penalty and landmarks that e names run with either: their gradient pass where a
 * gradient is formed and their weight is > 0, else their record alone. */
static unsigned ffd_parts(const sift3d_ffd_eval *e, int value, int gradient)
{
    const unsigned jac = !e->jac ? 0u : gradient && e->jac->weight > 0.0 ? FFD_JAC_GRAD : FFD_JAC_VALUE;
    const unsigned lm = !e->lm ? 0u : gradient && e->lm->weight > 0.0 ? FFD_LM_GRAD : FFD_LM_VALUE;
    return (value ? FFD_BEND_VALUE : 0u) | (gradient ? FFD_IMAGE | FFD_BEND_GRAD | FFD_COMBINE : 0u) | jac | lm;
}

/* what an entry has beside sift3d_hip_ffd_evaluate's arguments; all zero: nothing */
typedef struct {
    const float *d_WF, *d_WM;                    /* the masks ("Masks") or NULL */
    const ffd_mi_args *mi;                       /* the MI evaluation's further arguments, checked after the FFD
                                                    entries' own, or NULL (the MSD) */
    int nc;                                      /* 0 (one volume each, the single-channel kernels) or the channels of
                                                    the stacks d_F and d_M (the channels entry, which has checked it) */
    const sift3d_ffd_jac *jac;                   /* the penalty or NULL (the landmarks entry only) */
    struct ffd_lm_host_s *lmh;                   /* the landmarks entry, which has checked them and their buffers (else
                                                    NULL): the host side of the landmark term, */
    sift3d_ffd_lm *lm;                           /* and the term */
} ffd_entry_opts;

/* the shared body of the evaluation entries */
static int ffd_evaluate_entry(const char *what, const float *d_F, int ox, int oy, int oz, const float *d_M, int nx,
                              int ny, int nz, const float *d_lattice, int gx, int gy, int gz, int dx, int dy, int dz,
                              const double *A, double bending, float *d_field, void *d_record, float *d_grad,
                              void *d_work, void *stream, const ffd_entry_opts *o)
{
    const float *d_WF = o->d_WF, *d_WM = o->d_WM;
    const ffd_mi_args *mi = o->mi;
    const int ch = o->nc ? o->nc : 1;
    sift3d_ffd_mi z;
    sift3d_ffd_eval e;
    int delta[3];
    double st[27];
    float s_f = 0.0f;
    if (!d_F || !d_M || !d_lattice || !d_field || !d_record || !d_grad || !d_work || (mi && !mi->d_W))
        return refuse(what, "NULL argument");
    if (check_ffd_lattice(what, ox, oy, oz, gx, gy, gz, dx, dy, dz) || check_dims(what, nx, ny, nz) ||
        (A && check_affine(what, A)))
        return SIFT3D_FAILURE;
    if (!isfinite(bending) || bending < 0)
        return refuse(what, "the bending weight must be finite and not negative");
    if (check_aligned(what, ADDR(d_record), ADDR(d_F) | ADDR(d_M) | ADDR(d_lattice) | ADDR(d_field) | ADDR(d_grad) |
                                                ADDR(d_WF) | ADDR(d_WM)))
        return SIFT3D_FAILURE;
    if (ADDR(d_work) & 15)
        return refuse(what, "a buffer is misaligned");
    if (mi && (parzen_check(what, mi->bins, mi->lo_f, mi->hi_f, mi->lo_m, mi->hi_m, &s_f) ||
               check_aligned(what, ADDR(mi->d_W), 0)))
        return SIFT3D_FAILURE;
    {
        const range_t in[] = { { d_F, image_bytes(ox, oy, oz, ch) }, { d_M, image_bytes(nx, ny, nz, ch) },
                               { d_lattice, image_bytes(gx, gy, gz, 3) },
                               { d_WF, d_WF ? image_bytes(ox, oy, oz, 1) : 0 },
                               { d_WM, d_WM ? image_bytes(nx, ny, nz, 1) : 0 },
                               { mi ? mi->d_W : NULL, mi ? (size_t)mi->bins * mi->bins * sizeof(double) : 0 } };
        const range_t out[] = { { d_field, field_bytes(ox, oy, oz) },
                                { d_record, sift3d_amd_ffd_record_bytes(gx, gy, gz) },
                                { d_grad, image_bytes(gx, gy, gz, 3) },
                                { d_work, sift3d_amd_ffd_evaluate_work_bytes(ox, oy, oz, dx, dy, dz) } };
        if (ranges_aliased(out, 4, in, 6))
            return refuse(what, ALIASED);
    }
    delta[0] = dx; delta[1] = dy; delta[2] = dz;
    ffd_stencils(delta, st);
    if (ffd_upload_weights(dx, dy, dz, (float *)d_work, stream) ||
        sift3d_ffd_field_launch(what, d_lattice, gx, gy, gz, dx, dy, dz, (const float *)d_work, A, ox, oy, oz, d_field,
                                stream) ||
        (o->lm && ffd_lm_prepare(o->lmh, o->lm, gx, gy, gz, delta, 1.0, stream)))
        return SIFT3D_FAILURE;
    if (mi)
        z = (sift3d_ffd_mi){ mi->bins, mi->lo_f, s_f, mi->lo_m, mi->hi_m, mi->d_W };
    e = (sift3d_ffd_eval){ .d_F = d_F, .d_M = d_M, .ox = ox, .oy = oy, .oz = oz, .nx = nx, .ny = ny, .nz = nz,
                           .nc = o->nc, .d_WF = d_WF, .d_WM = d_WM, .d_field = d_field, .d_lat = d_lattice, .gx = gx,
                           .gy = gy, .gz = gz, .dx = dx, .dy = dy, .dz = dz, .d_w = (const float *)d_work,
                           .stencils = st, .bending = bending, .mi = mi ? &z : NULL, .jac = o->jac, .lm = o->lm,
                           .d_rec = (double *)d_record, .d_grad = d_grad,
                           .d_work = (double *)((char *)d_work + pad16(ffd_weights_bytes(dx, dy, dz))),
                           .stream = stream };
    return sift3d_ffd_evaluate_launch(what, ffd_parts(&e, 1, 1), &e);
}

int sift3d_hip_ffd_evaluate(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                            const float *d_lattice, int gx, int gy, int gz, int dx, int dy, int dz, const double *A,
                            double bending, float *d_field, void *d_record, float *d_grad, void *d_work, void *stream)
{
    const ffd_entry_opts o = { .nc = 0 };
    return ffd_evaluate_entry("sift3d_hip_ffd_evaluate", d_F, ox, oy, oz, d_M, nx, ny, nz, d_lattice, gx, gy, gz, dx,
                              dy, dz, A, bending, d_field, d_record, d_grad, d_work, stream, &o);
}

int sift3d_hip_ffd_evaluate_masked(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                   const float *d_lattice, int gx, int gy, int gz, int dx, int dy, int dz,
                                   const double *A, double bending, float *d_field, void *d_record, float *d_grad,
                                   void *d_work, void *stream, const float *d_WF, const float *d_WM)
{
    const ffd_entry_opts o = { .d_WF = d_WF, .d_WM = d_WM };
    return ffd_evaluate_entry("sift3d_hip_ffd_evaluate_masked", d_F, ox, oy, oz, d_M, nx, ny, nz, d_lattice, gx, gy,
                              gz, dx, dy, dz, A, bending, d_field, d_record, d_grad, d_work, stream, &o);
}

/* one force volume whatever nc is: the single-channel evaluation's work */
size_t sift3d_amd_ffd_evaluate_channels_work_bytes(int ox, int oy, int oz, int dx, int dy, int dz)
{
    return sift3d_amd_ffd_evaluate_work_bytes(ox, oy, oz, dx, dy, dz);
}

int sift3d_hip_ffd_evaluate_channels(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                     int nc, const float *d_lattice, int gx, int gy, int gz, int dx, int dy, int dz,
                                     const double *A, double bending, float *d_field, void *d_record, float *d_grad,
                                     void *d_work, void *stream, const float *d_WF, const float *d_WM)
{
    static const char what[] = "sift3d_hip_ffd_evaluate_channels";
    const ffd_entry_opts o = { .d_WF = d_WF, .d_WM = d_WM, .nc = nc };
    if (check_channels(what, nc))
        return SIFT3D_FAILURE;
    return ffd_evaluate_entry(what, d_F, ox, oy, oz, d_M, nx, ny, nz, d_lattice, gx, gy, gz, dx, dy, dz, A, bending,
                              d_field, d_record, d_grad, d_work, stream, &o);
}

int sift3d_hip_ffd_mi_evaluate(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                               const float *d_lattice, int gx, int gy, int gz, int dx, int dy, int dz, const double *A,
                               double bending, float *d_field, void *d_record, float *d_grad, void *d_work,
                               void *stream, const float *d_WF, const float *d_WM, int bins, float lo_f, float hi_f,
                               float lo_m, float hi_m, const double *d_W)
{
    const ffd_mi_args mi = { bins, lo_f, hi_f, lo_m, hi_m, d_W };
    const ffd_entry_opts o = { .d_WF = d_WF, .d_WM = d_WM, .mi = &mi };
    return ffd_evaluate_entry("sift3d_hip_ffd_mi_evaluate", d_F, ox, oy, oz, d_M, nx, ny, nz, d_lattice, gx, gy, gz, dx,
                              dy, dz, A, bending, d_field, d_record, d_grad, d_work, stream, &o);
}

size_t sift3d_amd_ffd_bending_work_bytes(int gx, int gy, int gz)
{
    if (gx < 4 || gy < 4 || gz < 4)
        return 0;
    return (2 * (size_t)SIFT3D_AMD_SIMILARITY_GRID + 18 * grid_voxels(gx - 2, gy - 2, gz - 2)) * sizeof(double);
}

int sift3d_hip_ffd_bending(const float *d_lattice, int gx, int gy, int gz, int dx, int dy, int dz, void *d_record,
                           void *d_work, void *stream)
{
    static const char what[] = "sift3d_hip_ffd_bending";
    sift3d_ffd_eval e;
    int delta[3];
    double st[27];
    if (!d_lattice || !d_record || !d_work)
        return refuse(what, "NULL argument");
    if (gx < 4 || gy < 4 || gz < 4)
        return refuse(what, "a lattice has at least 4 control points along every axis");
    if (!ffd_spacing_ok(dx, dy, dz))
        return refuse(what, "the spacing must be in [1, SIFT3D_AMD_FFD_MAX_SPACING]");
    if (check_aligned(what, ADDR(d_record) | ADDR(d_work), ADDR(d_lattice)))
        return SIFT3D_FAILURE;
    {
        const range_t in[] = { { d_lattice, image_bytes(gx, gy, gz, 3) } };
        const range_t out[] = { { d_record, sift3d_amd_ffd_record_bytes(gx, gy, gz) },
                                { d_work, sift3d_amd_ffd_bending_work_bytes(gx, gy, gz) } };
        if (ranges_aliased(out, 2, in, 1))
            return refuse(what, ALIASED);
    }
    delta[0] = dx; delta[1] = dy; delta[2] = dz;
    ffd_stencils(delta, st);
    /* the launcher's scratch layout with an empty image grid: slots, then D */
    e = (sift3d_ffd_eval){ .d_lat = d_lattice, .gx = gx, .gy = gy, .gz = gz, .dx = dx, .dy = dy, .dz = dz, .stencils = st,
                           .d_rec = (double *)d_record, .d_work = (double *)d_work, .stream = stream };
    return sift3d_ffd_evaluate_launch(what, FFD_BEND_VALUE | FFD_BEND_GRAD, &e);
}

int sift3d_hip_ffd_refine2(const float *d_coarse, int ox, int oy, int oz, int dx, int dy, int dz, float *d_fine,
                           void *stream)
{
    static const char what[] = "sift3d_hip_ffd_refine2";
    int cx, cy, cz, fx, fy, fz;
    if (!d_coarse || !d_fine)
        return refuse(what, "NULL argument");
    if (check_dims(what, ox, oy, oz))
        return SIFT3D_FAILURE;
    if (!ffd_spacing_ok(dx, dy, dz))
        return refuse(what, "the spacing must be in [1, SIFT3D_AMD_FFD_MAX_SPACING]");
    if (check_aligned(what, 0, ADDR(d_coarse) | ADDR(d_fine)))
        return SIFT3D_FAILURE;
    cx = sift3d_amd_ffd_lattice_dim(multires_half(ox), dx);
    cy = sift3d_amd_ffd_lattice_dim(multires_half(oy), dy);
    cz = sift3d_amd_ffd_lattice_dim(multires_half(oz), dz);
    fx = sift3d_amd_ffd_lattice_dim(ox, dx);
    fy = sift3d_amd_ffd_lattice_dim(oy, dy);
    fz = sift3d_amd_ffd_lattice_dim(oz, dz);
    {
        const range_t in[] = { { d_coarse, image_bytes(cx, cy, cz, 3) } };
        const range_t out[] = { { d_fine, image_bytes(fx, fy, fz, 3) } };
        if (ranges_aliased(out, 1, in, 1))
            return refuse(what, ALIASED);
    }
    return sift3d_ffd_refine2_launch(d_coarse, cx, cy, cz, d_fine, fx, fy, fz, stream);
}

/* ---- Jacobian penalty of a field ---- */

size_t sift3d_amd_jacobian_penalty_work_bytes(int ox, int oy, int oz)
{
    if (ox <= 0 || oy <= 0 || oz <= 0)
        return 0;
    return (4 * (size_t)SIFT3D_AMD_SIMILARITY_GRID + grid_voxels(ox, oy, oz)) * sizeof(double);
}

int sift3d_hip_jacobian_penalty(const float *d_field, int ox, int oy, int oz, double ref, void *d_record, double *d_grad,
                                void *d_work, void *stream)
{
    static const char what[] = "sift3d_hip_jacobian_penalty";
    if (!d_field || !d_record || !d_work)
        return refuse(what, "NULL argument");
    if (check_dims(what, ox, oy, oz))
        return SIFT3D_FAILURE;
    if (!isfinite(ref) || ref == 0.0)
        return refuse(what, "the reference determinant must be finite and not 0");
    if (check_aligned(what, ADDR(d_record) | ADDR(d_grad) | ADDR(d_work), ADDR(d_field)))
        return SIFT3D_FAILURE;
    {
        const range_t in[] = { { d_field, field_bytes(ox, oy, oz) } };
        const range_t out[] = { { d_record, SIFT3D_AMD_JACOBIAN_PENALTY_RECORD_BYTES },
                                { d_work, sift3d_amd_jacobian_penalty_work_bytes(ox, oy, oz) },
                                { d_grad, d_grad ? 3 * grid_voxels(ox, oy, oz) * sizeof(double) : 0 } };
        if (ranges_aliased(out, 3, in, 1))
            return refuse(what, ALIASED);
    }
    return sift3d_jacobian_penalty_launch(what, d_field, ox, oy, oz, ref, (double *)d_record, d_grad, (double *)d_work,
                                          stream);
}

/* the weight tables, S and the adjoint's two intermediate arrays, then the penalty's work */
static size_t ffd_jacobian_gradient_doubles(int ox, int oy, int oz, int gy, int gz)
{
    return 3 * grid_voxels(ox, oy, oz) + 3 * grid_voxels(ox, oy, gz) + 3 * grid_voxels(ox, gy, gz);
}

size_t sift3d_amd_ffd_jacobian_gradient_work_bytes(int ox, int oy, int oz, int dx, int dy, int dz)
{
    if (ox <= 0 || oy <= 0 || oz <= 0 || !ffd_spacing_ok(dx, dy, dz))
        return 0;
    return pad16(ffd_weights_bytes(dx, dy, dz)) +
           ffd_jacobian_gradient_doubles(ox, oy, oz, sift3d_amd_ffd_lattice_dim(oy, dy),
                                         sift3d_amd_ffd_lattice_dim(oz, dz)) * sizeof(double) +
           sift3d_amd_jacobian_penalty_work_bytes(ox, oy, oz);
}

int sift3d_hip_ffd_jacobian_gradient(const float *d_field, int ox, int oy, int oz, int dx, int dy, int dz, double ref,
                                     void *d_record, double *d_GJ, void *d_work, void *stream)
{
    static const char what[] = "sift3d_hip_ffd_jacobian_gradient";
    int gx, gy, gz;
    if (!d_field || !d_record || !d_GJ || !d_work)
        return refuse(what, "NULL argument");
    if (check_dims(what, ox, oy, oz))
        return SIFT3D_FAILURE;
    if (!ffd_spacing_ok(dx, dy, dz))
        return refuse(what, "the spacing must be in [1, SIFT3D_AMD_FFD_MAX_SPACING]");
    if (!isfinite(ref) || ref == 0.0)
        return refuse(what, "the reference determinant must be finite and not 0");
    if (check_aligned(what, ADDR(d_record) | ADDR(d_GJ), ADDR(d_field)))
        return SIFT3D_FAILURE;
    if (ADDR(d_work) & 15)
        return refuse(what, "a buffer is misaligned");
    gx = sift3d_amd_ffd_lattice_dim(ox, dx);
    gy = sift3d_amd_ffd_lattice_dim(oy, dy);
    gz = sift3d_amd_ffd_lattice_dim(oz, dz);
    {
        const range_t in[] = { { d_field, field_bytes(ox, oy, oz) } };
        const range_t out[] = { { d_record, SIFT3D_AMD_JACOBIAN_PENALTY_RECORD_BYTES },
                                { d_GJ, 3 * grid_voxels(gx, gy, gz) * sizeof(double) },
                                { d_work, sift3d_amd_ffd_jacobian_gradient_work_bytes(ox, oy, oz, dx, dy, dz) } };
        if (ranges_aliased(out, 3, in, 1))
            return refuse(what, ALIASED);
    }
    if (ffd_upload_weights(dx, dy, dz, (float *)d_work, stream))
        return SIFT3D_FAILURE;
    return sift3d_ffd_jacobian_gradient_launch(what, d_field, ox, oy, oz, gx, gy, gz, dx, dy, dz, (const float *)d_work,
                                               ref, (double *)d_record, d_GJ,
                                               (double *)((char *)d_work + pad16(ffd_weights_bytes(dx, dy, dz))),
                                               stream);
}

/* ---- points and landmarks ("FFD landmarks") ---- */

int sift3d_hip_ffd_points(const float *d_lattice, int gx, int gy, int gz, int dx, int dy, int dz, const double *A,
                          const double *d_P, int m, double *d_T, void *stream)
{
    static const char what[] = "sift3d_hip_ffd_points";
    if (!d_lattice || !d_P || !d_T)
        return refuse(what, "NULL argument");
    if (gx < 4 || gy < 4 || gz < 4)
        return refuse(what, "a lattice has at least 4 control points along every axis");
    if (!ffd_spacing_ok(dx, dy, dz))
        return refuse(what, "the spacing must be in [1, SIFT3D_AMD_FFD_MAX_SPACING]");
    if (m < 1)
        return refuse(what, "the number of points must be positive");
    if ((A && check_affine(what, A)) || check_aligned(what, ADDR(d_P) | ADDR(d_T), ADDR(d_lattice)))
        return SIFT3D_FAILURE;
    {
        const range_t in[] = { { d_lattice, image_bytes(gx, gy, gz, 3) }, { d_P, (size_t)m * 3 * sizeof(double) } };
        const range_t out[] = { { d_T, (size_t)m * 3 * sizeof(double) } };
        if (ranges_aliased(out, 1, in, 2))
            return refuse(what, ALIASED);
    }
    return sift3d_ffd_points_launch(what, d_lattice, gx, gy, gz, dx, dy, dz, A, d_P, m, d_T, stream);
}

size_t sift3d_amd_ffd_landmarks_work_bytes(int m, int gx, int gy, int gz)
{
    if (m < 1 || m > SIFT3D_AMD_FFD_MAX_LANDMARKS || gx < 4 || gy < 4 || gz < 4)
        return 0;
    return pad16(sift3d_ffd_lm_doubles((size_t)m) * sizeof(double) +
                 ((size_t)m + grid_voxels(gx - 3, gy - 3, gz - 3) + 1) * sizeof(uint32_t));
}

size_t sift3d_amd_ffd_landmarks_struct_bytes(int which)
{
    return which == 0   ? sizeof(sift3d_amd_ffd_landmark_term)
           : which == 1 ? (size_t)SIFT3D_AMD_FFD_LANDMARKS_RECORD_BYTES
           : which == 2 ? (size_t)SIFT3D_AMD_FFD_MAX_LANDMARKS
           : which == 3 ? (size_t)SIFT3D_AMD_FFD_MAX_TRAIL
                        : 0;
}

/* the caller's landmarks and the host's staging of one level's: the rows of the work buffer that the host fills
 * (sift3d_ffd_landmarks.h), one allocation */
typedef struct ffd_lm_host_s {
    const double *P, *Q, *w;                     /* w may be NULL: all 1 */
    int m;
    double weight;                               /* the driver's lambda */
    sift3d_amd_ffd_landmark_term *out;           /* the driver's array parallel to the trail */
    double up;                                   /* the driver's 2^l on level l */
    double *rows;                                /* [7][m] */
    uint32_t *orig, *start, *cell;               /* [m], [cells + 1] of the finest lattice, [m] */
} ffd_lm_host;

static int check_landmarks(const char *what, const double *P, const double *Q, const double *w, int m)
{
    int i;
    if (!P || !Q)
        return refuse(what, "NULL argument");
    if (m < 1 || m > SIFT3D_AMD_FFD_MAX_LANDMARKS)
        return refuse(what, "the number of landmarks must be in [1, SIFT3D_AMD_FFD_MAX_LANDMARKS]");
    for (i = 0; i < 3 * m; i++)
        if (!isfinite(Q[i]))
            return refuse(what, "a moving landmark is not finite");
    for (i = 0; w && i < m; i++)
        if (!isfinite(w[i]) || w[i] < 0)
            return refuse(what, "a landmark weight must be finite and not negative");
    return SIFT3D_SUCCESS;
}

/* cells: those of the finest lattice the staging is used with */
static int ffd_lm_host_alloc(const char *what, ffd_lm_host *h, size_t cells)
{
    const size_t m = (size_t)h->m;
    h->rows = (double *)calloc(7 * m * sizeof(double) + (2 * m + cells + 1) * sizeof(uint32_t), 1);
    if (!h->rows)
        return refuse(what, "out of host memory");
    h->orig = (uint32_t *)(h->rows + 7 * m);
    h->start = h->orig + m;
    h->cell = h->start + cells + 1;
    return SIFT3D_SUCCESS;
}

/* the point rule of one axis: 1 and the cell where the coordinate is finite and 0 <= floor(x / delta) <= g - 4 */
static int ffd_lm_axis(double x, int delta, int g, uint32_t *i0)
{
    const double f = floor(x / (double)delta);
    if (!(f >= 0.0 && f <= (double)(g - 4)))
        return 0;
    *i0 = (uint32_t)f;
    return 1;
}

/* One level's landmarks to lm->d_work: P and Q times `scale` (a power of two: exact), the inside test on the lattice
 * (gx, gy, gz) at spacing d, a stable counting sort by cell (k0, j0, i0), i0 fastest, and the copies (staged by the
 * runtime before the call returns, as the weight tables').  lm->n leaves with the number inside. */
static int ffd_lm_prepare(ffd_lm_host *h, sift3d_ffd_lm *lm, int gx, int gy, int gz, const int *d, double scale,
                          void *stream)
{
    const size_t m = (size_t)h->m, cells = grid_voxels(gx - 3, gy - 3, gz - 3);
    double *dev_rows = (double *)lm->d_work + 3 * (size_t)SIFT3D_FFD_LM_GRID;
    uint32_t *dev_orig = (uint32_t *)(dev_rows + 22 * m);
    size_t i, c;
    memset(h->start, 0, (cells + 1) * sizeof(uint32_t));
    for (i = 0; i < m; i++) {
        uint32_t i0, j0, k0;
        if (ffd_lm_axis(h->P[3 * i] * scale, d[0], gx, &i0) && ffd_lm_axis(h->P[3 * i + 1] * scale, d[1], gy, &j0) &&
            ffd_lm_axis(h->P[3 * i + 2] * scale, d[2], gz, &k0)) {
            h->cell[i] = (uint32_t)(((size_t)k0 * (size_t)(gy - 3) + j0) * (size_t)(gx - 3) + i0);
            h->start[h->cell[i] + 1]++;
        } else
            h->cell[i] = UINT32_MAX;
    }
    for (c = 0; c < cells; c++)
        h->start[c + 1] += h->start[c];
    lm->n = (int)h->start[cells];
    for (i = 0; i < m; i++) {                                /* start[c] runs up to the end of cell c ... */
        int k;
        uint32_t pos;
        if (h->cell[i] == UINT32_MAX)
            continue;
        pos = h->start[h->cell[i]]++;
        for (k = 0; k < 3; k++) {
            h->rows[(size_t)k * m + pos] = h->P[3 * i + k] * scale;
            h->rows[(size_t)(3 + k) * m + pos] = h->Q[3 * i + k] * scale;
        }
        h->rows[6 * m + pos] = h->w ? h->w[i] : 1.0;
        h->orig[pos] = (uint32_t)i;
    }
    for (c = cells; c > 0; c--)                              /* ... and is put back to its beginning */
        h->start[c] = h->start[c - 1];
    h->start[0] = 0;
    if (sift3d_hip_memcpy_h2d(dev_rows, h->rows, 7 * m * sizeof(double), stream) ||
        sift3d_hip_memcpy_h2d(dev_orig, h->orig, m * sizeof(uint32_t), stream) ||
        sift3d_hip_memcpy_h2d(dev_orig + m, h->start, (cells + 1) * sizeof(uint32_t), stream))
        return SIFT3D_FAILURE;
    return SIFT3D_SUCCESS;
}

int sift3d_hip_ffd_landmarks(const float *d_lattice, int gx, int gy, int gz, int dx, int dy, int dz, const double *A,
                             const double *P, const double *Q, const double *w, int m, void *d_work, void *d_record,
                             double *d_r, double *d_GL, void *stream)
{
    static const char what[] = "sift3d_hip_ffd_landmarks";
    const int d[3] = { dx, dy, dz };
    ffd_lm_host h = { P, Q, w, m, 0.0, NULL, 1.0, NULL, NULL, NULL, NULL };
    sift3d_ffd_lm lm;
    int rc;
    if (!d_lattice || !d_work || !d_record)
        return refuse(what, "NULL argument");
    if (gx < 4 || gy < 4 || gz < 4)
        return refuse(what, "a lattice has at least 4 control points along every axis");
    if (!ffd_spacing_ok(dx, dy, dz))
        return refuse(what, "the spacing must be in [1, SIFT3D_AMD_FFD_MAX_SPACING]");
    if ((A && check_affine(what, A)) || check_landmarks(what, P, Q, w, m) ||
        check_aligned(what, ADDR(d_record) | ADDR(d_r) | ADDR(d_GL), ADDR(d_lattice)))
        return SIFT3D_FAILURE;
    if (ADDR(d_work) & 15)
        return refuse(what, "a buffer is misaligned");
    {
        const range_t in[] = { { d_lattice, image_bytes(gx, gy, gz, 3) } };
        const range_t out[] = { { d_record, SIFT3D_AMD_FFD_LANDMARKS_RECORD_BYTES },
                                { d_work, sift3d_amd_ffd_landmarks_work_bytes(m, gx, gy, gz) },
                                { d_r, d_r ? (size_t)m * 3 * sizeof(double) : 0 },
                                { d_GL, d_GL ? 3 * grid_voxels(gx, gy, gz) * sizeof(double) : 0 } };
        if (ranges_aliased(out, 4, in, 1))
            return refuse(what, ALIASED);
    }
    if (ffd_lm_host_alloc(what, &h, grid_voxels(gx - 3, gy - 3, gz - 3)))
        return SIFT3D_FAILURE;
    lm.weight = 0.0;
    lm.scale = 2.0;
    lm.A = A;
    lm.m = m;
    lm.d_rec = (double *)d_record;
    lm.d_GL = d_GL;
    lm.d_work = d_work;
    rc = ffd_lm_prepare(&h, &lm, gx, gy, gz, d, 1.0, stream) ||
         (d_r && sift3d_hip_memset(d_r, 0, (size_t)m * 3 * sizeof(double), stream)) ||
         sift3d_ffd_landmarks_launch(what, d_lattice, gx, gy, gz, dx, dy, dz, &lm, d_GL != NULL, d_r, stream);
    if (sift3d_hip_stream_sync(stream))                      /* the staging is released only behind its copies */
        rc = SIFT3D_FAILURE;
    free(h.rows);
    return rc ? SIFT3D_FAILURE : SIFT3D_SUCCESS;
}

/* the evaluation with the landmark term: d_lm holds the landmark record, GL and the landmarks' work; d_jac the penalty's
 * record, GJ and the penalty's work */
size_t sift3d_amd_ffd_evaluate_landmarks_bytes(int which, int m, int ox, int oy, int oz, int dx, int dy, int dz)
{
    const int gx = sift3d_amd_ffd_lattice_dim(ox, dx), gy = sift3d_amd_ffd_lattice_dim(oy, dy);
    const int gz = sift3d_amd_ffd_lattice_dim(oz, dz);
    const size_t lm = sift3d_amd_ffd_landmarks_work_bytes(m, gx, gy, gz);
    if (ox <= 0 || oy <= 0 || oz <= 0 || !ffd_spacing_ok(dx, dy, dz) || (which == 0 && !lm) || which < 0 || which > 1)
        return 0;
    return 32 + 3 * grid_voxels(gx, gy, gz) * sizeof(double) +
           (which == 0 ? lm : sift3d_amd_jacobian_penalty_work_bytes(ox, oy, oz));
}

static int ffd_jacobian_ref(const char *what, const double *A, double *ref);

int sift3d_hip_ffd_evaluate_landmarks(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                      const float *d_lattice, int gx, int gy, int gz, int dx, int dy, int dz,
                                      const double *A, double bending, float *d_field, void *d_record, float *d_grad,
                                      void *d_work, void *stream, const float *d_WF, const float *d_WM, double jacobian,
                                      void *d_jac, const double *P, const double *Q, const double *w, int m,
                                      double landmark_weight, void *d_lm)
{
    static const char what[] = "sift3d_hip_ffd_evaluate_landmarks";
    ffd_lm_host h = { P, Q, w, m, landmark_weight, NULL, 1.0, NULL, NULL, NULL, NULL };
    sift3d_ffd_jac jac;
    sift3d_ffd_lm lm;
    const ffd_entry_opts o = { .d_WF = d_WF, .d_WM = d_WM, .jac = d_jac ? &jac : NULL, .lmh = &h, .lm = &lm };
    double ref = 1.0;
    int rc;
    if (!d_F || !d_M || !d_lattice || !d_field || !d_record || !d_grad || !d_work || !d_lm)
        return refuse(what, "NULL argument");
    if (check_ffd_lattice(what, ox, oy, oz, gx, gy, gz, dx, dy, dz) || check_dims(what, nx, ny, nz))
        return SIFT3D_FAILURE;
    if (!isfinite(jacobian) || jacobian < 0)
        return refuse(what, "the Jacobian weight must be finite and not negative");
    if (jacobian != 0 && !d_jac)
        return refuse(what, "a Jacobian weight needs the penalty's buffer");
    if (!isfinite(landmark_weight) || landmark_weight < 0)
        return refuse(what, "the landmark weight must be finite and not negative");
    if (check_landmarks(what, P, Q, w, m) || (d_jac && ffd_jacobian_ref(what, A, &ref)) ||
        check_aligned(what, ADDR(d_jac) | ADDR(d_lm), 0))
        return SIFT3D_FAILURE;
    {
        const range_t in[] = { { d_F, image_bytes(ox, oy, oz, 1) }, { d_M, image_bytes(nx, ny, nz, 1) },
                               { d_lattice, image_bytes(gx, gy, gz, 3) },
                               { d_WF, d_WF ? image_bytes(ox, oy, oz, 1) : 0 },
                               { d_WM, d_WM ? image_bytes(nx, ny, nz, 1) : 0 },
                               { d_field, field_bytes(ox, oy, oz) },
                               { d_record, sift3d_amd_ffd_record_bytes(gx, gy, gz) },
                               { d_grad, image_bytes(gx, gy, gz, 3) },
                               { d_work, sift3d_amd_ffd_evaluate_work_bytes(ox, oy, oz, dx, dy, dz) } };
        const range_t out[] = { { d_lm, sift3d_amd_ffd_evaluate_landmarks_bytes(0, m, ox, oy, oz, dx, dy, dz) },
                                { d_jac, d_jac ? sift3d_amd_ffd_evaluate_landmarks_bytes(1, m, ox, oy, oz, dx, dy, dz)
                                               : 0 } };
        if (ranges_aliased(out, 2, in, 9))
            return refuse(what, ALIASED);
    }
    if (ffd_lm_host_alloc(what, &h, grid_voxels(gx - 3, gy - 3, gz - 3)))
        return SIFT3D_FAILURE;
    jac.weight = jacobian;
    jac.ref = ref;
    jac.d_rec = (double *)d_jac;
    jac.d_GJ = jac.d_rec + 4;
    jac.d_work = jac.d_GJ + 3 * grid_voxels(gx, gy, gz);
    lm.weight = landmark_weight;
    lm.scale = 2.0;
    lm.A = A;
    lm.n = 0;
    lm.m = m;
    lm.d_rec = (double *)d_lm;
    lm.d_GL = lm.d_rec + 4;
    lm.d_work = lm.d_GL + 3 * grid_voxels(gx, gy, gz);
    rc = ffd_evaluate_entry(what, d_F, ox, oy, oz, d_M, nx, ny, nz, d_lattice, gx, gy, gz, dx, dy, dz, A, bending,
                            d_field, d_record, d_grad, d_work, stream, &o);
    if (rc == SIFT3D_SUCCESS && sift3d_hip_stream_sync(stream))
        rc = SIFT3D_FAILURE;                                 /* the staging is released only behind its copies */
    free(h.rows);
    return rc;
}

/* ---- the driver ---- */

void sift3d_amd_ffd_refine_default_params(sift3d_amd_ffd_refine_params *p)
{
    if (!p)
        return;
    p->spacing[0] = p->spacing[1] = p->spacing[2] = 8;
    p->levels = 3;
    p->max_evaluations = 60;
    p->bending = 0.005;
    p->step0 = 1.0;
    p->step_max = 4.0;
    p->tol = 0.01;
    p->min_overlap = 0.5;
}

static int ffd_params_ok(const sift3d_amd_ffd_refine_params *p)
{
    return ffd_spacing_ok(p->spacing[0], p->spacing[1], p->spacing[2]) && p->levels >= 1 &&
           p->levels <= SIFT3D_AMD_DEMONS_MAX_LEVELS && p->max_evaluations >= 1 &&
           p->max_evaluations <= SIFT3D_AMD_FFD_MAX_EVALUATIONS && isfinite(p->bending) && p->bending >= 0 &&
           isfinite(p->step0) && p->step0 > 0 && isfinite(p->step_max) && p->step_max >= p->step0 &&
           isfinite(p->tol) && p->tol > 0 && p->min_overlap >= 0 && p->min_overlap <= 1;
}

size_t sift3d_amd_ffd_refine_struct_bytes(int which)
{
    return which == 0   ? sizeof(sift3d_amd_ffd_refine_params)
           : which == 1 ? sizeof(sift3d_amd_ffd_evaluation)
           : which == 2 ? sizeof(sift3d_amd_ffd_refine_result)
           : which == 3 ? (size_t)SIFT3D_AMD_FFD_RECORD_HEAD_BYTES
           : which == 4 ? (size_t)SIFT3D_AMD_FFD_MAX_EVALUATIONS
           : which == 5 ? (size_t)SIFT3D_AMD_DEMONS_MAX_LEVELS
           : which == 6 ? (size_t)SIFT3D_AMD_FFD_MAX_SPACING
                        : 0;
}

size_t sift3d_amd_ffd_level_struct_bytes(int which)
{
    return which == 0   ? sizeof(sift3d_amd_ffd_level)
           : which == 1 ? offsetof(sift3d_amd_ffd_level, d_F)
           : which == 2 ? offsetof(sift3d_amd_ffd_level, ox)
           : which == 3 ? offsetof(sift3d_amd_ffd_level, d_M)
           : which == 4 ? offsetof(sift3d_amd_ffd_level, nx)
           : which == 5 ? offsetof(sift3d_amd_ffd_level, d_WF)
           : which == 6 ? offsetof(sift3d_amd_ffd_level, d_WM)
                        : 0;
}

/* d_work of the driver, each part padded to 16 bytes: the evaluation's work on the level-0 grid (which covers every
 * coarser one), the record, five float lattices of level 0's size (c, c', their two gradients, the coarser level's
 * lattice), then per level l = 1 .. levels-1 the restricted fixed and moving volumes */
static size_t ffd_lattice_bytes(int ox, int oy, int oz, const int *d)
{
    return pad16(image_bytes(sift3d_amd_ffd_lattice_dim(ox, d[0]), sift3d_amd_ffd_lattice_dim(oy, d[1]),
                             sift3d_amd_ffd_lattice_dim(oz, d[2]), 3));
}

static size_t ffd_record_pad(int ox, int oy, int oz, const int *d)
{
    return pad16(sift3d_amd_ffd_record_bytes(sift3d_amd_ffd_lattice_dim(ox, d[0]), sift3d_amd_ffd_lattice_dim(oy, d[1]),
                                             sift3d_amd_ffd_lattice_dim(oz, d[2])));
}

size_t sift3d_amd_ffd_refine_work_bytes(int ox, int oy, int oz, int nx, int ny, int nz, int dx, int dy, int dz,
                                        int levels)
{
    const int d[3] = { dx, dy, dz };
    size_t total;
    int l;
    if (ox <= 0 || oy <= 0 || oz <= 0 || nx <= 0 || ny <= 0 || nz <= 0 || !ffd_spacing_ok(dx, dy, dz) || levels < 1 ||
        levels > SIFT3D_AMD_DEMONS_MAX_LEVELS)
        return 0;
    total = pad16(sift3d_amd_ffd_evaluate_work_bytes(ox, oy, oz, dx, dy, dz)) + ffd_record_pad(ox, oy, oz, d) +
            5 * ffd_lattice_bytes(ox, oy, oz, d);
    for (l = 1; l < levels; l++) {
        ox = multires_half(ox); oy = multires_half(oy); oz = multires_half(oz);
        nx = multires_half(nx); ny = multires_half(ny); nz = multires_half(nz);
        total += pad4(grid_voxels(ox, oy, oz)) * sizeof(float) + pad4(grid_voxels(nx, ny, nz)) * sizeof(float);
    }
    return total;
}

/* the masked driver's: the same, and the mask pyramid (sift3d_affine_refine.c) */
size_t sift3d_amd_ffd_refine_masked_work_bytes(int ox, int oy, int oz, int nx, int ny, int nz, int dx, int dy, int dz,
                                               int levels)
{
    const size_t plain = sift3d_amd_ffd_refine_work_bytes(ox, oy, oz, nx, ny, nz, dx, dy, dz, levels);
    return plain ? plain + mask_pyramid_bytes(ox, oy, oz, nx, ny, nz, levels) : 0;
}

/* the MI driver's: the masked driver's, then the MI affine driver's extra (the histogram and the count, copied to the
 * host together, then W), sized for SIFT3D_AMD_PARZEN_MAX_BINS whatever `bins` is */
size_t sift3d_amd_ffd_mi_refine_work_bytes(int ox, int oy, int oz, int nx, int ny, int nz, int dx, int dy, int dz,
                                           int levels)
{
    const size_t masked = sift3d_amd_ffd_refine_masked_work_bytes(ox, oy, oz, nx, ny, nz, dx, dy, dz, levels);
    return masked ? masked + MI_EXTRA_BYTES : 0;
}

typedef struct {
    const float *F, *M;
    int ox, oy, oz, nx, ny, nz, gx, gy, gz;
    const float *WF, *WM;                                    /* the level's masks, or NULL */
} ffd_level;

typedef struct {
    uint64_t n;
    double see, R, gmax;
} ffd_head;

/* the penalty's record ("Jacobian penalty") */
typedef struct {
    uint64_t nonpos;
    double sum, rmin, rmax;
} ffd_jac_head;

/* an evaluation on the host: the record's head and the image term of the cost (S_ee / n, or -mi; NaN when n == 0);
 * with a penalty its record and P = sum / N */
typedef struct {
    ffd_head h;
    double image;
    ffd_jac_head j;
    double P;
    double lm[3];                                /* with landmarks: S, Omega, rmax of their record */
    double L;                                    /* and the term in level-0 units: 4^l S / Omega, 0 when Omega == 0 */
} ffd_eval;

typedef struct {
    const int *d;                                /* spacing */
    const double *st;                            /* stencils */
    const float *d_w;
    double *d_rec, *d_eval;
    float *d_field;
    double bending;
    void *stream;
    mi_state *ms;                                /* MI (sift3d_affine_refine.c): bins, ranges, histogram, W; or NULL */
    sift3d_ffd_mi mi;                            /* MI: ms' bins, ranges and device table with the fixed bin's scale */
    const sift3d_ffd_jac *jac;                   /* the Jacobian penalty's weight and buffers; or NULL */
    int nc;                                      /* the channels of the levels' stacks; 0: single volumes */
    const sift3d_ffd_lm *lm;                     /* the landmark term's weight and buffers on this level; or NULL */
} ffd_ctx;

/* with a penalty: its record to the host, ahead of the wait that the caller makes */
static int ffd_jac_fetch(const ffd_ctx *x, ffd_eval *e)
{
    return x->jac ? sift3d_hip_memcpy_d2h(&e->j, x->jac->d_rec, sizeof(e->j), x->stream) : SIFT3D_SUCCESS;
}

static void ffd_jac_mean(const ffd_ctx *x, const ffd_level *lv, ffd_eval *e)
{
    e->P = x->jac ? e->j.sum / (double)grid_voxels(lv->ox, lv->oy, lv->oz) : 0.0;
}

/* with landmarks: S, Omega and rmax of their record to the host, ahead of the same wait */
static int ffd_lm_fetch(const ffd_ctx *x, ffd_eval *e)
{
    return x->lm ? sift3d_hip_memcpy_d2h(e->lm, x->lm->d_rec + 1, sizeof(e->lm), x->stream) : SIFT3D_SUCCESS;
}

/* lm->scale is 2 * 4^l */
static void ffd_lm_mean(const ffd_ctx *x, ffd_eval *e)
{
    e->L = x->lm && e->lm[1] != 0.0 ? ((0.5 * x->lm->scale) * e->lm[0]) / e->lm[1] : 0.0;
}

/* the descriptor of an evaluation at lattice c on `lv`, its gradient going to `grad` */
static sift3d_ffd_eval ffd_describe(const ffd_ctx *x, const ffd_level *lv, const float *c, float *grad)
{
    const sift3d_ffd_eval d = { .d_F = lv->F, .d_M = lv->M, .ox = lv->ox, .oy = lv->oy, .oz = lv->oz, .nx = lv->nx,
                                .ny = lv->ny, .nz = lv->nz, .nc = x->nc, .d_WF = lv->WF, .d_WM = lv->WM,
                                .d_field = x->d_field, .d_lat = c, .gx = lv->gx, .gy = lv->gy, .gz = lv->gz,
                                .dx = x->d[0], .dy = x->d[1], .dz = x->d[2], .d_w = x->d_w, .stencils = x->st,
                                .bending = x->bending, .mi = x->ms ? &x->mi : NULL, .jac = x->jac, .lm = x->lm,
                                .d_rec = x->d_rec, .d_grad = grad, .d_work = x->d_eval, .stream = x->stream };
    return d;
}

/* one evaluation at lattice c on `lv`: the field, then
 *   MSD: the record, R and the gradient, the head's copy to the host and the wait for it;
 *   MI:  the histogram through the field (its partial counts in the evaluation's partial slots) and R, histogram, count
 *        and head to the host and the wait for them, sift3d_amd_parzen_mi.  ms->W is left holding the table and
 *        ms->sim_trial the measures; no gradient is made (ffd_mi_gradient), and e->h.gmax is not meaningful.
 * With a penalty (x->jac) its passes run with the others and its record comes to the host in the same wait. */
static int ffd_evaluate(const char *what, const ffd_ctx *x, const ffd_level *lv, const double *A, const float *c,
                        float *grad, ffd_eval *e)
{
    mi_state *ms = x->ms;
    const sift3d_ffd_eval d = ffd_describe(x, lv, c, grad);
    if (sift3d_ffd_field_launch(what, c, lv->gx, lv->gy, lv->gz, x->d[0], x->d[1], x->d[2], x->d_w, A, lv->ox, lv->oy,
                                lv->oz, x->d_field, x->stream))
        return SIFT3D_FAILURE;
    if (ms) {
        const size_t cells = (size_t)ms->bins * ms->bins;
        if (sift3d_parzen_hist_launch(what, lv->F, lv->ox, lv->oy, lv->oz, lv->M, lv->nx, lv->ny, lv->nz, NULL,
                                      x->d_field, ms->bins, ms->lo_f, x->mi.s_f, ms->lo_m, ms->hi_m,
                                      (unsigned long long *)ms->d_hist, (unsigned long long *)(ms->d_hist + cells),
                                      x->d_eval, x->stream, lv->WF, lv->WM) ||
            sift3d_ffd_evaluate_launch(what, ffd_parts(&d, 1, 0), &d) ||
            sift3d_hip_memcpy_d2h(ms->hist, ms->d_hist, (cells + 1) * sizeof(uint64_t), x->stream) ||
            sift3d_hip_memcpy_d2h(&e->h, x->d_rec, sizeof(e->h), x->stream) || ffd_jac_fetch(x, e) ||
            ffd_lm_fetch(x, e) || sift3d_hip_stream_sync(x->stream) ||
            sift3d_amd_parzen_mi(ms->hist, ms->bins, &ms->sim_trial, ms->W))
            return SIFT3D_FAILURE;
        e->h.n = ms->hist[cells];
        e->h.see = 0.0;
        e->h.gmax = NAN;
        e->image = -ms->sim_trial.mi;                        /* NaN when nothing was counted */
        ffd_jac_mean(x, lv, e);
        ffd_lm_mean(x, e);
        return SIFT3D_SUCCESS;
    }
    if (sift3d_ffd_evaluate_launch(what, ffd_parts(&d, 1, 1), &d) ||
        sift3d_hip_memcpy_d2h(&e->h, x->d_rec, sizeof(e->h), x->stream) || ffd_jac_fetch(x, e) ||
        ffd_lm_fetch(x, e) || sift3d_hip_stream_sync(x->stream))
        return SIFT3D_FAILURE;
    e->image = e->h.n ? e->h.see / (double)e->h.n : NAN;
    ffd_jac_mean(x, lv, e);
    ffd_lm_mean(x, e);
    return SIFT3D_SUCCESS;
}

/* MI: the gradient at c, the lattice of the evaluation that left its table in ms->W, its field in d_field and its
 * second derivatives in the work buffer (no evaluation was made since): W to the device, the force, adjoint, bending
 * gradient and combine passes (with a penalty of weight > 0, its value and gradient passes on the same field: the same
 * record once more, S and GJ; with landmarks of weight > 0 their value and adjoint passes likewise; with weight 0
 * neither runs at all), gmax to the host and the wait for it */
static int ffd_mi_gradient(const char *what, const ffd_ctx *x, const ffd_level *lv, const float *c, float *grad,
                           ffd_eval *e)
{
    mi_state *ms = x->ms;
    sift3d_ffd_eval d = ffd_describe(x, lv, c, grad);
    ffd_head h;
    if (d.jac && !(d.jac->weight > 0))
        d.jac = NULL;
    if (d.lm && !(d.lm->weight > 0))
        d.lm = NULL;
    if (sift3d_hip_memcpy_h2d(ms->d_W, ms->W, (size_t)ms->bins * ms->bins * sizeof(double), x->stream) ||
        sift3d_ffd_evaluate_launch(what, ffd_parts(&d, 0, 1), &d) ||
        sift3d_hip_memcpy_d2h(&h, x->d_rec, sizeof(h), x->stream) || sift3d_hip_stream_sync(x->stream))
        return SIFT3D_FAILURE;
    e->h.gmax = h.gmax;
    return SIFT3D_SUCCESS;
}

/* jacobian: the penalty's weight; 0 (also: no penalty) adds no third term.  lambda: the landmark term's weight, as
 * jacobian */
static double ffd_cost(const ffd_eval *e, double bending, double jacobian, double lambda)
{
    const double two = e->image + bending * e->h.R;
    const double base = jacobian > 0 ? two + jacobian * e->P : two;
    return lambda > 0 ? base + lambda * e->L : base;
}

/* penalty: the caller's array parallel to the trail, or NULL; lmh: the landmarks with theirs, or NULL (n: those counted
 * on this level) */
static void ffd_trail(sift3d_amd_ffd_refine_result *res, const ffd_eval *v, double bending, double jacobian,
                      sift3d_amd_ffd_penalty *penalty, const ffd_lm_host *lmh, int n, double step, int accepted,
                      int level)
{
    sift3d_amd_ffd_evaluation *e = res->trail + res->evaluations++;
    const double lambda = lmh ? lmh->weight : 0.0;
    if (lmh) {
        sift3d_amd_ffd_landmark_term *t = lmh->out + (e - res->trail);
        t->L = v->L;
        t->rmax = v->lm[2] * lmh->up;
        t->counted = (uint64_t)n;
    }
    if (penalty) {
        sift3d_amd_ffd_penalty *q = penalty + (e - res->trail);
        q->P = v->P;
        q->rmin = v->j.rmin;
        q->nonpos = v->j.nonpos;
    }
    e->E = ffd_cost(v, bending, jacobian, lambda);
    e->msd = v->image;
    e->R = v->h.R;
    e->n = v->h.n;
    e->step = step;
    e->accepted = accepted;
    e->level = level;
}

/* the channels driver's work without the penalty's: the evaluation's, the record and the five lattices */
static size_t ffd_channels_base_bytes(int ox, int oy, int oz, const int *d)
{
    return pad16(sift3d_amd_ffd_evaluate_work_bytes(ox, oy, oz, d[0], d[1], d[2])) + ffd_record_pad(ox, oy, oz, d) +
           5 * ffd_lattice_bytes(ox, oy, oz, d);
}

/* what a driver has beside sift3d_amd_ffd_refine_device's arguments; all zero: nothing */
typedef struct {
    int masked;                                  /* selects the work buffer's size; the masks may still be NULL */
    const float *d_WF, *d_WM;
    mi_state *ms;                                /* MI (else NULL): bins and ranges, checked by the body after the FFD
                                                    drivers' own checks; the cost's image term is -mi, the gradient is
                                                    made only at the lattice a step starts from, and ms->sim leaves with
                                                    the measures at the final lattice on level 0 */
    double jacobian, ref;                        /* with `penalty`: the weight and the reference determinant, both
                                                    checked by the caller */
    sift3d_amd_ffd_penalty *penalty;             /* the Jacobian driver (else NULL): the array parallel to the trail;
                                                    the work buffer is that driver's */
    const sift3d_amd_ffd_level *src;             /* the channels driver (else NULL): the caller's levels, checked by the
                                                    caller, of nc channels each.  d_F .. d_WM are then level 0's; the
                                                    other levels are taken from src where the other drivers restrict
                                                    the level above, and the work buffer is
                                                    sift3d_amd_ffd_refine_channels_work_bytes() */
    int nc;
    ffd_lm_host *lmh;                            /* the landmarks driver (else NULL; never with src): the landmarks,
                                                    checked by the caller, their weight and the array parallel to the
                                                    trail, with staging for level 0's lattice; the work buffer is that
                                                    driver's whether or not there is a penalty */
} ffd_refine_opts;

/* the shared body of the drivers */
static int ffd_refine(const char *what, const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny,
                      int nz, const double *A_in, const sift3d_amd_ffd_refine_params *params,
                      sift3d_amd_ffd_refine_result *result, float *d_lattice, float *d_field, void *d_work,
                      void *stream, const ffd_refine_opts *o)
{
    const float *d_WF = o->d_WF, *d_WM = o->d_WM;
    mi_state *ms = o->ms;
    const double jacobian = o->jacobian;
    sift3d_amd_ffd_penalty *penalty = o->penalty;
    const sift3d_amd_ffd_level *src = o->src;
    ffd_lm_host *lmh = o->lmh;
    const int nc = o->nc;
    const int ch = src ? nc : 1;
    const double lambda = lmh ? lmh->weight : 0.0;
    sift3d_ffd_jac jac;
    sift3d_ffd_lm lm;
    sift3d_amd_ffd_refine_params prm;
    ffd_level lv[SIFT3D_AMD_DEMONS_MAX_LEVELS];
    ffd_eval rec, trial;
    size_t work_bytes;
    float s_f = 0.0f;                                        /* MI: the fixed bin's scale */
    ffd_ctx x;
    double A[12], st[27];
    float *c, *ct, *g, *gt, *prev;
    char *w = (char *)d_work;
    size_t off, lat;
    int l, i, have_A = A_in != NULL;
    if (!d_F || !d_M || !result || !d_lattice || !d_field || !d_work)
        return refuse(what, "NULL argument");
    if (params)
        prm = *params;
    else
        sift3d_amd_ffd_refine_default_params(&prm);
    if (check_dims(what, ox, oy, oz) || check_dims(what, nx, ny, nz) || (A_in && check_affine(what, A_in)))
        return SIFT3D_FAILURE;
    if (!ffd_params_ok(&prm))
        return refuse(what, "a parameter is out of range");
    if (check_aligned(what, 0, ADDR(d_F) | ADDR(d_M) | ADDR(d_lattice) | ADDR(d_field) | ADDR(d_WF) | ADDR(d_WM)))
        return SIFT3D_FAILURE;
    if (ADDR(d_work) & 15)
        return refuse(what, "a buffer is misaligned");
    lv[0] = (ffd_level){ d_F, d_M, ox, oy, oz, nx, ny, nz, sift3d_amd_ffd_lattice_dim(ox, prm.spacing[0]),
                         sift3d_amd_ffd_lattice_dim(oy, prm.spacing[1]), sift3d_amd_ffd_lattice_dim(oz, prm.spacing[2]),
                         d_WF, d_WM };
    {
        const range_t in[] = { { d_F, image_bytes(ox, oy, oz, ch) }, { d_M, image_bytes(nx, ny, nz, ch) },
                               { d_WF, d_WF ? image_bytes(ox, oy, oz, 1) : 0 },
                               { d_WM, d_WM ? image_bytes(nx, ny, nz, 1) : 0 } };
        const range_t out[] = { { d_lattice, image_bytes(lv[0].gx, lv[0].gy, lv[0].gz, 3) },
                                { d_field, field_bytes(ox, oy, oz) },
                                { d_work, lmh ? sift3d_amd_ffd_refine_landmarks_work_bytes(
                                                    ox, oy, oz, nx, ny, nz, prm.spacing[0], prm.spacing[1],
                                                    prm.spacing[2], prm.levels, lmh->m)
                                          : src ? sift3d_amd_ffd_refine_channels_work_bytes(ox, oy, oz, prm.spacing[0],
                                                                                          prm.spacing[1], prm.spacing[2])
                                              : (penalty  ? sift3d_amd_ffd_refine_jacobian_work_bytes
                                                 : ms     ? sift3d_amd_ffd_mi_refine_work_bytes
                                                 : o->masked ? sift3d_amd_ffd_refine_masked_work_bytes
                                                          : sift3d_amd_ffd_refine_work_bytes)(
                                                    ox, oy, oz, nx, ny, nz, prm.spacing[0], prm.spacing[1],
                                                    prm.spacing[2], prm.levels) } };
        if (ranges_aliased(out, 3, in, 4))
            return refuse(what, ALIASED);
        work_bytes = out[2].bytes;
    }
    if (ms && parzen_check(what, ms->bins, ms->lo_f, ms->hi_f, ms->lo_m, ms->hi_m, &s_f))
        return SIFT3D_FAILURE;
    result->evaluations = 0;
    result->stop = SIFT3D_AMD_FFD_STOP_EVALUATIONS;
    for (i = 0; i < 12; i++)
        A[i] = have_A ? A_in[i] : (i % 5 == 0 ? 1.0 : 0.0);
    ffd_stencils(prm.spacing, st);
    lat = ffd_lattice_bytes(ox, oy, oz, prm.spacing);
    x.d = prm.spacing;
    x.st = st;
    x.d_w = (const float *)w;
    x.d_eval = (double *)(w + pad16(ffd_weights_bytes(prm.spacing[0], prm.spacing[1], prm.spacing[2])));
    off = pad16(sift3d_amd_ffd_evaluate_work_bytes(ox, oy, oz, prm.spacing[0], prm.spacing[1], prm.spacing[2]));
    x.d_rec = (double *)(w + off);
    off += ffd_record_pad(ox, oy, oz, prm.spacing);
    c = (float *)(w + off);
    ct = (float *)(w + off + lat);
    g = (float *)(w + off + 2 * lat);
    gt = (float *)(w + off + 3 * lat);
    prev = (float *)(w + off + 4 * lat);
    off += 5 * lat;
    x.d_field = d_field;
    x.bending = prm.bending;
    x.stream = stream;
    x.ms = ms;
    x.jac = NULL;
    x.nc = src ? nc : 0;
    x.lm = NULL;
    lm.n = 0;
    if (lmh) {                                               /* behind everything the Jacobian driver lays out */
        char *at = w + pad16(sift3d_amd_ffd_refine_jacobian_work_bytes(ox, oy, oz, nx, ny, nz, prm.spacing[0],
                                                                       prm.spacing[1], prm.spacing[2], prm.levels));
        lm.weight = lambda;
        lm.m = lmh->m;
        lm.A = have_A ? A : NULL;
        lm.d_rec = (double *)at;
        lm.d_GL = (double *)(at + SIFT3D_AMD_FFD_LANDMARKS_RECORD_BYTES);
        lm.d_work = lm.d_GL + 3 * grid_voxels(lv[0].gx, lv[0].gy, lv[0].gz);
        x.lm = &lm;
    }
    if (penalty || lmh)                                      /* the MI driver's share of the larger buffer */
        work_bytes = src ? ffd_channels_base_bytes(ox, oy, oz, prm.spacing)
                         : sift3d_amd_ffd_mi_refine_work_bytes(ox, oy, oz, nx, ny, nz, prm.spacing[0], prm.spacing[1],
                                                               prm.spacing[2], prm.levels);
    if (penalty) {                                           /* behind everything the MI driver lays out (channels:
                                                                behind the lattices) */
        jac.weight = jacobian;
        jac.ref = o->ref;
        jac.d_rec = (double *)(w + work_bytes);
        jac.d_GJ = (double *)(w + work_bytes + SIFT3D_AMD_JACOBIAN_PENALTY_RECORD_BYTES);
        jac.d_work = jac.d_GJ + 3 * grid_voxels(lv[0].gx, lv[0].gy, lv[0].gz);
        x.jac = &jac;
    }
    if (ms) {                                                /* behind everything the masked driver lays out */
        ms->d_hist = (uint64_t *)(w + work_bytes - MI_EXTRA_BYTES);
        ms->d_W = (double *)(w + work_bytes - MI_TABLE_BYTES);
        x.mi = (sift3d_ffd_mi){ ms->bins, ms->lo_f, s_f, ms->lo_m, ms->hi_m, ms->d_W };
    }
    if (ffd_upload_weights(prm.spacing[0], prm.spacing[1], prm.spacing[2], (float *)w, stream))
        return SIFT3D_FAILURE;
    for (l = 1; l < prm.levels; l++) {                       /* level l from level l - 1; A's shift halves */
        const ffd_level *f = lv + l - 1;
        ffd_level *k = lv + l;
        float *cF = (float *)(w + off), *cM;
        *k = (ffd_level){ NULL, NULL, multires_half(f->ox), multires_half(f->oy), multires_half(f->oz),
                          multires_half(f->nx), multires_half(f->ny), multires_half(f->nz), 0, 0, 0, NULL, NULL };
        k->gx = sift3d_amd_ffd_lattice_dim(k->ox, prm.spacing[0]);
        k->gy = sift3d_amd_ffd_lattice_dim(k->oy, prm.spacing[1]);
        k->gz = sift3d_amd_ffd_lattice_dim(k->oz, prm.spacing[2]);
        if (src) {                                           /* the caller's level: the halving chain, checked */
            k->F = src[l].d_F;
            k->M = src[l].d_M;
            k->WF = src[l].d_WF;
            k->WM = src[l].d_WM;
        } else {
            off += pad4(grid_voxels(k->ox, k->oy, k->oz)) * sizeof(float);
            cM = (float *)(w + off);
            off += pad4(grid_voxels(k->nx, k->ny, k->nz)) * sizeof(float);
            if (sift3d_hip_restrict2(f->F, f->ox, f->oy, f->oz, 1, cF, 1.0f, stream) ||
                sift3d_hip_restrict2(f->M, f->nx, f->ny, f->nz, 1, cM, 1.0f, stream))
                return SIFT3D_FAILURE;
            k->F = cF;
            k->M = cM;
            if (mask_pyramid_level(f->WF, f->ox, f->oy, f->oz, f->WM, f->nx, f->ny, f->nz, w, &off, &k->WF, &k->WM,
                                   stream))
                return SIFT3D_FAILURE;
        }
        for (i = 3; i < 12; i += 4)
            A[i] = A[i] * 0.5;
    }
    for (l = prm.levels - 1; l >= 0; l--) {
        const ffd_level *v = lv + l;
        const size_t nc = 3 * grid_voxels(v->gx, v->gy, v->gz);
        double s = prm.step0, E;
        uint64_t n_first;
        int evals = 1, stop;
        int stale = ms != NULL;                              /* MI: g holds no gradient at c yet */
        if (l == prm.levels - 1) {
            if (sift3d_hip_memset(c, 0, nc * sizeof(float), stream))
                return SIFT3D_FAILURE;
        } else {
            float *t = prev;                                 /* the coarser level's result is in c */
            prev = c;
            c = t;
            if (sift3d_ffd_refine2_launch(prev, lv[l + 1].gx, lv[l + 1].gy, lv[l + 1].gz, c, v->gx, v->gy, v->gz,
                                          stream))
                return SIFT3D_FAILURE;
        }
        if (lmh) {                                           /* this level's landmarks: P, Q times 0.5^l, in cell order */
            lmh->up = ldexp(1.0, l);
            lm.scale = 2.0 * ldexp(1.0, 2 * l);
            if (ffd_lm_prepare(lmh, &lm, v->gx, v->gy, v->gz, prm.spacing, ldexp(1.0, -l), stream))
                return SIFT3D_FAILURE;
        }
        if (ffd_evaluate(what, &x, v, have_A ? A : NULL, c, g, &rec))
            return SIFT3D_FAILURE;
        if (ms)
            ms->sim = ms->sim_trial;
        ffd_trail(result, &rec, prm.bending, jacobian, penalty, lmh, lm.n, s, 1, l);
        n_first = rec.h.n;
        E = ffd_cost(&rec, prm.bending, jacobian, lambda);
        if (!isfinite(E))
            stop = SIFT3D_AMD_FFD_STOP_FAILED;
        else
            for (;;) {
                double Et;
                int accept;
                if (evals >= prm.max_evaluations) {
                    stop = SIFT3D_AMD_FFD_STOP_EVALUATIONS;
                    break;
                }
                if (stale) {                                 /* the gradient at the lattice this step starts from;
                                                                ms->W is still that lattice's */
                    if (ffd_mi_gradient(what, &x, v, c, g, &rec))
                        return SIFT3D_FAILURE;
                    stale = 0;
                }
                if (rec.h.gmax == 0.0) {
                    stop = SIFT3D_AMD_FFD_STOP_FLAT;
                    break;
                }
                if (sift3d_ffd_step_launch(c, g, (float)(s / rec.h.gmax), ct, nc, stream) ||
                    ffd_evaluate(what, &x, v, have_A ? A : NULL, ct, gt, &trial))
                    return SIFT3D_FAILURE;
                evals++;
                Et = ffd_cost(&trial, prm.bending, jacobian, lambda);
                accept = isfinite(Et) && (double)trial.h.n >= prm.min_overlap * (double)n_first && Et < E;
                ffd_trail(result, &trial, prm.bending, jacobian, penalty, lmh, lm.n, s, accept, l);
                if (!isfinite(Et) && !(ms && trial.h.n == 0)) {      /* MI: a trial that counts nothing is rejected */
                    stop = SIFT3D_AMD_FFD_STOP_FAILED;
                    break;
                }
                if (accept) {
                    float *t = c;
                    c = ct; ct = t;
                    t = g; g = gt; gt = t;
                    rec = trial;
                    E = Et;
                    stale = ms != NULL;
                    if (ms)
                        ms->sim = ms->sim_trial;
                    s = 2.0 * s < prm.step_max ? 2.0 * s : prm.step_max;
                } else
                    s = s * 0.5;
                if (s < prm.tol) {
                    stop = SIFT3D_AMD_FFD_STOP_CONVERGED;
                    break;
                }
            }
        result->stop = stop;
        if (l > 0)
            for (i = 3; i < 12; i += 4)
                A[i] = A[i] * 2.0;
    }
    /* the final lattice and its field (the last evaluation may have been a rejected trial) */
    if (sift3d_hip_memcpy_d2d(d_lattice, c, image_bytes(lv[0].gx, lv[0].gy, lv[0].gz, 3), stream) ||
        sift3d_ffd_field_launch(what, c, lv[0].gx, lv[0].gy, lv[0].gz, prm.spacing[0], prm.spacing[1], prm.spacing[2],
                                x.d_w, have_A ? A : NULL, ox, oy, oz, d_field, stream) ||
        sift3d_hip_stream_sync(stream))
        return SIFT3D_FAILURE;
    return SIFT3D_SUCCESS;
}

int sift3d_amd_ffd_refine_device(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                 const double *A_in, const sift3d_amd_ffd_refine_params *params,
                                 sift3d_amd_ffd_refine_result *result, float *d_lattice, float *d_field, void *d_work,
                                 void *stream)
{
    const ffd_refine_opts o = { .masked = 0 };
    return ffd_refine("sift3d_amd_ffd_refine_device", d_F, ox, oy, oz, d_M, nx, ny, nz, A_in, params, result,
                      d_lattice, d_field, d_work, stream, &o);
}

int sift3d_amd_ffd_refine_masked_device(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny,
                                        int nz, const double *A_in, const sift3d_amd_ffd_refine_params *params,
                                        sift3d_amd_ffd_refine_result *result, float *d_lattice, float *d_field,
                                        void *d_work, void *stream, const float *d_WF, const float *d_WM)
{
    const ffd_refine_opts o = { .masked = 1, .d_WF = d_WF, .d_WM = d_WM };
    return ffd_refine("sift3d_amd_ffd_refine_masked_device", d_F, ox, oy, oz, d_M, nx, ny, nz, A_in, params, result,
                      d_lattice, d_field, d_work, stream, &o);
}

int sift3d_amd_ffd_mi_refine_device(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                    const double *A_in, const sift3d_amd_ffd_refine_params *params,
                                    sift3d_amd_ffd_refine_result *result, float *d_lattice, float *d_field,
                                    void *d_work, void *stream, const float *d_WF, const float *d_WM, int bins,
                                    float lo_f, float hi_f, float lo_m, float hi_m, sift3d_amd_similarity *mi_out)
{
    static const char what[] = "sift3d_amd_ffd_mi_refine_device";
    mi_state ms;
    const ffd_refine_opts o = { .masked = 1, .d_WF = d_WF, .d_WM = d_WM, .ms = &ms };
    int rc;
    if (!mi_out)
        return refuse(what, "NULL argument");
    ms.bins = bins;
    ms.lo_f = lo_f; ms.hi_f = hi_f;
    ms.lo_m = lo_m; ms.hi_m = hi_m;
    ms.sim.n = 0;
    ms.sim.msd = ms.sim.ncc = ms.sim.mi = ms.sim.nmi = NAN;
    ms.sim.entropy_fixed = ms.sim.entropy_moving = ms.sim.entropy_joint = NAN;
    *mi_out = ms.sim;
    rc = ffd_refine(what, d_F, ox, oy, oz, d_M, nx, ny, nz, A_in, params, result, d_lattice, d_field, d_work, stream, &o);
    *mi_out = ms.sim;
    return rc;
}

/* the Jacobian driver's: the MI driver's, then the penalty's record, GJ on the finest lattice and the penalty's work on
 * the finest grid (which cover every coarser level's) */
size_t sift3d_amd_ffd_refine_jacobian_work_bytes(int ox, int oy, int oz, int nx, int ny, int nz, int dx, int dy, int dz,
                                                 int levels)
{
    const size_t mi = sift3d_amd_ffd_mi_refine_work_bytes(ox, oy, oz, nx, ny, nz, dx, dy, dz, levels);
    if (!mi)
        return 0;
    return mi + SIFT3D_AMD_JACOBIAN_PENALTY_RECORD_BYTES +
           3 * grid_voxels(sift3d_amd_ffd_lattice_dim(ox, dx), sift3d_amd_ffd_lattice_dim(oy, dy),
                           sift3d_amd_ffd_lattice_dim(oz, dz)) * sizeof(double) +
           sift3d_amd_jacobian_penalty_work_bytes(ox, oy, oz);
}

/* the penalty's reference determinant: det of A's linear part, 1.0 without A; refused when not finite or 0 */
static int ffd_jacobian_ref(const char *what, const double *A, double *ref)
{
    *ref = 1.0;
    if (!A)
        return SIFT3D_SUCCESS;
    if (check_affine(what, A))
        return SIFT3D_FAILURE;
    *ref = A[0] * (A[5] * A[10] - A[6] * A[9]) - A[1] * (A[4] * A[10] - A[6] * A[8]) +
           A[2] * (A[4] * A[9] - A[5] * A[8]);
    if (!isfinite(*ref) || *ref == 0.0)
        return refuse(what, "the linear part of A must have a finite determinant that is not 0");
    return SIFT3D_SUCCESS;
}

int sift3d_amd_ffd_refine_jacobian_device(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny,
                                          int nz, const double *A_in, const sift3d_amd_ffd_refine_params *params,
                                          sift3d_amd_ffd_refine_result *result, float *d_lattice, float *d_field,
                                          void *d_work, void *stream, const float *d_WF, const float *d_WM, int bins,
                                          float lo_f, float hi_f, float lo_m, float hi_m, sift3d_amd_similarity *mi_out,
                                          double jacobian, sift3d_amd_ffd_penalty *penalty)
{
    static const char what[] = "sift3d_amd_ffd_refine_jacobian_device";
    ffd_refine_opts o;
    mi_state ms;
    double ref = 1.0;
    int rc;
    if (!penalty || (bins != 0 && !mi_out))
        return refuse(what, "NULL argument");
    if (!isfinite(jacobian) || jacobian < 0)
        return refuse(what, "the Jacobian weight must be finite and not negative");
    if (ffd_jacobian_ref(what, A_in, &ref))
        return SIFT3D_FAILURE;
    ms.bins = bins;
    ms.lo_f = lo_f; ms.hi_f = hi_f;
    ms.lo_m = lo_m; ms.hi_m = hi_m;
    ms.sim.n = 0;
    ms.sim.msd = ms.sim.ncc = ms.sim.mi = ms.sim.nmi = NAN;
    ms.sim.entropy_fixed = ms.sim.entropy_moving = ms.sim.entropy_joint = NAN;
    if (mi_out)
        *mi_out = ms.sim;
    o = (ffd_refine_opts){ .masked = 1, .d_WF = d_WF, .d_WM = d_WM, .ms = bins != 0 ? &ms : NULL,
                           .jacobian = jacobian, .ref = ref, .penalty = penalty };
    rc = ffd_refine(what, d_F, ox, oy, oz, d_M, nx, ny, nz, A_in, params, result, d_lattice, d_field, d_work, stream, &o);
    if (mi_out)
        *mi_out = ms.sim;
    return rc;
}

/* ---- the landmarks driver ("FFD landmarks") ---- */

/* the Jacobian driver's (padded to 16), then the landmark record, GL on the finest lattice and the landmarks' work for
 * the finest lattice (which cover every coarser level's) */
size_t sift3d_amd_ffd_refine_landmarks_work_bytes(int ox, int oy, int oz, int nx, int ny, int nz, int dx, int dy, int dz,
                                                  int levels, int m)
{
    const size_t jac = sift3d_amd_ffd_refine_jacobian_work_bytes(ox, oy, oz, nx, ny, nz, dx, dy, dz, levels);
    const int gx = sift3d_amd_ffd_lattice_dim(ox, dx), gy = sift3d_amd_ffd_lattice_dim(oy, dy);
    const int gz = sift3d_amd_ffd_lattice_dim(oz, dz);
    const size_t lm = jac ? sift3d_amd_ffd_landmarks_work_bytes(m, gx, gy, gz) : 0;
    if (!lm)
        return 0;
    return pad16(jac) + SIFT3D_AMD_FFD_LANDMARKS_RECORD_BYTES + 3 * grid_voxels(gx, gy, gz) * sizeof(double) + lm;
}

int sift3d_amd_ffd_refine_landmarks_device(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny,
                                           int nz, const double *A_in, const sift3d_amd_ffd_refine_params *params,
                                           sift3d_amd_ffd_refine_result *result, float *d_lattice, float *d_field,
                                           void *d_work, void *stream, const float *d_WF, const float *d_WM, int bins,
                                           float lo_f, float hi_f, float lo_m, float hi_m,
                                           sift3d_amd_similarity *mi_out, double jacobian,
                                           sift3d_amd_ffd_penalty *penalty, const double *P, const double *Q,
                                           const double *w, int m, double landmark_weight,
                                           sift3d_amd_ffd_landmark_term *landmarks_out)
{
    static const char what[] = "sift3d_amd_ffd_refine_landmarks_device";
    ffd_lm_host h = { P, Q, w, m, landmark_weight, landmarks_out, 1.0, NULL, NULL, NULL, NULL };
    sift3d_amd_ffd_refine_params prm;
    ffd_refine_opts o;
    mi_state ms;
    double ref = 1.0;
    int rc;
    if (!landmarks_out || (bins != 0 && !mi_out))
        return refuse(what, "NULL argument");
    if (!isfinite(jacobian) || jacobian < 0)
        return refuse(what, "the Jacobian weight must be finite and not negative");
    if (jacobian != 0 && !penalty)
        return refuse(what, "a Jacobian weight needs the penalty array");
    if (!isfinite(landmark_weight) || landmark_weight < 0)
        return refuse(what, "the landmark weight must be finite and not negative");
    if (check_landmarks(what, P, Q, w, m) || (penalty && ffd_jacobian_ref(what, A_in, &ref)))
        return SIFT3D_FAILURE;
    if (params)
        prm = *params;
    else
        sift3d_amd_ffd_refine_default_params(&prm);
    if (check_dims(what, ox, oy, oz))                        /* what the staging's size is made of */
        return SIFT3D_FAILURE;
    if (!ffd_params_ok(&prm))
        return refuse(what, "a parameter is out of range");
    ms.bins = bins;
    ms.lo_f = lo_f; ms.hi_f = hi_f;
    ms.lo_m = lo_m; ms.hi_m = hi_m;
    ms.sim.n = 0;
    ms.sim.msd = ms.sim.ncc = ms.sim.mi = ms.sim.nmi = NAN;
    ms.sim.entropy_fixed = ms.sim.entropy_moving = ms.sim.entropy_joint = NAN;
    if (mi_out)
        *mi_out = ms.sim;
    if (ffd_lm_host_alloc(what, &h, grid_voxels(sift3d_amd_ffd_lattice_dim(ox, prm.spacing[0]) - 3,
                                                sift3d_amd_ffd_lattice_dim(oy, prm.spacing[1]) - 3,
                                                sift3d_amd_ffd_lattice_dim(oz, prm.spacing[2]) - 3)))
        return SIFT3D_FAILURE;
    o = (ffd_refine_opts){ .masked = 1, .d_WF = d_WF, .d_WM = d_WM, .ms = bins != 0 ? &ms : NULL,
                           .jacobian = jacobian, .ref = ref, .penalty = penalty, .lmh = &h };
    rc = ffd_refine(what, d_F, ox, oy, oz, d_M, nx, ny, nz, A_in, &prm, result, d_lattice, d_field, d_work, stream, &o);
    free(h.rows);                                            /* every copy from it was staged when its call returned */
    if (mi_out)
        *mi_out = ms.sim;
    return rc;
}

/* ---- the channels driver ("Multi-channel free-form deformation") ---- */

/* the evaluation's work, the record and the five lattices on the finest grid, then the penalty's record, GJ and work
 * (whether or not a penalty is asked for); no volume is held: the caller supplies every level */
size_t sift3d_amd_ffd_refine_channels_work_bytes(int ox, int oy, int oz, int dx, int dy, int dz)
{
    const int d[3] = { dx, dy, dz };
    if (ox <= 0 || oy <= 0 || oz <= 0 || !ffd_spacing_ok(dx, dy, dz))
        return 0;
    return ffd_channels_base_bytes(ox, oy, oz, d) + SIFT3D_AMD_JACOBIAN_PENALTY_RECORD_BYTES +
           3 * grid_voxels(sift3d_amd_ffd_lattice_dim(ox, dx), sift3d_amd_ffd_lattice_dim(oy, dy),
                           sift3d_amd_ffd_lattice_dim(oz, dz)) * sizeof(double) +
           sift3d_amd_jacobian_penalty_work_bytes(ox, oy, oz);
}

int sift3d_amd_ffd_refine_channels_device(const sift3d_amd_ffd_level *level, int levels, int nc, const double *A_in,
                                          const sift3d_amd_ffd_refine_params *params,
                                          sift3d_amd_ffd_refine_result *result, float *d_lattice, float *d_field,
                                          void *d_work, void *stream, double jacobian,
                                          sift3d_amd_ffd_penalty *penalty)
{
    static const char what[] = "sift3d_amd_ffd_refine_channels_device";
    ffd_refine_opts o;
    sift3d_amd_ffd_refine_params prm;
    double ref = 1.0;
    size_t work_bytes;
    int l;
    if (!level || !result || !d_lattice || !d_field || !d_work)
        return refuse(what, "NULL argument");
    if (levels < 1 || levels > SIFT3D_AMD_DEMONS_MAX_LEVELS)
        return refuse(what, "levels must be in [1, SIFT3D_AMD_DEMONS_MAX_LEVELS]");
    if (check_channels(what, nc))
        return SIFT3D_FAILURE;
    if (params)
        prm = *params;
    else
        sift3d_amd_ffd_refine_default_params(&prm);
    if (prm.levels != levels)
        return refuse(what, "params->levels must equal levels");
    if (!ffd_params_ok(&prm))
        return refuse(what, "a parameter is out of range");
    if (!isfinite(jacobian) || jacobian < 0)
        return refuse(what, "the Jacobian weight must be finite and not negative");
    if (jacobian != 0 && !penalty)
        return refuse(what, "a Jacobian weight needs the penalty array");
    if (penalty && ffd_jacobian_ref(what, A_in, &ref))
        return SIFT3D_FAILURE;
    work_bytes = sift3d_amd_ffd_refine_channels_work_bytes(level->ox, level->oy, level->oz, prm.spacing[0],
                                                           prm.spacing[1], prm.spacing[2]);
    for (l = 0; l < levels; l++) {
        const sift3d_amd_ffd_level *v = level + l;
        if (!v->d_F || !v->d_M)
            return refuse(what, "NULL level pointer");
        if (check_dims(what, v->ox, v->oy, v->oz) || check_dims(what, v->nx, v->ny, v->nz))
            return SIFT3D_FAILURE;
        if (l && (v->ox != multires_half(v[-1].ox) || v->oy != multires_half(v[-1].oy) ||
                  v->oz != multires_half(v[-1].oz) || v->nx != multires_half(v[-1].nx) ||
                  v->ny != multires_half(v[-1].ny) || v->nz != multires_half(v[-1].nz)))
            return refuse(what, "a level is not the half of the level above");
        if (check_aligned(what, 0, ADDR(v->d_F) | ADDR(v->d_M) | ADDR(v->d_WF) | ADDR(v->d_WM)))
            return SIFT3D_FAILURE;
        if (l) {                                             /* level 0 is checked with the outputs by the body */
            const range_t in[] = { { v->d_F, image_bytes(v->ox, v->oy, v->oz, nc) },
                                   { v->d_M, image_bytes(v->nx, v->ny, v->nz, nc) },
                                   { v->d_WF, v->d_WF ? image_bytes(v->ox, v->oy, v->oz, 1) : 0 },
                                   { v->d_WM, v->d_WM ? image_bytes(v->nx, v->ny, v->nz, 1) : 0 } };
            const range_t out[] = { { d_lattice, image_bytes(sift3d_amd_ffd_lattice_dim(level->ox, prm.spacing[0]),
                                                             sift3d_amd_ffd_lattice_dim(level->oy, prm.spacing[1]),
                                                             sift3d_amd_ffd_lattice_dim(level->oz, prm.spacing[2]), 3) },
                                    { d_field, field_bytes(level->ox, level->oy, level->oz) },
                                    { d_work, work_bytes } };
            if (ranges_aliased(out, 3, in, 4))
                return refuse(what, ALIASED);
        }
    }
    o = (ffd_refine_opts){ .masked = 1, .d_WF = level->d_WF, .d_WM = level->d_WM, .jacobian = jacobian, .ref = ref,
                           .penalty = penalty, .src = level, .nc = nc };
    return ffd_refine(what, level->d_F, level->ox, level->oy, level->oz, level->d_M, level->nx, level->ny, level->nz,
                      A_in, &prm, result, d_lattice, d_field, d_work, stream, &o);
}
