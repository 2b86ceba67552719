/* sift3d_affine_refine.c -- intensity-driven affine refinement: the checked device entry of the normal equations, the
 * Levenberg-Marquardt step and the parameter update on the host, and the driver that iterates them
 * (included at the end of sift3d_host.c, after sift3d_similarity.c).
 *
 * The contract is in include/sift3d_amd.h, "Intensity-driven affine refinement" (the MSD) and "Affine refinement under
 * a linear intensity map (NCC)": two metrics, each with its pass, its record, its cost and its step, and one driver
 * loop over either (affine_metric).  The kernels are in sift3d_affine_refine.hip, reached through the launchers below
 * after the checks here.  Arguments are checked before the device is touched, so bad input is refused on a machine
 * without a GPU too. */

int sift3d_affine_normal_launch(const char *fn, const float *d_F, int ox, int oy, int oz, const float *d_M, int nx,
                                int ny, int nz, const double *A, void *d_record, void *d_work, void *stream,
                                const float *d_WF, const float *d_WM);

int sift3d_affine_ncc_normal_launch(const char *fn, const float *d_F, int ox, int oy, int oz, const float *d_M, int nx,
                                    int ny, int nz, const double *A, void *d_record, void *d_work, void *stream,
                                    const float *d_WF, const float *d_WM);

int sift3d_parzen_hist_launch(const char *fn, const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny,
                              int nz, const double *A, const float *d_field, int bins, float lo_f, float s_f,
                              float lo_m, float hi_m, unsigned long long *d_hist, unsigned long long *d_count, void *d_work,
                              void *stream, const float *d_WF, const float *d_WM);

int sift3d_affine_mi_normal_launch(const char *fn, const float *d_F, int ox, int oy, int oz, const float *d_M, int nx,
                                   int ny, int nz, const double *A, int bins, float lo_f, float s_f, float lo_m,
                                   float hi_m, const double *d_W, void *d_record, void *d_work, void *stream,
                                   const float *d_WF, const float *d_WM);

/* a double per statistic (60 + 12 + 1, and the uint64 count) per partial slot; NCC: 60 + 36 + 5 and the count */
#define AFFINE_NORMAL_WORK_BYTES ((size_t)SIFT3D_AMD_SIMILARITY_GRID * 74 * 8)
#define AFFINE_NCC_WORK_BYTES ((size_t)SIFT3D_AMD_SIMILARITY_GRID * 102 * 8)

size_t sift3d_amd_affine_normal_work_bytes(int ox, int oy, int oz)
{
    if (ox <= 0 || oy <= 0 || oz <= 0)
        return 0;
    return AFFINE_NORMAL_WORK_BYTES;
}

size_t sift3d_amd_affine_ncc_normal_work_bytes(int ox, int oy, int oz)
{
    if (ox <= 0 || oy <= 0 || oz <= 0)
        return 0;
    return AFFINE_NCC_WORK_BYTES;
}

/* the shared body of the three entries: d_WF, d_WM are the masks ("Masks") or NULL; ncc selects the record, the work
 * buffer's size and the launcher */
static int affine_normal_eqs(const char *what, const float *d_F, int ox, int oy, int oz, const float *d_M, int nx,
                             int ny, int nz, const double *A, void *d_record, void *d_work, void *stream,
                             const float *d_WF, const float *d_WM, int ncc)
{
    if (!d_F || !d_M || !A || !d_record || !d_work)
        return refuse(what, "NULL argument");
    if (check_dims(what, ox, oy, oz) || check_dims(what, nx, ny, nz) || check_affine(what, A) ||
        check_aligned(what, ADDR(d_record) | ADDR(d_work), ADDR(d_F) | ADDR(d_M) | ADDR(d_WF) | ADDR(d_WM)))
        return SIFT3D_FAILURE;
    {
        const range_t in[] = { { d_F, image_bytes(ox, oy, oz, 1) }, { d_M, image_bytes(nx, ny, nz, 1) },
                               { d_WF, d_WF ? image_bytes(ox, oy, oz, 1) : 0 },
                               { d_WM, d_WM ? image_bytes(nx, ny, nz, 1) : 0 } };
        const range_t out[] = { { d_record, ncc ? SIFT3D_AMD_AFFINE_NCC_BYTES : SIFT3D_AMD_AFFINE_NORMAL_BYTES },
                                { d_work, ncc ? AFFINE_NCC_WORK_BYTES : AFFINE_NORMAL_WORK_BYTES } };
        if (ranges_aliased(out, 2, in, 4))
            return refuse(what, ALIASED);
    }
    return (ncc ? sift3d_affine_ncc_normal_launch : sift3d_affine_normal_launch)(what, d_F, ox, oy, oz, d_M, nx, ny, nz,
                                                                                 A, d_record, d_work, stream, d_WF,
                                                                                 d_WM);
}

int sift3d_hip_affine_normal_eqs(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                 const double *A, void *d_record, void *d_work, void *stream)
{
    return affine_normal_eqs("sift3d_hip_affine_normal_eqs", d_F, ox, oy, oz, d_M, nx, ny, nz, A, d_record, d_work,
                             stream, NULL, NULL, 0);
}

int sift3d_hip_affine_normal_eqs_masked(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny,
                                        int nz, const double *A, void *d_record, void *d_work, void *stream,
                                        const float *d_WF, const float *d_WM)
{
    return affine_normal_eqs("sift3d_hip_affine_normal_eqs_masked", d_F, ox, oy, oz, d_M, nx, ny, nz, A, d_record,
                             d_work, stream, d_WF, d_WM, 0);
}

int sift3d_hip_affine_ncc_normal_eqs(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny,
                                     int nz, const double *A, void *d_record, void *d_work, void *stream,
                                     const float *d_WF, const float *d_WM)
{
    return affine_normal_eqs("sift3d_hip_affine_ncc_normal_eqs", d_F, ox, oy, oz, d_M, nx, ny, nz, A, d_record,
                             d_work, stream, d_WF, d_WM, 1);
}

/* ---- Mattes mutual information: the window, the histogram pass, the cost and the table, the record pass ---- */
#include "sift3d_parzen.h"

#define PARZEN_HIST_WORK_BYTES ((size_t)SIFT3D_AMD_SIMILARITY_GRID * 8)       /* a uint64 count per partial slot */

static int parzen_bins_ok(int bins)
{
    return bins >= 4 && bins <= SIFT3D_AMD_PARZEN_MAX_BINS;
}

/* bins and the two ranges, refused as "Similarity measures" refuses them; *s_f is the fixed volume's float scale */
static int parzen_check(const char *what, int bins, float lo_f, float hi_f, float lo_m, float hi_m, float *s_f)
{
    if (!parzen_bins_ok(bins))
        return refuse(what, "bins must be in [4, SIFT3D_AMD_PARZEN_MAX_BINS]");
    *s_f = bin_scale(bins, lo_f, hi_f);
    if (*s_f == 0.0f || bin_scale(bins, lo_m, hi_m) == 0.0f)
        return refuse(what, "a range must be finite, lo < hi, and wide enough for bins / (hi - lo) in float");
    return SIFT3D_SUCCESS;
}

int sift3d_amd_parzen_window(float m, float lo, float hi, int bins, int *k0, uint32_t *q, double *dw, int *out)
{
    static const char what[] = "sift3d_amd_parzen_window";
    float s;
    if (!k0 || !q || !dw || !out)
        return refuse(what, "NULL argument");
    if (parzen_check(what, bins, lo, hi, lo, hi, &s))
        return SIFT3D_FAILURE;
    parzen_window(m, lo, parzen_scale(lo, hi, bins), bins, k0, q, dw, out);
    return SIFT3D_SUCCESS;
}

size_t sift3d_amd_parzen_hist_work_bytes(int ox, int oy, int oz)
{
    if (ox <= 0 || oy <= 0 || oz <= 0)
        return 0;
    return PARZEN_HIST_WORK_BYTES;
}

/* the shared body of the two entries: the pull map is A, or with A == NULL the field d_field [3][oz][oy][ox] */
static int parzen_hist(const char *what, const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny,
                       int nz, const double *A, const float *d_field, int bins, float lo_f, float hi_f, float lo_m,
                       float hi_m, uint64_t *d_hist, uint64_t *d_count, void *d_work, void *stream, const float *d_WF,
                       const float *d_WM)
{
    float s_f;
    if (!d_F || !d_M || (!A && !d_field) || !d_hist || !d_count || !d_work)
        return refuse(what, "NULL argument");
    if (check_dims(what, ox, oy, oz) || check_dims(what, nx, ny, nz) ||
        parzen_check(what, bins, lo_f, hi_f, lo_m, hi_m, &s_f) || (A && check_affine(what, A)) ||
        check_aligned(what, ADDR(d_hist) | ADDR(d_count) | ADDR(d_work),
                      ADDR(d_F) | ADDR(d_M) | ADDR(d_field) | ADDR(d_WF) | ADDR(d_WM)))
        return SIFT3D_FAILURE;
    {
        const range_t in[] = { { d_F, image_bytes(ox, oy, oz, 1) }, { d_M, image_bytes(nx, ny, nz, 1) },
                               { d_WF, d_WF ? image_bytes(ox, oy, oz, 1) : 0 },
                               { d_WM, d_WM ? image_bytes(nx, ny, nz, 1) : 0 },
                               { d_field, d_field ? field_bytes(ox, oy, oz) : 0 } };
        const range_t out[] = { { d_hist, (size_t)bins * bins * sizeof(uint64_t) }, { d_count, sizeof(uint64_t) },
                                { d_work, PARZEN_HIST_WORK_BYTES } };
        if (ranges_aliased(out, 3, in, 5))
            return refuse(what, ALIASED);
    }
    return sift3d_parzen_hist_launch(what, d_F, ox, oy, oz, d_M, nx, ny, nz, A, d_field, bins, lo_f, s_f, lo_m, hi_m,
                                     (unsigned long long *)d_hist, (unsigned long long *)d_count, d_work, stream,
                                     d_WF, d_WM);
}

int sift3d_hip_parzen_hist_affine(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                  const double *A, int bins, float lo_f, float hi_f, float lo_m, float hi_m,
                                  uint64_t *d_hist, uint64_t *d_count, void *d_work, void *stream, const float *d_WF,
                                  const float *d_WM)
{
    static const char what[] = "sift3d_hip_parzen_hist_affine";
    if (!A)
        return refuse(what, "NULL argument");
    return parzen_hist(what, d_F, ox, oy, oz, d_M, nx, ny, nz, A, NULL, bins, lo_f, hi_f, lo_m, hi_m, d_hist, d_count,
                       d_work, stream, d_WF, d_WM);
}

/* "Mutual-information free-form deformation (Mattes)": the same histogram with the sample point of a field */
int sift3d_hip_parzen_hist_field(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                 const float *d_field, int bins, float lo_f, float hi_f, float lo_m, float hi_m,
                                 uint64_t *d_hist, uint64_t *d_count, void *d_work, void *stream, const float *d_WF,
                                 const float *d_WM)
{
    static const char what[] = "sift3d_hip_parzen_hist_field";
    if (!d_field)
        return refuse(what, "NULL argument");
    return parzen_hist(what, d_F, ox, oy, oz, d_M, nx, ny, nz, NULL, d_field, bins, lo_f, hi_f, lo_m, hi_m, d_hist,
                       d_count, d_work, stream, d_WF, d_WM);
}

int sift3d_amd_parzen_mi(const uint64_t *hist, int bins, sift3d_amd_similarity *out, double *W)
{
    static const char what[] = "sift3d_amd_parzen_mi";
    uint64_t r[SIFT3D_AMD_PARZEN_MAX_BINS], c[SIFT3D_AMD_PARZEN_MAX_BINS], total = 0;
    int i, j;
    if (!hist || !out)
        return refuse(what, "NULL argument");
    if (!parzen_bins_ok(bins))
        return refuse(what, "bins must be in [4, SIFT3D_AMD_PARZEN_MAX_BINS]");
    marginals(hist, bins, r, c);
    for (i = 0; i < bins; i++)
        total += r[i];
    out->n = total;
    out->msd = out->ncc = NAN;
    if (total == 0)
        out->mi = out->nmi = out->entropy_fixed = out->entropy_moving = out->entropy_joint = NAN;
    else
        entropy_measures(hist, bins, r, c, total, out);
    if (W)
        for (i = 0; i < bins; i++)
            for (j = 0; j < bins; j++) {
                const uint64_t h = hist[(size_t)i * bins + j];
                W[(size_t)i * bins + j] = h ? log((double)h / (double)c[j]) : 0.0;
            }
    return SIFT3D_SUCCESS;
}

int sift3d_hip_affine_mi_normal_eqs(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                    const double *A, int bins, float lo_f, float hi_f, float lo_m, float hi_m,
                                    const double *d_W, void *d_record, void *d_work, void *stream, const float *d_WF,
                                    const float *d_WM)
{
    static const char what[] = "sift3d_hip_affine_mi_normal_eqs";
    float s_f;
    if (!d_F || !d_M || !A || !d_W || !d_record || !d_work)
        return refuse(what, "NULL argument");
    if (check_dims(what, ox, oy, oz) || check_dims(what, nx, ny, nz) ||
        parzen_check(what, bins, lo_f, hi_f, lo_m, hi_m, &s_f) || check_affine(what, A) ||
        check_aligned(what, ADDR(d_record) | ADDR(d_work) | ADDR(d_W),
                      ADDR(d_F) | ADDR(d_M) | ADDR(d_WF) | ADDR(d_WM)))
        return SIFT3D_FAILURE;
    {
        const range_t in[] = { { d_F, image_bytes(ox, oy, oz, 1) }, { d_M, image_bytes(nx, ny, nz, 1) },
                               { d_WF, d_WF ? image_bytes(ox, oy, oz, 1) : 0 },
                               { d_WM, d_WM ? image_bytes(nx, ny, nz, 1) : 0 },
                               { d_W, (size_t)bins * bins * sizeof(double) } };
        const range_t out[] = { { d_record, SIFT3D_AMD_AFFINE_NORMAL_BYTES }, { d_work, AFFINE_NORMAL_WORK_BYTES } };
        if (ranges_aliased(out, 2, in, 5))
            return refuse(what, ALIASED);
    }
    return sift3d_affine_mi_normal_launch(what, d_F, ox, oy, oz, d_M, nx, ny, nz, A, bins, lo_f, s_f, lo_m, hi_m, d_W,
                                          d_record, d_work, stream, d_WF, d_WM);
}

/* ---- host arithmetic on a record (the order of every operation is the header's) ---- */

typedef struct {
    uint64_t n;
    double see, b[12], H[144];
} affine_record;

typedef struct {
    uint64_t n;
    double S_m, S_f, S_mm, S_fm, S_ff, u[12], v[12], w[12], H[144];
} affine_ncc_record;

#define LM_MAX 14                                            /* the 12 parameters, and alpha and beta */

/* K x = y for the m x m matrix whose lower triangle is in K (row stride LM_MAX), factored in place: K = C C^T row by
 * row, then the two triangular solves; x replaces y.  -1 when K is not positive definite (a zero on the
 * diagonal included) or the solution is not finite. */
static int cholesky_solve(double *K, int m, double *y)
{
    int i, j, k;
    for (i = 0; i < m; i++) {
        for (j = 0; j <= i; j++) {
            double s = K[i * LM_MAX + j];
            for (k = 0; k < j; k++)
                s -= K[i * LM_MAX + k] * K[j * LM_MAX + k];
            if (i == j) {
                if (!(s > 0.0) || !isfinite(s))
                    return SIFT3D_FAILURE;
                K[i * LM_MAX + i] = sqrt(s);
            } else
                K[i * LM_MAX + j] = s / K[j * LM_MAX + j];
        }
    }
    for (i = 0; i < m; i++) {                                /* C z = y */
        double s = y[i];
        for (k = 0; k < i; k++)
            s -= K[i * LM_MAX + k] * y[k];
        y[i] = s / K[i * LM_MAX + i];
    }
    for (i = m - 1; i >= 0; i--) {                           /* C^T x = z */
        double s = y[i];
        for (k = i + 1; k < m; k++)
            s -= K[k * LM_MAX + i] * y[k];
        y[i] = s / K[i * LM_MAX + i];
        if (!isfinite(y[i]))
            return SIFT3D_FAILURE;
    }
    return SIFT3D_SUCCESS;
}

/* the checks the two steps share, and the free parameters among the 12 in idx; their number, 0 to refuse */
static int lm_free_set(const char *what, const void *record, unsigned free_mask, double lambda, double *delta, int *idx)
{
    int m = 0, i;
    if (!record || !delta)
        return refuse(what, "NULL argument"), 0;
    if (!isfinite(lambda) || lambda < 0)
        return refuse(what, "lambda must be finite and not negative"), 0;
    for (i = 0; i < 12; i++) {
        delta[i] = 0.0;
        if (free_mask & (1u << i))
            idx[m++] = i;
    }
    return free_mask & ~0xFFFu ? 0 : m;
}

int sift3d_amd_affine_lm_step(const void *record, unsigned free_mask, double lambda, double *delta)
{
    affine_record r;
    double K[LM_MAX * LM_MAX], y[LM_MAX];
    int idx[LM_MAX], i, j;
    const int m = lm_free_set("sift3d_amd_affine_lm_step", record, free_mask, lambda, delta, idx);
    if (m == 0)
        return SIFT3D_FAILURE;
    memcpy(&r, record, sizeof(r));
    if (r.n == 0)
        return SIFT3D_FAILURE;
    /* K = H + lambda diag H on the free set (its lower triangle), K delta = -b */
    for (i = 0; i < m; i++) {
        for (j = 0; j <= i; j++) {
            const double h = r.H[idx[i] * 12 + idx[j]];
            K[i * LM_MAX + j] = i == j ? h + lambda * h : h;
        }
        y[i] = -r.b[idx[i]];
    }
    if (cholesky_solve(K, m, y))
        return SIFT3D_FAILURE;
    for (i = 0; i < m; i++)
        delta[idx[i]] = y[i];
    return SIFT3D_SUCCESS;
}

/* out = alpha, beta, cost, ncc of the record's sums, in the header's order of operations; 0 where the fit is undefined
 * (out is then all NaN) */
static int ncc_fit(const affine_ncc_record *r, double *out)
{
    const double nd = (double)r->n;
    double vm, vf, c, alpha;
    out[0] = out[1] = out[2] = out[3] = NAN;
    if (r->n < 2)
        return 0;
    vm = r->S_mm - r->S_m * r->S_m / nd;
    vf = r->S_ff - r->S_f * r->S_f / nd;
    c = r->S_fm - r->S_f * r->S_m / nd;
    if (!(vm > 0))
        return 0;
    alpha = c / vm;
    out[0] = alpha;
    out[1] = (r->S_f - alpha * r->S_m) / nd;
    out[2] = (vf - alpha * c) / nd;
    if (!(out[2] >= 0))
        out[2] = 0.0;
    out[3] = vf <= 0 || vm <= 0 ? 0.0 : c / sqrt(vf * vm);
    return 1;
}

int sift3d_amd_affine_ncc_fit(const void *record, double *out)
{
    affine_ncc_record r;
    if (!record || !out)
        return refuse("sift3d_amd_affine_ncc_fit", "NULL argument");
    memcpy(&r, record, sizeof(r));
    return ncc_fit(&r, out) ? SIFT3D_SUCCESS : SIFT3D_FAILURE;
}

int sift3d_amd_affine_ncc_lm_step(const void *record, unsigned free_mask, double lambda, double *delta)
{
    affine_ncc_record r;
    double K[LM_MAX * LM_MAX], y[LM_MAX], fit[4], alpha, beta, nd;
    int idx[LM_MAX], i, j;
    int m = lm_free_set("sift3d_amd_affine_ncc_lm_step", record, free_mask, lambda, delta, idx);
    if (m == 0)
        return SIFT3D_FAILURE;
    memcpy(&r, record, sizeof(r));
    if (!ncc_fit(&r, fit))
        return SIFT3D_FAILURE;                              /* n < 2 or V_m <= 0 */
    alpha = fit[0];
    beta = fit[1];
    nd = (double)r.n;
    idx[m++] = 12;                                           /* alpha and beta are always free */
    idx[m++] = 13;
    /* K = H14 + lambda diag H14 on the free set (its lower triangle), K delta = -b14 */
    for (i = 0; i < m; i++) {
        const int p = idx[i];
        for (j = 0; j <= i; j++) {
            const int q = idx[j];                            /* q <= p */
            const double h = p < 12    ? (alpha * alpha) * r.H[p * 12 + q]
                             : p == 12 ? (q < 12 ? alpha * r.v[q] : r.S_mm)
                                       : (q < 12 ? alpha * r.u[q] : q == 12 ? r.S_m : nd);
            K[i * LM_MAX + j] = i == j ? h + lambda * h : h;
        }
        y[i] = -(p < 12    ? alpha * ((alpha * r.v[p] + beta * r.u[p]) - r.w[p])
                 : p == 12 ? (alpha * r.S_mm + beta * r.S_m) - r.S_fm
                           : (alpha * r.S_m + beta * nd) - r.S_f);
    }
    if (cholesky_solve(K, m, y))
        return SIFT3D_FAILURE;                              /* alpha == 0 makes it so */
    for (i = 0; i < m - 2; i++)
        delta[idx[i]] = y[i];
    return SIFT3D_SUCCESS;
}

int sift3d_amd_affine_apply_delta(const double *A, const double *delta, int ox, int oy, int oz, double *A_out)
{
    static const char what[] = "sift3d_amd_affine_apply_delta";
    double c[3], out[12];
    int d, j;
    if (!A || !delta || !A_out)
        return refuse(what, "NULL argument");
    if (check_dims(what, ox, oy, oz))
        return SIFT3D_FAILURE;
    c[0] = (double)(ox - 1) / 2.0;
    c[1] = (double)(oy - 1) / 2.0;
    c[2] = (double)(oz - 1) / 2.0;
    for (d = 0; d < 3; d++) {
        const double *a = A + 4 * d;
        double *o = out + 4 * d;
        const double t = a[3] + ((a[0] * c[0] + a[1] * c[1]) + a[2] * c[2]);
        for (j = 0; j < 3; j++)
            o[j] = a[j] + delta[4 * d + j];
        o[3] = (t + delta[4 * d + 3]) - ((o[0] * c[0] + o[1] * c[1]) + o[2] * c[2]);
    }
    memcpy(A_out, out, sizeof(out));
    return SIFT3D_SUCCESS;
}

/* ---- the driver ---- */

void sift3d_amd_affine_refine_default_params(sift3d_amd_affine_refine_params *p)
{
    if (!p)
        return;
    p->free_mask = 0xFFF;
    p->levels = 1;
    p->max_evaluations = 30;
    p->lambda0 = 1e-3;
    p->lambda_factor = 10.0;
    p->lambda_min = 1e-9;
    p->lambda_max = 1e7;
    p->tol = 1e-3;
    p->min_overlap = 0.5;
}

static int affine_params_ok(const sift3d_amd_affine_refine_params *p)
{
    return p->free_mask >= 1 && p->free_mask <= 0xFFF && p->levels >= 1 && p->levels <= SIFT3D_AMD_DEMONS_MAX_LEVELS &&
           p->max_evaluations >= 1 && p->max_evaluations <= SIFT3D_AMD_AFFINE_MAX_EVALUATIONS &&
           isfinite(p->lambda0) && p->lambda0 > 0 && isfinite(p->lambda_factor) && p->lambda_factor > 1 &&
           isfinite(p->lambda_min) && p->lambda_min > 0 && isfinite(p->lambda_max) && p->lambda_max >= p->lambda0 &&
           isfinite(p->tol) && p->tol >= 0 && p->min_overlap >= 0 && p->min_overlap <= 1;
}

size_t sift3d_amd_affine_refine_struct_bytes(int which)
{
    return which == 0   ? sizeof(sift3d_amd_affine_refine_params)
           : which == 1 ? sizeof(sift3d_amd_affine_evaluation)
           : which == 2 ? sizeof(sift3d_amd_affine_refine_result)
           : which == 3 ? (size_t)SIFT3D_AMD_AFFINE_NORMAL_BYTES
           : which == 4 ? (size_t)SIFT3D_AMD_AFFINE_MAX_EVALUATIONS
           : which == 5 ? (size_t)SIFT3D_AMD_DEMONS_MAX_LEVELS
                        : 0;
}

/* ---- the two metrics of the driver ---- */
typedef union {
    uint64_t n;                                              /* both records begin with the count */
    affine_record msd;
    affine_ncc_record ncc;
} affine_eval;

static double msd_cost(const affine_eval *e)
{
    return e->n ? e->msd.see / (double)e->n : NAN;
}

static double ncc_cost(const affine_eval *e)
{
    double fit[4];
    ncc_fit(&e->ncc, fit);
    return fit[2];                                           /* NaN where the fit is undefined */
}

typedef struct {
    int ncc;                                                 /* which pass affine_normal_eqs launches */
    int mi;                                                  /* an evaluation is the histogram pass (mi_state) */
    size_t record_bytes, normal_work_bytes;
    size_t extra_bytes;                                      /* of d_work behind the record (MI: hist, count, W) */
    double (*cost)(const affine_eval *);                     /* what a step must lower; NaN: never accepted */
    int (*step)(const void *record, unsigned free_mask, double lambda, double *delta);
} affine_metric;

/* MI, behind the record: the histogram [MAX][MAX] uint64 and the count (copied to the host together), padded to 16
 * bytes, then W [MAX][MAX] double; the sizes are those of SIFT3D_AMD_PARZEN_MAX_BINS whatever `bins` is */
#define MI_TABLE_BYTES ((size_t)SIFT3D_AMD_PARZEN_MAX_BINS * SIFT3D_AMD_PARZEN_MAX_BINS * 8)
#define MI_EXTRA_BYTES (2 * MI_TABLE_BYTES + 16)

static const affine_metric METRIC_MSD = { 0, 0, SIFT3D_AMD_AFFINE_NORMAL_BYTES, AFFINE_NORMAL_WORK_BYTES, 0, msd_cost,
                                          sift3d_amd_affine_lm_step };
static const affine_metric METRIC_NCC = { 1, 0, SIFT3D_AMD_AFFINE_NCC_BYTES, AFFINE_NCC_WORK_BYTES, 0, ncc_cost,
                                          sift3d_amd_affine_ncc_lm_step };
static const affine_metric METRIC_MI = { 0, 1, SIFT3D_AMD_AFFINE_NORMAL_BYTES, AFFINE_NORMAL_WORK_BYTES,
                                         MI_EXTRA_BYTES, NULL, sift3d_amd_affine_lm_step };

/* what the MI driver carries from evaluation to evaluation */
typedef struct {
    int bins;
    float lo_f, hi_f, lo_m, hi_m;
    uint64_t *d_hist;                                        /* in d_work: [bins][bins], then the count */
    double *d_W;                                             /* in d_work */
    uint64_t hist[SIFT3D_AMD_PARZEN_MAX_BINS * SIFT3D_AMD_PARZEN_MAX_BINS + 1];     /* the last evaluation's, and count */
    double W[SIFT3D_AMD_PARZEN_MAX_BINS * SIFT3D_AMD_PARZEN_MAX_BINS];              /* the last evaluation's table */
    sift3d_amd_similarity sim, sim_trial;                    /* measures at A; at the last evaluation */
} mi_state;

/* d_work, in bytes: the normal equations' partial slots, the record, then per level l = 1 .. levels-1 the restricted
 * fixed and moving volumes, each rounded up to a multiple of 16 bytes */
static size_t affine_record_pad(const affine_metric *mt)
{
    return (mt->record_bytes + 15) / 16 * 16 + mt->extra_bytes;
}

static size_t affine_work_bytes(const affine_metric *mt, int ox, int oy, int oz, int nx, int ny, int nz, int levels)
{
    size_t total = mt->normal_work_bytes + affine_record_pad(mt);
    int l;
    if (ox <= 0 || oy <= 0 || oz <= 0 || nx <= 0 || ny <= 0 || nz <= 0 || levels < 1 ||
        levels > SIFT3D_AMD_DEMONS_MAX_LEVELS)
        return 0;
    for (l = 1; l < levels; l++) {
        ox = multires_half(ox); oy = multires_half(oy); oz = multires_half(oz);
        nx = multires_half(nx); ny = multires_half(ny); nz = multires_half(nz);
        total += pad4(grid_voxels(ox, oy, oz)) * sizeof(float) + pad4(grid_voxels(nx, ny, nz)) * sizeof(float);
    }
    return total;
}

size_t sift3d_amd_affine_refine_work_bytes(int ox, int oy, int oz, int nx, int ny, int nz, int levels)
{
    return affine_work_bytes(&METRIC_MSD, ox, oy, oz, nx, ny, nz, levels);
}

/* ---- the mask pyramid of the two masked drivers (this one and sift3d_ffd.c's): the layout rule, stated once ----
 * Per level l = 1 .. levels-1, behind that level's restricted fixed and moving volumes: the fixed mask, then the
 * moving mask, each present only where the caller gave one, each rounded up to a multiple of 16 bytes. */

/* room for both masks on every level below the first (dims > 0, levels >= 1: checked by the callers) */
static size_t mask_pyramid_bytes(int ox, int oy, int oz, int nx, int ny, int nz, int levels)
{
    size_t total = 0;
    int l;
    for (l = 1; l < levels; l++) {
        ox = multires_half(ox); oy = multires_half(oy); oz = multires_half(oz);
        nx = multires_half(nx); ny = multires_half(ny); nz = multires_half(nz);
        total += pad4(grid_voxels(ox, oy, oz)) * sizeof(float) + pad4(grid_voxels(nx, ny, nz)) * sizeof(float);
    }
    return total;
}

/* One level's masks at w + *off from the FLOAT masks of the level above (never a thresholded copy), by
 * sift3d_hip_restrict2 at scale 1; a NULL mask stays NULL and takes no room.  (fo.., fn..: the grids of the level
 * above.)  *off moves past what was written. */
static int mask_pyramid_level(const float *fWF, int fox, int foy, int foz, const float *fWM, int fnx, int fny, int fnz,
                              char *w, size_t *off, const float **cWF, const float **cWM, void *stream)
{
    *cWF = *cWM = NULL;
    if (fWF) {
        float *c = (float *)(w + *off);
        *off += pad4(grid_voxels(multires_half(fox), multires_half(foy), multires_half(foz))) * sizeof(float);
        if (sift3d_hip_restrict2(fWF, fox, foy, foz, 1, c, 1.0f, stream))
            return SIFT3D_FAILURE;
        *cWF = c;
    }
    if (fWM) {
        float *c = (float *)(w + *off);
        *off += pad4(grid_voxels(multires_half(fnx), multires_half(fny), multires_half(fnz))) * sizeof(float);
        if (sift3d_hip_restrict2(fWM, fnx, fny, fnz, 1, c, 1.0f, stream))
            return SIFT3D_FAILURE;
        *cWM = c;
    }
    return SIFT3D_SUCCESS;
}

/* the drivers that take masks: the same, and the mask pyramid */
static size_t affine_masked_work_bytes(const affine_metric *mt, int ox, int oy, int oz, int nx, int ny, int nz,
                                       int levels)
{
    const size_t plain = affine_work_bytes(mt, ox, oy, oz, nx, ny, nz, levels);
    return plain ? plain + mask_pyramid_bytes(ox, oy, oz, nx, ny, nz, levels) : 0;
}

size_t sift3d_amd_affine_refine_masked_work_bytes(int ox, int oy, int oz, int nx, int ny, int nz, int levels)
{
    return affine_masked_work_bytes(&METRIC_MSD, ox, oy, oz, nx, ny, nz, levels);
}

size_t sift3d_amd_affine_ncc_refine_work_bytes(int ox, int oy, int oz, int nx, int ny, int nz, int levels)
{
    return affine_masked_work_bytes(&METRIC_NCC, ox, oy, oz, nx, ny, nz, levels);
}

size_t sift3d_amd_affine_mi_refine_work_bytes(int ox, int oy, int oz, int nx, int ny, int nz, int levels)
{
    return affine_masked_work_bytes(&METRIC_MI, ox, oy, oz, nx, ny, nz, levels);
}

/* the largest distance by which the maps A and B move a corner of the grid apart */
static double affine_corner_move(const double *A, const double *B, int ox, int oy, int oz)
{
    double worst = 0.0;
    int c, d;
    for (c = 0; c < 8; c++) {
        const double x = c & 1 ? ox - 1 : 0, y = c & 2 ? oy - 1 : 0, z = c & 4 ? oz - 1 : 0;
        double s = 0.0;
        for (d = 0; d < 3; d++) {
            const double *a = A + 4 * d, *b = B + 4 * d;
            const double e = (b[0] - a[0]) * x + (((b[1] - a[1]) * y + (b[2] - a[2]) * z) + (b[3] - a[3]));
            s += e * e;
        }
        s = sqrt(s);
        if (!(s <= worst))
            worst = s;                                      /* a NaN is the largest */
    }
    return worst;
}

typedef struct {
    const float *F, *M;
    int ox, oy, oz, nx, ny, nz;
    const float *WF, *WM;                                    /* the level's masks, or NULL */
} affine_level;

/* one evaluation at A on `lv`: the metric's pass, the record's copy to the host and the wait for it, and the cost.
 * MI: the histogram pass, histogram and count to the host, sift3d_amd_parzen_mi; rec holds the count alone (the rest
 * zero) until mi_record fills it, ms->W the table and ms->sim_trial the measures. */
static int affine_evaluate(const affine_metric *mt, mi_state *ms, const affine_level *lv, const double *A,
                           void *d_record, void *d_work, void *stream, affine_eval *rec, double *cost)
{
    const char *what = mt->ncc               ? "sift3d_hip_affine_ncc_normal_eqs"
                       : lv->WF || lv->WM ? "sift3d_hip_affine_normal_eqs_masked"
                                          : "sift3d_hip_affine_normal_eqs";
    if (mt->mi) {
        const size_t cells = (size_t)ms->bins * ms->bins;
        if (sift3d_hip_parzen_hist_affine(lv->F, lv->ox, lv->oy, lv->oz, lv->M, lv->nx, lv->ny, lv->nz, A, ms->bins,
                                          ms->lo_f, ms->hi_f, ms->lo_m, ms->hi_m, ms->d_hist, ms->d_hist + cells,
                                          d_work, stream, lv->WF, lv->WM) ||
            sift3d_hip_memcpy_d2h(ms->hist, ms->d_hist, (cells + 1) * sizeof(uint64_t), stream) ||
            sift3d_hip_stream_sync(stream) || sift3d_amd_parzen_mi(ms->hist, ms->bins, &ms->sim_trial, ms->W))
            return SIFT3D_FAILURE;
        memset(rec, 0, sizeof(*rec));
        rec->n = ms->hist[cells];
        *cost = -ms->sim_trial.mi;                           /* NaN when nothing was counted */
        return SIFT3D_SUCCESS;
    }
    if (affine_normal_eqs(what, lv->F, lv->ox, lv->oy, lv->oz, lv->M, lv->nx, lv->ny, lv->nz, A, d_record, d_work,
                          stream, lv->WF, lv->WM, mt->ncc) ||
        sift3d_hip_memcpy_d2h(rec, d_record, mt->record_bytes, stream) || sift3d_hip_stream_sync(stream))
        return SIFT3D_FAILURE;
    *cost = mt->cost(rec);
    return SIFT3D_SUCCESS;
}

/* MI: the record at A, the map of the evaluation that left its table in ms->W: W to the device, the record pass, the
 * record to the host and the wait for it */
static int mi_record(mi_state *ms, const affine_level *lv, const double *A, void *d_record, void *d_work, void *stream,
                     affine_eval *rec)
{
    return sift3d_hip_memcpy_h2d(ms->d_W, ms->W, (size_t)ms->bins * ms->bins * sizeof(double), stream) ||
           sift3d_hip_affine_mi_normal_eqs(lv->F, lv->ox, lv->oy, lv->oz, lv->M, lv->nx, lv->ny, lv->nz, A, ms->bins,
                                           ms->lo_f, ms->hi_f, ms->lo_m, ms->hi_m, ms->d_W, d_record, d_work, stream,
                                           lv->WF, lv->WM) ||
           sift3d_hip_memcpy_d2h(&rec->msd, d_record, SIFT3D_AMD_AFFINE_NORMAL_BYTES, stream) ||
           sift3d_hip_stream_sync(stream);
}

static void affine_trail(sift3d_amd_affine_refine_result *res, uint64_t n, double cost, double lambda, int accepted,
                         int level)
{
    sift3d_amd_affine_evaluation *e = res->trail + res->evaluations++;
    e->msd = cost;
    e->n = n;
    e->lambda = lambda;
    e->accepted = accepted;
    e->level = level;
}

/* the shared body of the four drivers: `masked` selects the work buffer's size; the masks may still be NULL.  fit_out
 * (NCC; else NULL): the fit at the final A on level 0, NaN where it is undefined or no evaluation was made.  ms (MI;
 * else NULL): bins and ranges, checked by the caller; ms->sim leaves with the measures at the final A on level 0. */
static int affine_refine(const affine_metric *mt, const char *what, const float *d_F, int ox, int oy, int oz,
                         const float *d_M, int nx, int ny, int nz, double *A_io,
                         const sift3d_amd_affine_refine_params *params, sift3d_amd_affine_refine_result *result,
                         double *fit_out, void *d_work, void *stream, int masked, const float *d_WF,
                         const float *d_WM, mi_state *ms)
{
    sift3d_amd_affine_refine_params prm;
    affine_level lv[SIFT3D_AMD_DEMONS_MAX_LEVELS];
    affine_eval rec, trial;
    double A[12], At[12], delta[12], cost, cost_t;
    char *w = (char *)d_work;
    void *d_record;
    size_t off;
    int l, i;
    if (!d_F || !d_M || !A_io || !result || !d_work || (mt->ncc && !fit_out))
        return refuse(what, "NULL argument");
    if (params)
        prm = *params;
    else
        sift3d_amd_affine_refine_default_params(&prm);
    if (check_dims(what, ox, oy, oz) || check_dims(what, nx, ny, nz) || check_affine(what, A_io))
        return SIFT3D_FAILURE;
    if (!affine_params_ok(&prm))
        return refuse(what, "a parameter is out of range");
    if (check_aligned(what, ADDR(d_work), ADDR(d_F) | ADDR(d_M) | ADDR(d_WF) | ADDR(d_WM)))
        return SIFT3D_FAILURE;
    {
        const range_t in[] = { { d_F, image_bytes(ox, oy, oz, 1) }, { d_M, image_bytes(nx, ny, nz, 1) },
                               { d_WF, d_WF ? image_bytes(ox, oy, oz, 1) : 0 },
                               { d_WM, d_WM ? image_bytes(nx, ny, nz, 1) : 0 } };
        size_t (*const bytes_of)(const affine_metric *, int, int, int, int, int, int, int) =
            masked ? affine_masked_work_bytes : affine_work_bytes;
        const range_t out[] = { { d_work, bytes_of(mt, ox, oy, oz, nx, ny, nz, prm.levels) } };
        if (ranges_aliased(out, 1, in, 4))
            return refuse(what, ALIASED);
    }
    result->evaluations = 0;
    result->stop = SIFT3D_AMD_AFFINE_STOP_EVALUATIONS;
    memcpy(result->A, A_io, sizeof(result->A));
    if (fit_out)
        fit_out[0] = fit_out[1] = fit_out[2] = fit_out[3] = NAN;
    d_record = w + mt->normal_work_bytes;
    off = mt->normal_work_bytes + affine_record_pad(mt);
    if (ms) {
        ms->d_hist = (uint64_t *)(w + off - MI_EXTRA_BYTES);
        ms->d_W = (double *)(w + off - MI_TABLE_BYTES);
    }
    lv[0] = (affine_level){ d_F, d_M, ox, oy, oz, nx, ny, nz, d_WF, d_WM };
    memcpy(A, A_io, sizeof(A));
    for (l = 1; l < prm.levels; l++) {                       /* level l from level l - 1; A's shift halves */
        const affine_level *f = lv + l - 1;
        affine_level *c = lv + l;
        float *cF = (float *)(w + off), *cM;
        *c = (affine_level){ NULL, NULL, multires_half(f->ox), multires_half(f->oy), multires_half(f->oz),
                             multires_half(f->nx), multires_half(f->ny), multires_half(f->nz), NULL, NULL };
        off += pad4(grid_voxels(c->ox, c->oy, c->oz)) * sizeof(float);
        cM = (float *)(w + off);
        off += pad4(grid_voxels(c->nx, c->ny, c->nz)) * sizeof(float);
        if (sift3d_hip_restrict2(f->F, f->ox, f->oy, f->oz, 1, cF, 1.0f, stream) ||
            sift3d_hip_restrict2(f->M, f->nx, f->ny, f->nz, 1, cM, 1.0f, stream))
            return SIFT3D_FAILURE;
        c->F = cF;
        c->M = cM;
        if (mask_pyramid_level(f->WF, f->ox, f->oy, f->oz, f->WM, f->nx, f->ny, f->nz, w, &off, &c->WF, &c->WM, stream))
            return SIFT3D_FAILURE;
        for (i = 3; i < 12; i += 4)
            A[i] = A[i] * 0.5;
    }
    for (l = prm.levels - 1; l >= 0; l--) {
        const affine_level *v = lv + l;
        double lambda = prm.lambda0;
        uint64_t n_first;
        int evals = 1, stop;
        int stale = mt->mi;                                  /* MI: rec holds no record of A yet */
        if (affine_evaluate(mt, ms, v, A, d_record, w, stream, &rec, &cost))
            return SIFT3D_FAILURE;
        if (ms)
            ms->sim = ms->sim_trial;
        affine_trail(result, rec.n, cost, lambda, 1, l);
        n_first = rec.n;
        for (;;) {
            int accept;
            if (evals >= prm.max_evaluations) {
                stop = SIFT3D_AMD_AFFINE_STOP_EVALUATIONS;
                break;
            }
            if (stale) {                                     /* the record of the map this step starts from; ms->W
                                                                is still that map's: no evaluation was made since */
                if (rec.n && mi_record(ms, v, A, d_record, w, stream, &rec))
                    return SIFT3D_FAILURE;
                stale = 0;
            }
            if (mt->step(&rec, prm.free_mask, lambda, delta) ||
                sift3d_amd_affine_apply_delta(A, delta, v->ox, v->oy, v->oz, At) || check_affine(what, At)) {
                stop = SIFT3D_AMD_AFFINE_STOP_LM_FAILED;
                break;
            }
            if (affine_evaluate(mt, ms, v, At, d_record, w, stream, &trial, &cost_t))
                return SIFT3D_FAILURE;
            evals++;
            accept = trial.n > 0 && (double)trial.n >= prm.min_overlap * (double)n_first && cost_t < cost;
            affine_trail(result, trial.n, cost_t, lambda, accept, l);
            if (accept) {
                const double move = affine_corner_move(A, At, v->ox, v->oy, v->oz);
                memcpy(A, At, sizeof(A));
                rec = trial;
                cost = cost_t;
                stale = mt->mi;
                if (ms)
                    ms->sim = ms->sim_trial;
                lambda = lambda / prm.lambda_factor;
                if (lambda < prm.lambda_min)
                    lambda = prm.lambda_min;
                if (move < prm.tol) {
                    stop = SIFT3D_AMD_AFFINE_STOP_CONVERGED;
                    break;
                }
            } else {
                lambda = lambda * prm.lambda_factor;
                if (lambda > prm.lambda_max) {
                    stop = SIFT3D_AMD_AFFINE_STOP_LAMBDA;
                    break;
                }
            }
        }
        result->stop = stop;
        if (l > 0)
            for (i = 3; i < 12; i += 4)
                A[i] = A[i] * 2.0;
    }
    memcpy(A_io, A, sizeof(A));
    memcpy(result->A, A, sizeof(A));
    if (fit_out)
        ncc_fit(&rec.ncc, fit_out);                          /* level 0's last accepted evaluation: the record at A */
    return SIFT3D_SUCCESS;
}

int sift3d_amd_affine_refine_device(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                    double *A_io, const sift3d_amd_affine_refine_params *params,
                                    sift3d_amd_affine_refine_result *result, void *d_work, void *stream)
{
    return affine_refine(&METRIC_MSD, "sift3d_amd_affine_refine_device", d_F, ox, oy, oz, d_M, nx, ny, nz, A_io, params,
                         result, NULL, d_work, stream, 0, NULL, NULL, NULL);
}

int sift3d_amd_affine_refine_masked_device(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny,
                                           int nz, double *A_io, const sift3d_amd_affine_refine_params *params,
                                           sift3d_amd_affine_refine_result *result, void *d_work, void *stream,
                                           const float *d_WF, const float *d_WM)
{
    return affine_refine(&METRIC_MSD, "sift3d_amd_affine_refine_masked_device", d_F, ox, oy, oz, d_M, nx, ny, nz, A_io,
                         params, result, NULL, d_work, stream, 1, d_WF, d_WM, NULL);
}

int sift3d_amd_affine_ncc_refine_device(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny,
                                        int nz, double *A_io, const sift3d_amd_affine_refine_params *params,
                                        sift3d_amd_affine_refine_result *result, double *fit_out, void *d_work,
                                        void *stream, const float *d_WF, const float *d_WM)
{
    return affine_refine(&METRIC_NCC, "sift3d_amd_affine_ncc_refine_device", d_F, ox, oy, oz, d_M, nx, ny, nz, A_io,
                         params, result, fit_out, d_work, stream, 1, d_WF, d_WM, NULL);
}

int sift3d_amd_affine_mi_refine_device(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny,
                                       int nz, double *A_io, int bins, float lo_f, float hi_f, float lo_m, float hi_m,
                                       const sift3d_amd_affine_refine_params *params,
                                       sift3d_amd_affine_refine_result *result, sift3d_amd_similarity *mi_out,
                                       void *d_work, void *stream, const float *d_WF, const float *d_WM)
{
    static const char what[] = "sift3d_amd_affine_mi_refine_device";
    mi_state ms;
    float s_f;
    int rc;
    if (!mi_out)
        return refuse(what, "NULL argument");
    if (parzen_check(what, bins, lo_f, hi_f, lo_m, hi_m, &s_f))
        return SIFT3D_FAILURE;
    ms.bins = bins;
    ms.lo_f = lo_f; ms.hi_f = hi_f;
    ms.lo_m = lo_m; ms.hi_m = hi_m;
    ms.sim.n = 0;
    ms.sim.msd = ms.sim.ncc = ms.sim.mi = ms.sim.nmi = NAN;
    ms.sim.entropy_fixed = ms.sim.entropy_moving = ms.sim.entropy_joint = NAN;
    *mi_out = ms.sim;
    rc = affine_refine(&METRIC_MI, what, d_F, ox, oy, oz, d_M, nx, ny, nz, A_io, params, result, NULL, d_work, stream, 1,
                       d_WF, d_WM, &ms);
    *mi_out = ms.sim;
    return rc;
}
