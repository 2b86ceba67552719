/* sift3d_similarity.c -- similarity measures: the checked device entries and the host arithmetic on their results
 * (included at the end of sift3d_host.c, after sift3d_checks.c).
 *
 * The contract is in include/sift3d_amd.h, "Similarity measures"; the kernels are in sift3d_similarity.hip, reached
 * through the launcher below after the checks here.  Arguments are checked before the device is touched, so bad
 * input is refused on a machine without a GPU too. */

int sift3d_similarity_launch(const char *fn, const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny,
                             int nz, const double *A, const float *d_field, int interp, int bins, float lo_f,
                             float s_f, float lo_m, float s_m, unsigned long long *d_hist, void *d_stats, void *d_work,
                             void *stream, const float *d_WF, const float *d_WM);

#define SIMILARITY_WORK_BYTES ((size_t)SIFT3D_AMD_SIMILARITY_GRID * 7 * 8)    /* a uint64 and six doubles per slot */

static int bins_ok(int bins)
{
    return bins >= 2 && bins <= SIFT3D_AMD_SIMILARITY_MAX_BINS;
}

size_t sift3d_amd_similarity_work_bytes(int ox, int oy, int oz, int bins)
{
    if (ox <= 0 || oy <= 0 || oz <= 0 || !bins_ok(bins))
        return 0;
    return SIMILARITY_WORK_BYTES;
}

/* s = (float) B / (hi - lo), float, or 0 when the range is refused */
static float bin_scale(int bins, float lo, float hi)
{
    float w, s;
    if (!isfinite(lo) || !isfinite(hi) || !(lo < hi))
        return 0.0f;
    w = hi - lo;
    if (!isfinite(w))
        return 0.0f;
    s = (float)bins / w;
    return isfinite(s) && s > 0.0f ? s : 0.0f;
}

/* the shared body of the four entries: A == NULL is the field one; d_WF, d_WM are the masks ("Masks") or NULL */
static int similarity(const char *what, const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny,
                      int nz, const double *A, const float *d_field, int interp, int bins, float lo_f, float hi_f,
                      float lo_m, float hi_m, uint64_t *d_hist, void *d_stats, void *d_work, void *stream,
                      const float *d_WF, const float *d_WM)
{
    float s_f, s_m;
    if (!d_F || !d_M || (!A && !d_field) || !d_hist || !d_stats || !d_work)
        return refuse(what, "NULL argument");
    if (check_dims(what, ox, oy, oz) || check_dims(what, nx, ny, nz))
        return SIFT3D_FAILURE;
    if (!bins_ok(bins))
        return refuse(what, "bins must be in [2, SIFT3D_AMD_SIMILARITY_MAX_BINS]");
    s_f = bin_scale(bins, lo_f, hi_f);
    s_m = bin_scale(bins, lo_m, hi_m);
    if (s_f == 0.0f || s_m == 0.0f)
        return refuse(what, "a range must be finite, lo < hi, and wide enough for bins / (hi - lo) in float");
    if (interp != SIFT3D_AMD_INTERP_NEAREST && interp != SIFT3D_AMD_INTERP_LINEAR)
        return refuse(what, "unknown interpolation mode");
    if ((A && check_affine(what, A)) ||
        check_aligned(what, ADDR(d_hist) | ADDR(d_stats) | ADDR(d_work),
                      ADDR(d_F) | ADDR(d_M) | ADDR(d_field) | ADDR(d_WF) | ADDR(d_WM)))
        return SIFT3D_FAILURE;
    {
        const range_t in[] = { { d_F, image_bytes(ox, oy, oz, 1) }, { d_M, image_bytes(nx, ny, nz, 1) },
                               { d_field, d_field ? field_bytes(ox, oy, oz) : 0 },
                               { d_WF, d_WF ? image_bytes(ox, oy, oz, 1) : 0 },
                               { d_WM, d_WM ? image_bytes(nx, ny, nz, 1) : 0 } };
        const range_t out[] = { { d_hist, (size_t)bins * bins * sizeof(uint64_t) },
                                { d_stats, SIFT3D_AMD_SIMILARITY_STATS_BYTES }, { d_work, SIMILARITY_WORK_BYTES } };
        if (ranges_aliased(out, 3, in, d_field ? 3 : 2) || ranges_aliased(out, 3, in + 3, 2))
            return refuse(what, ALIASED);
    }
    return sift3d_similarity_launch(what, d_F, ox, oy, oz, d_M, nx, ny, nz, A, d_field, interp, bins, lo_f, s_f, lo_m,
                                    s_m, (unsigned long long *)d_hist, d_stats, d_work, stream, d_WF, d_WM);
}

int sift3d_hip_similarity_affine(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                 const double *A, int interp, int bins, float lo_f, float hi_f, float lo_m, float hi_m,
                                 uint64_t *d_hist, void *d_stats, void *d_work, void *stream)
{
    static const char what[] = "sift3d_hip_similarity_affine";
    if (!A)
        return refuse(what, "NULL argument");
    return similarity(what, d_F, ox, oy, oz, d_M, nx, ny, nz, A, NULL, interp, bins, lo_f, hi_f, lo_m, hi_m, d_hist,
                      d_stats, d_work, stream, NULL, NULL);
}

int sift3d_hip_similarity_field(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                const float *d_field, int interp, int bins, float lo_f, float hi_f, float lo_m,
                                float hi_m, uint64_t *d_hist, void *d_stats, void *d_work, void *stream)
{
    static const char what[] = "sift3d_hip_similarity_field";
    if (!d_field)
        return refuse(what, "NULL argument");
    return similarity(what, d_F, ox, oy, oz, d_M, nx, ny, nz, NULL, d_field, interp, bins, lo_f, hi_f, lo_m, hi_m,
                      d_hist, d_stats, d_work, stream, NULL, NULL);
}

int sift3d_hip_similarity_affine_masked(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny,
                                        int nz, const double *A, int interp, int bins, float lo_f, float hi_f,
                                        float lo_m, float hi_m, uint64_t *d_hist, void *d_stats, void *d_work,
                                        void *stream, const float *d_WF, const float *d_WM)
{
    static const char what[] = "sift3d_hip_similarity_affine_masked";
    if (!A)
        return refuse(what, "NULL argument");
    return similarity(what, d_F, ox, oy, oz, d_M, nx, ny, nz, A, NULL, interp, bins, lo_f, hi_f, lo_m, hi_m, d_hist,
                      d_stats, d_work, stream, d_WF, d_WM);
}

int sift3d_hip_similarity_field_masked(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny,
                                       int nz, const float *d_field, int interp, int bins, float lo_f, float hi_f,
                                       float lo_m, float hi_m, uint64_t *d_hist, void *d_stats, void *d_work,
                                       void *stream, const float *d_WF, const float *d_WM)
{
    static const char what[] = "sift3d_hip_similarity_field_masked";
    if (!d_field)
        return refuse(what, "NULL argument");
    return similarity(what, d_F, ox, oy, oz, d_M, nx, ny, nz, NULL, d_field, interp, bins, lo_f, hi_f, lo_m, hi_m,
                      d_hist, d_stats, d_work, stream, d_WF, d_WM);
}

/* ---- host arithmetic on a histogram and a stats record (the order of every sum is the header's) ---- */

/* acc = acc - p log p over the non-zero counts in order, p = (double) k / (double) total */
static double entropy_of(const uint64_t *k, size_t n, uint64_t total)
{
    const double t = (double)total;
    double acc = 0.0;
    size_t i;
    for (i = 0; i < n; i++)
        if (k[i]) {
            const double p = (double)k[i] / t;
            acc = acc - p * log(p);
        }
    return acc;
}

/* r[i] = sum_j hist[i][j], c[j] = sum_i hist[i][j] */
static void marginals(const uint64_t *hist, int B, uint64_t *r, uint64_t *c)
{
    int i, j;
    for (i = 0; i < B; i++)
        r[i] = c[i] = 0;
    for (i = 0; i < B; i++)
        for (j = 0; j < B; j++) {
            r[i] += hist[(size_t)i * B + j];
            c[j] += hist[(size_t)i * B + j];
        }
}

/* the three entropies, mi and nmi of hist [B][B] with marginals r, c and total N > 0, in the header's order (shared with
 * sift3d_amd_parzen_mi in sift3d_affine_refine.c) */
static void entropy_measures(const uint64_t *hist, int B, const uint64_t *r, const uint64_t *c, uint64_t total,
                             sift3d_amd_similarity *out)
{
    const double hf = entropy_of(r, (size_t)B, total);
    const double hm = entropy_of(c, (size_t)B, total);
    const double hfm = entropy_of(hist, (size_t)B * B, total);
    out->entropy_fixed = hf;
    out->entropy_moving = hm;
    out->entropy_joint = hfm;
    out->mi = (hf + hm) - hfm;
    out->nmi = hfm == 0 ? 0.0 : (hf + hm) / hfm;
}

int sift3d_amd_similarity_measures(const uint64_t *hist, int bins, const void *stats, sift3d_amd_similarity *out)
{
    static const char what[] = "sift3d_amd_similarity_measures";
    uint64_t r[SIFT3D_AMD_SIMILARITY_MAX_BINS], c[SIFT3D_AMD_SIMILARITY_MAX_BINS], n, total = 0;
    double s[6], nd, vf, vm;
    int i;
    if (!hist || !stats || !out)
        return refuse(what, "NULL argument");
    if (!bins_ok(bins))
        return refuse(what, "bins must be in [2, SIFT3D_AMD_SIMILARITY_MAX_BINS]");
    memcpy(&n, stats, sizeof(n));
    memcpy(s, (const char *)stats + 8, sizeof(s));
    out->n = n;
    marginals(hist, bins, r, c);
    for (i = 0; i < bins; i++)
        total += r[i];
    if (n == 0 || total == 0) {
        out->msd = out->ncc = out->mi = out->nmi = NAN;
        out->entropy_fixed = out->entropy_moving = out->entropy_joint = NAN;
        return SIFT3D_SUCCESS;
    }
    nd = (double)n;
    out->msd = s[5] / nd;
    vf = s[2] - s[0] * s[0] / nd;
    vm = s[3] - s[1] * s[1] / nd;
    out->ncc = vf <= 0 || vm <= 0 ? 0.0 : (s[4] - s[0] * s[1] / nd) / sqrt(vf * vm);
    entropy_measures(hist, bins, r, c, total, out);
    return SIFT3D_SUCCESS;
}

int sift3d_amd_label_overlap(const uint64_t *hist, int L, double *dice, double *jaccard, uint64_t *vol_f,
                             uint64_t *vol_m)
{
    static const char what[] = "sift3d_amd_label_overlap";
    uint64_t r[SIFT3D_AMD_SIMILARITY_MAX_BINS], c[SIFT3D_AMD_SIMILARITY_MAX_BINS];
    int k;
    if (!hist)
        return refuse(what, "NULL argument");
    if (L < 1 || L > SIFT3D_AMD_SIMILARITY_MAX_BINS)
        return refuse(what, "the number of labels must be in [1, SIFT3D_AMD_SIMILARITY_MAX_BINS]");
    marginals(hist, L, r, c);
    for (k = 0; k < L; k++) {
        const uint64_t hkk = hist[(size_t)k * L + k], both = r[k] + c[k];
        if (dice)
            dice[k] = both ? (double)(2 * hkk) / (double)both : NAN;
        if (jaccard)
            jaccard[k] = both ? (double)hkk / (double)(both - hkk) : NAN;
        if (vol_f)
            vol_f[k] = r[k];
        if (vol_m)
            vol_m[k] = c[k];
    }
    return SIFT3D_SUCCESS;
}
