/* sift3d_init.c -- initial transforms for the intensity refinements: the checked device entries of the moments pass and
 * of the batched similarity, the frame of a moments record, the candidate maps, their ranking and the driver that
 * strings them together (included at the end of sift3d_host.c, after sift3d_affine_refine.c and sift3d_ffd.c).
 *
 * The contract is in include/sift3d_amd.h, "Initial transforms: moments and candidate search"; the kernels are in
 * sift3d_init.hip, reached through the launchers below after the checks here.  Arguments are checked before the device
 * is touched, so bad input is refused on a machine without a GPU too. */

int sift3d_moments_launch(const char *fn, const float *d_V, int nx, int ny, int nz, const float *d_W, int binary,
                          float floor, void *d_record, void *d_work, void *stream);
unsigned sift3d_similarity_batch_grid(int ox, int oy, int oz);
int sift3d_similarity_batch_launch(const char *fn, const float *d_F, int ox, int oy, int oz, const float *d_M, int nx,
                                   int ny, int nz, const double *A, int K, int interp, int bins, float lo_f, float s_f,
                                   float lo_m, float s_m, unsigned long long *d_hist, void *d_stats, void *d_work,
                                   void *stream, const float *d_WF, const float *d_WM);

/* ---- moments ---- */

#define MOMENTS_WORK_BYTES ((size_t)SIFT3D_AMD_SIMILARITY_GRID * 11 * 8)      /* a uint64 and ten doubles per slot */

size_t sift3d_amd_moments_work_bytes(int nx, int ny, int nz)
{
    if (nx <= 0 || ny <= 0 || nz <= 0)
        return 0;
    return MOMENTS_WORK_BYTES;
}

int sift3d_hip_moments(const float *d_V, int nx, int ny, int nz, const float *d_W, int weight, float floor,
                       void *d_record, void *d_work, void *stream)
{
    static const char what[] = "sift3d_hip_moments";
    if (!d_V || !d_record || !d_work)
        return refuse(what, "NULL argument");
    if (check_dims(what, nx, ny, nz))
        return SIFT3D_FAILURE;
    if (!isfinite(floor))
        return refuse(what, "the floor is not finite");
    if (weight != SIFT3D_AMD_MOMENTS_INTENSITY && weight != SIFT3D_AMD_MOMENTS_BINARY)
        return refuse(what, "unknown weight");
    if (check_aligned(what, ADDR(d_record) | ADDR(d_work), ADDR(d_V) | ADDR(d_W)))
        return SIFT3D_FAILURE;
    {
        const range_t in[] = { { d_V, image_bytes(nx, ny, nz, 1) }, { d_W, d_W ? image_bytes(nx, ny, nz, 1) : 0 } };
        const range_t out[] = { { d_record, SIFT3D_AMD_MOMENTS_BYTES }, { d_work, MOMENTS_WORK_BYTES } };
        if (ranges_aliased(out, 2, in, 2))
            return refuse(what, ALIASED);
    }
    return sift3d_moments_launch(what, d_V, nx, ny, nz, d_W, weight == SIFT3D_AMD_MOMENTS_BINARY, floor, d_record,
                                 d_work, stream);
}

/* cyclic Jacobi on the symmetric 3 x 3 matrix a (upper triangle read); v's COLUMNS leave as the eigenvectors */
static void jacobi3(double a[3][3], double v[3][3])
{
    int sweep, p, q, i;
    double scale;
    for (p = 0; p < 3; p++)
        for (q = 0; q < 3; q++)
            v[p][q] = p == q ? 1.0 : 0.0;
    scale = (fabs(a[0][0]) + fabs(a[1][1])) + fabs(a[2][2]);
    a[1][0] = a[0][1]; a[2][0] = a[0][2]; a[2][1] = a[1][2];
    for (sweep = 0; sweep < 64; sweep++) {                   /* quadratic: a handful of sweeps */
        const double off = (a[0][1] * a[0][1] + a[0][2] * a[0][2]) + a[1][2] * a[1][2];
        if (off <= (1e-60 * scale) * scale)
            break;
        for (p = 0; p < 2; p++)
            for (q = p + 1; q < 3; q++) {
                double theta, t, c, s;
                if (a[p][q] == 0.0)
                    continue;
                theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
                t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                c = 1.0 / sqrt(t * t + 1.0);
                s = t * c;
                for (i = 0; i < 3; i++) {                    /* a <- a J */
                    const double aip = a[i][p], aiq = a[i][q];
                    a[i][p] = c * aip - s * aiq;
                    a[i][q] = s * aip + c * aiq;
                }
                for (i = 0; i < 3; i++) {                    /* a <- J^T a */
                    const double api = a[p][i], aqi = a[q][i];
                    a[p][i] = c * api - s * aqi;
                    a[q][i] = s * api + c * aqi;
                }
                a[p][q] = a[q][p] = 0.0;
                for (i = 0; i < 3; i++) {
                    const double vip = v[i][p], viq = v[i][q];
                    v[i][p] = c * vip - s * viq;
                    v[i][q] = s * vip + c * viq;
                }
            }
    }
}

int sift3d_amd_moments_frame(const void *record, int nx, int ny, int nz, double *centroid, double *axes, double *lambda)
{
    static const char what[] = "sift3d_amd_moments_frame";
    static const int IJ[6][2] = { { 0, 0 }, { 0, 1 }, { 0, 2 }, { 1, 1 }, { 1, 2 }, { 2, 2 } };
    uint64_t n;
    double s[10], mu[3], a[3][3], v[3][3], c[3], ev[3], R[3][3];
    int order[3] = { 0, 1, 2 }, i, j, r;
    if (!record || !centroid || !axes || !lambda)
        return refuse(what, "NULL argument");
    if (check_dims(what, nx, ny, nz))
        return SIFT3D_FAILURE;
    memcpy(&n, record, sizeof(n));
    memcpy(s, (const char *)record + 8, sizeof(s));
    for (i = 0; i < 10; i++)
        if (!isfinite(s[i]))
            return refuse(what, "the record is not finite");
    if (n == 0 || !(s[0] > 0))
        return refuse(what, "the record counts nothing");
    c[0] = (double)(nx - 1) / 2.0; c[1] = (double)(ny - 1) / 2.0; c[2] = (double)(nz - 1) / 2.0;
    for (i = 0; i < 3; i++)
        mu[i] = s[1 + i] / s[0];
    for (i = 0; i < 6; i++)
        a[IJ[i][0]][IJ[i][1]] = s[4 + i] / s[0] - mu[IJ[i][0]] * mu[IJ[i][1]];
    for (i = 0; i < 3; i++)
        for (j = i; j < 3; j++)
            if (!isfinite(a[i][j]))
                return refuse(what, "the covariance is not finite");
    jacobi3(a, v);
    for (i = 0; i < 3; i++)
        ev[i] = a[i][i];
    /* descending, the lower index first among equals (insertion sort: stable) */
    for (i = 1; i < 3; i++)
        for (j = i; j > 0 && ev[order[j]] > ev[order[j - 1]]; j--) {
            const int t = order[j];
            order[j] = order[j - 1];
            order[j - 1] = t;
        }
    for (r = 0; r < 2; r++) {
        int big = 0;
        for (i = 0; i < 3; i++)
            R[r][i] = v[i][order[r]];
        for (i = 1; i < 3; i++)
            if (fabs(R[r][i]) > fabs(R[r][big]))
                big = i;
        if (R[r][big] < 0)
            for (i = 0; i < 3; i++)
                R[r][i] = -R[r][i];
    }
    R[2][0] = R[0][1] * R[1][2] - R[0][2] * R[1][1];
    R[2][1] = R[0][2] * R[1][0] - R[0][0] * R[1][2];
    R[2][2] = R[0][0] * R[1][1] - R[0][1] * R[1][0];
    for (i = 0; i < 3; i++) {
        if (!isfinite(ev[i]) || !isfinite(R[i][0]) || !isfinite(R[i][1]) || !isfinite(R[i][2]))
            return refuse(what, "the frame is not finite");
    }
    for (i = 0; i < 3; i++) {
        centroid[i] = c[i] + mu[i];
        lambda[i] = ev[order[i]];
        for (j = 0; j < 3; j++)
            axes[3 * i + j] = R[i][j];
    }
    return SIFT3D_SUCCESS;
}

/* ---- batched similarity ---- */

static size_t batch_work_bytes(int ox, int oy, int oz, int K)
{
    return (size_t)K * sift3d_similarity_batch_grid(ox, oy, oz) * 7 * 8;     /* a uint64 and six doubles per slot */
}

static int batch_bins_ok(int bins)
{
    return bins == 0 || bins_ok(bins);
}

size_t sift3d_amd_similarity_batch_work_bytes(int ox, int oy, int oz, int bins, int K)
{
    if (ox <= 0 || oy <= 0 || oz <= 0 || !batch_bins_ok(bins) || K < 1 || K > SIFT3D_AMD_SIMILARITY_BATCH_MAX)
        return 0;
    return batch_work_bytes(ox, oy, oz, K);
}

static int similarity_batch(const char *what, const float *d_F, int ox, int oy, int oz, const float *d_M, int nx,
                            int ny, int nz, const double *A, int K, int interp, int bins, float lo_f, float hi_f,
                            float lo_m, float hi_m, uint64_t *d_hist, void *d_stats, void *d_work, void *stream,
                            const float *d_WF, const float *d_WM)
{
    float s_f = 0.0f, s_m = 0.0f;
    size_t work;
    int k;
    if (!d_F || !d_M || !A || !d_stats || !d_work)
        return refuse(what, "NULL argument");
    if (check_dims(what, ox, oy, oz) || check_dims(what, nx, ny, nz))
        return SIFT3D_FAILURE;
    if (K < 1 || K > SIFT3D_AMD_SIMILARITY_BATCH_MAX)
        return refuse(what, "K must be in [1, SIFT3D_AMD_SIMILARITY_BATCH_MAX]");
    if (!batch_bins_ok(bins))
        return refuse(what, "bins must be 0 or in [2, SIFT3D_AMD_SIMILARITY_MAX_BINS]");
    if ((bins == 0) != (d_hist == NULL))
        return refuse(what, "bins == 0 goes with a NULL histogram, and only with one");
    if (bins) {
        s_f = bin_scale(bins, lo_f, hi_f);
        s_m = bin_scale(bins, lo_m, hi_m);
        if (s_f == 0.0f || s_m == 0.0f)
            return refuse(what, "a range must be finite, lo < hi, and wide enough for bins / (hi - lo) in float");
    }
    if (interp != SIFT3D_AMD_INTERP_NEAREST && interp != SIFT3D_AMD_INTERP_LINEAR)
        return refuse(what, "unknown interpolation mode");
    for (k = 0; k < K; k++)
        if (check_affine(what, A + 12 * (size_t)k))
            return SIFT3D_FAILURE;
    if (check_aligned(what, ADDR(d_hist) | ADDR(d_stats) | ADDR(d_work), ADDR(d_F) | ADDR(d_M) | ADDR(d_WF) | ADDR(d_WM)))
        return SIFT3D_FAILURE;
    work = batch_work_bytes(ox, oy, oz, K);
    if (!work)
        return refuse(what, "grid too large");
    {
        const range_t in[] = { { d_F, image_bytes(ox, oy, oz, 1) }, { d_M, image_bytes(nx, ny, nz, 1) },
                               { d_WF, d_WF ? image_bytes(ox, oy, oz, 1) : 0 },
                               { d_WM, d_WM ? image_bytes(nx, ny, nz, 1) : 0 } };
        const range_t out[] = { { d_stats, (size_t)K * SIFT3D_AMD_SIMILARITY_STATS_BYTES }, { d_work, work },
                                { d_hist, (size_t)K * bins * bins * sizeof(uint64_t) } };
        if (ranges_aliased(out, bins ? 3 : 2, in, 4))
            return refuse(what, ALIASED);
    }
    return sift3d_similarity_batch_launch(what, d_F, ox, oy, oz, d_M, nx, ny, nz, A, K, interp, bins, lo_f, s_f, lo_m,
                                          s_m, (unsigned long long *)d_hist, d_stats, d_work, stream, d_WF, d_WM);
}

int sift3d_hip_similarity_affine_batch(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny,
                                       int nz, const double *A, int K, int interp, int bins, float lo_f, float hi_f,
                                       float lo_m, float hi_m, uint64_t *d_hist, void *d_stats, void *d_work,
                                       void *stream)
{
    return similarity_batch("sift3d_hip_similarity_affine_batch", d_F, ox, oy, oz, d_M, nx, ny, nz, A, K, interp, bins,
                            lo_f, hi_f, lo_m, hi_m, d_hist, d_stats, d_work, stream, NULL, NULL);
}

int sift3d_hip_similarity_affine_batch_masked(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx,
                                              int ny, int nz, const double *A, int K, int interp, int bins, float lo_f,
                                              float hi_f, float lo_m, float hi_m, uint64_t *d_hist, void *d_stats,
                                              void *d_work, void *stream, const float *d_WF, const float *d_WM)
{
    return similarity_batch("sift3d_hip_similarity_affine_batch_masked", d_F, ox, oy, oz, d_M, nx, ny, nz, A, K, interp,
                            bins, lo_f, hi_f, lo_m, hi_m, d_hist, d_stats, d_work, stream, d_WF, d_WM);
}

/* ---- candidates ---- */

void sift3d_amd_affine_init_default_params(sift3d_amd_affine_init_params *p)
{
    int d;
    if (!p)
        return;
    p->mode = SIFT3D_AMD_INIT_SEARCH;
    p->metric = SIFT3D_AMD_INIT_MI;
    p->levels = 3;
    p->weight = SIFT3D_AMD_MOMENTS_BINARY;
    p->floor_f = p->floor_m = 0.0f;
    p->bins = 32;
    p->lo_f = p->lo_m = 0.0f;
    p->hi_f = p->hi_m = 1.0f;
    for (d = 0; d < 3; d++) {
        p->range_deg[d] = 90.0;
        p->range_vox[d] = 0.0;
    }
    p->step_deg = 30.0;
    p->step_vox = 1.0;
    p->min_overlap = 0.5;
}

size_t sift3d_amd_affine_init_struct_bytes(int which)
{
    return which == 0   ? sizeof(sift3d_amd_affine_init_params)
           : which == 1 ? sizeof(sift3d_amd_frame)
           : which == 2 ? sizeof(sift3d_amd_affine_init_result)
           : which == 3 ? (size_t)SIFT3D_AMD_MOMENTS_BYTES
           : which == 4 ? (size_t)SIFT3D_AMD_SIMILARITY_BATCH_MAX
           : which == 5 ? (size_t)SIFT3D_AMD_INIT_MAX_CANDIDATES
           : which == 6 ? (size_t)SIFT3D_AMD_INIT_KEEP
                        : 0;
}

/* the values per axis of a range and a step, 2 floor(range / step) + 1; 0 where they are refused */
static long init_axis_count(double range, double step)
{
    double h;
    if (!isfinite(range) || range < 0 || !isfinite(step) || !(step > 0))
        return 0;
    h = floor(range / step);
    return h > SIFT3D_AMD_INIT_MAX_CANDIDATES ? SIFT3D_AMD_INIT_MAX_CANDIDATES + 1 : 2 * (long)h + 1;
}

/* K of SEARCH, or 0 where a range or a step is refused or K would pass SIFT3D_AMD_INIT_MAX_CANDIDATES */
static int init_search_count(const sift3d_amd_affine_init_params *p, long *na, long *nt)
{
    long K = 1;
    int d;
    for (d = 0; d < 3; d++) {
        na[d] = init_axis_count(p->range_deg[d], p->step_deg);
        nt[d] = init_axis_count(p->range_vox[d], p->step_vox);
    }
    for (d = 0; d < 3; d++) {
        if (!na[d] || !nt[d])
            return 0;
        K *= na[d];
        if (K > SIFT3D_AMD_INIT_MAX_CANDIDATES)
            return 0;
        K *= nt[d];
        if (K > SIFT3D_AMD_INIT_MAX_CANDIDATES)
            return 0;
    }
    return (int)K;
}

static int frame_ok(const sift3d_amd_frame *f)
{
    int i;
    for (i = 0; i < 3; i++)
        if (!isfinite(f->centroid[i]))
            return 0;
    for (i = 0; i < 9; i++)
        if (!isfinite(f->axes[i]))
            return 0;
    return 1;
}

/* C = A B, each entry (a0 b0 + a1 b1) + a2 b2 */
static void mat3_mul(const double *A, const double *B, double *Cm)
{
    int i, j;
    for (i = 0; i < 3; i++)
        for (j = 0; j < 3; j++)
            Cm[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

/* the candidate q = R (p - c_F) + c_M + t as a 3 x 4 pull map */
static void init_candidate(const double *R, const double *cF, const double *cM, const double *t, double *A)
{
    int d;
    for (d = 0; d < 3; d++) {
        A[4 * d] = R[3 * d];
        A[4 * d + 1] = R[3 * d + 1];
        A[4 * d + 2] = R[3 * d + 2];
        A[4 * d + 3] = (cM[d] + t[d]) - ((R[3 * d] * cF[0] + R[3 * d + 1] * cF[1]) + R[3 * d + 2] * cF[2]);
    }
}

int sift3d_amd_affine_init_candidates(int mode, const sift3d_amd_frame *frame_F,
                                      const sift3d_amd_frame *frame_M,
                                      const sift3d_amd_affine_init_params *params, double *A_out, int *K)
{
    static const char what[] = "sift3d_amd_affine_init_candidates";
    static const double I3[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, T0[3] = { 0, 0, 0 };
    static const double SIGNS[4][3] = { { 1, 1, 1 }, { 1, -1, -1 }, { -1, 1, -1 }, { -1, -1, 1 } };
    sift3d_amd_affine_init_params prm;
    const double *cF, *cM;
    long na[3], nt[3];
    int count, cap;
    if (!frame_F || !frame_M || !K)
        return refuse(what, "NULL argument");
    if (params)
        prm = *params;
    else
        sift3d_amd_affine_init_default_params(&prm);
    if (!frame_ok(frame_F) || !frame_ok(frame_M))
        return refuse(what, "a frame is not finite");
    if (mode == SIFT3D_AMD_INIT_CENTROID)
        count = 1;
    else if (mode == SIFT3D_AMD_INIT_AXES)
        count = 5;
    else if (mode == SIFT3D_AMD_INIT_SEARCH) {
        count = init_search_count(&prm, na, nt);
        if (!count)
            return refuse(what, "a search range or step is refused, or there are more than "
                                "SIFT3D_AMD_INIT_MAX_CANDIDATES candidates");
    } else
        return refuse(what, "unknown mode");
    cap = *K;
    if (A_out && cap < count)
        return refuse(what, "A_out holds fewer maps than there are candidates");
    *K = count;
    if (!A_out)
        return SIFT3D_SUCCESS;
    cF = frame_F->centroid;
    cM = frame_M->centroid;
    if (mode != SIFT3D_AMD_INIT_SEARCH) {
        int s, i, j;
        init_candidate(I3, cF, cM, T0, A_out);
        for (s = 0; s + 1 < count; s++) {                    /* R = V_M^T D_s V_F */
            double DV[9], VMt[9], R[9];
            for (i = 0; i < 3; i++)
                for (j = 0; j < 3; j++) {
                    DV[3 * i + j] = SIGNS[s][i] * frame_F->axes[3 * i + j];
                    VMt[3 * i + j] = frame_M->axes[3 * j + i];
                }
            mat3_mul(VMt, DV, R);
            init_candidate(R, cF, cM, T0, A_out + 12 * (size_t)(s + 1));
        }
        return SIFT3D_SUCCESS;
    }
    {
        const double rad = M_PI / 180.0;
        long ia, ib, ig, ix, iy, iz;
        size_t k = 0;
        for (iz = 0; iz < nt[2]; iz++)
        for (iy = 0; iy < nt[1]; iy++)
        for (ix = 0; ix < nt[0]; ix++)
        for (ig = 0; ig < na[2]; ig++)
        for (ib = 0; ib < na[1]; ib++)
        for (ia = 0; ia < na[0]; ia++) {
            const double al = (double)(ia - (na[0] - 1) / 2) * prm.step_deg;
            const double be = (double)(ib - (na[1] - 1) / 2) * prm.step_deg;
            const double ga = (double)(ig - (na[2] - 1) / 2) * prm.step_deg;
            const double t[3] = { (double)(ix - (nt[0] - 1) / 2) * prm.step_vox,
                                  (double)(iy - (nt[1] - 1) / 2) * prm.step_vox,
                                  (double)(iz - (nt[2] - 1) / 2) * prm.step_vox };
            const double ca = cos(al * rad), sa = sin(al * rad), cb = cos(be * rad), sb = sin(be * rad);
            const double cg = cos(ga * rad), sg = sin(ga * rad);
            const double Rx[9] = { 1, 0, 0, 0, ca, -sa, 0, sa, ca };
            const double Ry[9] = { cb, 0, sb, 0, 1, 0, -sb, 0, cb };
            const double Rz[9] = { cg, -sg, 0, sg, cg, 0, 0, 0, 1 };
            double RyRx[9], R[9];
            mat3_mul(Ry, Rx, RyRx);
            mat3_mul(Rz, RyRx, R);
            init_candidate(R, cF, cM, t, A_out + 12 * k++);
        }
    }
    return SIFT3D_SUCCESS;
}

/* ---- ranking ---- */

/* the cost of one candidate from its stats record (and, MI, its histogram); NaN where nothing was counted */
static double init_cost(int metric, const void *stats, const uint64_t *hist, int bins, uint64_t *n_out)
{
    uint64_t n;
    double s[6], nd, vf, vm, ncc;
    memcpy(&n, stats, sizeof(n));
    memcpy(s, (const char *)stats + 8, sizeof(s));
    *n_out = n;
    if (n == 0)
        return NAN;
    nd = (double)n;
    if (metric == SIFT3D_AMD_INIT_MSD)
        return s[5] / nd;
    if (metric == SIFT3D_AMD_INIT_NCC) {
        vf = s[2] - s[0] * s[0] / nd;
        vm = s[3] - s[1] * s[1] / nd;
        ncc = vf <= 0 || vm <= 0 ? 0.0 : (s[4] - s[0] * s[1] / nd) / sqrt(vf * vm);
        return 1.0 - ncc * ncc;
    }
    {
        sift3d_amd_similarity sim;
        if (sift3d_amd_similarity_measures(hist, bins, stats, &sim))
            return NAN;
        return -sim.mi;
    }
}

/* order[0 .. *count - 1]: the eligible candidates by ascending cost, ties to the lower index (insertion by cost, in
 * index order) */
static void init_order(int K, const double *cost, const uint64_t *n, double min_overlap, int *order, int *count)
{
    uint64_t n_max = 0;
    int k, m = 0;
    for (k = 0; k < K; k++)
        if (n[k] > n_max)
            n_max = n[k];
    for (k = 0; k < K; k++) {
        int j;
        if (!isfinite(cost[k]) || n[k] == 0 || !((double)n[k] >= min_overlap * (double)n_max))
            continue;
        for (j = m; j > 0 && cost[order[j - 1]] > cost[k]; j--)
            order[j] = order[j - 1];
        order[j] = k;
        m++;
    }
    *count = m;
}

int sift3d_amd_affine_init_rank(int metric, int K, const void *stats, const uint64_t *hist, int bins,
                                double min_overlap, double *cost_out, uint64_t *n_out, int *order_out, int *count_out)
{
    static const char what[] = "sift3d_amd_affine_init_rank";
    int k;
    if (!stats || !cost_out || !n_out || !order_out || !count_out)
        return refuse(what, "NULL argument");
    if (metric != SIFT3D_AMD_INIT_MSD && metric != SIFT3D_AMD_INIT_NCC && metric != SIFT3D_AMD_INIT_MI)
        return refuse(what, "unknown metric");
    if (K < 1 || K > SIFT3D_AMD_INIT_MAX_CANDIDATES)
        return refuse(what, "K must be in [1, SIFT3D_AMD_INIT_MAX_CANDIDATES]");
    if (metric == SIFT3D_AMD_INIT_MI && (!hist || !bins_ok(bins)))
        return refuse(what, "MI needs the histograms and bins in [2, SIFT3D_AMD_SIMILARITY_MAX_BINS]");
    if (!(min_overlap >= 0 && min_overlap <= 1))
        return refuse(what, "min_overlap must be in [0, 1]");
    for (k = 0; k < K; k++)
        cost_out[k] = init_cost(metric, (const char *)stats + (size_t)k * SIFT3D_AMD_SIMILARITY_STATS_BYTES,
                                metric == SIFT3D_AMD_INIT_MI ? hist + (size_t)k * bins * bins : NULL, bins, n_out + k);
    init_order(K, cost_out, n_out, min_overlap, order_out, count_out);
    return *count_out ? SIFT3D_SUCCESS : refuse(what, "no candidate is eligible");
}

/* ---- the driver ---- */

static int init_params_ok(const sift3d_amd_affine_init_params *p)
{
    return (p->mode == SIFT3D_AMD_INIT_CENTROID || p->mode == SIFT3D_AMD_INIT_AXES || p->mode == SIFT3D_AMD_INIT_SEARCH) &&
           (p->metric == SIFT3D_AMD_INIT_MSD || p->metric == SIFT3D_AMD_INIT_NCC || p->metric == SIFT3D_AMD_INIT_MI) &&
           p->levels >= 1 && p->levels <= SIFT3D_AMD_DEMONS_MAX_LEVELS &&
           (p->weight == SIFT3D_AMD_MOMENTS_INTENSITY || p->weight == SIFT3D_AMD_MOMENTS_BINARY) &&
           isfinite(p->floor_f) && isfinite(p->floor_m) &&
           (p->metric != SIFT3D_AMD_INIT_MI ||
            (bins_ok(p->bins) && bin_scale(p->bins, p->lo_f, p->hi_f) != 0.0f &&
             bin_scale(p->bins, p->lo_m, p->hi_m) != 0.0f)) &&
           p->min_overlap >= 0 && p->min_overlap <= 1;
}

/* the levels the driver runs: the largest l <= levels whose coarsest grids keep every axis at 8 or more (1 at least) */
int sift3d_amd_affine_init_levels(int ox, int oy, int oz, int nx, int ny, int nz, int levels)
{
    int d[6] = { ox, oy, oz, nx, ny, nz }, l, i;
    if (levels < 1)
        return 0;
    for (l = 1; l < levels; l++) {
        for (i = 0; i < 6; i++)
            if (multires_half(d[i]) < 8)
                return l;
        for (i = 0; i < 6; i++)
            d[i] = multires_half(d[i]);
    }
    return levels;
}

/* K of the params' mode (0 where SEARCH refuses its ranges) */
static int init_count(const sift3d_amd_affine_init_params *p)
{
    long na[3], nt[3];
    return p->mode == SIFT3D_AMD_INIT_CENTROID ? 1 : p->mode == SIFT3D_AMD_INIT_AXES ? 5 : init_search_count(p, na, nt);
}

/* d_work, in bytes: the moments' partial slots, the two moments records (padded to 16 bytes each), then for a chunk of
 * Kc = min(K, SIFT3D_AMD_SIMILARITY_BATCH_MAX) candidates on the coarsest grid the batch's work buffer, the Kc stats
 * records and (MI) the Kc histograms, each padded to 16 bytes; then the pyramid as sift3d_amd_affine_refine_device
 * lays it out: per level the restricted fixed and moving volumes and room for a mask beside each (given or not) */
static size_t init_layout(int ox, int oy, int oz, int nx, int ny, int nz, const sift3d_amd_affine_init_params *p,
                          int levels, int K, size_t *off_batch, size_t *off_stats,
                          size_t *off_hist, size_t *off_pyramid)
{
    const int Kc = K < SIFT3D_AMD_SIMILARITY_BATCH_MAX ? K : SIFT3D_AMD_SIMILARITY_BATCH_MAX;
    const int bins = p->metric == SIFT3D_AMD_INIT_MI ? p->bins : 0;
    size_t total = MOMENTS_WORK_BYTES + 2 * pad16(SIFT3D_AMD_MOMENTS_BYTES);
    int cx = ox, cy = oy, cz = oz, l;
    for (l = 1; l < levels; l++) {
        cx = multires_half(cx); cy = multires_half(cy); cz = multires_half(cz);
    }
    *off_batch = total;
    total += pad16(batch_work_bytes(cx, cy, cz, Kc));
    *off_stats = total;
    total += pad16((size_t)Kc * SIFT3D_AMD_SIMILARITY_STATS_BYTES);
    *off_hist = total;
    total += pad16((size_t)Kc * bins * bins * sizeof(uint64_t));
    *off_pyramid = total;
    for (l = 1; l < levels; l++) {
        ox = multires_half(ox); oy = multires_half(oy); oz = multires_half(oz);
        nx = multires_half(nx); ny = multires_half(ny); nz = multires_half(nz);
        total += 2 * (pad4(grid_voxels(ox, oy, oz)) + pad4(grid_voxels(nx, ny, nz))) * sizeof(float);
    }
    return total;
}

size_t sift3d_amd_affine_init_work_bytes(int ox, int oy, int oz, int nx, int ny, int nz,
                                         const sift3d_amd_affine_init_params *params)
{
    sift3d_amd_affine_init_params prm;
    size_t a, b, c, d;
    int K;
    if (params)
        prm = *params;
    else
        sift3d_amd_affine_init_default_params(&prm);
    if (ox <= 0 || oy <= 0 || oz <= 0 || nx <= 0 || ny <= 0 || nz <= 0 || !init_params_ok(&prm))
        return 0;
    K = init_count(&prm);
    if (!K)
        return 0;
    return init_layout(ox, oy, oz, nx, ny, nz, &prm, sift3d_amd_affine_init_levels(ox, oy, oz, nx, ny, nz, prm.levels),
                       K, &a, &b, &c, &d);
}

int sift3d_amd_affine_init_device(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                  const float *d_WF, const float *d_WM, const sift3d_amd_affine_init_params *params,
                                  sift3d_amd_affine_init_result *result, double *costs_out, uint64_t *counts_out,
                                  void *d_work, void *stream)
{
    static const char what[] = "sift3d_amd_affine_init_device";
    sift3d_amd_affine_init_params prm, cprm;
    affine_level lv[SIFT3D_AMD_DEMONS_MAX_LEVELS];
    const affine_level *c;
    sift3d_amd_frame fr[2];
    unsigned char rec[2][SIFT3D_AMD_MOMENTS_BYTES];
    char *w = (char *)d_work;
    size_t off_batch, off_stats, off_hist, off, total, cells;
    double *A = NULL, *cost = NULL, scale;
    uint64_t *n = NULL, *hist = NULL;
    unsigned char *stats = NULL;
    int *order = NULL;
    int levels, K, Kc, bins, l, k0, i, d, m = 0, rc = SIFT3D_FAILURE;
    if (!d_F || !d_M || !result || !d_work)
        return refuse(what, "NULL argument");
    if (params)
        prm = *params;
    else
        sift3d_amd_affine_init_default_params(&prm);
    if (check_dims(what, ox, oy, oz) || check_dims(what, nx, ny, nz))
        return SIFT3D_FAILURE;
    if (!init_params_ok(&prm))
        return refuse(what, "a parameter is out of range");
    K = init_count(&prm);
    if (!K)
        return refuse(what, "a search range or step is refused, or there are more than SIFT3D_AMD_INIT_MAX_CANDIDATES "
                            "candidates");
    if (check_aligned(what, ADDR(d_work), ADDR(d_F) | ADDR(d_M) | ADDR(d_WF) | ADDR(d_WM)))
        return SIFT3D_FAILURE;
    levels = sift3d_amd_affine_init_levels(ox, oy, oz, nx, ny, nz, prm.levels);
    total = init_layout(ox, oy, oz, nx, ny, nz, &prm, levels, K, &off_batch, &off_stats, &off_hist, &off);
    {
        const range_t in[] = { { d_F, image_bytes(ox, oy, oz, 1) }, { d_M, image_bytes(nx, ny, nz, 1) },
                               { d_WF, d_WF ? image_bytes(ox, oy, oz, 1) : 0 },
                               { d_WM, d_WM ? image_bytes(nx, ny, nz, 1) : 0 } };
        const range_t out[] = { { d_work, total } };
        if (ranges_aliased(out, 1, in, 4))
            return refuse(what, ALIASED);
    }
    Kc = K < SIFT3D_AMD_SIMILARITY_BATCH_MAX ? K : SIFT3D_AMD_SIMILARITY_BATCH_MAX;
    bins = prm.metric == SIFT3D_AMD_INIT_MI ? prm.bins : 0;
    cells = (size_t)bins * bins;
    /* 1. the pyramid */
    lv[0] = (affine_level){ d_F, d_M, ox, oy, oz, nx, ny, nz, d_WF, d_WM };
    for (l = 1; l < levels; l++) {
        const affine_level *f = lv + l - 1;
        affine_level *k = lv + l;
        float *cF = (float *)(w + off), *cM;
        *k = (affine_level){ NULL, NULL, multires_half(f->ox), multires_half(f->oy), multires_half(f->oz),
                             multires_half(f->nx), multires_half(f->ny), multires_half(f->nz), NULL, NULL };
        off += pad4(grid_voxels(k->ox, k->oy, k->oz)) * sizeof(float);
        cM = (float *)(w + off);
        off += pad4(grid_voxels(k->nx, k->ny, k->nz)) * sizeof(float);
        if (sift3d_hip_restrict2(f->F, f->ox, f->oy, f->oz, 1, cF, 1.0f, stream) ||
            sift3d_hip_restrict2(f->M, f->nx, f->ny, f->nz, 1, cM, 1.0f, stream))
            return SIFT3D_FAILURE;
        k->F = cF;
        k->M = cM;
        if (mask_pyramid_level(f->WF, f->ox, f->oy, f->oz, f->WM, f->nx, f->ny, f->nz, w, &off, &k->WF, &k->WM, stream))
            return SIFT3D_FAILURE;
    }
    c = lv + levels - 1;
    scale = ldexp(1.0, levels - 1);
    /* 2. the moments of both at the coarsest level, 3. the frames */
    {
        void *d_rec0 = w + MOMENTS_WORK_BYTES, *d_rec1 = w + MOMENTS_WORK_BYTES + pad16(SIFT3D_AMD_MOMENTS_BYTES);
        if (sift3d_hip_moments(c->F, c->ox, c->oy, c->oz, c->WF, prm.weight, prm.floor_f, d_rec0, w, stream) ||
            sift3d_hip_memcpy_d2h(rec[0], d_rec0, SIFT3D_AMD_MOMENTS_BYTES, stream) ||
            sift3d_hip_moments(c->M, c->nx, c->ny, c->nz, c->WM, prm.weight, prm.floor_m, d_rec1, w, stream) ||
            sift3d_hip_memcpy_d2h(rec[1], d_rec1, SIFT3D_AMD_MOMENTS_BYTES, stream) || sift3d_hip_stream_sync(stream))
            return SIFT3D_FAILURE;
    }
    if (sift3d_amd_moments_frame(rec[0], c->ox, c->oy, c->oz, fr[0].centroid, fr[0].axes, fr[0].lambda) ||
        sift3d_amd_moments_frame(rec[1], c->nx, c->ny, c->nz, fr[1].centroid, fr[1].axes, fr[1].lambda))
        return refuse(what, "a volume has nothing above its floor (inside its mask)");
    /* the search offsets are level-0 voxels */
    cprm = prm;
    for (d = 0; d < 3; d++)
        cprm.range_vox[d] = prm.range_vox[d] / scale;
    cprm.step_vox = prm.step_vox / scale;
    A = (double *)malloc((size_t)K * 12 * sizeof(double));
    cost = (double *)malloc((size_t)K * sizeof(double));
    n = (uint64_t *)malloc((size_t)K * sizeof(uint64_t));
    order = (int *)malloc((size_t)K * sizeof(int));
    stats = (unsigned char *)malloc((size_t)Kc * SIFT3D_AMD_SIMILARITY_STATS_BYTES);
    hist = cells ? (uint64_t *)malloc((size_t)Kc * cells * sizeof(uint64_t)) : NULL;
    if (!A || !cost || !n || !order || !stats || (cells && !hist)) {
        refuse(what, "out of host memory");
        goto done;
    }
    i = K;
    if (sift3d_amd_affine_init_candidates(prm.mode, fr, fr + 1, &cprm, A, &i))
        goto done;
    /* 4. the scores, a chunk at a time: one copy to the host and one wait per chunk */
    for (k0 = 0; k0 < K; k0 += Kc) {
        const int nk = K - k0 < Kc ? K - k0 : Kc;
        uint64_t *d_hist = cells ? (uint64_t *)(w + off_hist) : NULL;
        if (similarity_batch(what, c->F, c->ox, c->oy, c->oz, c->M, c->nx, c->ny, c->nz, A + 12 * (size_t)k0, nk,
                             SIFT3D_AMD_INTERP_LINEAR, bins, prm.lo_f, prm.hi_f, prm.lo_m, prm.hi_m, d_hist,
                             w + off_stats, w + off_batch, stream, c->WF, c->WM) ||
            sift3d_hip_memcpy_d2h(stats, w + off_stats, (size_t)nk * SIFT3D_AMD_SIMILARITY_STATS_BYTES, stream) ||
            (cells && sift3d_hip_memcpy_d2h(hist, d_hist, (size_t)nk * cells * sizeof(uint64_t), stream)) ||
            sift3d_hip_stream_sync(stream))
            goto done;
        for (i = 0; i < nk; i++)
            cost[k0 + i] = init_cost(prm.metric, stats + (size_t)i * SIFT3D_AMD_SIMILARITY_STATS_BYTES,
                                     cells ? hist + (size_t)i * cells : NULL, bins, n + k0 + i);
    }
    /* 5. the ranking, and the best map on level 0 */
    result->K = K;
    result->levels = levels;
    result->kept = 0;
    for (i = 0; i < 2; i++) {
        sift3d_amd_frame *o = i ? &result->frame_m : &result->frame_f;
        *o = fr[i];
        for (d = 0; d < 3; d++) {
            o->centroid[d] = fr[i].centroid[d] * scale;
            o->lambda[d] = fr[i].lambda[d] * (scale * scale);
        }
    }
    init_order(K, cost, n, prm.min_overlap, order, &m);
    if (costs_out)
        memcpy(costs_out, cost, (size_t)K * sizeof(double));
    if (counts_out)
        memcpy(counts_out, n, (size_t)K * sizeof(uint64_t));
    if (!m) {
        refuse(what, "no candidate is eligible");
        goto done;
    }
    rc = SIFT3D_SUCCESS;
    result->kept = m < SIFT3D_AMD_INIT_KEEP ? m : SIFT3D_AMD_INIT_KEEP;
    for (i = 0; i < result->kept; i++) {
        result->keep_index[i] = order[i];
        result->keep_cost[i] = cost[order[i]];
        result->keep_n[i] = n[order[i]];
    }
    result->index = order[0];
    result->cost = cost[order[0]];
    result->n = n[order[0]];
    memcpy(result->A, A + 12 * (size_t)order[0], sizeof(result->A));
    for (l = 1; l < levels; l++)
        for (i = 3; i < 12; i += 4)
            result->A[i] = result->A[i] * 2.0;
done:
    free(A); free(cost); free(n); free(order); free(stats); free(hist);
    return rc;
}
