/* sift3d_distance.c -- Euclidean distance transforms and surface distances: the checked device entries, the
 * per-label driver and the host arithmetic on the sorted lists (included at the end of sift3d_host.c, after
 * sift3d_checks.c).
 *
 * The contract is in include/sift3d_amd.h, "Distance transforms and surface distances"; the kernels are in
 * sift3d_distance.hip, reached through the launchers below after the checks here.  Arguments are checked before the
 * device is touched, so bad input is refused on a machine without a GPU too. */

int sift3d_distance_launch(const char *fn, const float *d_mask, int nx, int ny, int nz, float wx, float wy, float wz,
                           int invert, int root, float *d_out, float *d_work, void *stream);
int sift3d_signed_combine_launch(const char *fn, const float *d_mask, const float *d_d2set, float *d_io, size_t n,
                                 void *stream);
int sift3d_label_surface_launch(const char *fn, const float *d_labels, int nx, int ny, int nz, int label,
                                float *d_surface, uint64_t *d_count, void *stream);
int sift3d_surface_collect_launch(const char *fn, const float *d_surface, const float *d_d2, size_t n, float *d_list,
                                  size_t capacity, uint64_t *d_count, void *stream);

static int distance_dims_ok(int nx, int ny, int nz)
{
    return nx > 0 && ny > 0 && nz > 0 && nx <= SIFT3D_AMD_DISTANCE_MAX_DIM && ny <= SIFT3D_AMD_DISTANCE_MAX_DIM &&
           nz <= SIFT3D_AMD_DISTANCE_MAX_DIM;
}

static int check_distance_dims(const char *what, int nx, int ny, int nz)
{
    return distance_dims_ok(nx, ny, nz) ? SIFT3D_SUCCESS
                                        : refuse(what, "dimensions must be in [1, SIFT3D_AMD_DISTANCE_MAX_DIM]");
}

/* w[a] = (float) (s_a * s_a), the product in double; spacing == NULL: all 1 */
static int distance_weights(const char *what, const double *spacing, float *w)
{
    int a;
    for (a = 0; a < 3; a++) {
        const double s = spacing ? spacing[a] : 1.0;
        if (!isfinite(s) || s < 1e-6 || s > 1e6)
            return refuse(what, "a spacing must be finite and in [1e-6, 1e6]");
        w[a] = (float)(s * s);
    }
    return SIFT3D_SUCCESS;
}

size_t sift3d_amd_distance_work_bytes(int nx, int ny, int nz)
{
    return distance_dims_ok(nx, ny, nz) ? 2 * image_bytes(nx, ny, nz, 1) : 0;
}

/* the shared body of sift3d_hip_distance_sq (root == 0) and sift3d_hip_distance (root != 0) */
static int distance(const char *what, const float *d_mask, int nx, int ny, int nz, const double *spacing, int invert,
                    int root, float *d_out, void *d_work, void *stream)
{
    float w[3];
    if (!d_mask || !d_out || !d_work)
        return refuse(what, "NULL argument");
    if (check_distance_dims(what, nx, ny, nz) || distance_weights(what, spacing, w) ||
        check_aligned(what, 0, ADDR(d_mask) | ADDR(d_out) | ADDR(d_work)))
        return SIFT3D_FAILURE;
    {
        const size_t vol = image_bytes(nx, ny, nz, 1);
        const range_t in[] = { { d_mask, vol } };
        const range_t out[] = { { d_out, vol }, { d_work, vol } };            /* the first volume of the work buffer */
        if (ranges_aliased(out, 2, in, 1))
            return refuse(what, ALIASED);
    }
    return sift3d_distance_launch(what, d_mask, nx, ny, nz, w[0], w[1], w[2], invert != 0, root, d_out,
                                  (float *)d_work, stream);
}

int sift3d_hip_distance_sq(const float *d_mask, int nx, int ny, int nz, const double *spacing, int invert,
                           float *d_out, void *d_work, void *stream)
{
    return distance("sift3d_hip_distance_sq", d_mask, nx, ny, nz, spacing, invert, 0, d_out, d_work, stream);
}

int sift3d_hip_distance(const float *d_mask, int nx, int ny, int nz, const double *spacing, int invert, float *d_out,
                        void *d_work, void *stream)
{
    return distance("sift3d_hip_distance", d_mask, nx, ny, nz, spacing, invert, 1, d_out, d_work, stream);
}

int sift3d_hip_distance_signed(const float *d_mask, int nx, int ny, int nz, const double *spacing, float *d_out,
                               void *d_work, void *stream)
{
    static const char what[] = "sift3d_hip_distance_signed";
    float w[3], *d_w0 = (float *)d_work, *d_w1;
    size_t vol;
    if (!d_mask || !d_out || !d_work)
        return refuse(what, "NULL argument");
    if (check_distance_dims(what, nx, ny, nz) || distance_weights(what, spacing, w) ||
        check_aligned(what, 0, ADDR(d_mask) | ADDR(d_out) | ADDR(d_work)))
        return SIFT3D_FAILURE;
    vol = image_bytes(nx, ny, nz, 1);
    {
        const range_t in[] = { { d_mask, vol } };
        const range_t out[] = { { d_out, vol }, { d_work, 2 * vol } };
        if (ranges_aliased(out, 2, in, 1))
            return refuse(what, ALIASED);
    }
    d_w1 = d_w0 + grid_voxels(nx, ny, nz);
    /* D2 to the set into the second work volume, D2 to the complement into d_out, then the signs and the roots */
    if (sift3d_distance_launch(what, d_mask, nx, ny, nz, w[0], w[1], w[2], 0, 0, d_w1, d_w0, stream) ||
        sift3d_distance_launch(what, d_mask, nx, ny, nz, w[0], w[1], w[2], 1, 0, d_out, d_w0, stream))
        return SIFT3D_FAILURE;
    return sift3d_signed_combine_launch(what, d_mask, d_w1, d_out, grid_voxels(nx, ny, nz), stream);
}

int sift3d_hip_label_surface(const float *d_labels, int nx, int ny, int nz, int label, float *d_surface,
                             uint64_t *d_count, void *stream)
{
    static const char what[] = "sift3d_hip_label_surface";
    if (!d_labels || !d_surface || !d_count)
        return refuse(what, "NULL argument");
    if (check_distance_dims(what, nx, ny, nz) || check_aligned(what, ADDR(d_count), ADDR(d_labels) | ADDR(d_surface)))
        return SIFT3D_FAILURE;
    {
        const size_t vol = image_bytes(nx, ny, nz, 1);
        const range_t in[] = { { d_labels, vol } };
        const range_t out[] = { { d_surface, vol }, { d_count, sizeof(uint64_t) } };
        if (ranges_aliased(out, 2, in, 1))
            return refuse(what, ALIASED);
    }
    return sift3d_label_surface_launch(what, d_labels, nx, ny, nz, label, d_surface, d_count, stream);
}

#define DISTANCE_MAX_VOXELS \
    ((size_t)SIFT3D_AMD_DISTANCE_MAX_DIM * SIFT3D_AMD_DISTANCE_MAX_DIM * SIFT3D_AMD_DISTANCE_MAX_DIM)

int sift3d_hip_surface_collect(const float *d_surface, const float *d_d2, size_t n_voxels, float *d_list,
                               size_t capacity, uint64_t *d_count, void *stream)
{
    static const char what[] = "sift3d_hip_surface_collect";
    if (!d_surface || !d_d2 || !d_list || !d_count)
        return refuse(what, "NULL argument");
    if (n_voxels < 1 || n_voxels > DISTANCE_MAX_VOXELS)
        return refuse(what, "the number of voxels must be in [1, SIFT3D_AMD_DISTANCE_MAX_DIM^3]");
    if (capacity > DISTANCE_MAX_VOXELS)
        return refuse(what, "the capacity must not exceed SIFT3D_AMD_DISTANCE_MAX_DIM^3");
    if (check_aligned(what, ADDR(d_count), ADDR(d_surface) | ADDR(d_d2) | ADDR(d_list)))
        return SIFT3D_FAILURE;
    {
        const range_t in[] = { { d_surface, n_voxels * sizeof(float) }, { d_d2, n_voxels * sizeof(float) } };
        const range_t out[] = { { d_list, capacity * sizeof(float) }, { d_count, sizeof(uint64_t) } };
        if (ranges_aliased(out, 2, in, 2))
            return refuse(what, ALIASED);
    }
    return sift3d_surface_collect_launch(what, d_surface, d_d2, n_voxels, d_list, capacity, d_count, stream);
}

/* ---- host arithmetic on two sorted lists (the order of every sum is the header's) ---- */

/* sum of d[0 .. n-1] in ascending order, double */
static double list_sum(const float *d, uint64_t n)
{
    double acc = 0.0;
    uint64_t i;
    for (i = 0; i < n; i++)
        acc = acc + (double)d[i];
    return acc;
}

int sift3d_amd_surface_measures(const float *d_fm, uint64_t n_f, const float *d_mf, uint64_t n_m,
                                sift3d_amd_surface_result *out)
{
    static const char what[] = "sift3d_amd_surface_measures";
    double sum_fm, sum_mf, pos, lo = 0.0, hi = 0.0;
    uint64_t n, i, a = 0, b = 0, k;
    if (!out || (n_f && !d_fm) || (n_m && !d_mf))
        return refuse(what, "NULL argument");
    out->n_f = n_f;
    out->n_m = n_m;
    if (n_f == 0 || n_m == 0) {
        out->hausdorff = out->hd95 = out->assd = out->mean_fm = out->mean_mf = out->max_fm = out->max_mf = NAN;
        return SIFT3D_SUCCESS;
    }
    sum_fm = list_sum(d_fm, n_f);
    sum_mf = list_sum(d_mf, n_m);
    n = n_f + n_m;
    out->max_fm = (double)d_fm[n_f - 1];
    out->max_mf = (double)d_mf[n_m - 1];
    out->mean_fm = sum_fm / (double)n_f;
    out->mean_mf = sum_mf / (double)n_m;
    out->hausdorff = out->max_fm > out->max_mf ? out->max_fm : out->max_mf;
    out->assd = (sum_fm + sum_mf) / (double)n;
    /* d[i] and d[min(i + 1, n - 1)] of the merged ascending list, by walking the merge */
    pos = 0.95 * (double)(n - 1);
    i = (uint64_t)floor(pos);
    for (k = 0; k <= i + 1 && k < n; k++) {
        const double v = b >= n_m || (a < n_f && d_fm[a] <= d_mf[b]) ? (double)d_fm[a++] : (double)d_mf[b++];
        if (k == i)
            lo = hi = v;
        else if (k == i + 1)
            hi = v;
    }
    out->hd95 = lo + (pos - (double)i) * (hi - lo);
    return SIFT3D_SUCCESS;
}

/* ---- the per-label driver ---- */

/* d_work: surface of F, surface of M, D2, the transform's scratch, the list (a volume each), then four counters */
#define SURFACE_WORK_VOLUMES 5

size_t sift3d_amd_surface_distances_work_bytes(int nx, int ny, int nz)
{
    return distance_dims_ok(nx, ny, nz)
               ? ((SURFACE_WORK_VOLUMES * image_bytes(nx, ny, nz, 1) + 7) & ~(size_t)7) + 4 * sizeof(uint64_t) : 0;
}

static int float_ascending(const void *a, const void *b)
{
    const float x = *(const float *)a, y = *(const float *)b;
    return (x > y) - (x < y);
}

int sift3d_amd_surface_distances_device(const float *d_LF, const float *d_LM, int nx, int ny, int nz, const int *labels,
                                        int n_labels, const double *spacing, sift3d_amd_surface_result *results,
                                        void *d_work, void *stream)
{
    static const char what[] = "sift3d_amd_surface_distances_device";
    float w[3], *d_sf, *d_sm, *d_d2, *d_edt, *d_list, *h = NULL;
    uint64_t *d_cnt, cnt[4];
    size_t nvox, vol, h_cap = 0;
    int l, rc = SIFT3D_FAILURE;
    if (!d_LF || !d_LM || !labels || !results || !d_work)
        return refuse(what, "NULL argument");
    if (check_distance_dims(what, nx, ny, nz))
        return SIFT3D_FAILURE;
    if (n_labels < 1 || n_labels > SIFT3D_AMD_SIMILARITY_MAX_BINS)
        return refuse(what, "the number of labels must be in [1, SIFT3D_AMD_SIMILARITY_MAX_BINS]");
    if (distance_weights(what, spacing, w) || check_aligned(what, ADDR(d_work), ADDR(d_LF) | ADDR(d_LM)))
        return SIFT3D_FAILURE;
    nvox = grid_voxels(nx, ny, nz);
    vol = image_bytes(nx, ny, nz, 1);
    {
        const range_t in[] = { { d_LF, vol }, { d_LM, vol } };
        const range_t out[] = { { d_work, sift3d_amd_surface_distances_work_bytes(nx, ny, nz) } };
        if (ranges_aliased(out, 1, in, 2))
            return refuse(what, ALIASED);
    }
    d_sf = (float *)d_work;
    d_sm = d_sf + nvox;
    d_d2 = d_sm + nvox;
    d_edt = d_d2 + nvox;
    d_list = d_edt + nvox;
    d_cnt = (uint64_t *)((char *)d_work + ((SURFACE_WORK_VOLUMES * vol + 7) & ~(size_t)7));
    for (l = 0; l < n_labels; l++) {
        sift3d_amd_surface_result *r = results + l;
        size_t n_f, n_m;
        if (sift3d_hip_label_surface(d_LF, nx, ny, nz, labels[l], d_sf, d_cnt, stream) ||
            sift3d_hip_label_surface(d_LM, nx, ny, nz, labels[l], d_sm, d_cnt + 1, stream) ||
            sift3d_hip_memcpy_d2h(cnt, d_cnt, 2 * sizeof(uint64_t), stream) || sift3d_hip_stream_sync(stream))
            goto done;
        n_f = (size_t)cnt[0];
        n_m = (size_t)cnt[1];
        if (n_f == 0 || n_m == 0) {
            if (sift3d_amd_surface_measures(NULL, 0, NULL, 0, r))              /* every measure NaN */
                goto done;
            r->n_f = n_f;
            r->n_m = n_m;
            continue;
        }
        if (n_f + n_m > h_cap) {
            float *grown = (float *)realloc(h, (n_f + n_m) * sizeof(float));
            if (!grown) {
                refuse(what, "out of host memory");
                goto done;
            }
            h = grown;
            h_cap = n_f + n_m;
        }
        /* d_fm: D to the moving surface at the fixed surface's voxels; then the other direction through the same list */
        if (sift3d_hip_distance_sq(d_sm, nx, ny, nz, spacing, 0, d_d2, d_edt, stream) ||
            sift3d_hip_surface_collect(d_sf, d_d2, nvox, d_list, n_f, d_cnt + 2, stream) ||
            sift3d_hip_memcpy_d2h(h, d_list, n_f * sizeof(float), stream) ||
            sift3d_hip_distance_sq(d_sf, nx, ny, nz, spacing, 0, d_d2, d_edt, stream) ||
            sift3d_hip_surface_collect(d_sm, d_d2, nvox, d_list, n_m, d_cnt + 3, stream) ||
            sift3d_hip_memcpy_d2h(h + n_f, d_list, n_m * sizeof(float), stream) ||
            sift3d_hip_memcpy_d2h(cnt + 2, d_cnt + 2, 2 * sizeof(uint64_t), stream) || sift3d_hip_stream_sync(stream))
            goto done;
        if (cnt[2] != n_f || cnt[3] != n_m) {
            refuse(what, "the collected counts differ from the surface counts");
            goto done;
        }
        qsort(h, n_f, sizeof(float), float_ascending);
        qsort(h + n_f, n_m, sizeof(float), float_ascending);
        if (sift3d_amd_surface_measures(h, n_f, h + n_f, n_m, r))
            goto done;
    }
    rc = SIFT3D_SUCCESS;
done:
    free(h);
    return rc;
}
