/* sift3d_field_ops.c -- field composition, exponential, inverse and the diffeomorphic demons driver (included at
 * the end of sift3d_host.c, after sift3d_demons.c, whose range checks and blur it shares).
 *
 * The contract is in include/sift3d_amd.h, "Field composition, exponential and inverse".  The composition sample is
 * k_field_compose of sift3d_warp.hip, reached through the launcher below after the checks here; the exponential
 * and the inverse ping-pong inside d_work.  Arguments are checked before the device is touched, so bad input is
 * refused on a machine without a GPU too. */

int sift3d_field_compose_launch(const float *d_u, int ux, int uy, int uz, const float *d_v, int ox, int oy, int oz,
                                float *d_out, int mode, void *d_stats, void *d_work, void *stream);
int sift3d_field_scale_launch(float *d_dst, const float *d_src, size_t n, float s, void *stream);

/* floats of the invert driver's d_work ahead of its second iterate: the composition's partials */
#define FIELD_PART_FLOATS (SIFT3D_AMD_FIELD_WORK_BYTES / sizeof(float))

static int field_dims(const char *what, int ox, int oy, int oz)
{
    if (ox <= 0 || oy <= 0 || oz <= 0) {
        ERR("%s: dimensions must be positive \n", what);
        return SIFT3D_FAILURE;
    }
    return SIFT3D_SUCCESS;
}

static size_t field_bytes(int ox, int oy, int oz)
{
    return 3 * ((size_t)ox * oy * oz) * sizeof(float);
}

int sift3d_hip_field_compose(const float *d_u, int ux, int uy, int uz, const float *d_v, int ox, int oy, int oz,
                             float *d_out, int mode, void *d_stats, void *d_work, void *stream)
{
    static const char what[] = "sift3d_hip_field_compose";
    demons_range in[2], out[3];
    int nout = 0;
    if (!d_u || !d_v || (!d_out && !d_stats) || (d_stats && !d_work)) {
        ERR("%s: NULL argument \n", what);
        return SIFT3D_FAILURE;
    }
    if (field_dims(what, ux, uy, uz) || field_dims(what, ox, oy, oz))
        return SIFT3D_FAILURE;
    if (mode != SIFT3D_AMD_FIELD_COMPOSE && mode != SIFT3D_AMD_FIELD_INVERT) {
        ERR("%s: unknown mode \n", what);
        return SIFT3D_FAILURE;
    }
    if ((((uintptr_t)d_stats | (uintptr_t)d_work) & 7) || (((uintptr_t)d_u | (uintptr_t)d_v | (uintptr_t)d_out) & 3)) {
        ERR("%s: a buffer is misaligned \n", what);
        return SIFT3D_FAILURE;
    }
    in[0].p = d_u; in[0].bytes = field_bytes(ux, uy, uz);
    in[1].p = d_v; in[1].bytes = field_bytes(ox, oy, oz);
    if (d_out) {
        out[nout].p = d_out; out[nout].bytes = field_bytes(ox, oy, oz); nout++;
    }
    if (d_stats) {
        out[nout].p = d_stats; out[nout].bytes = SIFT3D_AMD_FIELD_STATS_BYTES; nout++;
        out[nout].p = d_work; out[nout].bytes = SIFT3D_AMD_FIELD_WORK_BYTES; nout++;
    }
    if (demons_aliased(out, nout, in, 2)) {
        ERR("%s: an output overlaps an input, the work buffer or another output \n", what);
        return SIFT3D_FAILURE;
    }
    return sift3d_field_compose_launch(d_u, ux, uy, uz, d_v, ox, oy, oz, d_out, mode, d_stats, d_work, stream);
}

size_t sift3d_amd_field_exp_work_floats(int ox, int oy, int oz)
{
    if (ox <= 0 || oy <= 0 || oz <= 0)
        return 0;
    return 3 * ((size_t)ox * oy * oz);
}

/* w_K of the exponential into d_out, w_0 = d_v * 2^-K, ping-pong between d_out and d_other (K >= 1); d_v may be
 * d_other (it is read only by the scaling) */
static int field_exp_run(const float *d_v, int ox, int oy, int oz, int K, float *d_out, float *d_other, void *stream)
{
    const size_t n3 = 3 * ((size_t)ox * oy * oz);
    float *a, *b;
    int k;
    /* w_k for even k lands in `a`: choose it so that w_K is in d_out */
    a = (K % 2 == 0) ? d_out : d_other;
    b = (K % 2 == 0) ? d_other : d_out;
    if (sift3d_field_scale_launch(a, d_v, n3, (float)ldexp(1.0, -K), stream))
        return SIFT3D_FAILURE;
    for (k = 0; k < K; k++) {
        float *src = (k % 2 == 0) ? a : b, *dst = (k % 2 == 0) ? b : a;
        if (sift3d_field_compose_launch(src, ox, oy, oz, src, ox, oy, oz, dst, SIFT3D_AMD_FIELD_COMPOSE, NULL, NULL,
                                        stream))
            return SIFT3D_FAILURE;
    }
    return SIFT3D_SUCCESS;
}

int sift3d_amd_field_exp_device(const float *d_v, int ox, int oy, int oz, int squarings, float *d_out, float *d_work,
                                void *stream)
{
    static const char what[] = "sift3d_amd_field_exp_device";
    demons_range in[1], out[2];
    if (!d_v || !d_out || !d_work) {
        ERR("%s: NULL argument \n", what);
        return SIFT3D_FAILURE;
    }
    if (field_dims(what, ox, oy, oz))
        return SIFT3D_FAILURE;
    if (squarings < 0 || squarings > SIFT3D_AMD_FIELD_MAX_SQUARINGS) {
        ERR("%s: squarings must be in [0, SIFT3D_AMD_FIELD_MAX_SQUARINGS] \n", what);
        return SIFT3D_FAILURE;
    }
    if ((((uintptr_t)d_v | (uintptr_t)d_out) & 3) || ((uintptr_t)d_work & 7)) {
        ERR("%s: a buffer is misaligned \n", what);
        return SIFT3D_FAILURE;
    }
    in[0].p = d_v; in[0].bytes = field_bytes(ox, oy, oz);
    out[0].p = d_out; out[0].bytes = field_bytes(ox, oy, oz);
    out[1].p = d_work; out[1].bytes = sift3d_amd_field_exp_work_floats(ox, oy, oz) * sizeof(float);
    if (demons_aliased(out, 2, in, 1)) {
        ERR("%s: an output overlaps an input, the work buffer or another output \n", what);
        return SIFT3D_FAILURE;
    }
    if (squarings == 0)
        return sift3d_hip_memcpy_d2d(d_out, d_v, field_bytes(ox, oy, oz), stream);
    return field_exp_run(d_v, ox, oy, oz, squarings, d_out, d_work, stream);
}

size_t sift3d_amd_field_invert_work_floats(int ox, int oy, int oz)
{
    if (ox <= 0 || oy <= 0 || oz <= 0)
        return 0;
    return FIELD_PART_FLOATS + 3 * ((size_t)ox * oy * oz);
}

int sift3d_amd_field_invert_device(const float *d_u, int ux, int uy, int uz, float *d_w, int ox, int oy, int oz,
                                   int iterations, float *d_work, void *d_stats, void *stream)
{
    static const char what[] = "sift3d_amd_field_invert_device";
    demons_range in[1], out[3];
    float *cur, *nxt, *t;
    int k;
    if (!d_u || !d_w || !d_work || !d_stats) {
        ERR("%s: NULL argument \n", what);
        return SIFT3D_FAILURE;
    }
    if (field_dims(what, ux, uy, uz) || field_dims(what, ox, oy, oz))
        return SIFT3D_FAILURE;
    if (iterations < 0) {
        ERR("%s: the number of iterations must not be negative \n", what);
        return SIFT3D_FAILURE;
    }
    if ((((uintptr_t)d_u | (uintptr_t)d_w) & 3) || (((uintptr_t)d_work | (uintptr_t)d_stats) & 7)) {
        ERR("%s: a buffer is misaligned \n", what);
        return SIFT3D_FAILURE;
    }
    in[0].p = d_u; in[0].bytes = field_bytes(ux, uy, uz);
    out[0].p = d_w; out[0].bytes = field_bytes(ox, oy, oz);
    out[1].p = d_work; out[1].bytes = sift3d_amd_field_invert_work_floats(ox, oy, oz) * sizeof(float);
    out[2].p = d_stats; out[2].bytes = (size_t)SIFT3D_AMD_FIELD_STATS_BYTES * ((size_t)iterations + 1);
    if (demons_aliased(out, 3, in, 1)) {
        ERR("%s: an output overlaps an input, the work buffer or another output \n", what);
        return SIFT3D_FAILURE;
    }
    cur = d_w;
    nxt = d_work + FIELD_PART_FLOATS;
    for (k = 0; k < iterations; k++) {
        if (sift3d_field_compose_launch(d_u, ux, uy, uz, cur, ox, oy, oz, nxt, SIFT3D_AMD_FIELD_INVERT,
                                        (char *)d_stats + (size_t)SIFT3D_AMD_FIELD_STATS_BYTES * k, d_work, stream))
            return SIFT3D_FAILURE;
        t = cur; cur = nxt; nxt = t;
    }
    if (sift3d_field_compose_launch(d_u, ux, uy, uz, cur, ox, oy, oz, NULL, SIFT3D_AMD_FIELD_INVERT,
                                    (char *)d_stats + (size_t)SIFT3D_AMD_FIELD_STATS_BYTES * iterations, d_work,
                                    stream))
        return SIFT3D_FAILURE;
    if (cur != d_w)
        return sift3d_hip_memcpy_d2d(d_w, cur, field_bytes(ox, oy, oz), stream);
    return SIFT3D_SUCCESS;
}

size_t sift3d_amd_demons_work_floats_ex(int nx, int ny, int nz, int nc, int update)
{
    const size_t base = sift3d_amd_demons_work_floats(nx, ny, nz, nc);
    if (!base)
        return 0;
    if (update == SIFT3D_AMD_DEMONS_ADDITIVE)
        return base;
    if (update == SIFT3D_AMD_DEMONS_DIFFEOMORPHIC)
        return base + 6 * ((size_t)nx * ny * nz);
    return 0;
}

/* each of the 3 channels of src [3][nz][ny][nx] through blur_level into dst (units 1, unit 1.0); blur_level takes
 * src != dst: its x pass reads src into the first intermediate and only its last pass writes dst */
static int demons_blur3_to(const float *src, float *dst, const int *dims, const filter_t *f, float *tmp, void *stream)
{
    static const double lu[3] = { 1.0, 1.0, 1.0 };
    const size_t n = (size_t)dims[0] * dims[1] * dims[2];
    int c;
    for (c = 0; c < 3; c++)
        if (blur_level(NULL, src + (size_t)c * n, dst + (size_t)c * n, dims, lu, f, stream, tmp, tmp + n, -1, NULL))
            return SIFT3D_FAILURE;
    return SIFT3D_SUCCESS;
}

int sift3d_amd_demons_device_ex(const float *d_F, int nx, int ny, int nz, const float *d_M, int mx, int my, int mz,
                                int nc, float *d_u, int iterations, double alpha, double sigma_fluid,
                                double sigma_diffusion, int update, int squarings, float *d_work, void *d_stats,
                                void *stream)
{
    static const char what[] = "sift3d_amd_demons_device_ex";
    const int dims[3] = { nx, ny, nz };
    size_t n;
    float *d_W, *d_step, *d_tmp, *d_unew, *d_pp;
    filter_t ff, fd;
    demons_range in[2], out[3];
    int k, rc = SIFT3D_FAILURE;
    if (update != SIFT3D_AMD_DEMONS_ADDITIVE && update != SIFT3D_AMD_DEMONS_DIFFEOMORPHIC) {
        ERR("%s: unknown update \n", what);
        return SIFT3D_FAILURE;
    }
    if (squarings < 0 || squarings > SIFT3D_AMD_FIELD_MAX_SQUARINGS) {
        ERR("%s: squarings must be in [0, SIFT3D_AMD_FIELD_MAX_SQUARINGS] \n", what);
        return SIFT3D_FAILURE;
    }
    if (update == SIFT3D_AMD_DEMONS_ADDITIVE)
        return sift3d_amd_demons_device(d_F, nx, ny, nz, d_M, mx, my, mz, nc, d_u, iterations, alpha, sigma_fluid,
                                        sigma_diffusion, d_work, d_stats, stream);
    /* the additive driver's checks, with the larger work buffer */
    if (!d_F || !d_M || !d_u || !d_work || !d_stats) {
        ERR("%s: NULL argument \n", what);
        return SIFT3D_FAILURE;
    }
    if (demons_check(what, nx, ny, nz, mx, my, mz, nc, alpha))
        return SIFT3D_FAILURE;
    if (iterations < 0) {
        ERR("%s: the number of iterations must not be negative \n", what);
        return SIFT3D_FAILURE;
    }
    if (!isfinite(sigma_fluid) || sigma_fluid < 0 || !isfinite(sigma_diffusion) || sigma_diffusion < 0) {
        ERR("%s: the sigmas must be finite and not negative \n", what);
        return SIFT3D_FAILURE;
    }
    if ((((uintptr_t)d_stats | (uintptr_t)d_work) & 7) || (((uintptr_t)d_F | (uintptr_t)d_M | (uintptr_t)d_u) & 3)) {
        ERR("%s: a buffer is misaligned \n", what);
        return SIFT3D_FAILURE;
    }
    n = (size_t)nx * ny * nz;
    in[0].p = d_F; in[0].bytes = (size_t)nc * n * sizeof(float);
    in[1].p = d_M; in[1].bytes = (size_t)nc * ((size_t)mx * my * mz) * sizeof(float);
    out[0].p = d_u; out[0].bytes = 3 * n * sizeof(float);
    out[1].p = d_work; out[1].bytes = sift3d_amd_demons_work_floats_ex(nx, ny, nz, nc, update) * sizeof(float);
    out[2].p = d_stats; out[2].bytes = (size_t)SIFT3D_AMD_DEMONS_STATS_BYTES * (iterations > 0 ? iterations : 1);
    if (demons_aliased(out, 3, in, 2)) {
        ERR("%s: an output overlaps an input, the work buffer or another output \n", what);
        return SIFT3D_FAILURE;
    }
    if (iterations == 0)
        return SIFT3D_SUCCESS;
    ff.taps = fd.taps = NULL;
    if ((sigma_fluid > 0 && gauss_filter(&ff, sigma_fluid)) || (sigma_diffusion > 0 && gauss_filter(&fd, sigma_diffusion)))
        goto done;
    /* the additive driver's layout, then u_new and the exponential's second buffer */
    d_W = d_work + DEMONS_PART_FLOATS;
    d_step = d_W + (size_t)nc * n;
    d_tmp = d_step + 3 * n;
    d_unew = d_tmp + 2 * n;
    d_pp = d_unew + 3 * n;
    for (k = 0; k < iterations; k++) {
        const float *e = d_step;
        if (sift3d_hip_warp_field(d_M, mx, my, mz, nc, d_u, nx, ny, nz, d_W, SIFT3D_AMD_INTERP_LINEAR, 0.0f, stream) ||
            sift3d_demons_force_launch(d_F, nx, ny, nz, d_W, d_u, mx, my, mz, nc, alpha, d_step,
                                       (char *)d_stats + (size_t)SIFT3D_AMD_DEMONS_STATS_BYTES * k, d_work, stream))
            goto done;
        if (sigma_fluid > 0 && demons_blur3(d_step, dims, &ff, d_tmp, stream))
            goto done;
        /* e = exp(delta): w_0 = delta * 2^-K, then K squarings between d_pp and d_step (delta is read only by the
         * scaling); K == 0: e = delta itself */
        if (squarings > 0) {
            if (field_exp_run(d_step, nx, ny, nz, squarings, d_pp, d_step, stream))
                goto done;
            e = d_pp;
        }
        if (sift3d_field_compose_launch(d_u, nx, ny, nz, e, nx, ny, nz, d_unew, SIFT3D_AMD_FIELD_COMPOSE, NULL, NULL,
                                        stream))
            goto done;
        if (sigma_diffusion > 0) {
            if (demons_blur3_to(d_unew, d_u, dims, &fd, d_tmp, stream))
                goto done;
        } else if (sift3d_hip_memcpy_d2d(d_u, d_unew, 3 * n * sizeof(float), stream)) {
            goto done;
        }
    }
    rc = SIFT3D_SUCCESS;
done:
    free(ff.taps);
    free(fd.taps);
    return rc;
}
