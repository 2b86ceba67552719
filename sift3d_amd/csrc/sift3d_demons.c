/* sift3d_demons.c -- dense demons refinement of a displacement field (included at the end of sift3d_host.c).
 *
 * The contract is in include/sift3d_amd.h, "Dense demons refinement".  The force and the field update are
 * kernels of sift3d_demons.hip (reached through the launchers below, after the checks here); the warp is
 * sift3d_hip_warp_field and the smoothing the detector's own blur (blur_level), in place per channel, as for the
 * dense descriptors.  Arguments are checked before the device is touched, so bad input is refused on a machine
 * without a GPU too. */

int sift3d_demons_force_launch(const float *d_F, int nx, int ny, int nz, const float *d_W, const float *d_u, int mx,
                               int my, int mz, int nc, double alpha, float *d_step, void *d_stats, void *d_work,
                               void *stream);
int sift3d_demons_field_add_launch(float *d_u, const float *d_step, size_t n, void *stream);

/* floats of d_work ahead of W: the force's partials */
#define DEMONS_PART_FLOATS (SIFT3D_AMD_DEMONS_FORCE_WORK_BYTES / sizeof(float))

typedef struct {
    const void *p;
    size_t bytes;
} demons_range;

static int demons_overlap(demons_range a, demons_range b)
{
    const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
    return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

/* every output against every input and every other output */
static int demons_aliased(const demons_range *out, int nout, const demons_range *in, int nin)
{
    int i, j;
    for (i = 0; i < nout; i++) {
        for (j = 0; j < nin; j++)
            if (demons_overlap(out[i], in[j]))
                return 1;
        for (j = i + 1; j < nout; j++)
            if (demons_overlap(out[i], out[j]))
                return 1;
    }
    return 0;
}

static int demons_check(const char *what, int nx, int ny, int nz, int mx, int my, int mz, int nc, double alpha)
{
    if (nx <= 0 || ny <= 0 || nz <= 0 || mx <= 0 || my <= 0 || mz <= 0) {
        ERR("%s: dimensions must be positive \n", what);
        return SIFT3D_FAILURE;
    }
    if (nc < 1) {
        ERR("%s: the number of channels must be positive \n", what);
        return SIFT3D_FAILURE;
    }
    if (!isfinite(alpha) || !(alpha > 0)) {
        ERR("%s: alpha must be positive and finite \n", what);
        return SIFT3D_FAILURE;
    }
    return SIFT3D_SUCCESS;
}

int sift3d_hip_demons_force(const float *d_F, int nx, int ny, int nz, const float *d_W, const float *d_u, int mx,
                            int my, int mz, int nc, double alpha, float *d_step, void *d_stats, void *d_work,
                            void *stream)
{
    static const char what[] = "sift3d_hip_demons_force";
    size_t n;
    demons_range in[3], out[3];
    if (!d_F || !d_W || !d_u || !d_step || !d_stats || !d_work) {
        ERR("%s: NULL argument \n", what);
        return SIFT3D_FAILURE;
    }
    if (demons_check(what, nx, ny, nz, mx, my, mz, nc, alpha))
        return SIFT3D_FAILURE;
    if ((((uintptr_t)d_stats | (uintptr_t)d_work) & 7) ||
        (((uintptr_t)d_F | (uintptr_t)d_W | (uintptr_t)d_u | (uintptr_t)d_step) & 3)) {
        ERR("%s: a buffer is misaligned \n", what);
        return SIFT3D_FAILURE;
    }
    n = (size_t)nx * ny * nz;
    in[0].p = d_F; in[0].bytes = (size_t)nc * n * sizeof(float);
    in[1].p = d_W; in[1].bytes = (size_t)nc * n * sizeof(float);
    in[2].p = d_u; in[2].bytes = 3 * n * sizeof(float);
    out[0].p = d_step; out[0].bytes = 3 * n * sizeof(float);
    out[1].p = d_stats; out[1].bytes = SIFT3D_AMD_DEMONS_STATS_BYTES;
    out[2].p = d_work; out[2].bytes = SIFT3D_AMD_DEMONS_FORCE_WORK_BYTES;
    if (demons_aliased(out, 3, in, 3)) {
        ERR("%s: an output overlaps an input, the work buffer or another output \n", what);
        return SIFT3D_FAILURE;
    }
    return sift3d_demons_force_launch(d_F, nx, ny, nz, d_W, d_u, mx, my, mz, nc, alpha, d_step, d_stats, d_work,
                                      stream);
}

size_t sift3d_amd_demons_work_floats(int nx, int ny, int nz, int nc)
{
    if (nx <= 0 || ny <= 0 || nz <= 0 || nc < 1)
        return 0;
    /* partials, W (nc planes), delta (3), the blur's two intermediates */
    return DEMONS_PART_FLOATS + ((size_t)nc + 5) * ((size_t)nx * ny * nz);
}

/* each of the 3 channels of v [3][nz][ny][nx] through blur_level in place (units 1, unit 1.0) */
static int demons_blur3(float *v, const int *dims, const filter_t *f, float *tmp, void *stream)
{
    static const double lu[3] = { 1.0, 1.0, 1.0 };
    const size_t n = (size_t)dims[0] * dims[1] * dims[2];
    int c;
    for (c = 0; c < 3; c++) {
        float *ch = v + (size_t)c * n;
        if (blur_level(NULL, ch, ch, dims, lu, f, stream, tmp, tmp + n, -1, NULL))
            return SIFT3D_FAILURE;
    }
    return SIFT3D_SUCCESS;
}

int sift3d_amd_demons_device(const float *d_F, int nx, int ny, int nz, const float *d_M, int mx, int my, int mz,
                             int nc, float *d_u, int iterations, double alpha, double sigma_fluid,
                             double sigma_diffusion, float *d_work, void *d_stats, void *stream)
{
    static const char what[] = "sift3d_amd_demons_device";
    const int dims[3] = { nx, ny, nz };
    size_t n;
    float *d_W, *d_step, *d_tmp;
    filter_t ff, fd;
    demons_range in[2], out[3];
    int k, rc = SIFT3D_FAILURE;
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
    if ((((uintptr_t)d_stats | (uintptr_t)d_work) & 7) ||
        (((uintptr_t)d_F | (uintptr_t)d_M | (uintptr_t)d_u) & 3)) {
        ERR("%s: a buffer is misaligned \n", what);
        return SIFT3D_FAILURE;
    }
    n = (size_t)nx * ny * nz;
    in[0].p = d_F; in[0].bytes = (size_t)nc * n * sizeof(float);
    in[1].p = d_M; in[1].bytes = (size_t)nc * ((size_t)mx * my * mz) * sizeof(float);
    out[0].p = d_u; out[0].bytes = 3 * n * sizeof(float);
    out[1].p = d_work; out[1].bytes = sift3d_amd_demons_work_floats(nx, ny, nz, nc) * sizeof(float);
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
    d_W = d_work + DEMONS_PART_FLOATS;
    d_step = d_W + (size_t)nc * n;
    d_tmp = d_step + 3 * n;
    for (k = 0; k < iterations; k++) {
        if (sift3d_hip_warp_field(d_M, mx, my, mz, nc, d_u, nx, ny, nz, d_W, SIFT3D_AMD_INTERP_LINEAR, 0.0f, stream) ||
            sift3d_demons_force_launch(d_F, nx, ny, nz, d_W, d_u, mx, my, mz, nc, alpha, d_step,
                                       (char *)d_stats + (size_t)SIFT3D_AMD_DEMONS_STATS_BYTES * k, d_work, stream))
            goto done;
        if (sigma_fluid > 0 && demons_blur3(d_step, dims, &ff, d_tmp, stream))
            goto done;
        if (sift3d_demons_field_add_launch(d_u, d_step, 3 * n, stream))
            goto done;
        if (sigma_diffusion > 0 && demons_blur3(d_u, dims, &fd, d_tmp, stream))
            goto done;
    }
    rc = SIFT3D_SUCCESS;
done:
    free(ff.taps);
    free(fd.taps);
    return rc;
}
