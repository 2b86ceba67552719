/* sift3d_lncc.c -- local cross-correlation: the checked statistics pass, force and field normalisation, and the
 * demons-style driver that iterates them (included at the end of sift3d_host.c, after sift3d_demons.c, whose level
 * tables, mask checks, blur and pyramid offsets it uses as they are).
 *
 * The contract is in include/sift3d_amd.h, "Local cross-correlation".  The kernels are sift3d_lncc.hip's, reached
 * through the launchers below after the checks here; the warp is sift3d_hip_warp_field, the exponential field_exp_run,
 * the composition sift3d_field_compose_launch and the smoothing demons_blur3, word for word as demons_run uses them.
 * Arguments are checked before the device is touched, so bad input is refused on a machine without a GPU too. */

int sift3d_lncc_valid_launch(const float *d_u, int nx, int ny, int nz, int mx, int my, int mz, const float *d_WF,
                             const float *d_WM, float *d_v, void *stream);
int sift3d_lncc_stats_launch(const float *d_F, const float *d_W, const float *d_v, int nx, int ny, int nz, int radius,
                             float *d_cc, double *d_coef, void *d_stats, void *d_part, void *stream);
int sift3d_lncc_force_launch(const float *d_F, const float *d_W, const float *d_v, int nx, int ny, int nz, int radius,
                             const double *d_coef, float *d_force, void *stream);
int sift3d_field_normalize_launch(float *d_field, size_t n, double step, void *d_work, void *stream);

static int check_radius(const char *what, int radius)
{
    return radius < 1 || radius > SIFT3D_AMD_LNCC_MAX_RADIUS
               ? refuse(what, "radius must be in [1, SIFT3D_AMD_LNCC_MAX_RADIUS]") : SIFT3D_SUCCESS;
}

static int check_step(const char *what, double step)
{
    return !isfinite(step) || !(step > 0) ? refuse(what, "step must be positive and finite") : SIFT3D_SUCCESS;
}

/* the partials, then v (n floats), rounded up to 8 bytes */
static size_t lncc_work_bytes(size_t n)
{
    return SIFT3D_AMD_LNCC_PARTIAL_BYTES + ((n * sizeof(float) + 7) & ~(size_t)7);
}

size_t sift3d_amd_lncc_work_bytes(int nx, int ny, int nz)
{
    return nx <= 0 || ny <= 0 || nz <= 0 ? 0 : lncc_work_bytes(grid_voxels(nx, ny, nz));
}

/* what the two passes check alike: the three inputs and the masks against the outputs */
static int lncc_check_pass(const char *what, const float *d_F, int nx, int ny, int nz, const float *d_W,
                           const float *d_u, int mx, int my, int mz, const float *d_WF, const float *d_WM,
                           const range_t *more_in, int nmore, const range_t *out, int nout)
{
    range_t in[4];
    int k;
    in[0] = (range_t){ d_F, image_bytes(nx, ny, nz, 1) };
    in[1] = (range_t){ d_W, image_bytes(nx, ny, nz, 1) };
    in[2] = (range_t){ d_u, field_bytes(nx, ny, nz) };
    for (k = 0; k < nmore; k++)
        in[3 + k] = more_in[k];
    if (ranges_aliased(out, nout, in, 3 + nmore))
        return refuse(what, ALIASED);
    if (check_demons_mask(what, d_WF, grid_voxels(nx, ny, nz), out, nout) ||
        check_demons_mask(what, d_WM, grid_voxels(mx, my, mz), out, nout))
        return SIFT3D_FAILURE;
    return SIFT3D_SUCCESS;
}

int sift3d_hip_lncc(const float *d_F, int nx, int ny, int nz, const float *d_W, const float *d_u, int mx, int my,
                    int mz, const float *d_WF, const float *d_WM, int radius, float *d_cc, double *d_coef,
                    void *d_stats, void *d_work, void *stream)
{
    static const char what[] = "sift3d_hip_lncc";
    range_t out[4];
    int nout = 0;
    size_t n;
    if (!d_F || !d_W || !d_u || !d_stats || !d_work)
        return refuse(what, "NULL argument");
    if (check_dims(what, nx, ny, nz) || check_dims(what, mx, my, mz) || check_radius(what, radius) ||
        check_aligned(what, ADDR(d_stats) | ADDR(d_work) | ADDR(d_coef),
                      ADDR(d_F) | ADDR(d_W) | ADDR(d_u) | ADDR(d_cc)))
        return SIFT3D_FAILURE;
    n = grid_voxels(nx, ny, nz);
    out[nout++] = (range_t){ d_stats, SIFT3D_AMD_DEMONS_STATS_BYTES };
    out[nout++] = (range_t){ d_work, lncc_work_bytes(n) };
    if (d_cc)
        out[nout++] = (range_t){ d_cc, n * sizeof(float) };
    if (d_coef)
        out[nout++] = (range_t){ d_coef, 4 * n * sizeof(double) };
    if (lncc_check_pass(what, d_F, nx, ny, nz, d_W, d_u, mx, my, mz, d_WF, d_WM, NULL, 0, out, nout))
        return SIFT3D_FAILURE;
    {
        float *d_v = (float *)((char *)d_work + SIFT3D_AMD_LNCC_PARTIAL_BYTES);
        if (sift3d_lncc_valid_launch(d_u, nx, ny, nz, mx, my, mz, d_WF, d_WM, d_v, stream))
            return SIFT3D_FAILURE;
        return sift3d_lncc_stats_launch(d_F, d_W, d_v, nx, ny, nz, radius, d_cc, d_coef, d_stats, d_work, stream);
    }
}

int sift3d_hip_lncc_force(const float *d_F, int nx, int ny, int nz, const float *d_W, const float *d_u, int mx, int my,
                          int mz, const float *d_WF, const float *d_WM, int radius, const double *d_coef,
                          float *d_force, void *d_work, void *stream)
{
    static const char what[] = "sift3d_hip_lncc_force";
    size_t n;
    if (!d_F || !d_W || !d_u || !d_coef || !d_force || !d_work)
        return refuse(what, "NULL argument");
    if (check_dims(what, nx, ny, nz) || check_dims(what, mx, my, mz) || check_radius(what, radius) ||
        check_aligned(what, ADDR(d_work) | ADDR(d_coef), ADDR(d_F) | ADDR(d_W) | ADDR(d_u) | ADDR(d_force)))
        return SIFT3D_FAILURE;
    n = grid_voxels(nx, ny, nz);
    {
        const range_t coef = { d_coef, 4 * n * sizeof(double) };
        const range_t out[] = { { d_force, field_bytes(nx, ny, nz) }, { d_work, lncc_work_bytes(n) } };
        float *d_v = (float *)((char *)d_work + SIFT3D_AMD_LNCC_PARTIAL_BYTES);
        if (lncc_check_pass(what, d_F, nx, ny, nz, d_W, d_u, mx, my, mz, d_WF, d_WM, &coef, 1, out, 2))
            return SIFT3D_FAILURE;
        if (sift3d_lncc_valid_launch(d_u, nx, ny, nz, mx, my, mz, d_WF, d_WM, d_v, stream))
            return SIFT3D_FAILURE;
        return sift3d_lncc_force_launch(d_F, d_W, d_v, nx, ny, nz, radius, d_coef, d_force, stream);
    }
}

int sift3d_hip_field_normalize(float *d_field, int nx, int ny, int nz, double step, void *d_work, void *stream)
{
    static const char what[] = "sift3d_hip_field_normalize";
    if (!d_field || !d_work)
        return refuse(what, "NULL argument");
    if (check_dims(what, nx, ny, nz) || check_step(what, step) || check_aligned(what, ADDR(d_work), ADDR(d_field)))
        return SIFT3D_FAILURE;
    if (ranges_overlap((range_t){ d_field, field_bytes(nx, ny, nz) },
                       (range_t){ d_work, SIFT3D_AMD_FIELD_NORMALIZE_WORK_BYTES }))
        return refuse(what, ALIASED);
    return sift3d_field_normalize_launch(d_field, grid_voxels(nx, ny, nz), step, d_work, stream);
}

/* ---- the driver ---- */

/* One level's scratch, as offsets in floats into d_work: the statistics' partials and the normalisation's work at 0,
 * then the four coefficient volumes (doubles: 8 n floats, 8-byte aligned as the head is a multiple of 8 bytes), v, W,
 * phi (3), the blur's two intermediates; the diffeomorphic update adds u_new (3) and the exponential's second buffer
 * (3).  The size function and lncc_run both read it from here. */
typedef struct {
    size_t norm, coef, v, W, step, tmp, unew, pp, total;
} lncc_layout;

static lncc_layout lncc_layout_of(size_t n, int update)
{
    const size_t extra = update == SIFT3D_AMD_DEMONS_DIFFEOMORPHIC ? 3 * n : 0;
    lncc_layout l;
    l.norm = SIFT3D_AMD_LNCC_PARTIAL_BYTES / sizeof(float);
    l.coef = l.norm + SIFT3D_AMD_FIELD_NORMALIZE_WORK_BYTES / sizeof(float);
    l.v = l.coef + 8 * n;
    l.W = l.v + n;
    l.step = l.W + n;
    l.tmp = l.step + 3 * n;
    l.unew = l.tmp + 2 * n;
    l.pp = l.unew + extra;
    l.total = l.pp + extra;
    return l;
}

size_t sift3d_amd_demons_lncc_work_floats(int nx, int ny, int nz, int update, int levels)
{
    if (nx <= 0 || ny <= 0 || nz <= 0 || levels < 1 || levels > SIFT3D_AMD_DEMONS_MAX_LEVELS ||
        (update != SIFT3D_AMD_DEMONS_ADDITIVE && update != SIFT3D_AMD_DEMONS_DIFFEOMORPHIC))
        return 0;
    return pyramid_field_offset(lncc_layout_of(grid_voxels(nx, ny, nz), update).total, nx, ny, nz, levels);
}

typedef struct {
    int radius;
    double step, sigma_fluid, sigma_diffusion;
    int update, squarings;
} lncc_params;

/* demons_validate's checks for this driver: one channel, radius and step in place of nc and alpha */
static int lncc_validate(const char *what, const sift3d_amd_demons_level *level,
                         const sift3d_amd_demons_level_masks *masks, int levels, const lncc_params *p,
                         const float *d_u, const float *d_work, size_t work_floats, const void *d_stats)
{
    range_t in[2 * SIFT3D_AMD_DEMONS_MAX_LEVELS];
    uintptr_t or4 = ADDR(d_u);
    size_t total = 0;
    int l;
    if (!level || !d_u || !d_work || !d_stats)
        return refuse(what, "NULL argument");
    if (levels < 1 || levels > SIFT3D_AMD_DEMONS_MAX_LEVELS)
        return refuse(what, "levels must be in [1, SIFT3D_AMD_DEMONS_MAX_LEVELS]");
    if (check_update(what, p->update) || check_squarings(what, p->squarings) || check_radius(what, p->radius) ||
        check_step(what, p->step) || check_sigmas(what, p->sigma_fluid, p->sigma_diffusion))
        return SIFT3D_FAILURE;
    for (l = 0; l < levels; l++) {
        const sift3d_amd_demons_level *v = level + l;
        if (!v->d_F || !v->d_M)
            return refuse(what, "NULL argument");
        if (check_dims(what, v->nx, v->ny, v->nz) || check_dims(what, v->mx, v->my, v->mz) ||
            check_iterations(what, v->iterations))
            return SIFT3D_FAILURE;
        if (l > 0 && (v->nx != multires_half(v[-1].nx) || v->ny != multires_half(v[-1].ny) ||
                      v->nz != multires_half(v[-1].nz) || v->mx != multires_half(v[-1].mx) ||
                      v->my != multires_half(v[-1].my) || v->mz != multires_half(v[-1].mz)))
            return refuse(what, "a level's dimensions are not the halves of the level above");
        total += (size_t)v->iterations;
        or4 |= ADDR(v->d_F) | ADDR(v->d_M);
        in[2 * l] = (range_t){ v->d_F, image_bytes(v->nx, v->ny, v->nz, 1) };
        in[2 * l + 1] = (range_t){ v->d_M, image_bytes(v->mx, v->my, v->mz, 1) };
    }
    if (check_aligned(what, ADDR(d_stats) | ADDR(d_work), or4))
        return SIFT3D_FAILURE;
    {
        const range_t out[] = { { d_u, field_bytes(level->nx, level->ny, level->nz) },
                                { d_work, work_floats * sizeof(float) },
                                { d_stats, (size_t)SIFT3D_AMD_DEMONS_STATS_BYTES * (total > 0 ? total : 1) } };
        if (ranges_aliased(out, 3, in, 2 * levels))
            return refuse(what, ALIASED);
        for (l = 0; masks && l < levels; l++)
            if (check_demons_mask(what, masks[l].d_WF, grid_voxels(level[l].nx, level[l].ny, level[l].nz), out, 3) ||
                check_demons_mask(what, masks[l].d_WM, grid_voxels(level[l].mx, level[l].my, level[l].mz), out, 3))
                return SIFT3D_FAILURE;
    }
    return SIFT3D_SUCCESS;
}

/* v->iterations iterations of one level on its field d_u, unchecked; arguments as demons_run's */
static int lncc_run(const sift3d_amd_demons_level *v, const float *d_WF, const float *d_WM, const lncc_params *p,
                    float *d_u, const filter_t *ff, const filter_t *fd, float *d_work, char *d_stats, void *stream)
{
    const int dims[3] = { v->nx, v->ny, v->nz };
    const size_t n = grid_voxels(v->nx, v->ny, v->nz);
    const lncc_layout at = lncc_layout_of(n, p->update);
    double *d_coef = (double *)(d_work + at.coef);
    float *d_v = d_work + at.v, *d_W = d_work + at.W, *d_step = d_work + at.step, *d_tmp = d_work + at.tmp,
          *d_unew = d_work + at.unew, *d_pp = d_work + at.pp;
    int k;
    for (k = 0; k < v->iterations; k++) {
        const float *e = d_step;
        if (sift3d_hip_warp_field(v->d_M, v->mx, v->my, v->mz, 1, d_u, v->nx, v->ny, v->nz, d_W,
                                  SIFT3D_AMD_INTERP_LINEAR, 0.0f, stream) ||
            sift3d_lncc_valid_launch(d_u, v->nx, v->ny, v->nz, v->mx, v->my, v->mz, d_WF, d_WM, d_v, stream) ||
            sift3d_lncc_stats_launch(v->d_F, d_W, d_v, v->nx, v->ny, v->nz, p->radius, NULL, d_coef,
                                     d_stats + (size_t)SIFT3D_AMD_DEMONS_STATS_BYTES * k, d_work, stream) ||
            sift3d_lncc_force_launch(v->d_F, d_W, d_v, v->nx, v->ny, v->nz, p->radius, d_coef, d_step, stream))
            return SIFT3D_FAILURE;
        if (p->sigma_fluid > 0 && demons_blur3(d_step, d_step, dims, ff, d_tmp, stream))
            return SIFT3D_FAILURE;
        if (sift3d_field_normalize_launch(d_step, n, p->step, d_work + at.norm, stream))
            return SIFT3D_FAILURE;
        if (p->update == SIFT3D_AMD_DEMONS_ADDITIVE) {
            if (sift3d_demons_field_add_launch(d_u, d_step, 3 * n, stream) ||
                (p->sigma_diffusion > 0 && demons_blur3(d_u, d_u, dims, fd, d_tmp, stream)))
                return SIFT3D_FAILURE;
            continue;
        }
        /* e = exp(phi), then u <- COMPOSE(u, e): demons_run's diffeomorphic update word for word */
        if (p->squarings > 0) {
            if (field_exp_run(d_step, v->nx, v->ny, v->nz, p->squarings, 1.0, d_pp, d_step, stream))
                return SIFT3D_FAILURE;
            e = d_pp;
        }
        if (sift3d_field_compose_launch(d_u, v->nx, v->ny, v->nz, e, v->nx, v->ny, v->nz, d_unew,
                                        SIFT3D_AMD_FIELD_COMPOSE, NULL, NULL, stream) ||
            (p->sigma_diffusion > 0 ? demons_blur3(d_unew, d_u, dims, fd, d_tmp, stream)
                                    : sift3d_hip_memcpy_d2d(d_u, d_unew, 3 * n * sizeof(float), stream)))
            return SIFT3D_FAILURE;
    }
    return SIFT3D_SUCCESS;
}

int sift3d_amd_demons_lncc_device(const sift3d_amd_demons_level *level, const sift3d_amd_demons_level_masks *masks,
                                  int levels, int radius, float *d_u, double step, double sigma_fluid,
                                  double sigma_diffusion, int update, int squarings, float *d_work, void *d_stats,
                                  void *stream)
{
    static const char what[] = "sift3d_amd_demons_lncc_device";
    const lncc_params p = { radius, step, sigma_fluid, sigma_diffusion, update, squarings };
    /* (a NULL level table is refused below before the size matters) */
    const size_t need = level ? sift3d_amd_demons_lncc_work_floats(level->nx, level->ny, level->nz, update, levels) : 0;
    float *u[SIFT3D_AMD_DEMONS_MAX_LEVELS];
    filter_t ff, fd;
    size_t rec = 0, total = 0, scratch;
    int l, rc = SIFT3D_FAILURE;
    if (lncc_validate(what, level, masks, levels, &p, d_u, d_work, need, d_stats))
        return SIFT3D_FAILURE;
    /* the level fields: level 0 is d_u, the others follow the finest level's scratch in d_work (a halved grid needs
     * no more scratch than the finest: the layout grows with the voxels alone) */
    scratch = lncc_layout_of(grid_voxels(level->nx, level->ny, level->nz), update).total;
    u[0] = d_u;
    for (l = 1; l < levels; l++) {
        u[l] = d_work + pyramid_field_offset(scratch, level->nx, level->ny, level->nz, l);
        if (sift3d_restrict2_launch(u[l - 1], level[l - 1].nx, level[l - 1].ny, level[l - 1].nz, 3, u[l], 0.5f,
                                    stream))
            return SIFT3D_FAILURE;
    }
    for (l = 0; l < levels; l++)
        total += (size_t)level[l].iterations;
    ff.taps = fd.taps = NULL;
    if (total > 0 && ((sigma_fluid > 0 && gauss_filter(&ff, sigma_fluid)) ||
                      (sigma_diffusion > 0 && gauss_filter(&fd, sigma_diffusion))))
        goto done;
    for (l = levels - 1; l >= 0; l--) {
        if (lncc_run(level + l, masks ? masks[l].d_WF : NULL, masks ? masks[l].d_WM : NULL, &p, u[l], &ff, &fd, d_work,
                     (char *)d_stats + (size_t)SIFT3D_AMD_DEMONS_STATS_BYTES * rec, stream))
            goto done;
        rec += (size_t)level[l].iterations;
        if (l > 0 &&
            sift3d_field_prolong2_launch(u[l], u[l - 1], level[l - 1].nx, level[l - 1].ny, level[l - 1].nz, stream))
            goto done;
    }
    rc = SIFT3D_SUCCESS;
done:
    free(ff.taps);
    free(fd.taps);
    return rc;
}
