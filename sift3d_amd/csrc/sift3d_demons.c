/* sift3d_demons.c -- dense demons refinement of a displacement field: the checked force, the two grid transfers
 * and the one driver behind sift3d_amd_demons_device, sift3d_amd_demons_device_ex and
 * sift3d_amd_demons_multires_device, and sift3d_amd_logdemons_device, which runs its own iteration (logdemons_run)
 * through the same driver, and the masked forms of the force and of the two pyramid entries ("Masks in demons": the
 * same functions with the masks, which the unmasked entries pass as NULL) (included at the end of sift3d_host.c, after
 * sift3d_field_ops.c).
 *
 * The contract is in include/sift3d_amd.h, "Dense demons refinement", "Diffeomorphic demons", "Multi-resolution
 * demons" and "Log-domain demons".  The force and the additive update are kernels of sift3d_demons.hip, the bracket
 * and the symmetric update of sift3d_field_bracket.hip and the transfers kernels of sift3d_multires.hip, reached
 * through the launchers below after the checks here; the warp is sift3d_hip_warp_field, the exponential
 * field_exp_run, and the smoothing the detector's own blur (blur_level) per channel, as for the dense descriptors.
 * A demons problem is a list of levels (one for the two single-level entries): demons_drive validates it once,
 * builds the two Gaussian filters once and runs demons_run or logdemons_run, which check nothing, on every level.
 * Arguments are checked before the device is touched, so bad input is refused on a machine without a GPU too. */

int sift3d_demons_force_launch(const float *d_F, int nx, int ny, int nz, const float *d_W, const float *d_u, int mx,
                               int my, int mz, int nc, double alpha, float *d_step, void *d_stats, void *d_work,
                               void *stream, const float *d_WF, const float *d_WM);
int sift3d_demons_field_add_launch(float *d_u, const float *d_step, size_t n, void *stream);
int sift3d_restrict2_launch(const float *d_src, int nx, int ny, int nz, int nc, float *d_dst, float scale,
                            void *stream);
int sift3d_field_prolong2_launch(const float *d_coarse, float *d_fine, int nx, int ny, int nz, void *stream);
int sift3d_velocity_symmetrize_launch(float *d_v, const float *d_zf, const float *d_zb, size_t n, int bch,
                                      void *stream);

static int check_alpha(const char *what, double alpha)
{
    return !isfinite(alpha) || !(alpha > 0) ? refuse(what, "alpha must be positive and finite") : SIFT3D_SUCCESS;
}

static int check_update(const char *what, int update)
{
    return update != SIFT3D_AMD_DEMONS_ADDITIVE && update != SIFT3D_AMD_DEMONS_DIFFEOMORPHIC
               ? refuse(what, "unknown update") : SIFT3D_SUCCESS;
}

/* a non-NULL mask (n voxels) is 4-byte aligned and overlaps none of the nout ranges the call writes */
static int check_demons_mask(const char *what, const float *d_w, size_t n, const range_t *out, int nout)
{
    const range_t r = { d_w, n * sizeof(float) };
    if (!d_w)
        return SIFT3D_SUCCESS;
    if (check_aligned(what, 0, ADDR(d_w)))
        return SIFT3D_FAILURE;
    return ranges_aliased(out, nout, &r, 1) ? refuse(what, ALIASED) : SIFT3D_SUCCESS;
}

/* the shared body of the two force entries: d_WF, d_WM are the masks ("Masks in demons") or NULL */
static int demons_force_entry(const char *what, const float *d_F, int nx, int ny, int nz, const float *d_W,
                              const float *d_u, int mx, int my, int mz, int nc, double alpha, float *d_step,
                              void *d_stats, void *d_work, void *stream, const float *d_WF, const float *d_WM)
{
    if (!d_F || !d_W || !d_u || !d_step || !d_stats || !d_work)
        return refuse(what, "NULL argument");
    if (check_dims(what, nx, ny, nz) || check_dims(what, mx, my, mz) || check_channels(what, nc) ||
        check_alpha(what, alpha) ||
        check_aligned(what, ADDR(d_stats) | ADDR(d_work), ADDR(d_F) | ADDR(d_W) | ADDR(d_u) | ADDR(d_step)))
        return SIFT3D_FAILURE;
    {
        const range_t in[] = { { d_F, image_bytes(nx, ny, nz, nc) }, { d_W, image_bytes(nx, ny, nz, nc) },
                               { d_u, field_bytes(nx, ny, nz) } };
        const range_t out[] = { { d_step, field_bytes(nx, ny, nz) }, { d_stats, SIFT3D_AMD_DEMONS_STATS_BYTES },
                                { d_work, SIFT3D_AMD_DEMONS_FORCE_WORK_BYTES } };
        if (ranges_aliased(out, 3, in, 3))
            return refuse(what, ALIASED);
        if (check_demons_mask(what, d_WF, grid_voxels(nx, ny, nz), out, 3) ||
            check_demons_mask(what, d_WM, grid_voxels(mx, my, mz), out, 3))
            return SIFT3D_FAILURE;
    }
    return sift3d_demons_force_launch(d_F, nx, ny, nz, d_W, d_u, mx, my, mz, nc, alpha, d_step, d_stats, d_work,
                                      stream, d_WF, d_WM);
}

int sift3d_hip_demons_force(const float *d_F, int nx, int ny, int nz, const float *d_W, const float *d_u, int mx,
                            int my, int mz, int nc, double alpha, float *d_step, void *d_stats, void *d_work,
                            void *stream)
{
    return demons_force_entry("sift3d_hip_demons_force", d_F, nx, ny, nz, d_W, d_u, mx, my, mz, nc, alpha, d_step,
                              d_stats, d_work, stream, NULL, NULL);
}

int sift3d_hip_demons_force_masked(const float *d_F, int nx, int ny, int nz, const float *d_W, const float *d_u, int mx,
                                   int my, int mz, int nc, double alpha, float *d_step, void *d_stats, void *d_work,
                                   void *stream, const float *d_WF, const float *d_WM)
{
    return demons_force_entry("sift3d_hip_demons_force_masked", d_F, nx, ny, nz, d_W, d_u, mx, my, mz, nc, alpha,
                              d_step, d_stats, d_work, stream, d_WF, d_WM);
}

/* ---- the grid transfers ---- */

static int multires_half(int n)
{
    return (n + 1) / 2;
}

static size_t multires_coarse_voxels(int nx, int ny, int nz)
{
    return grid_voxels(multires_half(nx), multires_half(ny), multires_half(nz));
}

int sift3d_hip_restrict2(const float *d_src, int nx, int ny, int nz, int nc, float *d_dst, float scale, void *stream)
{
    static const char what[] = "sift3d_hip_restrict2";
    if (!d_src || !d_dst)
        return refuse(what, "NULL argument");
    if (check_dims(what, nx, ny, nz) || check_channels(what, nc))
        return SIFT3D_FAILURE;
    if (!isfinite(scale))
        return refuse(what, "the scale must be finite");
    if (check_aligned(what, 0, ADDR(d_src) | ADDR(d_dst)))
        return SIFT3D_FAILURE;
    if (ranges_overlap((range_t){ d_dst, (size_t)nc * multires_coarse_voxels(nx, ny, nz) * sizeof(float) },
                       (range_t){ d_src, image_bytes(nx, ny, nz, nc) }))
        return refuse(what, "the output overlaps the input");
    return sift3d_restrict2_launch(d_src, nx, ny, nz, nc, d_dst, scale, stream);
}

int sift3d_hip_field_prolong2(const float *d_coarse, float *d_fine, int nx, int ny, int nz, void *stream)
{
    static const char what[] = "sift3d_hip_field_prolong2";
    if (!d_coarse || !d_fine)
        return refuse(what, "NULL argument");
    if (check_dims(what, nx, ny, nz) || check_aligned(what, 0, ADDR(d_coarse) | ADDR(d_fine)))
        return SIFT3D_FAILURE;
    if (ranges_overlap((range_t){ d_fine, field_bytes(nx, ny, nz) },
                       (range_t){ d_coarse, 3 * multires_coarse_voxels(nx, ny, nz) * sizeof(float) }))
        return refuse(what, "the output overlaps the input");
    return sift3d_field_prolong2_launch(d_coarse, d_fine, nx, ny, nz, stream);
}

/* ---- the work buffer ---- */

/* One level's scratch, as offsets in floats into d_work: the force's partials at 0, W (nc planes), delta (3), the
 * blur's two intermediates; the diffeomorphic update adds u_new (3) and the exponential's second buffer (3).  The
 * size functions and demons_run both read it from here. */
typedef struct {
    size_t W, step, tmp, unew, pp, total;
} demons_layout;

static demons_layout demons_layout_of(size_t n, int nc, int update)
{
    const size_t extra = update == SIFT3D_AMD_DEMONS_DIFFEOMORPHIC ? 3 * n : 0;
    demons_layout l;
    l.W = SIFT3D_AMD_DEMONS_FORCE_WORK_BYTES / sizeof(float);
    l.step = l.W + (size_t)nc * n;
    l.tmp = l.step + 3 * n;
    l.unew = l.tmp + 2 * n;
    l.pp = l.unew + extra;
    l.total = l.pp + extra;
    return l;
}

size_t sift3d_amd_demons_work_floats_ex(int nx, int ny, int nz, int nc, int update)
{
    if (nx <= 0 || ny <= 0 || nz <= 0 || nc < 1 ||
        (update != SIFT3D_AMD_DEMONS_ADDITIVE && update != SIFT3D_AMD_DEMONS_DIFFEOMORPHIC))
        return 0;
    return demons_layout_of(grid_voxels(nx, ny, nz), nc, update).total;
}

size_t sift3d_amd_demons_work_floats(int nx, int ny, int nz, int nc)
{
    return sift3d_amd_demons_work_floats_ex(nx, ny, nz, nc, SIFT3D_AMD_DEMONS_ADDITIVE);
}

static size_t pad4(size_t floats)
{
    return (floats + 3) & ~(size_t)3;
}

/* One level's scratch of log-domain demons, as offsets in floats into d_work: the force's partials at 0 (SYMMETRIC:
 * then the backward statistics, 4 floats), W (nc planes), delta (3), the blur's two intermediates, e = exp(+-v) and
 * the exponential's second buffer (3 each; after the forces: n = -v), z (3: the BCH output, Z_f); SYMMETRIC adds
 * delta_b and Z_b (3 each).  The header states the total. */
typedef struct {
    size_t bstats, W, step, tmp, e, pp, z, stepb, zb, total;
} logdemons_layout;

static logdemons_layout logdemons_layout_of(size_t n, int nc, int symmetric)
{
    logdemons_layout l;
    l.bstats = SIFT3D_AMD_DEMONS_FORCE_WORK_BYTES / sizeof(float);
    l.W = l.bstats + (symmetric ? 4 : 0);
    l.step = l.W + (size_t)nc * n;
    l.tmp = l.step + 3 * n;
    l.e = l.tmp + 2 * n;
    l.pp = l.e + 3 * n;
    l.z = l.pp + 3 * n;
    l.stepb = l.z + 3 * n;
    l.zb = l.stepb + (symmetric ? 3 * n : 0);
    l.total = l.zb + (symmetric ? 3 * n : 0);
    return l;
}

/* Where level l's field (l >= 1) starts in the pyramid's d_work, in floats, under a finest grid (nx, ny, nz): after
 * level 0's scratch, which every level uses in turn, and the fields of levels 1 .. l-1, each padded to a multiple
 * of 4 floats so that every field is 16-byte aligned when d_work is.  l == levels gives the whole buffer.  A level
 * field is safe from its own level's scratch only because no coarser level needs more scratch than level 0 (a
 * halved grid has no more voxels); demons_validate refuses a level for which that does not hold. */
static size_t pyramid_field_offset(size_t scratch, int nx, int ny, int nz, int l)
{
    size_t at = pad4(scratch);
    int k;
    for (k = 1; k < l; k++) {
        nx = multires_half(nx); ny = multires_half(ny); nz = multires_half(nz);
        at += pad4(3 * grid_voxels(nx, ny, nz));
    }
    return at;
}

size_t sift3d_amd_demons_multires_work_floats(int nx, int ny, int nz, int nc, int update, int levels)
{
    if (levels < 1 || levels > SIFT3D_AMD_DEMONS_MAX_LEVELS ||
        !sift3d_amd_demons_work_floats_ex(nx, ny, nz, nc, update))
        return 0;
    return pyramid_field_offset(sift3d_amd_demons_work_floats_ex(nx, ny, nz, nc, update), nx, ny, nz, levels);
}

/* ---- the driver ---- */

/* logdomain == 0: the displacement drivers (update, squarings); 1: log-domain demons, squarings = Kv, and update is
 * not read */
typedef struct {
    int nc;
    double alpha, sigma_fluid, sigma_diffusion;
    int update, squarings;
    int logdomain, symmetric, bch;
} demons_params;

/* one level's scratch in floats */
static size_t demons_scratch(const demons_params *p, int nx, int ny, int nz)
{
    return p->logdomain ? logdemons_layout_of(grid_voxels(nx, ny, nz), p->nc, p->symmetric).total
                        : sift3d_amd_demons_work_floats_ex(nx, ny, nz, p->nc, p->update);
}

static int check_log(const char *what, const demons_params *p)
{
    if (p->symmetric != 0 && p->symmetric != 1)
        return refuse(what, "symmetric must be 0 or 1");
    return p->bch != 0 && p->bch != 1 ? refuse(what, "bch must be 0 or 1") : SIFT3D_SUCCESS;
}

/* 0 when the problem may run: level [levels] (level 0 the finest), masks [levels] or NULL, the field d_u on level
 * 0's grid, work_floats floats of d_work, one statistics record per iteration (room for one when there is none) */
static int demons_validate(const char *what, const sift3d_amd_demons_level *level,
                           const sift3d_amd_demons_level_masks *masks, int levels, const demons_params *p,
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
    if ((p->logdomain ? check_log(what, p) : check_update(what, p->update)) ||
        check_squarings(what, p->squarings) || check_channels(what, p->nc) || check_alpha(what, p->alpha) ||
        check_sigmas(what, p->sigma_fluid, p->sigma_diffusion))
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
        if (p->logdomain && p->symmetric && (v->nx != v->mx || v->ny != v->my || v->nz != v->mz))
            return refuse(what, "the symmetric update needs fixed and moving volumes of one shape");
        if (demons_scratch(p, v->nx, v->ny, v->nz) > demons_scratch(p, level->nx, level->ny, level->nz))
            return refuse(what, "a level needs more scratch than the finest");
        total += (size_t)v->iterations;
        or4 |= ADDR(v->d_F) | ADDR(v->d_M);
        in[2 * l] = (range_t){ v->d_F, image_bytes(v->nx, v->ny, v->nz, p->nc) };
        in[2 * l + 1] = (range_t){ v->d_M, image_bytes(v->mx, v->my, v->mz, p->nc) };
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

/* each of the 3 channels of src [3][nz][ny][nx] through blur_level into dst (units 1, unit 1.0); dst may be src
 * (blur_level's x pass reads src into the first intermediate and only its last pass writes dst) */
static int demons_blur3(const float *src, float *dst, const int *dims, const filter_t *f, float *tmp, void *stream)
{
    static const double lu[3] = { 1.0, 1.0, 1.0 };
    const size_t n = grid_voxels(dims[0], dims[1], dims[2]);
    int c;
    for (c = 0; c < 3; c++)
        if (blur_level(NULL, src + (size_t)c * n, dst + (size_t)c * n, dims, lu, f, stream, tmp, tmp + n, -1, NULL))
            return SIFT3D_FAILURE;
    return SIFT3D_SUCCESS;
}

/* v->iterations iterations of one level on its field d_u, unchecked; d_WF, d_WM: the level's masks or NULL; ff, fd:
 * the filters of the two sigmas (read only where the sigma is positive); one statistics record per iteration from
 * d_stats on */
static int demons_run(const sift3d_amd_demons_level *v, const float *d_WF, const float *d_WM, const demons_params *p,
                      float *d_u, const filter_t *ff, const filter_t *fd, float *d_work, char *d_stats, void *stream)
{
    const int dims[3] = { v->nx, v->ny, v->nz };
    const size_t n = grid_voxels(v->nx, v->ny, v->nz);
    const demons_layout at = demons_layout_of(n, p->nc, p->update);
    float *d_W = d_work + at.W, *d_step = d_work + at.step, *d_tmp = d_work + at.tmp, *d_unew = d_work + at.unew,
          *d_pp = d_work + at.pp;
    int k;
    for (k = 0; k < v->iterations; k++) {
        const float *e = d_step;
        if (sift3d_hip_warp_field(v->d_M, v->mx, v->my, v->mz, p->nc, d_u, v->nx, v->ny, v->nz, d_W,
                                  SIFT3D_AMD_INTERP_LINEAR, 0.0f, stream) ||
            sift3d_demons_force_launch(v->d_F, v->nx, v->ny, v->nz, d_W, d_u, v->mx, v->my, v->mz, p->nc, p->alpha,
                                       d_step, d_stats + (size_t)SIFT3D_AMD_DEMONS_STATS_BYTES * k, d_work, stream,
                                       d_WF, d_WM))
            return SIFT3D_FAILURE;
        if (p->sigma_fluid > 0 && demons_blur3(d_step, d_step, dims, ff, d_tmp, stream))
            return SIFT3D_FAILURE;
        if (p->update == SIFT3D_AMD_DEMONS_ADDITIVE) {
            if (sift3d_demons_field_add_launch(d_u, d_step, 3 * n, stream) ||
                (p->sigma_diffusion > 0 && demons_blur3(d_u, d_u, dims, fd, d_tmp, stream)))
                return SIFT3D_FAILURE;
            continue;
        }
        /* e = exp(delta): w_0 = delta * 2^-K, then K squarings between d_pp and d_step (delta is read only by the
         * scaling); K == 0: e = delta itself */
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

/* v->iterations iterations of log-domain demons on one level's velocity d_v, unchecked ("Log-domain demons": LOG, or
 * SYMMETRIC with p->symmetric); arguments as demons_run's */
static int logdemons_run(const sift3d_amd_demons_level *v, const float *d_WF, const float *d_WM,
                         const demons_params *p, float *d_v, const filter_t *ff, const filter_t *fd, float *d_work,
                         char *d_stats, void *stream)
{
    const int dims[3] = { v->nx, v->ny, v->nz };
    const size_t n = grid_voxels(v->nx, v->ny, v->nz);
    const logdemons_layout at = logdemons_layout_of(n, p->nc, p->symmetric);
    float *d_W = d_work + at.W, *d_step = d_work + at.step, *d_tmp = d_work + at.tmp, *d_e = d_work + at.e,
          *d_pp = d_work + at.pp, *d_z = d_work + at.z, *d_stepb = d_work + at.stepb, *d_zb = d_work + at.zb;
    const int K = p->squarings;
    int k;
    for (k = 0; k < v->iterations; k++) {
        /* e = exp(v); K == 0: v itself */
        const float *e = K > 0 ? d_e : d_v;
        if ((K > 0 && field_exp_run(d_v, v->nx, v->ny, v->nz, K, 1.0, d_e, d_pp, stream)) ||
            sift3d_hip_warp_field(v->d_M, v->mx, v->my, v->mz, p->nc, e, v->nx, v->ny, v->nz, d_W,
                                  SIFT3D_AMD_INTERP_LINEAR, 0.0f, stream) ||
            sift3d_demons_force_launch(v->d_F, v->nx, v->ny, v->nz, d_W, e, v->mx, v->my, v->mz, p->nc, p->alpha,
                                       d_step, d_stats + (size_t)SIFT3D_AMD_DEMONS_STATS_BYTES * k, d_work, stream,
                                       d_WF, d_WM) ||
            (p->sigma_fluid > 0 && demons_blur3(d_step, d_step, dims, ff, d_tmp, stream)))
            return SIFT3D_FAILURE;
        if (!p->symmetric) {
            if (p->bch ? (sift3d_field_bracket_launch(d_v, d_step, v->nx, v->ny, v->nz, d_z, SIFT3D_AMD_FIELD_BCH1,
                                                      stream) ||
                          (p->sigma_diffusion > 0 ? demons_blur3(d_z, d_v, dims, fd, d_tmp, stream)
                                                  : sift3d_hip_memcpy_d2d(d_v, d_z, 3 * n * sizeof(float), stream)))
                       : (sift3d_demons_field_add_launch(d_v, d_step, 3 * n, stream) ||
                          (p->sigma_diffusion > 0 && demons_blur3(d_v, d_v, dims, fd, d_tmp, stream))))
                return SIFT3D_FAILURE;
            continue;
        }
        /* the backward force: the roles of F and M, and of their masks, exchanged (one shape), read through
         * e- = exp(-v) */
        if (field_exp_run(d_v, v->nx, v->ny, v->nz, K, -1.0, d_e, d_pp, stream) ||
            sift3d_hip_warp_field(v->d_F, v->nx, v->ny, v->nz, p->nc, d_e, v->nx, v->ny, v->nz, d_W,
                                  SIFT3D_AMD_INTERP_LINEAR, 0.0f, stream) ||
            sift3d_demons_force_launch(v->d_M, v->nx, v->ny, v->nz, d_W, d_e, v->nx, v->ny, v->nz, p->nc, p->alpha,
                                       d_stepb, d_work + at.bstats, d_work, stream, d_WM, d_WF) ||
            (p->sigma_fluid > 0 && demons_blur3(d_stepb, d_stepb, dims, ff, d_tmp, stream)))
            return SIFT3D_FAILURE;
        if (p->bch) {
            /* n = -v into e's buffer, which the forces have finished with */
            if (sift3d_field_scale_launch(d_e, d_v, 3 * n, -1.0f, stream) ||
                sift3d_field_bracket_launch(d_v, d_step, v->nx, v->ny, v->nz, d_z, SIFT3D_AMD_FIELD_BCH1, stream) ||
                sift3d_field_bracket_launch(d_e, d_stepb, v->nx, v->ny, v->nz, d_zb, SIFT3D_AMD_FIELD_BCH1, stream) ||
                sift3d_velocity_symmetrize_launch(d_v, d_z, d_zb, 3 * n, 1, stream))
                return SIFT3D_FAILURE;
        } else if (sift3d_velocity_symmetrize_launch(d_v, d_step, d_stepb, 3 * n, 0, stream))
            return SIFT3D_FAILURE;
        if (p->sigma_diffusion > 0 && demons_blur3(d_v, d_v, dims, fd, d_tmp, stream))
            return SIFT3D_FAILURE;
    }
    return SIFT3D_SUCCESS;
}

/* The three entries: validate once, restrict the field down the pyramid (nothing with one level), build the two
 * filters once when there is an iteration to run, then per level, coarsest first, run it and hand its field up. */
static int demons_drive(const char *what, const sift3d_amd_demons_level *level,
                        const sift3d_amd_demons_level_masks *masks, int levels, const demons_params *p, float *d_u,
                        float *d_work, size_t work_floats, void *d_stats, void *stream)
{
    float *u[SIFT3D_AMD_DEMONS_MAX_LEVELS];
    filter_t ff, fd;
    size_t rec = 0, total = 0;
    int l, rc = SIFT3D_FAILURE;
    if (demons_validate(what, level, masks, levels, p, d_u, d_work, work_floats, d_stats))
        return SIFT3D_FAILURE;
    /* the level fields: level 0 is d_u, the others follow the finest level's scratch in d_work */
    u[0] = d_u;
    for (l = 1; l < levels; l++) {
        u[l] = d_work + pyramid_field_offset(demons_scratch(p, level->nx, level->ny, level->nz), level->nx, level->ny,
                                             level->nz, l);
        if (sift3d_restrict2_launch(u[l - 1], level[l - 1].nx, level[l - 1].ny, level[l - 1].nz, 3, u[l], 0.5f,
                                    stream))
            return SIFT3D_FAILURE;
    }
    for (l = 0; l < levels; l++)
        total += (size_t)level[l].iterations;
    ff.taps = fd.taps = NULL;
    if (total > 0 && ((p->sigma_fluid > 0 && gauss_filter(&ff, p->sigma_fluid)) ||
                      (p->sigma_diffusion > 0 && gauss_filter(&fd, p->sigma_diffusion))))
        goto done;
    for (l = levels - 1; l >= 0; l--) {
        if ((p->logdomain ? logdemons_run : demons_run)(level + l, masks ? masks[l].d_WF : NULL,
                                                  masks ? masks[l].d_WM : NULL, p, u[l], &ff, &fd, d_work,
                                                  (char *)d_stats + (size_t)SIFT3D_AMD_DEMONS_STATS_BYTES * rec,
                                                  stream))
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

int sift3d_amd_demons_device_ex(const float *d_F, int nx, int ny, int nz, const float *d_M, int mx, int my, int mz,
                                int nc, float *d_u, int iterations, double alpha, double sigma_fluid,
                                double sigma_diffusion, int update, int squarings, float *d_work, void *d_stats,
                                void *stream)
{
    const sift3d_amd_demons_level v = { d_F, nx, ny, nz, d_M, mx, my, mz, iterations };
    const demons_params p = { nc, alpha, sigma_fluid, sigma_diffusion, update, squarings, 0, 0, 0 };
    return demons_drive("sift3d_amd_demons_device_ex", &v, NULL, 1, &p, d_u, d_work,
                        sift3d_amd_demons_work_floats_ex(nx, ny, nz, nc, update), d_stats, stream);
}

int sift3d_amd_demons_device(const float *d_F, int nx, int ny, int nz, const float *d_M, int mx, int my, int mz,
                             int nc, float *d_u, int iterations, double alpha, double sigma_fluid,
                             double sigma_diffusion, float *d_work, void *d_stats, void *stream)
{
    const sift3d_amd_demons_level v = { d_F, nx, ny, nz, d_M, mx, my, mz, iterations };
    const demons_params p = { nc, alpha, sigma_fluid, sigma_diffusion, SIFT3D_AMD_DEMONS_ADDITIVE, 0, 0, 0, 0 };
    return demons_drive("sift3d_amd_demons_device", &v, NULL, 1, &p, d_u, d_work,
                        sift3d_amd_demons_work_floats(nx, ny, nz, nc), d_stats, stream);
}

int sift3d_amd_demons_multires_device(const sift3d_amd_demons_level *level, int levels, int nc, float *d_u,
                                      double alpha, double sigma_fluid, double sigma_diffusion, int update,
                                      int squarings, float *d_work, void *d_stats, void *stream)
{
    const demons_params p = { nc, alpha, sigma_fluid, sigma_diffusion, update, squarings, 0, 0, 0 };
    /* (a NULL level table is refused by the driver before the size matters) */
    const size_t need = level ? sift3d_amd_demons_multires_work_floats(level->nx, level->ny, level->nz, nc, update,
                                                                       levels) : 0;
    return demons_drive("sift3d_amd_demons_multires_device", level, NULL, levels, &p, d_u, d_work, need, d_stats,
                        stream);
}

int sift3d_amd_demons_masked_device(const sift3d_amd_demons_level *level, const sift3d_amd_demons_level_masks *masks,
                                    int levels, int nc, float *d_u, double alpha, double sigma_fluid,
                                    double sigma_diffusion, int update, int squarings, float *d_work, void *d_stats,
                                    void *stream)
{
    const demons_params p = { nc, alpha, sigma_fluid, sigma_diffusion, update, squarings, 0, 0, 0 };
    const size_t need = level ? sift3d_amd_demons_multires_work_floats(level->nx, level->ny, level->nz, nc, update,
                                                                       levels) : 0;
    return demons_drive("sift3d_amd_demons_masked_device", level, masks, levels, &p, d_u, d_work, need, d_stats,
                        stream);
}

size_t sift3d_amd_logdemons_work_floats(int nx, int ny, int nz, int nc, int symmetric, int levels)
{
    if (nx <= 0 || ny <= 0 || nz <= 0 || nc < 1 || (symmetric != 0 && symmetric != 1) || levels < 1 ||
        levels > SIFT3D_AMD_DEMONS_MAX_LEVELS)
        return 0;
    return pyramid_field_offset(logdemons_layout_of(grid_voxels(nx, ny, nz), nc, symmetric).total, nx, ny, nz, levels);
}

int sift3d_amd_logdemons_device(const sift3d_amd_demons_level *level, int levels, int nc, float *d_v, double alpha,
                                double sigma_fluid, double sigma_diffusion, int symmetric, int bch,
                                int velocity_squarings, float *d_work, void *d_stats, void *stream)
{
    const demons_params p = { nc, alpha, sigma_fluid, sigma_diffusion, 0, velocity_squarings, 1, symmetric, bch };
    /* (a NULL level table and a bad `symmetric` are refused by the driver before the size matters) */
    const size_t need = level ? sift3d_amd_logdemons_work_floats(level->nx, level->ny, level->nz, nc, symmetric, levels)
                              : 0;
    return demons_drive("sift3d_amd_logdemons_device", level, NULL, levels, &p, d_v, d_work, need, d_stats, stream);
}

int sift3d_amd_logdemons_masked_device(const sift3d_amd_demons_level *level,
                                       const sift3d_amd_demons_level_masks *masks, int levels, int nc, float *d_v,
                                       double alpha, double sigma_fluid, double sigma_diffusion, int symmetric, int bch,
                                       int velocity_squarings, float *d_work, void *d_stats, void *stream)
{
    const demons_params p = { nc, alpha, sigma_fluid, sigma_diffusion, 0, velocity_squarings, 1, symmetric, bch };
    const size_t need = level ? sift3d_amd_logdemons_work_floats(level->nx, level->ny, level->nz, nc, symmetric, levels)
                              : 0;
    return demons_drive("sift3d_amd_logdemons_masked_device", level, masks, levels, &p, d_v, d_work, need, d_stats,
                        stream);
}
