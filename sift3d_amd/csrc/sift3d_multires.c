/* sift3d_multires.c -- multi-resolution demons: the checked entries of the two grid transfers and the pyramid
 * driver (included at the end of sift3d_host.c, after sift3d_field_ops.c, whose range checks and drivers it uses).
 *
 * The contract is in include/sift3d_amd.h, "Multi-resolution demons".  The transfers are kernels of
 * sift3d_multires.hip, reached through the launchers below after the checks here; every level's loop is
 * sift3d_amd_demons_device_ex itself.  Arguments are checked before the device is touched, so bad input is refused
 * on a machine without a GPU too. */

int sift3d_restrict2_launch(const float *d_src, int nx, int ny, int nz, int nc, float *d_dst, float scale,
                            void *stream);
int sift3d_field_prolong2_launch(const float *d_coarse, float *d_fine, int nx, int ny, int nz, void *stream);

static int multires_half(int n)
{
    return (n + 1) / 2;
}

static size_t multires_coarse_voxels(int nx, int ny, int nz)
{
    return (size_t)multires_half(nx) * multires_half(ny) * multires_half(nz);
}

int sift3d_hip_restrict2(const float *d_src, int nx, int ny, int nz, int nc, float *d_dst, float scale, void *stream)
{
    static const char what[] = "sift3d_hip_restrict2";
    demons_range in[1], out[1];
    if (!d_src || !d_dst) {
        ERR("%s: NULL argument \n", what);
        return SIFT3D_FAILURE;
    }
    if (field_dims(what, nx, ny, nz))
        return SIFT3D_FAILURE;
    if (nc < 1) {
        ERR("%s: the number of channels must be positive \n", what);
        return SIFT3D_FAILURE;
    }
    if (!isfinite(scale)) {
        ERR("%s: the scale must be finite \n", what);
        return SIFT3D_FAILURE;
    }
    if (((uintptr_t)d_src | (uintptr_t)d_dst) & 3) {
        ERR("%s: a buffer is misaligned \n", what);
        return SIFT3D_FAILURE;
    }
    in[0].p = d_src; in[0].bytes = (size_t)nc * ((size_t)nx * ny * nz) * sizeof(float);
    out[0].p = d_dst; out[0].bytes = (size_t)nc * multires_coarse_voxels(nx, ny, nz) * sizeof(float);
    if (demons_aliased(out, 1, in, 1)) {
        ERR("%s: the output overlaps the input \n", what);
        return SIFT3D_FAILURE;
    }
    return sift3d_restrict2_launch(d_src, nx, ny, nz, nc, d_dst, scale, stream);
}

int sift3d_hip_field_prolong2(const float *d_coarse, float *d_fine, int nx, int ny, int nz, void *stream)
{
    static const char what[] = "sift3d_hip_field_prolong2";
    demons_range in[1], out[1];
    if (!d_coarse || !d_fine) {
        ERR("%s: NULL argument \n", what);
        return SIFT3D_FAILURE;
    }
    if (field_dims(what, nx, ny, nz))
        return SIFT3D_FAILURE;
    if (((uintptr_t)d_coarse | (uintptr_t)d_fine) & 3) {
        ERR("%s: a buffer is misaligned \n", what);
        return SIFT3D_FAILURE;
    }
    in[0].p = d_coarse; in[0].bytes = 3 * multires_coarse_voxels(nx, ny, nz) * sizeof(float);
    out[0].p = d_fine; out[0].bytes = field_bytes(nx, ny, nz);
    if (demons_aliased(out, 1, in, 1)) {
        ERR("%s: the output overlaps the input \n", what);
        return SIFT3D_FAILURE;
    }
    return sift3d_field_prolong2_launch(d_coarse, d_fine, nx, ny, nz, stream);
}

/* floats of the level fields 1 .. levels-1 under a finest grid (nx, ny, nz); each padded to a multiple of 4 floats,
 * so that every level's field is 16-byte aligned when the work buffer is */
static size_t multires_field_floats(int nx, int ny, int nz, int levels)
{
    size_t total = 0;
    int l;
    for (l = 1; l < levels; l++) {
        nx = multires_half(nx); ny = multires_half(ny); nz = multires_half(nz);
        total += (3 * ((size_t)nx * ny * nz) + 3) & ~(size_t)3;
    }
    return total;
}

/* the finest level's demons scratch, padded to a multiple of 4 floats */
static size_t multires_demons_floats(int nx, int ny, int nz, int nc, int update)
{
    return (sift3d_amd_demons_work_floats_ex(nx, ny, nz, nc, update) + 3) & ~(size_t)3;
}

size_t sift3d_amd_demons_multires_work_floats(int nx, int ny, int nz, int nc, int update, int levels)
{
    if (levels < 1 || levels > SIFT3D_AMD_DEMONS_MAX_LEVELS || !sift3d_amd_demons_work_floats_ex(nx, ny, nz, nc, update))
        return 0;
    return multires_demons_floats(nx, ny, nz, nc, update) + multires_field_floats(nx, ny, nz, levels);
}

int sift3d_amd_demons_multires_device(const sift3d_amd_demons_level *level, int levels, int nc, float *d_u,
                                      double alpha, double sigma_fluid, double sigma_diffusion, int update,
                                      int squarings, float *d_work, void *d_stats, void *stream)
{
    static const char what[] = "sift3d_amd_demons_multires_device";
    demons_range in[2 * SIFT3D_AMD_DEMONS_MAX_LEVELS], out[3];
    float *u[SIFT3D_AMD_DEMONS_MAX_LEVELS];
    size_t total = 0, rec;
    int l;
    if (!level || !d_u || !d_work || !d_stats) {
        ERR("%s: NULL argument \n", what);
        return SIFT3D_FAILURE;
    }
    if (levels < 1 || levels > SIFT3D_AMD_DEMONS_MAX_LEVELS) {
        ERR("%s: levels must be in [1, SIFT3D_AMD_DEMONS_MAX_LEVELS] \n", what);
        return SIFT3D_FAILURE;
    }
    if (update != SIFT3D_AMD_DEMONS_ADDITIVE && update != SIFT3D_AMD_DEMONS_DIFFEOMORPHIC) {
        ERR("%s: unknown update \n", what);
        return SIFT3D_FAILURE;
    }
    if (squarings < 0 || squarings > SIFT3D_AMD_FIELD_MAX_SQUARINGS) {
        ERR("%s: squarings must be in [0, SIFT3D_AMD_FIELD_MAX_SQUARINGS] \n", what);
        return SIFT3D_FAILURE;
    }
    if (!isfinite(sigma_fluid) || sigma_fluid < 0 || !isfinite(sigma_diffusion) || sigma_diffusion < 0) {
        ERR("%s: the sigmas must be finite and not negative \n", what);
        return SIFT3D_FAILURE;
    }
    if ((((uintptr_t)d_stats | (uintptr_t)d_work) & 7) || ((uintptr_t)d_u & 3)) {
        ERR("%s: a buffer is misaligned \n", what);
        return SIFT3D_FAILURE;
    }
    for (l = 0; l < levels; l++) {
        const sift3d_amd_demons_level *v = level + l;
        if (!v->d_F || !v->d_M) {
            ERR("%s: NULL argument \n", what);
            return SIFT3D_FAILURE;
        }
        if (demons_check(what, v->nx, v->ny, v->nz, v->mx, v->my, v->mz, nc, alpha))
            return SIFT3D_FAILURE;
        if (v->iterations < 0) {
            ERR("%s: the number of iterations must not be negative \n", what);
            return SIFT3D_FAILURE;
        }
        if (((uintptr_t)v->d_F | (uintptr_t)v->d_M) & 3) {
            ERR("%s: a buffer is misaligned \n", what);
            return SIFT3D_FAILURE;
        }
        if (l > 0) {
            const sift3d_amd_demons_level *f = v - 1;
            if (v->nx != multires_half(f->nx) || v->ny != multires_half(f->ny) || v->nz != multires_half(f->nz) ||
                v->mx != multires_half(f->mx) || v->my != multires_half(f->my) || v->mz != multires_half(f->mz)) {
                ERR("%s: a level's dimensions are not the halves of the level above \n", what);
                return SIFT3D_FAILURE;
            }
        }
        total += (size_t)v->iterations;
        in[2 * l].p = v->d_F;
        in[2 * l].bytes = (size_t)nc * ((size_t)v->nx * v->ny * v->nz) * sizeof(float);
        in[2 * l + 1].p = v->d_M;
        in[2 * l + 1].bytes = (size_t)nc * ((size_t)v->mx * v->my * v->mz) * sizeof(float);
    }
    out[0].p = d_u; out[0].bytes = field_bytes(level[0].nx, level[0].ny, level[0].nz);
    out[1].p = d_work;
    out[1].bytes = sift3d_amd_demons_multires_work_floats(level[0].nx, level[0].ny, level[0].nz, nc, update, levels) *
                   sizeof(float);
    out[2].p = d_stats; out[2].bytes = (size_t)SIFT3D_AMD_DEMONS_STATS_BYTES * (total > 0 ? total : 1);
    if (demons_aliased(out, 3, in, 2 * levels)) {
        ERR("%s: an output overlaps an input, the work buffer or another output \n", what);
        return SIFT3D_FAILURE;
    }
    /* the level fields: level 0 is d_u, the others follow the finest level's demons scratch in d_work */
    u[0] = d_u;
    {
        float *next = d_work + multires_demons_floats(level[0].nx, level[0].ny, level[0].nz, nc, update);
        for (l = 1; l < levels; l++) {
            u[l] = next;
            next += (3 * ((size_t)level[l].nx * level[l].ny * level[l].nz) + 3) & ~(size_t)3;
        }
    }
    for (l = 1; l < levels; l++)
        if (sift3d_restrict2_launch(u[l - 1], level[l - 1].nx, level[l - 1].ny, level[l - 1].nz, 3, u[l], 0.5f, stream))
            return SIFT3D_FAILURE;
    rec = 0;
    for (l = levels - 1; l >= 0; l--) {
        const sift3d_amd_demons_level *v = level + l;
        /* a level without iterations has nothing to run (and no statistics record of its own to point at) */
        if (v->iterations > 0 &&
            sift3d_amd_demons_device_ex(v->d_F, v->nx, v->ny, v->nz, v->d_M, v->mx, v->my, v->mz, nc, u[l],
                                        v->iterations, alpha, sigma_fluid, sigma_diffusion, update, squarings, d_work,
                                        (char *)d_stats + (size_t)SIFT3D_AMD_DEMONS_STATS_BYTES * rec, stream))
            return SIFT3D_FAILURE;
        rec += (size_t)v->iterations;
        if (l > 0 && sift3d_field_prolong2_launch(u[l], u[l - 1], level[l - 1].nx, level[l - 1].ny, level[l - 1].nz, stream))
            return SIFT3D_FAILURE;
    }
    return SIFT3D_SUCCESS;
}
