/* sift3d_discrete.c -- discrete displacement search: the checked entries of the cost volume, the coupled selection,
 * the block-field smoothing and expansion, and the coarse-to-fine driver (included at the end of sift3d_host.c, after
 * sift3d_demons.c and sift3d_block_fit.c, whose pyramid helpers and fill launcher it uses as they are).
 *
 * The contract is in include/sift3d_amd.h, "Discrete displacement search".  The kernels are sift3d_discrete.hip's,
 * reached through the launchers below after the checks here.  Arguments are checked before the device is touched, so
 * bad input is refused on a machine without a GPU too. */

int sift3d_cost_volume_launch(const float *d_F, const float *d_W, int nc, int nx, int ny, int nz, const float *d_VF,
                              const float *d_VW, int radius, float *d_cost, void *stream);
int sift3d_cost_select_launch(const float *d_cost, int nbx, int nby, int nbz, int radius, const float *d_u,
                              double theta, float *d_v, float *d_data, void *d_stats, void *d_work, void *stream);
int sift3d_block_field_smooth_launch(const float *d_src, float *d_dst, int nbx, int nby, int nbz, void *stream);
int sift3d_block_field_expand_launch(const float *d_b, int nbx, int nby, int nbz, float *d_w, int nx, int ny, int nz,
                                     void *stream);

static int discrete_radius_ok(int radius)
{
    return radius >= 1 && radius <= SIFT3D_AMD_DISCRETE_MAX_RADIUS;
}

static size_t discrete_labels(int radius)
{
    const size_t d = 2 * (size_t)radius + 1;
    return d * d * d;
}

static int check_discrete_radius(const char *what, int radius)
{
    return !discrete_radius_ok(radius) ? refuse(what, "radius must be in [1, SIFT3D_AMD_DISCRETE_MAX_RADIUS]")
                                       : SIFT3D_SUCCESS;
}

static int check_discrete_channels(const char *what, int nc)
{
    return nc < 1 || nc > SIFT3D_AMD_DISCRETE_MAX_CHANNELS
               ? refuse(what, "the number of channels must be in [1, SIFT3D_AMD_DISCRETE_MAX_CHANNELS]")
               : SIFT3D_SUCCESS;
}

static int check_discrete_theta(const char *what, double theta)
{
    return !isfinite(theta) || theta < 0 ? refuse(what, "theta must be finite and not negative") : SIFT3D_SUCCESS;
}

static int check_discrete_passes(const char *what, int passes)
{
    return passes < 0 || passes > SIFT3D_AMD_DISCRETE_MAX_PASSES
               ? refuse(what, "passes must be in [0, SIFT3D_AMD_DISCRETE_MAX_PASSES]") : SIFT3D_SUCCESS;
}

/* ---- cost volume ---- */

size_t sift3d_amd_cost_volume_bytes(int nx, int ny, int nz, int radius)
{
    if (nx < 4 || ny < 4 || nz < 4 || !discrete_radius_ok(radius))
        return 0;
    return grid_voxels(nx / 4, ny / 4, nz / 4) * discrete_labels(radius) * sizeof(float);
}

size_t sift3d_amd_cost_volume_work_bytes(int nx, int ny, int nz, int nc, int radius)
{
    return 0;
}

int sift3d_hip_cost_volume(const float *d_F, const float *d_W, int nc, int nx, int ny, int nz, const float *d_VF,
                           const float *d_VW, int radius, float *d_cost, void *d_work, void *stream)
{
    static const char what[] = "sift3d_hip_cost_volume";
    if (!d_F || !d_W || !d_cost)
        return refuse(what, "NULL argument");
    if (check_dims(what, nx, ny, nz))
        return SIFT3D_FAILURE;
    if (nx < 4 || ny < 4 || nz < 4)
        return refuse(what, "every dimension must hold a block of 4 voxels");
    if (check_discrete_channels(what, nc) || check_discrete_radius(what, radius) ||
        check_aligned(what, 0, ADDR(d_F) | ADDR(d_W) | ADDR(d_VF) | ADDR(d_VW) | ADDR(d_cost)))
        return SIFT3D_FAILURE;
    {
        const size_t vol = image_bytes(nx, ny, nz, 1);
        const range_t in[] = { { d_F, vol * nc }, { d_W, vol * nc }, { d_VF, d_VF ? vol : 0 },
                               { d_VW, d_VW ? vol : 0 } };
        const range_t out[] = { { d_cost, sift3d_amd_cost_volume_bytes(nx, ny, nz, radius) } };
        if (ranges_aliased(out, 1, in, 4))
            return refuse(what, ALIASED);
    }
    return sift3d_cost_volume_launch(d_F, d_W, nc, nx, ny, nz, d_VF, d_VW, radius, d_cost, stream);
}

/* ---- coupled selection ---- */

size_t sift3d_amd_cost_select_work_bytes(int nbx, int nby, int nbz)
{
    return nbx <= 0 || nby <= 0 || nbz <= 0 ? 0 : SIFT3D_AMD_COST_SELECT_WORK_BYTES;
}

int sift3d_hip_cost_select(const float *d_cost, int nbx, int nby, int nbz, int radius, const float *d_u, double theta,
                           float *d_v, float *d_data, void *d_stats, void *d_work, void *stream)
{
    static const char what[] = "sift3d_hip_cost_select";
    size_t nb;
    if (!d_cost || !d_u || !d_v || !d_data || !d_stats || !d_work)
        return refuse(what, "NULL argument");
    if (check_dims(what, nbx, nby, nbz) || check_discrete_radius(what, radius) || check_discrete_theta(what, theta) ||
        check_aligned(what, ADDR(d_stats) | ADDR(d_work), ADDR(d_cost) | ADDR(d_u) | ADDR(d_v) | ADDR(d_data)))
        return SIFT3D_FAILURE;
    nb = grid_voxels(nbx, nby, nbz);
    {
        const range_t in[] = { { d_cost, nb * discrete_labels(radius) * sizeof(float) },
                               { d_u, 3 * nb * sizeof(float) } };
        const range_t out[] = { { d_v, 3 * nb * sizeof(float) }, { d_data, nb * sizeof(float) },
                                { d_stats, SIFT3D_AMD_DEMONS_STATS_BYTES },
                                { d_work, SIFT3D_AMD_COST_SELECT_WORK_BYTES } };
        if (ranges_aliased(out, 4, in, 2))
            return refuse(what, ALIASED);
    }
    return sift3d_cost_select_launch(d_cost, nbx, nby, nbz, radius, d_u, theta, d_v, d_data, d_stats, d_work, stream);
}

/* ---- block-field smoothing and expansion ---- */

size_t sift3d_amd_block_field_smooth_work_bytes(int nbx, int nby, int nbz, int passes)
{
    if (nbx <= 0 || nby <= 0 || nbz <= 0 || passes < 0 || passes > SIFT3D_AMD_DISCRETE_MAX_PASSES)
        return 0;
    return passes >= 2 ? 3 * grid_voxels(nbx, nby, nbz) * sizeof(float) : 0;
}

/* `passes` passes from d_src to d_dst, unchecked: the passes alternate between d_dst and d_tmp (3 nb floats, read
 * with passes >= 2 only) so that the last one writes d_dst */
static int block_field_smooth_run(const float *d_src, float *d_dst, int nbx, int nby, int nbz, int passes,
                                  float *d_tmp, void *stream)
{
    const float *from = d_src;
    int p;
    if (passes == 0)
        return sift3d_hip_memcpy_d2d(d_dst, d_src, 3 * grid_voxels(nbx, nby, nbz) * sizeof(float), stream);
    for (p = 1; p <= passes; p++) {
        float *to = (passes - p) % 2 == 0 ? d_dst : d_tmp;
        if (sift3d_block_field_smooth_launch(from, to, nbx, nby, nbz, stream))
            return SIFT3D_FAILURE;
        from = to;
    }
    return SIFT3D_SUCCESS;
}

int sift3d_hip_block_field_smooth(const float *d_src, float *d_dst, int nbx, int nby, int nbz, int passes,
                                  void *d_work, void *stream)
{
    static const char what[] = "sift3d_hip_block_field_smooth";
    size_t bytes, need;
    if (!d_src || !d_dst)
        return refuse(what, "NULL argument");
    if (check_dims(what, nbx, nby, nbz) || check_discrete_passes(what, passes))
        return SIFT3D_FAILURE;
    need = sift3d_amd_block_field_smooth_work_bytes(nbx, nby, nbz, passes);
    if (need && !d_work)
        return refuse(what, "NULL argument");
    if (check_aligned(what, ADDR(d_work), ADDR(d_src) | ADDR(d_dst)))
        return SIFT3D_FAILURE;
    bytes = 3 * grid_voxels(nbx, nby, nbz) * sizeof(float);
    {
        const range_t in[] = { { d_src, bytes } };
        const range_t out[] = { { d_dst, bytes }, { d_work, d_work ? need : 0 } };
        if (ranges_aliased(out, 2, in, 1))
            return refuse(what, ALIASED);
    }
    return block_field_smooth_run(d_src, d_dst, nbx, nby, nbz, passes, (float *)d_work, stream);
}

int sift3d_hip_block_field_expand(const float *d_b, int nbx, int nby, int nbz, float *d_w, int nx, int ny, int nz,
                                  void *stream)
{
    static const char what[] = "sift3d_hip_block_field_expand";
    if (!d_b || !d_w)
        return refuse(what, "NULL argument");
    if (check_dims(what, nbx, nby, nbz) || check_dims(what, nx, ny, nz))
        return SIFT3D_FAILURE;
    if (nbx != nx / 4 || nby != ny / 4 || nbz != nz / 4)
        return refuse(what, "the block grid is not the voxel grid's, n / 4 per axis");
    if (check_aligned(what, 0, ADDR(d_b) | ADDR(d_w)))
        return SIFT3D_FAILURE;
    if (ranges_overlap((range_t){ d_w, field_bytes(nx, ny, nz) },
                       (range_t){ d_b, 3 * grid_voxels(nbx, nby, nbz) * sizeof(float) }))
        return refuse(what, "the output overlaps the input");
    return sift3d_block_field_expand_launch(d_b, nbx, nby, nbz, d_w, nx, ny, nz, stream);
}

/* ---- the driver ---- */

void sift3d_amd_discrete_register_default_params(sift3d_amd_discrete_register_params *p)
{
    static const double theta[6] = SIFT3D_AMD_DISCRETE_DEFAULT_THETAS;
    int i;
    if (!p)
        return;
    memset(p, 0, sizeof(*p));
    p->radius = 4;
    p->passes = 2;
    p->n_theta = 6;
    for (i = 0; i < 6; i++)
        p->theta[i] = theta[i];
}

size_t sift3d_amd_discrete_register_struct_bytes(int which)
{
    return which == 0   ? sizeof(sift3d_amd_discrete_register_params)
           : which == 1 ? (size_t)SIFT3D_AMD_DISCRETE_MAX_RADIUS
           : which == 2 ? (size_t)SIFT3D_AMD_DISCRETE_MAX_CHANNELS
           : which == 3 ? (size_t)SIFT3D_AMD_DISCRETE_MAX_THETAS
           : which == 4 ? (size_t)SIFT3D_AMD_DISCRETE_MAX_PASSES
           : which == 5 ? (size_t)SIFT3D_AMD_COST_SELECT_WORK_BYTES
                        : 0;
}

/* The finest level's scratch, as offsets in floats into d_work; every coarser level uses the same buffers (none needs
 * more: a halved grid has no more voxels or blocks).  The header states the total. */
typedef struct {
    size_t part, W, VW, ones, C, v, b, data, tmp, w, unew, levels;
} discrete_layout;

static discrete_layout discrete_layout_of(int nx, int ny, int nz, int mx, int my, int mz, int nc, int radius,
                                          int mask_moving)
{
    const size_t n = grid_voxels(nx, ny, nz), m = grid_voxels(mx, my, mz), nb = grid_voxels(nx / 4, ny / 4, nz / 4);
    discrete_layout l;
    l.part = 0;
    l.W = pad4(SIFT3D_AMD_COST_SELECT_WORK_BYTES / sizeof(float));
    l.VW = l.W + pad4((size_t)nc * n);
    l.ones = l.VW + pad4(n);
    l.C = l.ones + (mask_moving ? 0 : pad4(m));
    l.v = l.C + pad4(nb * discrete_labels(radius));
    l.b = l.v + pad4(3 * nb);
    l.data = l.b + pad4(3 * nb);
    l.tmp = l.data + pad4(nb);
    l.w = l.tmp + pad4(3 * nb);
    l.unew = l.w + pad4(3 * n);
    l.levels = l.unew + pad4(3 * n);
    return l;
}

size_t sift3d_amd_discrete_register_work_floats(int nx, int ny, int nz, int mx, int my, int mz, int nc, int levels,
                                                int radius, int mask_fixed, int mask_moving)
{
    size_t at;
    int l;
    if (nx <= 0 || ny <= 0 || nz <= 0 || mx <= 0 || my <= 0 || mz <= 0 || nc < 1 ||
        nc > SIFT3D_AMD_DISCRETE_MAX_CHANNELS || levels < 1 || levels > SIFT3D_AMD_DEMONS_MAX_LEVELS ||
        !discrete_radius_ok(radius))
        return 0;
    at = discrete_layout_of(nx, ny, nz, mx, my, mz, nc, radius, mask_moving).levels;
    for (l = 0; l < levels; l++) {
        if (nx < 4 || ny < 4 || nz < 4)
            return 0;
        if (l > 0)
            at += pad4(3 * grid_voxels(nx, ny, nz)) + (mask_fixed ? pad4(grid_voxels(nx, ny, nz)) : 0) +
                  (mask_moving ? pad4(grid_voxels(mx, my, mz)) : 0);
        nx = multires_half(nx); ny = multires_half(ny); nz = multires_half(nz);
        mx = multires_half(mx); my = multires_half(my); mz = multires_half(mz);
    }
    return at;
}

int sift3d_amd_discrete_register_device(const sift3d_amd_demons_level *level, int levels, int nc, const float *d_VF,
                                        const float *d_VM, float *d_u,
                                        const sift3d_amd_discrete_register_params *params, void *d_stats,
                                        float *d_work, void *stream)
{
    static const char what[] = "sift3d_amd_discrete_register_device";
    sift3d_amd_discrete_register_params prm;
    range_t in[2 * SIFT3D_AMD_DEMONS_MAX_LEVELS + 2];
    float *u[SIFT3D_AMD_DEMONS_MAX_LEVELS];
    const float *VF[SIFT3D_AMD_DEMONS_MAX_LEVELS], *VM[SIFT3D_AMD_DEMONS_MAX_LEVELS];
    discrete_layout at;
    uintptr_t or4 = ADDR(d_u) | ADDR(d_VF) | ADDR(d_VM);
    size_t need, off, rec = 0;
    int l, j;
    if (!level || !d_u || !d_stats || !d_work)
        return refuse(what, "NULL argument");
    if (params)
        prm = *params;
    else
        sift3d_amd_discrete_register_default_params(&prm);
    if (levels < 1 || levels > SIFT3D_AMD_DEMONS_MAX_LEVELS)
        return refuse(what, "levels must be in [1, SIFT3D_AMD_DEMONS_MAX_LEVELS]");
    if (check_discrete_channels(what, nc) || check_discrete_radius(what, prm.radius) ||
        check_discrete_passes(what, prm.passes))
        return SIFT3D_FAILURE;
    if (prm.n_theta < 1 || prm.n_theta > SIFT3D_AMD_DISCRETE_MAX_THETAS)
        return refuse(what, "n_theta must be in [1, SIFT3D_AMD_DISCRETE_MAX_THETAS]");
    for (j = 0; j < prm.n_theta; j++)
        if (check_discrete_theta(what, prm.theta[j]))
            return SIFT3D_FAILURE;
    for (l = 0; l < levels; l++) {
        const sift3d_amd_demons_level *v = level + l;
        if (!v->d_F || !v->d_M)
            return refuse(what, "NULL argument");
        if (check_dims(what, v->nx, v->ny, v->nz) || check_dims(what, v->mx, v->my, v->mz))
            return SIFT3D_FAILURE;
        if (v->nx < 4 || v->ny < 4 || v->nz < 4)
            return refuse(what, "every level's fixed grid must hold a block of 4 voxels on every axis");
        if (l > 0 && (v->nx != multires_half(v[-1].nx) || v->ny != multires_half(v[-1].ny) ||
                      v->nz != multires_half(v[-1].nz) || v->mx != multires_half(v[-1].mx) ||
                      v->my != multires_half(v[-1].my) || v->mz != multires_half(v[-1].mz)))
            return refuse(what, "a level's dimensions are not the halves of the level above");
        or4 |= ADDR(v->d_F) | ADDR(v->d_M);
        in[2 * l] = (range_t){ v->d_F, image_bytes(v->nx, v->ny, v->nz, nc) };
        in[2 * l + 1] = (range_t){ v->d_M, image_bytes(v->mx, v->my, v->mz, nc) };
    }
    in[2 * levels] = (range_t){ d_VF, d_VF ? image_bytes(level->nx, level->ny, level->nz, 1) : 0 };
    in[2 * levels + 1] = (range_t){ d_VM, d_VM ? image_bytes(level->mx, level->my, level->mz, 1) : 0 };
    need = sift3d_amd_discrete_register_work_floats(level->nx, level->ny, level->nz, level->mx, level->my, level->mz,
                                                    nc, levels, prm.radius, d_VF != NULL, d_VM != NULL);
    if (!need)
        return refuse(what, "every level's fixed grid must hold a block of 4 voxels on every axis");
    if (check_aligned(what, ADDR(d_stats) | ADDR(d_work), or4))
        return SIFT3D_FAILURE;
    {
        const range_t out[] = { { d_u, field_bytes(level->nx, level->ny, level->nz) },
                                { d_work, need * sizeof(float) },
                                { d_stats, (size_t)SIFT3D_AMD_DEMONS_STATS_BYTES * levels * prm.n_theta } };
        if (ranges_aliased(out, 3, in, 2 * levels + 2))
            return refuse(what, ALIASED);
    }

    at = discrete_layout_of(level->nx, level->ny, level->nz, level->mx, level->my, level->mz, nc, prm.radius,
                            d_VM != NULL);
    if (!d_VM && sift3d_block_fill_launch(d_work + at.ones, grid_voxels(level->mx, level->my, level->mz), 1.0f, stream))
        return SIFT3D_FAILURE;
    /* the level fields and masks: level 0's are the caller's, the others follow the scratch */
    u[0] = d_u;
    VF[0] = d_VF;
    VM[0] = d_VM;
    off = at.levels;
    for (l = 1; l < levels; l++) {
        const sift3d_amd_demons_level *f = level + l - 1, *c = level + l;
        u[l] = d_work + off;
        off += pad4(3 * grid_voxels(c->nx, c->ny, c->nz));
        if (sift3d_restrict2_launch(u[l - 1], f->nx, f->ny, f->nz, 3, u[l], 0.5f, stream))
            return SIFT3D_FAILURE;
        VF[l] = VM[l] = NULL;
        if (d_VF) {
            float *m = d_work + off;
            off += pad4(grid_voxels(c->nx, c->ny, c->nz));
            if (sift3d_restrict2_launch(VF[l - 1], f->nx, f->ny, f->nz, 1, m, 1.0f, stream))
                return SIFT3D_FAILURE;
            VF[l] = m;
        }
        if (d_VM) {
            float *m = d_work + off;
            off += pad4(grid_voxels(c->mx, c->my, c->mz));
            if (sift3d_restrict2_launch(VM[l - 1], f->mx, f->my, f->mz, 1, m, 1.0f, stream))
                return SIFT3D_FAILURE;
            VM[l] = m;
        }
    }
    for (l = levels - 1; l >= 0; l--) {
        const sift3d_amd_demons_level *v = level + l;
        const int nbx = v->nx / 4, nby = v->ny / 4, nbz = v->nz / 4;
        const size_t n = grid_voxels(v->nx, v->ny, v->nz), nb = grid_voxels(nbx, nby, nbz);
        float *d_W = d_work + at.W, *d_VW = d_work + at.VW, *d_C = d_work + at.C, *d_v = d_work + at.v,
              *d_b = d_work + at.b, *d_data = d_work + at.data, *d_tmp = d_work + at.tmp, *d_w = d_work + at.w,
              *d_unew = d_work + at.unew;
        if (sift3d_hip_warp_field(v->d_M, v->mx, v->my, v->mz, nc, u[l], v->nx, v->ny, v->nz, d_W,
                                  SIFT3D_AMD_INTERP_LINEAR, 0.0f, stream) ||
            sift3d_hip_warp_field(VM[l] ? VM[l] : d_work + at.ones, v->mx, v->my, v->mz, 1, u[l], v->nx, v->ny, v->nz,
                                  d_VW, SIFT3D_AMD_INTERP_NEAREST, 0.0f, stream) ||
            sift3d_cost_volume_launch(v->d_F, d_W, nc, v->nx, v->ny, v->nz, VF[l], d_VW, prm.radius, d_C, stream) ||
            sift3d_hip_memset(d_b, 0, 3 * nb * sizeof(float), stream))
            return SIFT3D_FAILURE;
        for (j = 0; j < prm.n_theta; j++, rec++)
            if (sift3d_cost_select_launch(d_C, nbx, nby, nbz, prm.radius, d_b, prm.theta[j], d_v, d_data,
                                          (char *)d_stats + (size_t)SIFT3D_AMD_DEMONS_STATS_BYTES * rec,
                                          d_work + at.part, stream) ||
                block_field_smooth_run(d_v, d_b, nbx, nby, nbz, prm.passes, d_tmp, stream))
                return SIFT3D_FAILURE;
        if (sift3d_block_field_expand_launch(d_b, nbx, nby, nbz, d_w, v->nx, v->ny, v->nz, stream) ||
            sift3d_field_compose_launch(u[l], v->nx, v->ny, v->nz, d_w, v->nx, v->ny, v->nz, d_unew,
                                        SIFT3D_AMD_FIELD_COMPOSE, NULL, NULL, stream) ||
            sift3d_hip_memcpy_d2d(u[l], d_unew, 3 * n * sizeof(float), stream))
            return SIFT3D_FAILURE;
        if (l > 0 &&
            sift3d_field_prolong2_launch(u[l], u[l - 1], level[l - 1].nx, level[l - 1].ny, level[l - 1].nz, stream))
            return SIFT3D_FAILURE;
    }
    return SIFT3D_SUCCESS;
}
