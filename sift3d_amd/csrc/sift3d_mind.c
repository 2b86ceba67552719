/* sift3d_mind.c -- MIND-SSC self-similarity descriptors: the checked entry (included at the end of sift3d_host.c,
 * after sift3d_checks.c, whose helpers it uses).
 *
 * The contract is in include/sift3d_amd.h, "MIND self-similarity descriptors".  The kernels are sift3d_mind.hip's,
 * reached through the launcher below after the checks here.  Arguments are checked before the device is touched, so
 * bad input is refused on a machine without a GPU too. */

int sift3d_mind_launch(const float *d_src, int nx, int ny, int nz, int radius, int dilation, double vlo, double vhi,
                       float *d_out, double *d_D, double *d_V, void *d_stats, void *d_work, void *stream);

/* the per-workgroup partials: 2048 slots of a double and a uint64 */
#define MIND_WORK_BYTES 32768

size_t sift3d_amd_mind_work_bytes(int nx, int ny, int nz)
{
    return nx <= 0 || ny <= 0 || nz <= 0 ? 0 : MIND_WORK_BYTES;
}

int sift3d_hip_mind_ssc(const float *d_src, int nx, int ny, int nz, int radius, int dilation, double vlo, double vhi,
                        float *d_out, double *d_D, double *d_V, void *d_stats, void *d_work, void *stream)
{
    static const char what[] = "sift3d_hip_mind_ssc";
    range_t out[5], in;
    int nout = 0;
    size_t n;
    if (!d_src || !d_work)
        return refuse(what, "NULL argument");
    if (!d_out && !d_D && !d_V && !d_stats)
        return refuse(what, "no output asked for");
    if (check_dims(what, nx, ny, nz))
        return SIFT3D_FAILURE;
    if (radius < 1 || radius > SIFT3D_AMD_MIND_MAX_RADIUS)
        return refuse(what, "radius must be in [1, SIFT3D_AMD_MIND_MAX_RADIUS]");
    if (dilation < 1 || dilation > SIFT3D_AMD_MIND_MAX_DILATION)
        return refuse(what, "dilation must be in [1, SIFT3D_AMD_MIND_MAX_DILATION]");
    /* (written so that a NaN fails either test) */
    if (!(vlo >= 0) || !(vhi >= vlo))
        return refuse(what, "the clamps must satisfy 0 <= vlo <= vhi");
    if (check_aligned(what, ADDR(d_D) | ADDR(d_V) | ADDR(d_stats) | ADDR(d_work), ADDR(d_src) | ADDR(d_out)))
        return SIFT3D_FAILURE;
    n = grid_voxels(nx, ny, nz);
    in = (range_t){ d_src, n * sizeof(float) };
    out[nout++] = (range_t){ d_work, MIND_WORK_BYTES };
    if (d_out)
        out[nout++] = (range_t){ d_out, SIFT3D_AMD_MIND_CHANNELS * n * sizeof(float) };
    if (d_D)
        out[nout++] = (range_t){ d_D, SIFT3D_AMD_MIND_CHANNELS * n * sizeof(double) };
    if (d_V)
        out[nout++] = (range_t){ d_V, n * sizeof(double) };
    if (d_stats)
        out[nout++] = (range_t){ d_stats, SIFT3D_AMD_DEMONS_STATS_BYTES };
    if (ranges_aliased(out, nout, &in, 1))
        return refuse(what, ALIASED);
    return sift3d_mind_launch(d_src, nx, ny, nz, radius, dilation, vlo, vhi, d_out, d_D, d_V, d_stats, d_work, stream);
}
