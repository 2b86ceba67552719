/* sift3d_checks.c -- the argument checks shared by the entries of sift3d_warp.c, sift3d_dense.c, sift3d_field_ops.c,
 * sift3d_demons.c and sift3d_bspline.c (included at the end of sift3d_host.c, ahead of them).
 *
 * An entry states what it checks with these and refuses with `return refuse(what, why)`: -1 and one line on stderr
 * that names the entry the caller called.  All of it is host arithmetic, so bad input is refused before the device
 * is touched, on a machine without a GPU too. */

typedef struct {
    const void *p;
    size_t bytes;
} range_t;

static const char ALIASED[] = "an output overlaps an input, the work buffer or another output";

static int refuse(const char *what, const char *why)
{
    ERR("%s: %s \n", what, why);
    return SIFT3D_FAILURE;
}

static int ranges_overlap(range_t a, range_t b)
{
    const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
    return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

/* every output against every input and every other output */
static int ranges_aliased(const range_t *out, int nout, const range_t *in, int nin)
{
    int i, j;
    for (i = 0; i < nout; i++) {
        for (j = 0; j < nin; j++)
            if (ranges_overlap(out[i], in[j]))
                return 1;
        for (j = i + 1; j < nout; j++)
            if (ranges_overlap(out[i], out[j]))
                return 1;
    }
    return 0;
}

static size_t grid_voxels(int nx, int ny, int nz)
{
    return (size_t)nx * ny * nz;
}

/* bytes of a float image [nc][nz][ny][nx]; a displacement field has nc = 3 */
static size_t image_bytes(int nx, int ny, int nz, int nc)
{
    return (size_t)nc * grid_voxels(nx, ny, nz) * sizeof(float);
}

static size_t field_bytes(int ox, int oy, int oz)
{
    return image_bytes(ox, oy, oz, 3);
}

static int check_dims(const char *what, int nx, int ny, int nz)
{
    return nx <= 0 || ny <= 0 || nz <= 0 ? refuse(what, "dimensions must be positive") : SIFT3D_SUCCESS;
}

static int check_channels(const char *what, int nc)
{
    return nc < 1 ? refuse(what, "the number of channels must be positive") : SIFT3D_SUCCESS;
}

static int check_affine(const char *what, const double *A)
{
    int i;
    for (i = 0; i < 12; i++)
        if (!isfinite(A[i]))
            return refuse(what, "the affine map is not finite");
    return SIFT3D_SUCCESS;
}

static int check_iterations(const char *what, int iterations)
{
    return iterations < 0 ? refuse(what, "the number of iterations must not be negative") : SIFT3D_SUCCESS;
}

static int check_squarings(const char *what, int squarings)
{
    return squarings < 0 || squarings > SIFT3D_AMD_FIELD_MAX_SQUARINGS
               ? refuse(what, "squarings must be in [0, SIFT3D_AMD_FIELD_MAX_SQUARINGS]") : SIFT3D_SUCCESS;
}

static int check_sigmas(const char *what, double sigma_fluid, double sigma_diffusion)
{
    return !isfinite(sigma_fluid) || sigma_fluid < 0 || !isfinite(sigma_diffusion) || sigma_diffusion < 0
               ? refuse(what, "the sigmas must be finite and not negative") : SIFT3D_SUCCESS;
}

/* or8 / or4: the addresses that must be 8- / 4-byte aligned, or-ed together (a NULL passes) */
#define ADDR(p) ((uintptr_t)(p))
static int check_aligned(const char *what, uintptr_t or8, uintptr_t or4)
{
    return (or8 & 7) || (or4 & 3) ? refuse(what, "a buffer is misaligned") : SIFT3D_SUCCESS;
}
