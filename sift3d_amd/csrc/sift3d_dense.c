/* sift3d_dense.c -- dense descriptor images, plain and rotation-invariant (included at the end of
 * sift3d_host.c).
 *
 * The contract is in include/sift3d_amd.h.  The device stages are sift3d_hip_dense_bin and
 * sift3d_hip_dense_normalize (sift3d_describe.hip, beside the face tables they share with the sparse
 * descriptor); the window between them is the detector's own blur (blur_level), run once per channel
 * in place.  Arguments are checked before the device is touched, so bad input is refused on a machine
 * without a GPU too. */

size_t sift3d_amd_dense_work_floats(int nx, int ny, int nz)
{
    if (nx <= 0 || ny <= 0 || nz <= 0)
        return 0;
    /* the x-pass result, and the y-pass result when the fused y+z kernel does not apply */
    return 2 * (size_t)nx * ny * nz;
}

static int dense_check(const char *what, int nx, int ny, int nz, const double *units3, double sigma)
{
    int k;
    if (check_dims(what, nx, ny, nz))
        return SIFT3D_FAILURE;
    if (!isfinite(sigma) || !(sigma > 0))
        return refuse(what, "sigma must be positive and finite");
    for (k = 0; k < 3; k++)
        if (!isfinite(units3[k]) || !(units3[k] > 0))
            return refuse(what, "units must be positive and finite");
    return SIFT3D_SUCCESS;
}

int sift3d_amd_dense_descriptors_device(const float *d_src, int nx, int ny, int nz, const double *units3,
                                        double sigma, float *d_out, float *d_work, void *stream)
{
    static const char what[] = "sift3d_amd_dense_descriptors_device";
    const int dims[3] = { nx, ny, nz };
    const size_t n = grid_voxels(nx, ny, nz);
    const range_t out = { d_out, 12 * n * sizeof(float) };
    filter_t f;
    int c, rc = SIFT3D_FAILURE;
    if (!d_src || !d_out || !d_work || !units3)
        return refuse(what, "NULL argument");
    if (dense_check(what, nx, ny, nz, units3, sigma))
        return SIFT3D_FAILURE;
    if (ranges_overlap(out, (range_t){ d_src, n * sizeof(float) }) ||
        ranges_overlap(out, (range_t){ d_work, 2 * n * sizeof(float) }))
        return refuse(what, "the output overlaps the source or the work buffer");
    if (sift3d_amd_init())        /* (the face tables; refuses without a device) */
        return SIFT3D_FAILURE;
    if (gauss_filter(&f, sigma))
        return SIFT3D_FAILURE;
    if (sift3d_hip_dense_bin(d_src, nx, ny, nz, units3[0], units3[1], units3[2], d_out, stream))
        goto done;
    for (c = 0; c < 12; c++) {
        float *ch = d_out + (size_t)c * n;
        if (blur_level(NULL, ch, ch, dims, units3, &f, stream, d_work, d_work + n, -1, NULL))
            goto done;
    }
    if (sift3d_hip_dense_normalize(d_out, n, stream))
        goto done;
    rc = SIFT3D_SUCCESS;
done:
    free(f.taps);
    return rc;
}

int sift3d_amd_image_dense_descriptors(const sift3d_image *im, double sigma, float *out)
{
    static const char what[] = "sift3d_amd_image_dense_descriptors";
    float *d_src = NULL, *d_out = NULL, *d_work = NULL;
    double units[3];
    size_t n;
    int rc = SIFT3D_FAILURE;
    if (!im || !out || !im->data)
        return refuse(what, "NULL argument");
    if (im->nc != 1)
        return refuse(what, "only single-channel images are supported");
    units[0] = im->ux; units[1] = im->uy; units[2] = im->uz;
    if (dense_check(what, im->nx, im->ny, im->nz, units, sigma))
        return SIFT3D_FAILURE;
    if (!sift3d_amd_device_available()) {
        ERR("sift3d_amd: no HIP device is available; this library has no CPU path \n");
        return SIFT3D_FAILURE;
    }
    n = (size_t)im->nx * im->ny * im->nz;
    d_src = (float *)sift3d_hip_malloc(n * sizeof(float));
    d_out = (float *)sift3d_hip_malloc(12 * n * sizeof(float));
    d_work = (float *)sift3d_hip_malloc(sift3d_amd_dense_work_floats(im->nx, im->ny, im->nz) * sizeof(float));
    if (d_src && d_out && d_work && !sift3d_hip_memcpy_h2d(d_src, im->data, n * sizeof(float), NULL) &&
        !sift3d_amd_dense_descriptors_device(d_src, im->nx, im->ny, im->nz, units, sigma, d_out, d_work, NULL) &&
        !sift3d_hip_memcpy_d2h(out, d_out, 12 * n * sizeof(float), NULL) && !sift3d_hip_stream_sync(NULL))
        rc = SIFT3D_SUCCESS;
    sift3d_hip_free(d_src);
    sift3d_hip_free(d_out);
    sift3d_hip_free(d_work);
    return rc;
}

/* ---- rotation-invariant variant: R2 (sift3d_hip_dense_orient) into d_work, R3, R4 ---- */

size_t sift3d_amd_dense_rotate_work_floats(int nx, int ny, int nz)
{
    if (nx <= 0 || ny <= 0 || nz <= 0)
        return 0;
    return 9 * (size_t)nx * ny * nz;        /* R, 9 planes */
}

int sift3d_amd_dense_descriptors_rotate_device(const float *d_src, int nx, int ny, int nz, const double *units3,
                                               double sigma, float *d_out, float *d_work, void *stream)
{
    static const char what[] = "sift3d_amd_dense_descriptors_rotate_device";
    const size_t n = grid_voxels(nx, ny, nz);
    const range_t in = { d_src, n * sizeof(float) };
    const range_t out[] = { { d_out, 12 * n * sizeof(float) }, { d_work, 9 * n * sizeof(float) } };
    if (!d_src || !d_out || !d_work || !units3)
        return refuse(what, "NULL argument");
    if (dense_check(what, nx, ny, nz, units3, sigma))
        return SIFT3D_FAILURE;
    if (ranges_aliased(out, 2, &in, 1))
        return refuse(what, "the output or the work buffer overlaps another buffer");
    if (sift3d_amd_init())        /* (the face tables; refuses without a device) */
        return SIFT3D_FAILURE;
    if (sift3d_hip_dense_orient(d_src, nx, ny, nz, units3[0], units3[1], units3[2], sigma, d_work, NULL, stream) ||
        sift3d_hip_dense_rotate_bin(d_src, nx, ny, nz, units3[0], units3[1], units3[2], sigma, d_work, d_out,
                                    stream) ||
        sift3d_hip_dense_normalize(d_out, n, stream))
        return SIFT3D_FAILURE;
    return SIFT3D_SUCCESS;
}

int sift3d_amd_image_dense_descriptors_rotate(const sift3d_image *im, double sigma, float *out)
{
    static const char what[] = "sift3d_amd_image_dense_descriptors_rotate";
    float *d_src = NULL, *d_out = NULL, *d_work = NULL;
    double units[3];
    size_t n;
    int rc = SIFT3D_FAILURE;
    if (!im || !out || !im->data)
        return refuse(what, "NULL argument");
    if (im->nc != 1)
        return refuse(what, "only single-channel images are supported");
    units[0] = im->ux; units[1] = im->uy; units[2] = im->uz;
    if (dense_check(what, im->nx, im->ny, im->nz, units, sigma))
        return SIFT3D_FAILURE;
    if (!sift3d_amd_device_available()) {
        ERR("sift3d_amd: no HIP device is available; this library has no CPU path \n");
        return SIFT3D_FAILURE;
    }
    n = (size_t)im->nx * im->ny * im->nz;
    d_src = (float *)sift3d_hip_malloc(n * sizeof(float));
    d_out = (float *)sift3d_hip_malloc(12 * n * sizeof(float));
    d_work = (float *)sift3d_hip_malloc(sift3d_amd_dense_rotate_work_floats(im->nx, im->ny, im->nz) * sizeof(float));
    if (d_src && d_out && d_work && !sift3d_hip_memcpy_h2d(d_src, im->data, n * sizeof(float), NULL) &&
        !sift3d_amd_dense_descriptors_rotate_device(d_src, im->nx, im->ny, im->nz, units, sigma, d_out, d_work,
                                                    NULL) &&
        !sift3d_hip_memcpy_d2h(out, d_out, 12 * n * sizeof(float), NULL) && !sift3d_hip_stream_sync(NULL))
        rc = SIFT3D_SUCCESS;
    sift3d_hip_free(d_src);
    sift3d_hip_free(d_out);
    sift3d_hip_free(d_work);
    return rc;
}
