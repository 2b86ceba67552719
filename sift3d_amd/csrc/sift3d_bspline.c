/* sift3d_bspline.c -- cubic B-spline resampling: the checked device entries and the blocking host forms (included
 * at the end of sift3d_host.c, after sift3d_checks.c).
 *
 * The contract is in include/sift3d_amd.h, "Cubic B-spline resampling"; the kernels are in sift3d_bspline.hip,
 * reached through the launchers below after the checks here.  Arguments are checked before the device is touched,
 * so bad input is refused on a machine without a GPU too. */

int sift3d_bspline_prefilter_launch(const float *d_src, int nx, int ny, int nz, int nc, float *d_coef, float *d_work,
                                    void *stream);
int sift3d_bspline_warp_affine_launch(const float *d_coef, int nx, int ny, int nz, float *d_dst, int ox, int oy, int oz,
                                      const double *A, float fill, void *stream);
int sift3d_bspline_warp_field_launch(const float *d_coef, int nx, int ny, int nz, int nc, const float *d_field, int ox,
                                     int oy, int oz, float *d_dst, float fill, void *stream);

size_t sift3d_hip_bspline_work_floats(int nx, int ny, int nz)
{
    if (nx <= 0 || ny <= 0 || nz <= 0)
        return 0;
    return grid_voxels(nx, ny, nz);
}

int sift3d_hip_bspline_prefilter(const float *d_src, int nx, int ny, int nz, int nc, float *d_coef, float *d_work,
                                 void *stream)
{
    static const char what[] = "sift3d_hip_bspline_prefilter";
    if (!d_src || !d_coef || !d_work)
        return refuse(what, "NULL argument");
    if (check_dims(what, nx, ny, nz) || check_channels(what, nc) ||
        check_aligned(what, 0, ADDR(d_src) | ADDR(d_coef) | ADDR(d_work)))
        return SIFT3D_FAILURE;
    {
        const range_t in[] = { { d_src, image_bytes(nx, ny, nz, nc) } };
        const range_t out[] = { { d_coef, image_bytes(nx, ny, nz, nc) }, { d_work, image_bytes(nx, ny, nz, 1) } };
        if (ranges_aliased(out, 2, in, 1))
            return refuse(what, ALIASED);
    }
    return sift3d_bspline_prefilter_launch(d_src, nx, ny, nz, nc, d_coef, d_work, stream);
}

int sift3d_hip_bspline_warp_affine(const float *d_coef, int nx, int ny, int nz, float *d_dst, int ox, int oy, int oz,
                                   const double *A, float fill, void *stream)
{
    static const char what[] = "sift3d_hip_bspline_warp_affine";
    if (!d_coef || !d_dst || !A)
        return refuse(what, "NULL argument");
    if (check_dims(what, nx, ny, nz) || check_dims(what, ox, oy, oz) || check_affine(what, A) ||
        check_aligned(what, 0, ADDR(d_coef) | ADDR(d_dst)))
        return SIFT3D_FAILURE;
    {
        const range_t in[] = { { d_coef, image_bytes(nx, ny, nz, 1) } };
        const range_t out[] = { { d_dst, image_bytes(ox, oy, oz, 1) } };
        if (ranges_aliased(out, 1, in, 1))
            return refuse(what, ALIASED);
    }
    return sift3d_bspline_warp_affine_launch(d_coef, nx, ny, nz, d_dst, ox, oy, oz, A, fill, stream);
}

int sift3d_hip_bspline_warp_field(const float *d_coef, int nx, int ny, int nz, int nc, const float *d_field, int ox,
                                  int oy, int oz, float *d_dst, float fill, void *stream)
{
    static const char what[] = "sift3d_hip_bspline_warp_field";
    if (!d_coef || !d_field || !d_dst)
        return refuse(what, "NULL argument");
    if (check_dims(what, nx, ny, nz) || check_dims(what, ox, oy, oz) || check_channels(what, nc) ||
        check_aligned(what, 0, ADDR(d_coef) | ADDR(d_field) | ADDR(d_dst)))
        return SIFT3D_FAILURE;
    {
        const range_t in[] = { { d_coef, image_bytes(nx, ny, nz, nc) }, { d_field, field_bytes(ox, oy, oz) } };
        const range_t out[] = { { d_dst, image_bytes(ox, oy, oz, nc) } };
        if (ranges_aliased(out, 1, in, 2))
            return refuse(what, ALIASED);
    }
    return sift3d_bspline_warp_field_launch(d_coef, nx, ny, nz, nc, d_field, ox, oy, oz, d_dst, fill, stream);
}

/* ---- blocking host forms ---- */

int sift3d_amd_bspline_prefilter(const float *src, int nx, int ny, int nz, int nc, float *coef)
{
    static const char what[] = "sift3d_amd_bspline_prefilter";
    float *d_src = NULL, *d_coef = NULL, *d_work = NULL;
    size_t nb;
    int rc = SIFT3D_FAILURE;
    if (!src || !coef)
        return refuse(what, "NULL argument");
    if (check_dims(what, nx, ny, nz) || check_channels(what, nc))
        return SIFT3D_FAILURE;
    nb = image_bytes(nx, ny, nz, nc);
    if (ranges_overlap((range_t){ coef, nb }, (range_t){ src, nb }))
        return refuse(what, ALIASED);
    if (!sift3d_amd_device_available()) {
        ERR("sift3d_amd: no HIP device is available; this library has no CPU path \n");
        return SIFT3D_FAILURE;
    }
    d_src = (float *)sift3d_hip_malloc(nb);
    d_coef = (float *)sift3d_hip_malloc(nb);
    d_work = (float *)sift3d_hip_malloc(image_bytes(nx, ny, nz, 1));
    if (d_src && d_coef && d_work && !sift3d_hip_memcpy_h2d(d_src, src, nb, NULL) &&
        !sift3d_hip_bspline_prefilter(d_src, nx, ny, nz, nc, d_coef, d_work, NULL) &&
        !sift3d_hip_memcpy_d2h(coef, d_coef, nb, NULL) && !sift3d_hip_stream_sync(NULL))
        rc = SIFT3D_SUCCESS;
    sift3d_hip_free(d_src);
    sift3d_hip_free(d_coef);
    sift3d_hip_free(d_work);
    return rc;
}

/* the shared body of the two image forms: field == NULL is the affine one */
static int image_bspline_warp(const char *what, const sift3d_image *src, const double *A, const float *field,
                              float fill, sift3d_image *dst)
{
    float *d_src = NULL, *d_coef = NULL, *d_work = NULL, *d_dst = NULL, *d_field = NULL;
    size_t ns, nd;
    int rc = SIFT3D_FAILURE;
    if (!src || !dst || (!A && !field) || !src->data || !dst->data)
        return refuse(what, "NULL argument");
    if (src->nc != 1 || dst->nc != 1)
        return refuse(what, "only single-channel images are supported");
    if (check_dims(what, src->nx, src->ny, src->nz) || check_dims(what, dst->nx, dst->ny, dst->nz) ||
        (A && check_affine(what, A)))
        return SIFT3D_FAILURE;
    ns = image_bytes(src->nx, src->ny, src->nz, 1);
    nd = image_bytes(dst->nx, dst->ny, dst->nz, 1);
    if (ranges_overlap((range_t){ dst->data, nd }, (range_t){ src->data, ns }) ||
        (field && ranges_overlap((range_t){ dst->data, nd }, (range_t){ field, 3 * nd })))
        return refuse(what, "the destination overlaps the source or the field");
    if (!sift3d_amd_device_available()) {
        ERR("sift3d_amd: no HIP device is available; this library has no CPU path \n");
        return SIFT3D_FAILURE;
    }
    d_src = (float *)sift3d_hip_malloc(ns);
    d_coef = (float *)sift3d_hip_malloc(ns);
    d_work = (float *)sift3d_hip_malloc(ns);
    d_dst = (float *)sift3d_hip_malloc(nd);
    d_field = field ? (float *)sift3d_hip_malloc(3 * nd) : NULL;
    if (d_src && d_coef && d_work && d_dst && (d_field || !field) &&
        !sift3d_hip_memcpy_h2d(d_src, src->data, ns, NULL) &&
        !sift3d_hip_bspline_prefilter(d_src, src->nx, src->ny, src->nz, 1, d_coef, d_work, NULL) &&
        (field ? !sift3d_hip_memcpy_h2d(d_field, field, 3 * nd, NULL) &&
                     !sift3d_hip_bspline_warp_field(d_coef, src->nx, src->ny, src->nz, 1, d_field, dst->nx, dst->ny,
                                                    dst->nz, d_dst, fill, NULL)
               : !sift3d_hip_bspline_warp_affine(d_coef, src->nx, src->ny, src->nz, d_dst, dst->nx, dst->ny, dst->nz,
                                                 A, fill, NULL)) &&
        !sift3d_hip_memcpy_d2h(dst->data, d_dst, nd, NULL) && !sift3d_hip_stream_sync(NULL))
        rc = SIFT3D_SUCCESS;
    sift3d_hip_free(d_src);
    sift3d_hip_free(d_coef);
    sift3d_hip_free(d_work);
    sift3d_hip_free(d_dst);
    sift3d_hip_free(d_field);
    return rc;
}

int sift3d_amd_image_bspline_warp_affine(const sift3d_image *src, const double *A, float fill, sift3d_image *dst)
{
    static const char what[] = "sift3d_amd_image_bspline_warp_affine";
    if (!A)
        return refuse(what, "NULL argument");
    return image_bspline_warp(what, src, A, NULL, fill, dst);
}

int sift3d_amd_image_bspline_warp_field(const sift3d_image *src, const float *field, float fill, sift3d_image *dst)
{
    static const char what[] = "sift3d_amd_image_bspline_warp_field";
    if (!field)
        return refuse(what, "NULL argument");
    return image_bspline_warp(what, src, NULL, field, fill, dst);
}
