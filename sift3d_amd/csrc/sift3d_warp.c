/* sift3d_warp.c -- affine resampling of host images and inversion of affine maps (included at the
 * end of sift3d_host.c).
 *
 * The device kernel is sift3d_hip_warp_affine (sift3d_warp.hip); this file holds the blocking form on
 * host image objects, which uploads the source, resamples into the destination's grid and downloads
 * the result.  Arguments are checked before the device is touched, so bad input is refused on a
 * machine without a GPU too. */

int sift3d_amd_affine_invert(const double *A, double *Ainv)
{
    double m[9], c[9], det, scale = 1.0, t[3];
    int i, r;
    if (!A || !Ainv)
        return SIFT3D_FAILURE;
    for (i = 0; i < 12; i++)
        if (!isfinite(A[i]))
            return SIFT3D_FAILURE;
    for (r = 0; r < 3; r++)
        for (i = 0; i < 3; i++)
            m[3 * r + i] = A[4 * r + i];
    /* cofactors: c[3*j + i] = cofactor of m[i][j] (the adjugate, row-major) */
    c[0] = m[4] * m[8] - m[5] * m[7];
    c[1] = m[2] * m[7] - m[1] * m[8];
    c[2] = m[1] * m[5] - m[2] * m[4];
    c[3] = m[5] * m[6] - m[3] * m[8];
    c[4] = m[0] * m[8] - m[2] * m[6];
    c[5] = m[2] * m[3] - m[0] * m[5];
    c[6] = m[3] * m[7] - m[4] * m[6];
    c[7] = m[1] * m[6] - m[0] * m[7];
    c[8] = m[0] * m[4] - m[1] * m[3];
    det = m[0] * c[0] + m[1] * c[3] + m[2] * c[6];
    /* singular relative to the size of the rows: |det| <= prod |row| (Hadamard), so the ratio is a
     * scale-free measure of how far the rows are from being linearly dependent */
    for (r = 0; r < 3; r++)
        scale *= sqrt(m[3 * r] * m[3 * r] + m[3 * r + 1] * m[3 * r + 1] + m[3 * r + 2] * m[3 * r + 2]);
    if (!isfinite(det) || !(scale > 0.0) || !(fabs(det) > 1e-12 * scale))
        return SIFT3D_FAILURE;
    for (i = 0; i < 9; i++)
        c[i] /= det;
    for (r = 0; r < 3; r++)
        t[r] = -(c[3 * r] * A[3] + c[3 * r + 1] * A[7] + c[3 * r + 2] * A[11]);
    for (r = 0; r < 3; r++) {
        for (i = 0; i < 3; i++)
            Ainv[4 * r + i] = c[3 * r + i];
        Ainv[4 * r + 3] = t[r];
    }
    for (i = 0; i < 12; i++)
        if (!isfinite(Ainv[i]))
            return SIFT3D_FAILURE;
    return SIFT3D_SUCCESS;
}

int sift3d_amd_image_warp_affine(const sift3d_image *src, const double *A, int interp, float fill,
                                 sift3d_image *dst)
{
    float *d_src = NULL, *d_dst = NULL;
    size_t ns, nd;
    int i, rc = SIFT3D_FAILURE;
    if (!src || !dst || !A || !src->data || !dst->data) {
        ERR("sift3d_amd_image_warp_affine: NULL argument \n");
        return SIFT3D_FAILURE;
    }
    if (src->nc != 1 || dst->nc != 1) {
        ERR("sift3d_amd_image_warp_affine: only single-channel images are supported \n");
        return SIFT3D_FAILURE;
    }
    if (check_dims("sift3d_amd_image_warp_affine", src->nx, src->ny, src->nz) ||
        check_dims("sift3d_amd_image_warp_affine", dst->nx, dst->ny, dst->nz))
        return SIFT3D_FAILURE;
    if (interp != SIFT3D_AMD_INTERP_NEAREST && interp != SIFT3D_AMD_INTERP_LINEAR) {
        ERR("sift3d_amd_image_warp_affine: unknown interpolation mode %d \n", interp);
        return SIFT3D_FAILURE;
    }
    for (i = 0; i < 12; i++)
        if (!isfinite(A[i])) {
            ERR("sift3d_amd_image_warp_affine: the affine map is not finite \n");
            return SIFT3D_FAILURE;
        }
    if (!sift3d_amd_device_available()) {
        ERR("sift3d_amd: no HIP device is available; this library has no CPU path \n");
        return SIFT3D_FAILURE;
    }
    ns = sizeof(float) * (size_t)src->nx * src->ny * src->nz;
    nd = sizeof(float) * (size_t)dst->nx * dst->ny * dst->nz;
    d_src = (float *)sift3d_hip_malloc(ns);
    d_dst = (float *)sift3d_hip_malloc(nd);
    if (d_src && d_dst && !sift3d_hip_memcpy_h2d(d_src, src->data, ns, NULL) &&
        !sift3d_hip_warp_affine(d_src, src->nx, src->ny, src->nz, d_dst, dst->nx, dst->ny, dst->nz, A, interp,
                                fill, NULL) &&
        !sift3d_hip_memcpy_d2h(dst->data, d_dst, nd, NULL) && !sift3d_hip_stream_sync(NULL))
        rc = SIFT3D_SUCCESS;
    sift3d_hip_free(d_src);
    sift3d_hip_free(d_dst);
    return rc;
}

/* ---- displacement fields: blocking host forms of sift3d_hip_warp_field / sift3d_hip_jacobian_det ---- */

int sift3d_amd_image_warp_field(const sift3d_image *src, const float *field, int interp, float fill,
                                sift3d_image *dst)
{
    float *d_src = NULL, *d_dst = NULL, *d_field = NULL;
    size_t ns, nd;
    int rc = SIFT3D_FAILURE;
    if (!src || !dst || !field || !src->data || !dst->data) {
        ERR("sift3d_amd_image_warp_field: NULL argument \n");
        return SIFT3D_FAILURE;
    }
    if (src->nc != 1 || dst->nc != 1) {
        ERR("sift3d_amd_image_warp_field: only single-channel images are supported \n");
        return SIFT3D_FAILURE;
    }
    if (check_dims("sift3d_amd_image_warp_field", src->nx, src->ny, src->nz) ||
        check_dims("sift3d_amd_image_warp_field", dst->nx, dst->ny, dst->nz))
        return SIFT3D_FAILURE;
    if (interp != SIFT3D_AMD_INTERP_NEAREST && interp != SIFT3D_AMD_INTERP_LINEAR) {
        ERR("sift3d_amd_image_warp_field: unknown interpolation mode %d \n", interp);
        return SIFT3D_FAILURE;
    }
    ns = sizeof(float) * (size_t)src->nx * src->ny * src->nz;
    nd = sizeof(float) * (size_t)dst->nx * dst->ny * dst->nz;
    if (ranges_overlap((range_t){ dst->data, nd }, (range_t){ src->data, ns }) ||
        ranges_overlap((range_t){ dst->data, nd }, (range_t){ field, 3 * nd })) {
        ERR("sift3d_amd_image_warp_field: the destination overlaps the source or the field \n");
        return SIFT3D_FAILURE;
    }
    if (!sift3d_amd_device_available()) {
        ERR("sift3d_amd: no HIP device is available; this library has no CPU path \n");
        return SIFT3D_FAILURE;
    }
    d_src = (float *)sift3d_hip_malloc(ns);
    d_dst = (float *)sift3d_hip_malloc(nd);
    d_field = (float *)sift3d_hip_malloc(3 * nd);
    if (d_src && d_dst && d_field && !sift3d_hip_memcpy_h2d(d_src, src->data, ns, NULL) &&
        !sift3d_hip_memcpy_h2d(d_field, field, 3 * nd, NULL) &&
        !sift3d_hip_warp_field(d_src, src->nx, src->ny, src->nz, 1, d_field, dst->nx, dst->ny, dst->nz, d_dst,
                               interp, fill, NULL) &&
        !sift3d_hip_memcpy_d2h(dst->data, d_dst, nd, NULL) && !sift3d_hip_stream_sync(NULL))
        rc = SIFT3D_SUCCESS;
    sift3d_hip_free(d_src);
    sift3d_hip_free(d_dst);
    sift3d_hip_free(d_field);
    return rc;
}

int sift3d_amd_jacobian_det(const float *field, int ox, int oy, int oz, float *det, uint64_t *folded, float *min,
                            float *max)
{
    float *d_field = NULL, *d_det = NULL;
    unsigned char *d_stats = NULL, stats[SIFT3D_AMD_JACOBIAN_STATS_BYTES];
    size_t nd;
    int rc = SIFT3D_FAILURE;
    if (!field || !folded || !min || !max) {
        ERR("sift3d_amd_jacobian_det: NULL argument \n");
        return SIFT3D_FAILURE;
    }
    if (check_dims("sift3d_amd_jacobian_det", ox, oy, oz))
        return SIFT3D_FAILURE;
    nd = sizeof(float) * (size_t)ox * oy * oz;
    if (det && ranges_overlap((range_t){ det, nd }, (range_t){ field, 3 * nd })) {
        ERR("sift3d_amd_jacobian_det: det overlaps the field \n");
        return SIFT3D_FAILURE;
    }
    if (!sift3d_amd_device_available()) {
        ERR("sift3d_amd: no HIP device is available; this library has no CPU path \n");
        return SIFT3D_FAILURE;
    }
    d_field = (float *)sift3d_hip_malloc(3 * nd);
    d_det = det ? (float *)sift3d_hip_malloc(nd) : NULL;
    d_stats = (unsigned char *)sift3d_hip_malloc(SIFT3D_AMD_JACOBIAN_STATS_BYTES);
    if (d_field && (d_det || !det) && d_stats && !sift3d_hip_memcpy_h2d(d_field, field, 3 * nd, NULL) &&
        !sift3d_hip_jacobian_det(d_field, ox, oy, oz, d_det, d_stats, NULL) &&
        (!det || !sift3d_hip_memcpy_d2h(det, d_det, nd, NULL)) &&
        !sift3d_hip_memcpy_d2h(stats, d_stats, sizeof(stats), NULL) && !sift3d_hip_stream_sync(NULL)) {
        memcpy(folded, stats, 8);
        memcpy(min, stats + 8, 4);
        memcpy(max, stats + 12, 4);
        rc = SIFT3D_SUCCESS;
    }
    sift3d_hip_free(d_field);
    sift3d_hip_free(d_det);
    sift3d_hip_free(d_stats);
    return rc;
}
