/* sift3d_field_ops.c -- field composition, exponential and inverse (included at the end of sift3d_host.c, after
 * sift3d_checks.c and ahead of sift3d_demons.c, whose diffeomorphic update uses the exponential).
 *
 * The contract is in include/sift3d_amd.h, "Field composition, exponential and inverse".  The composition sample is
 * k_field_compose of sift3d_warp.hip, reached through the launcher below after the checks here; the exponential
 * and the inverse ping-pong inside d_work.  Arguments are checked before the device is touched, so bad input is
 * refused on a machine without a GPU too. */

int sift3d_field_compose_launch(const float *d_u, int ux, int uy, int uz, const float *d_v, int ox, int oy, int oz,
                                float *d_out, int mode, void *d_stats, void *d_work, void *stream);
int sift3d_field_scale_launch(float *d_dst, const float *d_src, size_t n, float s, void *stream);
int sift3d_field_bracket_launch(const float *d_a, const float *d_b, int ox, int oy, int oz, float *d_out, int mode,
                                void *stream);

/* floats of the invert driver's d_work ahead of its second iterate: the composition's partials */
#define FIELD_PART_FLOATS (SIFT3D_AMD_FIELD_WORK_BYTES / sizeof(float))

int sift3d_hip_field_compose(const float *d_u, int ux, int uy, int uz, const float *d_v, int ox, int oy, int oz,
                             float *d_out, int mode, void *d_stats, void *d_work, void *stream)
{
    static const char what[] = "sift3d_hip_field_compose";
    range_t out[3];
    int nout = 0;
    if (!d_u || !d_v || (!d_out && !d_stats) || (d_stats && !d_work))
        return refuse(what, "NULL argument");
    if (check_dims(what, ux, uy, uz) || check_dims(what, ox, oy, oz))
        return SIFT3D_FAILURE;
    if (mode != SIFT3D_AMD_FIELD_COMPOSE && mode != SIFT3D_AMD_FIELD_INVERT)
        return refuse(what, "unknown mode");
    if (check_aligned(what, ADDR(d_stats) | ADDR(d_work), ADDR(d_u) | ADDR(d_v) | ADDR(d_out)))
        return SIFT3D_FAILURE;
    if (d_out)
        out[nout++] = (range_t){ d_out, field_bytes(ox, oy, oz) };
    if (d_stats) {
        out[nout++] = (range_t){ d_stats, SIFT3D_AMD_FIELD_STATS_BYTES };
        out[nout++] = (range_t){ d_work, SIFT3D_AMD_FIELD_WORK_BYTES };
    }
    {
        const range_t in[] = { { d_u, field_bytes(ux, uy, uz) }, { d_v, field_bytes(ox, oy, oz) } };
        if (ranges_aliased(out, nout, in, 2))
            return refuse(what, ALIASED);
    }
    return sift3d_field_compose_launch(d_u, ux, uy, uz, d_v, ox, oy, oz, d_out, mode, d_stats, d_work, stream);
}

size_t sift3d_amd_field_exp_work_floats(int ox, int oy, int oz)
{
    if (ox <= 0 || oy <= 0 || oz <= 0)
        return 0;
    return 3 * grid_voxels(ox, oy, oz);
}

/* w_K of the exponential into d_out, w_0 = d_v * (sign * 2^-K) with sign +1 or -1 (exp(v), exp(-v)), ping-pong
 * between d_out and d_other (K >= 1; K == 0 only scales, into d_out); d_v may be d_other (it is read only by the
 * scaling) */
static int field_exp_run(const float *d_v, int ox, int oy, int oz, int K, double sign, float *d_out, float *d_other,
                         void *stream)
{
    const size_t n3 = 3 * grid_voxels(ox, oy, oz);
    float *a, *b;
    int k;
    /* w_k for even k lands in `a`: choose it so that w_K is in d_out */
    a = (K % 2 == 0) ? d_out : d_other;
    b = (K % 2 == 0) ? d_other : d_out;
    if (sift3d_field_scale_launch(a, d_v, n3, (float)ldexp(sign, -K), stream))
        return SIFT3D_FAILURE;
    for (k = 0; k < K; k++) {
        float *src = (k % 2 == 0) ? a : b, *dst = (k % 2 == 0) ? b : a;
        if (sift3d_field_compose_launch(src, ox, oy, oz, src, ox, oy, oz, dst, SIFT3D_AMD_FIELD_COMPOSE, NULL, NULL,
                                        stream))
            return SIFT3D_FAILURE;
    }
    return SIFT3D_SUCCESS;
}

/* the two exponential entries: the checks, then exp(v) (negate 0; K == 0 copies) or exp(-v) (negate 1) */
static int field_exp_checked(const char *what, const float *d_v, int ox, int oy, int oz, int squarings, int negate,
                             float *d_out, float *d_work, void *stream)
{
    if (!d_v || !d_out || !d_work)
        return refuse(what, "NULL argument");
    if (check_dims(what, ox, oy, oz) || check_squarings(what, squarings) ||
        check_aligned(what, ADDR(d_work), ADDR(d_v) | ADDR(d_out)))
        return SIFT3D_FAILURE;
    {
        const range_t in[] = { { d_v, field_bytes(ox, oy, oz) } };
        const range_t out[] = { { d_out, field_bytes(ox, oy, oz) },
                                { d_work, sift3d_amd_field_exp_work_floats(ox, oy, oz) * sizeof(float) } };
        if (ranges_aliased(out, 2, in, 1))
            return refuse(what, ALIASED);
    }
    if (squarings == 0 && !negate)
        return sift3d_hip_memcpy_d2d(d_out, d_v, field_bytes(ox, oy, oz), stream);
    return field_exp_run(d_v, ox, oy, oz, squarings, negate ? -1.0 : 1.0, d_out, d_work, stream);
}

int sift3d_amd_field_exp_device(const float *d_v, int ox, int oy, int oz, int squarings, float *d_out, float *d_work,
                                void *stream)
{
    return field_exp_checked("sift3d_amd_field_exp_device", d_v, ox, oy, oz, squarings, 0, d_out, d_work, stream);
}

int sift3d_amd_field_exp_signed_device(const float *d_v, int ox, int oy, int oz, int squarings, int negate,
                                       float *d_out, float *d_work, void *stream)
{
    static const char what[] = "sift3d_amd_field_exp_signed_device";
    if (negate != 0 && negate != 1)
        return refuse(what, "negate must be 0 or 1");
    return field_exp_checked(what, d_v, ox, oy, oz, squarings, negate, d_out, d_work, stream);
}

int sift3d_hip_field_bracket(const float *d_a, const float *d_b, int ox, int oy, int oz, float *d_out, int mode,
                             void *stream)
{
    static const char what[] = "sift3d_hip_field_bracket";
    if (!d_a || !d_b || !d_out)
        return refuse(what, "NULL argument");
    if (check_dims(what, ox, oy, oz))
        return SIFT3D_FAILURE;
    if (mode != SIFT3D_AMD_FIELD_BRACKET && mode != SIFT3D_AMD_FIELD_BCH1)
        return refuse(what, "unknown mode");
    if (check_aligned(what, 0, ADDR(d_a) | ADDR(d_b) | ADDR(d_out)))
        return SIFT3D_FAILURE;
    {
        const range_t in[] = { { d_a, field_bytes(ox, oy, oz) }, { d_b, field_bytes(ox, oy, oz) } };
        const range_t out[] = { { d_out, field_bytes(ox, oy, oz) } };
        if (ranges_aliased(out, 1, in, 2))
            return refuse(what, ALIASED);
    }
    return sift3d_field_bracket_launch(d_a, d_b, ox, oy, oz, d_out, mode, stream);
}

size_t sift3d_amd_field_invert_work_floats(int ox, int oy, int oz)
{
    if (ox <= 0 || oy <= 0 || oz <= 0)
        return 0;
    return FIELD_PART_FLOATS + 3 * grid_voxels(ox, oy, oz);
}

int sift3d_amd_field_invert_device(const float *d_u, int ux, int uy, int uz, float *d_w, int ox, int oy, int oz,
                                   int iterations, float *d_work, void *d_stats, void *stream)
{
    static const char what[] = "sift3d_amd_field_invert_device";
    float *cur, *nxt, *t;
    int k;
    if (!d_u || !d_w || !d_work || !d_stats)
        return refuse(what, "NULL argument");
    if (check_dims(what, ux, uy, uz) || check_dims(what, ox, oy, oz) || check_iterations(what, iterations) ||
        check_aligned(what, ADDR(d_work) | ADDR(d_stats), ADDR(d_u) | ADDR(d_w)))
        return SIFT3D_FAILURE;
    {
        const range_t in[] = { { d_u, field_bytes(ux, uy, uz) } };
        const range_t out[] = { { d_w, field_bytes(ox, oy, oz) },
                                { d_work, sift3d_amd_field_invert_work_floats(ox, oy, oz) * sizeof(float) },
                                { d_stats, (size_t)SIFT3D_AMD_FIELD_STATS_BYTES * ((size_t)iterations + 1) } };
        if (ranges_aliased(out, 3, in, 1))
            return refuse(what, ALIASED);
    }
    cur = d_w;
    nxt = d_work + FIELD_PART_FLOATS;
    for (k = 0; k < iterations; k++) {
        if (sift3d_field_compose_launch(d_u, ux, uy, uz, cur, ox, oy, oz, nxt, SIFT3D_AMD_FIELD_INVERT,
                                        (char *)d_stats + (size_t)SIFT3D_AMD_FIELD_STATS_BYTES * k, d_work, stream))
            return SIFT3D_FAILURE;
        t = cur; cur = nxt; nxt = t;
    }
    if (sift3d_field_compose_launch(d_u, ux, uy, uz, cur, ox, oy, oz, NULL, SIFT3D_AMD_FIELD_INVERT,
                                    (char *)d_stats + (size_t)SIFT3D_AMD_FIELD_STATS_BYTES * iterations, d_work,
                                    stream))
        return SIFT3D_FAILURE;
    if (cur != d_w)
        return sift3d_hip_memcpy_d2d(d_w, cur, field_bytes(ox, oy, oz), stream);
    return SIFT3D_SUCCESS;
}
