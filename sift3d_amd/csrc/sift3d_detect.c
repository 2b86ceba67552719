/* sift3d_detect.c -- the hot path: the host drivers of detect and describe on one device.
 * Included by sift3d_host.c (private layouts, stores, filter bank and geometry: there); the files included
 * after it (sift3d_sharded.c, sift3d_dense.c, sift3d_demons.c) use blur_level and host_threads.
 *
 * detect_on_device and sift3d_extract_descriptors are lists of stages; what one stage of a detect call
 * decides for the later ones travels in a detect_run.  Every comment on WHY the schedule is as it is carries
 * a measurement and stays with the calls it explains. */

/* ------------------------------------------------------------------------ */
/* the hot path                                                              */
/* ------------------------------------------------------------------------ */
static int require_device(void)
{
    if (!sift3d_amd_device_available()) {
        ERR("sift3d_amd: no HIP device is available; this library has no CPU path \n");
        return SIFT3D_FAILURE;
    }
    return SIFT3D_SUCCESS;
}

static int ensure_device(sift3d_detector *d)
{
    int i;
    if (d->stream) {
        /* a detector lives on the device it first ran on (its streams, pyramids, tables) */
        if (sift3d_hip_current_device() != d->device) {
            ERR("sift3d_amd: this detector belongs to HIP device %d, the current device is %d \n",
                d->device, sift3d_hip_current_device());
            return SIFT3D_FAILURE;
        }
        return SIFT3D_SUCCESS;
    }
    if (require_device())
        return SIFT3D_FAILURE;
    d->device = sift3d_hip_current_device();
    if (!(d->stream = sift3d_hip_stream_create()) || !(d->oct_stream = sift3d_hip_stream_create_high()) ||
        !(d->side_stream = sift3d_hip_stream_create_high()) || !(d->ev_fork = sift3d_hip_event_create()) ||
        !(d->ev_join = sift3d_hip_event_create()) || !(d->ev_join2 = sift3d_hip_event_create()) ||
        !(d->ev_part = sift3d_hip_event_create()) ||
        !(d->ev_pyr[0] = sift3d_hip_event_create()) || !(d->ev_pyr[1] = sift3d_hip_event_create()))
        return SIFT3D_FAILURE;
    for (i = 0; i < 32; i++)
        if (!(d->ev_oct[i] = sift3d_hip_event_create()))
            return SIFT3D_FAILURE;
    for (i = 0; i < 8; i++)
        if (!(d->ev[i] = sift3d_hip_event_create()))
            return SIFT3D_FAILURE;
    for (i = 0; i < SIFT3D_AMD_TIMED_BLURS * 3; i++)
        if (!(d->ev_blur[i / 3][i % 3] = sift3d_hip_event_create()))
            return SIFT3D_FAILURE;
    return upload_mesh();
}

/* One-time device-side tables for callers of the stage ABI that do not go through a
 * detector (the multi-GPU driver). */
int sift3d_amd_init(void)
{
    return require_device() ? SIFT3D_FAILURE : upload_mesh();
}

static int ensure_cand_capacity(sift3d_detector *d, uint32_t cap)
{
    if (cap <= d->cand_cap)
        return SIFT3D_SUCCESS;
    free_cand_arrays(d);
    d->d_cand = (sift3d_hip_cand *)sift3d_hip_malloc(sizeof(sift3d_hip_cand) * (size_t)cap);
    d->h_cand = (sift3d_hip_cand *)sift3d_hip_host_alloc(sizeof(sift3d_hip_cand) * (size_t)cap);
    d->h_R = (float *)sift3d_hip_host_alloc(sizeof(float) * 9 * (size_t)cap);
    /* (+ 4 page-locked words behind the flags: the candidate counts land there -- a copy into pageable memory
     * would hold the host until it has been carried out) */
    d->h_keep = (int32_t *)sift3d_hip_host_alloc(sizeof(int32_t) * ((size_t)cap + 4));
    if (!d->d_cand || !d->h_cand || !d->h_R || !d->h_keep)
        return SIFT3D_FAILURE;
    d->cand_cap = cap;
    return SIFT3D_SUCCESS;
}

/* `waiter` goes on when what `src` holds so far has ended: an event recorded there, then waited for */
static int stream_after(void *waiter, void *ev, void *src)
{
    return sift3d_hip_event_record(ev, src) || sift3d_hip_stream_wait_event(waiter, ev);
}

/* ---- what the stages ask of the detector's arrays (d_scalars: laid out as the struct says) ---- */
static inline float *dogmax_slot(const sift3d_detector *d, int o) { return d->d_scalars + 8 + o * d->ndl; }
static inline float *dogmax_bound_slot(const sift3d_detector *d, int o) { return dogmax_slot(d, d->num_octaves + o); }
static inline uint32_t *cand_counter(const sift3d_detector *d) { return (uint32_t *)(d->d_scalars + 1); }
static inline const float *const *octave_levels(const sift3d_detector *d, int o)
{
    return (const float *const *)(d->d_g + o * d->ngl);
}
/* the extrema work area of an octave's side-by-side sweep (octaves >= 1: kept between the two phases) */
static inline void *extrema_work(const sift3d_detector *d, int o, size_t *bytes)
{
    *bytes = o ? sift3d_hip_extrema_work_bytes(d->odims[o][0], d->odims[o][1], d->odims[o][2], 3) : d->work_bytes;
    return o ? (void *)((char *)d->d_work2 + d->work2_off[o]) : d->d_work;
}
/* the DoG-free extrema sweep (sift3d_hip_extrema_gauss6) covers octave o: the default configuration */
static inline int dog_free_covers(const sift3d_detector *d, int o)
{
    return !d->cuboid_extrema && d->ngl == 6 && (d->odims[o][0] & 3) == 0 && d->odims[o][2] >= 3;
}
/* octaves whose dogmax scan is gathered by the extrema sweep: those large enough for the saved bytes to
 * outweigh four more (short) launches */
static inline int est_octave(const sift3d_detector *d, int o)
{
    return d->est0 && octave_voxels(d, o) >= ((size_t)1 << 21);
}

/* DoG levels of one octave in memory -- only for configurations the DoG-free extrema sweep
 * does not cover (sift3d_hip_extrema_gauss6) */
static int ensure_dog_octave(sift3d_detector *d, int o)
{
    const size_t n = octave_voxels(d, o);
    int s;
    for (s = 0; s < d->ndl; s++)
        if (!d->d_d[o * d->ndl + s] &&
            !(d->d_d[o * d->ndl + s] = (float *)sift3d_hip_malloc(n * sizeof(float))))
            return SIFT3D_FAILURE;
    return SIFT3D_SUCCESS;
}

/* Half widths (bit hw) at which one k_fir_xyz_dma launch beats k_fir_x_u1f + k_fir_yz_dma inside a pyramid
 * build, the first blur -- which divides by the image's maximum -- included; volumes below FIR_XYZ_MIN_VOXELS
 * keep the pair: at 128^3 it is faster at every width (profiles/microbench/fir_xyz_mi355x.txt). */
#define FIR_XYZ_WINS 0x3Cu
#define FIR_XYZ_MIN_VOXELS ((size_t)256 * 256 * 256)
static int fir_xyz_wins(int hw, size_t voxels)
{
    return hw >= 1 && hw <= 8 && ((FIR_XYZ_WINS >> hw) & 1) && voxels >= FIR_XYZ_MIN_VOXELS;
}

/* One FIR pass of a blur along `axis` over the whole volume; d_scale_max (x pass only, else NULL): of
 * src / *d_scale_max.  Returns what the launch returns (the scaled x pass: 1 when it cannot do that). */
static int fir_pass(const float *src, float *dst, const int *dims, const double *lu, const filter_t *f, int axis,
                    const float *d_scale_max, void *stream)
{
    sift3d_hip_fir_args a;
    memset(&a, 0, sizeof(a));
    a.src = src; a.dst = dst;
    a.nx = dims[0]; a.ny = dims[1]; a.nz = dims[2];
    a.axis = axis; a.width = f->width; a.taps = f->taps;
    a.unit_factor = (float)(1.0 / lu[axis]);       /* unit = 1.0: sift.c:675, imutil.c:754-755 */
    a.n_glob = dims[2]; a.z_lo = 0; a.z_hi = dims[2];
    return d_scale_max ? sift3d_hip_fir_x_scaled(&a, d_scale_max, stream) : sift3d_hip_fir(&a, stream);
}

/* apply_Sep_FIR_filter (imutil.c:1127-1206) on the device: x, y, z passes, no permute copies.  Octave 0 of
 * a pyramid (tap spacing 1): ONE launch for the narrow filters on large volumes (fir_xyz_wins: no intermediate
 * leaves the chip), else the x pass into tmp_a and the fused y+z launch; other spacings: three passes with the
 * two intermediates in the scratch volumes.  dst may be src.  d (may be NULL: no timing)
 * holds the events of the timed blurs; slot < 0 times nothing */
/* d_scale_max (first blur of the pyramid only, else NULL): the blur of src / *d_scale_max -- im_scale folded
 * into the x pass; returns 2 without doing anything when the configuration's x pass cannot do that (the
 * caller then scales the image first) */
static int blur_level(sift3d_detector *d, const float *src, float *dst, const int *dims,
                      const double *lu, const filter_t *f, void *stream, float *tmp_a, float *tmp_b,
                      int slot, const float *d_scale_max)
{
    const float *in = src;
    float *outs[3] = { tmp_a, tmp_b, dst };
    int ax = 0;
    /* tap spacing 1 on y and z (octave 0 of a unit-spaced volume): one launch, or the x pass, then the fused
     * y+z kernel -- the y-pass result never goes to HBM */
    if ((float)(1.0 / lu[1]) == 1.0f && (float)(1.0 / lu[2]) == 1.0f) {
        int rc;
        if (!d || slot >= SIFT3D_AMD_TIMED_BLURS)
            slot = -1;
        if (slot >= 0)
            sift3d_hip_event_record(d->ev_blur[slot][0], stream);
        /* the whole blur in one launch where that is covered and measured faster than the pair below: neither
         * intermediate goes to HBM, tmp_a is not used.  Its time is the slot's y+z time; its x time reads 0.
         * (The pyramid only -- d is set --: the smoothing passes of the demons and dense drivers were not
         * measured and keep the pair.) */
        if (d && fir_xyz_wins(f->width / 2, (size_t)dims[0] * dims[1] * dims[2]) &&
            sift3d_hip_fir_xyz_covers(src, dst, dims[0], dims[1], dims[2], f->width, (float)(1.0 / lu[0]),
                                      (float)(1.0 / lu[1]), (float)(1.0 / lu[2]))) {
            if (sift3d_hip_fir_xyz(src, dst, dims[0], dims[1], dims[2], f->taps, f->width, d_scale_max, stream))
                return SIFT3D_FAILURE;
            if (slot >= 0) {
                sift3d_hip_event_record(d->ev_blur[slot][2], stream);
                d->yz_timed |= 1u << slot;
                d->xyz_timed |= 1u << slot;
            }
            return SIFT3D_SUCCESS;
        }
        rc = fir_pass(src, tmp_a, dims, lu, f, 0, d_scale_max, stream);
        if (rc == 1 && d_scale_max)
            return 2;
        if (rc != SIFT3D_SUCCESS)
            return SIFT3D_FAILURE;
        if (slot >= 0)
            sift3d_hip_event_record(d->ev_blur[slot][1], stream);
        /* (asking first: the fused kernel refuses rows shorter than 4 outright) */
        rc = sift3d_hip_fir_yz_u1_covers(tmp_a, dst, dims[0], dims[1], f->width, dims[2])
                 ? sift3d_hip_fir_yz_u1(tmp_a, dst, dims[0], dims[1], dims[2], f->taps, f->width, dims[2], 0, 0,
                                        dims[2], stream)
                 : 1;
        if (rc == SIFT3D_SUCCESS) {
            if (slot >= 0) {
                sift3d_hip_event_record(d->ev_blur[slot][2], stream);
                d->yz_timed |= 1u << slot;
            }
            return SIFT3D_SUCCESS;
        }
        if (rc != 1)
            return SIFT3D_FAILURE;
        in = tmp_a;                 /* not covered: finish with separate y and z passes */
        ax = 1;
    } else if (d_scale_max) {
        return 2;
    }
    for (; ax < 3; ax++) {
        if (fir_pass(in, outs[ax], dims, lu, f, ax, NULL, stream))
            return SIFT3D_FAILURE;
        in = outs[ax];
    }
    return SIFT3D_SUCCESS;
}

/* device part of sift3d_detect_keypoints (sift.c:1217-1249) */
/* Host loops over the candidate / keypoint lists (10^5 records at 512^3) run between the last kernel of
 * one stage and the first of the next, with the device idle: a few threads, statically split so that the
 * order of the records -- the reference's scan order -- is kept. */
#define HOST_THREADS_MAX 8
static int host_threads(size_t n)
{
    int t = omp_get_num_procs();
    if (t > HOST_THREADS_MAX)
        t = HOST_THREADS_MAX;
    if (n < 4096 || t < 1)
        t = 1;
    return t;
}

/* scratch of the orientation kernels: sized by the level count and the candidate capacity; its zeroing is
 * complete before any stream's kernels use it */
static int orient_scratch(sift3d_detector *d)
{
    return orient_tab_reserve(&d->d_otab, &d->otab_bytes, d->num_octaves * d->ngl, d->cand_cap, d->stream, 1);
}

/* Candidates first .. first + n - 1 (all of levels lv_lo .. lv_hi - 1) through the orientation kernels.  R and
 * the keep flags are written by the kernels straight into the page-locked host arrays (mapped into the device's
 * address space; only kept candidates' matrices are written): no device staging, no copy after the kernels. */
static int orient_part(sift3d_detector *d, int lv_lo, int lv_hi, uint32_t first, uint32_t n, int slot, void *stream)
{
    float *r_view = (float *)sift3d_hip_host_device_ptr(d->h_R);
    int32_t *k_view = (int32_t *)sift3d_hip_host_device_ptr(d->h_keep);
    if (!r_view || !k_view)
        return SIFT3D_FAILURE;
    /* the serial sums pack window-relative x and y into 10 bits each (sift3d_hip_orient_window_fits) */
    for (int t = lv_lo; n && t < lv_hi; t++) {
        const sift3d_hip_level *L = d->h_levels + t;
        if (!sift3d_hip_orient_window_fits(L->nx, L->ny, (double)L->ux, (double)L->uy, L->sd)) {
            ERR("sift3d_amd: the orientation window of a %d x %d level with units (%f, %f) at scale %f is wider "
                "than 1023 voxels \n", L->nx, L->ny, (double)L->ux, (double)L->uy, L->sd);
            return SIFT3D_FAILURE;
        }
    }
    return sift3d_hip_orient_tab_part(d->d_levels, d->num_octaves * d->ngl, lv_lo, lv_hi, d->d_cand, first, n,
                                      d->corner_thresh, r_view, k_view, d->orient_serial ? NULL : d->d_otab,
                                      d->cand_cap, slot, stream);
}

/* What the stages of ONE detect call pass to each other: every field is set by the stage that decides it and
 * only read after that.  Nothing of it outlives the call. */
typedef struct {
    const float *vol;      /* the volume on the device, n0 voxels */
    size_t n0;
    double t_start;
    int side;              /* default configuration on every octave: octaves >= 1 beside octave 0 after the pyramid */
    int ds;                /* octave o + 1 starts from level ds + 1 (Gaussian index) of octave o */
    int forked, overlap;   /* the pyramid is built on three chains; the main stream does not wait for the other two */
    int im_stored;         /* the first blur could not fold the scale: d_im holds the scaled image */
    uint32_t count, count_a; /* candidates; count_a of them are octave 0's (split emission) */
    int oriented;          /* the extrema stage has emitted the list in two parts and oriented both */
} detect_run;

/* set_im_SIFT3D (sift.c:629-659), the level table, then max|v| (im_scale's divisor, imutil.c:698-713) */
static int detect_begin(sift3d_detector *d, detect_run *r, const float *d_vol, int nx, int ny, int nz,
                        double ux, double uy, double uz)
{
    const int dims_changed = !d->have_im || d->nx != nx || d->ny != ny || d->nz != nz ||
                             !d->num_octaves;
    uint64_t rng;
    int o;
    memset(r, 0, sizeof(*r));
    r->t_start = now_s();
    r->vol = d_vol;
    r->n0 = (size_t)nx * ny * nz;

    d->have_im = 1;
    d->nx = nx; d->ny = ny; d->nz = nz;
    d->units[0] = ux; d->units[1] = uy; d->units[2] = uz;
    d->have_pyramid = 0;
    d->im_valid = 0;                    /* (both are set again only by a call that succeeds) */
    d->last_vol = NULL;
    d->t_pending &= ~1;                 /* the stage events are re-recorded from here on */
    if (dims_changed && resize_detector(d)) {
        d->have_im = 0;
        return SIFT3D_FAILURE;
    }
    fill_level_table(d);
    if (sift3d_hip_memcpy_h2d(d->d_levels, d->h_levels,
                              sizeof(sift3d_hip_level) * (size_t)d->num_octaves * d->ngl, d->stream))
        return SIFT3D_FAILURE;

    rng = range_start("sift3d: max|v|");
    sift3d_hip_event_record(d->ev[0], d->stream);
    if (sift3d_hip_memset(d->d_scalars, 0, sizeof(float) * (8 + 2 * (size_t)d->num_octaves * d->ndl), d->stream) ||
        sift3d_hip_absmax(d_vol, r->n0, d->d_scalars, d->stream))
        return SIFT3D_FAILURE;
    d->yz_timed = 0;
    d->xyz_timed = 0;
    d->parts_timed = 0;
    d->pyr_chains = 0;
    /* Default configuration on every octave (and a second stream at hand): the stages after the pyramid run
     * octave 0 on the main stream and the short launches of octaves >= 1 beside it -- in the DoG stage and
     * again for the extrema sweeps, whose results are then emitted in octave order. */
    r->side = d->num_octaves > 1 && d->num_octaves <= 32 && d->d_work2;
    for (o = 0; o < d->num_octaves && r->side; o++)
        r->side = dog_free_covers(d, o);
    range_stop(rng);
    return SIFT3D_SUCCESS;
}

/* levels s_lo .. s_hi - 1 of octave o, each from the level below it (gauss_octave[s], sift.c:689), on
 * `stream` with the scratch volumes ta, tb; octave 0's blurs are the timed ones */
static int blur_levels(sift3d_detector *d, int o, int s_lo, int s_hi, void *stream, float *ta, float *tb)
{
    double lu[3];
    int s;
    level_units(d, o, lu);
    for (s = s_lo; s < s_hi; s++)
        if (blur_level(d, d->d_g[o * d->ngl + s - 1], d->d_g[o * d->ngl + s], d->odims[o], lu, &d->filt[s],
                       stream, ta, tb, o == 0 ? s : -1, NULL))
            return SIFT3D_FAILURE;
    return SIFT3D_SUCCESS;
}

/* the first level of octave o + 1 from its source level of octave o (sift.c:696-704) */
static int downsample_octave(sift3d_detector *d, const detect_run *r, int o, void *stream)
{
    return sift3d_hip_downsample2(d->d_g[o * d->ngl + r->ds + 1], d->odims[o][0], d->odims[o][1],
                                  d->d_g[(o + 1) * d->ngl], d->odims[o + 1][0], d->odims[o + 1][1],
                                  d->odims[o + 1][2], stream);
}

/* The first blur reads the volume itself and divides every sample by the maximum as it stages it (im_scale,
 * imutil.c:698-713): the scaled image -- read by nothing else -- is not stored (8 B/voxel less;
 * sift3d_amd_copy_level forms it on demand from `last_vol`).  Where the x pass cannot do that (other tap
 * spacings) the image is scaled first, as before. */
static int first_blur(sift3d_detector *d, detect_run *r)
{
    double lu[3];
    int rc;
    level_units(d, 0, lu);
    rc = blur_level(d, r->vol, d->d_g[0], d->odims[0], lu, &d->filt[0], d->stream, d->d_tmp_a, d->d_tmp_b, 0,
                    d->d_scalars);
    if (rc == 2) {
        if (sift3d_hip_scale(r->vol, d->d_im, r->n0, d->d_scalars, d->stream) ||
            blur_level(d, d->d_im, d->d_g[0], d->odims[0], lu, &d->filt[0], d->stream, d->d_tmp_a, d->d_tmp_b,
                       0, NULL))
            return SIFT3D_FAILURE;
        r->im_stored = 1;
        return SIFT3D_SUCCESS;
    }
    return rc;
}

/* The pyramid on three chains.  Octave o + 1 starts from level max(s_end - 2, first_level) of octave o
 * (sift.c:696-704); the levels after it belong to octave o alone.  So once that level of octave 0 exists, the
 * smaller octaves -- short kernels that cannot fill the device -- are built on a second stream BESIDE the
 * last levels of octave 0, their own last levels (which nothing waits for) on a third, and all are joined
 * before the DoG stage. */
static int build_forked_octaves(sift3d_detector *d, const detect_run *r)
{
    const int rest = r->ds + 2;  /* first level of an octave that no later octave depends on */
    int o;
    /* octave 0 up to the source level, then the fork */
    if (blur_levels(d, 0, 1, rest, d->stream, d->d_tmp_a, d->d_tmp_b) ||
        stream_after(d->oct_stream, d->ev_fork, d->stream) || downsample_octave(d, r, 0, d->oct_stream))
        return SIFT3D_FAILURE;
    /* The last levels of octave 0 are held back until octave 1 has reached ITS source level.  The
     * fused y+z kernel keeps one or two workgroups on every CU for its whole duration: beside it
     * the passes of octave 1 -- which the whole chain of smaller octaves waits for -- get what
     * registers and LDS it leaves (in the step 2-7x their stand-alone time), and it loses
     * bandwidth to them.  Octave 1's first levels alone take 0.4 ms; the pyramid's total does
     * not change (3.47-3.51 against 3.48-3.49 ms), the two large kernels' interference does. */
    /* (forked: octave 1 exists and reaches the point where they are enqueued) */
    for (o = 1; o < d->num_octaves; o++) {
        if (blur_levels(d, o, 1, rest, d->oct_stream, d->d_tmp2_a, d->d_tmp2_b))
            return SIFT3D_FAILURE;
        /* the rest of this octave leaves the critical chain */
        if (stream_after(d->side_stream, d->ev_oct[o], d->oct_stream) ||
            (o != d->num_octaves - 1 && downsample_octave(d, r, o, d->oct_stream)))
            return SIFT3D_FAILURE;
        /* ... and now octave 0's last levels, on the main stream */
        if (o == 1 && (sift3d_hip_stream_wait_event(d->stream, d->ev_oct[o]) ||
                       blur_levels(d, 0, rest, d->ngl, d->stream, d->d_tmp_a, d->d_tmp_b)))
            return SIFT3D_FAILURE;
        if (blur_levels(d, o, rest, d->ngl, d->side_stream, d->d_tmp3_a, d->d_tmp3_b))
            return SIFT3D_FAILURE;
    }
    return SIFT3D_SUCCESS;
}

/* build_gpyr, sift.c:662-711 */
static int build_pyramid(sift3d_detector *d, detect_run *r, int pyramid_only)
{
    const int s_end = d->ngl - 2;
    int o;
    sift3d_hip_event_record(d->ev[1], d->stream);
    if (first_blur(d, r))
        return SIFT3D_FAILURE;
    r->ds = s_end - 2 > -1 ? s_end - 2 : -1;
    r->forked = d->num_octaves > 1 && d->num_octaves <= 32 && r->ds + 1 < d->ngl - 1;
    if (r->forked) {
        if (build_forked_octaves(d, r))
            return SIFT3D_FAILURE;
        /* Round 5: the main stream does NOT wait for the chains of the smaller octaves here.  Octave 0's
         * DoG maxima and extrema sweep (0.9 ms, device-filling) need octave 0's levels only and start
         * when its last blur ends; the two side chains wait for EACH OTHER (an octave's levels 4, 5 are
         * built on the side stream, its first ones on the octave stream) and go on with their own
         * octaves' DoG maxima and sweeps.  All three meet again before scan + emission. */
        r->overlap = r->side && !pyramid_only;
        d->pyr_chains = 1;
        if (sift3d_hip_event_record(d->ev_pyr[0], d->oct_stream) ||
            sift3d_hip_event_record(d->ev_pyr[1], d->side_stream))
            return SIFT3D_FAILURE;
        if (r->overlap) {
            if (sift3d_hip_stream_wait_event(d->oct_stream, d->ev_pyr[1]) ||
                sift3d_hip_stream_wait_event(d->side_stream, d->ev_pyr[0]))
                return SIFT3D_FAILURE;
        } else if (sift3d_hip_stream_wait_event(d->stream, d->ev_pyr[0]) ||
                   sift3d_hip_stream_wait_event(d->stream, d->ev_pyr[1])) {
            return SIFT3D_FAILURE;
        }
    } else {
        /* one chain (a single octave): every octave in turn on the main stream */
        for (o = 0; o < d->num_octaves; o++)
            if (blur_levels(d, o, 1, d->ngl, d->stream, d->d_tmp_a, d->d_tmp_b) ||
                (o != d->num_octaves - 1 && downsample_octave(d, r, o, d->stream)))
                return SIFT3D_FAILURE;
    }
    sift3d_hip_event_record(d->ev[2], d->stream);
    return SIFT3D_SUCCESS;
}

/* build_dog (sift.c:713-732) + the dogmax scan (sift.c:821-826).  Default configuration: only
 * the maxima are computed here; the extrema sweep forms the differences itself and no DoG
 * level is stored.  Otherwise (cuboid neighbourhood, another level count, rows that are not
 * whole quads) the octave's DoG levels are stored as the reference does. */
/* Default configuration on every octave (and a second stream at hand): octave 0 on the main
 * stream, the short launches of octaves >= 1 beside it -- in the DoG stage and again for the
 * extrema sweeps, whose results are then emitted in octave order. */
static int dog_stage(sift3d_detector *d, const detect_run *r)
{
    const int side = r->side;
    int o, s;
    if (side && !r->overlap && stream_after(d->oct_stream, d->ev_fork, d->stream))
        return SIFT3D_FAILURE;
    for (o = 0; o < d->num_octaves; o++) {
        const size_t n = octave_voxels(d, o);
        int rc = 1;
        d->dog_free[o] = 0;
        if (side && est_octave(d, o))
            /* the large octaves (nearly all of the pyramid's bytes): lower bounds of their maxima from a
             * sub-lattice; the extrema sweep gathers the exact ones (sift3d_hip_extrema_gauss6_est_phase) */
            rc = sift3d_hip_dogmax_sub(octave_levels(d, o), d->odims[o][0], d->odims[o][1], d->odims[o][2],
                                       dogmax_bound_slot(d, o), o > 0 ? d->oct_stream : d->stream);
        else if (dog_free_covers(d, o))
            rc = sift3d_hip_dogmax_stack(octave_levels(d, o), d->ngl, n, dogmax_slot(d, o),
                                         side && o > 0 ? d->oct_stream : d->stream);
        if (rc == SIFT3D_SUCCESS) {
            d->dog_free[o] = 1;
            continue;
        }
        if (side) {
            ERR("sift3d_amd: octave %d is not covered by the DoG-free path \n", o);
            return SIFT3D_FAILURE;
        }
        if (rc != 1 || ensure_dog_octave(d, o))
            return SIFT3D_FAILURE;
        /* one pass over the octave's Gaussian levels when the stack kernel covers it */
        rc = sift3d_hip_dog_stack(octave_levels(d, o), d->d_d + o * d->ndl, d->ngl, n, dogmax_slot(d, o), d->stream);
        if (rc == SIFT3D_SUCCESS)
            continue;
        if (rc != 1)
            return SIFT3D_FAILURE;
        for (s = 0; s < d->ndl; s++)
            if (sift3d_hip_subtract_absmax(d->d_g[o * d->ngl + s], d->d_g[o * d->ngl + s + 1],
                                           d->d_d[o * d->ndl + s], n, dogmax_slot(d, o) + s, d->stream))
                return SIFT3D_FAILURE;
    }
    /* (overlap: the DoG maxima of octaves >= 1 are on the octave stream; the small octaves' sweeps, on the side
     * stream, wait for them -- the main stream does not) */
    if (side && stream_after(r->overlap ? d->side_stream : d->stream, d->ev_join, d->oct_stream))
        return SIFT3D_FAILURE;
    sift3d_hip_event_record(d->ev[3], d->stream);
    return SIFT3D_SUCCESS;
}

/* One phase of the DoG-free sweep of every octave.  Phase 1 on three chains: octave 0 | octaves 1, 2 | the
 * small octaves, whose 4-40 us launches (four per octave, each waiting for its predecessor) otherwise queue
 * behind octave 1's sweep and end the stage 0.1 ms after octave 0 has finished; phase 2 (scan + emission per
 * octave, where the joint finish does not cover the list) on the main stream, in octave order. */
static int sweep_side_octaves(sift3d_detector *d, int phase)
{
    int o;
    for (o = 0; o < d->num_octaves; o++) {
        void *const xs = phase != 1 || o == 0 ? d->stream : o <= 2 ? d->oct_stream : d->side_stream;
        size_t wb;
        void *wk = extrema_work(d, o, &wb);
        if (est_octave(d, o)
                ? sift3d_hip_extrema_gauss6_est_phase(octave_levels(d, o), dogmax_bound_slot(d, o), dogmax_slot(d, o),
                                                      d->odims[o][0], d->odims[o][1], d->odims[o][2], o * d->ngl + 1,
                                                      d->peak_thresh, d->d_cand, d->cand_cap, cand_counter(d), wk,
                                                      wb, xs, phase)
                : sift3d_hip_extrema_gauss6_phase(octave_levels(d, o), dogmax_slot(d, o), d->odims[o][0],
                                                  d->odims[o][1], d->odims[o][2], 1, d->odims[o][2] - 1,
                                                  o * d->ngl + 1, d->peak_thresh, d->d_cand, d->cand_cap,
                                                  cand_counter(d), wk, wb, xs, phase))
            return SIFT3D_FAILURE;       /* (coverage was established by the dogmax calls) */
    }
    return SIFT3D_SUCCESS;
}

/* what scan + emission (sift3d_hip_extrema_gauss6_finish) are told of every octave */
static void finish_octaves(const sift3d_detector *d, sift3d_hip_extrema_oct *oc)
{
    int o;
    for (o = 0; o < d->num_octaves; o++) {
        oc[o].d_g = octave_levels(d, o);
        oc[o].nx = d->odims[o][0]; oc[o].ny = d->odims[o][1]; oc[o].nz = d->odims[o][2];
        oc[o].tag0 = o * d->ngl + 1;
        oc[o].d_work = extrema_work(d, o, &oc[o].work_bytes);
    }
}

/* The default schedule's first attempt.  Octave 0's candidates are the head of the list whatever the smaller
 * octaves hold (sift.c:835-868: octave order) -- a third of it on the bench volume, whose blobs put most
 * extrema into octaves >= 1; more where the structure is fine.  Their scan + emission and their ORIENTATION
 * (device-filling: 1.5 ms for the whole list at 512^3) start as soon as octave 0's sweep has ended, on the
 * main stream; the chains of the smaller octaves -- latency-bound launches that end later -- finish beside
 * them, and their candidates are emitted behind octave 0's and oriented on the octave stream, whose kernels
 * are dispatched first.  Same list, same order.
 * Returns with r->oriented set, or -- a list that does not fit -- with r->count > d->cand_cap. */
static int finish_split_and_orient_octave0(sift3d_detector *d, detect_run *r)
{
    sift3d_hip_extrema_oct oc[32];
    volatile uint32_t *h_cnt = (volatile uint32_t *)(d->h_keep + d->cand_cap);
    uint32_t count_a;
    finish_octaves(d, oc);
    /* both emissions are enqueued before the host waits for the first count: the smaller
     * octaves' scan starts from octave 0's total (ev_part orders the two on the device) and
     * runs when their sweeps have ended -- not when the host has come back from its wait
     * and has launched octave 0's orientation kernels, which it would then queue behind */
    if (sift3d_hip_extrema_gauss6_finish(oc, 1, d->peak_thresh, d->d_cand, d->cand_cap, cand_counter(d), d->stream) ||
        sift3d_hip_memcpy_d2h((void *)(h_cnt + 0), d->d_scalars + 1, sizeof(uint32_t), d->stream) ||
        sift3d_hip_event_record(d->ev_part, d->stream) ||
        sift3d_hip_event_record(d->ev_join2, d->side_stream) ||
        sift3d_hip_stream_wait_event(d->oct_stream, d->ev_join2) ||
        sift3d_hip_stream_wait_event(d->oct_stream, d->ev_part) ||
        sift3d_hip_extrema_gauss6_finish(oc + 1, d->num_octaves - 1, d->peak_thresh, d->d_cand, d->cand_cap,
                                         cand_counter(d), d->oct_stream) ||
        sift3d_hip_memcpy_d2h((void *)(h_cnt + 1), d->d_scalars + 1, sizeof(uint32_t), d->oct_stream) ||
        sift3d_hip_stream_sync(d->stream))
        return SIFT3D_FAILURE;
    r->count = r->count_a = count_a = h_cnt[0];
    sift3d_hip_event_record(d->ev[4], d->stream);
    /* (a list that does not fit: the rest is still counted, then everything is grown
     * by the caller for the second attempt) */
    if (count_a <= d->cand_cap && orient_scratch(d))
        return SIFT3D_FAILURE;
    if (count_a && count_a <= d->cand_cap && orient_part(d, 0, d->ngl, 0, count_a, 0, d->stream))
        return SIFT3D_FAILURE;
    /* (on the main stream, ordinary priority: with the smaller octaves' launches behind
     * it in the dispatch order the two parts end together -- measured; at the chains'
     * priority this part ends 0.25 ms earlier and the other one 0.2 ms later) */
    sift3d_hip_event_record(d->ev_part, d->stream);
    /* (the records' copy: on the side stream, which has nothing else to do from here on) */
    if ((count_a && count_a <= d->cand_cap &&
         sift3d_hip_memcpy_d2h(d->h_cand, d->d_cand, sizeof(sift3d_hip_cand) * (size_t)count_a, d->side_stream)) ||
        sift3d_hip_stream_sync(d->oct_stream))
        return SIFT3D_FAILURE;
    r->count = h_cnt[1];
    if (r->count > d->cand_cap)
        return SIFT3D_SUCCESS;          /* (count_a <= count) */
    if (r->count > count_a &&
        (orient_part(d, d->ngl, d->num_octaves * d->ngl, count_a, r->count - count_a, 1, d->oct_stream) ||
         sift3d_hip_memcpy_d2h(d->h_cand + count_a, d->d_cand + count_a,
                               sizeof(sift3d_hip_cand) * (size_t)(r->count - count_a), d->oct_stream)))
        return SIFT3D_FAILURE;
    if (stream_after(d->stream, d->ev_join, d->oct_stream))
        return SIFT3D_FAILURE;
    r->oriented = 1;
    d->parts_timed = 1;
    return SIFT3D_SUCCESS;
}

/* The three chains meet on the main stream, then scan + emission of every octave in two launches (octave order
 * is kept by the scan) -- or, where those do not cover the list, phase 2 of every octave's own sweep. */
static int finish_joint(sift3d_detector *d)
{
    sift3d_hip_extrema_oct oc[32];
    int rc;
    if (stream_after(d->stream, d->ev_join, d->oct_stream) || stream_after(d->stream, d->ev_join2, d->side_stream))
        return SIFT3D_FAILURE;
    finish_octaves(d, oc);
    rc = sift3d_hip_extrema_gauss6_finish(oc, d->num_octaves, d->peak_thresh, d->d_cand, d->cand_cap,
                                          cand_counter(d), d->stream);
    if (rc == 1)
        return sweep_side_octaves(d, 2);
    return rc == SIFT3D_SUCCESS ? SIFT3D_SUCCESS : SIFT3D_FAILURE;
}

/* not `side`: every octave in turn on the main stream -- the DoG-free sweep where the DoG stage found it
 * covered, else the sweep over the stored DoG levels */
static int sweep_per_octave(sift3d_detector *d)
{
    const int nl = d->ndl - 2;
    int o, s;
    for (o = 0; o < d->num_octaves; o++) {
        sift3d_hip_extrema_level lv[8];
        if (nl > 8) {
            ERR("sift3d_amd: at most 8 keypoint levels per octave are supported \n");
            return SIFT3D_FAILURE;
        }
        if (d->dog_free[o]) {
            if (sift3d_hip_extrema_gauss6(octave_levels(d, o), dogmax_slot(d, o), d->odims[o][0], d->odims[o][1],
                                          d->odims[o][2], 1, d->odims[o][2] - 1, o * d->ngl + 1, d->peak_thresh,
                                          d->d_cand, d->cand_cap, cand_counter(d), d->d_work, d->work_bytes,
                                          d->stream))
                return SIFT3D_FAILURE;       /* (coverage was established by the dogmax call) */
            continue;
        }
        for (s = 0; s < nl; s++) {
            lv[s].prev = d->d_d[o * d->ndl + s];
            lv[s].cur = d->d_d[o * d->ndl + s + 1];
            lv[s].next = d->d_d[o * d->ndl + s + 2];
            lv[s].d_absmax = dogmax_slot(d, o) + s + 1;
            lv[s].z_lo = 1;
            lv[s].z_hi = d->odims[o][2] - 1;
            lv[s].tag = o * d->ngl + s + 1;      /* Gaussian level (o, s) of the table */
        }
        if (sift3d_hip_extrema_mode(lv, nl, d->odims[o][0], d->odims[o][1], d->odims[o][2], d->peak_thresh,
                                    d->cuboid_extrema, d->d_cand, d->cand_cap, cand_counter(d), d->d_work,
                                    d->work_bytes, d->stream))
            return SIFT3D_FAILURE;
    }
    return SIFT3D_SUCCESS;
}

/* detect_extrema, sift.c:735-871: at most two attempts -- a list that does not fit the candidate arrays is
 * still counted, the arrays are grown to hold it, and the stage runs once more */
static int extrema_stage(sift3d_detector *d, detect_run *r)
{
    int attempt;
    if (d->ndl < 3) {
        printf("detect_extrema: Requires at least 3 levels per octave, provided only %d \n", d->ndl);
        return SIFT3D_FAILURE;
    }
    if (ensure_cand_capacity(d, d->cand_cap ? d->cand_cap : d->cand_cap0 ? d->cand_cap0 : (1u << 18)))
        return SIFT3D_FAILURE;
    for (attempt = 0; attempt < 2; attempt++) {
        /* the default schedule's first attempt: octave 0 is emitted and oriented ahead of the others */
        const int split = r->overlap && attempt == 0 && d->num_octaves - 1 <= SIFT3D_HIP_EXTREMA_MAX_OCT;
        if (sift3d_hip_memset(d->d_scalars + 1, 0, sizeof(uint32_t), d->stream))
            return SIFT3D_FAILURE;
        if (r->side) {
            /* the sweeps side by side, then scan + emission in octave order */
            /* (overlap, first attempt: the side chains are already where they must be and do NOT wait for the
             * main stream, which may still be inside octave 0's last blur) */
            if ((!r->overlap || attempt > 0) && (stream_after(d->oct_stream, d->ev_fork, d->stream) ||
                                                 sift3d_hip_stream_wait_event(d->side_stream, d->ev_fork)))
                return SIFT3D_FAILURE;
            if (sweep_side_octaves(d, 1) || (split ? finish_split_and_orient_octave0(d, r) : finish_joint(d)))
                return SIFT3D_FAILURE;
        } else if (sweep_per_octave(d)) {
            return SIFT3D_FAILURE;
        }
        /* (split: the counts were read where the two parts were emitted) */
        if (!split && (sift3d_hip_memcpy_d2h(&r->count, d->d_scalars + 1, sizeof(r->count), d->stream) ||
                       sift3d_hip_stream_sync(d->stream)))
            return SIFT3D_FAILURE;
        if (r->oriented || r->count <= d->cand_cap)
            break;
        /* the list does not fit: nothing of this attempt is kept (its launches must have ended before the
         * arrays they use are replaced) */
        if (split && (sift3d_hip_stream_sync(d->stream) || sift3d_hip_stream_sync(d->oct_stream) ||
                      sift3d_hip_stream_sync(d->side_stream)))
            return SIFT3D_FAILURE;
        if (ensure_cand_capacity(d, r->count + r->count / 4 + 1024))
            return SIFT3D_FAILURE;
    }
    if (!r->oriented)
        sift3d_hip_event_record(d->ev[4], d->stream);
    d->ncand = (int)r->count;
    return SIFT3D_SUCCESS;
}

/* assign_orientations, sift.c:1109-1167 (the default schedule has started it in the extrema stage, octave 0
 * first); returns when every stream of the call has ended */
static int orient_rest(sift3d_detector *d, const detect_run *r)
{
    if (r->count && !r->oriented) {
        /* The candidate records are final (the host has just read their count): their copy runs on the
         * side stream beside the orientation kernels. */
        if (orient_scratch(d) ||
            sift3d_hip_memcpy_d2h(d->h_cand, d->d_cand, sizeof(sift3d_hip_cand) * (size_t)r->count, d->oct_stream) ||
            orient_part(d, 0, d->num_octaves * d->ngl, 0, r->count, 0, d->stream))
            return SIFT3D_FAILURE;
    }
    sift3d_hip_event_record(d->ev[5], d->stream);
    if (sift3d_hip_stream_sync(d->stream) || (r->count && sift3d_hip_stream_sync(d->oct_stream)) ||
        (r->oriented && sift3d_hip_stream_sync(d->side_stream)))
        return SIFT3D_FAILURE;
    return SIFT3D_SUCCESS;
}

/* keypoint store: dimensions of the first octave (sift.c:756-759), then the in-place
 * compaction of assign_orientations.  copy_Keypoint does not copy `strength`
 * (sift.c:372-384), so slot j keeps the strength of CANDIDATE j (quirk Q2). */
static int compact_keypoints(sift3d_detector *d, uint32_t count, sift3d_keypoint_store *kp)
{
    const int nt = host_threads(count);
    size_t pre[HOST_THREADS_MAX + 1];
    int rc = SIFT3D_SUCCESS;
    kp->nx = d->odims[0][0];
    kp->ny = d->odims[0][1];
    kp->nz = d->odims[0][2];
    pre[0] = 0;
#pragma omp parallel num_threads(nt)
    {
        /* the team may be smaller than asked for (a caller inside its own parallel region,
         * OMP_THREAD_LIMIT, OMP_DYNAMIC): the list is cut by the team's real size */
        const int nth = omp_get_num_threads(), t = omp_get_thread_num();
        const size_t lo = (size_t)count * t / nth, hi = (size_t)count * (t + 1) / nth;
        size_t q, jj = 0;
        for (q = lo; q < hi; q++)
            jj += d->h_keep[q] != 0;
        pre[t + 1] = jj;
#pragma omp barrier
#pragma omp single
        {
            int u;
            for (u = 0; u < nth; u++)
                pre[u + 1] += pre[u];
            rc = kp_store_resize(kp, pre[nth]);
        }
        /* (implicit barrier) */
        if (rc == SIFT3D_SUCCESS) {
            jj = pre[t];
            for (q = lo; q < hi; q++) {
                const sift3d_hip_cand *c = d->h_cand + q;
                const sift3d_hip_level *L = d->h_levels + c->tag;
                keypoint_t *k;
                uint32_t plane, rem, zq;
                if (!d->h_keep[q])
                    continue;
                k = kp->buf + jj;
                plane = (uint32_t)L->nx * (uint32_t)L->ny;      /* (a level has < 2^32 voxels) */
                zq = c->idx / plane;
                rem = c->idx - zq * plane;
                k->o = c->tag / d->ngl;
                k->s = c->tag % d->ngl - 1;
                k->xd = (double)(rem % (uint32_t)L->nx);
                k->yd = (double)(rem / (uint32_t)L->nx);
                k->zd = (double)zq;
                k->sd = L->sd;
                memcpy(k->R, d->h_R + 9 * q, sizeof(k->R));
                k->strength = d->h_cand[jj].val;
                jj++;
            }
        }
    }
    return rc;
}

/* what a call that succeeded leaves behind, the pyramid alone or all of it */
static int detect_end(sift3d_detector *d, const detect_run *r)
{
    d->have_pyramid = 1;
    d->im_valid = r->im_stored;
    /* The scaled image is formed on demand (sift3d_amd_copy_level, which = 2) from the volume -- but only from
     * the detector's OWN upload buffer: a caller's device pointer is not kept beyond the call (it may be
     * freed or reused the moment this returns). */
    d->last_vol = r->vol == d->d_in ? r->vol : NULL;
    d->t_pending |= 1;                  /* (the stage events are read when sift3d_amd_timings asks) */
    d->t[T_DETECT_WALL] = now_s() - r->t_start;
    return SIFT3D_SUCCESS;
}

static int detect_on_device(sift3d_detector *d, const float *d_vol, int nx, int ny, int nz,
                            double ux, double uy, double uz, sift3d_keypoint_store *kp, int pyramid_only)
{
    detect_run r;
    uint64_t rng;
    double t_compact;
    int e;

    if (detect_begin(d, &r, d_vol, nx, ny, nz, ux, uy, uz))
        return SIFT3D_FAILURE;
    rng = range_start("sift3d: Gaussian pyramid");
    if (build_pyramid(d, &r, pyramid_only))
        return SIFT3D_FAILURE;
    range_stop(rng);
    if (pyramid_only) {
        /* sift3d_amd_build_pyramid_device: the Gaussian pyramid alone (bench.py's pyramid-only leg) */
        for (e = 3; e <= 5; e++)
            sift3d_hip_event_record(d->ev[e], d->stream);      /* (the later stages: empty) */
        d->ncand = 0;
        return sift3d_hip_stream_sync(d->stream) ? SIFT3D_FAILURE : detect_end(d, &r);
    }
    rng = range_start("sift3d: DoG maxima");
    if (dog_stage(d, &r))
        return SIFT3D_FAILURE;
    range_stop(rng);
    rng = range_start("sift3d: extrema");
    if (extrema_stage(d, &r))
        return SIFT3D_FAILURE;
    range_stop(rng);
    rng = range_start("sift3d: orientation");
    if (orient_rest(d, &r))
        return SIFT3D_FAILURE;
    range_stop(rng);
    t_compact = now_s();
    if (compact_keypoints(d, r.count, kp))
        return SIFT3D_FAILURE;
    detect_end(d, &r);
    d->t[T_COMPACT] = now_s() - t_compact;
    return SIFT3D_SUCCESS;
}

/* the arguments of the two entry points that take a volume in device memory */
static int check_device_volume(const sift3d_detector *d, const float *d_volume, int nx, int ny, int nz,
                               double ux, double uy, double uz)
{
    if (!d || !d_volume || nx < 1 || ny < 1 || nz < 1)
        return SIFT3D_FAILURE;
    if (!(ux > 0) || !(uy > 0) || !(uz > 0)) {          /* as sift3d_amd_image_set_units */
        ERR("sift3d_amd: voxel spacing must be positive, provided (%f, %f, %f) \n", ux, uy, uz);
        return SIFT3D_FAILURE;
    }
    return SIFT3D_SUCCESS;
}

int sift3d_amd_detect_keypoints_device(sift3d_detector *d, const float *d_volume, int nx, int ny,
                                       int nz, double ux, double uy, double uz,
                                       sift3d_keypoint_store *store)
{
    if (!store || check_device_volume(d, d_volume, nx, ny, nz, ux, uy, uz) || ensure_device(d))
        return SIFT3D_FAILURE;
    return detect_on_device(d, d_volume, nx, ny, nz, ux, uy, uz, store, 0);
}

/* The Gaussian pyramid alone (max|v|, the scaling folded into the first blur, build_gpyr: sift.c:645-649,
 * 662-711) of a volume in device memory -- the part of sift3d_amd_detect_keypoints_device that BASELINE's
 * second metric ("achieved HBM GB/s on the Gauss pyramid") names, for a timed leg of its own: inside a whole
 * step the pyramid's last launches share the device with octave 0's extrema sweep.  Blocks until the levels
 * are complete; sift3d_amd_timings()[1] / [6] hold its device time, sift3d_amd_copy_level reads the levels. */
int sift3d_amd_build_pyramid_device(sift3d_detector *d, const float *d_volume, int nx, int ny, int nz,
                                    double ux, double uy, double uz)
{
    if (check_device_volume(d, d_volume, nx, ny, nz, ux, uy, uz) || ensure_device(d))
        return SIFT3D_FAILURE;
    return detect_on_device(d, d_volume, nx, ny, nz, ux, uy, uz, NULL, 1);
}

int sift3d_detect_keypoints(sift3d_detector *const d, const sift3d_image *const im, sift3d_keypoint_store *const kp)
{
    size_t n;
    if (im->nc != 1) {                                 /* sift.c:1221-1226 */
        ERR("SIFT3D_detect_keypoints: invalid number of image channels: %d -- only "
            "single-channel images are supported \n", im->nc);
        return SIFT3D_FAILURE;
    }
    if (!im->data)
        return SIFT3D_FAILURE;                         /* im_copy_data, imutil.c:653-654 */
    if (ensure_device(d))
        return SIFT3D_FAILURE;
    n = (size_t)im->nx * im->ny * im->nz;
    if (n > d->in_cap) {
        sift3d_hip_free(d->d_in);
        d->in_cap = 0;
        if (!(d->d_in = (float *)sift3d_hip_malloc(n * sizeof(float))))
            return SIFT3D_FAILURE;
        d->in_cap = n;
    }
    if (sift3d_hip_memcpy_h2d(d->d_in, im->data, n * sizeof(float), d->stream))
        return SIFT3D_FAILURE;
    return detect_on_device(d, d->d_in, im->nx, im->ny, im->nz, im->ux, im->uy, im->uz, kp, 0);
}

/* ------------------------------------------------------------------------ */
/* describe                                                                  */
/* ------------------------------------------------------------------------ */
static int key_outside(const sift3d_detector *d, const keypoint_t *k, double f)
{
    return k->xd < 0 || k->yd < 0 || k->zd < 0 || k->xd * f >= (double)d->nx || k->yd * f >= (double)d->ny ||
           k->zd * f >= (double)d->nz;
}

static int key_level_missing(const sift3d_detector *d, const keypoint_t *k)
{
    return k->o < 0 || k->o >= d->num_octaves || k->s < -1 || k->s > d->ngl - 2;
}

/* verify_keys, sift.c:1171-1212 (against the retained image dimensions), detector_has_gpyr, then the levels
 * the keypoints name.  The checks run on a few threads; the first offender (if any) is then reported in list
 * order. */
static int verify_keys(const sift3d_detector *d, const sift3d_keypoint_store *kp)
{
    const int num = (int)kp->num;
    int i, bad = 0, lvbad = 0;
    if (num < 1) {
        ERR("verify_keys: invalid number of keypoints: %d \n", num);
        return SIFT3D_FAILURE;
    }
#pragma omp parallel for num_threads(host_threads((size_t)num)) schedule(static) reduction(| : bad, lvbad)
    for (i = 0; i < num; i++) {
        const keypoint_t *k = kp->buf + i;
        const double f = k->o >= 0 && k->o < 64 ? (double)(1ull << k->o) : ldexp(1.0, k->o);
        bad |= key_outside(d, k, f) || k->sd <= 0;
        lvbad |= key_level_missing(d, k);
    }
    for (i = 0; i < num && bad; i++) {
        const keypoint_t *k = kp->buf + i;
        if (key_outside(d, k, ldexp(1.0, k->o))) {
            ERR("verify_keys: keypoint %d (%f, %f, %f) octave %d exceeds image dimensions "
                "(%d, %d, %d) \n", i, k->xd, k->yd, k->zd, k->o, d->nx, d->ny, d->nz);
            return SIFT3D_FAILURE;
        }
        if (k->sd <= 0) {
            ERR("verify_keys: keypoint %d has invalid scale %f \n", i, k->sd);
            return SIFT3D_FAILURE;
        }
    }
    if (bad)
        return SIFT3D_FAILURE;       /* (a NaN coordinate: every comparison above is false) */
    /* detector_has_gpyr, sift.c:1544-1549, 1623-1628 */
    if (!d->have_pyramid || !d->num_octaves) {
        ERR("SIFT3D_extract_descriptors: no Gaussian pyramid is available. Make sure "
            "SIFT3D_detect_keypoints was called prior to calling this function. \n");
        return SIFT3D_FAILURE;
    }
    for (i = 0; i < num && lvbad; i++) {
        const keypoint_t *k = kp->buf + i;
        if (key_level_missing(d, k)) {
            ERR("sift3d_amd: keypoint %d refers to pyramid level (%d, %d) which does not exist \n", i, k->o, k->s);
            return SIFT3D_FAILURE;
        }
    }
    return SIFT3D_SUCCESS;
}

/* k_describe queues a window voxel as its offsets in the window's box, packed into 32 bits in fields as wide
 * as the box's extents need (sift3d_describe.hip).  Every box fits when the octave-0 extents do; otherwise a
 * keypoint whose box does not fit is refused here, before any launch. */
static int check_window_packing(const sift3d_detector *d, const sift3d_keypoint_store *kp)
{
    const int num = (int)kp->num;
    int i;
    if (pack_bits(d->odims[0][0]) + pack_bits(d->odims[0][1]) + pack_bits(d->odims[0][2]) <= 32)
        return SIFT3D_SUCCESS;
    for (i = 0; i < num; i++) {
        const keypoint_t *k = kp->buf + i;
        const double rad = 14.142135624 * k->sd * (1.0 + 1e-6);       /* sift.c:1453-1454 */
        int bits = 0, a;
        for (a = 0; a < 3; a++) {
            const double lu = ldexp(d->units[a], k->o), ext = 2.0 * rad / lu + 3.0;
            const int n = d->odims[k->o][a];
            bits += pack_bits(ext < (double)n ? (long)ext : n);
        }
        if (bits > 32) {
            ERR("sift3d_amd: keypoint %d: its descriptor window (sd %f) spans more than 2^32 voxels of its "
                "box \n", i, k->sd);
            return SIFT3D_FAILURE;
        }
    }
    return SIFT3D_SUCCESS;
}

enum { DESC_LV_MAX = 32 };     /* Gaussian levels per octave that order_keypoints has buckets for */

/* the describe kernel's input list (page-locked), for num keypoints */
static int ensure_kp_list(sift3d_detector *d, int num)
{
    if (describe_list_reserve(&d->h_kp, &d->kp_cap, (uint32_t)num))
        return SIFT3D_FAILURE;
    if (d->ngl > DESC_LV_MAX) {
        ERR("sift3d_amd: at most %d Gaussian levels per octave are supported \n", DESC_LV_MAX);
        return SIFT3D_FAILURE;
    }
    return SIFT3D_SUCCESS;
}

/* 1 when the keypoint may take the lattice variant of the fast kernel (sift3d_hip_describe_lattice's contract):
 * it sits on a voxel -- the test on the float centre that the kernel would make --, carries the bits of its
 * level's sd, and the level qualifies.  What detect produces on an isotropic volume always does. */
static inline int lattice_keypoint(const sift3d_detector *d, const keypoint_t *k)
{
    const sift3d_hip_level *L = d->h_levels + (k->o * d->ngl + k->s + 1);
    const float c[3] = { (float)k->xd, (float)k->yd, (float)k->zd };
    int a;
    for (a = 0; a < 3; a++)
        if (!(c[a] >= 0.0f && c[a] < 8388608.0f && (float)(int)c[a] == c[a]))
            return 0;
    return memcmp(&k->sd, &L->sd, sizeof(double)) == 0 &&
           sift3d_hip_describe_lattice_level(L->ux, L->uy, L->uz, L->sd);
}

/* Bucket b = level (reference-order kernel), ngl + level (fast commit) or 2 * ngl + level (fast commit, lattice
 * variant): the kernel is chosen per keypoint, from its own sd (exact_desc_keypoint) and centre. */
static inline int desc_bucket(const sift3d_detector *d, const keypoint_t *k)
{
    if (exact_desc_keypoint(d->exact_desc, k->sd, k->o, d->units))
        return k->s + 1;
    return k->s + 1 + (lattice_keypoint(d, k) ? 2 : 1) * d->ngl;
}

/* Launch order: the keypoints of the reference-order kernel first, then the others, those of the lattice
 * variant last (*n_lattice of them); within each part widest windows first.  The window radius in level
 * voxels grows with the level index s only (14.14 * sigma0 * 2^(s/K)) for detect's keypoints, and a keypoint of the last level costs ~4x one of
 * the first; longest-job-first keeps the tail of the one-wave-per-keypoint kernel short.  row1 sends
 * every histogram to its keypoint's row.
 * A stable counting sort by (kernel, level) on a few threads: per-thread counts per bucket, then every
 * thread places the keypoints of its part of the list.  Fills d->h_kp; returns the number of keypoints
 * of the reference-order kernel, which lead the list. */
static size_t order_keypoints(sift3d_detector *d, const sift3d_keypoint_store *kp, size_t *n_lattice)
{
    const size_t num = kp->num;
    const int nt = host_threads(num), nlv = d->ngl;       /* s + 1 in [0, ngl) */
    size_t cnt[HOST_THREADS_MAX][3 * DESC_LV_MAX], start[HOST_THREADS_MAX][3 * DESC_LV_MAX];
    size_t n_exact = 0, lattice_first = num;
    memset(cnt, 0, sizeof(cnt));
#pragma omp parallel num_threads(nt)
    {
        const int nth = omp_get_num_threads(), t = omp_get_thread_num();  /* (nth <= nt: see compact_keypoints) */
        const size_t lo = num * t / nth, hi = num * (t + 1) / nth;
        size_t q;
        for (q = lo; q < hi; q++)
            cnt[t][desc_bucket(d, kp->buf + q)]++;
#pragma omp barrier
#pragma omp single
        {
            size_t pos = 0;
            int b, u;
            for (b = 0; b < 3 * nlv; b++) {
                /* levels descending in each part */
                const int bk = b < nlv ? nlv - 1 - b : b < 2 * nlv ? 3 * nlv - 1 - b : 5 * nlv - 1 - b;
                if (b == nlv)
                    n_exact = pos;         /* (the exact ones lead the list) */
                if (b == 2 * nlv)
                    lattice_first = pos;
                for (u = 0; u < nth; u++) {
                    start[u][bk] = pos;
                    pos += cnt[u][bk];
                }
            }
        }
        /* (implicit barrier) */
        for (q = lo; q < hi; q++) {
            const keypoint_t *k = kp->buf + q;
            describe_record(d->h_kp + start[t][desc_bucket(d, k)]++, k, d->ngl, q);
        }
    }
    *n_lattice = num - lattice_first;
    return n_exact;
}

/* do_extract_descriptors, sift.c:1561-1596: the store sized for num descriptors of the detector's image */
static int ensure_descriptor_store(const sift3d_detector *d, sift3d_descriptor_store *desc, size_t num)
{
    if (desc_store_reserve(desc, num, d->odims[0][0], d->odims[0][1], d->odims[0][2]))
        return SIFT3D_FAILURE;
    if (desc->keep_device && num > desc->d_cap) {
        sift3d_hip_free(desc->d_hist);
        desc->d_cap = 0;
        desc->d_hist = (float *)sift3d_hip_malloc(sizeof(float) * DESC_NUMEL * desc->cap);
        if (!desc->d_hist)
            return SIFT3D_FAILURE;
        desc->d_cap = desc->cap;
    }
    return SIFT3D_SUCCESS;
}

int sift3d_extract_descriptors(sift3d_detector *const d, const sift3d_keypoint_store *const kp,
                               sift3d_descriptor_store *const desc)
{
    const int num = (int)kp->num;
    const double t_start = now_s();
    size_t n_exact, n_lattice;
    uint64_t rng;

    if (verify_keys(d, kp) || check_window_packing(d, kp) || ensure_kp_list(d, num))
        return SIFT3D_FAILURE;
    n_exact = order_keypoints(d, kp, &n_lattice);
    if (ensure_descriptor_store(d, desc, (size_t)num))
        return SIFT3D_FAILURE;
    d->t_pending &= ~2;
    rng = range_start("sift3d: descriptors");
    sift3d_hip_event_record(d->ev[6], d->stream);
    if (describe_enqueue(d->d_levels, d->h_levels, d->num_octaves * d->ngl, d->h_kp, (uint32_t)num,
                         (uint32_t)n_exact, (uint32_t)n_lattice, desc, desc->keep_device ? desc->d_hist : NULL,
                         d->d_wlut, &d->d_dpart, &d->dpart_bytes, d->stream))
        return SIFT3D_FAILURE;
    sift3d_hip_event_record(d->ev[7], d->stream);
    desc_store_fill_xyzsd(desc, kp->buf, NULL, 0, (size_t)num);      /* (beside the kernel) */
    if (sift3d_hip_stream_sync(d->stream))
        return SIFT3D_FAILURE;
    range_stop(rng);
    if (desc->keep_device)
        desc->d_num = (size_t)num;
    d->t_pending |= 2;
    d->t[T_DESCRIBE_WALL] = now_s() - t_start;
    return SIFT3D_SUCCESS;
}
