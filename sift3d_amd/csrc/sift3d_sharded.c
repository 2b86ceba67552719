/* sift3d_sharded.c -- Z-slab multi-GPU detect + describe, host side in C (included at the end of
 * sift3d_host.c: it uses the private store layouts).
 *
 * One process per GPU; the volume is cut along z into one slab per rank.  Everything that is
 * local in z runs unchanged on the slab (x / y FIR passes, dogmax, extrema, down-sampling on
 * 2^k-aligned slab boundaries); exactly three kinds of exchange cross ranks, all through a small
 * transport vtable (sift3d_amd_transport: RCCL send/recv, all-reduce, all-gather over xGMI in
 * production -- sift3d_amd_rccl_transport below -- or anything a test provides):
 *
 *   halo      nearest-neighbour exchange of z planes: the input of every z FIR pass
 *             (ceil(hw * unit_factor) + 1 planes per side), and after the pyramid the planes the
 *             orientation / descriptor windows of this rank's keypoints reach into;
 *   max       all-reduce(max) of max|input| (im_scale, imutil.c:699-713) and of the per-level
 *             max|DoG| (sift.c:821-826) -- order-free, hence exact;
 *   gather    all-gather of the per-level candidate counts, the candidates' |DoG| values and the
 *             ORIENTED keypoints (rejected candidates never leave their rank).
 *
 * The ORDER in which one detect call issues them is the invariant every rank keeps, whatever fails
 * locally (SH_DO / SH_COMM below).  sift3d_amd_sharded_detect is the list of the stages that issue
 * them; DESIGN.md section 5, "The exchanges of one detect call, in order", is the list itself.
 *
 * Ranks are concatenated in slab order inside each (octave, level), which reproduces the
 * reference's global (o, s, z, y, x) order and its stale-strength quirk (sift.c:372-384), so the
 * result equals the single-GPU result bit for bit (tests/test_gpu_sharded.py).  Mirror rules
 * apply at the GLOBAL faces only: the stage kernels take the global length and the slab offset.
 * Octaves whose slabs would be thinner than the window halo are all-gathered and computed on
 * every rank (< 1 % of the voxels); their window work is still split by z.
 *
 * The z-halo exchange of a blur overlaps with the z pass of the slab's interior planes: the
 * exchange is enqueued on a second stream as soon as the x pass has finished, the interior planes
 * (which need no halo) are filtered meanwhile, the 2 * reach boundary planes afterwards.
 *
 * Scope: everything the drop-in API accepts -- any number of keypoint levels per octave
 * (sift.c:527-533), the cuboid extrema neighbourhood (sift.c:24, 761-796), any volume size (the
 * reference halves dimensions with integer division, imutil.c:1545-1547, so rows that are not
 * whole quads are a normal case).  Octaves the DoG-free extrema sweep does not cover store their
 * DoG levels and take sift3d_hip_extrema_mode, exactly as the single-GPU path does
 * (sift3d_detect.c: detect_on_device).  tests/sharded_py.py is the same orchestration in Python on a
 * pluggable compute backend: test infrastructure for the gloo runs on the CPU oracle. */

#include <dlfcn.h>

#define SH_MAX_K 8                  /* keypoint levels per octave (as sift3d_host.c) */
#define SH_MAX_NGL (SH_MAX_K + 3)
#define SH_MAX_NDL (SH_MAX_K + 2)
#define SH_MAX_OCT 32
#define SH_MAX_WORLD 64

typedef struct {
    float *t;           /* device planes [off, off + nloc) of the level */
    int off, nloc;      /* local buffer */
    int z0, z1;         /* owned (or, on replicated octaves, work-split) planes, global */
    int nz_glob;
} sh_level;

struct sift3d_amd_sharded {
    sift3d_amd_transport T;
    int rank, world;
    double peak_thresh, corner_thresh, sigma_n, sigma0;
    double units[3];
    int nx, ny, nz;
    /* geometry */
    int num_octaves, o_shard, halo;
    int dims[SH_MAX_OCT][3];
    int b0[SH_MAX_WORLD + 1];
    int bounds[SH_MAX_OCT][SH_MAX_WORLD + 1];
    int K, ngl, ndl;                 /* keypoint / Gaussian / DoG levels per octave */
    int cuboid;
    int exact_desc;                  /* sift3d_amd_detector_set_exact_descriptors of `params` */
    int dog_free[SH_MAX_OCT];        /* octave takes the DoG-free sweep (no stored DoG levels) */
    int win_reach[SH_MAX_NGL];
    filter_t filt[SH_MAX_NGL];
    /* device state */
    /* The pyramid's three dependency chains, as in the single-GPU path (detect_on_device): [0] octave 0,
     * [1] the first levels of the octaves >= 1 (their down-sampling source included), [2] their last
     * levels, which nothing but their own DoG waits for.  A chain has its stream, its scratch volumes and
     * its pair of events around the z-halo exchange (which always travels on comm_stream).  The extrema
     * sweeps of the octaves >= 1 run on chain 1's stream beside octave 0's. */
    struct sh_chain {
        void *stream;
        float *tmp_a, *tmp_b;
        void *ev_x, *ev_halo;
    } chain[3];
    void *stream;                    /* = chain[0].stream, the main stream: every collective but the halos */
    void *comm_stream;
    void *ev[5];                     /* the marks between the stages that t[] is read from (sh_end) */
    void *ev_fork, *ev_join, *ev_join2, *ev_tr, *ev_oct[SH_MAX_OCT];
    void *d_work2;                          /* work areas of the side sweeps, kept until the ordered emission */
    size_t work2_off[SH_MAX_OCT], work2_sz[SH_MAX_OCT], work2_bytes;
    sh_level G[SH_MAX_OCT][SH_MAX_NGL];
    float *D[SH_MAX_OCT][SH_MAX_NDL];   /* stored DoG levels (geometry of G[o][*]), where needed */
    float *d_im, *d_raw, *d_stage;
    size_t stage_elems;
    int in_z0, in_z1;
    float *d_scalars;                /* [0] input max, [1] candidate count, [8 + ndl o + k] dogmax */
    sift3d_hip_level h_levels[SH_MAX_OCT * SH_MAX_NGL], *d_levels;
    void *d_work;
    size_t work_bytes;
    float *d_wlut;
    void *d_dpart;         /* scratch of the descriptor kernel's split windows */
    size_t dpart_bytes;
    void *d_otab;          /* orientation window tables + candidate sums (sift3d_hip_orient_tab) */
    size_t otab_bytes;
    sift3d_hip_cand *d_cand;
    float *d_R;
    int32_t *d_keep;
    uint32_t cand_cap;
    uint32_t cand_cap0;              /* capacity the next detect starts from while none is allocated (0: 2^18) */
    void *d_xchg, *h_xchg;           /* the ranks' gathered blocks (device); the final list (pinned host) */
    size_t xchg_bytes, hxchg_cap;
    void *d_cnt, *h_cnt, *d_tab, *h_tab, *d_out, *d_pack;   /* counts, segment tables, list, scan scratch */
    size_t cnt_cap, hcnt_cap, tab_cap, htab_cap, out_cap, pack_cap;
    void *d_gath;                    /* descriptor gather staging (sift3d_amd_sharded_gather_descriptors) */
    size_t gath_cap;
    int failed, inject;              /* local failure mark of the running call; test hook */
    sift3d_hip_kp *h_kp;
    uint32_t kp_cap;
    int ncand;
    /* [0] pyramid (device s)  [1] detect wall  [2] describe wall  [3] DoG maxima + extrema (device s,
     * incl. the all-reduce)  [4] wait for the window halos + orientation (device s)  [5] gathers +
     * global list (host s)  [6] input scaling (device s, incl. the all-reduce) */
    double t[8];
    double t_gather0;
};

static int sh_sharded(const sift3d_amd_sharded *S, int o) { return o < S->o_shard; }

static double sh_scale(const sift3d_amd_sharded *S, int o, int s)
{
    return S->sigma0 * pow(2.0, o + (double)s / S->K);           /* imutil.c:1578-1579 */
}

static size_t sh_plane(const sift3d_amd_sharded *S, int o) { return (size_t)S->dims[o][0] * S->dims[o][1]; }

/* ---- what the stages ask of the driver's arrays (d_scalars: laid out as the struct says) ---- */
static inline float *sh_dogmax_slot(const sift3d_amd_sharded *S, int o) { return S->d_scalars + 8 + S->ndl * o; }
static inline uint32_t *sh_cand_counter(const sift3d_amd_sharded *S) { return (uint32_t *)(S->d_scalars + 1); }
/* the capacity of the candidate arrays, or the one the next detect starts from */
static inline uint32_t sh_cand_capacity(const sift3d_amd_sharded *S)
{
    return S->cand_cap ? S->cand_cap : S->cand_cap0 ? S->cand_cap0 : (1u << 18);
}
/* the planes [*lo, *hi) of octave o's level buffers that this rank owns (replicated octaves: all of them) */
static inline void sh_owned(const sift3d_amd_sharded *S, int o, int *lo, int *hi)
{
    const sh_level *L = &S->G[o][0];
    *lo = sh_sharded(S, o) ? L->z0 - L->off : 0;
    *hi = sh_sharded(S, o) ? L->z1 - L->off : L->nloc;
}
/* the Gaussian levels of octave o from plane `first` of their buffers on */
static inline void sh_level_ptrs(const sift3d_amd_sharded *S, int o, int first, const float **g)
{
    int s;
    for (s = 0; s < S->ngl; s++)
        g[s] = S->G[o][s].t + (size_t)first * sh_plane(S, o);
}
/* the extrema work area of octave o (side: the sweeps run side by side and those of the octaves >= 1 keep theirs
 * between the two phases) */
static inline void *sh_extrema_work(const sift3d_amd_sharded *S, int o, int side, size_t *bytes)
{
    *bytes = side && o > 0 ? S->work2_sz[o] : S->work_bytes;
    return side && o > 0 ? (void *)((char *)S->d_work2 + S->work2_off[o]) : S->d_work;
}
/* The rank that owns keypoint k -- describes it, and sends its row in the descriptor gather: the one whose
 * planes of octave k->o hold k->zd (bounds ascend; what lies outside the volume goes to the first or last rank).
 * One rank: 0. */
static inline int sh_owner(const sift3d_amd_sharded *S, const keypoint_t *k)
{
    int r = 0;
    while (r < S->world - 1 && !(k->zd < (double)S->bounds[k->o][r + 1]))
        r++;
    return r;
}
/* the slabs zb[0 .. world] in which the first replicated octave t leaves the ranks' down-sampling; returns the
 * planes of the largest (at least 1) */
static int sh_transition_slabs(const sift3d_amd_sharded *S, int t, int *zb)
{
    const int mzg = S->dims[t][2];
    int r, mxn = 1;
    for (r = 0; r < S->world; r++)
        zb[r] = (S->b0[r] >> t) < mzg ? (S->b0[r] >> t) : mzg;
    zb[S->world] = mzg;
    for (r = 0; r < S->world; r++)
        if (zb[r + 1] - zb[r] > mxn)
            mxn = zb[r + 1] - zb[r];
    return mxn;
}

/* ---- geometry ------------------------------------------------------------------------------ */
static int sh_geometry(sift3d_amd_sharded *S)
{
    int mn = S->nx < S->ny ? S->nx : S->ny, last, o, r, d[3], align, min_slab;
    mn = mn < S->nz ? mn : S->nz;
    last = (int)log2((double)mn) - 3;                              /* sift.c:442-444 */
    if (last < 0) {
        ERR("resize_SIFT3D: input image is too small: must have at least 8 voxels in each "
            "dimension \n");
        return SIFT3D_FAILURE;
    }
    S->num_octaves = last + 1;
    if (S->num_octaves > SH_MAX_OCT)
        return SIFT3D_FAILURE;
    d[0] = S->nx; d[1] = S->ny; d[2] = S->nz;
    for (o = 0; o < S->num_octaves; o++) {
        memcpy(S->dims[o], d, sizeof(d));
        d[0] /= 2; d[1] /= 2; d[2] /= 2;                           /* imutil.c:1545-1547 */
    }
    min_slab = S->halo + 8;
    S->o_shard = 0;
    if (S->world > 1)
        while (S->o_shard < S->num_octaves && S->dims[S->o_shard][2] / S->world >= min_slab)
            S->o_shard++;
    /* slab bounds at octave 0: multiples of 2^o_shard, so that every slab boundary is even in
     * every sharded octave and im_downsample_2x never needs a neighbour's plane */
    align = 1 << S->o_shard;
    S->b0[0] = 0;
    for (r = 1; r < S->world; r++)
        S->b0[r] = (int)nearbyint((double)S->nz * r / S->world / align) * align;
    S->b0[S->world] = S->nz;
    for (o = 0; o < S->num_octaves; o++) {
        const int nzo = S->dims[o][2];
        for (r = 0; r < S->world; r++)
            S->bounds[o][r] = sh_sharded(S, o) ? ((S->b0[r] >> o) < nzo ? (S->b0[r] >> o) : nzo)
                                                 : (int)((long)nzo * r / S->world);
        S->bounds[o][S->world] = nzo;
    }
    return SIFT3D_SUCCESS;
}

/* ---- the driver's resources ------------------------------------------------------------------ */
/* what every stream of the driver holds has ended */
static int sh_sync_streams(const sift3d_amd_sharded *S)
{
    void *const st[4] = { S->stream, S->comm_stream, S->chain[1].stream, S->chain[2].stream };
    int i, rc = SIFT3D_SUCCESS;
    for (i = 0; i < 4; i++)
        if (st[i] && sift3d_hip_stream_sync(st[i]))
            rc = SIFT3D_FAILURE;
    return rc;
}

static void sh_free_cand(sift3d_amd_sharded *S)
{
    sift3d_hip_free(S->d_cand); sift3d_hip_free(S->d_R); sift3d_hip_free(S->d_keep);
    S->d_cand = NULL; S->d_R = NULL; S->d_keep = NULL;
    S->cand_cap = 0;
}

void sift3d_amd_sharded_free(sift3d_amd_sharded *S)
{
    int o, s, i;
    if (!S)
        return;
    sh_sync_streams(S);
    for (o = 0; o < SH_MAX_OCT; o++) {
        for (s = 0; s < SH_MAX_NGL; s++)
            sift3d_hip_free(S->G[o][s].t);
        for (s = 0; s < SH_MAX_NDL; s++)
            sift3d_hip_free(S->D[o][s]);
        sift3d_hip_event_destroy(S->ev_oct[o]);
    }
    for (s = 0; s < SH_MAX_NGL; s++)
        free(S->filt[s].taps);
    sh_free_cand(S);
    sift3d_hip_free(S->d_im); sift3d_hip_free(S->d_raw); sift3d_hip_free(S->d_stage); sift3d_hip_free(S->d_scalars);
    sift3d_hip_free(S->d_levels); sift3d_hip_free(S->d_work); sift3d_hip_free(S->d_work2); sift3d_hip_free(S->d_xchg);
    sift3d_hip_free(S->d_wlut); sift3d_hip_free(S->d_otab); sift3d_hip_free(S->d_dpart); sift3d_hip_free(S->d_cnt);
    sift3d_hip_free(S->d_tab); sift3d_hip_free(S->d_out); sift3d_hip_free(S->d_pack); sift3d_hip_free(S->d_gath);
    sift3d_hip_host_free(S->h_xchg); sift3d_hip_host_free(S->h_kp);
    sift3d_hip_host_free(S->h_cnt); sift3d_hip_host_free(S->h_tab);
    sift3d_hip_event_destroy(S->ev_fork); sift3d_hip_event_destroy(S->ev_join);
    sift3d_hip_event_destroy(S->ev_join2); sift3d_hip_event_destroy(S->ev_tr);
    for (i = 0; i < 5; i++)
        sift3d_hip_event_destroy(S->ev[i]);
    for (i = 2; i >= 0; i--) {
        struct sh_chain *C = &S->chain[i];
        sift3d_hip_free(C->tmp_a); sift3d_hip_free(C->tmp_b);
        sift3d_hip_event_destroy(C->ev_x); sift3d_hip_event_destroy(C->ev_halo);
        if (i == 0)
            sift3d_hip_stream_destroy(S->comm_stream);
        sift3d_hip_stream_destroy(C->stream);
    }
    free(S);
}

/* the streams and events (the streams in this order: main, communication, the two side chains) */
static int sh_create_streams(sift3d_amd_sharded *S)
{
    void **const ev[4] = { &S->ev_fork, &S->ev_join, &S->ev_join2, &S->ev_tr };
    int i, o;
    S->stream = S->chain[0].stream = sift3d_hip_stream_create();
    S->comm_stream = sift3d_hip_stream_create();
    S->chain[1].stream = sift3d_hip_stream_create_high();
    S->chain[2].stream = sift3d_hip_stream_create_high();
    if (!S->stream || !S->comm_stream || !S->chain[1].stream || !S->chain[2].stream)
        return SIFT3D_FAILURE;
    for (i = 0; i < 3; i++)
        if (!(S->chain[i].ev_x = sift3d_hip_event_create()) || !(S->chain[i].ev_halo = sift3d_hip_event_create()))
            return SIFT3D_FAILURE;
    for (i = 0; i < 5; i++)
        if (!(S->ev[i] = sift3d_hip_event_create()))
            return SIFT3D_FAILURE;
    for (i = 0; i < 4; i++)
        if (!(*ev[i] = sift3d_hip_event_create()))
            return SIFT3D_FAILURE;
    for (o = 0; o < S->num_octaves; o++)
        if (!(S->ev_oct[o] = sift3d_hip_event_create()))
            return SIFT3D_FAILURE;
    return SIFT3D_SUCCESS;
}

/* the Gaussian levels (and, where the DoG-free sweep does not apply, the DoG levels) of every octave: the owned
 * planes and the halo around them; with them the sizes of the extrema work areas */
static int sh_alloc_levels(sift3d_amd_sharded *S)
{
    int o, s;
    for (o = 0; o < S->num_octaves; o++) {
        const int nzo = S->dims[o][2];
        const int z0 = S->bounds[o][S->rank], z1 = S->bounds[o][S->rank + 1];
        const int off = sh_sharded(S, o) ? (z0 - S->halo > 0 ? z0 - S->halo : 0) : 0;
        const int hi = sh_sharded(S, o) ? (z1 + S->halo < nzo ? z1 + S->halo : nzo) : nzo;
        const size_t bytes = sh_plane(S, o) * (size_t)(hi - off) * sizeof(float);
        const size_t w = sift3d_hip_extrema_work_bytes(S->dims[o][0], S->dims[o][1], hi - off, S->K);
        S->work_bytes = w > S->work_bytes ? w : S->work_bytes;
        if (o >= 1) {
            S->work2_off[o] = S->work2_bytes;
            S->work2_sz[o] = w;
            S->work2_bytes += (w + 255) & ~(size_t)255;
        }
        /* (all levels of an octave share one geometry -- the fused sweeps take them as a stack; only
         * the keypoint levels 1..K USE the full window halo, the others a blur's or the extrema
         * test's reach) */
        for (s = 0; s < S->ngl; s++) {
            sh_level *L = &S->G[o][s];
            L->off = off; L->nloc = hi - off; L->z0 = z0; L->z1 = z1; L->nz_glob = nzo;
            if (!(L->t = (float *)sift3d_hip_malloc(bytes)))
                return SIFT3D_FAILURE;
        }
        for (s = 0; s < S->ndl && !S->dog_free[o]; s++)
            if (!(S->D[o][s] = (float *)sift3d_hip_malloc(bytes)))
                return SIFT3D_FAILURE;
    }
    return SIFT3D_SUCCESS;
}

/* the chains' scratch volumes, the input slab, the transition's staging, scalars, tables and work areas */
static int sh_alloc_scratch(sift3d_amd_sharded *S)
{
    const size_t n0 = sh_plane(S, 0) * (size_t)S->G[0][0].nloc;
    const size_t n1 = S->num_octaves > 1 ? sh_plane(S, 1) * (size_t)S->G[1][0].nloc : 4;
    int zb[SH_MAX_WORLD + 1], i;
    for (i = 0; i < 3; i++) {
        struct sh_chain *C = &S->chain[i];
        C->tmp_a = (float *)sift3d_hip_malloc((i ? n1 : n0) * sizeof(float));
        C->tmp_b = (float *)sift3d_hip_malloc((i ? n1 : n0) * sizeof(float));
        if (!C->tmp_a || !C->tmp_b)
            return SIFT3D_FAILURE;
    }
    S->in_z0 = sh_sharded(S, 0) ? S->bounds[0][S->rank] : 0;
    S->in_z1 = sh_sharded(S, 0) ? S->bounds[0][S->rank + 1] : S->nz;
    S->d_im = (float *)sift3d_hip_malloc(n0 * sizeof(float));
    S->d_raw = (float *)sift3d_hip_malloc(sh_plane(S, 0) * (size_t)(S->in_z1 - S->in_z0) * sizeof(float));
    /* staging of the sharded -> replicated transition: this rank's down-sampled slab, then the
     * world slabs gathered (all padded to the largest) */
    S->stage_elems = 16;
    if (S->world > 1 && S->o_shard >= 1 && S->o_shard < S->num_octaves)
        S->stage_elems = (size_t)sh_transition_slabs(S, S->o_shard, zb) * sh_plane(S, S->o_shard) *
                         (size_t)(S->world + 1);
    S->d_stage = (float *)sift3d_hip_malloc(S->stage_elems * sizeof(float));
    S->d_scalars = (float *)sift3d_hip_malloc(sizeof(float) * (8 + SH_MAX_NDL * SH_MAX_OCT));
    S->d_levels = (sift3d_hip_level *)sift3d_hip_malloc(sizeof(sift3d_hip_level) * SH_MAX_OCT * SH_MAX_NGL);
    S->d_work = sift3d_hip_malloc(S->work_bytes);
    if (S->work2_bytes && !(S->d_work2 = sift3d_hip_malloc(S->work2_bytes)))
        return SIFT3D_FAILURE;
    S->d_wlut = (float *)sift3d_hip_malloc(sizeof(float) *
                                           sift3d_hip_describe_wlut_floats(S->num_octaves * S->ngl));
    return S->d_wlut && S->d_im && S->d_raw && S->d_stage && S->d_scalars && S->d_levels && S->d_work
               ? SIFT3D_SUCCESS : SIFT3D_FAILURE;
}

/* level table (window kernels), on the host and on the device */
static int sh_level_table(sift3d_amd_sharded *S)
{
    int o, s;
    for (o = 0; o < S->num_octaves; o++)
        for (s = 0; s < S->ngl; s++) {
            sift3d_hip_level *L = &S->h_levels[o * S->ngl + s];
            L->data = S->G[o][s].t;
            L->nx = S->dims[o][0]; L->ny = S->dims[o][1]; L->nz = S->G[o][s].nloc;
            L->z_off = S->G[o][s].off;
            L->nz_glob = S->dims[o][2];
            L->ux = (float)(S->units[0] * ldexp(1.0, o));
            L->uy = (float)(S->units[1] * ldexp(1.0, o));
            L->uz = (float)(S->units[2] * ldexp(1.0, o));
            L->octave = o;
            L->sd = sh_scale(S, o, s - 1);
        }
    return sift3d_hip_memcpy_h2d(S->d_levels, S->h_levels, sizeof(sift3d_hip_level) * (size_t)S->num_octaves * S->ngl,
                                 S->stream) ||
           sift3d_hip_stream_sync(S->stream);
}

sift3d_amd_sharded *sift3d_amd_sharded_create(int nx, int ny, int nz, const sift3d_amd_transport *T,
                                              const sift3d_detector *params, double ux, double uy,
                                              double uz)
{
    sift3d_amd_sharded *S;
    int o, s, i, hw_max = 0, blur_reach;
    if (!T || T->world < 1 || T->world > SH_MAX_WORLD || T->rank < 0 || T->rank >= T->world ||
        nx < 8 || ny < 8 || nz < 8 || !(ux > 0) || !(uy > 0) || !(uz > 0))
        return NULL;
    if (T->world > 1 && (!T->halo || !T->allreduce_max || !T->allgather))
        return NULL;
    if (!sift3d_amd_device_available()) {
        ERR("sift3d_amd: no HIP device is available; this library has no CPU path \n");
        return NULL;
    }
    if (params && (params->num_kp_levels < 1 || params->num_kp_levels > SH_MAX_K)) {
        ERR("sift3d_amd_sharded: 1 to %d keypoint levels per octave are supported \n", SH_MAX_K);
        return NULL;
    }
    S = (sift3d_amd_sharded *)calloc(1, sizeof(*S));
    if (!S)
        return NULL;
    S->K = params ? params->num_kp_levels : 3;
    S->ngl = S->K + 3;                                             /* sift.c:434-437 */
    S->ndl = S->K + 2;
    S->cuboid = params ? params->cuboid_extrema : 0;
    S->exact_desc = params ? params->exact_desc : 0;
    S->T = *T;
    S->rank = T->rank; S->world = T->world;
    S->peak_thresh = params ? params->peak_thresh : peak_thresh_default;
    S->corner_thresh = params ? params->corner_thresh : corner_thresh_default;
    S->sigma_n = params ? params->sigma_n : sigma_n_default;
    S->sigma0 = params ? params->sigma0 : sigma0_default;
    S->units[0] = ux; S->units[1] = uy; S->units[2] = uz;
    S->nx = nx; S->ny = ny; S->nz = nz;
    if (S->sigma0 * pow(2.0, -1.0 / S->K) < S->sigma_n) {          /* imutil.c:1582-1588 */
        ERR("set_scales_Pyramid: sigma_n too large for these settings. \n");
        goto fail;
    }
    /* filter bank (make_gss, imutil.c:1360-1409) */
    for (i = 0; i < S->ngl; i++) {
        const double s_cur = i == 0 ? S->sigma_n : S->sigma0 * pow(2.0, (double)(i - 2) / S->K);
        const double s_next = S->sigma0 * pow(2.0, (double)(i - 1) / S->K);
        if (gauss_filter(&S->filt[i], sqrt(s_next * s_next - s_cur * s_cur)))
            goto fail;
        if (S->filt[i].width / 2 > hw_max)
            hw_max = S->filt[i].width / 2;
    }
    /* halo planes a slab needs from its neighbours, in LEVEL planes (the same in every octave):
     * descriptor window of Gaussian level s: 14.1422 * sigma0 * 2^((s-1)/K) / uz + 2
     * (sift.c:1453-1454); z pass: ceil(hw * unit_factor) + 1 (imutil.c:756-757) */
    for (s = 0; s < S->ngl; s++)
        S->win_reach[s] = (s >= 1 && s <= S->K)
                              ? (int)ceil(14.1422 * S->sigma0 * pow(2.0, (double)(s - 1) / S->K) / uz) + 2
                              : 1;
    blur_reach = (int)ceil((double)hw_max * (double)(float)(1.0 / uz)) + 1;
    S->halo = blur_reach;
    for (s = 0; s < S->ngl; s++)
        if (S->win_reach[s] > S->halo)
            S->halo = S->win_reach[s];
    if (S->halo > 500) {
        ERR("sift3d_amd_sharded: sigma0 / units give a %d-plane window \n", S->halo);
        goto fail;
    }
    if (sh_geometry(S))
        goto fail;
    /* the DoG-free sweep covers the default level count and 8-neighbour test on rows of whole quads
     * (sift3d_hip_dogmax_stack / sift3d_hip_extrema_gauss6); other octaves store their DoG levels */
    for (o = 0; o < S->num_octaves; o++)
        S->dog_free[o] = !S->cuboid && S->ngl == 6 && (S->dims[o][0] & 3) == 0;
    if (sh_create_streams(S) || upload_mesh() || sh_alloc_levels(S) || sh_alloc_scratch(S) || sh_level_table(S))
        goto fail;
    return S;
fail:
    sift3d_amd_sharded_free(S);
    return NULL;
}

int sift3d_amd_sharded_own_planes(const sift3d_amd_sharded *S, int *z0, int *z1)
{
    if (!S)
        return SIFT3D_FAILURE;
    if (z0) *z0 = S->in_z0;
    if (z1) *z1 = S->in_z1;
    return SIFT3D_SUCCESS;
}

float *sift3d_amd_sharded_input(sift3d_amd_sharded *S) { return S ? S->d_raw : NULL; }

int sift3d_amd_sharded_synth(sift3d_amd_sharded *S, uint64_t seed)
{
    if (!S)
        return SIFT3D_FAILURE;
    if (sift3d_hip_synth_lattice(S->d_raw, S->nx, S->ny, S->in_z1 - S->in_z0, S->in_z0, seed, S->stream))
        return SIFT3D_FAILURE;
    return sift3d_hip_stream_sync(S->stream);
}

int sift3d_amd_sharded_num_candidates(const sift3d_amd_sharded *S) { return S ? S->ncand : -1; }
const double *sift3d_amd_sharded_timings(const sift3d_amd_sharded *S) { return S ? S->t : NULL; }
int sift3d_amd_sharded_info(const sift3d_amd_sharded *S, int *num_octaves, int *o_shard, int *halo)
{
    if (!S)
        return SIFT3D_FAILURE;
    if (num_octaves) *num_octaves = S->num_octaves;
    if (o_shard) *o_shard = S->o_shard;
    if (halo) *halo = S->halo;
    return SIFT3D_SUCCESS;
}

/* ---- exchanges ------------------------------------------------------------------------------ */
/* Fill halo planes on both sides of the owned range of a level buffer (plane stride `plane`,
 * geometry of `L`) from the slab neighbours, on `stream`: the planes at distance (d0, h] from the
 * slab boundary (d0 = 0: all h of them). */
static int sh_halo_range(sift3d_amd_sharded *S, float *t, const sh_level *L, size_t plane, int d0, int h,
                         void *stream)
{
    const int a = L->z0 - L->off, b = L->z1 - L->off;
    const int lo = S->rank > 0 && L->z0 > 0, hi = S->rank < S->world - 1 && L->z1 < L->nz_glob;
    if (S->world == 1 || h <= d0 || (!lo && !hi))
        return SIFT3D_SUCCESS;
    if (h > S->halo || h > b - a || d0 < 0) {
        ERR("sift3d_amd_sharded: a %d-plane halo does not fit slabs of %d planes \n", h, b - a);
        return SIFT3D_FAILURE;
    }
    return S->T.halo(S->T.ctx, lo ? t + (size_t)(a + d0) * plane : NULL, lo ? t + (size_t)(a - h) * plane : NULL,
                     hi ? t + (size_t)(b - h) * plane : NULL, hi ? t + (size_t)(b + d0) * plane : NULL,
                     (size_t)(h - d0) * plane * sizeof(float), stream);
}

/* one FIR pass along `axis` over planes [z_lo, z_hi) of a level buffer of octave o (nloc planes from global
 * plane `off`) */
static sift3d_hip_fir_args sh_fir_args(const sift3d_amd_sharded *S, const float *src, float *dst, int o, int nloc,
                                       int axis, const filter_t *f, float uf, int off, int z_lo, int z_hi)
{
    sift3d_hip_fir_args a;
    memset(&a, 0, sizeof(a));
    a.src = src; a.dst = dst;
    a.nx = S->dims[o][0]; a.ny = S->dims[o][1]; a.nz = nloc;
    a.axis = axis; a.width = f->width; a.taps = f->taps;
    a.unit_factor = uf;
    a.n_glob = S->dims[o][2]; a.off = off;
    a.z_lo = z_lo; a.z_hi = z_hi;
    return a;
}

static int sh_fir(sift3d_amd_sharded *S, const float *src, float *dst, int o, int nloc, int axis,
                  const filter_t *f, float uf, int off, int z_lo, int z_hi, void *stream)
{
    const sift3d_hip_fir_args a = sh_fir_args(S, src, dst, o, nloc, axis, f, uf, off, z_lo, z_hi);
    return sift3d_hip_fir(&a, stream);
}

/* ---- failures between collectives ------------------------------------------------------------- */
/* detect and describe are collective.  A rank whose LOCAL work fails (a launch, an allocation, an injected
 * test failure) must not leave the others waiting in the next exchange: it marks itself failed, skips its
 * remaining local work and still issues every exchange in the common order (with whatever its buffers hold);
 * its status word travels behind the first all-gather of the step (the counts) and behind the second (the
 * records), and EVERY rank returns SIFT3D_FAILURE at the same point, with the transport in step for the next
 * call -- the reference's "every stage returns -1 to its caller" (immacros.h:27-32), across ranks.  A
 * failure of the transport itself is everybody's by nature and returns at once.
 *
 * The contract of every stage of sift3d_amd_sharded_detect (and of sh_blur below them):
 *   - it returns non-zero only for what is everybody's failure -- a transport error (SH_COMM), or a condition
 *     that every rank computes alike (the geometry, the gathered counts, the status words) -- and the caller
 *     returns at once (sh_begin also refuses, before anything is issued, arguments no call can run with);
 *   - a local failure only marks S->failed (SH_DO), and the stage still issues its exchanges;
 *   - the exception: the exchange buffers themselves (sh_exchange_counts, sh_exchange_records).  Where they
 *     cannot be allocated there is nothing to send in, and the stage returns;
 *   - local work is guarded by !S->failed, the candidate count or an owned range that is not empty; an exchange
 *     by nothing but the geometry. */
#define SH_DO(call)                                        \
    do {                                                   \
        if (!S->failed && (call))                          \
            S->failed = __LINE__;                          \
    } while (0)
#define SH_COMM(call)                                      \
    do {                                                   \
        if (call)                                          \
            return SIFT3D_FAILURE;                         \
    } while (0)

/* the failing rank's own line of a call that fails on every rank */
static void sh_report_local_failure(const sift3d_amd_sharded *S)
{
    if (S->failed)
        ERR("sift3d_amd_sharded_detect: rank %d failed locally (mark %d) \n", S->rank, S->failed);
}

/* test hook: the next detect (where = 1: before the pyramid, 2: after the extrema, 3: between the two
 * all-gathers) or describe-gather (4) of THIS rank fails locally */
int sift3d_amd_sharded_inject_failure(sift3d_amd_sharded *S, int where)
{
    if (!S || where < 0 || where > 4)
        return SIFT3D_FAILURE;
    S->inject = where;
    return SIFT3D_SUCCESS;
}

/* this rank's candidate arrays: released, the next detect starts from `cap` (0: 2^18); grown by a detect
 * that overflows them */
int sift3d_amd_sharded_set_candidate_capacity(sift3d_amd_sharded *S, int cap)
{
    if (!S || cap < 0 || sh_sync_streams(S))
        return SIFT3D_FAILURE;
    sh_free_cand(S);
    S->cand_cap0 = (uint32_t)cap;
    return SIFT3D_SUCCESS;
}

int sift3d_amd_sharded_candidate_capacity(const sift3d_amd_sharded *S)
{
    return S ? (int)sh_cand_capacity(S) : -1;
}

/* apply_Sep_FIR_filter (imutil.c:1127-1206) on level s of octave o: src -> G[o][s], with filter s.  Sharded
 * octaves: x (and y) on the owned planes, halo exchange of the z pass's input (on the communication stream, in
 * host issue order) overlapped with the z pass of the interior planes. */
/* d_scale_max (the first blur of the pyramid only, else NULL): the blur of src / *d_scale_max -- im_scale
 * folded into the x pass (sift3d_hip_fir_x_scaled); returns 2 without doing anything when that x pass does
 * not cover the configuration (the same answer on every rank) */
static int sh_blur(sift3d_amd_sharded *S, const struct sh_chain *C, int o, int s, const float *src,
                   const float *d_scale_max)
{
    const sh_level *Lg = &S->G[o][s];
    const filter_t *f = &S->filt[s];
    float *dst = Lg->t;
    const size_t plane = sh_plane(S, o);
    const int nx = S->dims[o][0], ny = S->dims[o][1], nzo = S->dims[o][2];
    const float ufx = (float)(1.0 / (S->units[0] * ldexp(1.0, o)));
    const float ufy = (float)(1.0 / (S->units[1] * ldexp(1.0, o)));
    const float ufz = (float)(1.0 / (S->units[2] * ldexp(1.0, o)));
    const int hw = f->width / 2;
    const int reach = (int)ceilf((float)hw * ufz) + 1;
    const int exch = S->world > 1 && sh_sharded(S, o);
    float *zin;
    int fused, a, b, ia, ib;
    sh_owned(S, o, &a, &b);
    if (d_scale_max) {
        const sift3d_hip_fir_args fa = sh_fir_args(S, src, C->tmp_a, o, Lg->nloc, 0, f, ufx, 0, a, b);
        /* (whether this x pass covers the configuration does not depend on the rank) */
        if (!sift3d_hip_fir_x_scaled_covers(&fa))
            return 2;
        SH_DO(sift3d_hip_fir_x_scaled(&fa, d_scale_max, C->stream) != SIFT3D_SUCCESS);
    } else {
        SH_DO(sh_fir(S, src, C->tmp_a, o, Lg->nloc, 0, f, ufx, 0, a, b, C->stream));
    }
    fused = ufy == 1.0f && ufz == 1.0f && sift3d_hip_fir_yz_u1_covers(C->tmp_a, dst, nx, ny, f->width, nzo);
    zin = C->tmp_a;
    if (!fused) {
        SH_DO(sh_fir(S, C->tmp_a, C->tmp_b, o, Lg->nloc, 1, f, ufy, 0, a, b, C->stream));
        zin = C->tmp_b;
    }
    /* interior planes need no halo: [ia, ib) */
    ia = exch && Lg->z0 > 0 ? a + reach : a;
    ib = exch && Lg->z1 < nzo ? b - reach : b;
    if (ib < ia)
        ia = ib = a;                                     /* thin slab: everything after the exchange */
    if (exch) {
        SH_COMM(stream_after(S->comm_stream, C->ev_x, C->stream) ||
                sh_halo_range(S, zin, Lg, plane, 0, reach, S->comm_stream) ||
                sift3d_hip_event_record(C->ev_halo, S->comm_stream));
    }
#define SH_ZPASS(lo_, hi_)                                                                           \
    do {                                                                                             \
        if ((hi_) > (lo_)) {                                                                         \
            if (fused)                                                                               \
                SH_DO(sift3d_hip_fir_yz_u1(zin, dst, nx, ny, Lg->nloc, f->taps, f->width, nzo,       \
                                           Lg->off, (lo_), (hi_), C->stream) != SIFT3D_SUCCESS);     \
            else                                                                                     \
                SH_DO(sh_fir(S, zin, dst, o, Lg->nloc, 2, f, ufz, Lg->off, (lo_), (hi_), C->stream)); \
        }                                                                                            \
    } while (0)
    SH_ZPASS(ia, ib);
    if (exch) {
        SH_COMM(sift3d_hip_stream_wait_event(C->stream, C->ev_halo));
        SH_ZPASS(a, ia);
        SH_ZPASS(ib, b);
    }
#undef SH_ZPASS
    return SIFT3D_SUCCESS;
}

/* a buffer of at least `bytes` (grown with a quarter of slack) in device memory, or in page-locked host memory */
static int sh_ensure(void **p, size_t *cap, size_t bytes, int pinned)
{
    if (bytes <= *cap)
        return SIFT3D_SUCCESS;
    (pinned ? sift3d_hip_host_free : sift3d_hip_free)(*p);
    *cap = 0;
    *p = (pinned ? sift3d_hip_host_alloc : sift3d_hip_malloc)(bytes + bytes / 4);
    if (!*p)
        return SIFT3D_FAILURE;
    *cap = bytes + bytes / 4;
    return SIFT3D_SUCCESS;
}
static int sh_ensure_dev(void **p, size_t *cap, size_t bytes) { return sh_ensure(p, cap, bytes, 0); }
static int sh_ensure_pinned(void **p, size_t *cap, size_t bytes) { return sh_ensure(p, cap, bytes, 1); }

/* all-gather of one device block per rank, on the main stream (one rank: a copy) */
static int sh_allgather_dev(sift3d_amd_sharded *S, const void *d_mine, void *d_all, size_t bytes)
{
    if (S->world == 1)
        return sift3d_hip_memcpy_d2d(d_all, d_mine, bytes, S->stream);
    return S->T.allgather(S->T.ctx, d_mine, d_all, bytes, S->stream);
}

static int sh_ensure_cand(sift3d_amd_sharded *S, uint32_t cap)
{
    if (cap <= S->cand_cap)
        return SIFT3D_SUCCESS;
    sh_free_cand(S);
    S->d_cand = (sift3d_hip_cand *)sift3d_hip_malloc(sizeof(sift3d_hip_cand) * (size_t)cap);
    S->d_R = (float *)sift3d_hip_malloc(sizeof(float) * 9 * (size_t)cap);
    S->d_keep = (int32_t *)sift3d_hip_malloc(sizeof(int32_t) * (size_t)cap);
    if (!S->d_cand || !S->d_R || !S->d_keep)
        return SIFT3D_FAILURE;
    S->cand_cap = cap;
    return SIFT3D_SUCCESS;
}

/* ---- detect -------------------------------------------------------------------------------- */
typedef struct {          /* a record of the global list as sift3d_hip_slab_build delivers it */
    int32_t o, s, x, y, z;
    float R[9];
    float strength;
    int32_t pad;
} sh_out;

/* The tables sift3d_hip_slab_build searches and the layout of a rank's block of the second all-gather, from the
 * gathered count blocks (host only; include/sift3d_amd.h).  Per rank: prefix sums over keys (ck kept, cc
 * candidates); per (key, rank), keys major: the segment starts of the two global orders. */
int sift3d_amd_slab_table(const void *cnt, size_t cnt_stride, int world, int nkey, uint32_t *tab,
                          sift3d_amd_slab_layout *lay)
{
    const int W = world, nseg = nkey * W;
    uint32_t *segk, *segc, *ck, *cc;
    size_t maxc = 0, maxk = 0, tot_c = 0, tot_k = 0;
    int r, k;
    if (!cnt || !tab || !lay || W < 1 || nkey < 1 || nkey > 256 || cnt_stride < sizeof(int32_t) * 2 * (size_t)nkey)
        return SIFT3D_FAILURE;
    /* every total is a uint32 in the tables and in the kernel's arguments: the counts are non-negative int32, at
     * most 256 * world of them, so the sums below cannot wrap a size_t before they are checked */
    for (r = 0; r < W; r++) {
        const int32_t *a = (const int32_t *)((const char *)cnt + cnt_stride * (size_t)r);
        for (k = 0; k < nkey; k++) {
            if (a[2 * k] < 0 || a[2 * k + 1] < 0)
                return SIFT3D_FAILURE;
            tot_c += (size_t)a[2 * k];
            tot_k += (size_t)a[2 * k + 1];
        }
    }
    if (tot_c > UINT32_MAX || tot_k > UINT32_MAX)
        return SIFT3D_FAILURE;
    tot_c = tot_k = 0;
    segk = tab; segc = segk + nseg + 1; ck = segc + nseg + 1; cc = ck + (size_t)W * (nkey + 1);
    for (r = 0; r < W; r++) {
        const int32_t *a = (const int32_t *)((const char *)cnt + cnt_stride * (size_t)r);
        ck[(size_t)r * (nkey + 1)] = cc[(size_t)r * (nkey + 1)] = 0;
        for (k = 0; k < nkey; k++) {
            cc[(size_t)r * (nkey + 1) + k + 1] = cc[(size_t)r * (nkey + 1) + k] + (uint32_t)a[2 * k];
            ck[(size_t)r * (nkey + 1) + k + 1] = ck[(size_t)r * (nkey + 1) + k] + (uint32_t)a[2 * k + 1];
        }
        if (cc[(size_t)r * (nkey + 1) + nkey] > maxc) maxc = cc[(size_t)r * (nkey + 1) + nkey];
        if (ck[(size_t)r * (nkey + 1) + nkey] > maxk) maxk = ck[(size_t)r * (nkey + 1) + nkey];
    }
    for (k = 0; k < nkey; k++)
        for (r = 0; r < W; r++) {
            segc[(size_t)k * W + r] = (uint32_t)tot_c;
            segk[(size_t)k * W + r] = (uint32_t)tot_k;
            tot_c += cc[(size_t)r * (nkey + 1) + k + 1] - cc[(size_t)r * (nkey + 1) + k];
            tot_k += ck[(size_t)r * (nkey + 1) + k + 1] - ck[(size_t)r * (nkey + 1) + k];
        }
    segc[nseg] = (uint32_t)tot_c;
    segk[nseg] = (uint32_t)tot_k;
    lay->tot_c = tot_c; lay->tot_k = tot_k; lay->maxc = maxc; lay->maxk = maxk;
    /* a rank's block: [values of all its candidates][its kept records][status word] */
    lay->roff = (sizeof(float) * (maxc ? maxc : 1) + 15) & ~(size_t)15;
    lay->toff = lay->roff + ((56 * (maxk ? maxk : 1) + 15) & ~(size_t)15);
    lay->blk = lay->toff + 16;
    return SIFT3D_SUCCESS;
}

/* What the stages of ONE detect call pass to each other: every field is set by the stage that decides it and
 * only read after that.  Nothing of it outlives the call. */
typedef struct {
    double t_start;
    int nkey;                    /* (octave, keypoint level) pairs: the keys of the global order */
    int all_free;                /* every octave takes the DoG-free sweep */
    uint32_t count;              /* this rank's candidates; 0 once it has failed */
    size_t cnt_bytes;            /* a rank's block of the first all-gather: 2 counts per key, status word */
    size_t tab_words;            /* words of the segment tables */
    sift3d_amd_slab_layout lay;  /* totals of all ranks, a rank's block of the second all-gather */
} sh_run;

/* the two status words this rank sends, behind the gathered counts in the page-locked count buffer */
static inline int32_t *sh_status_words(const sift3d_amd_sharded *S, const sh_run *r)
{
    return (int32_t *)((char *)S->h_cnt + r->cnt_bytes * (size_t)S->world);
}

/* arguments, the failure mark, and set_im_SIFT3D: scale by the GLOBAL max|v| (sift.c:645-649; im_scale itself is
 * folded into the first blur, or run there).  EXCHANGE: all-reduce of one float, main stream. */
static int sh_begin(sift3d_amd_sharded *S, const sift3d_keypoint_store *kp, sh_run *r)
{
    int o;
    memset(r, 0, sizeof(*r));
    r->t_start = now_s();
    if (!S || !kp)
        return SIFT3D_FAILURE;
    r->nkey = S->num_octaves * S->K;
    if (r->nkey > 256)
        return SIFT3D_FAILURE;
    r->all_free = 1;
    for (o = 0; o < S->num_octaves; o++)
        r->all_free = r->all_free && S->dog_free[o];
    S->failed = S->inject == 1 ? -1 : 0;
    sift3d_hip_event_record(S->ev[4], S->stream);
    SH_DO(sift3d_hip_memset(S->d_scalars, 0, sizeof(float) * (8 + SH_MAX_NDL * SH_MAX_OCT), S->stream) ||
          sift3d_hip_absmax(S->d_raw, sh_plane(S, 0) * (size_t)(S->in_z1 - S->in_z0), S->d_scalars, S->stream));
    if (S->world > 1)
        SH_COMM(S->T.allreduce_max(S->T.ctx, S->d_scalars, 1, S->stream));
    return SIFT3D_SUCCESS;
}

/* the first blur reads the raw slab and scales as it stages (im_scale folded into the x pass: the scaled image is
 * not stored); where that x pass does not apply, scale first.  EXCHANGE: the blur's halo. */
static int sh_first_blur(sift3d_amd_sharded *S)
{
    const struct sh_chain *C0 = &S->chain[0];
    int a0, b0, rc;
    sh_owned(S, 0, &a0, &b0);
    /* (d_raw holds the owned planes only: plane index a0 of the level buffer is its plane 0) */
    rc = sh_blur(S, C0, 0, 0, S->d_raw - (size_t)a0 * sh_plane(S, 0), S->d_scalars);
    if (rc == 2) {
        SH_DO(sift3d_hip_scale(S->d_raw, S->d_im + (size_t)a0 * sh_plane(S, 0),
                               sh_plane(S, 0) * (size_t)(S->in_z1 - S->in_z0), S->d_scalars, S->stream));
        return sh_blur(S, C0, 0, 0, S->d_im, NULL);
    }
    return rc;
}

/* octave o + 1 from Gaussian level K of octave o (max(s_end - 2, first_level), sift.c:696-704), both sharded or
 * both replicated: the owned planes, on stream ds */
static void sh_downsample(sift3d_amd_sharded *S, int o, void *ds)
{
    const sh_level *src = &S->G[o][S->K];
    sh_level *dst = &S->G[o + 1][0];
    const int z0 = sh_sharded(S, o + 1) ? dst->z0 : 0, z1 = sh_sharded(S, o + 1) ? dst->z1 : S->dims[o + 1][2];
    if (z1 > z0)
        SH_DO(sift3d_hip_downsample2(src->t + (size_t)(2 * z0 - src->off) * sh_plane(S, o), S->dims[o][0],
                                     S->dims[o][1], dst->t + (size_t)(z0 - dst->off) * sh_plane(S, o + 1),
                                     S->dims[o + 1][0], S->dims[o + 1][1], z1 - z0, ds));
}

/* The same across the transition to the replicated octaves: down-sample the owned planes into a staging slab,
 * all-gather the slabs (padded to the largest), copy them into place.  EXCHANGE: the all-gather, on the MAIN
 * stream (behind what that stream holds), where every other collective of a step is issued; stream ds, which
 * builds the next octave, goes on behind it. */
static int sh_transition(sift3d_amd_sharded *S, int o, void *ds)
{
    const sh_level *src = &S->G[o][S->K];
    sh_level *dst = &S->G[o + 1][0];
    const size_t pl_d = sh_plane(S, o + 1);
    int zb[SH_MAX_WORLD + 1], r;
    const size_t slab = (size_t)sh_transition_slabs(S, o + 1, zb) * pl_d;
    const int z0 = zb[S->rank], z1 = zb[S->rank + 1];
    float *mine = S->d_stage, *all = mine + slab;
    if (slab * (size_t)(S->world + 1) > S->stage_elems)
        return SIFT3D_FAILURE;       /* (geometry: the same on every rank) */
    SH_DO(sift3d_hip_memset(mine, 0, slab * sizeof(float), ds));
    if (z1 > z0)
        SH_DO(sift3d_hip_downsample2(src->t + (size_t)(2 * z0 - src->off) * sh_plane(S, o), S->dims[o][0],
                                     S->dims[o][1], mine, S->dims[o + 1][0], S->dims[o + 1][1], z1 - z0, ds));
    if (ds != S->stream)
        SH_COMM(stream_after(S->stream, S->ev_tr, ds));
    SH_COMM(S->T.allgather(S->T.ctx, mine, all, slab * sizeof(float), S->stream));
    for (r = 0; r < S->world; r++)
        if (zb[r + 1] > zb[r])
            SH_DO(sift3d_hip_memcpy_d2d(dst->t + (size_t)zb[r] * pl_d, all + (size_t)r * slab,
                                        (size_t)(zb[r + 1] - zb[r]) * pl_d * sizeof(float), S->stream));
    if (ds != S->stream)
        SH_COMM(stream_after(ds, S->ev_tr, S->stream));
    return SIFT3D_SUCCESS;
}

/* build_gpyr, sift.c:662-711 -- on three dependency chains, as the single-GPU path builds it
 * (detect_on_device): octave o + 1 starts from level K of octave o (sift.c:696-704) and the levels after
 * K feed nothing but their octave's DoG, so once level K of octave 0 exists the smaller octaves --
 * short launches that cannot fill the device -- are built on a second stream BESIDE the last levels of
 * octave 0, their own last levels on a third, and all are joined before the DoG stage.
 * EXCHANGES: the z-halo exchange of every blur of a sharded octave; those of all chains travel on the one
 * communication stream in the order the host issues them here (the same on every rank): octave by octave, levels
 * 0 (octave 0 only), 1 .. K, then K + 1 .. ngl - 1.  Between the two groups of the last sharded octave: the
 * transition's all-gather. */
static int sh_pyramid(sift3d_amd_sharded *S)
{
    const int forked = S->num_octaves > 1 && S->K + 1 < S->ngl;
    int o, s;
    SH_COMM(sh_first_blur(S));
    for (o = 0; o < S->num_octaves; o++) {
        const struct sh_chain *Ca = &S->chain[o > 0 && forked ? 1 : 0];        /* levels 1 .. K */
        const struct sh_chain *Cb = &S->chain[o > 0 && forked ? 2 : 0];        /* levels K + 1 .. */
        for (s = 1; s <= S->K && s < S->ngl; s++)
            SH_COMM(sh_blur(S, Ca, o, s, S->G[o][s - 1].t, NULL));
        /* level K exists: the next octave (chain 1) and this octave's last levels (chain 2, or the main stream
         * for octave 0) go their own ways */
        if (forked && o == 0)
            SH_COMM(stream_after(S->chain[1].stream, S->ev_fork, S->stream));
        else if (forked)
            SH_COMM(stream_after(Cb->stream, S->ev_oct[o], Ca->stream));
        if (o != S->num_octaves - 1) {
            void *ds = forked ? S->chain[1].stream : S->stream;      /* the stream that builds the next octave */
            if (sh_sharded(S, o) && !sh_sharded(S, o + 1))
                SH_COMM(sh_transition(S, o, ds));
            else
                sh_downsample(S, o, ds);
        }
        for (s = S->K + 1; s < S->ngl; s++)
            SH_COMM(sh_blur(S, Cb, o, s, S->G[o][s - 1].t, NULL));
    }
    if (forked)
        SH_COMM(stream_after(S->stream, S->ev_join, S->chain[1].stream) ||
                stream_after(S->stream, S->ev_join2, S->chain[2].stream));
    return SIFT3D_SUCCESS;
}

/* The nearest halo plane of every level of the sharded octaves: the extrema test looks one plane past the slab,
 * and stored DoG levels are formed on it.  EXCHANGES: one halo per level, main stream. */
static int sh_nearest_halos(sift3d_amd_sharded *S)
{
    int o, s;
    for (o = 0; o < S->o_shard; o++)
        for (s = 0; s < S->ngl; s++)
            SH_COMM(sh_halo_range(S, S->G[o][s].t, &S->G[o][s], sh_plane(S, o), 0, 1, S->stream));
    return SIFT3D_SUCCESS;
}

/* the stored DoG levels of octave o (build_dog, sift.c:713-732) and their maxima, on the owned planes [lo, hi) and
 * one plane around them -- the neighbours' planes are theirs to count, but a maximum does not mind a plane twice */
static void sh_dog_octave(sift3d_amd_sharded *S, int o, int lo, int hi)
{
    const int lo2 = lo > 0 ? lo - 1 : 0, hi2 = hi < S->G[o][0].nloc ? hi + 1 : S->G[o][0].nloc;
    const size_t n2 = (size_t)(hi2 - lo2) * sh_plane(S, o);
    const float *g[SH_MAX_NGL];
    float *dd[SH_MAX_NDL];
    int s, rc = 0;
    sh_level_ptrs(S, o, lo2, g);
    for (s = 0; s < S->ndl; s++)
        dd[s] = S->D[o][s] + (size_t)lo2 * sh_plane(S, o);
    if (!S->failed)
        rc = sift3d_hip_dog_stack(g, dd, S->ngl, n2, sh_dogmax_slot(S, o), S->stream);
    if (rc == 1) {
        for (s = 0; s < S->ndl; s++)
            SH_DO(sift3d_hip_subtract_absmax(g[s], g[s + 1], dd[s], n2, sh_dogmax_slot(S, o) + s, S->stream));
    } else if (rc != SIFT3D_SUCCESS) {
        SH_DO(1);
    }
}

/* dogmax (sift.c:821-826) of every octave on the owned planes (every plane is owned by some rank), one all-reduce
 * for all of them.  Octaves of the DoG-free sweep store no DoG level; the others form theirs.
 * EXCHANGE: all-reduce of ndl * num_octaves floats, main stream. */
static int sh_dog_stage(sift3d_amd_sharded *S)
{
    int o, lo, hi;
    for (o = 0; o < S->num_octaves; o++) {
        const float *g[SH_MAX_NGL];
        sh_owned(S, o, &lo, &hi);
        if (hi <= lo)
            continue;
        if (S->dog_free[o]) {
            sh_level_ptrs(S, o, lo, g);
            SH_DO(sift3d_hip_dogmax_stack(g, S->ngl, (size_t)(hi - lo) * sh_plane(S, o), sh_dogmax_slot(S, o),
                                          S->stream) != SIFT3D_SUCCESS);
        } else {
            sh_dog_octave(S, o, lo, hi);
        }
    }
    if (S->world > 1)
        SH_COMM(S->T.allreduce_max(S->T.ctx, S->d_scalars + 8, S->ndl * S->num_octaves, S->stream));
    return SIFT3D_SUCCESS;
}

/* The windows of the orientation and descriptor kernels reach win_reach[s] planes into the neighbours' slabs: the
 * largest exchange of a step.  EXCHANGES: one halo per level of the sharded octaves, on the communication stream
 * WHILE the extrema are found; awaited by sh_orient_stage.  (No collective is issued on the compute stream in
 * between: one communicator, one order.) */
static int sh_window_halos_begin(sift3d_amd_sharded *S)
{
    int o, s;
    if (S->world == 1 || S->o_shard == 0)
        return SIFT3D_SUCCESS;
    SH_COMM(stream_after(S->comm_stream, S->chain[0].ev_x, S->stream));
    for (o = 0; o < S->o_shard; o++)
        for (s = 0; s < S->ngl; s++)
            SH_COMM(sh_halo_range(S, S->G[o][s].t, &S->G[o][s], sh_plane(S, o), 1, S->win_reach[s],
                                  S->comm_stream));
    SH_COMM(sift3d_hip_event_record(S->chain[0].ev_halo, S->comm_stream));
    return SIFT3D_SUCCESS;
}

/* the extrema sweep of octave o on this rank's interior planes: the DoG-free sweep's phase (0: all of it; side by
 * side 1: the sweep, on chain 1's stream for the octaves >= 1, 2: scan + emission) or, on stored DoG levels,
 * sift3d_hip_extrema_mode */
static void sh_sweep_octave(sift3d_amd_sharded *S, int o, int side, int phase)
{
    const sh_level *L = &S->G[o][0];
    const int nzo = S->dims[o][2];
    const int zl = (L->z0 > 1 ? L->z0 : 1) - L->off, zh = (L->z1 < nzo - 1 ? L->z1 : nzo - 1) - L->off;
    size_t wb;
    void *wk = sh_extrema_work(S, o, side, &wb);
    int s;
    if (L->nloc < 3 || zh <= zl)
        return;                              /* no interior plane on this rank */
    if (S->dog_free[o]) {
        const float *g[SH_MAX_NGL];
        sh_level_ptrs(S, o, 0, g);
        SH_DO(sift3d_hip_extrema_gauss6_phase(g, sh_dogmax_slot(S, o), S->dims[o][0], S->dims[o][1], L->nloc, zl, zh,
                                              o * S->ngl + 1, S->peak_thresh, S->d_cand, S->cand_cap,
                                              sh_cand_counter(S), wk, wb,
                                              phase == 1 && o > 0 ? S->chain[1].stream : S->stream,
                                              phase) != SIFT3D_SUCCESS);
    } else {
        sift3d_hip_extrema_level lv[SH_MAX_K];
        for (s = 0; s < S->K; s++) {
            lv[s].prev = S->D[o][s];
            lv[s].cur = S->D[o][s + 1];
            lv[s].next = S->D[o][s + 2];
            lv[s].d_absmax = sh_dogmax_slot(S, o) + s + 1;
            lv[s].z_lo = zl; lv[s].z_hi = zh;
            lv[s].tag = o * S->ngl + s + 1;          /* Gaussian level (o, s) of the table */
        }
        SH_DO(sift3d_hip_extrema_mode(lv, S->K, S->dims[o][0], S->dims[o][1], L->nloc, S->peak_thresh, S->cuboid,
                                      S->d_cand, S->cand_cap, sh_cand_counter(S), wk, wb, S->stream));
    }
}

/* detect_extrema (sift.c:735-871) on the owned planes: at most two attempts -- a list that does not fit the
 * candidate arrays is still counted, the arrays are grown to hold it, and the sweeps run once more.  No exchange. */
static int sh_extrema_stage(sift3d_amd_sharded *S, sh_run *r)
{
    /* with every octave on the DoG-free sweep: the sweeps of octaves >= 1 (short launches) beside octave 0's on a
     * second stream, then scan + emission in octave order (sift3d_hip_extrema_gauss6_phase); otherwise octave by
     * octave */
    const int side = r->all_free && S->num_octaves > 1 && S->d_work2 != NULL;
    int attempt, phase, o;
    SH_DO(sh_ensure_cand(S, sh_cand_capacity(S)));
    for (attempt = 0; attempt < 2 && !S->failed; attempt++) {
        SH_DO(sift3d_hip_memset(sh_cand_counter(S), 0, sizeof(uint32_t), S->stream));
        if (side)
            SH_COMM(stream_after(S->chain[1].stream, S->ev_fork, S->stream));
        for (phase = side ? 1 : 0; phase <= (side ? 2 : 0); phase++) {
            for (o = 0; o < S->num_octaves; o++)
                sh_sweep_octave(S, o, side, phase);
            if (phase == 1)
                SH_COMM(stream_after(S->stream, S->ev_join, S->chain[1].stream));
        }
        SH_DO(sift3d_hip_memcpy_d2h(&r->count, sh_cand_counter(S), sizeof(r->count), S->stream));
        SH_COMM(sift3d_hip_stream_sync(S->stream));
        if (S->failed || r->count <= S->cand_cap)
            break;
        SH_DO(sh_ensure_cand(S, r->count + r->count / 4 + 1024));
    }
    if (S->inject == 2)
        S->failed = -2;
    if (S->failed)
        r->count = 0;
    return SIFT3D_SUCCESS;
}

/* assign_orientations (sift.c:1109-1167) for the local candidates, once the window halos have arrived.  No
 * exchange (the wait closes sh_window_halos_begin's). */
static int sh_orient_stage(sift3d_amd_sharded *S, sh_run *r)
{
    const int nlev = S->num_octaves * S->ngl;
    if (S->world > 1 && S->o_shard > 0)
        SH_COMM(sift3d_hip_stream_wait_event(S->stream, S->chain[0].ev_halo));
    /* the serial sums pack window-relative x and y into 10 bits each (sift3d_hip_orient_window_fits) */
    for (int t = 0; r->count && !S->failed && t < nlev; t++) {
        const sift3d_hip_level *L = S->h_levels + t;
        if (!sift3d_hip_orient_window_fits(L->nx, L->ny, (double)L->ux, (double)L->uy, L->sd)) {
            ERR("sift3d_amd_sharded: the orientation window of a %d x %d level with units (%f, %f) at scale %f is "
                "wider than 1023 voxels \n", L->nx, L->ny, (double)L->ux, (double)L->uy, L->sd);
            SH_DO(1);
            r->count = 0;
        }
    }
    if (r->count) {
        SH_DO(orient_tab_reserve(&S->d_otab, &S->otab_bytes, nlev, S->cand_cap, S->stream, 0));
        SH_DO(sift3d_hip_orient_tab(S->d_levels, nlev, S->d_cand, r->count, S->corner_thresh, S->d_R, S->d_keep,
                                    S->d_otab, S->cand_cap, S->stream));
        if (S->failed)
            r->count = 0;
    }
    return SIFT3D_SUCCESS;
}

/* The exchange of the keypoints: per-(octave, level) counts, the candidates' |DoG| values and the
 * ORIENTED keypoints -- device to device.  First the counts, with this rank's status word behind them: the host
 * needs the result to size the second all-gather.  EXCHANGE: all-gather of cnt_bytes per rank, main stream.
 * Returns failure, on every rank, when any rank has failed so far. */
static int sh_exchange_counts(sift3d_amd_sharded *S, sh_run *r)
{
    const int W = S->world;
    char *mine;
    int32_t *h_stat;
    int q, any_failed = 0;
    r->cnt_bytes = ((sizeof(int32_t) * 2 * (size_t)r->nkey + 15) & ~(size_t)15) + 16;
    /* [W blocks gathered][mine] */
    if (sh_ensure_dev(&S->d_cnt, &S->cnt_cap, r->cnt_bytes * (size_t)(W + 1)) ||
        sh_ensure_pinned(&S->h_cnt, &S->hcnt_cap, r->cnt_bytes * (size_t)W + 64))
        return SIFT3D_FAILURE;               /* (the exchange buffers themselves: nothing to send in) */
    mine = (char *)S->d_cnt + r->cnt_bytes * (size_t)W;
    h_stat = sh_status_words(S, r);
    SH_DO(sift3d_hip_slab_count(S->d_cand, S->d_keep, r->count, S->ngl, S->K, r->nkey, (int32_t *)mine, S->stream));
    h_stat[0] = S->failed;
    SH_COMM(sift3d_hip_memcpy_h2d(mine + r->cnt_bytes - 16, h_stat, sizeof(int32_t), S->stream) ||
            sh_allgather_dev(S, mine, S->d_cnt, r->cnt_bytes) ||
            sift3d_hip_memcpy_d2h(S->h_cnt, S->d_cnt, r->cnt_bytes * (size_t)W, S->stream) ||
            sift3d_hip_stream_sync(S->stream));
    for (q = 0; q < W; q++)
        any_failed |= *(const int32_t *)((const char *)S->h_cnt + r->cnt_bytes * (size_t)(q + 1) - 16) != 0;
    if (any_failed)
        sh_report_local_failure(S);
    return any_failed ? SIFT3D_FAILURE : SIFT3D_SUCCESS;
}

/* Then values + records in ONE block per rank; the global list is built by a kernel on every rank
 * (sift3d_hip_slab_build: (o, s) major, ranks in slab order inside a level -- their z ranges are disjoint and
 * ascending --, a rank's own (z, y, x) order inside its segment) and read back once.  EXCHANGE: all-gather of
 * lay.blk bytes per rank, main stream.  Returns failure, on every rank, when any rank has failed. */
static int sh_exchange_records(sift3d_amd_sharded *S, sh_run *r, sift3d_keypoint_store *kp)
{
    const int W = S->world;
    const sift3d_amd_slab_layout *lay = &r->lay;
    int32_t *h_stat = sh_status_words(S, r);
    char *mine;
    /* prefix sums over keys per rank (ck kept, cc candidates), segment starts of the global orders */
    r->tab_words = 2 * ((size_t)r->nkey * W + 1) + 2 * (size_t)W * (r->nkey + 1);
    if (sh_ensure_pinned(&S->h_tab, &S->htab_cap, sizeof(uint32_t) * r->tab_words) ||
        sh_ensure_dev(&S->d_tab, &S->tab_cap, sizeof(uint32_t) * r->tab_words))
        return SIFT3D_FAILURE;
    if (sift3d_amd_slab_table(S->h_cnt, r->cnt_bytes, W, r->nkey, (uint32_t *)S->h_tab, &r->lay) != SIFT3D_SUCCESS) {
        ERR("sift3d_amd_sharded_detect: the candidate counts of the %d ranks do not fit 32 bits \n", W);
        return SIFT3D_FAILURE;               /* on every rank: all of them see the same counts */
    }
    S->ncand = (int)lay->tot_c;
    if (S->inject == 3)
        S->failed = -3;
    /* this rank's block: [values of all its candidates][its kept records][status word] */
    if (sh_ensure_dev(&S->d_xchg, &S->xchg_bytes, lay->blk * (size_t)(W + 1)) ||
        sh_ensure_dev(&S->d_out, &S->out_cap, 64 + 64 * (lay->tot_k ? lay->tot_k : 1)) ||
        sh_ensure_pinned(&S->h_xchg, &S->hxchg_cap, 64 + 64 * (lay->tot_k ? lay->tot_k : 1)) ||
        sh_ensure_dev(&S->d_pack, &S->pack_cap, sift3d_hip_slab_pack_scratch_bytes(S->cand_cap)))
        return SIFT3D_FAILURE;
    /* keypoint store: dimensions of the first octave (sift.c:756-759) */
    kp->nx = S->nx; kp->ny = S->ny; kp->nz = S->nz;
    SH_DO(kp_store_resize(kp, lay->tot_k));
    mine = (char *)S->d_xchg + lay->blk * (size_t)W;
    SH_DO(sift3d_hip_memcpy_h2d(S->d_tab, S->h_tab, sizeof(uint32_t) * r->tab_words, S->stream));
    SH_DO(sift3d_hip_slab_pack(S->d_levels, S->d_cand, S->d_keep, S->d_R, r->count, S->ngl, (float *)mine,
                               mine + lay->roff, S->d_pack, S->stream));
    h_stat[1] = S->failed;
    SH_COMM(sift3d_hip_memcpy_h2d(mine + lay->toff, h_stat + 1, sizeof(int32_t), S->stream) ||
            sh_allgather_dev(S, mine, S->d_xchg, lay->blk));
    /* (copy_Keypoint omits `strength`, sift.c:372-384: slot j keeps GLOBAL candidate j's value) */
    SH_DO(sift3d_hip_slab_build(S->d_xchg, lay->blk, lay->roff, lay->toff, W, r->nkey, (const uint32_t *)S->d_tab,
                                (uint32_t)lay->tot_k, (uint32_t)lay->tot_c, S->d_out, S->stream));
    SH_COMM(sift3d_hip_memcpy_d2h(S->h_xchg, S->d_out, 64 + 64 * lay->tot_k, S->stream) ||
            sift3d_hip_stream_sync(S->stream));
    if (S->failed || *(const int32_t *)S->h_xchg != 0) {
        sh_report_local_failure(S);
        return SIFT3D_FAILURE;               /* on every rank: the status words are in everybody's list */
    }
    return SIFT3D_SUCCESS;
}

/* the records into the store: a few threads, each on a contiguous part; a segment holds one (octave, level),
 * i.e. one scale (imutil.c:1578-1579) */
static void sh_fill_store(const sift3d_amd_sharded *S, const sh_run *r, sift3d_keypoint_store *kp)
{
    const sh_out *rec = (const sh_out *)((const char *)S->h_xchg + 64);
    const size_t tot_k = r->lay.tot_k;
    const int nt = host_threads(tot_k);
    double sdk[256];
    int k;
    for (k = 0; k < r->nkey; k++)
        sdk[k] = sh_scale(S, k / S->K, k % S->K);
#pragma omp parallel num_threads(nt)
    {
        const int nth = omp_get_num_threads(), t = omp_get_thread_num();   /* (the team's real size) */
        const size_t lo = tot_k * (size_t)t / nth, hi = tot_k * (size_t)(t + 1) / nth;
        size_t g;
        for (g = lo; g < hi; g++) {
            keypoint_t *kk = kp->buf + g;
            kk->o = rec[g].o; kk->s = rec[g].s;
            kk->xd = rec[g].x; kk->yd = rec[g].y; kk->zd = rec[g].z;
            kk->sd = sdk[rec[g].o * S->K + rec[g].s];
            memcpy(kk->R, rec[g].R, sizeof(kk->R));
            kk->strength = rec[g].strength;
        }
    }
}

/* the call's timers: S->t[] as the struct says, from the marks the driver recorded between the stages */
static void sh_end(sift3d_amd_sharded *S, const sh_run *r)
{
    S->t[0] = 1e-3 * sift3d_hip_event_elapsed_ms(S->ev[0], S->ev[1]);
    S->t[3] = 1e-3 * sift3d_hip_event_elapsed_ms(S->ev[1], S->ev[2]);
    S->t[4] = 1e-3 * sift3d_hip_event_elapsed_ms(S->ev[2], S->ev[3]);
    S->t[5] = now_s() - S->t_gather0;
    S->t[6] = 1e-3 * sift3d_hip_event_elapsed_ms(S->ev[4], S->ev[0]);
    S->t[1] = now_s() - r->t_start;
}

/* One detect call: the stages in the order in which they issue their exchanges (each stage's comment names its
 * own; DESIGN.md section 5 has the whole list), with the marks of the stage timers between them. */
int sift3d_amd_sharded_detect(sift3d_amd_sharded *S, sift3d_keypoint_store *kp)
{
    sh_run r;
    if (sh_begin(S, kp, &r))
        return SIFT3D_FAILURE;
    sift3d_hip_event_record(S->ev[0], S->stream);
    if (sh_pyramid(S))
        return SIFT3D_FAILURE;
    sift3d_hip_event_record(S->ev[1], S->stream);
    if (sh_nearest_halos(S) || sh_dog_stage(S) || sh_window_halos_begin(S) || sh_extrema_stage(S, &r))
        return SIFT3D_FAILURE;
    sift3d_hip_event_record(S->ev[2], S->stream);
    if (sh_orient_stage(S, &r))
        return SIFT3D_FAILURE;
    sift3d_hip_event_record(S->ev[3], S->stream);
    S->t_gather0 = now_s();
    if (sh_exchange_counts(S, &r) || sh_exchange_records(S, &r, kp))
        return SIFT3D_FAILURE;
    sh_fill_store(S, &r, kp);
    sh_end(S, &r);
    return SIFT3D_SUCCESS;
}

/* ---- describe ------------------------------------------------------------------------------ */
enum { SH_LVM = 16 };     /* keypoint levels per octave that sh_order_keypoints has buckets for */
typedef char sh_levels_fit_the_buckets[SH_MAX_K <= SH_LVM ? 1 : -1];

static inline int sh_level_missing(const sift3d_amd_sharded *S, const keypoint_t *k)
{
    return k->o < 0 || k->o >= S->num_octaves || k->s < 0 || k->s >= S->K;
}

/* The keypoints this rank owns, in list order, into own_idx: counted and placed by a few threads, each on a
 * contiguous part of the list.  Returns their number, or -1 for a list with a level the pyramid does not have. */
static int sh_own_keypoints(const sift3d_amd_sharded *S, const sift3d_keypoint_store *kp, int *own_idx)
{
    const size_t num = kp->num;
    const int nt = host_threads(num);
    size_t pre[HOST_THREADS_MAX + 1], total = 0;
    int bad = 0;
    pre[0] = 0;
#pragma omp parallel num_threads(nt) reduction(| : bad)
    {
        const int nth = omp_get_num_threads(), t = omp_get_thread_num();  /* (the team's real size) */
        const size_t lo = num * t / nth, hi = num * (t + 1) / nth;
        size_t q, jj = 0;
        for (q = lo; q < hi; q++) {
            if (sh_level_missing(S, kp->buf + q))
                bad = 1;
            else
                jj += sh_owner(S, kp->buf + q) == S->rank;
        }
        pre[t + 1] = jj;
#pragma omp barrier
#pragma omp single
        {
            int u;
            for (u = 0; u < nth; u++)
                pre[u + 1] += pre[u];
            total = pre[nth];
        }
        /* (implicit barrier) */
        jj = pre[t];
        for (q = lo; q < hi; q++)
            if (!sh_level_missing(S, kp->buf + q) && sh_owner(S, kp->buf + q) == S->rank)
                own_idx[jj++] = (int)q;
    }
    return bad ? -1 : (int)total;
}

/* Launch order of this rank's n keypoints: widest windows first, each histogram to its own row (a stable counting
 * sort by level, as order_keypoints of the single-GPU driver, but with ONE threshold for all of a level: the
 * first level that takes the reference-order kernel).  Fills S->h_kp and the rows' coordinates; returns the
 * number of keypoints of the reference-order kernel, which lead the list. */
static size_t sh_order_keypoints(sift3d_amd_sharded *S, const sift3d_keypoint_store *kp, const int *own_idx, int n,
                                 sift3d_descriptor_store *desc)
{
    const int nt = host_threads((size_t)n);
    /* (Gaussian index of the first level that takes the reference-order kernel; keypoint level s has
     * Gaussian index s + 1) */
    const int s_exact = exact_desc_first_level(S->exact_desc, S->ngl, S->K, S->sigma0, S->units) - 1;
    size_t cnt[HOST_THREADS_MAX][SH_LVM], start[HOST_THREADS_MAX][SH_LVM], n_exact = 0;
    memset(cnt, 0, sizeof(cnt));
#pragma omp parallel num_threads(nt)
    {
        const int nth = omp_get_num_threads(), t = omp_get_thread_num();
        const size_t lo = (size_t)n * t / nth, hi = (size_t)n * (t + 1) / nth;
        size_t q;
        for (q = lo; q < hi; q++)
            cnt[t][kp->buf[own_idx[q]].s]++;
#pragma omp barrier
#pragma omp single
        {
            size_t p = 0;
            int lv, u;
            for (lv = S->K - 1; lv >= 0; lv--) {
                if (lv == s_exact - 1)
                    n_exact = p;           /* (widest windows first: the exact ones lead the list) */
                for (u = 0; u < nth; u++) {
                    start[u][lv] = p;
                    p += cnt[u][lv];
                }
            }
            if (s_exact <= 0)
                n_exact = p;
        }
        /* (implicit barrier) */
        for (q = lo; q < hi; q++)
            describe_record(S->h_kp + start[t][kp->buf[own_idx[q]].s]++, kp->buf + own_idx[q], S->ngl, q);
        desc_store_fill_xyzsd(desc, kp->buf, own_idx, lo, hi);
    }
    return n_exact;
}

/* Descriptors of the keypoints this rank owns (by z).  own_idx (capacity: the number of
 * keypoints) receives their positions in `kp`; desc their descriptors in that order.  The union
 * over ranks covers every keypoint exactly once.  No exchange. */
int sift3d_amd_sharded_describe(sift3d_amd_sharded *S, const sift3d_keypoint_store *kp,
                                sift3d_descriptor_store *desc, int *own_idx, int *n_own)
{
    const double t_start = now_s();
    size_t n_exact;
    int n;
    if (!S || !kp || !desc || !own_idx || !n_own)
        return SIFT3D_FAILURE;
    n = sh_own_keypoints(S, kp, own_idx);
    if (n < 0)
        return SIFT3D_FAILURE;
    *n_own = n;
    if (desc_store_reserve(desc, (size_t)n, S->nx, S->ny, S->nz))
        return SIFT3D_FAILURE;
    if (!n)
        return SIFT3D_SUCCESS;
    if (describe_list_reserve(&S->h_kp, &S->kp_cap, (uint32_t)n))
        return SIFT3D_FAILURE;
    n_exact = sh_order_keypoints(S, kp, own_idx, n, desc);
    /* (no lattice variant, no rows in device memory) */
    if (describe_enqueue(S->d_levels, S->h_levels, S->num_octaves * S->ngl, S->h_kp, (uint32_t)n, (uint32_t)n_exact,
                         0, desc, NULL, S->d_wlut, &S->d_dpart, &S->dpart_bytes, S->stream) ||
        sift3d_hip_stream_sync(S->stream))
        return SIFT3D_FAILURE;
    S->t[2] = now_s() - t_start;
    return SIFT3D_SUCCESS;
}

/* ---- descriptor gather ("computed by the owning rank and gathered (N x 771 f32)") ---- */
/* EXCHANGE: one all-gather of the ranks' row blocks (padded to the largest, status word behind), main stream. */
int sift3d_amd_sharded_gather_descriptors(sift3d_amd_sharded *S, const sift3d_keypoint_store *kp,
                                          const sift3d_descriptor_store *own, const int *own_idx, int n_own,
                                          sift3d_descriptor_store *all, int root)
{
    const int W = S ? S->world : 0;
    size_t num, maxn = 0, blk, q;
    size_t cnt[SH_MAX_WORLD];
    uint32_t *map = NULL;
    int32_t *h_stat;
    int r, want, failed = 0, any = 0, rc = SIFT3D_FAILURE;
    if (!S || !kp || !own || !all || (n_own > 0 && !own_idx) || root >= W)
        return SIFT3D_FAILURE;
    num = kp->num;
    want = root < 0 || root == S->rank;
    if (S->inject == 4)
        failed = -4;
    /* who owns which keypoint follows from the list and the slab bounds: every rank derives every rank's
     * rows (sh_owner, the rule of sift3d_amd_sharded_describe) */
    memset(cnt, 0, sizeof(cnt));
    map = (uint32_t *)malloc(sizeof(uint32_t) * (num ? num : 1));
    if (!map)
        failed = failed ? failed : __LINE__;
    /* (the counts size the exchange: every rank must arrive at the same ones, whatever failed locally) */
    for (q = 0; q < num; q++) {
        const keypoint_t *k = kp->buf + q;
        int rr;
        if (k->o < 0 || k->o >= S->num_octaves) {
            failed = failed ? failed : __LINE__;       /* (the list is the same on every rank) */
            if (map)
                map[q] = 0;
            continue;
        }
        rr = sh_owner(S, k);
        if (map)
            map[q] = ((uint32_t)rr << 24) | (uint32_t)(cnt[rr] & 0xffffffu);
        cnt[rr]++;
    }
    for (r = 0; r < W; r++)
        if (cnt[r] > maxn)
            maxn = cnt[r];
    if (maxn >= (1u << 24))
        goto done;                                     /* (the same on every rank) */
    if (!failed && (size_t)(n_own < 0 ? 0 : n_own) != cnt[S->rank])
        failed = __LINE__;                             /* desc_own is not this rank's describe result */
    if (!failed && (own->num != cnt[S->rank] || (cnt[S->rank] && !own->hist)))
        failed = __LINE__;
    blk = DESC_NUMEL * sizeof(float) * (maxn ? maxn : 1) + 16;
    if (sh_ensure_dev(&S->d_gath, &S->gath_cap, blk * (size_t)(W + 1)) ||
        sh_ensure_pinned(&S->h_cnt, &S->hcnt_cap, 16 * (size_t)W + 64))
        goto done;                                     /* (the exchange buffers themselves) */
    h_stat = (int32_t *)((char *)S->h_cnt + 16 * (size_t)W);
    {
        char *mine = (char *)S->d_gath + blk * (size_t)W;
        if (!failed && cnt[S->rank] &&
            sift3d_hip_memcpy_h2d(mine, own->hist, DESC_NUMEL * sizeof(float) * cnt[S->rank], S->stream))
            failed = __LINE__;
        h_stat[0] = failed;
        if (sift3d_hip_memcpy_h2d(mine + blk - 16, h_stat, sizeof(int32_t), S->stream) ||
            sh_allgather_dev(S, mine, S->d_gath, blk) ||
            sift3d_hip_memcpy2d_d2h(S->h_cnt, 16, (char *)S->d_gath + blk - 16, blk, 16, (size_t)W, S->stream) ||
            sift3d_hip_stream_sync(S->stream))
            goto done;
    }
    for (r = 0; r < W; r++)
        any |= *(const int32_t *)((const char *)S->h_cnt + 16 * (size_t)r) != 0;
    if (any) {
        if (failed)
            ERR("sift3d_amd_sharded_gather_descriptors: rank %d failed locally (mark %d) \n", S->rank, failed);
        goto done;                                     /* on every rank, here */
    }
    if (want && (!map || desc_store_reserve(all, num, S->nx, S->ny, S->nz)))
        goto done;                                     /* (no map: reported above, so not reached with one) */
    rc = SIFT3D_SUCCESS;
    if (want && num) {
        /* rows into the global order on the device, one copy into the store's page-locked array */
        void *d_map = sift3d_hip_malloc(sizeof(uint32_t) * num);
        void *d_rows = sift3d_hip_malloc(sizeof(float) * DESC_NUMEL * num);
        if (!d_map || !d_rows ||
            sift3d_hip_memcpy_h2d(d_map, map, sizeof(uint32_t) * num, S->stream) ||
            sift3d_hip_rows_scatter((float *)d_rows, S->d_gath, blk, (const uint32_t *)d_map, (uint32_t)num,
                                    S->stream) ||
            sift3d_hip_memcpy_d2h(all->hist, d_rows, sizeof(float) * DESC_NUMEL * num, S->stream) ||
            sift3d_hip_stream_sync(S->stream))
            rc = SIFT3D_FAILURE;
        sift3d_hip_free(d_map);
        sift3d_hip_free(d_rows);
        desc_store_fill_xyzsd(all, kp->buf, NULL, 0, num);
    }
done:
    free(map);
    return rc;
}

/* ---- RCCL transport (librccl is loaded at run time: single-GPU users do not need it) -------- */
typedef struct { char internal[128]; } sh_nccl_id;
typedef void *sh_nccl_comm;
typedef struct {
    void *lib;
    sh_nccl_comm comm;
    int rank, world;
    int (*GetUniqueId)(sh_nccl_id *);
    int (*CommInitRank)(sh_nccl_comm *, int, sh_nccl_id, int);
    int (*CommDestroy)(sh_nccl_comm);
    int (*Send)(const void *, size_t, int, int, sh_nccl_comm, void *);
    int (*Recv)(void *, size_t, int, int, sh_nccl_comm, void *);
    int (*AllReduce)(const void *, void *, size_t, int, int, sh_nccl_comm, void *);
    int (*AllGather)(const void *, void *, size_t, int, sh_nccl_comm, void *);
    int (*GroupStart)(void);
    int (*GroupEnd)(void);
} sh_rccl;

enum { SH_NCCL_INT8 = 0, SH_NCCL_FLOAT32 = 7, SH_NCCL_MAX = 2 };   /* rccl.h: ncclDataType_t, ncclRedOp_t */

static int sh_rccl_load(sh_rccl *R)
{
    static const char *names[] = { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" };
    size_t i;
    for (i = 0; i < sizeof(names) / sizeof(names[0]) && !R->lib; i++)
        R->lib = dlopen(names[i], RTLD_NOW | RTLD_GLOBAL);
    if (!R->lib) {
        ERR("sift3d_amd: librccl could not be loaded: %s \n", dlerror());
        return SIFT3D_FAILURE;
    }
#define SH_SYM(field, name)                                             \
    do {                                                                \
        *(void **)(&R->field) = dlsym(R->lib, name);                    \
        if (!R->field) {                                                \
            ERR("sift3d_amd: librccl lacks %s \n", name);              \
            return SIFT3D_FAILURE;                                      \
        }                                                               \
    } while (0)
    SH_SYM(GetUniqueId, "ncclGetUniqueId");
    SH_SYM(CommInitRank, "ncclCommInitRank");
    SH_SYM(CommDestroy, "ncclCommDestroy");
    SH_SYM(Send, "ncclSend");
    SH_SYM(Recv, "ncclRecv");
    SH_SYM(AllReduce, "ncclAllReduce");
    SH_SYM(AllGather, "ncclAllGather");
    SH_SYM(GroupStart, "ncclGroupStart");
    SH_SYM(GroupEnd, "ncclGroupEnd");
#undef SH_SYM
    return SIFT3D_SUCCESS;
}

static int sh_rccl_halo(void *ctx, const void *send_lo, void *recv_lo, const void *send_hi, void *recv_hi,
                        size_t bytes, void *stream)
{
    sh_rccl *R = (sh_rccl *)ctx;
    int rc = 0;
    rc |= R->GroupStart();
    if (recv_lo) rc |= R->Recv(recv_lo, bytes, SH_NCCL_INT8, R->rank - 1, R->comm, stream);
    if (recv_hi) rc |= R->Recv(recv_hi, bytes, SH_NCCL_INT8, R->rank + 1, R->comm, stream);
    if (send_lo) rc |= R->Send(send_lo, bytes, SH_NCCL_INT8, R->rank - 1, R->comm, stream);
    if (send_hi) rc |= R->Send(send_hi, bytes, SH_NCCL_INT8, R->rank + 1, R->comm, stream);
    rc |= R->GroupEnd();
    return rc ? SIFT3D_FAILURE : SIFT3D_SUCCESS;
}

static int sh_rccl_allreduce_max(void *ctx, float *d_buf, int n, void *stream)
{
    sh_rccl *R = (sh_rccl *)ctx;
    return R->AllReduce(d_buf, d_buf, (size_t)n, SH_NCCL_FLOAT32, SH_NCCL_MAX, R->comm, stream)
               ? SIFT3D_FAILURE : SIFT3D_SUCCESS;
}

static int sh_rccl_allgather(void *ctx, const void *d_send, void *d_recv, size_t bytes, void *stream)
{
    sh_rccl *R = (sh_rccl *)ctx;
    return R->AllGather(d_send, d_recv, bytes, SH_NCCL_INT8, R->comm, stream) ? SIFT3D_FAILURE
                                                                              : SIFT3D_SUCCESS;
}

int sift3d_amd_rccl_unique_id(void *id128)
{
    sh_rccl R;
    memset(&R, 0, sizeof(R));
    if (!id128 || sh_rccl_load(&R))
        return SIFT3D_FAILURE;
    return R.GetUniqueId((sh_nccl_id *)id128) ? SIFT3D_FAILURE : SIFT3D_SUCCESS;
}

int sift3d_amd_rccl_transport(sift3d_amd_transport *out, int world, int rank, const void *id128)
{
    sh_rccl *R;
    sh_nccl_id id;
    if (!out || !id128 || world < 1 || rank < 0 || rank >= world)
        return SIFT3D_FAILURE;
    R = (sh_rccl *)calloc(1, sizeof(*R));
    if (!R || sh_rccl_load(R)) {
        free(R);
        return SIFT3D_FAILURE;
    }
    memcpy(&id, id128, sizeof(id));
    R->rank = rank; R->world = world;
    if (R->CommInitRank(&R->comm, world, id, rank)) {
        ERR("sift3d_amd: ncclCommInitRank failed (rank %d of %d) \n", rank, world);
        free(R);
        return SIFT3D_FAILURE;
    }
    memset(out, 0, sizeof(*out));
    out->rank = rank; out->world = world; out->ctx = R;
    out->halo = sh_rccl_halo;
    out->allreduce_max = sh_rccl_allreduce_max;
    out->allgather = sh_rccl_allgather;
    return SIFT3D_SUCCESS;
}

void sift3d_amd_rccl_transport_free(sift3d_amd_transport *t)
{
    sh_rccl *R;
    if (!t || !t->ctx)
        return;
    R = (sh_rccl *)t->ctx;
    if (R->comm)
        R->CommDestroy(R->comm);
    free(R);
    t->ctx = NULL;
}

/* ranks as threads of one process: the stream-ordered rehearsal transport */
#include "sift3d_thread_transport.c"
