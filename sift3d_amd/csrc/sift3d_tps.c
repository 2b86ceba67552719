/* sift3d_tps.c -- thin-plate spline: the fit, its evaluation in double, the device layout, and the
 * blocking warp of host images (included at the end of sift3d_host.c).  Contract: include/sift3d_amd.h,
 * "Thin-plate spline"; the device kernel is sift3d_hip_warp_tps (sift3d_warp.hip).
 *
 * The fit solves the saddle system [Phi + lambda I, P; P^T, 0] [w; a] = [y; 0] without LAPACK:
 *   1. Householder QR of P = [1 x y z] (m x 4): Q^T P = [R; 0], Q = H0 H1 H2 H3;
 *   2. B = Q^T (Phi + lambda I) Q, by two-sided rank-2 updates, one per reflector;
 *   3. w = Q [0; g] with B22 g = (Q^T y)[4:], B22 = B[4:, 4:] positive definite for distinct, non-coplanar
 *      points and lambda >= 0 (phi(r) = -r is conditionally positive definite): Cholesky;
 *   4. R a = (Q^T y)[:4] - B[:4, 4:] g.
 * Steps 2 and 3 are O(m^2) and O(m^3 / 3); both run on an explicit OpenMP team of at most 16 threads, and
 * every element is computed by one thread in a fixed order, so the result does not depend on the team. */

static int tps_threads(void)
{
    int t = omp_get_num_procs();
    if (t > 16)
        t = 16;
    return t < 1 ? 1 : t;
}

static double tps_dist(const double *a, const double *b)
{
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

typedef struct {
    double x, y, z;
    int i;
} tps_key;

static int tps_key_cmp(const void *pa, const void *pb)
{
    const tps_key *a = (const tps_key *)pa, *b = (const tps_key *)pb;
    if (a->x != b->x)
        return a->x < b->x ? -1 : 1;
    if (a->y != b->y)
        return a->y < b->y ? -1 : 1;
    if (a->z != b->z)
        return a->z < b->z ? -1 : 1;
    return (a->i > b->i) - (a->i < b->i);
}

/* keep[0 .. count-1] = the indices of the distinct src points, ascending (of equal points the lowest
 * index is kept); returns count, or -1 when out of memory */
static int tps_distinct(const double *src, int n, int *keep)
{
    tps_key *k = (tps_key *)malloc(sizeof(tps_key) * (size_t)n);
    unsigned char *dup = (unsigned char *)calloc((size_t)n, 1);
    int i, cnt = 0;
    if (!k || !dup) {
        free(k);
        free(dup);
        return -1;
    }
    for (i = 0; i < n; i++) {
        k[i].x = src[3 * (size_t)i];
        k[i].y = src[3 * (size_t)i + 1];
        k[i].z = src[3 * (size_t)i + 2];
        k[i].i = i;
    }
    qsort(k, (size_t)n, sizeof(tps_key), tps_key_cmp);
    for (i = 1; i < n; i++)
        if (k[i].x == k[i - 1].x && k[i].y == k[i - 1].y && k[i].z == k[i - 1].z)
            dup[k[i].i] = 1;           /* a run is sorted by index: its first element stays */
    for (i = 0; i < n; i++)
        if (!dup[i])
            keep[cnt++] = i;
    free(k);
    free(dup);
    return cnt;
}

/* greedy farthest-point sampling of mmax of the nc points src[cand[j]] (the rule in the header);
 * cand is overwritten with the chosen indices, ascending.  -1 when out of memory. */
static int tps_thin(const double *src, int *cand, int nc, int mmax)
{
    double *d = (double *)malloc(sizeof(double) * (size_t)nc);
    unsigned char *taken = (unsigned char *)calloc((size_t)nc, 1);
    int j, s, cur = 0, cnt = 0;
    if (!d || !taken) {
        free(d);
        free(taken);
        return -1;
    }
    for (j = 0; j < nc; j++)
        d[j] = INFINITY;
    for (s = 0; s < mmax; s++) {
        const double *c = src + 3 * (size_t)cand[cur];
        double bd = -1.0;
        int best = -1;
        taken[cur] = 1;
        if (s == mmax - 1)
            break;
        for (j = 0; j < nc; j++) {
            const double *p = src + 3 * (size_t)cand[j];
            const double dx = p[0] - c[0], dy = p[1] - c[1], dz = p[2] - c[2];
            const double dd = (dx * dx + dy * dy) + dz * dz;
            if (taken[j])
                continue;
            if (dd < d[j])
                d[j] = dd;
            if (d[j] > bd) {           /* strict: the lowest index on ties */
                bd = d[j];
                best = j;
            }
        }
        cur = best;
    }
    for (j = 0; j < nc; j++)
        if (taken[j])
            cand[cnt++] = cand[j];
    free(d);
    free(taken);
    return 0;
}

/* H = I - tau v v^T (v: m entries, zero above k) applied from both sides of the symmetric m x m K:
 * K <- H K H = K - v q^T - q v^T with p = tau K v, q = p - (tau / 2) (p^T v) v */
static void tps_reflect2(double *K, int m, const double *v, double tau, double *p, int nt)
{
    double pv = 0.0;
    int i;
    if (tau == 0.0)
        return;
#pragma omp parallel for schedule(static) num_threads(nt)
    for (i = 0; i < m; i++) {
        const double *row = K + (size_t)i * m;
        double s = 0.0;
        int j;
        for (j = 0; j < m; j++)
            s += row[j] * v[j];
        p[i] = tau * s;
    }
    for (i = 0; i < m; i++)
        pv += p[i] * v[i];
    for (i = 0; i < m; i++)
        p[i] -= 0.5 * tau * pv * v[i];
#pragma omp parallel for schedule(static) num_threads(nt)
    for (i = 0; i < m; i++) {
        double *row = K + (size_t)i * m;
        int j;
        for (j = 0; j < m; j++)
            row[j] -= v[i] * p[j] + p[i] * v[j];
    }
}

/* H = I - tau v v^T applied to the m x 3 Y from the left */
static void tps_reflect1(double *Y, int m, const double *v, double tau)
{
    int i, d;
    for (d = 0; d < 3; d++) {
        double s = 0.0;
        for (i = 0; i < m; i++)
            s += v[i] * Y[3 * (size_t)i + d];
        s *= tau;
        for (i = 0; i < m; i++)
            Y[3 * (size_t)i + d] -= s * v[i];
    }
}

/* the fit on m distinct points c (m x 3) with values y (m x 3): w (m x 3), A (12).  0, or -1 when P has
 * rank < 4 (coplanar points), the factorisation fails or memory runs out. */
static int tps_solve(const double *c, const double *y, int m, double lambda, double *w, double *A)
{
    const int n2 = m - 4, nt = tps_threads();
    double *K = (double *)malloc(sizeof(double) * (size_t)m * m);
    double *V = (double *)calloc((size_t)4 * m, sizeof(double));   /* reflector k: V + k m */
    double *Y = (double *)malloc(sizeof(double) * 3 * (size_t)m);
    double *P = (double *)malloc(sizeof(double) * 4 * (size_t)m);  /* column-major m x 4 */
    double *tmp = (double *)malloc(sizeof(double) * (size_t)m);
    double tau[4], R[4][4], norm0[4], a[4][3];
    int i, j, k, d, ok = 1;
    if (!K || !V || !Y || !P || !tmp) {
        ok = 0;
        goto done;
    }
    memcpy(Y, y, sizeof(double) * 3 * (size_t)m);
    for (i = 0; i < m; i++) {
        P[i] = 1.0;
        for (k = 0; k < 3; k++)
            P[(size_t)(k + 1) * m + i] = c[3 * (size_t)i + k];
    }
    for (k = 0; k < 4; k++) {
        double s = 0.0;
        for (i = 0; i < m; i++)
            s += P[(size_t)k * m + i] * P[(size_t)k * m + i];
        norm0[k] = sqrt(s);
    }
    /* 1. Householder QR of P */
    memset(R, 0, sizeof(R));
    for (k = 0; k < 4; k++) {
        double *col = P + (size_t)k * m, *v = V + (size_t)k * m, s = 0.0, alpha, vv = 0.0;
        for (i = k; i < m; i++)
            s += col[i] * col[i];
        alpha = col[k] >= 0.0 ? -sqrt(s) : sqrt(s);
        for (i = k; i < m; i++)
            v[i] = col[i];
        v[k] -= alpha;
        for (i = k; i < m; i++)
            vv += v[i] * v[i];
        if (!(fabs(alpha) > 1e-9 * norm0[k]) || !(vv > 0.0)) {
            ok = 0;                                      /* rank < 4: coplanar (or collinear) points */
            goto done;
        }
        tau[k] = 2.0 / vv;
        R[k][k] = alpha;
        for (j = k + 1; j < 4; j++) {
            double *cj = P + (size_t)j * m, t = 0.0;
            for (i = k; i < m; i++)
                t += v[i] * cj[i];
            t *= tau[k];
            for (i = k; i < m; i++)
                cj[i] -= t * v[i];
            R[k][j] = cj[k];
        }
    }
    /* 2. B = Q^T (Phi + lambda I) Q, Q^T y */
#pragma omp parallel for schedule(static) num_threads(nt)
    for (i = 0; i < m; i++) {
        int jj;
        for (jj = 0; jj < m; jj++)
            K[(size_t)i * m + jj] = (i == jj ? lambda : 0.0) - tps_dist(c + 3 * (size_t)i, c + 3 * (size_t)jj);
    }
    for (k = 0; k < 4; k++) {
        tps_reflect2(K, m, V + (size_t)k * m, tau[k], tmp, nt);
        tps_reflect1(Y, m, V + (size_t)k * m, tau[k]);
    }
    /* 3. Cholesky of B22 = K[4:, 4:] in place (lower triangle, row-major with stride m) */
    {
        double *B = K + 4 * (size_t)m + 4;
#pragma omp parallel num_threads(nt) private(i, j)
        for (j = 0; j < n2; j++) {
#pragma omp single
            {
                const double *lj = B + (size_t)j * m;
                double s = lj[j];
                int q;
                for (q = 0; q < j; q++)
                    s -= lj[q] * lj[q];
                if (!(s > 0.0) || !isfinite(s))
                    ok = 0;
                else
                    B[(size_t)j * m + j] = sqrt(s);
            }
            if (!ok)
                break;
#pragma omp for schedule(static)
            for (i = j + 1; i < n2; i++) {
                const double *lj = B + (size_t)j * m;
                double *li = B + (size_t)i * m, s = li[j];
                int q;
                for (q = 0; q < j; q++)
                    s -= li[q] * lj[q];
                li[j] = s / lj[j];
            }
        }
        if (!ok)
            goto done;
        /* L L^T g = (Q^T y)[4:], g into Y[4:] */
        for (d = 0; d < 3; d++) {
            for (i = 0; i < n2; i++) {
                const double *li = B + (size_t)i * m;
                double s = Y[3 * (size_t)(4 + i) + d];
                for (j = 0; j < i; j++)
                    s -= li[j] * Y[3 * (size_t)(4 + j) + d];
                Y[3 * (size_t)(4 + i) + d] = s / li[i];
            }
            for (i = n2 - 1; i >= 0; i--) {
                double s = Y[3 * (size_t)(4 + i) + d];
                for (j = i + 1; j < n2; j++)
                    s -= B[(size_t)j * m + i] * Y[3 * (size_t)(4 + j) + d];
                Y[3 * (size_t)(4 + i) + d] = s / B[(size_t)i * m + i];
            }
        }
    }
    /* 4. R a = (Q^T y)[:4] - B[:4, 4:] g */
    for (d = 0; d < 3; d++) {
        double r[4];
        for (k = 0; k < 4; k++) {
            double s = Y[3 * (size_t)k + d];
            for (j = 0; j < n2; j++)
                s -= K[(size_t)k * m + 4 + j] * Y[3 * (size_t)(4 + j) + d];
            r[k] = s;
        }
        for (k = 3; k >= 0; k--) {
            double s = r[k];
            for (j = k + 1; j < 4; j++)
                s -= R[k][j] * a[j][d];
            a[k][d] = s / R[k][k];
        }
    }
    /* w = Q [0; g] = H0 H1 H2 H3 [0; g] */
    for (d = 0; d < 3; d++)
        for (i = 0; i < 4; i++)
            Y[3 * (size_t)i + d] = 0.0;
    for (k = 3; k >= 0; k--)
        tps_reflect1(Y, m, V + (size_t)k * m, tau[k]);
    for (i = 0; i < 3 * m; i++)
        if (!isfinite(Y[i]))
            ok = 0;
    for (d = 0; d < 3; d++) {
        A[4 * d + 0] = a[1][d];
        A[4 * d + 1] = a[2][d];
        A[4 * d + 2] = a[3][d];
        A[4 * d + 3] = a[0][d];
    }
    for (i = 0; i < 12; i++)
        if (!isfinite(A[i]))
            ok = 0;
    if (ok)
        memcpy(w, Y, sizeof(double) * 3 * (size_t)m);
done:
    free(K);
    free(V);
    free(Y);
    free(P);
    free(tmp);
    return ok ? 0 : -1;
}

int sift3d_amd_tps_fit(const double *src, const double *dst, int n, double smoothing, int max_points,
                       double *ctrl, double *weights, double *A, int *m)
{
    int *idx = NULL, cnt, mm, i, k, rc = SIFT3D_FAILURE;
    double *c = NULL, *y = NULL, *w = NULL, a[12];
    if (!src || !dst || !ctrl || !weights || !A || !m) {
        ERR("sift3d_amd_tps_fit: NULL argument \n");
        return SIFT3D_FAILURE;
    }
    if (n < 5 || max_points < 5 || max_points > SIFT3D_AMD_TPS_MAX_POINTS) {
        ERR("sift3d_amd_tps_fit: need n >= 5 and 5 <= max_points <= %d \n", SIFT3D_AMD_TPS_MAX_POINTS);
        return SIFT3D_FAILURE;
    }
    if (!isfinite(smoothing) || smoothing < 0.0) {
        ERR("sift3d_amd_tps_fit: the smoothing must be finite and >= 0 \n");
        return SIFT3D_FAILURE;
    }
    for (i = 0; i < 3 * n; i++)
        if (!isfinite(src[i]) || !isfinite(dst[i])) {
            ERR("sift3d_amd_tps_fit: the points are not finite \n");
            return SIFT3D_FAILURE;
        }
    idx = (int *)malloc(sizeof(int) * (size_t)n);
    if (!idx || (cnt = tps_distinct(src, n, idx)) < 0)
        goto done;
    if (cnt < 5) {
        ERR("sift3d_amd_tps_fit: fewer than 5 distinct points \n");
        goto done;
    }
    mm = cnt;
    if (cnt > max_points) {
        if (tps_thin(src, idx, cnt, max_points))
            goto done;
        mm = max_points;
    }
    c = (double *)malloc(sizeof(double) * 3 * (size_t)mm);
    y = (double *)malloc(sizeof(double) * 3 * (size_t)mm);
    w = (double *)malloc(sizeof(double) * 3 * (size_t)mm);
    if (!c || !y || !w)
        goto done;
    for (i = 0; i < mm; i++)
        for (k = 0; k < 3; k++) {
            c[3 * (size_t)i + k] = src[3 * (size_t)idx[i] + k];
            y[3 * (size_t)i + k] = dst[3 * (size_t)idx[i] + k];
        }
    if (tps_solve(c, y, mm, smoothing, w, a)) {
        ERR("sift3d_amd_tps_fit: coplanar control points or a failed factorisation \n");
        goto done;
    }
    memcpy(ctrl, c, sizeof(double) * 3 * (size_t)mm);
    memcpy(weights, w, sizeof(double) * 3 * (size_t)mm);
    memcpy(A, a, sizeof(a));
    *m = mm;
    rc = SIFT3D_SUCCESS;
done:
    free(idx);
    free(c);
    free(y);
    free(w);
    return rc;
}

int sift3d_amd_tps_apply(const double *ctrl, const double *weights, const double *A, int m, const double *p,
                         int n, double *q)
{
    int j;
    if (!ctrl || !weights || !A || !p || !q || m < 1 || n < 0)
        return SIFT3D_FAILURE;
#pragma omp parallel for schedule(static) num_threads(tps_threads())
    for (j = 0; j < n; j++) {
        const double *pj = p + 3 * (size_t)j;
        double s[3] = {0.0, 0.0, 0.0};
        int i, d;
        for (i = 0; i < m; i++) {
            const double phi = -tps_dist(pj, ctrl + 3 * (size_t)i);
            for (d = 0; d < 3; d++)
                s[d] += weights[3 * (size_t)i + d] * phi;
        }
        for (d = 0; d < 3; d++)
            q[3 * (size_t)j + d] = A[4 * d] * pj[0] + ((A[4 * d + 1] * pj[1] + A[4 * d + 2] * pj[2]) + A[4 * d + 3]) + s[d];
    }
    return SIFT3D_SUCCESS;
}

int sift3d_amd_tps_pack(const double *ctrl, const double *weights, int m, float *out)
{
    int i, k;
    if (!ctrl || !weights || !out || m < 1 || m > SIFT3D_AMD_TPS_MAX_POINTS)
        return SIFT3D_FAILURE;
    for (i = 0; i < 3 * m; i++)
        if (!isfinite((float)ctrl[i]) || !isfinite((float)weights[i]))
            return SIFT3D_FAILURE;
    for (i = 0; i < m; i++) {
        float *o = out + (size_t)SIFT3D_AMD_TPS_FLOATS * i;
        for (k = 0; k < 3; k++) {
            o[k] = (float)ctrl[3 * (size_t)i + k];
            o[4 + k] = -(float)weights[3 * (size_t)i + k];
        }
        o[3] = 0.0f;
        o[7] = 0.0f;
    }
    return SIFT3D_SUCCESS;
}

int sift3d_amd_image_warp_tps(const sift3d_image *src, const double *A, const float *tps, int m, int interp,
                              float fill, sift3d_image *dst)
{
    float *d_src = NULL, *d_dst = NULL, *d_tps = NULL;
    size_t ns, nd, nc;
    int i, rc = SIFT3D_FAILURE;
    if (!src || !dst || !A || !tps || !src->data || !dst->data) {
        ERR("sift3d_amd_image_warp_tps: NULL argument \n");
        return SIFT3D_FAILURE;
    }
    if (src->nc != 1 || dst->nc != 1) {
        ERR("sift3d_amd_image_warp_tps: only single-channel images are supported \n");
        return SIFT3D_FAILURE;
    }
    if (src->nx <= 0 || src->ny <= 0 || src->nz <= 0 || dst->nx <= 0 || dst->ny <= 0 || dst->nz <= 0) {
        ERR("sift3d_amd_image_warp_tps: dimensions must be positive \n");
        return SIFT3D_FAILURE;
    }
    if (m < 1 || m > SIFT3D_AMD_TPS_MAX_POINTS) {
        ERR("sift3d_amd_image_warp_tps: the number of control points must be in [1, %d] \n",
            SIFT3D_AMD_TPS_MAX_POINTS);
        return SIFT3D_FAILURE;
    }
    if (interp != SIFT3D_AMD_INTERP_NEAREST && interp != SIFT3D_AMD_INTERP_LINEAR) {
        ERR("sift3d_amd_image_warp_tps: unknown interpolation mode %d \n", interp);
        return SIFT3D_FAILURE;
    }
    for (i = 0; i < 12; i++)
        if (!isfinite(A[i])) {
            ERR("sift3d_amd_image_warp_tps: the affine map is not finite \n");
            return SIFT3D_FAILURE;
        }
    for (i = 0; i < SIFT3D_AMD_TPS_FLOATS * m; i++)
        if (!isfinite(tps[i])) {
            ERR("sift3d_amd_image_warp_tps: the control points or weights are not finite \n");
            return SIFT3D_FAILURE;
        }
    if (!sift3d_amd_device_available()) {
        ERR("sift3d_amd: no HIP device is available; this library has no CPU path \n");
        return SIFT3D_FAILURE;
    }
    ns = sizeof(float) * (size_t)src->nx * src->ny * src->nz;
    nd = sizeof(float) * (size_t)dst->nx * dst->ny * dst->nz;
    nc = sizeof(float) * SIFT3D_AMD_TPS_FLOATS * (size_t)m;
    d_src = (float *)sift3d_hip_malloc(ns);
    d_dst = (float *)sift3d_hip_malloc(nd);
    d_tps = (float *)sift3d_hip_malloc(nc);
    if (d_src && d_dst && d_tps && !sift3d_hip_memcpy_h2d(d_src, src->data, ns, NULL) &&
        !sift3d_hip_memcpy_h2d(d_tps, tps, nc, NULL) &&
        !sift3d_hip_warp_tps(d_src, src->nx, src->ny, src->nz, d_dst, dst->nx, dst->ny, dst->nz, A, d_tps, m,
                             interp, fill, NULL) &&
        !sift3d_hip_memcpy_d2h(dst->data, d_dst, nd, NULL) && !sift3d_hip_stream_sync(NULL))
        rc = SIFT3D_SUCCESS;
    sift3d_hip_free(d_src);
    sift3d_hip_free(d_dst);
    sift3d_hip_free(d_tps);
    return rc;
}
