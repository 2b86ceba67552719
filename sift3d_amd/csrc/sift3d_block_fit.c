/* sift3d_block_fit.c -- block matching: the checked entry of the matching kernel, the trimmed (LTS) point-pair fit
 * and the coarse-to-fine driver that iterates warp, match and fit (included at the end of sift3d_host.c, after
 * sift3d_affine_refine.c, whose corner distance and mask pyramid it uses as they are).
 *
 * The contract is in include/sift3d_amd.h, "Block matching".  The kernel is sift3d_block_match.hip's, reached through
 * the launcher below after the checks here.  Arguments are checked before the device is touched, so bad input is
 * refused on a machine without a GPU too. */

int sift3d_block_match_launch(const float *d_F, int nx, int ny, int nz, const float *d_W, const float *d_VF,
                              const float *d_VW, int radius, float *d_disp, float *d_cc, double *d_var, void *stream);
int sift3d_block_fill_launch(float *d_dst, size_t n, float value, void *stream);

static int check_block_radius(const char *what, int radius)
{
    return radius < 1 || radius > SIFT3D_AMD_BLOCK_MAX_RADIUS
               ? refuse(what, "radius must be in [1, SIFT3D_AMD_BLOCK_MAX_RADIUS]") : SIFT3D_SUCCESS;
}

size_t sift3d_amd_block_match_work_bytes(int nx, int ny, int nz, int radius)
{
    return 0;
}

int sift3d_hip_block_match(const float *d_F, int nx, int ny, int nz, const float *d_W, const float *d_VF,
                           const float *d_VW, int radius, float *d_disp, float *d_cc, double *d_var, void *d_work,
                           void *stream)
{
    static const char what[] = "sift3d_hip_block_match";
    size_t nb;
    if (!d_F || !d_W || !d_disp || !d_cc || !d_var)
        return refuse(what, "NULL argument");
    if (check_dims(what, nx, ny, nz))
        return SIFT3D_FAILURE;
    if (nx < 4 || ny < 4 || nz < 4)
        return refuse(what, "every dimension must hold a block of 4 voxels");
    if (check_block_radius(what, radius) ||
        check_aligned(what, ADDR(d_var), ADDR(d_F) | ADDR(d_W) | ADDR(d_VF) | ADDR(d_VW) | ADDR(d_disp) | ADDR(d_cc)))
        return SIFT3D_FAILURE;
    nb = grid_voxels(nx / 4, ny / 4, nz / 4);
    {
        const size_t vol = image_bytes(nx, ny, nz, 1);
        const range_t in[] = { { d_F, vol }, { d_W, vol }, { d_VF, d_VF ? vol : 0 }, { d_VW, d_VW ? vol : 0 } };
        const range_t out[] = { { d_disp, 3 * nb * sizeof(float) }, { d_cc, nb * sizeof(float) },
                                { d_var, nb * sizeof(double) } };
        if (ranges_aliased(out, 3, in, 4))
            return refuse(what, ALIASED);
    }
    return sift3d_block_match_launch(d_F, nx, ny, nz, d_W, d_VF, d_VW, radius, d_disp, d_cc, d_var, stream);
}

/* ---- the trimmed fit ---- */

static const int FIT_NMIN[3] = { 1, 3, 4 };
#define FIT_DEGENERATE 1e-10

static int fit_threads(int n)
{
    int t = omp_get_num_procs();
    if (t > 16)
        t = 16;
    if (t > (n + 4095) / 4096)
        t = (n + 4095) / 4096;
    return t < 1 ? 1 : t;
}

/* eigenvalues (on the diagonal of a) and eigenvectors (the columns of v) of the symmetric m x m matrix a, m <= 4, by
 * cyclic Jacobi rotations */
static void jacobi_eig(double *a, int m, double *v)
{
    int sweep, p, q, k;
    for (p = 0; p < m; p++)
        for (q = 0; q < m; q++)
            v[p * m + q] = p == q ? 1.0 : 0.0;
    for (sweep = 0; sweep < 64; sweep++) {
        double off = 0.0, diag = 0.0;
        for (p = 0; p < m; p++) {
            diag += a[p * m + p] * a[p * m + p];
            for (q = p + 1; q < m; q++)
                off += a[p * m + q] * a[p * m + q];
        }
        if (!(off > 1e-40 * diag))
            break;
        for (p = 0; p < m; p++)
            for (q = p + 1; q < m; q++) {
                const double apq = a[p * m + q];
                double theta, t, c, s;
                if (apq == 0.0)
                    continue;
                theta = (a[q * m + q] - a[p * m + p]) / (2.0 * apq);
                t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                c = 1.0 / sqrt(t * t + 1.0);
                s = t * c;
                for (k = 0; k < m; k++) {                    /* columns p, q */
                    const double akp = a[k * m + p], akq = a[k * m + q];
                    a[k * m + p] = c * akp - s * akq;
                    a[k * m + q] = s * akp + c * akq;
                }
                for (k = 0; k < m; k++) {                    /* rows p, q */
                    const double apk = a[p * m + k], aqk = a[q * m + k];
                    a[p * m + k] = c * apk - s * aqk;
                    a[q * m + k] = s * apk + c * aqk;
                }
                for (k = 0; k < m; k++) {
                    const double vkp = v[k * m + p], vkq = v[k * m + q];
                    v[k * m + p] = c * vkp - s * vkq;
                    v[k * m + q] = s * vkp + c * vkq;
                }
            }
    }
}

/* the contract's degeneracy test on a 3 x 3 scatter matrix: rank below `need` (2: collinear, 3: coplanar) */
static int scatter_degenerate(const double S[3][3], int need)
{
    double a[9], v[9], l[3], t;
    int i, j;
    for (i = 0; i < 3; i++)
        for (j = 0; j < 3; j++)
            a[3 * i + j] = S[i][j];
    jacobi_eig(a, 3, v);
    for (i = 0; i < 3; i++)
        l[i] = a[4 * i];
    for (i = 0; i < 3; i++)                                  /* descending */
        for (j = i + 1; j < 3; j++)
            if (l[j] > l[i]) {
                t = l[i]; l[i] = l[j]; l[j] = t;
            }
    return !(l[0] > 0.0) || !(l[need - 1] > FIT_DEGENERATE * l[0]);
}

/* y ~ L x + t on the pairs with sel[i] != 0 (cnt of them), x = ss * src, y = sd * dst; sums serial, in index order */
static int fit_model(const double *src, const double *dst, int n, const unsigned char *sel, int cnt, int model,
                     const double *ss, const double *sd, double L[3][3], double t[3])
{
    double cx[3] = { 0, 0, 0 }, cy[3] = { 0, 0, 0 }, Sxx[3][3], Syy[3][3], Sxy[3][3];
    int i, a, b;
    for (i = 0; i < n; i++)
        if (sel[i])
            for (a = 0; a < 3; a++) {
                cx[a] += ss[a] * src[3 * (size_t)i + a];
                cy[a] += sd[a] * dst[3 * (size_t)i + a];
            }
    for (a = 0; a < 3; a++) {
        cx[a] /= cnt;
        cy[a] /= cnt;
    }
    memset(L, 0, 9 * sizeof(double));
    L[0][0] = L[1][1] = L[2][2] = 1.0;
    if (model != SIFT3D_AMD_MODEL_TRANSLATION) {
        memset(Sxx, 0, sizeof(Sxx));
        memset(Syy, 0, sizeof(Syy));
        memset(Sxy, 0, sizeof(Sxy));
        for (i = 0; i < n; i++)
            if (sel[i]) {
                double x[3], y[3];
                for (a = 0; a < 3; a++) {
                    x[a] = ss[a] * src[3 * (size_t)i + a] - cx[a];
                    y[a] = sd[a] * dst[3 * (size_t)i + a] - cy[a];
                }
                for (a = 0; a < 3; a++)
                    for (b = 0; b < 3; b++) {
                        Sxx[a][b] += x[a] * x[b];
                        Syy[a][b] += y[a] * y[b];
                        Sxy[a][b] += x[a] * y[b];
                    }
            }
    }
    if (model == SIFT3D_AMD_MODEL_RIGID) {
        /* Horn 1987: the unit quaternion of the rotation x -> y is the dominant eigenvector of N(Sxy) */
        double N[16], V[16], q[4], nq;
        int best = 0;
        if (scatter_degenerate(Sxx, 2) || scatter_degenerate(Syy, 2))
            return SIFT3D_FAILURE;
        N[0] = Sxy[0][0] + Sxy[1][1] + Sxy[2][2];
        N[1] = N[4] = Sxy[1][2] - Sxy[2][1];
        N[2] = N[8] = Sxy[2][0] - Sxy[0][2];
        N[3] = N[12] = Sxy[0][1] - Sxy[1][0];
        N[5] = Sxy[0][0] - Sxy[1][1] - Sxy[2][2];
        N[6] = N[9] = Sxy[0][1] + Sxy[1][0];
        N[7] = N[13] = Sxy[2][0] + Sxy[0][2];
        N[10] = -Sxy[0][0] + Sxy[1][1] - Sxy[2][2];
        N[11] = N[14] = Sxy[1][2] + Sxy[2][1];
        N[15] = -Sxy[0][0] - Sxy[1][1] + Sxy[2][2];
        jacobi_eig(N, 4, V);
        for (a = 1; a < 4; a++)
            if (N[5 * a] > N[5 * best])
                best = a;
        for (a = 0; a < 4; a++)
            q[a] = V[4 * a + best];
        nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        if (!(nq > 0.0) || !isfinite(nq))
            return SIFT3D_FAILURE;
        for (a = 0; a < 4; a++)
            q[a] /= nq;
        L[0][0] = q[0] * q[0] + q[1] * q[1] - q[2] * q[2] - q[3] * q[3];
        L[0][1] = 2.0 * (q[1] * q[2] - q[0] * q[3]);
        L[0][2] = 2.0 * (q[1] * q[3] + q[0] * q[2]);
        L[1][0] = 2.0 * (q[2] * q[1] + q[0] * q[3]);
        L[1][1] = q[0] * q[0] - q[1] * q[1] + q[2] * q[2] - q[3] * q[3];
        L[1][2] = 2.0 * (q[2] * q[3] - q[0] * q[1]);
        L[2][0] = 2.0 * (q[3] * q[1] - q[0] * q[2]);
        L[2][1] = 2.0 * (q[3] * q[2] + q[0] * q[1]);
        L[2][2] = q[0] * q[0] - q[1] * q[1] - q[2] * q[2] + q[3] * q[3];
    } else if (model == SIFT3D_AMD_MODEL_AFFINE) {
        /* L = Syx Sxx^-1 by the adjugate of the symmetric 3 x 3 Sxx */
        double adj[3][3], det;
        if (scatter_degenerate(Sxx, 3))
            return SIFT3D_FAILURE;
        adj[0][0] = Sxx[1][1] * Sxx[2][2] - Sxx[1][2] * Sxx[2][1];
        adj[0][1] = Sxx[0][2] * Sxx[2][1] - Sxx[0][1] * Sxx[2][2];
        adj[0][2] = Sxx[0][1] * Sxx[1][2] - Sxx[0][2] * Sxx[1][1];
        adj[1][1] = Sxx[0][0] * Sxx[2][2] - Sxx[0][2] * Sxx[2][0];
        adj[1][2] = Sxx[0][2] * Sxx[1][0] - Sxx[0][0] * Sxx[1][2];
        adj[2][2] = Sxx[0][0] * Sxx[1][1] - Sxx[0][1] * Sxx[1][0];
        adj[1][0] = adj[0][1];
        adj[2][0] = adj[0][2];
        adj[2][1] = adj[1][2];
        det = Sxx[0][0] * adj[0][0] + Sxx[0][1] * adj[1][0] + Sxx[0][2] * adj[2][0];
        if (!(det > 0.0) || !isfinite(det))
            return SIFT3D_FAILURE;
        for (a = 0; a < 3; a++)
            for (b = 0; b < 3; b++)                          /* Syx[a][j] = Sxy[j][a] */
                L[a][b] = (Sxy[0][a] * adj[0][b] + Sxy[1][a] * adj[1][b] + Sxy[2][a] * adj[2][b]) / det;
    }
    for (a = 0; a < 3; a++) {
        t[a] = cy[a] - (L[a][0] * cx[0] + L[a][1] * cx[1] + L[a][2] * cx[2]);
        if (!isfinite(t[a]) || !isfinite(L[a][0]) || !isfinite(L[a][1]) || !isfinite(L[a][2]))
            return SIFT3D_FAILURE;
    }
    return SIFT3D_SUCCESS;
}

static void fit_residuals(const double *src, const double *dst, int n, const double *ss, const double *sd,
                          double L[3][3], const double t[3], double *r)
{
    int i;
#pragma omp parallel for schedule(static) num_threads(fit_threads(n))
    for (i = 0; i < n; i++) {
        const double x0 = ss[0] * src[3 * (size_t)i], x1 = ss[1] * src[3 * (size_t)i + 1],
                     x2 = ss[2] * src[3 * (size_t)i + 2];
        double s = 0.0;
        int a;
        for (a = 0; a < 3; a++) {
            const double e = (L[a][0] * x0 + L[a][1] * x1 + L[a][2] * x2 + t[a]) - sd[a] * dst[3 * (size_t)i + a];
            s += e * e;
        }
        r[i] = s;
    }
}

/* sel[i] = 1 for the k entries of smallest (key, index), 0 for the others; idx: n ints of scratch.  Quickselect on the
 * total order (key, then index), so ties go to the lower index. */
static int key_less(const double *key, int a, int b)
{
    return key[a] < key[b] || (key[a] == key[b] && a < b);
}

static void select_smallest(const double *key, int n, int k, int *idx, unsigned char *sel)
{
    int lo = 0, hi = n - 1, i;
    for (i = 0; i < n; i++)
        idx[i] = i;
    while (lo < hi) {                                        /* idx[0 .. k-1] become the k smallest */
        const int mid = lo + (hi - lo) / 2;
        int pv, a = lo, b = hi, tmp;
        /* median of three as the pivot */
        if (key_less(key, idx[mid], idx[lo])) { tmp = idx[mid]; idx[mid] = idx[lo]; idx[lo] = tmp; }
        if (key_less(key, idx[hi], idx[lo])) { tmp = idx[hi]; idx[hi] = idx[lo]; idx[lo] = tmp; }
        if (key_less(key, idx[hi], idx[mid])) { tmp = idx[hi]; idx[hi] = idx[mid]; idx[mid] = tmp; }
        pv = idx[mid];
        while (a <= b) {
            while (key_less(key, idx[a], pv))
                a++;
            while (key_less(key, pv, idx[b]))
                b--;
            if (a <= b) {
                tmp = idx[a]; idx[a] = idx[b]; idx[b] = tmp;
                a++;
                b--;
            }
        }
        if (k - 1 <= b)
            hi = b;
        else if (k - 1 >= a)
            lo = a;
        else
            break;
    }
    memset(sel, 0, (size_t)n);
    for (i = 0; i < k; i++)
        sel[idx[i]] = 1;
}

int sift3d_amd_fit_trimmed(const double *src, const double *dst, int n, int model, double keep, int max_iter,
                           const double *scale_src, const double *scale_dst, double *T, unsigned char *used,
                           int *iterations)
{
    static const char what[] = "sift3d_amd_fit_trimmed";
    static const double one[3] = { 1.0, 1.0, 1.0 };
    const double *ss = scale_src ? scale_src : one, *sd = scale_dst ? scale_dst : one;
    double L[3][3], t[3], *r = NULL;
    unsigned char *cur = NULL, *next = NULL;
    int *idx = NULL;
    int i, a, b, k, refits = 0, rc = SIFT3D_FAILURE;
    if (!src || !dst || !T || !iterations)
        return refuse(what, "NULL argument");
    if (model != SIFT3D_AMD_MODEL_TRANSLATION && model != SIFT3D_AMD_MODEL_RIGID && model != SIFT3D_AMD_MODEL_AFFINE)
        return refuse(what, "unknown model");
    if (n < FIT_NMIN[model])
        return refuse(what, "too few point pairs for the model");
    if (!(keep > 0.0 && keep <= 1.0))
        return refuse(what, "keep must be in (0, 1]");
    if (max_iter < 0)
        return refuse(what, "max_iter must not be negative");
    for (a = 0; a < 3; a++)
        if (!(ss[a] > 0.0) || !isfinite(ss[a]) || !(sd[a] > 0.0) || !isfinite(sd[a]))
            return refuse(what, "the scales must be positive and finite");
    for (i = 0; i < n; i++)
        for (a = 0; a < 3; a++)
            if (!isfinite(src[3 * (size_t)i + a]) || !isfinite(dst[3 * (size_t)i + a]))
                return refuse(what, "the points are not finite");
    *iterations = 0;
    k = (int)ceil(keep * (double)n);
    if (k < FIT_NMIN[model])
        k = FIT_NMIN[model];
    if (k > n)
        k = n;
    r = (double *)malloc((size_t)n * sizeof(double));
    cur = (unsigned char *)malloc((size_t)n);
    next = (unsigned char *)malloc((size_t)n);
    idx = (int *)malloc((size_t)n * sizeof(int));
    if (!r || !cur || !next || !idx) {
        refuse(what, "out of memory");
        goto done;
    }
    memset(cur, 1, (size_t)n);
    if (fit_model(src, dst, n, cur, n, model, ss, sd, L, t)) {
        refuse(what, "the point set is degenerate for the model");
        goto done;
    }
    for (;;) {
        unsigned char *swap;
        fit_residuals(src, dst, n, ss, sd, L, t, r);
        select_smallest(r, n, k, idx, next);
        if (memcmp(cur, next, (size_t)n) == 0 || refits >= max_iter)
            break;
        swap = cur; cur = next; next = swap;
        if (fit_model(src, dst, n, cur, k, model, ss, sd, L, t)) {
            refuse(what, "the kept point set is degenerate for the model");
            goto done;
        }
        refits++;
    }
    for (a = 0; a < 3; a++) {
        for (b = 0; b < 3; b++)
            T[4 * a + b] = L[a][b] * ss[b] / sd[a];
        T[4 * a + 3] = t[a] / sd[a];
    }
    if (used)
        memcpy(used, cur, (size_t)n);
    *iterations = refits;
    rc = SIFT3D_SUCCESS;
done:
    free(r);
    free(cur);
    free(next);
    free(idx);
    return rc;
}

/* ---- the driver ---- */

void sift3d_amd_block_register_default_params(sift3d_amd_block_register_params *p)
{
    int a;
    if (!p)
        return;
    p->model = SIFT3D_AMD_MODEL_RIGID;
    p->levels = 3;
    p->iterations = 5;
    p->radius = 3;
    p->keep_blocks = 0.5;
    p->keep_inliers = 0.5;
    p->tol = 0.01;
    for (a = 0; a < 3; a++)
        p->spacing_fixed[a] = p->spacing_moving[a] = 1.0;
}

size_t sift3d_amd_block_register_struct_bytes(int which)
{
    switch (which) {
    case 0: return sizeof(sift3d_amd_block_register_params);
    case 1: return sizeof(sift3d_amd_block_iteration);
    case 2: return sizeof(sift3d_amd_block_register_result);
    case 3: return SIFT3D_AMD_BLOCK_MAX_ITERATIONS;
    case 4: return SIFT3D_AMD_BLOCK_MAX_RADIUS;
    default: return 0;
    }
}

/* The scratch, as offsets in floats into d_work: the records of level 0's blocks (var: doubles, first, so 8-byte
 * aligned; disp; cc), W and V_W on level 0's fixed grid, the ones on level 0's moving grid (absent with a moving
 * mask), then per level l >= 1 the restricted fixed and moving volumes and, where given, masks, in the order of the
 * mask pyramid of sift3d_affine_refine.c.  The size function and the driver both read it from here. */
typedef struct {
    size_t var, disp, cc, W, VW, ones, levels;
} block_layout;

static block_layout block_layout_of(int ox, int oy, int oz, int nx, int ny, int nz, int mask_moving)
{
    const size_t b0 = grid_voxels(ox / 4, oy / 4, oz / 4), n0 = pad4(grid_voxels(ox, oy, oz));
    block_layout l;
    l.var = 0;
    l.disp = 2 * b0;
    l.cc = 5 * b0;
    l.W = pad4(6 * b0);
    l.VW = l.W + n0;
    l.ones = l.VW + n0;
    l.levels = l.ones + (mask_moving ? 0 : pad4(grid_voxels(nx, ny, nz)));
    return l;
}

size_t sift3d_amd_block_register_work_floats(int ox, int oy, int oz, int nx, int ny, int nz, int levels, int mask_fixed,
                                             int mask_moving)
{
    size_t total;
    int l;
    if (ox <= 0 || oy <= 0 || oz <= 0 || nx <= 0 || ny <= 0 || nz <= 0 || levels < 1 ||
        levels > SIFT3D_AMD_DEMONS_MAX_LEVELS)
        return 0;
    if (ox < 8 || oy < 8 || oz < 8)
        return 0;
    total = block_layout_of(ox, oy, oz, nx, ny, nz, mask_moving).levels;
    for (l = 1; l < levels; l++) {
        ox = multires_half(ox); oy = multires_half(oy); oz = multires_half(oz);
        nx = multires_half(nx); ny = multires_half(ny); nz = multires_half(nz);
        if (ox < 8 || oy < 8 || oz < 8)
            return 0;
        total += (mask_fixed ? 2 : 1) * pad4(grid_voxels(ox, oy, oz)) +
                 (mask_moving ? 2 : 1) * pad4(grid_voxels(nx, ny, nz));
    }
    return total;
}

/* y = A p in sift3d_hip_warp_affine's order of operations */
static void affine_point(const double *A, const double *p, double *y)
{
    int d;
    for (d = 0; d < 3; d++)
        y[d] = A[4 * d] * p[0] + ((A[4 * d + 1] * p[1] + A[4 * d + 2] * p[2]) + A[4 * d + 3]);
}

static int block_params_ok(const sift3d_amd_block_register_params *p)
{
    int a;
    for (a = 0; a < 3; a++)
        if (!(p->spacing_fixed[a] > 0.0) || !isfinite(p->spacing_fixed[a]) || !(p->spacing_moving[a] > 0.0) ||
            !isfinite(p->spacing_moving[a]))
            return 0;
    return (p->model == SIFT3D_AMD_MODEL_TRANSLATION || p->model == SIFT3D_AMD_MODEL_RIGID ||
            p->model == SIFT3D_AMD_MODEL_AFFINE) &&
           p->levels >= 1 && p->levels <= SIFT3D_AMD_DEMONS_MAX_LEVELS && p->iterations >= 1 &&
           p->iterations <= SIFT3D_AMD_BLOCK_MAX_ITERATIONS && p->radius >= 1 &&
           p->radius <= SIFT3D_AMD_BLOCK_MAX_RADIUS && p->keep_blocks > 0.0 && p->keep_blocks <= 1.0 &&
           p->keep_inliers > 0.0 && p->keep_inliers <= 1.0 && isfinite(p->tol) && p->tol >= 0.0;
}

/* the host side of one iteration: selection, pairs, fit and the entry's figures from the records of a level whose
 * fixed grid has (nbx, nby, nbz) blocks.  Returns 0 and A_out, or -1 (FAILED) with the counts it reached. */
typedef struct {
    float *disp, *cc;
    double *var, *key, *src, *dst;
    int *idx, *blocks;
    unsigned char *sel, *used;
} block_host;

static int block_fit_iteration(const sift3d_amd_block_register_params *p, const block_host *h, int nbx, int nby,
                               int nbz, const double *A, sift3d_amd_block_iteration *e)
{
    const size_t nb = grid_voxels(nbx, nby, nbz);
    const int nmin = FIT_NMIN[p->model];
    double L[3][3], t[3], sum_cc = 0.0, sum_r = 0.0;
    int nvalid = 0, nsel, i, its;
    size_t b;
    for (b = 0; b < nb; b++)
        if (h->cc[b] >= 0.0f) {
            h->blocks[nvalid] = (int)b;
            h->key[nvalid] = -h->var[b];                     /* the largest variances: the smallest keys */
            nvalid++;
        }
    e->n_valid = nvalid;
    if (nvalid < nmin)
        return SIFT3D_FAILURE;
    nsel = (int)ceil(p->keep_blocks * (double)nvalid);
    if (nsel > nvalid)
        nsel = nvalid;
    e->n_selected = nsel;
    if (nsel < nmin)
        return SIFT3D_FAILURE;
    select_smallest(h->key, nvalid, nsel, h->idx, h->sel);
    for (i = 0, nsel = 0; i < nvalid; i++)                   /* block-index order */
        if (h->sel[i]) {
            const size_t blk = (size_t)h->blocks[i];
            const int bx = (int)(blk % (size_t)nbx), by = (int)(blk / (size_t)nbx % (size_t)nby),
                      bz = (int)(blk / ((size_t)nbx * nby));
            double *s = h->src + 3 * (size_t)nsel, q[3];
            s[0] = 4.0 * bx + 1.5;
            s[1] = 4.0 * by + 1.5;
            s[2] = 4.0 * bz + 1.5;
            q[0] = s[0] + (double)h->disp[blk];
            q[1] = s[1] + (double)h->disp[nb + blk];
            q[2] = s[2] + (double)h->disp[2 * nb + blk];
            affine_point(A, q, h->dst + 3 * (size_t)nsel);
            h->blocks[nsel] = (int)blk;                      /* nsel <= i: compacts in place */
            nsel++;
        }
    if (sift3d_amd_fit_trimmed(h->src, h->dst, nsel, p->model, p->keep_inliers, 20, p->spacing_fixed,
                               p->spacing_moving, e->A_out, h->used, &its) ||
        check_affine("sift3d_amd_block_register_device", e->A_out))
        return SIFT3D_FAILURE;
    /* the figures of the used pairs, in the fit's scaled units */
    {
        int a, c;
        for (a = 0; a < 3; a++) {
            for (c = 0; c < 3; c++)
                L[a][c] = e->A_out[4 * a + c] * p->spacing_moving[a] / p->spacing_fixed[c];
            t[a] = e->A_out[4 * a + 3] * p->spacing_moving[a];
        }
    }
    fit_residuals(h->src, h->dst, nsel, p->spacing_fixed, p->spacing_moving, L, t, h->key);
    e->n_used = 0;
    for (i = 0; i < nsel; i++)
        if (h->used[i]) {
            e->n_used++;
            sum_cc += (double)h->cc[h->blocks[i]];
            sum_r += h->key[i];
        }
    e->mean_cc = sum_cc / e->n_used;
    e->rms = sqrt(sum_r / e->n_used);
    return SIFT3D_SUCCESS;
}

int sift3d_amd_block_register_device(const float *d_F, int ox, int oy, int oz, const float *d_M, int nx, int ny, int nz,
                                     const float *d_WF, const float *d_WM, double *A_io,
                                     const sift3d_amd_block_register_params *params,
                                     sift3d_amd_block_register_result *result, float *d_work, void *stream)
{
    static const char what[] = "sift3d_amd_block_register_device";
    sift3d_amd_block_register_params prm;
    affine_level lv[SIFT3D_AMD_DEMONS_MAX_LEVELS];
    block_layout at;
    block_host h;
    double A[12];
    char *w = (char *)d_work;
    float *d_W, *d_VW, *d_ones, *d_disp, *d_cc;
    double *d_var;
    size_t need, off, nb0;
    int l, i, enqueued = 0, rc = SIFT3D_FAILURE;
    if (!d_F || !d_M || !A_io || !result || !d_work)
        return refuse(what, "NULL argument");
    if (params)
        prm = *params;
    else
        sift3d_amd_block_register_default_params(&prm);
    if (check_dims(what, ox, oy, oz) || check_dims(what, nx, ny, nz) || check_affine(what, A_io))
        return SIFT3D_FAILURE;
    if (!block_params_ok(&prm))
        return refuse(what, "a parameter is out of range");
    need = sift3d_amd_block_register_work_floats(ox, oy, oz, nx, ny, nz, prm.levels, d_WF != NULL, d_WM != NULL);
    if (!need)
        return refuse(what, "every level's fixed grid must be at least 8 voxels on every axis");
    if (check_aligned(what, ADDR(d_work), ADDR(d_F) | ADDR(d_M) | ADDR(d_WF) | ADDR(d_WM)))
        return SIFT3D_FAILURE;
    {
        const range_t in[] = { { d_F, image_bytes(ox, oy, oz, 1) }, { d_M, image_bytes(nx, ny, nz, 1) },
                               { d_WF, d_WF ? image_bytes(ox, oy, oz, 1) : 0 },
                               { d_WM, d_WM ? image_bytes(nx, ny, nz, 1) : 0 } };
        const range_t out[] = { { d_work, need * sizeof(float) } };
        if (ranges_aliased(out, 1, in, 4))
            return refuse(what, ALIASED);
    }
    result->iterations = 0;
    result->stop = SIFT3D_AMD_BLOCK_STOP_ITERATIONS;
    memcpy(result->A, A_io, sizeof(result->A));

    at = block_layout_of(ox, oy, oz, nx, ny, nz, d_WM != NULL);
    d_var = (double *)(d_work + at.var);
    d_disp = d_work + at.disp;
    d_cc = d_work + at.cc;
    d_W = d_work + at.W;
    d_VW = d_work + at.VW;
    d_ones = d_WM ? NULL : d_work + at.ones;
    off = at.levels * sizeof(float);
    nb0 = grid_voxels(ox / 4, oy / 4, oz / 4);

    memset(&h, 0, sizeof(h));
    h.disp = (float *)malloc(3 * nb0 * sizeof(float));
    h.cc = (float *)malloc(nb0 * sizeof(float));
    h.var = (double *)malloc(nb0 * sizeof(double));
    h.key = (double *)malloc(nb0 * sizeof(double));
    h.src = (double *)malloc(3 * nb0 * sizeof(double));
    h.dst = (double *)malloc(3 * nb0 * sizeof(double));
    h.idx = (int *)malloc(nb0 * sizeof(int));
    h.blocks = (int *)malloc(nb0 * sizeof(int));
    h.sel = (unsigned char *)malloc(nb0);
    h.used = (unsigned char *)malloc(nb0);
    if (!h.disp || !h.cc || !h.var || !h.key || !h.src || !h.dst || !h.idx || !h.blocks || !h.sel || !h.used ||
        nb0 > (size_t)INT32_MAX) {
        refuse(what, "out of memory");
        goto done;
    }

    enqueued = 1;
    if (d_ones && sift3d_block_fill_launch(d_ones, grid_voxels(nx, ny, nz), 1.0f, stream))
        goto done;
    lv[0] = (affine_level){ d_F, d_M, ox, oy, oz, nx, ny, nz, d_WF, d_WM };
    memcpy(A, A_io, sizeof(A));
    for (l = 1; l < prm.levels; l++) {                       /* level l from level l - 1; A's shift halves */
        const affine_level *f = lv + l - 1;
        affine_level *c = lv + l;
        float *cF = (float *)(w + off), *cM;
        *c = (affine_level){ NULL, NULL, multires_half(f->ox), multires_half(f->oy), multires_half(f->oz),
                             multires_half(f->nx), multires_half(f->ny), multires_half(f->nz), NULL, NULL };
        off += pad4(grid_voxels(c->ox, c->oy, c->oz)) * sizeof(float);
        cM = (float *)(w + off);
        off += pad4(grid_voxels(c->nx, c->ny, c->nz)) * sizeof(float);
        if (sift3d_hip_restrict2(f->F, f->ox, f->oy, f->oz, 1, cF, 1.0f, stream) ||
            sift3d_hip_restrict2(f->M, f->nx, f->ny, f->nz, 1, cM, 1.0f, stream))
            goto done;
        c->F = cF;
        c->M = cM;
        if (mask_pyramid_level(f->WF, f->ox, f->oy, f->oz, f->WM, f->nx, f->ny, f->nz, w, &off, &c->WF, &c->WM, stream))
            goto done;
        for (i = 3; i < 12; i += 4)
            A[i] = A[i] * 0.5;
    }
    for (l = prm.levels - 1; l >= 0; l--) {
        const affine_level *v = lv + l;
        const int nbx = v->ox / 4, nby = v->oy / 4, nbz = v->oz / 4;
        const size_t nb = grid_voxels(nbx, nby, nbz);
        int it, stop = SIFT3D_AMD_BLOCK_STOP_ITERATIONS;
        for (it = 0; it < prm.iterations; it++) {
            sift3d_amd_block_iteration *e = result->trail + result->iterations;
            memset(e, 0, sizeof(*e));
            e->level = l;
            memcpy(e->A_in, A, sizeof(A));
            memcpy(e->A_out, A, sizeof(A));
            e->mean_cc = e->rms = e->move = NAN;
            if (sift3d_hip_warp_affine(v->M, v->nx, v->ny, v->nz, d_W, v->ox, v->oy, v->oz, A,
                                       SIFT3D_AMD_INTERP_LINEAR, 0.0f, stream) ||
                sift3d_hip_warp_affine(v->WM ? v->WM : d_ones, v->nx, v->ny, v->nz, d_VW, v->ox, v->oy, v->oz, A,
                                       SIFT3D_AMD_INTERP_NEAREST, 0.0f, stream) ||
                sift3d_hip_block_match(v->F, v->ox, v->oy, v->oz, d_W, v->WF, d_VW, prm.radius, d_disp, d_cc, d_var,
                                       NULL, stream) ||
                sift3d_hip_memcpy_d2h(h.disp, d_disp, 3 * nb * sizeof(float), stream) ||
                sift3d_hip_memcpy_d2h(h.cc, d_cc, nb * sizeof(float), stream) ||
                sift3d_hip_memcpy_d2h(h.var, d_var, nb * sizeof(double), stream) || sift3d_hip_stream_sync(stream))
                goto done;
            result->iterations++;
            if (block_fit_iteration(&prm, &h, nbx, nby, nbz, A, e)) {
                memcpy(e->A_out, A, sizeof(A));
                e->n_used = 0;
                e->mean_cc = e->rms = e->move = NAN;
                stop = SIFT3D_AMD_BLOCK_STOP_FAILED;
                break;
            }
            e->move = affine_corner_move(A, e->A_out, v->ox, v->oy, v->oz);
            memcpy(A, e->A_out, sizeof(A));
            if (e->move < prm.tol) {
                stop = SIFT3D_AMD_BLOCK_STOP_CONVERGED;
                break;
            }
        }
        result->stop = stop;
        if (l > 0)
            for (i = 3; i < 12; i += 4)
                A[i] = A[i] * 2.0;
    }
    memcpy(A_io, A, sizeof(A));
    memcpy(result->A, A, sizeof(A));
    rc = SIFT3D_SUCCESS;
done:
    if (rc && enqueued)
        sift3d_hip_stream_sync(stream);                      /* no copy into the host records is left pending */
    free(h.disp); free(h.cc); free(h.var); free(h.key); free(h.src); free(h.dst);
    free(h.idx); free(h.blocks); free(h.sel); free(h.used);
    return rc;
}
