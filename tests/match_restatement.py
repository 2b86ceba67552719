"""numpy restatement of descriptor matching and the RANSAC affine fit (sift3d_match.hip, sift3d_register.c).

Both translation units build with -ffp-contract=off, and v_mfma_f32_32x32x2_f32 is a k-ordered f32 fma chain,
D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)) with k0 the lane half l >> 5 == 0.  So every value sift3d_hip_nn2 returns
and every decision of the matcher and of RANSAC is restated here bit for bit:

  nn2       k_row_norms (64 lane partials, then the xor butterfly), the fma chain of k_nn2 in the k order of its
            group() (per group of 8: 0, 4, 1, 5, 2, 6, 3, 7), e = |b|^2 - 2 a.b, the lexicographic (e, j) top-2
            and k_nn2_merge's max(|a|^2 + e, 0);
  matcher   sift3d_amd_matcher_match: Lowe's ratio test on squared f32 distances, forward-backward check;
  RANSAC    sift3d_amd_ransac_affine, literally, in Python floats (IEEE double, the C order of operations).
"""
import numpy as np

F = np.float32
KC = 32
# k order of one chunk of KC: four groups of eight, (8 g + 2 hf + j, 8 g + 4 + 2 hf + j) for hf, j in {0, 1}
CHUNK_ORDER = [8 * g + o for g in range(4) for o in (0, 4, 1, 5, 2, 6, 3, 7)]


def k_order(dim):
    assert dim % KC == 0 and dim >= KC
    return [c * KC + k for c in range(dim // KC) for k in CHUNK_ORDER]


def fma32(a, b, c):
    """Correctly rounded float32 fma(a, b, c), elementwise, emulated in float64: a * b is exact in float64,
    the sum is rounded to odd (53 >= 24 + 2 bits), so the final cast to float32 is the single correct
    rounding of a * b + c."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.asarray(c, np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                      # TwoSum: s + err == p + c exactly
    odd = (s.view(np.int64) & 1).astype(bool)
    fix = (err != 0) & ~odd & np.isfinite(s)
    if fix.any():
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def runs(nA, nB):
    """nn2_splits and the launcher's run length: (runs of B per row block of A, how many of them are empty)."""
    nblkA, nblkB = -(-nA // 128), -(-nB // 128)
    s = -(-2048 // nblkA) if nblkA > 0 else 1
    s = max(min(s, 16, nblkB), 1)
    per = max(-(-nblkB // s), 1)
    return s, sum(1 for r in range(s) if r * per * 128 >= nB)


def row_norms(a):
    """k_row_norms: lane L sums v * v (rounded product, then add) over k = L, L + 64, ...; then
    s += shfl_xor(s, o) for o = 32, 16, ..., 1; lane 0's value."""
    a = np.ascontiguousarray(a, F)
    n, dim = a.shape
    P = np.zeros((n, 64), F)
    for k in range(dim):
        v = a[:, k]
        P[:, k % 64] = P[:, k % 64] + v * v
    lanes = np.arange(64)
    o = 32
    while o:
        P = P + P[:, lanes ^ o]
        o >>= 1
    return P[:, 0].copy()


def dots(a, b):
    """a . b^T of k_nn2 (nA x nB float32): the fma chain from 0 in the kernel's k order."""
    a = np.ascontiguousarray(a, F)
    b = np.ascontiguousarray(b, F)
    acc = np.zeros((len(a), len(b)), F)
    for k in k_order(a.shape[1]):
        acc = fma32(a[:, k][:, None], b[:, k][None, :], acc)
    return acc


def top2(e):
    """Lexicographic (e, j) minimum of every row and the second-smallest e counting ties:
    (j, e1, e2), j = -1 and e1 = e2 = +inf without candidates."""
    n, m = e.shape
    if m == 0:
        return np.full(n, -1, np.int32), np.full(n, np.inf, F), np.full(n, np.inf, F)
    j = np.argmin(e, axis=1).astype(np.int32)         # (numpy: the first index of the minimum)
    rows = np.arange(n)
    e1 = e[rows, j]
    if m == 1:
        return j, e1, np.full(n, np.inf, F)
    rest = e.copy()
    rest[rows, j] = np.inf
    return j, e1, rest.min(axis=1).astype(F)


def nn2(a, b):
    """sift3d_hip_nn2 of float32 a (nA x dim) against b (nB x dim): (j int32, d1, d2 float32)."""
    a = np.ascontiguousarray(a, F)
    b = np.ascontiguousarray(b, F)
    na = row_norms(a)
    if len(b) == 0:
        return top2(np.zeros((len(a), 0), F))
    nb = row_norms(b)
    e = nb[None, :] - F(2.0) * dots(a, b)
    j, e1, e2 = top2(e)
    d1 = np.maximum(na + e1, F(0.0))
    with np.errstate(invalid="ignore"):
        d2 = np.maximum(na + e2, F(0.0))
    return j, d1.astype(F), d2.astype(F)


def match(fwd, bwd, nn_thresh):
    """sift3d_amd_matcher_match over the nn2 results of both directions (fwd: a -> b, bwd: b -> a, each
    (j, d1, d2)): match[i] = j or -1."""
    jf, f1, f2 = (np.asarray(x) for x in fwd)
    jb, b1, b2 = (np.asarray(x) for x in bwd)
    r2 = F(float(nn_thresh) * float(nn_thresh))      # (float)(nn_thresh * nn_thresh), the product in double
    with np.errstate(over="ignore", invalid="ignore"):
        okf = F(f1) < r2 * f2.astype(F)
        okb = F(b1) < r2 * b2.astype(F)
    out = np.full(len(jf), -1, np.int32)
    for i in range(len(jf)):
        j = int(jf[i])
        if j < 0 or not okf[i]:
            continue
        if int(jb[j]) != i or not okb[j]:
            continue
        out[i] = j
    return out


# ---- RANSAC ----------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1


def xorshift64(s):
    s ^= (s << 13) & M64
    s ^= s >> 7
    s ^= (s << 17) & M64
    return s


def solve4(M, R):
    """reg_solve4: Gauss-Jordan on [M | R^T] with partial pivoting; None below the 1e-12 pivot."""
    aug = [[M[i][j] for j in range(4)] + [R[j][i] for j in range(3)] for i in range(4)]
    for k in range(4):
        p = k
        for i in range(k + 1, 4):
            if abs(aug[i][k]) > abs(aug[p][k]):
                p = i
        if abs(aug[p][k]) < 1e-12:
            return None
        if p != k:
            aug[k], aug[p] = aug[p], aug[k]
        piv = aug[k][k]
        for j in range(k, 7):
            aug[k][j] /= piv
        for i in range(4):
            if i != k:
                f = aug[i][k]
                for j in range(k, 7):
                    aug[i][j] -= f * aug[k][j]
    return [[aug[j][4 + i] for j in range(4)] for i in range(3)]


def fit(src, dst, idx):
    """reg_fit: normal equations summed point by point, then solve4."""
    M = [[0.0] * 4 for _ in range(4)]
    R = [[0.0] * 4 for _ in range(3)]
    for q in idx:
        x, y = src[q], dst[q]
        h = (float(x[0]), float(x[1]), float(x[2]), 1.0)
        for i in range(4):
            for j in range(4):
                M[i][j] += h[i] * h[j]
        for i in range(3):
            for j in range(4):
                R[i][j] += float(y[i]) * h[j]
    return solve4(M, R)


def residual2(T, src, dst):
    """e2 of every point under T (3 x 4), in the C order: r = T0 x0 + T1 x1 + T2 x2 + T3 - y, e2 = 0 + r^2 ...
    (elementwise float64 numpy operations, each rounded once, as the C statements)."""
    x0, x1, x2 = src[:, 0], src[:, 1], src[:, 2]
    e2 = np.zeros(len(src))
    for k in range(3):
        r = T[k][0] * x0 + T[k][1] * x1 + T[k][2] * x2 + T[k][3] - dst[:, k]
        e2 = e2 + r * r
    return e2


def ransac_affine(src, dst, err_thresh, num_iter, seed):
    """sift3d_amd_ransac_affine: (tform 3 x 4, inlier mask uint8, num_inliers), or None on failure (the mask
    is then whatever the C code left in it, and is not compared)."""
    src = np.ascontiguousarray(src, np.float64).reshape(-1, 3)
    dst = np.ascontiguousarray(dst, np.float64).reshape(-1, 3)
    n = len(src)
    if n < 4 or num_iter < 1 or not err_thresh > 0:
        return None
    thr2 = err_thresh * err_thresh
    s = seed if seed else 88172645463325252
    picks = []
    for _ in range(num_iter):
        pick = []
        for _k in range(4):
            while True:
                s = xorshift64(s)
                q = s % n
                if q not in pick:
                    break
            pick.append(q)
        picks.append(pick)
    best_cnt, win = -1, -1
    for it, pick in enumerate(picks):
        T = fit(src, dst, pick)
        cnt = -1 if T is None else int((residual2(T, src, dst) <= thr2).sum())
        if cnt > best_cnt:
            best_cnt, win = cnt, it
    best = [[0.0] * 4 for _ in range(3)]
    if win >= 0:
        T = fit(src, dst, picks[win])
        if T is not None:
            best = T
    if best_cnt < 4:
        return None
    m, mask = 0, None
    for _pass in range(2):
        ok = residual2(best, src, dst) <= thr2
        mask = ok.astype(np.uint8)
        idx = np.nonzero(ok)[0].tolist()
        m = len(idx)
        if m < 4:
            break
        T = fit(src, dst, idx)
        if T is None:
            break
        best = T
    if m < 4:
        return None
    return np.array(best, np.float64), mask, m
