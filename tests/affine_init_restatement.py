"""numpy restatement of the initial-transform contract (include/sift3d_amd.h, "Initial transforms: moments and
candidate search"), float64.

moments: the ten sums correctly rounded (math.fsum) with the sum of |term| beside each, so that a bound on the device's
sum need not allow for the reference's own error.  frame, candidates and rank follow the header's order of operations
(the Jacobi rotations, the matrix products, the candidate's translation column), so they agree with the library to the
last bit where libm and numpy agree on sqrt, cos and sin.  score strings tests/similarity_restatement.py's joint and
measures together per candidate; init is the driver: restrict, moments, frames, candidates, scores, rank, carry up."""
import collections
import math

import numpy as np

from tests import multires_restatement as mr
from tests import similarity_restatement as sr

Moments = collections.namedtuple("Moments", "n sums terms")      # sums: S0, S1[3], S2[6]; terms: sum |term| per sum
Frame = collections.namedtuple("Frame", "centroid axes lam")
Init = collections.namedtuple("Init", "A index cost count K levels candidates costs counts order frame_f frame_m")
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
SIGNS = ((1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1))
DEFAULTS = dict(range_deg=(90.0, 90.0, 90.0), step_deg=30.0, range_vox=(0.0, 0.0, 0.0), step_vox=1.0)
MAX_CANDIDATES = 16384


def centre(shape):
    nz, ny, nx = shape
    return np.array([(nx - 1) / 2.0, (ny - 1) / 2.0, (nz - 1) / 2.0])


def moments(V, floor=0.0, weight="binary", mask=None):
    """the record of sift3d_hip_moments for V [nz, ny, nx]"""
    V = np.ascontiguousarray(V, np.float32)
    w = V - np.float32(floor)                                # float32
    with np.errstate(invalid="ignore"):
        counted = w > 0                                      # a NaN is not
    if mask is not None:
        with np.errstate(invalid="ignore"):
            counted &= np.asarray(mask, np.float32) >= np.float32(0.5)
    z, y, x = np.nonzero(counted)
    c = centre(V.shape)
    P = [x.astype(np.float64) - c[0], y.astype(np.float64) - c[1], z.astype(np.float64) - c[2]]
    W = np.ones(len(x)) if weight == "binary" else w[counted].astype(np.float64)
    terms = [W] + [W * P[d] for d in range(3)] + [(W * P[d]) * P[e] for d, e in PAIRS]
    return Moments(len(x), np.array([math.fsum(t.tolist()) for t in terms]),
                   np.array([float(np.abs(t).sum()) for t in terms]))


def jacobi3(a):
    """(diagonal, V with the eigenvectors as columns) of the symmetric 3 x 3 a by the header's cyclic Jacobi"""
    a = [[float(a[i][j]) for j in range(3)] for i in range(3)]
    v = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    scale = (abs(a[0][0]) + abs(a[1][1])) + abs(a[2][2])
    for i in range(3):
        for j in range(i):
            a[i][j] = a[j][i]
    for _ in range(64):
        off = (a[0][1] * a[0][1] + a[0][2] * a[0][2]) + a[1][2] * a[1][2]
        if off <= (1e-60 * scale) * scale:
            break
        for p in range(2):
            for q in range(p + 1, 3):
                if a[p][q] == 0.0:
                    continue
                theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q])
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for i in range(3):
                    aip, aiq = a[i][p], a[i][q]
                    a[i][p] = c * aip - s * aiq
                    a[i][q] = s * aip + c * aiq
                for i in range(3):
                    api, aqi = a[p][i], a[q][i]
                    a[p][i] = c * api - s * aqi
                    a[q][i] = s * api + c * aqi
                a[p][q] = a[q][p] = 0.0
                for i in range(3):
                    vip, viq = v[i][p], v[i][q]
                    v[i][p] = c * vip - s * viq
                    v[i][q] = s * vip + c * viq
    return [a[i][i] for i in range(3)], v


def frame(n, sums, shape):
    """sift3d_amd_moments_frame: the Frame, or None where the entry refuses"""
    s = [float(v) for v in sums]
    if n == 0 or not all(math.isfinite(v) for v in s) or not s[0] > 0:
        return None
    mu = [s[1 + d] / s[0] for d in range(3)]
    C = [[0.0] * 3 for _ in range(3)]
    for k, (d, e) in enumerate(PAIRS):
        C[d][e] = s[4 + k] / s[0] - mu[d] * mu[e]
    if not all(math.isfinite(C[d][e]) for d, e in PAIRS):
        return None
    ev, v = jacobi3(C)
    order = [0, 1, 2]
    for i in range(1, 3):                                    # descending, stable
        j = i
        while j > 0 and ev[order[j]] > ev[order[j - 1]]:
            order[j], order[j - 1] = order[j - 1], order[j]
            j -= 1
    R = np.zeros((3, 3))
    for r in range(2):
        row = [v[i][order[r]] for i in range(3)]
        big = 0
        for i in range(1, 3):
            if abs(row[i]) > abs(row[big]):
                big = i
        if row[big] < 0:
            row = [-e for e in row]
        R[r] = row
    R[2] = [R[0][1] * R[1][2] - R[0][2] * R[1][1], R[0][2] * R[1][0] - R[0][0] * R[1][2],
            R[0][0] * R[1][1] - R[0][1] * R[1][0]]
    if not (np.all(np.isfinite(R)) and all(math.isfinite(e) for e in ev)):
        return None
    return Frame(centre(shape) + np.array(mu), R, np.array([ev[k] for k in order]))


def mat3(A, B):
    """A B, each entry (a0 b0 + a1 b1) + a2 b2"""
    return np.array([[(A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j] for j in range(3)] for i in range(3)])


def candidate(R, cF, cM, t):
    A = np.zeros((3, 4))
    A[:, :3] = R
    for d in range(3):
        A[d, 3] = (cM[d] + t[d]) - ((R[d][0] * cF[0] + R[d][1] * cF[1]) + R[d][2] * cF[2])
    return A


def axis_values(rng, step):
    h = math.floor(rng / step)
    return [float(i - h) * step for i in range(2 * h + 1)]


def search_count(**search):
    s = dict(DEFAULTS, **search)
    K = 1
    for d in range(3):
        K *= len(axis_values(s["range_deg"][d], s["step_deg"])) * len(axis_values(s["range_vox"][d], s["step_vox"]))
    return K


def candidates(mode, fF, fM, **search):
    """sift3d_amd_affine_init_candidates: A [K, 3, 4]; None where SEARCH has too many"""
    cF, cM = fF.centroid, fM.centroid
    zero = (0.0, 0.0, 0.0)
    if mode == "centroid":
        return np.array([candidate(np.eye(3), cF, cM, zero)])
    if mode == "axes":
        out = [candidate(np.eye(3), cF, cM, zero)]
        for sg in SIGNS:
            DV = np.array([[sg[i] * fF.axes[i][j] for j in range(3)] for i in range(3)])
            out.append(candidate(mat3(np.asarray(fM.axes).T, DV), cF, cM, zero))
        return np.array(out)
    s = dict(DEFAULTS, **search)
    if search_count(**search) > MAX_CANDIDATES:
        return None
    ang = [axis_values(s["range_deg"][d], s["step_deg"]) for d in range(3)]
    off = [axis_values(s["range_vox"][d], s["step_vox"]) for d in range(3)]
    rad = math.pi / 180.0
    out = []
    for tz in off[2]:
        for ty in off[1]:
            for tx in off[0]:
                for ga in ang[2]:
                    for be in ang[1]:
                        for al in ang[0]:
                            ca, sa = math.cos(al * rad), math.sin(al * rad)
                            cb, sb = math.cos(be * rad), math.sin(be * rad)
                            cg, sg = math.cos(ga * rad), math.sin(ga * rad)
                            Rx = [[1, 0, 0], [0, ca, -sa], [0, sa, ca]]
                            Ry = [[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]]
                            Rz = [[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]]
                            out.append(candidate(mat3(Rz, mat3(Ry, Rx)), cF, cM, (tx, ty, tz)))
    return np.array(out)


def cost_of(metric, n, sums, hist=None):
    """one candidate's cost from its count, six sums and (mi) histogram"""
    if n == 0:
        return float("nan")
    s = [float(v) for v in sums]
    nd = float(n)
    if metric == "msd":
        return s[5] / nd
    if metric == "ncc":
        vf = s[2] - s[0] * s[0] / nd
        vm = s[3] - s[1] * s[1] / nd
        ncc = 0.0 if vf <= 0 or vm <= 0 else (s[4] - s[0] * s[1] / nd) / math.sqrt(vf * vm)
        return 1.0 - ncc * ncc
    return -sr.measures(hist, n, s).mi


def order_of(costs, counts, min_overlap=0.5):
    """the eligible candidates by ascending cost, ties to the lower index"""
    n_max = max(int(n) for n in counts)
    ok = [k for k in range(len(costs))
          if math.isfinite(costs[k]) and int(counts[k]) > 0 and float(counts[k]) >= min_overlap * float(n_max)]
    return sorted(ok, key=lambda k: (costs[k], k))


def score(F, M, A, metric="mi", bins=32, range_f=(0.0, 1.0), range_m=(0.0, 1.0)):
    """(costs, counts) of the candidates A [K, 3, 4] on one level, LINEAR"""
    costs, counts = [], []
    for a in A:
        hist, st = sr.joint(F, M, a, bins if metric == "mi" else 2, range_f, range_m, "linear")
        costs.append(cost_of(metric, st.count, st.sums, hist))
        counts.append(st.count)
    return np.array(costs), np.array(counts, np.uint64)


def init_levels(fshape, mshape, levels):
    dims = list(fshape) + list(mshape)
    for l in range(1, levels):
        if any((d + 1) // 2 < 8 for d in dims):
            return l
        dims = [(d + 1) // 2 for d in dims]
    return levels


def init(F, M, mode="search", metric="mi", levels=3, weight="binary", floor_f=0.0, floor_m=0.0, bins=32,
         range_f=(0.0, 1.0), range_m=(0.0, 1.0), min_overlap=0.5, **search):
    """the driver; None where a volume has nothing above its floor or no candidate is eligible"""
    F, M = np.ascontiguousarray(F, np.float32), np.ascontiguousarray(M, np.float32)
    levels = init_levels(F.shape, M.shape, levels)
    cF, cM = F, M
    for _ in range(levels - 1):
        cF, cM = mr.ref_restrict(cF), mr.ref_restrict(cM)
    scale = 2.0 ** (levels - 1)
    mf, mm = moments(cF, floor_f, weight), moments(cM, floor_m, weight)
    fF, fM = frame(mf.n, mf.sums, cF.shape), frame(mm.n, mm.sums, cM.shape)
    if fF is None or fM is None:
        return None
    s = dict(DEFAULTS, **search)
    s["range_vox"] = tuple(v / scale for v in s["range_vox"])
    s["step_vox"] = s["step_vox"] / scale
    A = candidates(mode, fF, fM, **s)
    costs, counts = score(cF, cM, A, metric, bins, range_f, range_m)
    order = order_of(costs, counts, min_overlap)
    if not order:
        return None
    best = A[order[0]].copy()
    best[:, 3] *= scale
    up = [Frame(f.centroid * scale, f.axes, f.lam * scale * scale) for f in (fF, fM)]
    return Init(best, order[0], costs[order[0]], int(counts[order[0]]), len(A), levels, A, costs, counts, order, *up)
