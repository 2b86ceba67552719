"""The slab driver's keypoint exchange (sift3d_amd/csrc/sift3d_slab.hip, sift3d_amd_slab_table), restated in numpy.

Not a mirror of the kernels: no prefix tables, no searches, no scans.

  rule      compaction(): the reference's rule on ONE global list.  Candidates stand in the reference's order --
            (octave, level) major, then (z, y, x) (sift.c:835-871) --; the in-place compaction copies a kept
            candidate's record to slot j but not its strength (copy_Keypoint, sift.c:372-384, 1148-1162: quirk Q2),
            so slot j keeps the strength of global CANDIDATE j.
  cutting   cut(): that list as W rank lists at per-octave z boundaries, each with its own level table (z_off, local
            nz, optionally halo planes in front of the first owned plane) and idx in the local buffer's coordinates.
  stages    counts(), packed(), table(), rebuild(), status(), scatter(): each stage's own contract, so that a failing
            test names the stage.
  cases     the count patterns, the hand-written tables and the lists the two test files share (data only).
"""
import numpy as np

CAND = np.dtype([("idx", "u4"), ("tag", "i4"), ("val", "f4")])
LEVEL = np.dtype([("data", "u8"), ("nx", "i4"), ("ny", "i4"), ("nz", "i4"), ("z_off", "i4"), ("nz_glob", "i4"),
                  ("ux", "f4"), ("uy", "f4"), ("uz", "f4"), ("octave", "i4"), ("sd", "f8")], align=True)
REC = np.dtype([("o", "i4"), ("s", "i4"), ("x", "i4"), ("y", "i4"), ("z", "i4"), ("R", "f4", (9,))])
OUT = np.dtype([("o", "i4"), ("s", "i4"), ("x", "i4"), ("y", "i4"), ("z", "i4"), ("R", "f4", (9,)),
                ("strength", "f4"), ("pad", "i4")])
GLOB = np.dtype([("o", "i4"), ("s", "i4"), ("x", "i4"), ("y", "i4"), ("z", "i4"), ("val", "f4")])
HEADER = 64
ROW = 768
assert (CAND.itemsize, LEVEL.itemsize, REC.itemsize, OUT.itemsize) == (12, 56, 56, 64)


# ---- the rule on one global list ------------------------------------------------------------------------------------

def compaction(glob, keep, R):
    """The keypoint list of the reference from its candidate list: every candidate is a keypoint with its strength;
    the kept ones are then moved forward in place, everything but the strength."""
    kp = np.zeros(len(glob), OUT)
    for f in ("o", "s", "x", "y", "z"):
        kp[f] = glob[f]
    kp["strength"] = glob["val"]
    j = 0
    for i in range(len(kp)):
        if keep[i]:
            for f in ("o", "s", "x", "y", "z"):
                kp[f][j] = kp[f][i]
            kp["R"][j] = R[i]
            j += 1
    return kp[:j].copy()


def in_reference_order(glob):
    order = np.lexsort((glob["x"], glob["y"], glob["z"], glob["s"], glob["o"]))
    return bool((order == np.arange(len(glob))).all())


# ---- cutting --------------------------------------------------------------------------------------------------------

def cut(glob, keep, R, dims, bounds, ngl, halo=0):
    """dims[o] = (nx, ny); bounds[o] = the W + 1 ascending z boundaries of octave o; halo: planes a rank's buffer holds
    in front of (and behind) its owned planes.  -> per rank dict(levels, cand, keep, R)."""
    W = len(bounds[0]) - 1
    ranks = []
    for r in range(W):
        levels = np.zeros(len(dims) * ngl, LEVEL)
        for o, (nx, ny) in enumerate(dims):
            lv = levels[o * ngl:(o + 1) * ngl]
            lv["nx"], lv["ny"], lv["octave"] = nx, ny, o
            lv["z_off"] = bounds[o][r] - halo
            lv["nz"] = bounds[o][r + 1] - bounds[o][r] + 2 * halo
            lv["nz_glob"] = bounds[o][-1]
        lo = np.array([bounds[o][r] for o in glob["o"]], np.int64).reshape(-1)
        hi = np.array([bounds[o][r + 1] for o in glob["o"]], np.int64).reshape(-1)
        mine = (glob["z"] >= lo) & (glob["z"] < hi)
        g = glob[mine]
        c = np.zeros(len(g), CAND)
        c["tag"] = g["o"] * ngl + g["s"] + 1
        L = levels[c["tag"]]
        c["idx"] = g["x"].astype(np.int64) + L["nx"].astype(np.int64) * (
            g["y"] + L["ny"].astype(np.int64) * (g["z"].astype(np.int64) - L["z_off"]))
        c["val"] = g["val"]
        ranks.append(dict(levels=levels, cand=c, keep=np.ascontiguousarray(keep[mine], np.int32),
                          R=np.ascontiguousarray(R[mine], np.float32)))
    return ranks


# ---- the stages' contracts ------------------------------------------------------------------------------------------

def keys_of(cand, ngl, K):
    return (cand["tag"] // ngl) * K + cand["tag"] % ngl - 1


def counts(cand, keep, ngl, K, nkey):
    """[2 key] candidates, [2 key + 1] kept ones (keep != 0)."""
    key = keys_of(cand, ngl, K)
    c = np.zeros((nkey, 2), np.int32)
    c[:, 0] = np.bincount(key, minlength=nkey)
    c[:, 1] = np.bincount(key[np.asarray(keep) != 0], minlength=nkey)
    return c.reshape(-1)


def packed(levels, cand, keep, R, ngl):
    """A rank's block: the values of all its candidates; its kept candidates, in order, in global coordinates."""
    k = np.asarray(keep) != 0
    c, L = cand[k], levels[cand["tag"][k]]
    idx, nx, ny = c["idx"].astype(np.int64), L["nx"].astype(np.int64), L["ny"].astype(np.int64)
    rec = np.zeros(len(c), REC)
    rec["o"], rec["s"] = c["tag"] // ngl, c["tag"] % ngl - 1
    rec["x"], rec["y"], rec["z"] = idx % nx, (idx // nx) % ny, idx // (nx * ny) + L["z_off"]
    rec["R"] = np.asarray(R, np.float32).reshape(-1, 9)[k]
    return cand["val"].copy(), rec


def round16(v):
    return (int(v) + 15) // 16 * 16


def table(cnt, nkey):
    """cnt [W, >= 2 nkey] -> (the words k_slab_build documents, the layout): where each (key, rank) segment starts in
    the two global orders (keys major), where each key starts in a rank's own lists."""
    cnt = np.asarray(cnt, np.int64)[:, :2 * nkey]
    W = cnt.shape[0]
    c, k = cnt[:, 0::2], cnt[:, 1::2]                                 # [rank, key]
    start = lambda a: np.concatenate(([0], np.cumsum(a)))
    own = lambda a: np.concatenate([start(a[r]) for r in range(W)])
    tot_c, tot_k = int(c.sum()), int(k.sum())
    if max(tot_c, tot_k) >= 2 ** 32 or (cnt < 0).any():
        return None, None
    tab = np.concatenate((start(k.T.reshape(-1)), start(c.T.reshape(-1)), own(k), own(c))).astype(np.uint32)
    maxc, maxk = int(c.sum(axis=1).max()), int(k.sum(axis=1).max())
    roff = round16(4 * max(maxc, 1))
    toff = roff + round16(56 * max(maxk, 1))
    return tab, dict(tot_c=tot_c, tot_k=tot_k, maxc=maxc, maxk=maxk, roff=roff, toff=toff, blk=toff + 16)


def rebuild(cnt, vals, recs, nkey):
    """The global list from the ranks' blocks: inside a key the ranks follow each other in slab order; position j of
    the kept records carries the value at position j of the candidates' values."""
    cnt = np.asarray(cnt, np.int64)[:, :2 * nkey]
    W = cnt.shape[0]
    pieces = lambda lists, n: [np.split(lists[r], np.cumsum(n[r])[:-1]) for r in range(W)]
    v, q = pieces(vals, cnt[:, 0::2]), pieces(recs, cnt[:, 1::2])
    gv = np.concatenate([v[r][k] for k in range(nkey) for r in range(W)])
    gq = np.concatenate([q[r][k] for k in range(nkey) for r in range(W)])
    out = np.zeros(len(gq), OUT)
    for f in REC.names:
        out[f] = gq[f]
    out["strength"] = gv[:len(gq)]
    return out


def status(words):
    """The header's word: the last rank's non-zero status, 0 when every rank succeeded."""
    bad = [int(w) for w in words if int(w) != 0]
    return bad[-1] if bad else 0


def scatter(blocks, rows_map):
    """blocks [nblocks, rows, 768]; row g of the result is row (map & 0xffffff) of block map >> 24."""
    m = np.asarray(rows_map, np.int64)
    return blocks[m >> 24, m & 0xffffff].reshape(len(m), ROW)


# ---- cases: the whole chain -----------------------------------------------------------------------------------------
K, NGL, NKEY = 3, 6, 6                                                # two octaves, three keypoint levels each
DIMS = [(37, 11), (18, 5)]
WORLDS = (1, 2, 3, 8)
PATTERNS = ("dense", "no_keep", "alternating", "rank_empty_first", "rank_empty_middle", "rank_empty_last",
            "key_empty_first", "key_empty_middle", "key_empty_last", "none_kept_next_to_all_kept",
            "one_kept_in_last_segment", "tot_k_equals_tot_c")
KEEP_VALUES = np.array([1, -1, 2, 0x100], np.int32)


def chain_bounds(W):
    """Octave 0: three planes a rank and two more on the last; octave 1: two and one more."""
    return [[3 * r for r in range(W)] + [3 * W + 2], [2 * r for r in range(W)] + [2 * W + 1]]


def special_floats(rng, shape):
    """Random bit patterns (NaNs with payloads, infinities, subnormals among them), -0.0 and subnormals planted."""
    a = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)
    flat = a.reshape(-1)
    plant = np.array([0x80000000, 0x00000001, 0x807fffff, 0x7fc00123, 0xffc0beef, 0x7f800001, 0x7f800000, 0],
                     np.uint32)
    flat[:min(len(plant), len(flat))] = plant[:len(flat)]
    rng.shuffle(flat)
    return a.view(np.float32)


def chain_case(W, pattern, seed=0):
    """-> dict(glob, keep, R, bounds, halo, seg): a global list whose (key, rank) segments hold seg[key, rank]
    candidates, and the keep flags of the pattern."""
    assert pattern in PATTERNS
    rng = np.random.Generator(np.random.PCG64([seed, W, PATTERNS.index(pattern)]))
    bounds = chain_bounds(W)
    seg = rng.integers(20, 120, size=(NKEY, W))
    mid_r, mid_k = W // 2, NKEY // 2
    if pattern.startswith("rank_empty"):
        seg[:, {"first": 0, "middle": mid_r, "last": W - 1}[pattern.split("_")[-1]]] = 0
    if pattern.startswith("key_empty"):
        seg[{"first": 0, "middle": mid_k, "last": NKEY - 1}[pattern.split("_")[-1]], :] = 0
    parts, owner = [], []
    for key in range(NKEY):
        o, s = divmod(key, K)
        nx, ny = DIMS[o]
        for r in range(W):
            lo, hi = bounds[o][r] * nx * ny, bounds[o][r + 1] * nx * ny
            v = np.sort(rng.choice(np.arange(lo, hi), size=int(seg[key, r]), replace=False))
            g = np.zeros(len(v), GLOB)
            g["o"], g["s"], g["x"], g["y"], g["z"] = o, s, v % nx, (v // nx) % ny, v // (nx * ny)
            parts.append(g)
            owner.append(np.full(len(v), key * W + r))
    glob, owner = np.concatenate(parts), np.concatenate(owner)
    n = len(glob)
    glob["val"] = special_floats(rng, n)
    R = special_floats(rng, (n, 9))
    keep = np.where(rng.random(n) < 0.5, rng.choice(KEEP_VALUES, n), 0).astype(np.int32)
    if pattern in ("dense", "tot_k_equals_tot_c"):
        keep = np.ones(n, np.int32) if pattern == "dense" else rng.choice(KEEP_VALUES, n).astype(np.int32)
    elif pattern == "no_keep":
        keep[:] = 0
    elif pattern == "alternating":
        keep = (np.arange(n) % 2).astype(np.int32)
    elif pattern == "none_kept_next_to_all_kept":
        a = (NKEY // 2) * W + W - 1                                   # last rank of a key, first rank of the next
        keep[owner == a] = 0
        keep[owner == a + 1] = -1
    elif pattern == "one_kept_in_last_segment":
        last = np.nonzero(owner == NKEY * W - 1)[0]
        keep[last] = 0
        keep[last[len(last) // 2]] = 2
    return dict(glob=glob, keep=keep, R=R, bounds=bounds, halo=2 * (PATTERNS.index(pattern) % 2), seg=seg)


def count_patterns():
    """(id, cnt [W, 2 NKEY]) of every chain case: what the table function sees."""
    for W in WORLDS:
        for p in PATTERNS:
            c = chain_case(W, p)
            ranks = cut(c["glob"], c["keep"], c["R"], DIMS, c["bounds"], NGL, c["halo"])
            yield "w%d-%s" % (W, p), np.stack([counts(x["cand"], x["keep"], NGL, K, NKEY) for x in ranks])


# ---- cases: slab_build on tables written by hand ----------------------------------------------------------------------
# 2 ranks x 3 keys.  cnt[rank] = (candidates, kept) of key 0, 1, 2.  Segments in global order: (k0, r0) (k0, r1) (k1, r0)
# (k1, r1) (k2, r0) (k2, r1).  tab = segk (7) | segc (7) | ck r0, r1 (4 each) | cc r0, r1 (4 each).
HAND = {
    # every segment filled
    "all_filled": dict(cnt=[[3, 2, 2, 1, 4, 2], [1, 1, 3, 3, 2, 0]],
                       tab=[0, 2, 3, 4, 7, 9, 9,  0, 3, 4, 6, 9, 13, 15,  0, 2, 3, 5,  0, 1, 4, 4,
                            0, 3, 5, 9,  0, 1, 4, 6]),
    # key 0 empty on both ranks, and rank 0 empty in key 1: a leading run of three empty segments
    "leading_run": dict(cnt=[[0, 0, 0, 0, 3, 2], [0, 0, 2, 2, 1, 1]],
                        tab=[0, 0, 0, 0, 2, 4, 5,  0, 0, 0, 0, 2, 5, 6,  0, 0, 0, 2,  0, 0, 2, 3,
                             0, 0, 0, 3,  0, 0, 2, 3]),
    # key 2 empty on both ranks and rank 1 empty in key 1: a trailing run
    "trailing_run": dict(cnt=[[2, 1, 3, 3, 0, 0], [2, 2, 0, 0, 0, 0]],
                         tab=[0, 1, 3, 6, 6, 6, 6,  0, 2, 4, 7, 7, 7, 7,  0, 1, 4, 4,  0, 2, 2, 2,
                              0, 2, 5, 5,  0, 2, 2, 2]),
    # rank 0 has no candidates at all
    "rank0_empty": dict(cnt=[[0, 0, 0, 0, 0, 0], [2, 1, 1, 1, 3, 2]],
                        tab=[0, 0, 1, 1, 2, 2, 4,  0, 0, 2, 2, 3, 3, 6,  0, 0, 0, 0,  0, 1, 2, 4,
                             0, 0, 0, 0,  0, 2, 3, 6]),
    # rank 1 has none
    "rank1_empty": dict(cnt=[[2, 1, 1, 1, 3, 2], [0, 0, 0, 0, 0, 0]],
                        tab=[0, 1, 1, 2, 2, 4, 4,  0, 2, 2, 3, 3, 6, 6,  0, 1, 2, 4,  0, 0, 0, 0,
                             0, 2, 3, 6,  0, 0, 0, 0]),
    # the middle key empty on both ranks
    "middle_key_empty": dict(cnt=[[2, 2, 0, 0, 1, 1], [1, 0, 0, 0, 2, 1]],
                             tab=[0, 2, 2, 2, 2, 3, 4,  0, 2, 3, 3, 3, 4, 6,  0, 2, 2, 3,  0, 0, 0, 1,
                                  0, 2, 2, 3,  0, 1, 1, 3]),
    # segments that hold candidates and no kept keypoint next to ones that are all kept
    "candidates_none_kept": dict(cnt=[[3, 0, 2, 2, 4, 0], [2, 2, 3, 0, 1, 1]],
                                 tab=[0, 0, 2, 4, 4, 4, 5,  0, 3, 5, 7, 10, 14, 15,  0, 0, 2, 2,  0, 2, 2, 3,
                                      0, 3, 5, 9,  0, 2, 5, 6]),
    # nothing kept anywhere: the launch writes the header alone
    "nothing_kept": dict(cnt=[[2, 0, 1, 0, 0, 0], [0, 0, 3, 0, 1, 0]],
                         tab=[0, 0, 0, 0, 0, 0, 0,  0, 2, 2, 3, 6, 6, 7,  0, 0, 0, 0,  0, 0, 0, 0,
                              0, 2, 3, 3,  0, 0, 3, 4]),
}


def hand_totk(t):
    """tot_k = 255, 256, 257 around the 256 keypoints of a workgroup: kept 100 + 27 on rank 0, 128 + (t - 255) on rank
    1; every candidate kept but 5 of rank 1's key 2."""
    e = t - 255
    return dict(cnt=[[100, 100, 0, 0, 27, 27], [0, 0, 128, 128, e + 5, e]],
                tab=[0, 100, 100, 100, 228, 255, 255 + e,  0, 100, 100, 100, 228, 255, 260 + e,
                     0, 100, 100, 127,  0, 0, 128, 128 + e,  0, 100, 100, 127,  0, 0, 128, 133 + e])


for _t in (255, 256, 257):
    HAND["tot_k_%d" % _t] = hand_totk(_t)

STATUSES = {"all_zero": [0, 0], "rank0_only": [-7, 0], "last_rank_only": [0, 5], "two_different": [-3, 9]}


def hand_blocks(name, seed=1):
    """Random values and records for a hand-written table: per rank vals [candidates], recs [kept]."""
    cnt = np.array(HAND[name]["cnt"], np.int64)
    rng = np.random.Generator(np.random.PCG64([seed, sorted(HAND).index(name)]))
    vals = [special_floats(rng, int(c[0::2].sum())) for c in cnt]
    recs = []
    for c in cnt:
        q = np.zeros(int(c[1::2].sum()), REC)
        q.view(np.uint32)[:] = special_floats(rng, 14 * len(q)).view(np.uint32)
        recs.append(q)
    return cnt.astype(np.int32), vals, recs
