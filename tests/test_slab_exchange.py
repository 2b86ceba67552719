"""GPU (-m gpu): the device stages of the slab driver's keypoint exchange (sift3d_amd/csrc/sift3d_slab.hip) on
CALLER-MADE candidate lists, bit for bit against tests/slab_restatement.py.

  a  the whole chain -- slab_count, sift3d_amd_slab_table, slab_pack, the all-gather as a copy of the ranks' blocks side
     by side, slab_build -- against the reference's compaction of the one global list, for 1, 2, 3 and 8 ranks;
  b  slab_count alone: the grid-stride loop (more than 262 144 candidates), the two-round LDS initialisation (more
     than 128 keys), any non-zero keep value, a count buffer that is not zero on entry;
  c  slab_pack alone: one and two rounds of the scan of the block sums, keep runs on and across the 4-, 64-, 256- and
     1024-candidate boundaries, indices up to the end of a level of 2^32 - 2^22 voxels, NaN payloads;
  d  slab_build alone on tables written by hand (tests/slab_restatement.py: HAND), statuses, the header, pad;
  e  rows_scatter, f  max_rows.

Floats are compared as bits.  Every buffer a kernel writes (cnt, vals, recs, the scan scratch, out, the scatter's and
the reduction's destination) is exactly as long as the entry promises and lies between two guard bands of 256 bytes
that must survive; every input must come back unchanged.  The level tables carry no voxel data: these kernels read nx,
ny and z_off only.

(c) takes the index 2^32 - 2049 as one of its cases: it lies behind the last plane of the 2048 x 2048 x 1023 level (whose
last row starts at 2^32 - 2^22 - 2048, also a case); the split is arithmetic on the index alone and nothing is read
there.
"""
import numpy as np
import pytest

from tests import slab_restatement as rs

G, SENTINEL, FILL = 256, 0xA5, 0x5A
U32 = np.uint32


@pytest.fixture(scope="module")
def gpu():
    import torch
    from sift3d_amd import api, hip
    if not torch.cuda.is_available() or not api.device_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    return hip, torch


class Guarded:
    """`nbytes` bytes on the device between two guard bands; the payload starts as `fill` (an array of that many bytes)
    or as FILL bytes."""

    def __init__(self, torch, nbytes, fill=None):
        self.n = int(nbytes)
        host = np.full(2 * G + self.n, SENTINEL, np.uint8)
        host[G:G + self.n] = FILL if fill is None else np.frombuffer(np.ascontiguousarray(fill).tobytes(), np.uint8)
        self.buf = torch.from_numpy(host).cuda()

    def view(self, dtype):
        return self.buf[G:G + self.n].view(dtype)

    def read(self, dtype=np.uint8):
        host = self.buf.cpu().numpy()
        assert (host[:G] == SENTINEL).all(), "the guard band in front was written"
        assert (host[G + self.n:] == SENTINEL).all(), "the guard band behind was written"
        return host[G:G + self.n].copy().view(dtype)


def up(torch, a, dtype=None):
    """A host array on the device: its bytes, seen as `dtype` (None: uint8)."""
    b = np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy()
    if not len(b):
        return torch.empty(0, dtype=dtype or torch.uint8, device="cuda")
    t = torch.from_numpy(b).cuda()
    return t if dtype is None else t.view(dtype)


def unchanged(t, a):
    return t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()


def bits(a):
    return np.ascontiguousarray(a).view(U32)


# ---- the stages on the device ---------------------------------------------------------------------------------------

def run_count(gpu, cand, keep, ngl, K, nkey, prefill=None):
    hip, torch = gpu
    d_c, d_k = up(torch, cand), up(torch, keep, torch.int32)
    g = Guarded(torch, 8 * nkey, prefill)
    hip.slab_count(d_c, d_k, len(cand), ngl, K, nkey, g.view(torch.int32))
    torch.cuda.synchronize()
    cnt = g.read(np.int32)
    assert unchanged(d_c, cand) and unchanged(d_k, keep)
    return cnt


def run_pack(gpu, levels, cand, keep, R, ngl):
    """-> vals, recs, the scan scratch as it is left, and the two guarded device buffers."""
    hip, torch = gpu
    n, kept = len(cand), int((np.asarray(keep) != 0).sum())
    d_l, d_c = up(torch, levels), up(torch, cand)
    d_k, d_R = up(torch, keep, torch.int32), up(torch, R, torch.float32)
    nscratch = hip.slab_pack_scratch_bytes(n)
    gv, gr = Guarded(torch, 4 * n), Guarded(torch, rs.REC.itemsize * kept)
    gs = Guarded(torch, nscratch, np.ones(nscratch // 4, U32))
    hip.slab_pack(d_l, d_c, d_k, d_R, n, ngl, gv.view(torch.float32), gr.view(torch.uint8), gs.view(torch.uint8))
    torch.cuda.synchronize()
    assert unchanged(d_l, levels) and unchanged(d_c, cand) and unchanged(d_k, keep) and unchanged(d_R, R)
    return gv.read(np.float32), gr.read(rs.REC), gs.read(U32), gv, gr


def check_pack(gpu, levels, cand, keep, R, ngl):
    vals, recs, scan, gv, gr = run_pack(gpu, levels, cand, keep, R, ngl)
    want_vals, want_recs = rs.packed(levels, cand, keep, R, ngl)
    np.testing.assert_array_equal(bits(vals), bits(want_vals))
    if len(recs) != len(want_recs) or recs.tobytes() != want_recs.tobytes():
        bad = np.nonzero((recs.view(U32).reshape(-1, 14) != want_recs.view(U32).reshape(-1, 14)).any(axis=1))[0]
        pytest.fail("%d of %d records differ, first at %d: %r, want %r"
                    % (len(bad), len(recs), bad[0], recs[bad[0]], want_recs[bad[0]]))
    # the scratch: the exclusive scan of the blocks' kept counts, and the entry's spare word untouched
    n = len(cand)
    nb = (n + 1023) // 1024
    per_block = np.bincount(np.nonzero(np.asarray(keep))[0] // 1024, minlength=nb)
    want_scan = np.concatenate((np.cumsum(per_block) - per_block, [1])) if n else np.ones(1)
    np.testing.assert_array_equal(scan, want_scan.astype(U32))
    return vals, recs, gv, gr


def run_build(gpu, d_all, host_all, lay, W, nkey, tab, want_status):
    """slab_build on the gathered blocks -> the records; checks the header, the guards and the inputs."""
    hip, torch = gpu
    tot_k, tot_c = lay["tot_k"], lay["tot_c"]
    d_tab = up(torch, tab)
    out = Guarded(torch, rs.HEADER + rs.OUT.itemsize * tot_k)
    hip.slab_build(d_all, lay["blk"], lay["roff"], lay["toff"], W, nkey, d_tab, tot_k, tot_c, out.view(torch.uint8))
    torch.cuda.synchronize()
    got = out.read()
    assert unchanged(d_all, host_all) and unchanged(d_tab, tab)
    assert int(got[:4].view(np.int32)[0]) == want_status
    assert (got[4:rs.HEADER] == FILL).all(), "bytes 4 ... 63 of the header were written"
    recs = got[rs.HEADER:].view(rs.OUT)
    assert len(recs) == tot_k and (recs["pad"] == 0).all()
    return recs


def gathered(lay, vals, recs, stats):
    """The all-gather's result on the host: the ranks' blocks side by side at stride blk."""
    blk = lay["blk"]
    a = np.full(len(vals) * blk, 0xC3, np.uint8)
    for r, (v, q, st) in enumerate(zip(vals, recs, stats)):
        a[r * blk:r * blk + 4 * len(v)] = np.frombuffer(v.tobytes(), np.uint8)
        a[r * blk + lay["roff"]:r * blk + lay["roff"] + 56 * len(q)] = np.frombuffer(q.tobytes(), np.uint8)
        a[r * blk + lay["toff"]:r * blk + lay["toff"] + 4] = np.frombuffer(np.int32(st).tobytes(), np.uint8)
    return a


def same_records(got, want):
    if len(got) != len(want) or got.tobytes() != want.tobytes():
        g, w = got.view(U32).reshape(-1, 16), want.view(U32).reshape(-1, 16)
        if len(g) != len(w):
            pytest.fail("%d records, want %d" % (len(g), len(w)))
        bad = np.nonzero((g != w).any(axis=1))[0]
        cols = np.nonzero((g != w).any(axis=0))[0]
        pytest.fail("%d of %d records differ (words %s), first at %d: %r, want %r"
                    % (len(bad), len(g), cols.tolist(), bad[0], got[bad[0]], want[bad[0]]))


# ---- a. the whole chain against the global compaction -----------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("pattern", rs.PATTERNS)
@pytest.mark.parametrize("W", rs.WORLDS)
def test_chain(gpu, W, pattern):
    hip, torch = gpu
    c = rs.chain_case(W, pattern)
    ranks = rs.cut(c["glob"], c["keep"], c["R"], rs.DIMS, c["bounds"], rs.NGL, c["halo"])
    want = rs.compaction(c["glob"], c["keep"], c["R"])
    # counts
    cnt = np.stack([run_count(gpu, x["cand"], x["keep"], rs.NGL, rs.K, rs.NKEY) for x in ranks])
    for r, x in enumerate(ranks):
        np.testing.assert_array_equal(cnt[r], rs.counts(x["cand"], x["keep"], rs.NGL, rs.K, rs.NKEY), "rank %d" % r)
    # the product's table
    tab, lay = hip.slab_table(cnt, rs.NKEY)
    want_tab, want_lay = rs.table(cnt, rs.NKEY)
    np.testing.assert_array_equal(tab, want_tab)
    assert lay == want_lay and lay["tot_c"] == len(c["glob"]) and lay["tot_k"] == len(want)
    # pack, and the all-gather as a copy on the device
    blk, roff, toff = lay["blk"], lay["roff"], lay["toff"]
    host_all = np.full(W * blk, 0xC3, np.uint8)
    for r in range(W):
        host_all[r * blk + toff:r * blk + toff + 4] = 0                     # the rank's status word
    d_all = torch.from_numpy(host_all.copy()).cuda()
    for r, x in enumerate(ranks):
        vals, recs, gv, gr = check_pack(gpu, x["levels"], x["cand"], x["keep"], x["R"], rs.NGL)
        d_all[r * blk:r * blk + gv.n].copy_(gv.view(torch.uint8))
        d_all[r * blk + roff:r * blk + roff + gr.n].copy_(gr.view(torch.uint8))
        host_all[r * blk:r * blk + gv.n] = vals.view(np.uint8)
        host_all[r * blk + roff:r * blk + roff + gr.n] = recs.view(np.uint8)
    got = run_build(gpu, d_all, host_all, lay, W, rs.NKEY, tab, 0)
    print("W", W, pattern, "halo", c["halo"], "candidates", lay["tot_c"], "kept", lay["tot_k"], "blk", blk)
    same_records(got, want)


# ---- b. slab_count alone ----------------------------------------------------------------------------------------------
COUNT_GEOMETRY = {1: (1, 4), 6: (3, 6), 128: (8, 11), 129: (3, 6), 256: (8, 11)}            # nkey -> K, ngl
COUNT_N = (1, 255, 256, 257, 262144, 262145 + 1027)


def count_list(nkey, n, seed, key=None):
    K, ngl = COUNT_GEOMETRY[nkey]
    rng = np.random.Generator(np.random.PCG64([seed, nkey, n]))
    k = rng.integers(0, nkey, n) if key is None else np.full(n, key)
    cand = np.zeros(n, rs.CAND)
    cand["tag"] = (k // K) * ngl + k % K + 1                                # inside the contract: tag % ngl in 1 ... K
    cand["idx"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    cand["val"] = rs.special_floats(rng, n)
    keep = np.where(rng.random(n) < 0.6, rng.choice(rs.KEEP_VALUES, n), 0).astype(np.int32)
    assert ((cand["tag"] % ngl >= 1) & (cand["tag"] % ngl <= K)).all()
    return cand, keep, ngl, K


@pytest.mark.gpu
@pytest.mark.parametrize("n", COUNT_N)
@pytest.mark.parametrize("nkey", sorted(COUNT_GEOMETRY))
def test_count(gpu, nkey, n):
    cand, keep, ngl, K = count_list(nkey, n, 11)
    cnt = run_count(gpu, cand, keep, ngl, K, nkey)
    want = rs.counts(cand, keep, ngl, K, nkey)
    np.testing.assert_array_equal(cnt, want)
    assert cnt[0::2].sum() == n and cnt[1::2].sum() == (keep != 0).sum()
    if n >= 262144 and nkey > 1:
        assert (want[0::2] > 0).all() and len(set(keep.tolist())) == 5      # every key, every keep value


@pytest.mark.gpu
@pytest.mark.parametrize("nkey, n", [(6, 257), (256, 257), (129, 0), (256, 262145 + 1027)])
def test_count_zeroes_a_buffer_of_ones(gpu, nkey, n):
    cand, keep, ngl, K = count_list(nkey, n, 12)
    cnt = run_count(gpu, cand, keep, ngl, K, nkey, prefill=np.ones(2 * nkey, np.int32))
    np.testing.assert_array_equal(cnt, rs.counts(cand, keep, ngl, K, nkey))


@pytest.mark.gpu
@pytest.mark.parametrize("nkey, key", [(6, 0), (6, 5), (256, 127), (256, 128), (256, 255), (129, 128)])
def test_count_all_candidates_in_one_key(gpu, nkey, key):
    n = 3000
    cand, keep, ngl, K = count_list(nkey, n, 13, key=key)
    cnt = run_count(gpu, cand, keep, ngl, K, nkey)
    want = np.zeros(2 * nkey, np.int32)
    want[2 * key], want[2 * key + 1] = n, (keep != 0).sum()
    np.testing.assert_array_equal(cnt, want)


# ---- c. slab_pack alone -----------------------------------------------------------------------------------------------
PACK_NGL = 6
PACK_N = (1, 3, 4, 5, 1023, 1024, 1025, 262144, 262145, 262144 + 1024 * 3 + 1)
RUN_N = 4 * 1024 + 7
RUN_BOUNDARIES = (4, 64, 256, 1024, 1028, 1088, 1280, 2048, 3072, 4096)


def pack_levels():
    """Two octaves of PACK_NGL levels, 64 planes each, the local buffers 7 planes into and 3 planes in front of the
    volume."""
    lv = np.zeros(2 * PACK_NGL, rs.LEVEL)
    lv["nx"], lv["ny"], lv["nz"] = np.repeat([37, 18], PACK_NGL), np.repeat([11, 5], PACK_NGL), 64
    lv["z_off"], lv["octave"] = np.repeat([7, -3], PACK_NGL), np.repeat([0, 1], PACK_NGL)
    return lv


def pack_list(n, seed, keep=None):
    rng = np.random.Generator(np.random.PCG64([seed, n]))
    lv = pack_levels()
    cand = np.zeros(n, rs.CAND)
    cand["tag"] = rng.integers(0, 2, n) * PACK_NGL + rng.integers(1, 4, n)
    L = lv[cand["tag"]]
    cand["idx"] = rng.integers(0, 2 ** 31, n) % (L["nx"].astype(np.int64) * L["ny"] * L["nz"])
    cand["val"] = rs.special_floats(rng, n)
    R = rs.special_floats(rng, (n, 9))
    if keep is None:
        keep = np.where(rng.random(n) < 0.5, rng.choice(rs.KEEP_VALUES, n), 0).astype(np.int32)
    return lv, cand, np.ascontiguousarray(keep, np.int32), R


@pytest.mark.gpu
@pytest.mark.parametrize("n", PACK_N)
def test_pack(gpu, n):
    lv, cand, keep, R = pack_list(n, 21)
    if n <= 5:
        keep[:] = [-1, 0, 2, 0x100, 1][:n]                                  # (the smallest lists: not left to chance)
    if n > 262144:
        keep[-1] = 2                                                        # (nor the one candidate of block 256)
    vals, recs, _, _ = check_pack(gpu, lv, cand, keep, R, PACK_NGL)
    nb = (n + 1023) // 1024
    if nb > 256:
        # the second round of the scan, with a carry: kept candidates in front of block 256 and behind it
        assert (keep[:262144] != 0).any() and (keep[262144:] != 0).any()
    assert len(recs) == (keep != 0).sum()


def run_pattern(kind):
    keep = np.zeros(RUN_N, np.int32)
    for b in RUN_BOUNDARIES:
        lo, hi = {"start_on": (b, b + 3), "end_on": (b - 3, b), "across": (b - 2, b + 2)}[kind]
        keep[lo:hi] = -1
    return keep


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["start_on", "end_on", "across"])
def test_pack_keep_runs_at_the_boundaries(gpu, kind):
    keep = run_pattern(kind)
    assert 0 < (keep != 0).sum() <= 4 * len(RUN_BOUNDARIES)
    lv, cand, keep, R = pack_list(RUN_N, 22, keep)
    check_pack(gpu, lv, cand, keep, R, PACK_NGL)


@pytest.mark.gpu
def test_pack_kept_only_in_the_last_block(gpu):
    n = 3 * 1024 + 5
    keep = np.zeros(n, np.int32)
    keep[3 * 1024:] = 2
    lv, cand, keep, R = pack_list(n, 23, keep)
    _, recs, _, _ = check_pack(gpu, lv, cand, keep, R, PACK_NGL)
    assert len(recs) == 5


@pytest.mark.gpu
def test_pack_kept_only_in_block_256(gpu):
    n = 262144 + 1024 * 3 + 1
    keep = np.zeros(n, np.int32)
    keep[262144:262144 + 1024] = 0x100
    keep[262144 + 3] = 0
    lv, cand, keep, R = pack_list(n, 24, keep)
    _, recs, _, _ = check_pack(gpu, lv, cand, keep, R, PACK_NGL)
    assert len(recs) == 1023


@pytest.mark.gpu
def test_pack_indices_up_to_the_end_of_a_level_of_nearly_2_32_voxels(gpu):
    nx = ny = 2048
    nz = 1023
    lv = np.zeros(PACK_NGL, rs.LEVEL)
    lv["nx"], lv["ny"], lv["nz"], lv["nz_glob"] = nx, ny, nz, 4096
    lv["z_off"] = [0, 0, 37, -5, 0, 0]                                    # tags 1, 2, 3: none, into, in front
    plane = nx * ny
    idx = [0, 2 ** 32 - 2049, 2 ** 32 - 2 ** 22 - 2048, 2 ** 32 - 2 ** 22 - 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1,
           plane - 1, plane, 5 * plane, 6 * plane - 1, 511 * plane + 2047, 512 * plane - 2048, 1022 * plane]
    assert nx * ny * nz == 2 ** 32 - 2 ** 22 and max(idx) < 2 ** 32
    cand = np.zeros(3 * len(idx) + 2, rs.CAND)
    cand["idx"][:3 * len(idx)] = np.tile(np.array(idx, np.uint64), 3)
    cand["tag"][:3 * len(idx)] = np.repeat([1, 2, 3], len(idx))
    cand["idx"][-2:], cand["tag"][-2:] = 2 ** 32 - 1, 2                    # two that are not kept
    rng = np.random.Generator(np.random.PCG64(25))
    cand["val"] = rs.special_floats(rng, len(cand))
    R = rs.special_floats(rng, (len(cand), 9))
    keep = np.ones(len(cand), np.int32)
    keep[-2:] = 0
    _, recs, _, _ = check_pack(gpu, lv, cand, keep, R, PACK_NGL)
    # by hand, beside the restatement: the level's last voxel, the voxels around 2^31, a plane's first and last
    n = len(idx)
    for t, z_off in enumerate((0, 37, -5)):
        q = recs[t * n:(t + 1) * n]
        assert (q["o"] == 0).all() and (q["s"] == t).all()
        xyz = lambda i: (int(q["x"][i]), int(q["y"][i]), int(q["z"][i]) - z_off)
        assert xyz(0) == (0, 0, 0) and xyz(2) == (0, 2047, 1022) and xyz(3) == (2047, 2047, 1022)
        assert xyz(4) == (2047, 2047, 511) and xyz(5) == (0, 0, 512) and xyz(6) == (1, 0, 512)
        assert xyz(7) == (2047, 2047, 0) and xyz(8) == (0, 0, 1) and xyz(9) == (0, 0, 5) and xyz(10) == (2047, 2047, 5)
        assert xyz(1) == (2047, 2046, 1023)


@pytest.mark.gpu
def test_pack_copies_special_floats_bit_for_bit(gpu):
    n = 1500
    lv, cand, keep, R = pack_list(n, 26, np.ones(1500, np.int32))
    special = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0xff8fffff, 0x80000000, 0x00000001, 0x807fffff,
                        0x007fffff, 0x7f800000, 0xff800000], U32)
    cand["val"][:10] = special.view(np.float32)
    R.reshape(-1).view(U32)[5:15] = special
    R.reshape(-1).view(U32)[-10:] = special
    vals, recs, _, _ = check_pack(gpu, lv, cand, keep, R, PACK_NGL)
    np.testing.assert_array_equal(bits(vals)[:10], special)
    np.testing.assert_array_equal(bits(recs["R"]).reshape(-1)[5:15], special)


# ---- d. slab_build alone, on tables written by hand -------------------------------------------------------------------

def build_by_hand(gpu, name, stats):
    _, torch = gpu
    cnt, vals, recs = rs.hand_blocks(name)
    tab = np.array(rs.HAND[name]["tab"], U32)
    c, k = cnt[:, 0::2].sum(axis=1), cnt[:, 1::2].sum(axis=1)
    roff = rs.round16(4 * max(int(c.max()), 1))
    toff = roff + rs.round16(56 * max(int(k.max()), 1))
    lay = dict(tot_c=int(c.sum()), tot_k=int(k.sum()), roff=roff, toff=toff, blk=toff + 16)
    assert int(tab[6]) == lay["tot_k"] and int(tab[13]) == lay["tot_c"]
    host_all = gathered(lay, vals, recs, stats)
    got = run_build(gpu, torch.from_numpy(host_all.copy()).cuda(), host_all, lay, 2, 3, tab, rs.status(stats))
    same_records(got, rs.rebuild(cnt, vals, recs, 3))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(rs.HAND))
def test_build_on_hand_written_tables(gpu, name):
    got = build_by_hand(gpu, name, [0, 0])
    assert len(got) == rs.HAND[name]["tab"][6]


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["all_filled", "nothing_kept"])
@pytest.mark.parametrize("name", sorted(rs.STATUSES))
def test_build_status_header(gpu, name, table):
    stats = rs.STATUSES[name]
    want = {"all_zero": 0, "rank0_only": -7, "last_rank_only": 5, "two_different": 9}[name]
    assert rs.status(stats) == want
    build_by_hand(gpu, table, stats)


# ---- e. rows_scatter ----------------------------------------------------------------------------------------------------

def scatter_cases():
    rng = np.random.Generator(np.random.PCG64(31))
    ident = np.arange(257)
    yield "identity", 1, 257, ident
    yield "reversal", 1, 257, ident[::-1].copy()
    yield "repeated_rows", 3, 5, (rng.integers(0, 3, 257) << 24) | rng.integers(0, 5, 257)
    for nb in (1, 3, 8):
        yield "blocks_%d" % nb, nb, 40, (rng.integers(0, nb, 257) << 24) | rng.integers(0, 40, 257)
    yield "n_0", 3, 5, np.zeros(0, np.int64)
    yield "n_1", 3, 5, np.array([(2 << 24) | 4])
    yield "last_row_of_the_last_block", 8, 40, np.array([(7 << 24) | 39, 0])


SCATTER = {c[0]: c[1:] for c in scatter_cases()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCATTER))
def test_rows_scatter(gpu, name):
    hip, torch = gpu
    nb, rows, m = SCATTER[name]
    n = len(m)
    rng = np.random.Generator(np.random.PCG64([32, nb, rows]))
    blocks = rs.special_floats(rng, (nb, rows, rs.ROW))
    blk = 4 * rs.ROW * rows + 16                                            # no multiple of the row's 3072 bytes
    assert blk % (4 * rs.ROW) != 0 and blk % 16 == 0
    host_all = np.full(nb * blk, 0xC3, np.uint8)
    for b in range(nb):
        host_all[b * blk:b * blk + 4 * rs.ROW * rows] = blocks[b].reshape(-1).view(np.uint8)
    d_all = torch.from_numpy(host_all.copy()).cuda()
    m32 = m.astype(U32)
    d_map = up(torch, m32)
    dst = Guarded(torch, 4 * rs.ROW * n)
    hip.rows_scatter(dst.view(torch.float32), d_all, blk, d_map, n)
    torch.cuda.synchronize()
    got = dst.read(np.float32).reshape(n, rs.ROW)
    assert unchanged(d_all, host_all) and unchanged(d_map, m32)
    np.testing.assert_array_equal(bits(got), bits(rs.scatter(blocks, m)))
    if name == "repeated_rows":
        assert len(set(m.tolist())) < n


# ---- f. max_rows ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("nrows", [1, 2, 8])
def test_max_rows(gpu, nrows, n):
    hip, torch = gpu
    rng = np.random.Generator(np.random.PCG64([41, nrows, n]))
    b = rng.integers(0, 2 ** 31, (nrows, n), dtype=np.uint64).astype(U32)
    b = np.minimum(b, U32(0x7f800000))                                      # non-negative, no NaN; +inf stays
    # whole columns of +0.0, of subnormals, a column whose maximum is +inf, one whose maximum is subnormal beside +0.0
    plant = [np.zeros(nrows, U32), rng.integers(1, 0x00800000, nrows).astype(U32),
             np.where(np.arange(nrows) == nrows - 1, 0x7f800000, 0x7f7fffff).astype(U32),
             np.where(np.arange(nrows) == nrows // 2, 0x00000001, 0).astype(U32)]
    for i, col in enumerate(plant[:n]):
        b[:, (i * 97) % n] = col
    rows = b.view(np.float32)
    d_rows = up(torch, rows, torch.float32)
    dst = Guarded(torch, 4 * n)
    hip.max_rows(dst.view(torch.float32), d_rows, nrows, n)
    torch.cuda.synchronize()
    got = dst.read(np.float32)
    assert unchanged(d_rows, rows)
    np.testing.assert_array_equal(bits(got), bits(np.max(rows, axis=0)))
