"""Host (no GPU): the slab driver's keypoint exchange without a device.

  table      sift3d_amd_slab_table (the tables k_slab_build searches and the layout of a rank's block, the one copy the
             driver uses) against tests/slab_restatement.py on the count pattern of every case tests/test_slab_exchange.py
             runs, and against the tables that test writes down by hand; its refusals (a total beyond 32 bits, negative
             counts, nkey, stride);
  rule       the restatement against itself: a global list cut into rank lists, counted, packed, exchanged and rebuilt
             by the stage restatements is the global compaction;
  refusals   of the device entries, before any device call: nkey 0 and 257, more candidates than the scan covers,
             and n == 0, which succeeds and touches nothing.
"""
import numpy as np
import pytest

from sift3d_amd import hip
from tests import slab_restatement as rs

PATTERNS = dict(rs.count_patterns())
FAKE = 0x1000000                                  # never dereferenced: every call below returns before a device call


def as_driver(cnt):
    """The driver's gathered blocks: the counts, padded to 16 bytes, with a status word behind them."""
    w = cnt.shape[1]
    wide = np.full((cnt.shape[0], (w + 3) // 4 * 4 + 4), -1, np.int32)
    wide[:, :w] = cnt
    return wide


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_table_on_the_chain_patterns(name):
    cnt = PATTERNS[name]
    want_tab, want = rs.table(cnt, rs.NKEY)
    for c in (cnt, as_driver(cnt)):
        tab, lay = hip.slab_table(c, rs.NKEY)
        np.testing.assert_array_equal(tab, want_tab)
        assert lay == want
    assert lay["blk"] % 16 == 0 and lay["roff"] >= 4 * lay["maxc"] and lay["toff"] - lay["roff"] >= 56 * lay["maxk"]


@pytest.mark.parametrize("name", sorted(rs.HAND))
def test_hand_written_tables(name):
    h = rs.HAND[name]
    cnt = np.array(h["cnt"], np.int32)
    tab, lay = hip.slab_table(cnt, 3)
    assert tab.tolist() == h["tab"]
    assert rs.table(cnt, 3)[0].tolist() == h["tab"]
    assert lay == rs.table(cnt, 3)[1]
    assert len(h["tab"]) == hip.slab_table_words(2, 3) == 30


def test_hand_patterns_are_the_empty_segment_patterns():
    seg = {n: np.array(h["cnt"])[:, 1::2].T.reshape(-1) for n, h in rs.HAND.items()}       # kept, in global order
    cand = {n: np.array(h["cnt"])[:, 0::2].T.reshape(-1) for n, h in rs.HAND.items()}
    assert (seg["all_filled"][:-1] > 0).all()
    assert (seg["leading_run"][:3] == 0).all() and seg["leading_run"][3] > 0
    assert (seg["trailing_run"][-3:] == 0).all() and seg["trailing_run"][2] > 0
    assert (cand["rank0_empty"][0::2] == 0).all() and (cand["rank1_empty"][1::2] == 0).all()
    assert (cand["middle_key_empty"][2:4] == 0).all()
    c, k = cand["candidates_none_kept"], seg["candidates_none_kept"]
    assert any(c[i] > 0 and k[i] == 0 and k[i + 1] == c[i + 1] > 0 for i in range(5))
    assert seg["nothing_kept"].sum() == 0 and cand["nothing_kept"].sum() > 0
    assert [int(seg["tot_k_%d" % t].sum()) for t in (255, 256, 257)] == [255, 256, 257]


def test_table_with_nkey_256_and_world_64():
    rng = np.random.Generator(np.random.PCG64(3))
    c = rng.integers(0, 1000, size=(64, 256))
    k = (c * rng.random((64, 256))).astype(np.int64)
    c[rng.random((64, 256)) < 0.3] = 0
    k = np.minimum(k, c)
    cnt = np.stack((c, k), axis=2).reshape(64, 512).astype(np.int32)
    tab, lay = hip.slab_table(cnt, 256)
    want_tab, want = rs.table(cnt, 256)
    np.testing.assert_array_equal(tab, want_tab)
    assert lay == want and lay["tot_k"] < lay["tot_c"]


def test_table_refuses_totals_beyond_32_bits():
    big = 2 ** 31 - 1
    fits = np.array([[big, 5], [big, 0], [1, 1]], np.int32)              # 2^32 - 1 candidates
    tab, lay = hip.slab_table(fits, 1)
    assert lay["tot_c"] == 2 ** 32 - 1 and tab[7] == 2 ** 32 - 1 and tab[3] == 6 and lay["tot_k"] == 6
    assert rs.table(fits, 1)[1] == lay
    for over in ([[big, 0], [big, 0], [2, 0]],                           # 2^32 candidates: the sum wraps to 0
                 [[big, big], [big, big], [big, 2]],                     # kept ones alone beyond
                 [[big, 0, big, 0], [big, 0, big, 0]]):                  # over two keys
        over = np.array(over, np.int32)
        assert rs.table(over, over.shape[1] // 2)[0] is None
        with pytest.raises(RuntimeError):
            hip.slab_table(over, over.shape[1] // 2)


def test_table_refuses_bad_arguments():
    cnt = np.array([[1, 1, 2, 0]], np.int32)
    assert hip.slab_table(cnt, 2)[1]["tot_c"] == 3
    for bad in (0, -1, 257):
        with pytest.raises(RuntimeError):
            hip.slab_table(cnt, bad)
    with pytest.raises(RuntimeError):
        hip.slab_table(cnt, 3)                                           # a stride shorter than 2 nkey counts
    with pytest.raises(RuntimeError):
        hip.slab_table(np.array([[1, 1, -2, 0]], np.int32), 2)           # a negative count
    L, lay = hip.lib(), hip.SlabLayout()
    tab = np.zeros(64, np.uint32)
    import ctypes as C
    assert L.sift3d_amd_slab_table(None, 16, 1, 2, tab.ctypes.data, C.byref(lay)) == -1
    assert L.sift3d_amd_slab_table(cnt.ctypes.data, 16, 1, 2, None, C.byref(lay)) == -1
    assert L.sift3d_amd_slab_table(cnt.ctypes.data, 16, 1, 2, tab.ctypes.data, None) == -1
    assert L.sift3d_amd_slab_table(cnt.ctypes.data, 16, 0, 2, tab.ctypes.data, C.byref(lay)) == -1
    for a in (np.zeros((1, 4), np.int64), np.zeros(4, np.int32), np.zeros((2, 8), np.int32)[:, ::2]):
        with pytest.raises(ValueError):
            hip.slab_table(a, 2)


# ---- the restatement against itself -----------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", rs.PATTERNS)
@pytest.mark.parametrize("W", rs.WORLDS)
def test_cut_exchange_rebuild_is_the_global_compaction(W, pattern):
    c = rs.chain_case(W, pattern)
    glob, keep, R = c["glob"], c["keep"], c["R"]
    assert rs.in_reference_order(glob)
    ranks = rs.cut(glob, keep, R, rs.DIMS, c["bounds"], rs.NGL, c["halo"])
    assert len(ranks) == W and sum(len(x["cand"]) for x in ranks) == len(glob)
    cnt = np.stack([rs.counts(x["cand"], x["keep"], rs.NGL, rs.K, rs.NKEY) for x in ranks])
    np.testing.assert_array_equal(cnt[:, 0::2].T, c["seg"])
    packs = [rs.packed(x["levels"], x["cand"], x["keep"], x["R"], rs.NGL) for x in ranks]
    got = rs.rebuild(cnt, [p[0] for p in packs], [p[1] for p in packs], rs.NKEY)
    want = rs.compaction(glob, keep, R)
    print("W", W, pattern, "halo", c["halo"], "candidates", len(glob), "kept", len(want))
    assert got.tobytes() == want.tobytes()
    assert len(want) == int((keep != 0).sum())
    # the pattern is what its name says
    kept = cnt[:, 1::2].T
    if pattern in ("dense", "tot_k_equals_tot_c"):
        assert len(want) == len(glob) > 256
    elif pattern == "no_keep":
        assert len(want) == 0 < len(glob)
    elif pattern.startswith("rank_empty"):
        assert (c["seg"].sum(axis=0) == 0).sum() == 1
    elif pattern.startswith("key_empty"):
        assert (c["seg"].sum(axis=1) == 0).sum() == 1
    elif pattern == "none_kept_next_to_all_kept":
        s, k = c["seg"].reshape(-1), kept.reshape(-1)
        a = (rs.NKEY // 2) * W + W - 1
        assert s[a] > 0 and k[a] == 0 and k[a + 1] == s[a + 1] > 0
    elif pattern == "one_kept_in_last_segment":
        assert kept[-1, -1] == 1 and c["seg"][-1, -1] > 1
    if c["halo"] and len(glob):
        # local coordinates: idx is not what it would be in the global volume, z_off is not the first owned plane
        L = ranks[-1]["levels"]
        assert (L["z_off"] == np.repeat([b[-2] - c["halo"] for b in c["bounds"]], rs.NGL)).all()
    if c["halo"]:
        assert (ranks[0]["levels"]["z_off"] < 0).all()


def test_compaction_keeps_the_strength_of_the_candidate_in_the_slot():
    g = np.zeros(5, rs.GLOB)
    g["x"], g["val"] = np.arange(5), np.arange(5) + 10.0
    R = np.arange(45, dtype=np.float32).reshape(5, 9)
    out = rs.compaction(g, [0, 1, 0, 0, 1], R)
    assert out["x"].tolist() == [1, 4] and out["strength"].tolist() == [10.0, 11.0]
    assert out["R"][:, 0].tolist() == [9.0, 36.0] and (out["pad"] == 0).all()


def test_status_and_scatter_restatements():
    assert rs.status([0, 0, 0]) == 0 and rs.status([4, 0]) == 4 and rs.status([0, -2]) == -2
    assert rs.status([3, 0, 9, 0]) == 9
    blocks = np.arange(2 * 3 * rs.ROW, dtype=np.float32).reshape(2, 3, rs.ROW)
    got = rs.scatter(blocks, [(1 << 24) | 2, 0, (1 << 24) | 2])
    assert got.shape == (3, rs.ROW) and got[0, 0] == 5 * rs.ROW and got[1, 0] == 0 and (got[2] == got[0]).all()


# ---- the device entries' refusals, before any device call -------------------------------------------------------------

def test_slab_count_refuses_nkey_0_and_257():
    L = hip.lib()
    for nkey in (0, 257, -1):
        assert L.sift3d_hip_slab_count(FAKE, FAKE, 10, 6, 3, nkey, FAKE, None) == -1


def test_slab_pack_refuses_more_blocks_than_the_scan_covers():
    L = hip.lib()
    most = 256 * 64 * 1024
    assert L.sift3d_hip_slab_pack(FAKE, FAKE, FAKE, FAKE, most + 1, 6, FAKE, FAKE, FAKE, None) == -1
    assert L.sift3d_hip_slab_pack(FAKE, FAKE, FAKE, FAKE, 2 ** 32 - 1, 6, FAKE, FAKE, FAKE, None) == -1


def test_no_candidates_is_a_success_that_touches_nothing():
    L = hip.lib()
    assert L.sift3d_hip_slab_pack(FAKE, FAKE, FAKE, FAKE, 0, 6, FAKE, FAKE, FAKE, None) == 0
    assert L.sift3d_hip_slab_pack(None, None, None, None, 0, 6, None, None, None, None) == 0
    assert L.sift3d_hip_rows_scatter(FAKE, FAKE, 3088, FAKE, 0, None) == 0
    assert L.sift3d_hip_max_rows(FAKE, FAKE, 4, 0, None) == 0
    assert L.sift3d_hip_max_rows(FAKE, FAKE, 0, 7, None) == 0


def test_scratch_bytes():
    f = hip.slab_pack_scratch_bytes
    assert [f(n) for n in (0, 1, 1024, 1025, 262144, 262145)] == [4, 8, 8, 12, 4 * 257, 4 * 258]
    assert f(2 ** 32 - 1) == 4 * (2 ** 22 + 1)                          # no 32-bit wrap in the rounding


def test_record_layouts_are_the_bindings():
    assert rs.CAND == hip.CAND_DTYPE and rs.LEVEL == hip.LEVEL_DTYPE
    assert rs.REC == hip.SLAB_REC_DTYPE and rs.OUT == hip.SLAB_OUT_DTYPE
    assert rs.HEADER == hip.SLAB_HEADER_BYTES and rs.ROW == hip.ROW_FLOATS


def test_bindings_want_device_tensors():
    import torch
    t = torch.zeros(12, dtype=torch.int32)
    with pytest.raises(ValueError):
        hip.slab_count(t, t, 1, 6, 3, 6, t)
    with pytest.raises(ValueError):
        hip.max_rows(t, t, 1, 1)
    with pytest.raises(ValueError):
        hip.rows_scatter(t, t, 16, t, 0)
