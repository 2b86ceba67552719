"""Host (no GPU): the inputs of tests/test_extrema_levels.py, pinned -- not the kernels.

  oracle      tests/extrema_restatement.py reproduces orc_find_extrema's candidates and orc_dogmax on the oracle's own
              DoG levels, default and cuboid builds (the oracle is pinned to the reference by the g3 / g5 fixtures), and
              the reference's records on the caller-made levels of the g9 fixtures (probe_extrema);
  conditions  on the cases of tests/extrema_cases.py: counts strictly between 0 and the number of interior voxels, every
              planted tie flips exactly its own voxel, the threshold voxels sit at thr and one ulp above it, the z-seam
              case has planted sites on both sides of a seam, the tile-count cases hit their counts, the two scan shapes
              need more than one scan chunk at both alignments of the block counts, and every instantiation and every
              route of sift3d_hip_extrema_mode is selected by a case (restated launch geometry).
"""
import json

import numpy as np
import pytest

from tests import extrema_cases as xc
from tests import extrema_restatement as xr
from tests import util

F = np.float32


def interior(shape):
    nz, ny, nx = shape
    return 3 * max(nz - 2, 0) * max(ny - 2, 0) * max(nx - 2, 0)


def keys(rec):
    return set(zip(rec["tag"].tolist(), rec["idx"].tolist()))


# ---- the restatement against the oracle and the reference -----------------------------------------------------------

@pytest.mark.parametrize("cuboid", [False, True])
@pytest.mark.parametrize("gen, n", [("survey", 32), ("lattice", (40, 24, 28))])
def test_restatement_reproduces_the_oracle(oracle_mod, gen, n, cuboid):
    so = oracle_mod
    vol = so.synth_survey(n) if gen == "survey" else so.synth_lattice(n, seed=5)
    o = so.Oracle(peak_thresh=xc.PEAK, cuboid_extrema=cuboid)
    assert o.set_volume(vol) == 0 and o.build_pyramids() == 0 and o.find_extrema() == 0
    cand = o.candidates()
    total = 0
    for oct_ in range(o.num_octaves):
        D = [o.level(1, oct_, s)[0] for s in range(-1, 4)]
        for s in range(3):                                      # (the keypoint levels: the ones the stage scans)
            assert xr.dogmax(D[s + 1]).tobytes() == F(o.dogmax(oct_, s)).tobytes()
        rec = xr.octave_records(D, xc.PEAK, cuboid=cuboid)
        c = cand[cand["o"] == oct_]
        nz, ny, nx = D[0].shape
        idx = c["x"] + nx * (c["y"] + ny * c["z"])
        np.testing.assert_array_equal(rec["idx"], idx)
        np.testing.assert_array_equal(rec["tag"], c["s"])
        np.testing.assert_array_equal(rec["val"].view(np.uint32), c["strength"].view(np.uint32))
        total += len(rec)
    print(gen, n, "cuboid" if cuboid else "8 neighbours", "candidates", total)
    assert total == len(cand) > 0
    o.close()


def g9_records(g, i, shape):
    nz, ny, nx = shape
    szyx = g["case%d_szyx" % i]
    r = np.zeros(len(szyx), xr.CAND_DTYPE)
    r["tag"] = szyx[:, 0]
    r["idx"] = szyx[:, 3] + nx * (szyx[:, 2] + ny * szyx[:, 1])
    r["val"] = g["case%d_strength" % i]
    return r


def g9_cases(name):
    """(recipe, state, peak, cuboid, the reference's records) per case of a fixture; the stored recipe must be the
    one tests/extrema_cases.py makes today."""
    g = util.load(name)
    mine = [c for c in xc.G9 if c[0] == name]
    stored = json.loads(str(g["cases"]))
    assert len(stored) == len(mine)
    for i, (c, (_, recipe, state, peak, cuboid)) in enumerate(zip(stored, mine)):
        assert c["recipe"] == json.loads(json.dumps(recipe)), "the recipe of %s case %d drifted" % (name, i)
        assert (c["state"], c["peak"], c["cuboid"]) == (state, peak, cuboid)
        yield recipe, state, peak, cuboid, g9_records(g, i, recipe["shape"])


G9_NAMES = sorted({c[0] for c in xc.G9})


@pytest.mark.parametrize("name", G9_NAMES)
def test_restatement_reproduces_the_reference_fixtures(name):
    assert util.have(name), "tests/golden/%s.npz is missing" % name
    for recipe, state, peak, cuboid, ref in g9_cases(name):
        got = xc.truth(recipe, state, peak, cuboid)
        print(name, recipe["name"], "state", state, "peak", peak, "cuboid", cuboid, "records", len(ref))
        assert got.tobytes() == ref.tobytes()


@pytest.mark.refprobe
@pytest.mark.parametrize("name", G9_NAMES)
def test_fixtures_regenerate(name):
    from oracle import make_golden, refprobe
    if not (refprobe.has_extrema() and refprobe.has_extrema(cuboid=True)):
        pytest.skip("oracle/_ref is not built here, or was built before ref_probe.c had probe_extrema")
    new, old = make_golden.g9_fixture(name), util.load(name)
    assert sorted(new) == sorted(old.files)
    for k in new:
        assert np.asarray(new[k]).tobytes() == old[k].tobytes(), k


# ---- conditions on the inputs ---------------------------------------------------------------------------------------

ALL_PLAIN = xc.SHAPES + xc.TILES + xc.TIES + xc.BORDERS + xc.EST + [xc.THRESHOLD, xc.SUBNORMAL]


@pytest.mark.parametrize("recipe", ALL_PLAIN, ids=lambda r: r["name"])
def test_levels_are_exact_and_counts_are_inside(recipe):
    for state in (0, 1):
        D, G = xc.build(recipe, state)
        for a, b in zip(xr.from_gauss(G), D):
            assert a.tobytes() == b.tobytes()                  # the Gaussian-level entries see the same DoG bits
        n = len(xc.truth(recipe, state))
        print(recipe["name"], "state", state, "candidates", n, "of", interior(recipe["shape"]))
        assert 0 < n < interior(recipe["shape"])


@pytest.mark.parametrize("recipe", xc.SCAN, ids=lambda r: r["name"])
def test_scan_shapes(recipe):
    nz, ny, nx = recipe["shape"]
    g = xr.gauss6_geometry(nx, ny, nz)
    D, G = xc.build(recipe)
    for a, b in zip(xr.from_gauss(G), D):
        assert a.tobytes() == b.tobytes()
    n = len(xc.truth(recipe))
    print(recipe["name"], g, "candidates", n)
    assert 0 < n < interior(recipe["shape"])
    assert 3 * g["nblk"] > xr.SCAN_CHUNK and g["scan_chunks"] == 2
    assert g["blk_aligned16"] == (g["nwords"] % 2 == 0)
    assert g["tiles"] % 8 != 0 and len(g["seams"]) > 1
    assert 6 * 4 * nz * ny * nx < 36e6                         # the six levels: about 34 MB


def test_scan_shapes_have_both_alignments():
    al = [xr.gauss6_geometry(*r["shape"][::-1])["blk_aligned16"] for r in xc.SCAN]
    assert sorted(al) == [False, True]
    # and a small shape whose word count is no multiple of 4 or of 128
    assert any(xr.gauss6_geometry(*r["shape"][::-1])["nwords"] % 4 for r in xc.SHAPES)


@pytest.mark.parametrize("recipe", xc.TIES + [xc.CUBOID_TIE], ids=lambda r: r["name"])
def test_each_tie_flips_exactly_its_own_voxel(recipe):
    cuboid = bool(recipe.get("cuboid"))
    nz, ny, nx = recipe["shape"]
    before, after = xc.truth(recipe, 0, cuboid=cuboid), xc.truth(recipe, 1, cuboid=cuboid)
    centres = {(s["k"] - 1, s["x"] + nx * (s["y"] + ny * s["z"])) for s in recipe["sites"]}
    print(recipe["name"], "sites", len(centres), "before", len(before), "after", len(after))
    assert len(centres) == len(recipe["sites"]) >= (18 if cuboid else 16)
    assert keys(before) - keys(after) == centres and not keys(after) - keys(before)
    if not cuboid:
        # every neighbour position, as a maximum and as a minimum
        for d in xc.DIRS8:
            for kind in ("max", "min"):
                assert any(s["label"].startswith(d + "@") and s["label"].endswith(kind) for s in recipe["sites"])


def test_tie_sites_reach_every_route():
    def xs(recipe, d):
        return {s["x"] for s in recipe["sites"] if s["label"].startswith(d + "@")}
    t16, t32, t64, seam, nx4 = xc.TIES
    for r, q in ((t16, 16), (t32, 32), (t64, 64), (seam, 16), (nx4, 16)):
        assert xr.txq(r["shape"][2]) == q
    # the segment end (ed[]): x = 4 TXQ - 1 | 4 TXQ; the 16-lane row inside a wider segment: x = 63 | 64
    for r, q in ((t16, 16), (t32, 32), (t64, 64)):
        assert 4 * q in xs(r, "x-") and 4 * q - 1 in xs(r, "x+")
        assert {2, 8} <= xs(r, "x-") and {1, 7} <= xs(r, "x+")       # same quad, adjacent lane
        ty = xr.tile_rows(r["shape"][2])
        ys = lambda d: {s["y"] for s in r["sites"] if s["label"].startswith(d + "@")}
        assert ty in ys("y-") and ty - 1 in ys("y+")                 # the halo rows above and below a tile
    assert 64 in xs(t32, "x-") and 63 in xs(t32, "x+") and 64 in xs(t64, "x-") and 63 in xs(t64, "x+")
    # the z seam: a site on its first plane looking down and on the plane before looking up
    g = xr.gauss6_geometry(*seam["shape"][::-1])
    assert g["gx"] * g["gy"] == 1 and len(g["seams"]) >= 1
    z0 = g["seams"][0]
    zs = lambda d: {s["z"] for s in seam["sites"] if s["label"].startswith(d + "@")}
    assert z0 in zs("z-") and z0 - 1 in zs("z+")
    assert xs(nx4, "x-") == {2} and xs(nx4, "x+") == {1}


def test_threshold_voxels():
    r = xc.THRESHOLD
    T = xr.threshold(xc.PEAK, xc.THR_DOGMAX)
    up = np.nextafter(T, F(1.0))
    assert T == F(0.9) and F(0.1) * F(9.0) == up != T               # the two roundings differ, by one ulp
    D, _ = xc.build(r)
    assert all(xr.dogmax(D[k]) == F(xc.THR_DOGMAX) for k in (1, 2, 3))
    nz, ny, nx = r["shape"]
    got = keys(xc.truth(r))
    want = {"at +thr": (T, False), "above +thr": (up, True), "at -thr": (-T, False), "below -thr": (-up, True),
            "positive minimum": (F(2.0), True)}
    seen = 0
    for s in r["sites"]:
        for lab, (v, kept) in want.items():
            if s["label"].startswith(lab):
                assert D[s["k"]][s["z"], s["y"], s["x"]].tobytes() == F(v).tobytes()
                assert ((s["k"] - 1, s["x"] + nx * (s["y"] + ny * s["z"])) in got) == kept, s
                # an extremum either way: without the threshold every one of them is kept
                seen += 1
    assert seen == 15
    free = keys(xr.octave_records(D, 0.0, absmax=[F(0)] * 5))
    assert all((s["k"] - 1, s["x"] + nx * (s["y"] + ny * s["z"])) in free for s in r["sites"]
               if not s["label"].startswith("dogmax"))
    assert len(xc.truth(r, peak=1.0)) == 0                          # |v| > dogmax never holds


def test_degenerate_levels_give_nothing():
    D, G = xc.build(xc.CONSTANT)
    assert all(xr.dogmax(d) == 0 for d in D) and len(xc.truth(xc.CONSTANT)) == 0
    D, G = xc.build(xc.INF)
    assert all(np.isfinite(g).all() for g in G)
    assert all(np.isinf(d).any() and np.isfinite(d).any() and not np.isnan(d).any() for d in D)
    assert all(np.isinf(xr.dogmax(d)) and np.isinf(xr.threshold(xc.PEAK, xr.dogmax(d))) for d in D)
    assert len(xc.truth(xc.INF)) == 0
    # (finite strict extrema are there: only the threshold rejects them)
    assert len(xr.octave_records(D, xc.PEAK, absmax=[F(1)] * 5)) > 0


def test_subnormal_copy_gives_the_base_candidates():
    D, G = xc.build(xc.SUBNORMAL)
    tiny = np.finfo(F).tiny
    assert all((np.abs(d) < tiny).all() for d in D) and all((np.abs(g) < tiny).all() for g in G)
    a, b = xc.truth(xc.SUBNORMAL), xc.truth(xc.SUBNORMAL_BASE)
    assert len(a) > 0 and keys(a) == keys(b)
    np.testing.assert_array_equal(a["val"], b["val"] * F(2.0 ** -140))


@pytest.mark.parametrize("recipe", xc.BORDERS, ids=lambda r: r["name"])
def test_border_plants(recipe):
    nz, ny, nx = recipe["shape"]
    D, _ = xc.build(recipe)
    got = keys(xc.truth(recipe))
    faces = kept = 0
    for s in recipe["sites"]:
        key = (s["k"] - 1, s["x"] + nx * (s["y"] + ny * s["z"]))
        if s["label"].startswith("face"):
            assert key not in got
            # strictly beyond every neighbour it has
            v = D[s["k"]][s["z"], s["y"], s["x"]]
            assert abs(v) == recipe["range"] + 17
            faces += 1
        else:
            assert key in got, s
            kept += 1
    assert faces == 12 and kept >= 8
    xs = {s["x"] for s in recipe["sites"] if not s["label"].startswith("face")}
    assert {1, nx - 2} <= xs and (nx < 66 or {63, 64} <= xs)


def test_tile_counts_and_instantiations():
    for r, (tiles, ny) in zip(xc.TILES, xc.TILE_COUNTS.items()):
        g = xr.gauss6_geometry(*r["shape"][::-1])
        assert g["tiles"] == tiles and g["txq"] == 16 and r["shape"][1] == ny
    assert sorted(xc.TILE_COUNTS) == [1, 7, 8, 9, 15, 17]
    # the remap sweeps every tile once; without its min(xcd, r) term it would not, at the counts that are no
    # multiple of 8 -- and every tile of these cases but the last (one face row) holds candidates, while the GPU test
    # fills the masks with ones before each call: a tile that is never swept shows in the records either way
    for T in list(xc.TILE_COUNTS) + [xr.gauss6_geometry(*r["shape"][::-1])["tiles"] for r in xc.SCAN]:
        assert sorted(xr.xcd_remap(T)) == list(range(T))
        naive = [(L & 7) * (T >> 3) + (L >> 3) for L in range(T)]
        assert (sorted(naive) == list(range(T))) == (T % 8 == 0 or T == 1)
    for r in xc.TILES[1:]:
        nz, ny, nx = r["shape"]
        rows = (xc.truth(r)["idx"] // nx) % ny
        assert ny % 16 == 1 and set((rows // 16).tolist()) == set(range(ny // 16))
    # every TXQ (each runs with EST off and on: all entries take every case), partial tiles in x and y, ny < TY
    rows = []
    for r in xc.SHAPES + xc.TILES + xc.SCAN:
        nz, ny, nx = r["shape"]
        g = xr.gauss6_geometry(nx, ny, nz)
        rows.append((r["name"], g["txq"], nx % (4 * g["txq"]) != 0, ny % g["ty"] != 0, ny < g["ty"], len(g["seams"])))
        print("%-18s TXQ %2d TY %2d tiles %4d (%d x %d x %d, ts %d) nwords %6d nblk %5d blk16 %d chunks %d"
              % (r["name"], g["txq"], g["ty"], g["tiles"], g["gx"], g["gy"], g["gz"], g["ts"], g["nwords"], g["nblk"],
                 g["blk_aligned16"], g["scan_chunks"]))
    for q in (16, 32, 64):
        mine = [x for x in rows if x[1] == q]
        assert any(x[2] for x in mine) and any(not x[2] for x in mine)        # partial and whole tiles in x
        assert any(x[3] for x in mine) and any(not x[3] for x in mine)        # and in y
    assert any(x[4] for x in rows) and any(x[5] for x in rows)
    shapes = [tuple(r["shape"]) for r in xc.SHAPES]
    assert {s[2] for s in shapes} >= {4, 8, 64, 68, 128, 132, 256, 260}
    assert {s[1] for s in shapes} >= {3, 16, 17, 19, 8, 11, 4, 7} and {s[0] for s in shapes} >= {3, 5, 35}


def test_z_seam_case_has_candidates_on_both_sides():
    seam = [x for x in xc.SHAPES if "seam" in x["name"]]
    assert {xr.txq(r["shape"][2]) for r in seam} == {16, 32, 64}
    for r in seam:
        nz, ny, nx = r["shape"]
        g = xr.gauss6_geometry(nx, ny, nz)
        assert g["gx"] * g["gy"] == 1 and g["seams"] == [18]
        z = xc.truth(r)["idx"] // (nx * ny)
        assert (z == g["seams"][0] - 1).any() and (z == g["seams"][0]).any()


def test_every_mode_route_is_selected():
    routes = set()
    for c in xc.MODE_CASES:
        nz, ny, nx = c["shape"]
        z = c.get("z", (1, nz - 1))
        same = isinstance(z, tuple)
        z0 = z if same else z[0]
        route = xr.mode_route(nx, nz, c["nlevels"], bool(c.get("cuboid")), True, not c.get("off4"), same, *z0)
        print("%-28s -> %s" % (c["name"], route))
        assert route == c["route"]
        routes.add(route)
        _, levels = xc.mode_levels(c)
        n = len(xr.records(levels, xc.PEAK, bool(c.get("cuboid"))))
        total = sum(max(L["z_hi"] - L["z_lo"], 0) for L in levels) * (ny - 2) * (nx - 2)
        assert (n == 0 and total == 0) or 0 < n < total
    assert routes == {"sweep3", "mask", "mask_cuboid"}
    assert {c["nlevels"] for c in xc.MODE_CASES} >= {1, 2, 3, 4, 8}
    assert {c["shape"][2] for c in xc.MODE_CASES} >= {5, 63, 65, 66}
    assert not xr.gauss6_covered(5, 5) and not xr.gauss6_covered(8, 2) and not xr.gauss6_covered(8, 5, 0, 4)
    assert not xr.gauss6_covered(8, 5, 1, 5) and not xr.gauss6_covered(8, 5, aligned=False) and xr.gauss6_covered(8, 3)


def test_est_cases():
    for r in xc.EST:
        D, _ = xc.build(r)
        sub = [xr.sub_lattice_max(d) for d in D]
        full = [xr.dogmax(d) for d in D]
        print(r["name"], "lattice", sub, "exact", full)
        assert all(s <= f for s, f in zip(sub, full))
        if r["name"] == "est_zero_lattice":
            assert all(s == 0 for s in sub) and all(f > 0 for f in full)
        else:
            assert all(s < f for s, f in zip(sub, full))            # the maximum is off the lattice
            z = r["plants"][0][1]
            for d, f in zip(D, full):
                assert (np.abs(d) == f).sum() == 1 and abs(d[z].max()) == f
    assert xr.sub_lattice_planes(3) == [1] and xr.sub_lattice_planes(6) == [1] and xr.sub_lattice_planes(7) == [1, 6]
    assert xr.sub_lattice_planes(1) == [0] and xr.sub_lattice_planes(2) == [1]


def test_sweep_segments_restated():
    # about 2048 workgroups in all, segments of 16 planes or more; the 512^3 octave: 128 tiles -> 16 segments of 32
    assert xr.sweep_segments(510, 2 * 128) == 64 and xr.sweep_segments(33, 1) == 17 and xr.sweep_segments(3, 1) == 3
    assert xr.sweep_segments(31, 1) == 31 and xr.sweep_segments(32, 1) == 16
