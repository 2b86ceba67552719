"""GPU (-m gpu): the orientation stage entries on CALLER-MADE candidate lists, against the oracle and the reference.

sift3d_hip_orient (serial sums) and sift3d_hip_orient_tab (window tables, parallel sums, decisions by margin, serial
re-run of the undecided) on lists detect never produces (tests/orient_cases.py).  The bars, for both entries in every
test:

  keep   exactly the oracle's (orc_orient_conf on the same level arrays), every entry 0 or 1 -- hip.orient_tab
         pre-fills keep with -7 and 2 means undecided, so every candidate was visited and resolved;
  R      of kept candidates bit for bit the oracle's (the stage's contract); R of rejected ones is not compared;
  g8     where the list is a fixture of the reference (tests/golden/g8_*): its status, and R within 1e-5 relative.
"""
import numpy as np
import pytest

from tests import orient_cases as oc
from tests import util

F = np.float32


@pytest.fixture(scope="module")
def gpu():
    import torch
    from sift3d_amd import api, hip
    if not torch.cuda.is_available() or not api.device_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    return api, hip, torch


class Stage:
    """The level table of a list on the device, and both entries over it."""

    def __init__(self, gpu, levels):
        _, self.hip, torch = gpu
        self.dev = [dict(L, data=torch.from_numpy(L["data"]).cuda()) for L in levels]
        self.d_levels, _ = self.hip.level_table(self.dev)
        self.n = len(levels)

    def run(self, cands, thresh, tab=None):
        return {"orient": self.hip.orient(self.d_levels, cands, thresh),
                "orient_tab": self.hip.orient_tab(self.d_levels, self.n, cands, thresh, tab=tab)}


def check(got, R_o, conf, status, thresh, what=""):
    want = oc.keep_at(conf, status, thresh)
    k = want == 1
    for name, (R, keep) in got.items():
        msg = "%s %s thresh %r" % (what, name, thresh)
        assert set(np.unique(keep).tolist()) <= {0, 1}, msg
        np.testing.assert_array_equal(keep, want, err_msg=msg)
        np.testing.assert_array_equal(R[k].view(np.uint32), R_o[k].view(np.uint32), err_msg=msg)
    return want


def noise_level(seed, shape):
    """16 blobs of the survey generator plus white PCG64 noise of amplitude 0.1: measured with the oracle, such a
    level gives all three verdicts (eigenvalue-ratio REJECT, conf below and above 0.2 ... 0.4) in numbers."""
    from oracle import sift3d_oracle as so
    v = np.random.Generator(np.random.PCG64(seed)).standard_normal(shape)
    return np.ascontiguousarray(so.synth_survey(tuple(shape[::-1]), nblob=16, seed=seed) + 0.1 * v, F)


# ---- a. the g8 fixtures ----------------------------------------------------------------------------------------

def g8_on_detector(gpu, oracle_mod, name):
    """Every list of a fixture over the GPU detector's own Gaussian levels (units from the oracle's pyramid)."""
    api = gpu[0]
    g = util.load(name)
    vol, units = util.golden_input(g, oracle_mod), tuple(float(v) for v in g["units"])
    det, kp = api.Detector(), api.KeypointStore()
    assert det.detect_keypoints(api.Image.from_array(vol, units), kp) == 0
    o = oracle_mod.Oracle()
    assert o.set_volume(vol, units) == 0 and o.num_octaves == int(g["num_octaves"])
    out = {}
    for case in oc.g8_cases(g):
        c = oc.g8_case(g, case)
        lu = {}
        for oct_ in set(c["os"][:, 0].tolist()):
            lu[oct_] = tuple(u * 2.0 ** oct_ for u in units)
        levels, cands, order = oc.g8_list(c, lambda o_, s: (det.level(0, o_, s), lu[o_]))
        out[case] = (c, levels, cands, order)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", oc.G8)
def test_fixture_lists(gpu, oracle_mod, name):
    tally = {t: [0, 0] for t in oc.THRESHOLDS}                # kept, rejected over the fixture's lists
    for case, (c, levels, cands, order) in g8_on_detector(gpu, oracle_mod, name).items():
        R_o, conf, status = oc.oracle(oracle_mod, levels, cands)
        # the oracle on these levels is the reference's verdict (the fixture)
        np.testing.assert_array_equal(status, c["status"][order], err_msg=case)
        ok = status == 0
        R_ref = c["R"][order].reshape(-1, 9)
        assert util.rel_err(R_o[ok], R_ref[ok]) <= oc.RTOL
        st = Stage(gpu, levels)
        for t in oc.THRESHOLDS:
            got = st.run(cands, t)
            want = check(got, R_o, conf, status, t, "%s/%s" % (name, case))
            np.testing.assert_array_equal(want, oc.keep_at(c["conf"][order], c["status"][order], t))
            for R, _ in got.values():
                assert util.rel_err(R[want == 1], R_ref[want == 1]) <= oc.RTOL
            kept = int(want.sum())
            print(name, case, "thresh", t, "kept", kept, "rejected", len(want) - kept)
            tally[t][0] += kept
            tally[t][1] += len(want) - kept
        if name in ("g8_survey", "g8_aniso"):
            # a window clipped at each of the six faces (sift.c:93-99)
            xyz = oc.voxels(levels, cands)
            lo, hi = np.zeros(3, bool), np.zeros(3, bool)
            for tag, L in enumerate(levels):
                m = cands["tag"] == tag
                n = L["data"].shape[::-1]
                for a in range(3):
                    r = 4.5 * L["sd"] / L["units"][a]
                    lo[a] |= bool((xyz[m, a] - r < 1).any())
                    hi[a] |= bool((xyz[m, a] + r > n[a] - 2).any())
            assert lo.all() and hi.all()
            assert len(levels) == 12 and (np.bincount(cands["tag"], minlength=12) > 0).all()
    # at least 10 % kept and 10 % rejected at one or more of the thresholds
    assert any(min(k, r) >= 0.1 * (k + r) for k, r in tally.values()), tally


# ---- b. the threshold at a candidate's own confidence -------------------------------------------------------------

def own_conf_picks(conf, status, tags, extra):
    """The accepted candidates of smallest and largest conf, and `extra` more spread over the levels."""
    ok = np.nonzero((status == 0) & (conf > 0.0) & (conf < 1.0))[0]
    by = ok[np.argsort(conf[ok], kind="stable")]
    picks = [int(by[0]), int(by[-1])]
    lv = np.unique(tags[ok])
    k = 0
    while len(picks) < extra + 2:
        t = lv[(k * max(1, len(lv) // extra)) % len(lv)]
        cand = [int(i) for i in ok[tags[ok] == t] if int(i) not in picks]
        picks.append(cand[(k * 7) % len(cand)])
        k += 1
    return picks


@pytest.mark.gpu
@pytest.mark.parametrize("name, extra", [("g8_survey", 6), ("g8_noise", 6)])
def test_threshold_at_own_confidence(gpu, oracle_mod, name, extra):
    """8 candidates per list (16 in all): the whole list at thresholds conf, nextafter(conf, 1), nextafter(conf, 0)
    of the chosen candidate -- it is kept at its own conf (sift.c:1100: conf < thresh rejects), rejected one ulp
    above -- and once at 1.0."""
    (c, levels, cands, order), = g8_on_detector(gpu, oracle_mod, name).values()
    R_o, conf, status = oc.oracle(oracle_mod, levels, cands)
    st = Stage(gpu, levels)
    picks = own_conf_picks(conf, status, cands["tag"], extra)
    assert len(set(picks)) == extra + 2
    acc = conf[status == 0]
    assert conf[picks[0]] == acc[acc > 0].min() and conf[picks[1]] == acc[acc < 1].max()
    print(name, "picked conf", [float(conf[i]) for i in picks], "levels", cands["tag"][picks].tolist())
    for i in picks:
        cf = float(conf[i])
        at = check(st.run(cands, cf), R_o, conf, status, cf, name)
        up = check(st.run(cands, np.nextafter(cf, 1.0)), R_o, conf, status, np.nextafter(cf, 1.0), name)
        dn = check(st.run(cands, np.nextafter(cf, 0.0)), R_o, conf, status, np.nextafter(cf, 0.0), name)
        assert at[i] == 1 and up[i] == 0 and dn[i] == 1
    top = check(st.run(cands, 1.0), R_o, conf, status, 1.0, name)
    print(name, "kept at 1.0:", int(top.sum()))


# ---- c. the gradient threshold ------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gradient_threshold(gpu, oracle_mod):
    """|vd_win|^2 < 1e-10 (sift.c:997): the faint fixture's level at scales 1, 1e-5, 1e-6 and on either side of
    the scale where one candidate's verdict flips (bisection with the oracle); an all-zero and a constant level;
    a level that is an even function about one candidate (its window gradient cancels, its tensor does not)."""
    lists = g8_on_detector(gpu, oracle_mod, "g8_faint")
    base = lists["x1"][1][0]["data"]
    xyz = lists["x1"][0]["xyz"]
    st1 = oc.oracle(oracle_mod, lists["x1"][1], lists["x1"][2])[2][np.argsort(lists["x1"][3])]
    st6 = oc.oracle(oracle_mod, lists["x1e-6"][1], lists["x1e-6"][2])[2][np.argsort(lists["x1e-6"][3])]
    flips = np.nonzero((st1 == 0) & (st6 == 1))[0]
    print("kept at scale 1:", int((st1 == 0).sum()), "at 1e-6:", int((st6 == 0).sum()), "flip:", len(flips))
    assert len(flips) > 0                                   # the threshold is straddled
    one = xyz[flips[len(flips) // 2]][None, :]
    lo, hi = 1e-6, 1.0                                      # rejected at lo, accepted at hi
    for _ in range(60):
        mid = float(F(np.sqrt(lo * hi)))
        if mid in (lo, hi):
            break
        if oracle_mod.orient_conf(base * F(mid), (1, 1, 1), 1.6, one)[3][0] == 0:
            hi = mid
        else:
            lo = mid
    assert oracle_mod.orient_conf(base * F(lo), (1, 1, 1), 1.6, one)[3][0] == 1
    assert oracle_mod.orient_conf(base * F(hi), (1, 1, 1), 1.6, one)[3][0] == 0 and hi / lo < 1.001
    print("flip scale between", lo, hi)
    even = oracle_mod.synth_survey(33)                      # mirrored through voxel (16, 16, 16)
    even = np.ascontiguousarray(F(0.5) * (even + even[::-1, ::-1, ::-1]), F)
    levels = [oc.level(base * F(f), 1.6) for f in (1.0, 1e-5, 1e-6, lo, hi)]
    levels += [oc.level(np.zeros((20, 20, 20), F), 1.6), oc.level(np.full((20, 20, 20), 0.75, F), 1.6),
               oc.level(even, 1.6)]
    flat = oc.random_voxels(np.random.default_rng(3), (20, 20, 20), 40)
    picks = [xyz] * 5 + [flat, flat, np.array([[16, 16, 16], [15, 16, 16], [16, 17, 16], [20, 12, 9]])]
    cands = oc.make_cands(levels, picks)
    R_o, conf, status = oc.oracle(oracle_mod, levels, cands)
    tag = cands["tag"]
    assert (status[tag == 5] == 1).all() and (status[tag == 6] == 1).all()
    ev = status[tag == 7]
    assert ev[0] == 1 and (ev[1:] == 0).any()               # the centre cancels; the tensor there is not zero
    i3, i4 = np.nonzero(tag == 3)[0], np.nonzero(tag == 4)[0]
    k = flips[len(flips) // 2]
    assert status[i3[k]] == 1 and status[i4[k]] == 0
    st = Stage(gpu, levels)
    for t in (0.0, 0.4):
        want = check(st.run(cands, t), R_o, conf, status, t, "faint")
        print("thresh", t, "kept per level", [int(want[tag == g].sum()) for g in range(8)])


# ---- d. table capacity and the table of weights -------------------------------------------------------------------

@pytest.mark.gpu
def test_table_capacity_and_weight_lut(gpu, oracle_mod):
    """One 40^3 array under 13 level descriptors: sd pairs on either side of the 8192-quad and the 4096-row limit of
    k_orient_table (no table: the serial path decides every candidate of the level) and of the weight table's
    rad^2 / u^2 < 191 (tests/test_orient_candidates_host.py shows that the pairs straddle)."""
    base = oracle_mod.synth_survey(40)
    levels = []
    for units, lo, hi, what in oc.LIMIT_PAIRS:
        a, b = oc.table_count(lo, units), oc.table_count(hi, units)
        assert (a["table"], b["table"]) == ((True, True) if what == "lut" else (True, False))
        levels += [oc.level(base, lo, units), oc.level(base, hi, units)]
    levels.append(oc.level(base, oc.NO_LUT[1], oc.NO_LUT[0]))
    rng = np.random.default_rng(17)
    centre = np.array([[x, y, z] for x in (19, 20) for y in (19, 21) for z in (18, 20)])
    picks = [np.concatenate([oc.random_voxels(rng, base.shape, 56), centre]) for _ in levels]
    cands = oc.make_cands(levels, picks)
    R_o, conf, status = oc.oracle(oracle_mod, levels, cands)
    st = Stage(gpu, levels)
    for t in (0.0, 0.4):
        want = check(st.run(cands, t), R_o, conf, status, t, "capacity")
        print("thresh", t, "kept per level", np.bincount(cands["tag"], weights=want).astype(int).tolist())
        assert 0 < want.sum() < len(want)


# ---- e. window geometry -------------------------------------------------------------------------------------------

def edge_voxels(rng, shape, n):
    """x in {1, 2, 3, nx - 5 .. nx - 2} with random y, z, then n random voxels."""
    nz, ny, nx = shape
    xs = [1, 2, 3] + list(range(nx - 5, nx - 1))
    p = oc.random_voxels(rng, shape, 4 * len(xs))
    p[:, 0] = np.tile(xs, 4)
    return np.concatenate([p, oc.random_voxels(rng, shape, n)])


@pytest.mark.gpu
def test_window_geometry(gpu, oracle_mod):
    """Levels smaller than the window (5 x 6 x 7; 3^3: a box of one voxel), rows that are not whole quads with
    candidates next to the x faces (the per-voxel path of k_orient_sums), a level of few long rows."""
    rng = np.random.default_rng(23)
    shapes = [(7, 6, 5), (3, 3, 3), (23, 29, 37), (11, 9, 130)]                  # [nz, ny, nx]
    levels = [oc.level(noise_level(30 + i, s), 1.6) for i, s in enumerate(shapes)]
    every = lambda s: np.array([[x, y, z] for z in range(1, s[0] - 1) for y in range(1, s[1] - 1)
                                for x in range(1, s[2] - 1)])
    picks = [every(shapes[0]), every(shapes[1]), edge_voxels(rng, shapes[2], 120), edge_voxels(rng, shapes[3], 120)]
    assert len(picks[1]) == 1
    for p, s in zip(picks[2:], shapes[2:]):
        assert set([1, 2, 3] + list(range(s[2] - 5, s[2] - 1))) <= set(p[:, 0].tolist())
    cands = oc.make_cands(levels, picks)
    R_o, conf, status = oc.oracle(oracle_mod, levels, cands)
    st = Stage(gpu, levels)
    for t in (0.0, 0.3):
        want = check(st.run(cands, t), R_o, conf, status, t, "geometry")
        print("thresh", t, "kept per level", np.bincount(cands["tag"], weights=want, minlength=4).astype(int).tolist(),
              "of", np.bincount(cands["tag"], minlength=4).tolist())
    assert 0 < want.sum() < len(want)


@pytest.mark.gpu
def test_z_slab_level(gpu, oracle_mod):
    """Planes [10, 34) of a 48-plane volume (off = 10, nz_glob = 48) against the oracle on the WHOLE volume.  The
    kernel clamps a window to the local planes and the oracle does not: only candidates whose window --
    ceil(4.5 sd / uz) + 1 planes each way -- lies inside the local planes are compared, and that is asserted first."""
    vol = oracle_mod.synth_survey((30, 28, 48))
    off, nzl, sd = 10, 24, 1.6
    slab = oc.level(vol[off:off + nzl], sd, off=off, nz_glob=48)
    other = oc.level(noise_level(3, (20, 20, 20)), sd)           # a whole level before the slab: tags 0 and 1
    wp = oc.window_planes(sd, 1.0)
    rng = np.random.default_rng(29)
    p = oc.random_voxels(rng, (48, 28, 30), 150)
    p[:, 2] = rng.integers(off + wp, off + nzl - 1 - wp + 1, len(p))
    assert wp == 9 and (p[:, 2] - wp >= off).all() and (p[:, 2] + wp <= off + nzl - 1).all()
    assert {off + wp, off + nzl - 1 - wp} <= set(p[:, 2].tolist())
    levels = [other, slab]
    cands = oc.make_cands(levels, [oc.random_voxels(rng, (20, 20, 20), 20), p])
    R_o, conf, status = oc.oracle(oracle_mod, levels, cands, whole={1: vol})
    R_s, conf_s, status_s = oc.oracle(oracle_mod, levels, cands)           # the oracle's own slab view agrees
    assert (status == status_s).all() and (conf == conf_s).all() and R_o.tobytes() == R_s.tobytes()
    st = Stage(gpu, levels)
    for t in (0.0, 0.4):
        want = check(st.run(cands, t), R_o, conf, status, t, "slab")
    assert 0 < want[cands["tag"] == 1].sum() < len(p)


# ---- f. the launch plan ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_launch_plan_populations(gpu, oracle_mod):
    """Level populations 1, 0, 7, 8, 0, 9, 33, 257 (the guards r < q, k q + r < m of k_orient_sums; levels without
    candidates between populated ones), and the same lists shuffled inside each level: equal per candidate."""
    pops = [1, 0, 7, 8, 0, 9, 33, 257]
    rng = np.random.default_rng(31)
    levels = [oc.level(noise_level(40 + i, (20, 21, 22)), 1.6 if i % 2 else 2.0) for i in range(len(pops))]
    picks = [oc.random_voxels(rng, (20, 21, 22), m) for m in pops]
    st = Stage(gpu, levels)
    cands = oc.make_cands(levels, picks)
    assert np.bincount(cands["tag"], minlength=8).tolist() == pops
    R_o, conf, status = oc.oracle(oracle_mod, levels, cands)
    want = check(st.run(cands, 0.3), R_o, conf, status, 0.3, "plan")
    assert 0 < want.sum() < len(want)
    perm = np.concatenate([np.nonzero(cands["tag"] == g)[0][rng.permutation(m)] for g, m in enumerate(pops)])
    assert (np.diff(cands["tag"][perm]) >= 0).all() and (perm != np.arange(len(perm))).any()
    check(st.run(cands[perm], 0.3), R_o[perm], conf[perm], status[perm], 0.3, "plan shuffled")


@pytest.mark.gpu
@pytest.mark.parametrize("nlevels", [62, 63])
def test_plan_limit(gpu, oracle_mod, nlevels):
    """62 levels: the largest launch plan (ORI_PLAN_MAX); 63: sift3d_hip_orient_tab falls back to the serial kernel."""
    rng = np.random.default_rng(37)
    levels = [oc.level(noise_level(100 + i, (12, 12, 12)), 1.6) for i in range(nlevels)]
    cands = oc.make_cands(levels, [oc.random_voxels(rng, (12, 12, 12), 3) for _ in levels])
    R_o, conf, status = oc.oracle(oracle_mod, levels, cands)
    want = check(Stage(gpu, levels).run(cands, 0.2), R_o, conf, status, 0.2, "%d levels" % nlevels)
    assert 0 < want.sum() < len(want)


@pytest.mark.gpu
def test_more_undecided_than_the_fix_grid(gpu, oracle_mod):
    """9000 candidates on one 26^3 level at sd 4.4 (no table: 8192 quads are not enough): every one is undecided
    and k_orient_fix's 8192 workgroups stride over them."""
    assert not oc.table_count(4.4, (1.0, 1.0, 1.0))["table"]
    levels = [oc.level(noise_level(7, (26, 26, 26)), 4.4)]
    rng = np.random.default_rng(41)
    cands = oc.make_cands(levels, [oc.random_voxels(rng, (26, 26, 26), 9000)])
    assert len(cands) > 8192 and len(np.unique(cands["idx"])) > 4000
    R_o, conf, status = oc.oracle(oracle_mod, levels, cands)
    want = check(Stage(gpu, levels).run(cands, 0.4), R_o, conf, status, 0.4, "9000")
    print("kept", int(want.sum()), "of", len(want))
    assert 0 < want.sum() < len(want)


# ---- g. scratch reuse -----------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_scratch_reuse(gpu, oracle_mod):
    """One scratch through tab= across calls: a table is kept only while (sd, ux, uy, uz, nx, ny) of its level stay
    the same -- the offsets i0 + nx (j + ny l) depend on all of them but nz.  Interior candidates, so that the
    table's offsets, not the clipped path, are read.  After every call: the oracle's results for the CURRENT levels."""
    _, hip, torch = gpu
    rng = np.random.default_rng(43)
    n = 48

    def vol(shape, seed):
        return noise_level(seed, shape)

    def three(mid):
        return [oc.level(vol((32, 36, 40), 50), 1.6), mid, oc.level(vol((32, 36, 40), 51), 2.0)]

    def picks_for(levels):
        out = []
        for L in levels:
            m = [int(np.ceil(4.5 * L["sd"] / u)) + 5 for u in L["units"]]
            nz, ny, nx = L["data"].shape
            assert nx - 2 * m[0] > 2 and ny - 2 * m[1] > 2 and nz - 2 * m[2] > 2
            out.append(np.stack([rng.integers(m[0], nx - m[0], n), rng.integers(m[1], ny - m[1], n),
                                 rng.integers(m[2], nz - m[2], n)], 1))
        return out

    a = vol((32, 36, 40), 52)
    steps = [("first", oc.level(a, 1.6)), ("again", oc.level(a, 1.6)), ("sd", oc.level(a, 1.7)),
             ("ux", oc.level(a, 1.7, (2.0, 1.0, 1.0))), ("uz", oc.level(a, 1.7, (2.0, 1.0, 2.0))),
             ("nx", oc.level(vol((32, 36, 44), 53), 1.7, (2.0, 1.0, 2.0))),
             ("ny", oc.level(vol((32, 40, 44), 54), 1.7, (2.0, 1.0, 2.0))),
             ("nz", oc.level(vol((36, 40, 44), 55), 1.7, (2.0, 1.0, 2.0)))]
    tab = torch.zeros(hip.orient_tab_bytes(3, 3 * n), dtype=torch.uint8, device="cuda")
    prev = None
    picks = None
    for what, mid in steps:
        levels = three(mid)
        if what != "again":
            picks = picks_for(levels)
        cands = oc.make_cands(levels, picks)
        R_o, conf, status = oc.oracle(oracle_mod, levels, cands)
        st = Stage(gpu, levels)
        R, keep = hip.orient_tab(st.d_levels, 3, cands, 0.3, tab=tab)
        want = check({"orient_tab(tab=)": (R, keep)}, R_o, conf, status, 0.3, what)
        assert 0 < want.sum() < len(want), what
        if what == "again":
            assert R.tobytes() == prev[0].tobytes() and keep.tobytes() == prev[1].tobytes()
        prev = (R, keep)
    with pytest.raises(ValueError):
        hip.orient_tab(st.d_levels, 3, cands, 0.3, tab=tab[:1024])
