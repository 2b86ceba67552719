"""GPU (-m gpu): the extrema stage entries on CALLER-MADE levels, bit for bit against tests/extrema_restatement.py.

sift3d_amd/csrc/sift3d_extrema.hip on levels detect never produces (tests/extrema_cases.py): exact ties on every
route a neighbour takes to the comparison, voxels at the threshold and one ulp above it, plants on and next to the
faces, slabs, the sub-lattice bounds of the EST path, more than one scan chunk, appends and short outputs, and octave
lists for the joint finish.  Every comparison is of the count and of the records' bytes in order; the output lies
between guard bands of sentinel words and the scratch is filled with ones before every call.  "All entries" are

  mode        sift3d_hip_extrema_mode on the stored DoG levels (k_extrema_sweep3),
  gauss6      sift3d_hip_extrema_gauss6 on the Gaussian levels with the exact maxima (k_extrema_sweep3g<TXQ, false>),
  est 1+2     sift3d_hip_dogmax_sub, then sift3d_hip_extrema_gauss6_est_phase phase 1 and phase 2 (<TXQ, true>),
  est 0       the same with phase 0,
  est+finish  phase 1, then sift3d_hip_extrema_gauss6_finish;

the EST entries also give the restated lattice maxima and the exact maxima bit for bit.  Which instantiation and
route a case selects is the host twin's business (tests/test_extrema_levels_host.py prints the table).
"""
import numpy as np
import pytest

from tests import extrema_cases as xc
from tests import extrema_restatement as xr

F = np.float32
SENTINEL = 0x5EA7BEEF                                       # as idx / tag: far outside any level; as val: 6e18
GUARD = 64                                                  # words before and after the records
ENTRIES = ("mode", "gauss6", "est 1+2", "est 0", "est+finish")


@pytest.fixture(scope="module")
def gpu():
    import torch
    from sift3d_amd import api, hip
    if not torch.cuda.is_available() or not api.device_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    assert hip.CAND_DTYPE == xr.CAND_DTYPE
    return hip, torch


class Out:
    """Room for `room` records carved out of a buffer of sentinel words; *d_count starts at `start`."""

    def __init__(self, torch, room, start=0):
        self.torch, self.room, self.start = torch, room, start
        self.buf = torch.full((2 * GUARD + 3 * room,), SENTINEL, dtype=torch.int32, device="cuda")
        self.count = torch.full((1,), start, dtype=torch.int32, device="cuda")
        self.ptr = self.buf.data_ptr() + 4 * GUARD

    def result(self, cap):
        """(final *d_count, the records written after `start`); everything else must still hold the sentinel."""
        total = int(self.count.item())
        b = self.buf.cpu().numpy()
        hi = max(min(cap, total), self.start)                # records lie at positions start <= pos < min(cap, count)
        assert np.all(b[:GUARD + 3 * self.start] == SENTINEL), "words before the append position were written"
        assert np.all(b[GUARD + 3 * hi:] == SENTINEL), "words beyond min(cap, count) were written"
        return total, b[GUARD + 3 * self.start:GUARD + 3 * hi].copy().view(xr.CAND_DTYPE)

    def untouched(self):
        return int(self.count.item()) == self.start and bool((self.buf == SENTINEL).all().item())


class Octave:
    """One octave's levels on the device: D (stored DoG) and G (Gaussian), their maxima, and the entries."""

    def __init__(self, gpu, D, G, tag0=0):
        self.hip, self.torch = gpu
        t = self.torch
        self.nz, self.ny, self.nx = D[0].shape
        self.D_host, self.tag0 = D, tag0
        self.D = [t.from_numpy(np.ascontiguousarray(d)).cuda() for d in D]
        self.G = [t.from_numpy(np.ascontiguousarray(g)).cuda() for g in G]
        self.maxima = xc.maxima(D)
        self.absmax = t.from_numpy(self.maxima.copy()).cuda()
        self.wb = self.hip.extrema_work_bytes(self.nx, self.ny, self.nz, 3)

    def work(self):
        return self.torch.full((self.wb,), 0xFF, dtype=self.torch.uint8, device="cuda")      # masks of ones

    def dims(self):
        return self.nx, self.ny, self.nz

    def est(self):
        """dogmax_sub into zeros; the restated lattice maxima bit for bit, lower bounds of the exact ones."""
        d_est = self.torch.zeros(5, dtype=self.torch.float32, device="cuda")
        assert self.hip.dogmax_sub(self.G, *self.dims(), d_est) == 0
        got = d_est.cpu().numpy()
        want = np.array([xr.sub_lattice_max(d) for d in self.D_host], F)
        assert got.tobytes() == want.tobytes(), (got, want)
        assert np.all(got <= self.maxima)
        return d_est

    def run(self, entry, peak, out, cap, z=None):
        hip, t = self.hip, self.torch
        nx, ny, nz = self.dims()
        z_lo, z_hi = (1, nz - 1) if z is None else z
        work = self.work()
        a = (out.ptr, cap, out.count, work, self.wb)
        if entry == "mode":
            lv = [dict(prev=self.D[k - 1], cur=self.D[k], next=self.D[k + 1], absmax=self.absmax[k:k + 1], z_lo=z_lo,
                       z_hi=z_hi, tag=self.tag0 + k - 1) for k in (1, 2, 3)]
            assert hip.extrema_into(lv, nx, ny, nz, peak, *a) == 0
        elif entry == "gauss6":
            assert hip.extrema_gauss6(self.G, self.absmax, nx, ny, nz, z_lo, z_hi, self.tag0, peak, *a) == 0
        elif entry == "gauss6 1+2":
            for phase in (1, 2):
                assert hip.extrema_gauss6(self.G, self.absmax, nx, ny, nz, z_lo, z_hi, self.tag0, peak, *a,
                                          phase=phase) == 0
        else:
            assert z is None
            d_est, d_exact = self.est(), t.zeros(5, dtype=t.float32, device="cuda")
            e = (self.G, d_est, d_exact, nx, ny, nz, self.tag0, peak) + a
            if entry == "est 1+2":
                assert hip.extrema_gauss6_est_phase(*e, phase=1) == 0
                assert out.untouched()                                  # phase 1 touches d_work only
                assert hip.extrema_gauss6_est_phase(*e, phase=2) == 0
            elif entry == "est 0":
                assert hip.extrema_gauss6_est_phase(*e, phase=0) == 0
            else:
                assert hip.extrema_gauss6_est_phase(*e, phase=1) == 0
                octs = [dict(gauss=self.G, nx=nx, ny=ny, nz=nz, tag0=self.tag0, d_work=work, work_bytes=self.wb)]
                assert hip.extrema_gauss6_finish(octs, peak, out.ptr, cap, out.count) == 0
            got = d_exact.cpu().numpy()
            assert got.tobytes() == self.maxima.tobytes(), ("exact maxima", got, self.maxima)
        return out.result(cap)

    def truth(self, peak, z=None):
        z = (None, None) if z is None else z
        return xr.octave_records(self.D_host, peak, self.maxima, self.tag0, z[0], z[1])


def all_entries(gpu, recipe, state=1, peak=xc.PEAK, entries=ENTRIES):
    """Every entry on a recipe's levels against the restatement; returns the records."""
    D, G = xc.build(recipe, state)
    o = Octave(gpu, D, G)
    want = o.truth(peak)
    counts = {}
    for e in entries:
        out = Out(gpu[1], len(want) + 1)
        n, rec = o.run(e, peak, out, len(want) + 1)
        counts[e] = n
        assert n == len(want), (recipe["name"], e, n, len(want))
        assert rec.tobytes() == want.tobytes(), (recipe["name"], e)
    print(recipe["name"], "state", state, "peak", peak, "restatement", len(want), counts)
    return want


def keys(rec):
    return set(zip(rec["tag"].tolist(), rec["idx"].tolist()))


# ---- a. every instantiation and route ---------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("recipe", xc.SHAPES + xc.TILES, ids=lambda r: r["name"])
def test_shapes_all_entries(gpu, recipe):
    assert len(all_entries(gpu, recipe)) > 0


# ---- b. ties ------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("recipe", xc.TIES, ids=lambda r: r["name"])
def test_ties_on_every_route(gpu, recipe):
    nz, ny, nx = recipe["shape"]
    before, after = all_entries(gpu, recipe, 0), all_entries(gpu, recipe, 1)
    centres = {(s["k"] - 1, s["x"] + nx * (s["y"] + ny * s["z"])) for s in recipe["sites"]}
    assert centres <= keys(before) and not centres & keys(after)     # a candidate before the tie, none after


@pytest.mark.gpu
def test_ties_cuboid(gpu):
    recipe = xc.CUBOID_TIE
    nz, ny, nx = recipe["shape"]
    seen = []
    for state in (0, 1):
        D, G = xc.build(recipe, state)
        o = Octave(gpu, D, G)
        want = xr.octave_records(D, xc.PEAK, o.maxima, cuboid=True)
        lv = [dict(prev=o.D[k - 1], cur=o.D[k], next=o.D[k + 1], absmax=o.absmax[k:k + 1], z_lo=1, z_hi=nz - 1,
                   tag=k - 1) for k in (1, 2, 3)]
        out = Out(gpu[1], len(want) + 1)
        assert o.hip.extrema_into(lv, nx, ny, nz, xc.PEAK, out.ptr, len(want) + 1, out.count, o.work(), o.wb,
                                  cuboid=True) == 0
        n, rec = out.result(len(want) + 1)
        print(recipe["name"], "state", state, "restatement", len(want), "mode cuboid", n)
        assert n == len(want) and rec.tobytes() == want.tobytes()
        seen.append(keys(rec))
    centres = {(s["k"] - 1, s["x"] + nx * (s["y"] + ny * s["z"])) for s in recipe["sites"]}
    assert centres <= seen[0] and not centres & seen[1]


# ---- c. the threshold ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_threshold_voxels(gpu):
    r = xc.THRESHOLD
    nz, ny, nx = r["shape"]
    got = keys(all_entries(gpu, r))
    for s in r["sites"]:
        key = (s["k"] - 1, s["x"] + nx * (s["y"] + ny * s["z"]))
        lab = s["label"]
        if lab.startswith("at "):
            assert key not in got, lab                                # |v| == thr: rejected
        elif not lab.startswith("dogmax"):
            assert key in got, lab                                    # one ulp beyond; a positive minimum
    assert len(all_entries(gpu, r, peak=1.0)) == 0                    # |v| > dogmax never holds


@pytest.mark.gpu
@pytest.mark.parametrize("recipe", [xc.CONSTANT, xc.INF], ids=lambda r: r["name"])
def test_degenerate_levels_give_nothing(gpu, recipe):
    assert len(all_entries(gpu, recipe)) == 0


@pytest.mark.gpu
def test_subnormal_levels(gpu):
    a, b = all_entries(gpu, xc.SUBNORMAL), all_entries(gpu, xc.SUBNORMAL_BASE)
    assert len(a) > 0 and keys(a) == keys(b)


# ---- d. borders ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("recipe", xc.BORDERS, ids=lambda r: r["name"])
def test_borders(gpu, recipe):
    nz, ny, nx = recipe["shape"]
    got = keys(all_entries(gpu, recipe))
    for s in recipe["sites"]:
        key = (s["k"] - 1, s["x"] + nx * (s["y"] + ny * s["z"]))
        assert (key in got) == (not s["label"].startswith("face")), s


# ---- e. slabs and the stored-DoG entry's routes -------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("z", [(2, 5), (1, 2), (7, 8), (4, 4), (5, 3)])
def test_gauss6_slabs(gpu, z):
    recipe = xc.plain("9x19x68 slab", 111, (9, 19, 68))
    D, G = xc.build(recipe)
    o = Octave(gpu, D, G, tag0=4)
    want = o.truth(xc.PEAK, z)                                        # the whole volume's maxima
    assert (len(want) > 0) == (z[1] > z[0])
    counts = {}
    for e in ("mode", "gauss6", "gauss6 1+2"):
        out = Out(gpu[1], len(want) + 1)
        n, rec = o.run(e, xc.PEAK, out, len(want) + 1, z)
        counts[e] = n
        assert n == len(want) and rec.tobytes() == want.tobytes(), e
    print(recipe["name"], "planes", z, "restatement", len(want), counts)


@pytest.mark.gpu
@pytest.mark.parametrize("case", xc.MODE_CASES, ids=lambda c: c["name"])
def test_mode_routes(gpu, case):
    hip, torch = gpu
    S, levels = xc.mode_levels(case)
    nz, ny, nx = case["shape"]
    cuboid = bool(case.get("cuboid"))
    want = xr.records(levels, xc.PEAK, cuboid)
    n = nz * ny * nx
    off = 1 if case.get("off4") else 0
    dev = []
    for a in S:
        flat = torch.zeros(n + 4, dtype=torch.float32, device="cuda")
        flat[off:off + n] = torch.from_numpy(a.reshape(-1)).cuda()
        dev.append(flat[off:off + n])
        assert dev[-1].data_ptr() % 16 == 4 * off
    absmax = torch.from_numpy(np.array([L["absmax"] for L in levels], F)).cuda()
    lv = [dict(prev=dev[i], cur=dev[i + 1], next=dev[i + 2], absmax=absmax[i:i + 1], z_lo=L["z_lo"], z_hi=L["z_hi"],
               tag=L["tag"]) for i, L in enumerate(levels)]
    wb = hip.extrema_work_bytes(nx, ny, nz, len(lv))
    work = torch.full((wb,), 0xFF, dtype=torch.uint8, device="cuda")
    out = Out(torch, len(want) + 1)
    assert hip.extrema_into(lv, nx, ny, nz, xc.PEAK, out.ptr, len(want) + 1, out.count, work, wb, cuboid=cuboid) == 0
    got_n, rec = out.result(len(want) + 1)
    print(case["name"], case["route"], "restatement", len(want), "mode", got_n)
    assert got_n == len(want) and rec.tobytes() == want.tobytes()


@pytest.mark.gpu
def test_uncovered_configurations_return_1_and_write_nothing(gpu):
    hip, torch = gpu

    def levels(shape, off=0):
        n = int(np.prod(shape))
        flat = [torch.ones(n + 4, dtype=torch.float32, device="cuda") for _ in range(6)]
        return [f[off:off + n] for f in flat]

    absmax = torch.ones(5, dtype=torch.float32, device="cuda")
    for what, (nz, ny, nx), off, z in (("nx % 4", (5, 6, 5), 0, None), ("nx % 4", (5, 6, 66), 0, None),
                                       ("4 bytes off", (5, 6, 8), 1, None), ("nz < 3", (2, 6, 8), 0, (1, 1)),
                                       ("z_lo < 1", (5, 6, 8), 0, (0, 4)), ("z_hi > nz - 1", (5, 6, 8), 0, (1, 5))):
        G = levels((nz, ny, nx), off)
        wb = hip.extrema_work_bytes(nx, ny, nz, 3)
        work = torch.full((wb,), 0xFF, dtype=torch.uint8, device="cuda")
        z_lo, z_hi = (1, nz - 1) if z is None else z
        out = Out(torch, 8, start=3)
        for phase in (None, 0, 1, 2):
            assert hip.extrema_gauss6(G, absmax, nx, ny, nz, z_lo, z_hi, 0, xc.PEAK, out.ptr, 8, out.count, work, wb,
                                      phase=phase) == 1, (what, phase)
        if z is None:
            d_est = torch.zeros(5, dtype=torch.float32, device="cuda")
            d_exact = torch.zeros(5, dtype=torch.float32, device="cuda")
            for phase in (0, 1, 2):
                assert hip.extrema_gauss6_est_phase(G, d_est, d_exact, nx, ny, nz, 0, xc.PEAK, out.ptr, 8, out.count,
                                                    work, wb, phase=phase) == 1, (what, phase)
            if what != "nz < 3":
                assert hip.dogmax_sub(G, nx, ny, nz, d_est) == 1, what
            assert not d_est.any().item() and not d_exact.any().item()
        assert out.untouched() and bool((work == 0xFF).all().item()), what
        print(what, (nz, ny, nx), "-> 1, nothing written")


# ---- f. EST -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("recipe", xc.EST, ids=lambda r: r["name"])
def test_est_maxima_off_the_lattice(gpu, recipe):
    # (Octave.est and Octave.run compare the lattice maxima and the gathered exact maxima bit for bit)
    assert len(all_entries(gpu, recipe)) > 0


# ---- g. scan, emit, append, cap -----------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("recipe", xc.SCAN, ids=lambda r: r["name"])
def test_scan_chunks_append_and_cap(gpu, recipe):
    """More than one scan chunk (3 * nblk > 8192) at both alignments of the block counts: appended after five
    records, through the stored-DoG entry, the EST entry and the joint finish; then phase 2 alone at four caps."""
    hip, torch = gpu
    D, G = xc.build(recipe)
    o = Octave(gpu, D, G, tag0=7)
    want = o.truth(xc.PEAK)
    total = 5 + len(want)
    counts = {}
    for e in ("mode", "est 0", "est+finish"):
        out = Out(torch, total + 1, start=5)
        n, rec = o.run(e, xc.PEAK, out, total + 1)
        counts[e] = n - 5
        assert n == total and rec.tobytes() == want.tobytes(), e
    print(recipe["name"], "restatement", len(want), counts)
    nx, ny, nz = o.dims()
    work = o.work()
    assert hip.extrema_gauss6(o.G, o.absmax, nx, ny, nz, 1, nz - 1, 7, xc.PEAK, None, 0, None, work, o.wb,
                              phase=1) == 0
    keep = work.clone()
    for cap in (0, total - 1, total, total + 1):
        work.copy_(keep)                                              # (phase 2 turns the counts into offsets)
        out = Out(torch, total + 1, start=5)
        assert hip.extrema_gauss6(o.G, o.absmax, nx, ny, nz, 1, nz - 1, 7, xc.PEAK, out.ptr, cap, out.count, work,
                                  o.wb, phase=2) == 0
        n, rec = out.result(cap)
        m = max(min(cap, total) - 5, 0)
        print(recipe["name"], "cap", cap, "count", n, "records written", len(rec))
        assert n == total and len(rec) == m and rec.tobytes() == want[:m].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_append_and_cap_small(gpu, entry):
    recipe = xc.SHAPES[3]
    D, G = xc.build(recipe)
    o = Octave(gpu, D, G)
    want = o.truth(xc.PEAK)
    total = 5 + len(want)
    for cap in (0, total - 1, total, total + 1):
        out = Out(gpu[1], total + 1, start=5)
        n, rec = o.run(entry, xc.PEAK, out, cap)
        m = max(min(cap, total) - 5, 0)
        assert n == total and len(rec) == m and rec.tobytes() == want[:m].tobytes(), cap
    print(recipe["name"], entry, "count", len(want), "caps 0,", total - 1, total, total + 1)


# ---- h. the joint finish ------------------------------------------------------------------------------------------

def octave_list(kinds):
    """Recipes of an octave list: an int picks xc.FINISH_DIMS, 'c' an all-constant octave of the dims before it."""
    out, dims = [], xc.FINISH_DIMS[0]
    for i, k in enumerate(kinds):
        if k == "c":
            out.append(dict(xc.CONSTANT, shape=list(dims)))
        else:
            dims = xc.FINISH_DIMS[k]
            out.append(xc.plain("oct %d" % i, 200 + i, dims))
    return out


LISTS = {"1": [0], "2": [0, 1], "5": [0, 1, 2, 3, 4], "constant first": ["c", 0, 1], "constant middle": [0, "c", "c", 2],
         "constant last": [1, 4, "c"], "12": [0, "c", 1, 2, 3, 4, 4, "c", 3, 2, 1, "c"]}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LISTS))
def test_finish_octave_lists(gpu, name):
    hip, torch = gpu
    octs = []
    for i, r in enumerate(octave_list(LISTS[name])):
        D, G = xc.build(r)
        octs.append(Octave(gpu, D, G, tag0=3 * i))
    assert len(octs) <= hip.EXTREMA_MAX_OCT == xr.MAX_OCT
    want = np.concatenate([o.truth(xc.PEAK) for o in octs])
    # per-octave phase-0 calls, appending in octave order
    a = Out(torch, len(want) + 1)
    for o in octs:
        assert hip.extrema_gauss6(o.G, o.absmax, *o.dims(), 1, o.nz - 1, o.tag0, xc.PEAK, a.ptr, len(want) + 1, a.count,
                                  o.work(), o.wb, phase=0) == 0
    n_a, rec_a = a.result(len(want) + 1)
    # phase 1 per octave (EST on the even ones), one finish
    b = Out(torch, len(want) + 1)
    desc = []
    for i, o in enumerate(octs):
        work = o.work()
        if i % 2 == 0:
            d_exact = torch.zeros(5, dtype=torch.float32, device="cuda")
            assert hip.extrema_gauss6_est_phase(o.G, o.est(), d_exact, *o.dims(), o.tag0, xc.PEAK, None, 0, None, work,
                                                o.wb, phase=1) == 0
        else:
            assert hip.extrema_gauss6(o.G, o.absmax, *o.dims(), 1, o.nz - 1, o.tag0, xc.PEAK, None, 0, None, work, o.wb,
                                      phase=1) == 0
        desc.append(dict(gauss=o.G, nx=o.nx, ny=o.ny, nz=o.nz, tag0=o.tag0, d_work=work, work_bytes=o.wb))
    assert hip.extrema_gauss6_finish(desc, xc.PEAK, b.ptr, len(want) + 1, b.count) == 0
    n_b, rec_b = b.result(len(want) + 1)
    print("octaves", name, [o.dims() for o in octs], "restatement", len(want), "per octave", n_a, "finish", n_b)
    assert n_a == n_b == len(want) > 0
    assert rec_a.tobytes() == want.tobytes() and rec_b.tobytes() == want.tobytes()
    if name == "12":
        # one octave more than a launch takes: 1, and neither d_out nor *d_count is touched
        c = Out(torch, 8, start=2)
        assert hip.extrema_gauss6_finish(desc + desc[:1], xc.PEAK, c.ptr, 8, c.count) == 1
        assert hip.extrema_gauss6_finish([], xc.PEAK, c.ptr, 8, c.count) == 1
        assert c.untouched()
