"""How the entries of sift3d_amd/hip.py are called, not what they compute (the numbers are held elsewhere): two
contracts of include/sift3d_amd.h on every entry that takes a work buffer or a stream.

A. d_work holds the library's own *_work_bytes() and nothing is assumed of its contents.  Every work-taking wrapper runs
   on a work view of exactly that size (rounded up to 4 as the wrappers round it) between two guard bands, the whole
   tensor filled with 0xFF (NaN as float and double, 2^64 - 1 as a counter) and then with 0x00, twice in a row on each
   fill without refilling.  Both bands must keep the fill and every result must be, byte for byte, that of the same call
   with work=None.
B. everything an entry does is ordered on the caller's stream.  Every entry runs on a fresh stream on zeroed twins of
   its device inputs, into which the real inputs are copied on that stream behind some milliseconds of queued work; the
   result must be that of the default stream, and must differ from that of the zeroed inputs, which is what makes a
   launch, clear or upload on another stream visible.

CALLS of tests/test_registration_wrappers.py is the first table (the seventeen registration wrappers); ROWS here is the
second, the work-taking wrappers outside them, with the library's size of each call beside it.  Two input sets: S, that
file's, and P, the padding set below.

P differs from the shape first meant for it, fixed (9, 11, 70): with the spacing (4, 3, 2) that grid's level-0 lattice
is 21 x 7 x 8, whose byte count 3 * gx * gy * gz * 4 is a multiple of 16, so no padding of a lattice slot would be
exercised.  (11, 9, 70), the same 6930 voxels, has the level-0 lattice 21 x 6 x 9.  Level 0's is the size of every
lattice slot in the drivers' layouts (five float lattices "of level 0's size", sift3d_ffd.c), and it is the one
asserted.  That of every level cannot be had at this size: an exhaustive search over fixed grids [3..19, 3..19, 65..89]
and every spacing in [1, 6]^3 finds no grid under 13090 voxels on which the lattices of all three levels have a byte
count that is no multiple of 16 while all three levels' voxel counts are no multiple of 4; levels 1 and 2 of P have
lattices 12 x 5 x 6 and 8 x 4 x 5."""
import collections

import numpy as np
import pytest

from tests import test_registration_wrappers as rw

pytestmark = pytest.mark.gpu

P = rw.Set(fshape=(11, 9, 70), mshape=(10, 9, 67), spacing=(4, 3, 2), levels=3, evaluations=3, bins=5, channels=2)
SETS = {"S": rw.S, "P": P}
TILE_X = 64                                                # TX of sift3d_resample.h: outputs per tile along x
SIM_BINS, LABELS, N_LABELS = 6, (1, 2), 3
SIGMA, ALPHA, SIGMA_FLUID, SIGMA_DIFFUSION, SQUARINGS = 1.6, 0.8, 1.0, 1.5, 2
MIN_BAND = 65536


# ---- the second table ------------------------------------------------------------------------------------------------
# call(h, x, kw): the wrapper on the inputs x with the keyword arguments kw (work=, the masks); what a call writes in
# place is cloned first, so that no call changes x.  size(h, x, masked): the library's own size in bytes of that call's
# work buffer.  masks(h, x): the mask arguments of the masked run, None where the entry takes none.  dtype: of the work
# tensor where the wrapper asks for one.
Row = collections.namedtuple("Row", "call size masks dtype", defaults=(None, "uint8"))


def _g(t):
    """(nx, ny, nz) of a volume, stack or field"""
    return tuple(t.shape[-3:])[::-1]


def _pair_masks(h, x):
    return dict(mask_fixed=x["WF"], mask_moving=x["WM"])


def _level_masks(levels):
    """one mask per level: level 0's, and ones below"""
    def masks(h, x):
        import torch

        def per_level(W):
            return [W] + [torch.ones(g, dtype=torch.float32, device="cuda")
                          for g in rw.pyramid(h, W.shape, levels(x))[1:]]
        return dict(masks_fixed=per_level(x["WF"]), masks_moving=per_level(x["WM"]))
    return masks


def _similarity(transform, moving="M", masks=_pair_masks):
    return Row(lambda h, x, kw: h.similarity(x["F"], x[moving], transform(x), SIM_BINS, rw.RANGE, rw.RANGE, **kw),
               lambda h, x, masked: h.lib().sift3d_amd_similarity_work_bytes(*_g(x["F"]), SIM_BINS), masks)


def _distance(mode):
    return Row(lambda h, x, kw: h.distance(x["mask"], (1.0, 1.5, 2.0), mode, **kw),
               lambda h, x, masked: h.lib().sift3d_amd_distance_work_bytes(*_g(x["mask"])))


def _empty_like(t, *lead):
    import torch
    return torch.empty(tuple(lead) + tuple(t.shape), dtype=torch.float32, device="cuda")


def _demons_force(h, x, kw):
    step = _empty_like(x["field"])
    stats = h.demons_force(x["F"], x["F2"], x["field"], step, ALPHA, x["M"].shape, **kw)
    return step, stats


def _demons(update):
    mode = 0 if update == "additive" else 1

    def call(h, x, kw):
        u = x["field"].clone()
        return u, h.demons(x["F"], x["M"], u, 2, ALPHA, SIGMA_FLUID, SIGMA_DIFFUSION, update=update,
                           squarings=SQUARINGS, **kw)

    def size(h, x, masked):                                # with a mask the call is the pyramid driver's, one level
        L = h.lib()
        return 4 * (L.sift3d_amd_demons_multires_work_floats(*_g(x["F"]), 1, mode, 1) if masked else
                    L.sift3d_amd_demons_work_floats_ex(*_g(x["F"]), 1, mode))
    return Row(call, size, _pair_masks)


def _iterations(x):
    return [2] + [1] * (len(x["Fs"]) - 1)


def _demons_multires(update):
    mode = 0 if update == "additive" else 1

    def call(h, x, kw):
        u = x["field"].clone()
        return u, h.demons_multires(x["Fs"], x["Ms"], u, _iterations(x), ALPHA, SIGMA_FLUID, SIGMA_DIFFUSION,
                                    update=update, squarings=SQUARINGS, **kw)
    return Row(call, lambda h, x, masked: 4 * h.lib().sift3d_amd_demons_multires_work_floats(
        *_g(x["Fs"][0]), x["Fs"][0].shape[0], mode, len(x["Fs"])), _level_masks(lambda x: len(x["Fs"])))


def _logdemons(symmetric):
    moving = "Fs2" if symmetric else "Ms"                  # the symmetric update needs one shape

    def call(h, x, kw):
        v = x["velocity"].clone()
        return v, h.logdemons(x["Fs"], x[moving], v, _iterations(x), ALPHA, SIGMA_FLUID, SIGMA_DIFFUSION,
                              symmetric=symmetric, bch=1, velocity_squarings=SQUARINGS, **kw)

    def masks(h, x):
        kw = _level_masks(lambda x: len(x["Fs"]))(h, x)
        if symmetric:
            kw["masks_moving"] = [x["WF2"]] + kw["masks_fixed"][1:]
        return kw
    return Row(call, lambda h, x, masked: 4 * h.lib().sift3d_amd_logdemons_work_floats(
        *_g(x["Fs"][0]), x["Fs"][0].shape[0], int(symmetric), len(x["Fs"])), masks)


def _field_compose(h, x, kw):
    out = _empty_like(x["field"])
    return out, h.field_compose(x["u"], x["field"], out, "compose", stats=True, **kw)


def _field_invert(h, x, kw):
    w = -x["field"]
    return w, h.field_invert(x["field"], w, 3, **kw)


def _lattice_dims(x):
    return tuple(x["lattice"].shape[1:])[::-1]


ROWS = {
    "bspline_prefilter": Row(lambda h, x, kw: h.bspline_prefilter(x["F"], **kw),
                             lambda h, x, masked: 4 * h.lib().sift3d_hip_bspline_work_floats(*_g(x["F"]))),
    "similarity_affine": _similarity(lambda x: x["A"]),
    "similarity_field": _similarity(lambda x: x["field"]),
    "similarity_none": _similarity(lambda x: None, "F2", lambda h, x: dict(mask_fixed=x["WF"], mask_moving=x["WF2"])),
    "distance_sq": _distance("sq"),
    "distance_root": _distance("root"),
    "distance_signed": _distance("signed"),
    # (the order of surface_collect's lists inside is not defined; the measures returned do not depend on it)
    "surface_distances": Row(lambda h, x, kw: h.surface_distances(x["LF"], x["LM"], LABELS, (1.0, 1.5, 2.0), **kw),
                             lambda h, x, masked: h.lib().sift3d_amd_surface_distances_work_bytes(*_g(x["LF"]))),
    "ffd_field": Row(lambda h, x, kw: h.ffd_field(x["lattice"], x["spacing"], _empty_like(x["F"], 3), x["A"], **kw),
                     lambda h, x, masked: h.lib().sift3d_amd_ffd_field_work_bytes(*x["spacing"])),
    "ffd_bending": Row(lambda h, x, kw: h.ffd_bending(x["lattice"], x["spacing"], **kw),
                       lambda h, x, masked: h.lib().sift3d_amd_ffd_bending_work_bytes(*_lattice_dims(x))),
    "jacobian_penalty": Row(lambda h, x, kw: h.jacobian_penalty(x["field"], 1.0, False, **kw),
                            lambda h, x, masked: h.lib().sift3d_amd_jacobian_penalty_work_bytes(*_g(x["field"]))),
    "jacobian_penalty_gradient":
        Row(lambda h, x, kw: h.jacobian_penalty(x["field"], 1.0, True, **kw),
            lambda h, x, masked: h.lib().sift3d_amd_jacobian_penalty_work_bytes(*_g(x["field"]))),
    "ffd_jacobian_gradient":
        Row(lambda h, x, kw: h.ffd_jacobian_gradient(x["field"], x["spacing"], 1.0, **kw),
            lambda h, x, masked: h.lib().sift3d_amd_ffd_jacobian_gradient_work_bytes(*_g(x["field"]), *x["spacing"])),
    "ffd_landmarks": Row(lambda h, x, kw: h.ffd_landmarks(x["lattice"], x["spacing"], x["P"], x["Q"], x["w"], x["A"],
                                                          **kw),
                         lambda h, x, masked: h.lib().sift3d_amd_ffd_landmarks_work_bytes(len(x["P"]),
                                                                                          *_lattice_dims(x))),
    "dense_descriptors": Row(lambda h, x, kw: h.dense_descriptors(x["F"], _empty_like(x["F"], 12), SIGMA, **kw),
                             lambda h, x, masked: 4 * h.lib().sift3d_amd_dense_work_floats(*_g(x["F"])),
                             dtype="float32"),
    "dense_descriptors_rotate":
        Row(lambda h, x, kw: h.dense_descriptors_rotate(x["F"], _empty_like(x["F"], 12), SIGMA, **kw),
            lambda h, x, masked: 4 * h.lib().sift3d_amd_dense_rotate_work_floats(*_g(x["F"])), dtype="float32"),
    "demons_force": Row(_demons_force, lambda h, x, masked: h.DEMONS_FORCE_WORK_BYTES, _pair_masks),
    "demons_additive": _demons("additive"),
    "demons_diffeomorphic": _demons("diffeomorphic"),
    "field_compose": Row(_field_compose, lambda h, x, masked: h.FIELD_WORK_BYTES),
    "field_exp": Row(lambda h, x, kw: h.field_exp(x["velocity"], _empty_like(x["velocity"]), SQUARINGS, **kw),
                     lambda h, x, masked: 4 * h.lib().sift3d_amd_field_exp_work_floats(*_g(x["velocity"]))),
    "field_invert": Row(_field_invert,
                        lambda h, x, masked: 4 * h.lib().sift3d_amd_field_invert_work_floats(*_g(x["field"]))),
    "demons_multires_additive": _demons_multires("additive"),
    "demons_multires_diffeomorphic": _demons_multires("diffeomorphic"),
    "logdemons": _logdemons(False),
    "logdemons_symmetric": _logdemons(True),
}


# ---- the entries that take no work buffer and had no stream test -----------------------------------------------------
def _surface_collect(h, x, kw):
    import torch
    out = torch.full((x["surface"].numel(),), -1.0, dtype=torch.float32, device="cuda")
    out, count = h.surface_collect(x["surface"], x["d2"], out)
    return torch.sort(out).values, count                   # the list's order is not defined: as a sorted multiset


def _api(name):
    def call(h, x, kw):
        from sift3d_amd import api
        if name == "ffd_transform_points":
            return api.ffd_transform_points(x["lattice"], x["spacing"], x["P"], x["A"])
        return tuple(api.label_overlap(x["LF"], x["LM"], x["A"], N_LABELS))
    return call


STREAM_ONLY = {
    "bspline_warp_affine": lambda h, x, kw: h.bspline_warp_affine(x["M"], _empty_like(x["F"]), x["A"]),
    "bspline_warp_field": lambda h, x, kw: h.bspline_warp_field(x["M"], _empty_like(x["F"]), x["field"]),
    "restrict2": lambda h, x, kw: h.restrict2(x["F"]),
    "field_prolong2": lambda h, x, kw: h.field_prolong2(x["field_half"], _empty_like(x["field"])),
    "ffd_transform_points": _api("ffd_transform_points"),
    "label_surface": lambda h, x, kw: h.label_surface(x["LF"], LABELS[0]),
    "surface_collect": _surface_collect,
    "label_overlap": _api("label_overlap"),
}

SCRATCH = [n for n in rw.NAMES if n not in rw.NO_WORK] + sorted(ROWS)       # part A: the entries that take work=
ENTRIES = rw.NAMES + sorted(ROWS) + sorted(STREAM_ONLY)                     # part B
assert len(set(ENTRIES)) == len(ENTRIES)


def takes_masks(name):
    return name in rw.CALLS or ROWS[name].masks is not None


def call(h, name, x, masked=False, **kw):
    """the entry `name` of either table (or of STREAM_ONLY) on the inputs x, with both masks of x where masked"""
    if name in rw.CALLS:
        if masked:
            kw.update(rw.mask_kw(h, name, x["WF"], x["WM"], x["set"].levels))
        return rw.CALLS[name](h, x, kw)
    if name in STREAM_ONLY:
        return STREAM_ONLY[name](h, x, kw)
    if masked:
        kw.update(ROWS[name].masks(h, x))
    return ROWS[name].call(h, x, kw)


def need_bytes(h, name, x, masked):
    """the library's own size of the work buffer of call(h, name, x, masked)"""
    if name in rw.CALLS:
        return rw.work_bytes(h, name, len(x["P"]), masked, x["set"])
    return ROWS[name].size(h, x, masked)


def inputs(h, s):
    """rw.inputs(h, s), and what the second table and STREAM_ONLY take beside it; no call writes any of it"""
    import torch
    x = rw.inputs(h, s)
    rng = np.random.default_rng(29)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    x["WF"], x["WM"] = rw.some_masks(s)
    x["WF2"] = dev(rng.random(s.fshape) < 0.8)
    x["F2"] = dev(rng.random(s.fshape))
    x["Fs2"] = [dev(rng.random((s.channels,) + g)) for g in rw.pyramid(h, s.fshape, s.levels)]
    x["u"] = dev((rng.random((3,) + tuple(s.mshape)) - 0.5) * 0.6)
    x["velocity"] = x["field"] * 0.5
    x["field_half"] = h.restrict2(x["field"], scale=0.5)
    x["mask"] = dev(rng.random(s.fshape) < 0.3)
    x["LF"], x["LM"] = (dev(rng.integers(0, N_LABELS, s.fshape)) for _ in range(2))
    x["surface"], _ = h.label_surface(x["LF"], LABELS[0])
    x["d2"] = h.distance((x["LM"] == LABELS[0]).float(), mode="sq")
    torch.cuda.synchronize()
    return x


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


@pytest.fixture(scope="module")
def data(hip):
    made = {}

    def get(which):
        if which not in made:
            made[which] = inputs(hip, SETS[which])
        return made[which]
    return get


@pytest.fixture(scope="module")
def delay():
    """about 2 ms of queued work per 20 in-place multiplies"""
    import torch
    return torch.ones((256, 512, 512), device="cuda")


def results(name, out):
    return rw.results(name, out) if name in rw.CALLS else rw.plain(out)


# ---- the sets --------------------------------------------------------------------------------------------------------
def test_p_is_a_padding_set(hip):
    """what makes P the padding set, asserted and not assumed (the docstring of this file on the lattices)"""
    fixed, moving = (rw.pyramid(hip, g, P.levels) for g in (P.fshape, P.mshape))
    for g in fixed + moving:
        assert int(np.prod(g)) % 4 != 0, g                  # pad4 of every level's volumes and masks adds something
    gz, gy, gx = hip.ffd_lattice_shape(P.fshape, P.spacing)[1:]
    assert (3 * gx * gy * gz * 4) % 16 != 0                 # pad16 of every lattice slot adds something
    assert TILE_X < P.fshape[2] <= 2 * TILE_X               # two tiles in x, the second one ragged
    assert int(np.prod(P.fshape)) <= 9 * 11 * 70


# ---- A: scratch ------------------------------------------------------------------------------------------------------
def guarded(need, fill, dtype):
    """(the work view of `need` bytes rounded up to 4, 16-byte aligned; the two bands round it), all filled with the
    byte `fill`: one uint8 tensor of G + need' + G bytes, G = max(MIN_BAND, need') rounded up to 16, so that a whole
    misplaced sub-buffer still lands inside a band"""
    import torch
    size = (need + 3) // 4 * 4
    G = (max(MIN_BAND, size) + 15) // 16 * 16
    whole = torch.full((G + size + G,), fill, dtype=torch.uint8, device="cuda")
    view = whole[G:G + size]
    assert view.data_ptr() % 16 == 0 and view.numel() == size
    return view.view(getattr(torch, dtype)), (whole[:G], whole[G + size:])


UNCHECKED = {"demons_force", "field_compose"}               # a constant size, which the wrapper does not look at

SCRATCH_CASES = [(n, s, m) for n in SCRATCH for s in sorted(SETS) for m in (False, True) if not m or takes_masks(n)]


@pytest.mark.parametrize("name,which,masked", SCRATCH_CASES,
                         ids=["%s-%s-%s" % (n, s, "masked" if m else "plain") for n, s, m in SCRATCH_CASES])
def test_work_of_the_librarys_size_guarded_and_poisoned(hip, data, name, which, masked):
    import torch
    x = data(which)
    need = need_bytes(hip, name, x, masked)
    assert need > 0
    want = results(name, call(hip, name, x, masked))
    dtype = "uint8" if name in rw.CALLS else ROWS[name].dtype
    if name not in UNCHECKED:                               # `need` is the wrapper's own figure
        with pytest.raises(ValueError):
            call(hip, name, x, masked, work=guarded(need, 0, dtype)[0][:-1])
    for fill in (0xFF, 0x00):
        work, bands = guarded(need, fill, dtype)
        for run in ("first", "second"):                     # the second finds what the first left behind
            got = results(name, call(hip, name, x, masked, work=work))
            torch.cuda.synchronize()
            spilt = [int((b != fill).sum()) for b in bands]
            assert spilt == [0, 0], "%s call on work of 0x%02X, %d bytes: bytes written before, behind: %s" % (
                run, fill, need, spilt)
            same = got == want
            assert same, "%s call on work of 0x%02X differs from work=None" % (run, fill)


# ---- B: streams ------------------------------------------------------------------------------------------------------
def tree(v, f):
    """v with f applied to every tensor in its lists, tuples and dicts"""
    import torch
    if isinstance(v, torch.Tensor):
        return f(v)
    if isinstance(v, dict):
        return {k: tree(e, f) for k, e in v.items()}
    if type(v) in (list, tuple):
        return type(v)(tree(e, f) for e in v)
    return v


def tensors(v):
    import torch
    if isinstance(v, torch.Tensor):
        yield v
    elif isinstance(v, dict):
        for k in v:
            yield from tensors(v[k])
    elif type(v) in (list, tuple):
        for e in v:
            yield from tensors(e)


@pytest.mark.parametrize("name", ENTRIES)
def test_entry_is_ordered_on_the_callers_stream(hip, data, delay, name):
    import torch
    x = data("S")
    hip.current_stream(refresh=True)
    want = results(name, call(hip, name, x))
    twins = tree(x, torch.zeros_like)
    # the premise: on the zeros, which is what any other stream would read, the entry gives something else
    differs = results(name, call(hip, name, twins)) != want
    assert differs, "all-zero inputs give the same bytes: a launch on another stream would not show"
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    try:
        with torch.cuda.stream(s):
            hip.current_stream(refresh=True)
            for _ in range(20):
                delay.mul_(1.0001)
            for twin, real in zip(tensors(twins), tensors(x)):
                twin.copy_(real)
            got = tree(call(hip, name, twins), lambda t: t.clone())
        hip.current_stream(refresh=True)
        torch.cuda.current_stream().wait_stream(s)
        same = results(name, got) == want
        assert same, "on a stream of its own behind a delayed producer the entry gives other bytes"
    finally:
        hip.current_stream(refresh=True)
