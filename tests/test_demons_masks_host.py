"""CPU (not gpu): the host side of masks in demons (include/sift3d_amd.h, "Masks in demons") -- the exported symbols;
the refusals of sift3d_hip_demons_force_masked, sift3d_amd_demons_masked_device and sift3d_amd_logdemons_masked_device
on made-up pointers (they check their arguments before any device call); the Python refusals; and the numpy
restatement (tests/demons_mask_restatement.py) against the unmasked one."""
import numpy as np
import pytest

from tests import demons_mask_restatement as dk
from tests import demons_restatement as dm
from tests import logdemons_restatement as lg
from tests import multires_restatement as mr

F32 = np.float32


@pytest.fixture(scope="module")
def api():
    from sift3d_amd import api as a
    a.lib()
    return a


@pytest.fixture(scope="module")
def bufs(api):
    """made-up addresses without a device; real allocations covering every range named below with one, so that a
    regressed check could not make a kernel touch unmapped memory"""
    from sift3d_amd import hip
    if api.device_available():
        b = [hip.lib().sift3d_hip_malloc(1 << 18) for _ in range(3)]
        assert all(b)
        yield b
        for p in b:
            hip.lib().sift3d_hip_free(p)
    else:
        yield [0x1000000, 0x2000000, 0x3000000]


EXPORTED = ["sift3d_hip_demons_force_masked", "sift3d_amd_demons_masked_device", "sift3d_amd_logdemons_masked_device"]


def test_symbols_exported(api):
    import inspect
    from sift3d_amd import _native, hip
    L = _native.load()
    for name in EXPORTED:
        assert hasattr(L, name), name
    hip.lib()
    assert [f[0] for f in hip.DemonsLevelMasks._fields_] == ["d_WF", "d_WM"]
    for fn, names in ((hip.demons_force, ("mask_fixed", "mask_moving")), (hip.demons, ("mask_fixed", "mask_moving")),
                      (hip.demons_multires, ("masks_fixed", "masks_moving")),
                      (hip.logdemons, ("masks_fixed", "masks_moving")),
                      (api.refine_field, ("mask_fixed", "mask_moving")),
                      (api.register_dense, ("mask_fixed", "mask_moving"))):
        par = inspect.signature(fn).parameters
        for n in names:
            assert n in par and par[n].default is None, (fn.__name__, n)


# ---- the C entries' refusals -----------------------------------------------------------------------------------------
VB = 512 * 4                                                # an 8^3 volume: 2048 bytes


def _force(L, a):
    return L.sift3d_hip_demons_force_masked(a["F"], a["nx"], a["ny"], a["nz"], a["W"], a["u"], a["mx"], a["my"],
                                            a["mz"], a["nc"], a["alpha"], a["step"], a["stats"], a["work"], None,
                                            a["WF"], a["WM"])


def test_force_masked_refusals(bufs):
    """F, W, u and the two masks in buffer 0, step and stats in 1, the partials in 2 (8^3, nc = 1)"""
    from sift3d_amd import hip
    L = hip.lib()
    A, B, W = bufs
    base = dict(F=A, nx=8, ny=8, nz=8, W=A + 8192, u=A + 16384, mx=8, my=8, mz=8, nc=1, alpha=1.0, step=B,
                stats=B + 8192, work=W, WF=A + 32768, WM=A + 40960)
    changes = [
        # the unmasked entry's refusals still hold with masks given
        dict(F=None), dict(step=None), dict(nx=0), dict(mz=0), dict(nc=0), dict(alpha=0.0), dict(stats=B + 8196),
        dict(F=A + 2), dict(step=A + 4 * 100), dict(work=B + 4 * 1000),
        # misaligned masks
        dict(WF=A + 32770), dict(WM=A + 40961), dict(WF=None, WM=A + 40962), dict(WF=A + 32769, WM=None),
        # a mask over an output or the partials
        dict(WF=B), dict(WF=B + 4 * 1535), dict(WM=B + 4 * 1000), dict(WM=B - VB + 4),          # d_step
        dict(WF=B + 8192), dict(WM=B + 8192 - VB + 8),                                          # d_stats
        dict(WF=W), dict(WM=W + 32768 - 4), dict(WF=None, WM=W + 4 * 100),                      # d_work
        dict(mx=16, my=16, mz=16, step=B + 16380, stats=B + 65536, WM=B),        # the moving mask has ITS grid's size
    ]
    for ch in changes:
        a = dict(base)
        a.update(ch)
        assert _force(L, a) == -1, ch
    # a mask may share memory with another input (it is only read): no refusal is defined for it, and with a NULL
    # stream and made-up pointers nothing may be launched here, so only the outputs are probed above


def _levels(hip, *rows):
    tab = (hip.DemonsLevel * len(rows))()
    for l, r in enumerate(rows):
        tab[l] = hip.DemonsLevel(*r)
    return tab


def _masks(hip, *rows):
    tab = (hip.DemonsLevelMasks * len(rows))()
    for l, r in enumerate(rows):
        tab[l] = hip.DemonsLevelMasks(*r)
    return tab


def _drv(L, a):
    return L.sift3d_amd_demons_masked_device(a["tab"], a["masks"], a["levels"], a["nc"], a["u"], a["alpha"], a["sf"],
                                             a["sd"], a["update"], a["K"], a["work"], a["stats"], None)


def _log(L, a):
    return L.sift3d_amd_logdemons_masked_device(a["tab"], a["masks"], a["levels"], a["nc"], a["u"], a["alpha"], a["sf"],
                                                a["sd"], a["sym"], a["bch"], a["K"], a["work"], a["stats"], None)


@pytest.mark.parametrize("entry", ["additive", "diffeomorphic", "logdomain", "symmetric"])
def test_driver_masked_refusals(bufs, entry):
    """F, M and the masks in buffer 0, u / v and the statistics in 1, the work buffer in 2 (8^3, nc = 1)"""
    from sift3d_amd import hip
    L = hip.lib()
    A, B, W = bufs
    M, WF, WM = A + 8192, A + 32768, A + 40960
    log = entry in ("logdomain", "symmetric")
    if log:
        floats = L.sift3d_amd_logdemons_work_floats(8, 8, 8, 1, int(entry == "symmetric"), 1)
        run = _log
    else:
        floats = L.sift3d_amd_demons_multires_work_floats(8, 8, 8, 1, int(entry == "diffeomorphic"), 1)
        run = _drv
    assert floats > 0

    def lv(**ch):
        r = dict(F=A, nx=8, ny=8, nz=8, M=M, mx=8, my=8, mz=8, it=3)
        r.update(ch)
        return _levels(hip, (r["F"], r["nx"], r["ny"], r["nz"], r["M"], r["mx"], r["my"], r["mz"], r["it"]))

    base = dict(tab=lv(), masks=_masks(hip, (WF, WM)), levels=1, nc=1, u=B, alpha=1.0, sf=1.0, sd=1.0,
                update=int(entry == "diffeomorphic"), K=2, sym=int(entry == "symmetric"), bch=1, work=W,
                stats=B + 8192)
    two = _levels(hip, (A, 8, 8, 8, M, 8, 8, 8, 1), (A, 5, 4, 4, M, 4, 4, 4, 1))
    changes = [
        # the unmasked entries' refusals, with masks and with a NULL mask table
        dict(tab=None), dict(u=None), dict(work=None), dict(stats=None), dict(levels=0), dict(levels=7),
        dict(tab=lv(F=None)), dict(tab=lv(nx=0)), dict(tab=lv(it=-1)), dict(nc=0), dict(alpha=0.0),
        dict(sf=-0.1), dict(sd=float("inf")), dict(K=-1), dict(K=21), dict(u=B + 2), dict(u=A + 4 * 300),
        dict(work=B), dict(stats=B + 4 * 1000),
        dict(masks=None, tab=None), dict(masks=None, u=A + 4 * 300), dict(masks=None, levels=7),
        # a bad level table: two levels whose second is not the half of the first
        dict(levels=2, tab=two, masks=_masks(hip, (WF, WM), (None, None))), dict(levels=2, tab=two, masks=None),
        # misaligned masks
        dict(masks=_masks(hip, (WF + 2, WM))), dict(masks=_masks(hip, (WF, WM + 1))),
        dict(masks=_masks(hip, (None, WM + 3))), dict(masks=_masks(hip, (WF + 1, None))),
        # a mask over d_u / d_v, d_stats or d_work
        dict(masks=_masks(hip, (B, WM))), dict(masks=_masks(hip, (WF, B + 4 * 1535))),
        dict(masks=_masks(hip, (B - VB + 4, None))),
        dict(masks=_masks(hip, (B + 8192, WM))), dict(masks=_masks(hip, (WF, B + 8192 + 16 * 3 - 4))),
        dict(masks=_masks(hip, (W, WM))), dict(masks=_masks(hip, (None, W + 4 * floats - 4))),
        dict(masks=_masks(hip, (W + 4 * 9000, None))),
    ]
    if not log:
        changes += [dict(update=2), dict(update=-1)]
    else:
        changes += [dict(bch=2), dict(sym=2)]
    if entry == "symmetric":
        changes += [dict(tab=lv(mx=7))]
    for ch in changes:
        a = dict(base)
        a.update(ch)
        assert run(L, a) == -1, ch
    # a second level's mask over the field is refused too (a well-formed two-level table)
    ok2 = _levels(hip, (A, 8, 8, 8, M, 8, 8, 8, 1), (A, 4, 4, 4, M, 4, 4, 4, 1))
    floats2 = (L.sift3d_amd_logdemons_work_floats(8, 8, 8, 1, base["sym"], 2) if log else
               L.sift3d_amd_demons_multires_work_floats(8, 8, 8, 1, base["update"], 2))
    for m in (_masks(hip, (WF, WM), (B + 4 * 100, None)), _masks(hip, (None, None), (None, W + 4 * floats2 - 4)),
              _masks(hip, (None, None), (WF + 2, None))):
        a = dict(base)
        a.update(levels=2, tab=ok2, masks=m)
        assert run(L, a) == -1


# ---- the Python refusals ---------------------------------------------------------------------------------------------
def test_python_refusals(api):
    from sift3d_amd import hip
    vol = np.zeros((5, 6, 7), F32)
    fld = np.zeros((3, 5, 6, 7), F32)
    for upd in ("additive", "diffeomorphic", "logdomain", "symmetric"):
        with pytest.raises(ValueError, match="mask_fixed must have its volume's shape"):
            api.refine_field(vol, vol, update=upd, mask_fixed=np.ones((5, 6, 8), bool))
        with pytest.raises(ValueError, match="mask_moving must have its volume's shape"):
            api.refine_field(vol, vol, update=upd, mask_moving=np.ones((4, 6, 7), F32))
    with pytest.raises(ValueError, match="bool, integer or float"):
        api.refine_field(vol, vol, mask_fixed=np.ones((5, 6, 7), np.complex64))
    with pytest.raises(ValueError, match="per level"):
        hip.demons_multires([vol], [vol], fld, [1], 1.0, masks_fixed=[None, None])
    with pytest.raises(ValueError, match="per level"):
        hip.demons_multires([vol, vol], [vol, vol], fld, [1, 1], 1.0, masks_moving=[None])
    with pytest.raises(ValueError, match="per level"):
        hip.logdemons([vol], [vol], fld, [1], 1.0, masks_moving=[])
    with pytest.raises(ValueError, match="per level"):
        hip.logdemons([vol], [vol], fld, [1], 1.0, masks_fixed=[None] * 3)


# ---- the restatement against the unmasked one ------------------------------------------------------------------------
def _bits(got, want, what):
    got = np.ascontiguousarray(got, F32)
    want = np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%s: %d of %d values differ" % (what, int(bad.sum()), bad.size)


def _case(nc, seed, shape=(7, 6, 9), mshape=(6, 8, 7)):
    rng = np.random.default_rng(seed)
    F = rng.normal(0, 1, (nc,) + shape).astype(F32)
    M = rng.normal(0, 1, (nc,) + mshape).astype(F32)
    W = (F + rng.normal(0, 0.5, F.shape)).astype(F32)
    u = rng.normal(0, 1.5, (3,) + shape).astype(F32)
    return F, M, W, u


@pytest.mark.parametrize("nc", [1, 12])
def test_restated_all_ones_masks_are_the_unmasked_force(nc):
    F, M, W, u = _case(nc, nc)
    mshape = M.shape[1:]
    want, sd, ins = dm.ref_force(F, W, u, mshape, 0.8)
    assert 0 < ins.sum() < ins.size
    for WF, WM in ((None, None), (np.ones(F.shape[1:], F32), None), (None, np.ones(mshape, F32)),
                   (np.ones(F.shape[1:], F32), np.full(mshape, 0.5, F32))):
        got, gsd, gins = dk.ref_force(F, W, u, mshape, 0.8, WF, WM)
        _bits(got, want, "all-in masks")
        assert np.array_equal(gins, ins)
        assert np.array_equal(gsd.view(np.uint64), sd.view(np.uint64))
        assert dm.ref_stats(gsd, gins) == dm.ref_stats(sd, ins)


def test_restated_all_ones_masks_are_the_unmasked_drivers(oracle_mod):
    F, M, _, u = _case(2, 5)
    ones = (np.ones(F.shape[1:], F32), np.ones(M.shape[1:], F32))
    args = (3, 0.8, 1.0, 1.5, oracle_mod)
    _bits(dk.ref_demons(F, M, u, *args, *ones)[0], dm.ref_demons(F, M, u, *args)[0], "additive")
    from tests import field_algebra_restatement as fa
    _bits(dk.ref_demons(F, M, u, *args, *ones, update="diffeomorphic", squarings=1)[0],
          fa.ref_demons_diffeo(F, M, u, 3, 0.8, 1.0, 1.5, 1, oracle_mod)[0], "diffeomorphic")
    _bits(dk.ref_logdemons(F, M, u, *args, *ones, bch=1, squarings=1)[0],
          lg.ref_logdemons(F, M, u, *args, bch=1, squarings=1)[0], "logdomain")
    M2 = (F + F32(0.25) * M[:, :1, :1, :1]).astype(F32)
    ones2 = (ones[0], ones[0])
    _bits(dk.ref_logdemons(F, M2, u, *args, *ones2, symmetric=True, squarings=1)[0],
          lg.ref_logdemons(F, M2, u, *args, symmetric=True, squarings=1)[0], "symmetric")
    Fs, Ms = mr.ref_pyramid(F, 2), mr.ref_pyramid(M, 2)
    _bits(dk.ref_multires(Fs, Ms, u, [2, 1], 0.8, 1.0, 1.5, oracle_mod, dk.mask_pyramid(ones[0], 2),
                          dk.mask_pyramid(ones[1], 2))[0],
          mr.ref_multires(Fs, Ms, u, [2, 1], 0.8, 1.0, 1.5, oracle_mod)[0], "two levels")


def test_restated_fixed_mask_all_out_gives_positive_zero():
    F, M, W, u = _case(3, 9)
    for WF in (np.zeros(F.shape[1:], F32), np.full(F.shape[1:], np.nan, F32), np.full(F.shape[1:], -1.0, F32),
               np.full(F.shape[1:], np.nextafter(F32(0.5), F32(0)), F32)):
        delta, sd, ins = dk.ref_force(F, W, u, M.shape[1:], 0.8, WF, None)
        assert not delta.view(np.uint32).any()                     # +0.0f, the sign bit clear
        assert not ins.any() and dm.ref_stats(sd, ins) == (0.0, 0)
    # and the moving mask all out
    delta, sd, ins = dk.ref_force(F, W, u, M.shape[1:], 0.8, None, np.zeros(M.shape[1:], F32))
    assert not delta.view(np.uint32).any() and dm.ref_stats(sd, ins) == (0.0, 0)


def test_restated_moving_mask_is_read_at_the_nearest_voxel():
    """u = 0.5 exactly: q is a half-integer and the mask voxel is the upper one (floor(q + 0.5)); q on the upper face
    m - 1 reads voxel m - 1"""
    shape = (3, 4, 6)
    u = np.zeros((3,) + shape, F32)
    u[0] = F32(0.5)
    WM = np.zeros(shape, F32)
    WM[:, :, 3] = 1.0
    ins = dk.counted(u, shape, None, WM)
    assert ins[:, :, 2].all() and not ins[:, :, 3].any() and ins.sum() == 12      # x = 2 reads voxel 3
    u[0] = 0.0
    u[0][:, :, 4] = 1.0                                                            # q = 5 = mx - 1 exactly
    WM[:] = 0.0
    WM[:, :, 5] = 1.0
    ins = dk.counted(u, shape, None, WM)
    assert ins[:, :, 4].all() and ins[:, :, 5].all() and ins.sum() == 24
