"""The pyramid kernels on subnormal, zero-background and extreme content (-m gpu), bit for bit.

Every other kernel-level test of this stage feeds it standard_normal noise of order 1, which cannot show a kernel
that flushes subnormals, a division that is not IEEE on denormal or huge operands, or a zone of an elementwise loop
that no test is large enough to reach.  The content classes, the table of FIR cases (one group per kernel path,
each with the launch condition that selects it) and the sizes are in tests/pyramid_content.py;
tests/test_pyramid_content_host.py proves on the CPU that the cases can fail (at least half of the reference
output words of the underflow classes are subnormals, and a flush changes at least half of them; measured there
over all FIR cases: `subnormal` 0.98 and 0.98 at the least, `fade` 0.81 and 0.92, `faint_spikes` 0.93 and 1.00 of its
nonzero words).

FIR: the reference is oracle_mod.fir_axis (mode 0), one axis after the other for the fused kernels; the entries
that divide by max|v| get the oracle's input from numpy's float32 division, which shares no code with the kernels.
The comparison is on the uint32 words, so that -0.0 and +0.0 are told apart; source and destination lie between
NaN guard bands, and the source must come back unchanged.

Elementwise kernels: absmax at every zone of its loop (the sizes are derived from grid_reduce in
pyramid_content.py), from views that start 0 .. 3 floats into an allocation; scale, subtract_absmax and the DoG
stacks on subnormal quotients and differences; downsample2 by both of its kernels on content in which every voxel
encodes its own index.
"""
import numpy as np
import pytest

from tests import pyramid_content as pc

pytestmark = pytest.mark.gpu
F = np.float32
GUARD = 4096


@pytest.fixture(scope="module")
def gpu():
    import torch
    from sift3d_amd import api, hip
    if not torch.cuda.is_available() or not api.device_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    hip.lib()
    return api, hip, torch


def _guarded(torch, shape, fill=None, off=0):
    """A tensor of `shape` between two NaN guard bands, starting `off` floats behind a 16-byte boundary; itself
    NaN or a copy of `fill`.  Returns (whole buffer, view)."""
    n = int(np.prod(shape))
    big = torch.full((n + 2 * GUARD + 4,), float("nan"), device="cuda")
    assert big.data_ptr() % 16 == 0
    view = big[GUARD + off:GUARD + off + n].view(shape)
    if fill is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(fill, F).reshape(shape)))
    return big, view


def _intact(torch, big, shape, off=0):
    n = int(np.prod(shape))
    return bool(torch.isnan(big[:GUARD + off]).all()) and bool(torch.isnan(big[GUARD + off + n:]).all())


def _bits(t):
    return pc.bits(t.cpu().numpy())


def _scalar(torch, value):
    return torch.from_numpy(np.asarray(value, F).reshape(1)).cuda()


def _takes_dma(shape):
    """launch_fir_yz's condition for k_fir_yz_dma (its z segments hold at most DMA_MAX_TS planes for nz <= 70)."""
    nz, ny, nx = shape
    return nx % 64 == 0 and ny % 64 == 0 and ny >= 128


# ----------------------------------------------------------------------------------------------------------------
# every FIR path x every class
# ----------------------------------------------------------------------------------------------------------------
def _launch(gpu, case, vol, taps, mx):
    """The case's entry on `vol` between guard bands; returns the destination as an array."""
    api, hip, torch = gpu
    sbig, src = _guarded(torch, vol.shape, vol)
    dbig, dst = _guarded(torch, vol.shape)
    smax = None if mx is None else _scalar(torch, mx)
    if case.entry in ("fir", "fir_v1"):
        (axis,) = case.axes
        hip.fir(src, dst, axis, taps, unit_factor=case.uf, variant=1 if case.entry == "fir_v1" else 0)
    elif case.entry == "x_scaled":
        assert hip.fir_x_scaled(src, dst, taps, smax) is True
    elif case.entry == "yz":
        assert _takes_dma(vol.shape) == (case.path == "9_yz_dma")
        assert hip.fir_yz(src, dst, taps) is True
    else:
        assert hip.fir_xyz(src, dst, taps, smax) is True
    torch.cuda.synchronize()
    assert _intact(torch, sbig, vol.shape) and _intact(torch, dbig, vol.shape), case.id
    assert np.array_equal(_bits(src), pc.bits(vol)), "%s: the source changed" % case.id
    if smax is not None:
        assert np.array_equal(_bits(smax), pc.bits(mx).reshape(1))
    return dst.cpu().numpy()


@pytest.mark.parametrize("case", pc.FIR_CASES, ids=lambda c: c.id)
def test_fir_path_on_every_class_vs_oracle(gpu, oracle_mod, case):
    taps = pc.taps(case.taps, gpu[0].gauss_filter)
    wrong = []
    for cls in case.classes():
        vol = pc.content(case, cls)
        ref_in, mx = vol, None
        if case.scaled:
            ref_in, mx = pc.scaled_input(vol)          # (asserts that the maximum is neither 0.0 nor 1.0)
        want = pc.oracle_fir(oracle_mod, ref_in, taps, case.axes, case.uf)
        got = _launch(gpu, case, vol, taps, mx)
        bad = pc.bits(got) != pc.bits(want)
        if bad.any():
            i = tuple(int(v[0]) for v in np.nonzero(bad))
            wrong.append("%s: %d of %d words differ, first at %r: got %r (0x%08x), want %r (0x%08x)"
                         % (cls, int(bad.sum()), bad.size, i, got[i], pc.bits(got)[i], want[i], pc.bits(want)[i]))
    assert not wrong, "%s\n  %s" % (case.id, "\n  ".join(wrong))


# ----------------------------------------------------------------------------------------------------------------
# absmax
# ----------------------------------------------------------------------------------------------------------------
def _absmax(gpu, view):
    api, hip, torch = gpu
    obig, out = _guarded(torch, (1,), np.zeros(1, F))
    hip.absmax(view, out)
    torch.cuda.synchronize()
    assert _intact(torch, obig, (1,))
    return _bits(out)[0]


@pytest.mark.parametrize("n", pc.ABSMAX_SIZES)
def test_absmax_every_zone_and_alignment(gpu, n):
    """One maximum among smaller integers, placed in turn at the first and the last element of every zone of
    k_absmax's loop that the size has (pyramid_content.absmax_zones), negative at one end and positive at the other;
    from views that start 0, 1, 2 and 3 floats behind a 16-byte boundary."""
    api, hip, torch = gpu
    bg = np.clip(pc.integer((n,), n % 1000), -400, 400)
    zones = pc.absmax_zones(n)
    assert zones
    top = F(7777.0)
    for off in range(4):
        big, view = _guarded(torch, (n,), bg, off)
        assert view.data_ptr() % 16 == 4 * off
        assert _absmax(gpu, view) == pc.bits(np.abs(bg).max())
        for zone, (first, last) in zones.items():
            for idx, val in ((first, -top), (last, top)):
                keep = float(bg[idx])
                view[idx] = float(val)
                got = _absmax(gpu, view)
                view[idx] = keep
                assert got == pc.bits(top), "n %d, offset %d, %s zone, element %d" % (n, off, zone, idx)
        assert _intact(torch, big, (n,), off)
        assert np.array_equal(_bits(view), pc.bits(bg))


@pytest.mark.parametrize("n", [5, 1023, 1024 * 1024 + 3])
def test_absmax_subnormal_maximum_and_signed_zeros(gpu, n):
    api, hip, torch = gpu
    zeros = np.zeros(n, F)
    zeros[1::2] = F(-0.0)
    for off in (0, 1):
        # every value -0.0 (or +-0.0): the result is +0.0, bit for bit
        for v in (np.full(n, F(-0.0), F), zeros):
            big, view = _guarded(torch, (n,), v, off)
            assert _absmax(gpu, view) == 0
        # a subnormal maximum beside +-0.0, in the quad zone and in the tail, negative and positive
        for idx, val in ((0, F(-5e-45)), (n - 1, F(7e-42)), (n // 2, F(-1e-39))):
            v = zeros.copy()
            v[idx] = val
            assert pc.is_subnormal(val)
            big, view = _guarded(torch, (n,), v, off)
            want = pc.bits(np.abs(v).max())
            assert want == pc.bits(np.abs(val)) and _absmax(gpu, view) == want, (n, off, idx)


# ----------------------------------------------------------------------------------------------------------------
# scale, subtract_absmax
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", pc.SCALED_CLASSES)
def test_scale_vs_ieee_division(gpu, cls):
    """hip.scale (k_scale's `v / max`) against numpy's float32 division: a subnormal numerator and denominator
    (`subnormal`: the maximum is about 2.8e-42), a subnormal numerator alone (`fade`), 2**100 (`huge`).  n is not
    a multiple of 4; source and destination start 0 .. 3 floats behind a 16-byte boundary."""
    api, hip, torch = gpu
    shape = (17, 21, 23)
    assert int(np.prod(shape)) % 4 == 3
    vol = pc.CLASSES[cls](shape, 41)
    want, mx = pc.scaled_input(vol)
    if cls == "subnormal":
        assert pc.is_subnormal(mx)
    for soff, doff in ((0, 0), (1, 1), (2, 3), (3, 0)):
        sbig, src = _guarded(torch, shape, vol, soff)
        dbig, dst = _guarded(torch, shape, None, doff)
        hip.scale(src, dst, _scalar(torch, mx))
        torch.cuda.synchronize()
        assert _intact(torch, sbig, shape, soff) and _intact(torch, dbig, shape, doff)
        assert np.array_equal(_bits(src), pc.bits(vol))
        bad = _bits(dst) != pc.bits(want)
        assert not bad.any(), "%s, offsets %d / %d: %d of %d quotients differ" % (cls, soff, doff, bad.sum(), bad.size)


@pytest.mark.parametrize("shape", [(17, 21, 23), (1, 1, pc.ABSMAX_SIZES[-1])],
                         ids=lambda s: "x".join(map(str, s)))
def test_subtract_absmax_exact_subnormal_differences(gpu, shape):
    """a from `fade`, b = a * float32(1 + 2**-20): a - b is exact and subnormal.  n % 4 == 3; the second size
    reaches the unrolled zone of k_sub_absmax's loop (the same three zones as k_absmax's)."""
    api, hip, torch = gpu
    n = int(np.prod(shape))
    assert n % 4 == 3
    a, b = pc.faded_levels(shape, 2, 17)
    want = a - b
    assert pc.is_subnormal(want).mean() > 0.5
    wmax = np.abs(want).max()
    assert pc.is_subnormal(wmax)
    for off in ((0, 1, 2, 3) if n < 10 ** 6 else (0, 1)):
        abig, da = _guarded(torch, shape, a, off)
        bbig, db = _guarded(torch, shape, b, (off + 1) % 4)
        dbig, dst = _guarded(torch, shape, None, (off + 2) % 4)
        mbig, dm = _guarded(torch, (1,), np.zeros(1, F))
        hip.subtract_absmax(da, db, dst, dm)
        torch.cuda.synchronize()
        assert _intact(torch, abig, shape, off) and _intact(torch, bbig, shape, (off + 1) % 4)
        assert _intact(torch, dbig, shape, (off + 2) % 4) and _intact(torch, mbig, (1,))
        bad = _bits(dst) != pc.bits(want)
        assert not bad.any(), "offset %d: %d of %d differences differ" % (off, bad.sum(), bad.size)
        assert _bits(dm)[0] == pc.bits(wmax), "offset %d" % off


# ----------------------------------------------------------------------------------------------------------------
# the DoG stacks
# ----------------------------------------------------------------------------------------------------------------
def _sub_lattice_max(a, b):
    """k_dogmax_sub's lattice: planes 1, 6, 11, ..., rows 0, 3, 6, ..., every x."""
    return np.abs(a[1::5, ::3] - b[1::5, ::3]).max()


@pytest.mark.parametrize("shape", [(18, 21, 37), (16, 16, 16)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("count", [2, 6])
def test_dog_stacks_on_subnormal_differences(gpu, shape, count):
    """hip.dog_stack, hip.dogmax_stack and (six levels) hip.dogmax_sub on levels whose differences are exact
    subnormals, the last pair identical (difference +0.0, maximum +0.0); 18 * 21 * 37 is no multiple of 4 (the
    scalar tail).  Entries that refuse ragged rows or unaligned levels must leave their outputs alone."""
    api, hip, torch = gpu
    lv = pc.faded_levels(shape, count, 23)
    want = [a - b for a, b in zip(lv, lv[1:])]
    want_max = np.array([np.abs(w).max() for w in want], F)
    assert pc.is_subnormal(want_max[0]) and (count < 3 or pc.bits(want_max[-1]) == 0)
    g = [_guarded(torch, shape, v) for v in lv]
    d = [_guarded(torch, shape) for _ in want]
    mbig, mm = _guarded(torch, (count - 1,), np.zeros(count - 1, F))
    m2big, mm2 = _guarded(torch, (count - 1,), np.zeros(count - 1, F))
    assert hip.dog_stack([v for _, v in g], [v for _, v in d], mm) is True
    assert hip.dogmax_stack([v for _, v in g], mm2) is True
    torch.cuda.synchronize()
    for k in range(count - 1):
        assert _intact(torch, d[k][0], shape) and _intact(torch, g[k][0], shape)
        assert np.array_equal(_bits(d[k][1]), pc.bits(want[k])), "difference %d" % k
    assert _intact(torch, mbig, (count - 1,)) and _intact(torch, m2big, (count - 1,))
    assert np.array_equal(_bits(mm), pc.bits(want_max)), "dog_stack maxima"
    assert np.array_equal(_bits(mm2), pc.bits(want_max)), "dogmax_stack maxima"
    if count == 6:
        nz, ny, nx = shape
        ebig, est = _guarded(torch, (5,), None if nx % 4 else np.zeros(5, F))
        rc = hip.dogmax_sub([v for _, v in g], nx, ny, nz, est)
        torch.cuda.synchronize()
        if nx % 4:
            # rows that are no whole quads: refused (sift3d_hip_dogmax_sub), nothing written
            assert rc == 1 and bool(torch.isnan(ebig).all())
        else:
            sub = np.array([_sub_lattice_max(a, b) for a, b in zip(lv, lv[1:])], F)
            assert rc == 0 and _intact(torch, ebig, (5,))
            assert pc.is_subnormal(sub[0]) and (sub <= want_max).all()
            assert np.array_equal(_bits(est), pc.bits(sub)), "dogmax_sub maxima"
    # levels that start one float behind a 16-byte boundary: all three entries refuse, and write nothing
    g1 = [_guarded(torch, shape, v, 1) for v in lv]
    d1 = [_guarded(torch, shape) for _ in want]
    nbig, nan_max = _guarded(torch, (5,))
    assert hip.dog_stack([v for _, v in g1], [v for _, v in d1], nan_max) is False
    assert hip.dogmax_stack([v for _, v in g1], nan_max) is False
    # ... and so does dog_stack for aligned levels with an unaligned destination
    d2 = [_guarded(torch, shape, None, 1) for _ in want]
    assert hip.dog_stack([v for _, v in g], [v for _, v in d2], nan_max) is False
    if count == 6 and shape[2] % 4 == 0:
        assert hip.dogmax_sub([v for _, v in g1], shape[2], shape[1], shape[0], nan_max) == 1
    torch.cuda.synchronize()
    assert bool(torch.isnan(nbig).all())
    assert all(bool(torch.isnan(b).all()) for b, _ in d1 + d2)


# ----------------------------------------------------------------------------------------------------------------
# downsample2
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,off,kernel", [
    # sift3d_hip_downsample2 takes k_downsample2_q where mx % 4 == 0, nx % 4 == 0, nx >= 2 mx and both pointers
    # are 16-byte aligned, k_downsample2 otherwise
    ((6, 10, 520), 0, "q"),       # (3, 5, 260): 65 quads a row -- two workgroups along x --, my = 5 no multiple of 4
    ((5, 9, 16), 0, "q"),         # (2, 4, 8): odd source ny and nz
    ((6, 10, 522), 0, "scalar"),  # (3, 5, 261): mx % 4 != 0
    ((6, 10, 520), 1, "scalar"),  # the first shape from a source one float behind a 16-byte boundary
], ids=["520_quad", "16_quad_odd_rows", "522_scalar", "520_unaligned_scalar"])
def test_downsample2_both_kernels(gpu, oracle_mod, shape, off, kernel):
    """Integer content in which every voxel holds its own index (exact in float32: fewer than 2**24 voxels), so
    that a wrong gather shows; against oracle_mod.downsample, which equals vol[::2, ::2, ::2]."""
    api, hip, torch = gpu
    nz, ny, nx = shape
    n = nz * ny * nx
    assert n < 2 ** 24
    vol = np.arange(n, dtype=F).reshape(shape)
    want = oracle_mod.downsample(vol)
    np.testing.assert_array_equal(want, vol[:2 * (nz // 2):2, :2 * (ny // 2):2, :2 * (nx // 2):2])
    mshape = want.shape
    assert mshape == (nz // 2, ny // 2, nx // 2)
    sbig, src = _guarded(torch, shape, vol, off)
    dbig, dst = _guarded(torch, mshape)
    quad = mshape[2] % 4 == 0 and nx % 4 == 0 and nx >= 2 * mshape[2] and src.data_ptr() % 16 == 0 \
        and dst.data_ptr() % 16 == 0
    assert quad == (kernel == "q")
    hip.downsample2(src, dst)
    torch.cuda.synchronize()
    assert _intact(torch, sbig, shape, off) and _intact(torch, dbig, mshape)
    assert np.array_equal(_bits(src), pc.bits(vol))
    assert np.array_equal(_bits(dst), pc.bits(want))
