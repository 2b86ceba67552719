"""Hostile content for the pyramid stage: what tests/test_pyramid_content*.py and tests/test_detect_content*.py feed
the FIR, scale, absmax, DoG and downsample kernels instead of noise of order 1.  Seeded, numpy only, no device.

Content classes (CLASSES): a generator takes a shape (nz, ny, nx) and a seed and returns float32; `base` is
standard_normal.

  subnormal      base * 2**-140                          every sample and every sum subnormal
  fade           base * 2**-(110 + min(x + y + z, 30))   normal at the corner of the origin, subnormal from
                                                         x + y + z = 16 on: the lines through that corner cross
                                                         from normal to subnormal, their sums are mixed.  The
                                                         exponent stops at 140 (the `subnormal` class's), so that
                                                         a long row (512 voxels) does not run out into zeros
  faint_spikes   +0.0 / -0.0 background in alternate planes, about 1 % of the voxels +-2**-128 * uniform(0.5, 1):
                 every product tap * v is rounded in the subnormal range; signed zeros
  huge           base * 2**100                           large exponents; no sum overflows (asserted on the
                                                         oracle's output by the host test)
  integer        round(base * 100)                       exact arithmetic, many equal values
  constant       float32(0.1) everywhere                 a plateau: the sum of the taps in the reference's order

Non-finite samples are deliberately left out and nothing is pinned on them: the unit-spacing fast paths document
that tap * ((1 - frac) * lo + frac * hi) equals tap * lo "for finite data" only (sift3d_kernels.hip, the comment
above ext_sample), and the scaled path turns an infinite maximum into NaNs in the reference as well.

The module also holds what the GPU file and its CPU twin must agree on: the table of FIR cases (one group per
kernel path, with the launch condition that selects it), the sizes and zones of the absmax loop, the level pairs
with exact subnormal differences, and the end-to-end volumes.
"""
import numpy as np

F = np.float32
UNDERFLOW_CLASSES = ("subnormal", "fade", "faint_spikes")
TINY = np.finfo(np.float32).tiny          # 2**-126, the smallest normal float32


def _base(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(F)


def subnormal(shape, seed):
    return _base(shape, seed) * F(2.0 ** -140)


def fade(shape, seed, cap=30):
    z, y, x = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    e = 110 + np.minimum(x + y + z, cap)
    return (_base(shape, seed).astype(np.float64) * np.ldexp(1.0, -e)).astype(F)     # (exact: a power of two)


def faint_spikes(shape, seed):
    rng = np.random.default_rng(seed)
    v = np.zeros(shape, F)
    v[1::2] = F(-0.0)
    hit = rng.random(shape) < 0.01
    amp = (rng.uniform(0.5, 1.0, shape) * np.where(rng.random(shape) < 0.5, -1.0, 1.0) * 2.0 ** -128).astype(F)
    v[hit] = amp[hit]
    return v


def huge(shape, seed):
    return _base(shape, seed) * F(2.0 ** 100)


def integer(shape, seed):
    return np.round(_base(shape, seed) * F(100)).astype(F)


def constant(shape, seed):
    return np.full(shape, F(0.1), F)


CLASSES = dict(subnormal=subnormal, fade=fade, faint_spikes=faint_spikes, huge=huge, integer=integer,
               constant=constant)
SCALED_CLASSES = ("subnormal", "fade", "huge")        # what the entries that divide by max|v| run on


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def is_subnormal(a):
    a = np.abs(np.asarray(a, F))
    return (a > 0) & (a < TINY)


def ftz(a):
    """`a` with every subnormal flushed to a zero of its sign: what a kernel built to flush would see and store."""
    a = np.array(a, F)
    a[is_subnormal(a)] *= F(0.0)
    return a


# ----------------------------------------------------------------------------------------------------------------
# FIR cases
# ----------------------------------------------------------------------------------------------------------------
# Gaussian taps: api.gauss_filter of the benchmark's octave-0 sigmas for half widths 2, 4 and 8; g9 (half width 9,
# beyond every template argument) and g33 (sigma 11: 67 taps, beyond the 65-tap tables) for the general kernels
SIGMA = {2: 0.5387011637869722, 4: 1.2262734984654078, 8: 2.4525469969308156, 9: 2.8, 33: 11.0}


def taps(name, gauss_filter):
    """'g<hw>': gauss_filter(SIGMA[hw]); 's<hw>': standard_normal(2 hw + 1), seeded -- signed taps, whose
    cancellation gives subnormal sums from normal terms."""
    hw = int(name[1:])
    if name[0] == "g":
        t = np.asarray(gauss_filter(SIGMA[hw]), F)
    else:
        t = np.random.default_rng(1000 + hw).standard_normal(2 * hw + 1).astype(F)
    assert len(t) == 2 * hw + 1
    return t


class FirCase:
    """entry: 'fir' (hip.fir, one launch per axis of `axes`), 'fir_v1' (hip.fir, variant=1), 'x_scaled'
    (hip.fir_x_scaled), 'yz' (hip.fir_yz), 'xyz' / 'xyz_scaled' (hip.fir_xyz)."""

    def __init__(self, path, entry, shape, taps, uf=1.0, axes=(0,)):
        self.path, self.entry, self.shape, self.taps, self.uf, self.axes = path, entry, shape, taps, F(uf), axes
        self.scaled = entry.endswith("scaled")
        self.id = "%s-%s-%s-%s-uf%.3g-ax%s" % (path, entry, "x".join(map(str, shape)), taps, uf,
                                               "".join(map(str, axes)))

    def classes(self):
        return SCALED_CLASSES if self.scaled else tuple(CLASSES)


def _each_axis(path, shape, taps_names, ufs, axes):
    return [FirCase(path, "fir", shape, t, uf, (ax,)) for t in taps_names for uf in ufs for ax in axes]


# One group per kernel path; the comment gives the launch condition (fir_impl, launch_fir_yz, sift3d_hip_fir_xyz)
# that selects it.  Source and destination of every launch are 16-byte aligned (the guard band is 4096 floats).
FIR_CASES = (
    # 1. k_fir_x_u1: uf == 1, axis 0, 1 <= hw <= 8, nx >= 2 hw + 2, and nx % 512 != 0 (launch_fir_x_u1) -- rows of
    #    one partial segment (23, 64); with scale_max its commit lambda divides (sift3d_hip_fir_x_scaled)
    _each_axis("1_x_u1", (19, 21, 23), ("g4", "g8", "s4"), (1.0,), (0,))
    + _each_axis("1_x_u1", (16, 24, 64), ("g2", "s2"), (1.0,), (0,))
    + [FirCase("1_x_u1", "x_scaled", (19, 21, 23), "g4")]
    # 2. k_fir_x_u1f<HW, SCALED>: as 1. with nx % 512 == 0 and aligned pointers; SCALED where scale_max is given
    + _each_axis("2_x_u1f", (3, 9, 512), ("g2", "g8"), (1.0,), (0,))
    + [FirCase("2_x_u1f", "x_scaled", (3, 9, 512), t) for t in ("g2", "g8")]
    # 3. k_fir_sweep_u1<HW, V>: uf == 1, axes 1 and 2, 1 <= hw <= 8, n >= 2 hw + 2.  V = 4 where the pointers are
    #    aligned and nx % 4 == 0 (axis 1) or nx * ny % 4 == 0 (axis 2): (20, 20, 24); V = 1 otherwise: (19, 21, 23)
    + _each_axis("3_sweep_u1_V4", (20, 20, 24), ("g4", "g8", "s4"), (1.0,), (1, 2))
    + _each_axis("3_sweep_u1_V1", (19, 21, 23), ("g4", "s8"), (1.0,), (1, 2))
    # 4. k_fir_x_dy<HW, S> (axis 0) / k_fir_sweep_dy<HW, S, 4> (axes 1, 2 with V == 4): uf 0.5 (S = 1) and 0.25
    #    (S = 2), hw <= 8 (launch_fir_dy_hw)
    + _each_axis("4_dy", (20, 20, 24), ("g4", "s4"), (0.5, 0.25), (0, 1, 2))
    + _each_axis("4_dy", (20, 20, 24), ("g8",), (0.5,), (0, 1, 2))
    # 5. k_fir_x_dyad<HW> / k_fir_sweep_dyad<HW, V>: a dyadic uf that 4. does not take -- uf 0.125 (shift 3; V = 4
    #    at this shape), and uf 0.5 with hw 9 (dispatch_int<1, 8> refuses: the run-time tap count <0>; V = 1)
    + _each_axis("5_dyad", (20, 20, 24), ("g4",), (0.125,), (0, 1, 2))
    + _each_axis("5_dyad_hw9", (19, 21, 23), ("g9",), (0.5,), (0, 1, 2))
    # 6. k_fir_literal: a uf that is no power of two (1 / 1.5, 1 / 0.7: anisotropic units), or variant == 1
    + _each_axis("6_literal", (17, 20, 24), ("g4",), (1.0 / 1.5, 1.0 / 0.7), (0, 1, 2))
    + [FirCase("6_literal", "fir_v1", (17, 20, 24), "g4", 1.0, (ax,)) for ax in (0, 1, 2)]
    # 7. k_fir_literal_chunk: width > SIFT3D_HIP_MAX_TAPS = 65 (67 taps: launches of 65 + 2 taps, the running sum
    #    carried in dst between them -- a subnormal running sum is the point)
    + _each_axis("7_literal_chunk", (41, 90, 100), ("g33",), (1.0, 0.125), (0, 1, 2))
    # 8. fused y+z without LDS-DMA (k_fir_yz_u1): hip.fir_yz accepts (nx % 4 == 0, aligned, ny and nz >= 2 hw + 2)
    #    and launch_fir_yz's DMA condition (nx % 64 == 0, ny % 64 == 0, ny >= 128) fails: nx = 20
    + [FirCase("8_yz_u1", "yz", (24, 100, 20), t, 1.0, (1, 2)) for t in ("g2", "g8")]
    # 9. k_fir_yz_dma: nx % 64 == 0, ny % 64 == 0, ny >= 128, z segments of at most DMA_MAX_TS planes; the fewest
    #    planes the entry accepts, 2 hw + 2
    + [FirCase("9_yz_dma", "yz", (2 * hw + 2, 128, 64), t, 1.0, (1, 2))
       for hw, t in ((2, "g2"), (8, "g8"), (2, "s2"), (8, "s8"))]
    # 10. k_fir_xyz_dma<.., SCALED>: sift3d_hip_fir_xyz_covers (uf 1 on every axis, nx % 64 == 0, ny % 64 == 0,
    #     ny >= 128, hw <= 8, aligned); nz = 3 is shorter than every window, 18 = 2 hw + 2 for 17 taps
    + [FirCase("10_xyz_dma", e, s, t, 1.0, (0, 1, 2))
       for e in ("xyz", "xyz_scaled") for s, t in (((3, 128, 64), "g2"), ((18, 128, 64), "g8"))]
)
FIR_CASES = tuple(FIR_CASES)
FIR_PATHS = ("1_x_u1", "2_x_u1f", "3_sweep_u1_V4", "3_sweep_u1_V1", "4_dy", "5_dyad", "5_dyad_hw9", "6_literal",
             "7_literal_chunk", "8_yz_u1", "9_yz_dma", "10_xyz_dma")


def content(case, cls):
    """The volume of one (case, class): seeded by the shape and the class, so that cases of one shape share it."""
    seed = sum(case.shape) * 7 + sorted(CLASSES).index(cls)
    return CLASSES[cls](case.shape, seed)


def scaled_input(vol):
    """im_scale (imutil.c:698-713) by numpy: float32 IEEE division by max |v| -- no code shared with the kernels."""
    mx = np.abs(vol).max()
    assert mx.dtype == F and mx != F(0.0) and mx != F(1.0)
    return (vol / mx).astype(F), mx


def oracle_fir(oracle_mod, vol, tap_values, axes, uf, flush=False):
    """The case's passes by the oracle, one axis after the other; flush=True: what a kernel would give that reads
    and stores subnormals as zeros."""
    if flush:
        vol = ftz(vol)
    for ax in axes:
        vol, r = oracle_mod.fir_axis(vol, tap_values, ax, uf=F(uf), mode=0)
        assert r == 0
        if flush:
            vol = ftz(vol)
    return vol


# ----------------------------------------------------------------------------------------------------------------
# absmax: the three zones of k_absmax's loop (and of k_sub_absmax's)
# ----------------------------------------------------------------------------------------------------------------
def grid_for(n, per_thread):
    """sift3d_kernels_common.h: workgroups of 256 threads, per_thread elements each, between 1 and 4096."""
    return min(max((n // per_thread + 255) // 256, 1), 256 * 16)


def grid_reduce(n):
    """sift3d_kernels_common.h: the streaming reductions take a quad per thread and at most 1024 workgroups."""
    return min(grid_for(n, 4), 256 * 4)


NTHR_MAX = 256 * 4 * 256                  # threads of the largest reduction grid: 262 144
# k_absmax: thread t takes quads t, t + T, t + 2T, ... (T = threads of the grid), four of them per round while
# `i + 3 T < n4`, then one per round, then the n % 4 floats of the tail.  With n4 <= T no thread has a second
# quad, and the unrolled zone needs n4 > 3 T, which the grid cap makes n > 12 * 262 144 = 3 145 728: the sizes
# below 1024 * 1024 + 3 have the one-quad zone and the tail only.  4 * (3 T) + 4 * T + 7 = 16 T + 7 has every thread
# in the unrolled zone for exactly one round, ONE quad (that of thread 0) in the one-quad zone behind it and a tail
# of three; the last size makes that 1000 quads, so that whole waves run the one-quad zone AFTER an unrolled round.
ABSMAX_SIZES = (1, 3, 4, 5, 1023, 1024 * 1024 + 3, 4 * (3 * NTHR_MAX) + 4 * NTHR_MAX + 7,
                4 * (4 * NTHR_MAX + 1000) + 3)


def absmax_zones(n):
    """The zones of k_absmax's loop at size n: dict(unrolled=, quad=, tail=) of the (first, last) element index
    that each zone reads, a zone the size does not have missing.  (The unrolled and the one-quad zone interleave
    where only some threads have a whole unrolled round; at ABSMAX_SIZES they are contiguous ranges.)"""
    T = grid_reduce(n) * 256
    n4 = n // 4
    q = np.arange(n4, dtype=np.int64)
    rnd = (q // T) // 4                                     # the round of its thread in which a quad falls
    unrolled = (q % T) + 4 * T * rnd + 3 * T < n4           # ... runs unrolled if the round's last quad exists
    out = {}
    for name, sel in (("unrolled", q[unrolled]), ("quad", q[~unrolled])):
        if len(sel):
            out[name] = (int(4 * sel[0]), int(4 * sel[-1] + 3))
    if n % 4:
        out["tail"] = (4 * n4, n - 1)
    return out


# ----------------------------------------------------------------------------------------------------------------
# level pairs whose differences are exact and mostly subnormal
# ----------------------------------------------------------------------------------------------------------------
def faded_levels(shape, count, seed):
    """`count` levels: the first is `fade` with its exponent stopped at 126 (values from 2**-110 down to the
    smallest normals), each next one the one before times float32(1 + 2**-20), rounded to float32 -- neighbours
    differ by a few units of the last place, so that their differences are exact and subnormal (2**-130 and
    below).  The last two levels are identical (difference +0.0, maximum +0.0) where count >= 3."""
    lv = [fade(shape, seed, cap=16)]
    for k in range(1, count):
        lv.append(lv[-1].copy() if (k == count - 1 and count >= 3) else lv[-1] * F(1 + 2.0 ** -20))
    return lv


# ----------------------------------------------------------------------------------------------------------------
# end-to-end volumes (tests/test_detect_content*.py, and the g3_spikes64 / g3_integer48 / g3_subnormal48 fixtures)
# ----------------------------------------------------------------------------------------------------------------
DETECT_SEED = 20261021
DETECT_CASES = ("spikes64", "boxed64", "integer48", "huge48", "tiny48", "subnormal48", "negative48")
SAME_AS_SURVEY48 = ("huge48", "tiny48", "subnormal48", "negative48")     # rescalings of synth_survey(48)


def detect_volume(name, so):
    """(volume, detector parameters) of an end-to-end case; `so` provides synth_survey (the oracle module)."""
    kw = {}
    if name == "spikes64":
        # exact zero but for twelve voxels of uniform(0.5, 1), at least 4 voxels from every face
        rng = np.random.default_rng(DETECT_SEED)
        vol = np.zeros((64, 64, 64), F)
        pos = rng.integers(4, 60, size=(12, 3))
        vol[pos[:, 0], pos[:, 1], pos[:, 2]] = rng.uniform(0.5, 1.0, 12).astype(F)
        assert np.count_nonzero(vol) == 12
        kw = dict(peak_thresh=0.02)
    elif name == "boxed64":
        # the survey volume inside the central cube of half side 64 // 5, exact zero outside
        n, h = 64, 64 // 5
        mask = np.zeros((n, n, n), F)
        mask[n // 2 - h:n // 2 + h, n // 2 - h:n // 2 + h, n // 2 - h:n // 2 + h] = 1
        vol = so.synth_survey(n) * mask
    else:
        s = so.synth_survey(48)
        if name == "integer48":
            # CT-like integers: none positive (the maximum of the survey volume maps to 0), with plateaus
            vol = np.round(s / s.max() * F(40)) * F(25) - F(1000)
            assert vol.max() <= 0 and vol.min() < -900 and len(np.unique(vol)) <= 100
        elif name == "huge48":
            vol = s * F(1e30)
        elif name == "tiny48":
            vol = s * F(1e-30)
        elif name == "subnormal48":
            # subnormal input; its maximum divides it back to order 1
            vol = (s * F(1e-20)) * F(1e-20)
            assert is_subnormal(vol.max())
        elif name == "negative48":
            vol = -s
        else:
            raise KeyError(name)
    vol = np.ascontiguousarray(vol, F)
    assert np.isfinite(vol).all()
    return vol, kw
