#!/usr/bin/env python3
"""Rates of the cubic B-spline kernels (sift3d_bspline.hip) at 512^3, beside the existing kernels they are measured
against, all in one run:

    prefilter                         sift3d_hip_bspline_prefilter    3 passes, 8 B/voxel each algorithmically
      against copy_ of the volume, and against the detector's separable blur with as many taps (2H + 1 = 33).  A
      level's blur at that width is three sift3d_hip_fir passes, its slowest form: the fused y+z kernel and the
      17-tap x kernel that make the pyramid fast stop at 17 taps, so this reference runs far below a copy's rate
    bspline_warp_affine               against sift3d_hip_warp_affine linear, the oblique map of warp_rate.py
    bspline_warp_field nc = 1 and 12  against sift3d_hip_warp_field linear, that map's field

    python3 profiles/microbench/bspline_rate.py > profiles/microbench/bspline_rate_mi355x.txt

Device events around `reps` back-to-back calls, per call; 3 trials that alternate between the kernels of a pair, the
minimum of each; one process, the device to itself.  Algorithmic bytes / time against the 8 TB/s HBM peak."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N = 512
HBM = 8e12


def _trial(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def _alternate(fns, reps):
    """min of 3 trials per function, the trials alternating between the functions (after one warm-up call each)"""
    for fn in fns:
        fn()
    best = [float("inf")] * len(fns)
    for _ in range(3):
        for i, fn in enumerate(fns):
            best[i] = min(best[i], _trial(fn, reps))
    return best


def _oblique():
    """warp_rate.py's oblique_s0.8: a rotation about (1, 2, 3) by 23 degrees, scaled by 0.8, about the centre"""
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    t = np.deg2rad(23.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    M = 0.8 * (np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K))
    c = np.full(3, (N - 1) / 2.0)
    return np.hstack([M, (c - M @ c)[:, None]])


def _taps33():
    from sift3d_amd import api
    for s in np.arange(2.0, 12.0, 0.05):
        t = api.gauss_filter(float(s))
        if len(t) == 33:
            return float(s), t
    sys.exit("no sigma gives 33 taps")


def run():
    import torch
    from sift3d_amd import hip
    vox = float(N) ** 3
    A = _oblique()
    src = torch.rand((N, N, N), device="cuda")
    dst = torch.empty_like(src)
    tmp = torch.empty_like(src)
    work = torch.empty_like(src)
    print("# cubic B-spline resampling, float32 %d^3, MI355X (gfx950); HIP events around back-to-back calls, per "
          "call, min of 3 alternating trials after one warm-up" % N)
    print("%-40s %10s %9s %10s %9s" % ("call", "ms", "alg GB", "frac 8TB/s", "x ref"))

    def line(name, ms, nbytes, ref=None):
        print("%-40s %10.4f %9.3f %10.3f %9s" % (name, ms, nbytes / 1e9, (nbytes / HBM * 1e3) / ms,
                                                 "-" if ref is None else "%.2f" % (ms / ref)))

    sigma, taps = _taps33()

    def blur():
        hip.fir(src, dst, 0, taps)
        hip.fir(dst, tmp, 1, taps)
        hip.fir(tmp, dst, 2, taps)

    ms = _alternate([lambda: dst.copy_(src), blur, lambda: hip.bspline_prefilter(src, dst, work)], 10)
    line("copy_", ms[0], 8 * vox)
    line("blur, 33 taps (sigma %.2f), 3 x fir" % sigma, ms[1], 24 * vox)
    line("bspline_prefilter (x ref: the blur)", ms[2], 24 * vox, ms[1])
    coef = hip.bspline_prefilter(src)
    ms = _alternate([lambda: hip.warp_affine(src, dst, A), lambda: hip.bspline_warp_affine(coef, dst, A)], 10)
    line("warp_affine linear", ms[0], 8 * vox)
    line("bspline_warp_affine", ms[1], 8 * vox, ms[0])
    field = torch.empty((3, N, N, N), device="cuda")
    hip.affine_field(field, A)
    ms = _alternate([lambda: hip.warp_field(src, dst, field), lambda: hip.bspline_warp_field(coef, dst, field)], 10)
    line("warp_field linear nc=1", ms[0], 20 * vox)
    line("bspline_warp_field nc=1", ms[1], 20 * vox, ms[0])
    del tmp, work, coef
    # (the cubic row samples src12 itself, raw values standing in for coefficients: the time does not depend on them)
    src12 = torch.rand((12, N, N, N), device="cuda")
    dst12 = torch.empty_like(src12)
    ms = _alternate([lambda: hip.warp_field(src12, dst12, field),
                     lambda: hip.bspline_warp_field(src12, dst12, field)], 3)
    line("warp_field linear nc=12", ms[0], 108 * vox)
    line("bspline_warp_field nc=12", ms[1], 108 * vox, ms[0])


if __name__ == "__main__":
    lib = os.environ.get("SIFT3D_AMD_LIB") or os.path.join(ROOT, "sift3d_amd", "libsift3d_amd.so")
    if not os.path.exists(lib):
        sys.exit("%s is missing -- build first: python3 -c \"from sift3d_amd import _native; _native.build()\"" % lib)
    run()
