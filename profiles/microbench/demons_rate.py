#!/usr/bin/env python3
"""Rates of the dense demons refinement (sift3d_demons.hip, sift3d_demons.c) at 512^3, nc = 12, sigma 1.6
(DESIGN.md §3.4.3):

    force            sift3d_hip_demons_force   120 B/voxel at nc = 12 (F 48 + W 48 + u 12 read, delta 12 written)
    warp_field nc=12 sift3d_hip_warp_field     the gate: the force takes no longer than this, in the same run
    one iteration    warp, force, fluid blur (3 channels), u += delta, diffusion blur (3 channels), each timed
    refine_field     50 iterations, features "descriptors" (both dense descriptor images included)

    python3 profiles/microbench/demons_rate.py > profiles/microbench/demons_rate_mi355x.txt

Device events around back-to-back calls, per call, min of 3 trials after one warm-up.  Kernel times, in a run of
their own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python3 profiles/microbench/demons_rate.py --launches
    python3 profiles/microbench/demons_rate.py --report OUT >> profiles/microbench/demons_rate_mi355x.txt"""
import argparse
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N = 512
NC = 12
HBM = 8e12


def _ms(fn, reps):
    import torch
    fn()
    best = float("inf")
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps)
    return best


def _setup():
    import torch
    from sift3d_amd import hip
    from field_rate import _oblique
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    F = torch.rand((NC, N, N, N), device="cuda", generator=g)
    M = torch.rand((NC, N, N, N), device="cuda", generator=g)
    W = torch.empty_like(F)
    u = (torch.rand((3, N, N, N), device="cuda", generator=g) - 0.5) * 2.0
    obl = torch.empty_like(u)
    hip.affine_field(obl, _oblique())
    step = torch.empty_like(u)
    return F, M, W, u, obl, step


def run():
    import torch
    from sift3d_amd import api, hip
    vox = float(N) ** 3
    F, M, W, u, obl, step = _setup()
    L, st = hip.lib(), hip.current_stream()
    stats = torch.empty(2, dtype=torch.int64, device="cuda")
    pw = torch.empty(hip.DEMONS_FORCE_WORK_BYTES // 8, dtype=torch.int64, device="cuda")
    print("# dense demons, float32 %d^3, nc = %d, MI355X (gfx950); HIP events around back-to-back calls, per call, "
          "min of 3 trials after one warm-up" % (N, NC))
    print("%-40s %10s %9s %10s" % ("call", "ms", "alg GB", "frac 8TB/s"))

    def line(name, ms, nbytes):
        print("%-40s %10.4f %9.3f %10.3f" % (name, ms, nbytes / 1e9, (nbytes / HBM * 1e3) / ms if nbytes else 0.0))

    def force():
        assert L.sift3d_hip_demons_force(F.data_ptr(), N, N, N, W.data_ptr(), u.data_ptr(), N, N, N, NC, 1.0,
                                         step.data_ptr(), stats.data_ptr(), pw.data_ptr(), st) == 0
    hip.warp_field(M, W, u)
    t_force = _ms(force, 5)
    t_warp_obl = _ms(lambda: hip.warp_field(M, W, obl), 5)
    line("force nc=12", t_force, 120 * vox)
    line("warp_field linear nc=12, oblique field", t_warp_obl, 108 * vox)
    print("# gate: force / warp_field nc=12 (same run) = %.3f (must be <= 1)" % (t_force / t_warp_obl))
    # one iteration, stage by stage (the driver's stages through their own entries)
    A = api
    t_warp = _ms(lambda: hip.warp_field(M, W, u), 5)
    work = torch.empty((hip.lib().sift3d_amd_demons_work_floats(N, N, N, NC) + 1) // 2, dtype=torch.float64,
                       device="cuda")
    line("iteration: warp_field (field ~ +-1 voxel)", t_warp, 108 * vox)
    line("iteration: force", t_force, 120 * vox)
    t1 = {}
    for sf, sd in ((0.0, 0.0), (1.0, 0.0), (0.0, 1.5), (1.0, 1.5)):
        uu = u.clone()
        t1[(sf, sd)] = _ms(lambda: hip.demons(F, M, uu, 1, 1.0, sf, sd, work), 3)
    line("iteration, no smoothing (warp+force+add)", t1[(0.0, 0.0)], 0)
    line("iteration, sigma_fluid 1.0", t1[(1.0, 0.0)], 0)
    line("iteration, sigma_diffusion 1.5", t1[(0.0, 1.5)], 0)
    line("iteration, sigma_fluid 1.0, sigma_diffusion 1.5", t1[(1.0, 1.5)], 0)
    print("# whole iterations: the field changes between calls and the warp's time follows it, so differences of "
          "these lines are no stage times; k_field_add and the blur passes are timed alone in the kernel trace below")
    line("iteration at the defaults (%g, %g, %g)" % (A.DEMONS_ALPHA, A.DEMONS_SIGMA_FLUID, A.DEMONS_SIGMA_DIFFUSION),
         _ms(lambda: hip.demons(F, M, u.clone(), 1, A.DEMONS_ALPHA, A.DEMONS_SIGMA_FLUID, A.DEMONS_SIGMA_DIFFUSION,
                                work), 3), 0)
    del F, M, W, work, obl
    torch.cuda.empty_cache()
    fixed = torch.empty((N, N, N), device="cuda")
    hip.synth_lattice(fixed, 0, 21)
    moving = torch.empty_like(fixed)
    hip.synth_lattice(moving, 0, 22)
    t_ref = _ms(lambda: api.refine_field(moving, fixed, None, 50, sigma=1.6), 1)
    line("refine_field, 50 iterations, descriptors", t_ref, 0)


def launches():
    """for the kernel trace: 1 warm-up + 3 forces, 1 + 3 warp_field nc=12 of the oblique field, 2 iterations"""
    import torch
    from sift3d_amd import hip
    F, M, W, u, obl, step = _setup()
    for _ in range(4):
        hip.demons_force(F, W, u, step, 1.0, (N, N, N))
    for _ in range(4):
        hip.warp_field(M, W, obl)
    hip.demons(F, M, u, 2, 1.0, 1.0, 1.5)
    torch.cuda.synchronize()


def report(d):
    rows = []
    for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    print("# rocprofv3 --kernel-trace --stats (a run of its own: %s)" % "demons_rate.py --launches")
    print("%-60s %7s %12s %12s %12s" % ("kernel", "calls", "avg ms", "min ms", "max ms"))
    for r in rows:
        name = r.get("Name", "")[:60]
        print("%-60s %7s %12.4f %12.4f %12.4f" % (name, r.get("Calls"), float(r.get("AverageNs", 0)) / 1e6,
                                                float(r.get("MinNs", 0)) / 1e6, float(r.get("MaxNs", 0)) / 1e6))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--report")
    a = ap.parse_args()
    if a.report:
        report(a.report)
    else:
        np.seterr(all="ignore")
        launches() if a.launches else run()
