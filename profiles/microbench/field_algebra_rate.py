#!/usr/bin/env python3
"""Rates of field composition, the exponential, the inverse and the diffeomorphic demons update (sift3d_warp.hip
k_field_compose, sift3d_field_ops.c) at 512^3, u = v = the field of DESIGN.md §3.4.2's oblique rotation (§3.4.4):

    COMPOSE                  sift3d_hip_field_compose, no statistics
    v + warp_field(u, v)     the composition before k_field_compose: warp_field nc = 3 into a temporary, then a torch add
    warp_field nc = 3        k_warp_field<2> on the same v
    INVERT step              sift3d_hip_field_compose INVERT with statistics
    exp, K = 4               sift3d_amd_field_exp_device
    demons iteration nc=12   one additive and one diffeomorphic iteration (K = 0 and 2), alpha 1, sigmas 1.0 / 1.5

Targets, same run: COMPOSE <= v + warp_field(u, v); COMPOSE <= 1.10 x warp_field nc = 3.

    python3 profiles/microbench/field_algebra_rate.py > profiles/microbench/field_algebra_rate_mi355x.txt

Device events around back-to-back calls, per call; the compared calls alternate within each of 3 trials after one
warm-up, and each keeps its minimum."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N = 512
NC = 12
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


def _min_alternating(fns, reps, trials=3):
    for fn in fns.values():
        fn()
    best = {k: float("inf") for k in fns}
    for _ in range(trials):
        for k, fn in fns.items():
            best[k] = min(best[k], _trial(fn, reps))
    return best


def run():
    import torch
    from sift3d_amd import hip
    from field_rate import _oblique
    vox = float(N) ** 3
    v = torch.empty((3, N, N, N), device="cuda")
    hip.affine_field(v, _oblique())
    u = v
    out = torch.empty_like(v)
    tmp = torch.empty_like(v)
    sum_out = torch.empty_like(v)
    print("# field composition, float32 %d^3 fields, u = v = the oblique rotation's field, MI355X (gfx950); HIP events "
          "around back-to-back calls, per call, min of 3 alternating trials after one warm-up" % N)
    print("%-44s %10s %9s %10s" % ("call", "ms", "alg GB", "frac 8TB/s"))

    def line(name, ms, nbytes):
        print("%-44s %10.4f %9.3f %10.3f" % (name, ms, nbytes / 1e9, (nbytes / HBM * 1e3) / ms if nbytes else 0.0))

    def compose():
        hip.field_compose(u, v, out, "compose")

    def parent():
        hip.warp_field(u, tmp, v)
        torch.add(v, tmp, out=sum_out)

    def warp3():
        hip.warp_field(u, tmp, v)

    t = _min_alternating({"compose": compose, "parent": parent, "warp": warp3}, 5)
    line("COMPOSE (no stats)", t["compose"], 24 * vox)
    line("v + warp_field(u, v) (parent's composition)", t["parent"], 60 * vox)
    line("warp_field linear nc=3 (k_warp_field<2>)", t["warp"], 24 * vox)
    r1 = t["compose"] / t["parent"]
    r2 = t["compose"] / t["warp"]
    print("# target 1: COMPOSE / (v + warp_field) = %.3f (must be <= 1): %s" % (r1, "met" if r1 <= 1 else "MISSED"))
    print("# target 2: COMPOSE / warp_field nc=3 = %.3f (must be <= 1.10): %s" % (r2, "met" if r2 <= 1.10 else "MISSED"))
    stats = torch.empty(4, dtype=torch.int64, device="cuda")
    work = torch.empty(hip.FIELD_WORK_BYTES // 8, dtype=torch.int64, device="cuda")
    ework = torch.empty(3 * N ** 3, dtype=torch.float32, device="cuda")
    t2 = _min_alternating({
        "invert": lambda: hip.field_compose(u, v, out, "invert", stats, work),
        "exp4": lambda: hip.field_exp(v, out, 4, ework),
    }, 3)
    line("INVERT step (with stats)", t2["invert"], 24 * vox)
    line("exp, K = 4 (scale + 4 COMPOSE)", t2["exp4"], 0)
    del out, tmp, sum_out, ework
    torch.cuda.empty_cache()
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    F = torch.rand((NC, N, N, N), device="cuda", generator=g)
    M = torch.rand((NC, N, N, N), device="cuda", generator=g)
    f0 = (torch.rand((3, N, N, N), device="cuda", generator=g) - 0.5) * 2.0
    uu = torch.empty_like(f0)
    dwork = torch.empty((hip.lib().sift3d_amd_demons_work_floats_ex(N, N, N, NC, 1) + 1) // 2, dtype=torch.float64,
                        device="cuda")

    def it(update, K):
        def f():
            uu.copy_(f0)
            hip.demons(F, M, uu, 1, 1.0, 1.0, 1.5, dwork, update=update, squarings=K)
        return f
    t3 = _min_alternating({"copy": lambda: uu.copy_(f0), "add": it("additive", 0), "dif0": it("diffeomorphic", 0),
                           "dif2": it("diffeomorphic", 2)}, 2)
    line("field copy (subtracted below)", t3["copy"], 24 * vox)
    line("demons iteration nc=12, additive", t3["add"] - t3["copy"], 0)
    line("demons iteration nc=12, diffeomorphic K=0", t3["dif0"] - t3["copy"], 0)
    line("demons iteration nc=12, diffeomorphic K=2", t3["dif2"] - t3["copy"], 0)


if __name__ == "__main__":
    np.seterr(all="ignore")
    run()
