#!/usr/bin/env python3
"""Rate of the Euclidean distance transform (sift3d_hip_distance_sq) and of one surface-distance call.

The transform at 256^3 and 512^3 on three masks -- a ball of radius n / 4, a thin shell (the ball's six-neighbour
surface: the surface-distance use case) and a single corner voxel (the worst case of the outward line search: all but
one line of the y pass and all but one plane of the z pass hold no feature nearby, so every voxel walks its whole line,
O(n) per voxel per pass) -- each at unit spacing and at (0.7, 1.3, 2.5).  Then one api.surface_distances call on two
256^3 four-label volumes (three nested balls, the moving ones shifted), which runs per label two surfaces, two
transforms, two collections and the host sort, and waits for the stream twice.

Times are HIP events around single calls, the median of `reps` after a warm-up (the corner mask: fewer, its calls are
long); the surface-distance call is synchronous and timed by the host clock, the median of 3.  Floor: the three passes
read and write 4 B per voxel each, 3 x 8 B per voxel, against the 8 TB/s HBM peak.

    python3 profiles/microbench/distance_rate.py [--label TEXT] [--sizes 512] [--no-surface] > OUT.txt

SIFT3D_AMD_LIB selects another build of the library: one made with `make DISTDEF="-DEDT_RUN=r -DEDT_STEP=s"` times the
line passes with r consecutive outputs per wave and s radii per step of the search."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from similarity_rate import _require_built  # noqa: E402

PEAK_BPS = 8.0e12
SPACINGS = (("unit", None), ("aniso", (0.7, 1.3, 2.5)))


def _ball(n, r, c=None):
    import torch
    c = [(n - 1) / 2.0] * 3 if c is None else c
    ax = [(torch.arange(n, device="cuda", dtype=torch.float32) - float(ci)) ** 2 for ci in c]
    return (ax[0][:, None, None] + ax[1][None, :, None] + ax[2][None, None, :]) <= float(r) ** 2


def _masks(n):
    import torch
    from sift3d_amd import hip
    ball = _ball(n, n / 4.0).float().contiguous()
    shell, count = hip.label_surface(ball, 1)
    corner = torch.zeros((n, n, n), device="cuda")
    corner[0, 0, 0] = 1
    return (("ball", ball), ("shell", shell), ("corner", corner)), int(count.item())


def _median_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), min(ms), max(ms)


def _labels(n, shift):
    """three nested balls: labels 3, 2, 1 from the centre outwards, 0 outside"""
    import torch
    c = [(n - 1) / 2.0 + s for s in shift]
    L = torch.zeros((n, n, n), device="cuda")
    for k, r in ((1, 0.40), (2, 0.28), (3, 0.15)):
        L[_ball(n, r * n, c)] = float(k)
    return L.contiguous()


def run(label, reps, sizes, surface):
    import torch
    from sift3d_amd import api, hip
    print("# Euclidean distance transform, float32, MI355X (gfx950)%s" % (label and "; " + label))
    print("# sift3d_hip_distance_sq: HIP events around single calls, median of %d (corner: %d) [min-max]; floor: "
          "3 passes x 8 B / voxel at 8 TB/s" % (reps, max(reps // 4, 3)))
    print("%-5s %-7s %-6s %30s %10s %9s" % ("n", "mask", "space", "ms", "floor ms", "of floor"))
    for n in sizes:
        masks, shell_voxels = _masks(n)
        out = torch.empty((n, n, n), device="cuda")
        work = torch.empty(hip.distance_work_bytes((n, n, n)) // 4, device="cuda")
        floor = 3 * 8.0 * float(n) ** 3 / PEAK_BPS * 1e3
        for name, mask in masks:
            for sname, sp in SPACINGS:
                r = max(reps // 4, 3) if name == "corner" else reps
                med, lo, hi = _median_ms(lambda: hip.distance(mask, sp, "sq", out=out, work=work), r)
                print("%-5d %-7s %-6s %10.3f [%8.3f-%8.3f] %10.3f %9.3f" % (n, name, sname, med, lo, hi, floor,
                                                                            floor / med))
        print("# n = %d: the shell holds %d voxels; corner: one feature at (0, 0, 0), the O(n)-per-voxel worst case of "
              "the outward search" % (n, shell_voxels))
        del masks, out, work
    if not surface:
        return
    n = 256
    LF, LM = _labels(n, (0, 0, 0)), _labels(n, (3, -2, 4))
    sec = []
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = api.surface_distances(LF, LM, num_labels=4, spacing=(0.7, 1.3, 2.5))
        sec.append(time.perf_counter() - t0)
    sec = sec[1:]                                            # the first call warms up
    print("# api.surface_distances, two %d^3 four-label volumes (three labels reported), spacing (0.7, 1.3, 2.5): host "
          "clock around the synchronous call, median of 3 [min-max]" % n)
    print("%-5d %-14s %10.3f [%8.3f-%8.3f] ms; surface voxels %s / %s; hausdorff %s" % (
        n, "surface_dist", 1e3 * float(np.median(sec)), 1e3 * min(sec), 1e3 * max(sec), res.n_fixed.tolist(),
        res.n_moving.tolist(), np.round(res.hausdorff, 4).tolist()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--label", default="")
    ap.add_argument("--sizes", default="256,512", help="the transform's volume edges")
    ap.add_argument("--no-surface", action="store_true", help="skip the surface-distance call")
    a = ap.parse_args()
    _require_built()
    run(a.label, a.reps, [int(v) for v in a.sizes.split(",")], not a.no_surface)


if __name__ == "__main__":
    main()
