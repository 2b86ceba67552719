#!/usr/bin/env python3
"""Which kernels the demons family launches, and how often: the check that a change of the host drivers
(sift3d_demons.c, sift3d_field_ops.c, sift3d_amd/hip.py, sift3d_amd/api.py) left the device work as it was.  One
pass over every driver at a modest size (48 x 40 x 36, two channels):

    hip.demons           both updates x squarings 0 / 2 x sigmas (0, 0) / (1, 2), 3 iterations, and 0 iterations
    hip.demons_multires  3 levels with iterations (2, 0, 3) (the middle level runs nothing), both updates
    hip.field_exp        0 and 3 squarings
    hip.field_invert     4 iterations
    api.refine_field     intensity and descriptors, 1 and 3 levels, both updates

In a run of its own, without counters, then the table kernel -> calls, which must be the same before and after:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python3 profiles/microbench/demons_launches.py
    python3 profiles/microbench/demons_launches.py --report OUT > profiles/microbench/demons_launches_mi355x.txt"""
import argparse
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SHAPE = (36, 40, 48)
NC = 2


def launches():
    import torch
    from sift3d_amd import api, hip
    g = torch.Generator(device="cuda")
    g.manual_seed(3)

    def stack(shape):
        return torch.rand((NC,) + tuple(shape), device="cuda", generator=g)

    shapes = [SHAPE, hip.half_shape(SHAPE), hip.half_shape(hip.half_shape(SHAPE))]
    Fs, Ms = [stack(s) for s in shapes], [stack(s) for s in shapes]
    u0 = (torch.rand((3,) + SHAPE, device="cuda", generator=g) - 0.5) * 2.0
    for update in ("additive", "diffeomorphic"):
        for squarings in (0, 2):
            for sf, sd in ((0.0, 0.0), (1.0, 2.0)):
                hip.demons(Fs[0], Ms[0], u0.clone(), 3, 1.0, sf, sd, update=update, squarings=squarings)
        hip.demons(Fs[0], Ms[0], u0.clone(), 0, 1.0, 1.0, 2.0, update=update, squarings=2)
        hip.demons_multires(Fs, Ms, u0.clone(), (2, 0, 3), 1.0, 1.0, 2.0, update=update, squarings=2)
    out = torch.empty_like(u0)
    for squarings in (0, 3):
        hip.field_exp(u0, out, squarings)
    hip.field_invert(u0 * 0.25, torch.zeros_like(u0), 4)
    fixed = torch.empty(SHAPE, device="cuda")
    hip.synth_lattice(fixed, 0, 21)
    moving = torch.roll(fixed, (1, 2, 1), (0, 1, 2)).contiguous()
    for features in ("intensity", "descriptors"):
        for levels in (1, 3):
            for update in ("additive", "diffeomorphic"):
                api.refine_field(moving, fixed, None, 3, alpha=0.5, features=features, update=update, levels=levels)
    torch.cuda.synchronize()


def report(d):
    calls = {}
    for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                name = r["Name"][:110]           # (torch's own kernels have names of kilobytes)
                calls[name] = calls.get(name, 0) + int(r["Calls"])
    print("# kernels launched by profiles/microbench/demons_launches.py (rocprofv3 --kernel-trace --stats, a run of "
          "its own), MI355X (gfx950)")
    print("%7s  %s" % ("calls", "kernel"))
    for name in sorted(calls):
        print("%7d  %s" % (calls[name], name))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--report")
    a = ap.parse_args()
    report(a.report) if a.report else launches()
