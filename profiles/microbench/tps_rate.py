#!/usr/bin/env python3
"""Rate of the thin-plate-spline resampling kernel (sift3d_hip_warp_tps) at 512^3 -> 512^3, linear mode,
for m = 256, 1024 and 4096 control points, and of the host fit (sift3d_amd_tps_fit) at m = 1024 and 2048.

The kernel is compute-bound: the cost model counts VALU instructions per voxel-point (one voxel, one
control point).  The counters of one case come from a run of their own:

    python3 profiles/microbench/tps_rate.py > profiles/microbench/tps_rate_mi355x.txt
    rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES --output-format csv -d OUT/pmc -o run -- \\
        python3 profiles/microbench/tps_rate.py --launches
    python3 profiles/microbench/tps_rate.py --report OUT/pmc >> profiles/microbench/tps_rate_mi355x.txt

--launches warms up once, then issues one call at m = 1024 (its launches are the last rows of the
counter file).  --report needs no GPU."""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N = 512
CU, SIMD, CLK = 256, 4, 2.4e9                     # MI355X: CUs, SIMDs per CU, peak engine clock


def _require_built():
    """Under rocprofv3 the GPU is initialised before Python starts: building from here (a fork + exec of
    make) is not allowed.  Build first."""
    lib = os.environ.get("SIFT3D_AMD_LIB") or os.path.join(ROOT, "sift3d_amd", "libsift3d_amd.so")
    if not os.path.exists(lib):
        sys.exit("%s is missing -- build first: python3 -c \"from sift3d_amd import _native; "
                 "_native.build()\"" % lib)


def _tps(m, seed=1):
    """m points over the grid, weights that move samples by ~2 voxels, a slight rotation"""
    from sift3d_amd import api
    rng = np.random.default_rng(seed)
    ctrl = rng.uniform(0, N - 1, (m, 3))
    w = rng.normal(0, 1, (m, 3))
    w -= w.mean(0)
    w *= 2.0 / (np.sqrt(m) * N / 4)
    c = np.full(3, (N - 1) / 2.0)
    t = np.deg2rad(5.0)
    R = np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]])
    A = np.hstack([R, (c - R @ c)[:, None]])
    return api.TPS(ctrl, w, A)


def _kernel_ms(m, reps=3):
    import torch
    from sift3d_amd import hip
    src = torch.rand((N, N, N), device="cuda")
    dst = torch.empty_like(src)
    tps = _tps(m)
    hip.warp_tps(src, dst, tps)                   # warm-up
    best = float("inf")
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hip.warp_tps(src, dst, tps)
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best, hip.warp_tps_launches((N, N, N), m)


def _fit_s(m, reps=3):
    from sift3d_amd import api
    rng = np.random.default_rng(m)
    src = rng.uniform(0, N - 1, (m, 3))
    dst = src + rng.normal(0, 2, (m, 3))
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        api.tps_fit(src, dst, 1.0, m)
        best = min(best, time.perf_counter() - t0)
    return best


def run():
    print("# sift3d_hip_warp_tps, float32 %d^3 -> %d^3, linear, MI355X (gfx950); device events, min of 3 "
          "after one warm-up (the call includes the 32 B/point upload)" % (N, N))
    print("# target: 512^3 at m = 1024 in 120 ms")
    print("%-8s %9s %10s %16s %20s" % ("m", "ms", "launches", "ps/voxel-point", "SIMD cyc/voxel-point"))
    for m in (256, 1024, 4096):
        ms, nl = _kernel_ms(m)
        vp = float(N) ** 3 * m
        print("%-8d %9.2f %10d %16.4f %20.3f" % (m, ms, nl, ms * 1e9 / vp, ms * 1e-3 * CU * SIMD * CLK / vp))
    print("# sift3d_amd_tps_fit (host, OpenMP team <= 16), min of 3")
    for m in (1024, 2048):
        print("fit m=%-5d %9.1f ms" % (m, _fit_s(m) * 1e3))


def launches():
    from sift3d_amd import hip
    import torch
    src = torch.rand((N, N, N), device="cuda")
    dst = torch.empty_like(src)
    tps = _tps(1024)
    hip.warp_tps(src, dst, tps)
    torch.cuda.synchronize()
    hip.warp_tps(src, dst, tps)
    torch.cuda.synchronize()
    print("launches per call: %d" % hip.warp_tps_launches((N, N, N), 1024))


def report(d):
    rows = []
    for f in sorted(glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)):
        with open(f) as fh:
            rows += [r for r in csv.DictReader(fh) if "k_warp_tps" in r.get("Kernel_Name", "")]
    tot = {}
    for r in rows:
        key = (r["Dispatch_Id"], r["Counter_Name"])
        tot[key] = tot.get(key, 0.0) + float(r["Counter_Value"])
    disp = sorted({int(k[0]) for k in tot})
    from sift3d_amd import hip
    nl = hip.warp_tps_launches((N, N, N), 1024)
    last = [str(x) for x in disp[-nl:]]                # the measured call: its launches are the last ones
    s = {c: sum(tot.get((x, c), 0.0) for x in last) for c in ("SQ_INSTS_VALU", "SQ_ACTIVE_INST_VALU",
                                                                "SQ_WAVE_CYCLES")}
    vp = float(N) ** 3 * 1024
    waves = float(N) ** 3 / 64
    print("# rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES, m = 1024, %d launches" % len(last))
    for c, v in s.items():
        print("%-20s %.4e" % (c, v))
    print("VALU instructions per voxel-point (per lane): %.2f   (model: ~14 add/mul + ~15 sqrt)"
          % (s["SQ_INSTS_VALU"] / (waves * 1024) * 1.0))
    print("VALU active / wave cycles: %.3f" % (s["SQ_ACTIVE_INST_VALU"] / max(s["SQ_WAVE_CYCLES"], 1.0)))
    _ = vp


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--report")
    a = ap.parse_args()
    if a.report:
        report(a.report)
    else:
        _require_built()
        launches() if a.launches else run()
