#!/usr/bin/env python3
"""Rates of the displacement-field kernels (sift3d_warp.hip) at 512^3, against the targets of DESIGN.md §3.4.2:

    affine field                        sift3d_hip_affine_field    12 B/voxel written
    TPS field, m = 1024                 sift3d_hip_tps_field       VALU, timed beside sift3d_hip_warp_tps
    warp_field, linear, nc = 1 and 12   sift3d_hip_warp_field      field of the oblique rotation of warp_rate.py
    jacobian_det, det written           sift3d_hip_jacobian_det    12 B/voxel read, 4 B written

    python3 profiles/microbench/field_rate.py > profiles/microbench/field_rate_mi355x.txt

Device events around `reps` back-to-back calls, per call, min of 3 trials after one warm-up; one process, the
device to itself.  Algorithmic bytes / time against the 8 TB/s HBM peak.  --only-jacobian times the Jacobian alone
(for comparing builds of the library through SIFT3D_AMD_LIB).

Counters, one rocprofv3 run per group (no tracing in the same run; FETCH_SIZE and WRITE_SIZE do not fit one run), each over --launches (every case: one
warm-up call, then 3 calls), then a report that needs no GPU:

    for g in "FETCH_SIZE" "WRITE_SIZE" "TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum" \
             "SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY" "SQ_INSTS_VALU SQ_ACTIVE_INST_VALU"; do
        rocprofv3 --pmc $g --output-format csv -d OUT/pmc_$n -o run -- python3 profiles/microbench/field_rate.py --launches
    done
    python3 profiles/microbench/field_rate.py --report OUT >> profiles/microbench/field_rate_mi355x.txt"""
import argparse
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N = 512
HBM = 8e12


def _require_built():
    lib = os.environ.get("SIFT3D_AMD_LIB") or os.path.join(ROOT, "sift3d_amd", "libsift3d_amd.so")
    if not os.path.exists(lib):
        sys.exit("%s is missing -- build first: python3 -c \"from sift3d_amd import _native; "
                 "_native.build()\"" % lib)


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


def _oblique():
    """warp_rate.py's oblique_s0.8: a rotation about (1, 2, 3) by 23 degrees, scaled by 0.8, about the centre"""
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    t = np.deg2rad(23.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    M = 0.8 * (np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K))
    c = np.full(3, (N - 1) / 2.0)
    return np.hstack([M, (c - M @ c)[:, None]])


def _tps(m, seed=1):
    """tps_rate.py's spline: m points over the grid, weights that move samples by ~2 voxels, a slight rotation"""
    from sift3d_amd import api
    rng = np.random.default_rng(seed)
    ctrl = rng.uniform(0, N - 1, (m, 3))
    w = rng.normal(0, 1, (m, 3))
    w -= w.mean(0)
    w *= 2.0 / (np.sqrt(m) * N / 4)
    c = np.full(3, (N - 1) / 2.0)
    t = np.deg2rad(5.0)
    R = np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]])
    return api.TPS(ctrl, w, np.hstack([R, (c - R @ c)[:, None]]))


def run():
    import torch
    from sift3d_amd import hip
    vox = float(N) ** 3
    A = _oblique()
    field = torch.empty((3, N, N, N), device="cuda")
    src = torch.rand((N, N, N), device="cuda")
    dst = torch.empty_like(src)
    print("# displacement fields, float32 %d^3, MI355X (gfx950); HIP events around back-to-back calls, per call, "
          "min of 3 trials after one warm-up" % N)
    print("%-34s %10s %10s %9s %9s" % ("call", "ms", "target ms", "alg GB", "frac 8TB/s"))

    def line(name, ms, target, nbytes):
        print("%-34s %10.4f %10s %9.3f %9.3f" % (name, ms, target, nbytes / 1e9,
                                                 (nbytes / HBM * 1e3) / ms if nbytes else 0.0))

    line("affine_field", _ms(lambda: hip.affine_field(field, A), 20), "0.4", 12 * vox)
    warp_ms = _ms(lambda: hip.warp_affine(src, dst, A), 20)
    line("warp_affine (for comparison)", warp_ms, "-", 8 * vox)
    line("warp_field linear nc=1", _ms(lambda: hip.warp_field(src, dst, field, "linear"), 20), "1.0", 20 * vox)
    line("warp_field nearest nc=1", _ms(lambda: hip.warp_field(src, dst, field, "nearest"), 20), "-", 20 * vox)
    src12 = torch.rand((12, N, N, N), device="cuda")
    dst12 = torch.empty_like(src12)
    line("warp_field linear nc=12", _ms(lambda: hip.warp_field(src12, dst12, field, "linear"), 5), "4.0", 108 * vox)
    del src12, dst12
    det = torch.empty((N, N, N), device="cuda")
    stats = torch.empty(2, dtype=torch.int64, device="cuda")
    L, st = hip.lib(), hip.current_stream()

    def jac(d):                                   # the C entry itself: hip.jacobian_det also reads the stats back
        assert L.sift3d_hip_jacobian_det(field.data_ptr(), N, N, N, d, stats.data_ptr(), st) == 0
    line("jacobian_det, det written", _ms(lambda: jac(det.data_ptr()), 20), "0.5", 16 * vox)
    line("jacobian_det, stats only", _ms(lambda: jac(None), 20), "-", 12 * vox)
    tps = _tps(1024)
    tf = _ms(lambda: hip.tps_field(field, tps), 1)
    tw = _ms(lambda: hip.warp_tps(src, dst, tps), 1)
    line("tps_field m=1024", tf, "%.1f" % (1.05 * tw), 0)
    line("warp_tps m=1024 (same run)", tw, "-", 0)
    print("# tps_field / warp_tps = %.3f (target <= 1.05); %d launches each"
          % (tf / tw, hip.tps_field_launches((N, N, N), 1024)))


CASES = [("affine_field", "k_affine_field"), ("warp_field nc=1", "k_warp_field"),
         ("warp_field nc=12", "k_warp_field"), ("jacobian_det det", "k_jacobian_det")]


def launches():
    """every case of CASES in order: one warm-up call, then 3 calls"""
    import torch
    from sift3d_amd import hip
    A = _oblique()
    field = torch.empty((3, N, N, N), device="cuda")
    src = torch.rand((N, N, N), device="cuda")
    dst = torch.empty_like(src)
    src12 = torch.rand((12, N, N, N), device="cuda")
    dst12 = torch.empty_like(src12)
    det = torch.empty((N, N, N), device="cuda")
    stats = torch.empty(2, dtype=torch.int64, device="cuda")
    L, st = hip.lib(), hip.current_stream()
    calls = [lambda: hip.affine_field(field, A), lambda: hip.warp_field(src, dst, field, "linear"),
             lambda: hip.warp_field(src12, dst12, field, "linear"),
             lambda: L.sift3d_hip_jacobian_det(field.data_ptr(), N, N, N, det.data_ptr(), stats.data_ptr(), st)]
    for fn in calls:
        for _ in range(4):
            fn()
        torch.cuda.synchronize()


def report(d):
    """per case: the mean of its last 3 dispatches of every counter collected under d"""
    rows = []
    for f in sorted(glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    by = {}                                           # (counter, kernel) -> {dispatch: value}
    for r in rows:
        k = next((kn for _, kn in CASES if kn in r.get("Kernel_Name", "")), None)
        if k is None:
            continue
        v = by.setdefault((r["Counter_Name"], k), {})
        v[int(r["Dispatch_Id"])] = v.get(int(r["Dispatch_Id"]), 0.0) + float(r["Counter_Value"])
    val = {}
    for (cn, kn), disp in by.items():
        ids = sorted(disp)
        seen = 0
        for name, k in CASES:
            if k != kn:
                continue
            part = ids[4 * seen:4 * seen + 4][1:]
            seen += 1
            if part:
                val[(name, cn)] = sum(disp[i] for i in part) / len(part)

    def g(name, cn):
        return val.get((name, cn), float("nan"))
    vox = float(N) ** 3
    # WRITE_SIZE calibrated on k_affine_field, whose 12 B/voxel of writes are known exactly
    wcal = 12 * vox / g("affine_field", "WRITE_SIZE")
    print("# counters (rocprofv3 --pmc, one run per group, mean of 3 dispatches after a warm-up), 512^3")
    print("# WRITE_SIZE calibrated on affine_field's 12 B/voxel: %.1f bytes per unit; FETCH_SIZE in the same unit"
          % wcal)
    print("%-20s %9s %9s %8s %8s %8s %8s %8s %10s" % ("case", "read GB", "write GB", "L1 hit", "wait",
                                                         "issue-st", "active", "VALU/cyc", "VALU/vox"))
    for name, _ in CASES:
        wc = g(name, "SQ_WAVE_CYCLES")
        l1 = 1.0 - g(name, "TCP_TCC_READ_REQ_sum") / g(name, "TCP_TOTAL_CACHE_ACCESSES_sum")
        print("%-20s %9.3f %9.3f %8.3f %8.3f %8.3f %8.3f %8.3f %10.2f" % (
            name, g(name, "FETCH_SIZE") * wcal / 1e9, g(name, "WRITE_SIZE") * wcal / 1e9, l1,
            g(name, "SQ_WAIT_ANY") / wc, g(name, "SQ_WAIT_INST_ANY") / wc, g(name, "SQ_ACTIVE_INST_ANY") / wc,
            g(name, "SQ_ACTIVE_INST_VALU") / wc, g(name, "SQ_INSTS_VALU") / (vox / 64)))
    print("# wait / issue-st / active: shares of SQ_WAVE_CYCLES waiting on memory or a barrier, stalled at issue, "
          "issuing; VALU/cyc: SQ_ACTIVE_INST_VALU / SQ_WAVE_CYCLES; VALU/vox: VALU instructions per wave-voxel "
          "(SQ_INSTS_VALU / (voxels / 64))")


def only_jacobian():
    import torch
    from sift3d_amd import hip
    field = torch.empty((3, N, N, N), device="cuda")
    hip.affine_field(field, _oblique())
    det = torch.empty((N, N, N), device="cuda")
    stats = torch.empty(2, dtype=torch.int64, device="cuda")
    L, st = hip.lib(), hip.current_stream()
    for name, d in (("jacobian_det, det written", det.data_ptr()), ("jacobian_det, stats only", None)):
        ms = _ms(lambda: L.sift3d_hip_jacobian_det(field.data_ptr(), N, N, N, d, stats.data_ptr(), st), 20)
        print("%-34s %10.4f ms   %.3f of 8 TB/s" % (name, ms, ((16 if d else 12) * N ** 3 / HBM * 1e3) / ms))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--only-jacobian", action="store_true")
    ap.add_argument("--report")
    a = ap.parse_args()
    if a.report:
        report(a.report)
    else:
        _require_built()
        launches() if a.launches else only_jacobian() if a.only_jacobian else run()
