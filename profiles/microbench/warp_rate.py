#!/usr/bin/env python3
"""Rate of the affine resampling kernel (sift3d_hip_warp_affine) at 512^3 -> 512^3.

Six cases: linear mode for the identity, a sub-voxel translation, 30-degree rotations about z and
about x, an oblique rotation with scale 0.8; nearest mode for the oblique map.  The algorithmic
traffic is 8 B per output voxel (one read of the source, one write), 1.07 GB per call; its share of
the 8 TB/s HBM peak is reported against device-event time and against kernel time.

    python3 profiles/microbench/warp_rate.py --events OUT/events.json
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/ktrace -o run -- \\
        python3 profiles/microbench/warp_rate.py --launches
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d OUT/pmc_fetch -o run -- \\
        python3 profiles/microbench/warp_rate.py --launches --reps 3
    rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum --output-format csv -d OUT/pmc_tcc -o run -- \\
        python3 profiles/microbench/warp_rate.py --launches --reps 3
    rocprofv3 --pmc TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum --output-format csv -d OUT/pmc_tcp -o run -- \\
        python3 profiles/microbench/warp_rate.py --launches --reps 3
    rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY --output-format csv \
        -d OUT/pmc_wave -o run -- python3 profiles/microbench/warp_rate.py --launches --reps 3
    python3 profiles/microbench/warp_rate.py --report OUT > profiles/microbench/warp_rate_mi355x.txt

--launches issues every case `reps` times in order on one stream (after one warm-up launch of
each), so the kernel trace and the counter rows are assigned to cases by dispatch order.  --report
needs no GPU."""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N = 512
PEAK_BPS = 8.0e12
ALG_BYTES = 8.0 * N ** 3


def _require_built():
    """These entry points run under rocprofv3, whose preloaded library has already initialised the GPU:
    building from here (a fork + exec of make) is not allowed on this pool.  Build first."""
    lib = os.environ.get("SIFT3D_AMD_LIB") or os.path.join(ROOT, "sift3d_amd", "libsift3d_amd.so")
    if not os.path.exists(lib):
        sys.exit("%s is missing -- build first: python3 -c \"from sift3d_amd import _native; "
                 "_native.build()\"" % lib)


def _rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def _about_center(M):
    c = np.full(3, (N - 1) / 2.0)
    return np.hstack([M, (c - M @ c)[:, None]])


def cases():
    oblique = _about_center(0.8 * _rot((1.0, 2.0, 3.0), 35.0))
    return [
        ("identity", "linear", np.hstack([np.eye(3), np.zeros((3, 1))])),
        ("translate(3.5,-2.25,1.75)", "linear", np.hstack([np.eye(3), np.array([[3.5], [-2.25], [1.75]])])),
        ("rot_z30", "linear", _about_center(_rot((0, 0, 1), 30.0))),
        ("rot_x30", "linear", _about_center(_rot((1, 0, 0), 30.0))),
        ("oblique_s0.8", "linear", oblique),
        ("oblique_s0.8", "nearest", oblique),
    ]


def _volumes():
    import torch
    from sift3d_amd import hip
    src = torch.empty((N, N, N), device="cuda")
    hip.synth_lattice(src, 0, 11)
    return src, torch.empty_like(src)


def events(path, reps=50, trials=3):
    import torch
    from sift3d_amd import hip
    src, dst = _volumes()
    out = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, interp, A in cases():
        for _ in range(5):
            hip.warp_affine(src, dst, A, interp)
        ms = []
        for _ in range(trials):
            e0.record()
            for _ in range(reps):
                hip.warp_affine(src, dst, A, interp)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / reps)
        out.append({"case": name, "interp": interp, "event_ms": ms})
        print("%-28s %-8s event %.4f ms (trials %s)" % (name, interp, min(ms), " ".join("%.4f" % m for m in ms)))
    with open(path, "w") as f:
        json.dump({"n": N, "reps": reps, "trials": trials, "cases": out}, f, indent=1)


def launches(reps):
    import torch
    from sift3d_amd import hip
    src, dst = _volumes()
    cs = cases()
    for _, interp, A in cs:                            # warm-up: one launch of each, in case order
        hip.warp_affine(src, dst, A, interp)
    for _, interp, A in cs:
        for _ in range(reps):
            hip.warp_affine(src, dst, A, interp)
    torch.cuda.synchronize()


def _rows(d, suffix):
    files = sorted(glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True))
    rows = []
    for fn in files:
        with open(fn) as f:
            rows += list(csv.DictReader(f))
    return rows


def _per_case(rows, reps, key):
    """rows of the warp kernel in dispatch order -> per case (skipping the warm-up launches)"""
    rows = [r for r in rows if "k_warp_affine" in r.get("Kernel_Name", "")]
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or 0))
    nc = len(cases())
    if len(rows) != nc * (reps + 1):
        return None
    timed = rows[nc:]
    return [[key(r) for r in timed[i * reps:(i + 1) * reps]] for i in range(nc)]


def _pmc(d, names, reps=3):
    rows = _rows(d, "counter_collection.csv")
    if not rows:
        return None
    # one row per (dispatch, counter): regroup by dispatch
    by = {}
    for r in rows:
        if "k_warp_affine" not in r.get("Kernel_Name", ""):
            continue
        k = int(r["Dispatch_Id"])
        by.setdefault(k, {"Kernel_Name": r["Kernel_Name"], "Dispatch_Id": k})[r["Counter_Name"]] = float(
            r["Counter_Value"])
    per = _per_case(list(by.values()), reps, lambda r: r)
    if per is None:
        return None
    return [{n: float(np.mean([r.get(n, np.nan) for r in rs])) for n in names} for rs in per]


def report(d):
    ev = json.load(open(os.path.join(d, "events.json")))
    kt = _rows(os.path.join(d, "ktrace"), "kernel_trace.csv")
    kreps = 10
    kms = _per_case(kt, kreps, lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    fetch = _pmc(os.path.join(d, "pmc_fetch"), ["FETCH_SIZE"])
    tcc = _pmc(os.path.join(d, "pmc_tcc"), ["TCC_HIT_sum", "TCC_MISS_sum"])
    tcp = _pmc(os.path.join(d, "pmc_tcp"), ["TCP_TOTAL_CACHE_ACCESSES_sum", "TCP_TCC_READ_REQ_sum"])
    wave = _pmc(os.path.join(d, "pmc_wave"), ["SQ_WAVE_CYCLES", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY",
                                              "SQ_ACTIVE_INST_ANY"])
    print("# sift3d_hip_warp_affine, %d^3 -> %d^3 float32, MI355X (gfx950)" % (N, N))
    print("# algorithmic bytes: 8 B / output voxel (one read, one write) = %.3f GB per call; "
          "share of the 8 TB/s HBM peak = %.3f ms / time" % (ALG_BYTES / 1e9, ALG_BYTES / PEAK_BPS * 1e3))
    print("# event: HIP events around %d back-to-back calls, per call (min of %d trials; spread in brackets)"
          % (ev["reps"], ev["trials"]))
    print("# kernel: rocprofv3 --kernel-trace, mean of %d dispatches per case (a run of its own)" % kreps)
    print("%-26s %-8s %20s %7s %10s %7s" % ("case", "interp", "event ms", "frac", "kernel ms", "frac"))
    for i, c in enumerate(ev["cases"]):
        e = c["event_ms"]
        k = float(np.mean(kms[i])) if kms else float("nan")
        print("%-26s %-8s %8.4f [%.4f-%.4f] %7.3f %10.4f %7.3f" % (
            c["case"], c["interp"], min(e), min(e), max(e), ALG_BYTES / PEAK_BPS * 1e3 / min(e),
            k, ALG_BYTES / PEAK_BPS * 1e3 / k))
    if kms is None:
        print("# (kernel trace missing or not in the expected dispatch order)")
    if fetch or tcc or tcp:
        print()
        print("# counters: rocprofv3 --pmc, one run per counter group, mean of 3 dispatches per case.")
        print("# 'read GB' ASSUMES that the identity case fetches its algorithmic %.1f MB from beyond L2 exactly once "
              "(not a known byte count: its tiles' 2-point stencil overlaps its neighbours'); the column is "
              "FETCH_SIZE x (that / identity's FETCH_SIZE), so only ratios between cases are measured." % (4.0 * N ** 3 / 1e6))
        cal = 4.0 * N ** 3 / fetch[0]["FETCH_SIZE"] if fetch else float("nan")     # bytes per FETCH_SIZE unit
        print("# calibration: %.1f bytes per FETCH_SIZE unit" % cal)
        print("%-26s %-8s %12s %10s %9s %9s" % ("case", "interp", "FETCH_SIZE", "read GB", "L2 hit", "L1 hit"))
        for i, c in enumerate(ev["cases"]):
            fs = fetch[i]["FETCH_SIZE"] if fetch else float("nan")
            l2 = tcc[i]["TCC_HIT_sum"] / (tcc[i]["TCC_HIT_sum"] + tcc[i]["TCC_MISS_sum"]) if tcc else float("nan")
            l1 = (1.0 - tcp[i]["TCP_TCC_READ_REQ_sum"] / tcp[i]["TCP_TOTAL_CACHE_ACCESSES_sum"]) if tcp else float("nan")
            print("%-26s %-8s %12.0f %10.3f %9.3f %9.3f" % (c["case"], c["interp"], fs, fs * cal / 1e9, l2, l1))

    if wave:
        print()
        print("# wave states (rocprofv3 --pmc, a run of its own): share of SQ_WAVE_CYCLES that waves spent waiting for")
        print("# memory / a barrier (SQ_WAIT_ANY), stalled at instruction issue (SQ_WAIT_INST_ANY: e.g. a vector-memory")
        print("# instruction the address unit cannot take yet) and issuing (SQ_ACTIVE_INST_ANY)")
        print("%-26s %-8s %9s %9s %9s" % ("case", "interp", "wait", "issue-st", "active"))
        for i, c in enumerate(ev["cases"]):
            w = wave[i]
            print("%-26s %-8s %9.3f %9.3f %9.3f" % (c["case"], c["interp"], w["SQ_WAIT_ANY"] / w["SQ_WAVE_CYCLES"],
                                                   w["SQ_WAIT_INST_ANY"] / w["SQ_WAVE_CYCLES"],
                                                   w["SQ_ACTIVE_INST_ANY"] / w["SQ_WAVE_CYCLES"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", metavar="JSON")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--report", metavar="DIR")
    a = ap.parse_args()
    if a.report:
        report(a.report)
        return
    _require_built()
    if a.events:
        events(a.events)
    elif a.launches:
        launches(a.reps)
    else:
        ap.error("one of --events, --launches, --report")


if __name__ == "__main__":
    main()
