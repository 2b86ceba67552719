#!/usr/bin/env python3
"""Rate of the dense descriptor image (sift3d_amd_dense_descriptors_device) at 512^3.

Three cases: isotropic units with sigma 1.6 (11 taps: x pass + the fused y+z kernel per channel),
units (0.8, 0.8, 2.0) with sigma 1.6 (separate x, y, z passes) and isotropic sigma 11 (67 taps: the
chunked literal FIR, separate passes).  Algorithmic bytes per voxel: bin 4 read + 48 written; per
channel an x pass 8 and a fused y+z pass 8 (or three passes, 24); normalize 96 -- 340 B / voxel
(45.6 GB per call) with the fused kernel, 436 B without.  Their share of the 8 TB/s HBM peak is
reported against device-event time and, per stage, against kernel time.

    python3 profiles/microbench/dense_rate.py --events OUT/events.json
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/ktrace -o run -- \\
        python3 profiles/microbench/dense_rate.py --launches
    python3 profiles/microbench/dense_rate.py --report OUT > profiles/microbench/dense_rate_mi355x.txt

--launches issues every case `reps` times in order on one stream (after one warm-up call of each);
the kernel trace is cut into calls at each k_dense_bin dispatch.  --report needs no GPU."""
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
TARGET_MS = 12.0


def _require_built():
    """These entry points run under rocprofv3, whose preloaded library has already initialised the GPU:
    they must not build (a fork + exec of make from that process).  Build first."""
    lib = os.environ.get("SIFT3D_AMD_LIB") or os.path.join(ROOT, "sift3d_amd", "libsift3d_amd.so")
    if not os.path.exists(lib):
        sys.exit("%s is missing -- build first: python3 -c \"from sift3d_amd import _native; "
                 "_native.build()\"" % lib)


def cases():
    # (name, units, sigma, algorithmic bytes per voxel)
    return [
        ("iso_s1.6", (1.0, 1.0, 1.0), 1.6, 52 + 12 * 16 + 96),
        ("aniso(0.8,0.8,2)_s1.6", (0.8, 0.8, 2.0), 1.6, 52 + 12 * 24 + 96),
        ("iso_s11", (1.0, 1.0, 1.0), 11.0, 52 + 12 * 24 + 96),
    ]


def _buffers():
    import torch
    from sift3d_amd import hip
    src = torch.empty((N, N, N), device="cuda")
    hip.synth_lattice(src, 0, 11)
    out = torch.empty((12, N, N, N), device="cuda")
    work = torch.empty(hip.lib().sift3d_amd_dense_work_floats(N, N, N), device="cuda")
    return src, out, work


def events(path, reps=10, trials=3):
    import torch
    from sift3d_amd import hip
    src, out, work = _buffers()
    res = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, units, sigma, _ in cases():
        for _ in range(2):
            hip.dense_descriptors(src, out, sigma, units, work)
        ms = []
        for _ in range(trials):
            e0.record()
            for _ in range(reps):
                hip.dense_descriptors(src, out, sigma, units, work)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / reps)
        res.append({"case": name, "event_ms": ms})
        print("%-24s event %.3f ms (trials %s)" % (name, min(ms), " ".join("%.3f" % m for m in ms)))
    with open(path, "w") as f:
        json.dump({"n": N, "reps": reps, "trials": trials, "cases": res}, f, indent=1)


def launches(reps):
    import torch
    from sift3d_amd import hip
    src, out, work = _buffers()
    for _, units, sigma, _ in cases():
        for _ in range(reps + 1):                      # the first call of each case is its warm-up
            hip.dense_descriptors(src, out, sigma, units, work)
    torch.cuda.synchronize()


def _rows(d, suffix):
    files = sorted(glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True))
    rows = []
    for fn in files:
        with open(fn) as f:
            rows += list(csv.DictReader(f))
    return rows


def _calls(rows, reps):
    """kernel rows in dispatch order -> per case, per timed call: {stage: ms}, span ms, blur kernel names"""
    rows = sorted(rows, key=lambda r: int(r.get("Dispatch_Id") or 0))
    calls = []
    for r in rows:
        name = r.get("Kernel_Name", "")
        if "k_dense_bin" in name:
            calls.append([])
        if calls:
            calls[-1].append(r)
    nc = len(cases())
    if len(calls) != nc * (reps + 1):
        return None
    per = []
    for i in range(nc):
        out = []
        for c in calls[i * (reps + 1) + 1:(i + 1) * (reps + 1)]:
            t = {"bin": 0.0, "blur": 0.0, "normalize": 0.0}
            names = set()
            for r in c:
                ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
                k = r["Kernel_Name"]
                if "k_dense_bin" in k:
                    t["bin"] += ms
                elif "k_dense_normalize" in k:
                    t["normalize"] += ms
                else:
                    t["blur"] += ms
                    names.add(k.split("(")[0].replace("void ", ""))
            span = (int(c[-1]["End_Timestamp"]) - int(c[0]["Start_Timestamp"])) * 1e-6
            out.append((t, span, names))
        per.append(out)
    return per


def report(d):
    ev = json.load(open(os.path.join(d, "events.json")))
    kreps = 5
    per = _calls(_rows(os.path.join(d, "ktrace"), "kernel_trace.csv"), kreps)
    print("# sift3d_amd_dense_descriptors_device, %d^3 float32 -> 12 x %d^3, MI355X (gfx950)" % (N, N))
    print("# algorithmic bytes / voxel: bin 52, blur 16 (x + fused y+z) or 24 (x, y, z) per channel x 12, "
          "normalize 96; share of the 8 TB/s HBM peak = (bytes / 8 TB/s) / time")
    print("# event: HIP events around %d back-to-back calls, per call (min of %d trials; spread in brackets); "
          "target %.0f ms" % (ev["reps"], ev["trials"], TARGET_MS))
    print("%-24s %6s %8s %22s %7s" % ("case", "B/vox", "GB", "event ms", "frac"))
    for c, (name, _, _, bpv) in zip(ev["cases"], cases()):
        e = c["event_ms"]
        gb = bpv * float(N) ** 3 / 1e9
        print("%-24s %6d %8.2f %9.3f [%.3f-%.3f] %7.3f" % (name, bpv, gb, min(e), min(e), max(e),
                                                         gb * 1e9 / PEAK_BPS * 1e3 / min(e)))
    print()
    if per is None:
        print("# (kernel trace missing or not in the expected dispatch order)")
        return
    print("# kernel: rocprofv3 --kernel-trace (a run of its own), mean of %d calls per case; 'span' = first "
          "kernel start to last kernel end" % kreps)
    print("%-24s %9s %7s %9s %7s %9s %7s %9s %9s" % ("case", "bin ms", "frac", "blur ms", "frac", "norm ms", "frac",
                                                  "sum ms", "span ms"))
    for (name, _, _, bpv), calls in zip(cases(), per):
        blur_b = bpv - 52 - 96
        m = {k: float(np.mean([t[k] for t, _, _ in calls])) for k in ("bin", "blur", "normalize")}
        span = float(np.mean([s for _, s, _ in calls]))
        f = lambda b, ms: b * float(N) ** 3 / PEAK_BPS * 1e3 / ms
        print("%-24s %9.3f %7.3f %9.3f %7.3f %9.3f %7.3f %9.3f %9.3f" % (
            name, m["bin"], f(52, m["bin"]), m["blur"], f(blur_b, m["blur"]), m["normalize"],
            f(96, m["normalize"]), sum(m.values()), span))
    for (name, _, _, _), calls in zip(cases(), per):
        print("# %s blur kernels: %s" % (name, ", ".join(sorted(calls[0][2]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", metavar="JSON")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
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
