#!/usr/bin/env python3
"""Time of the Jacobian penalty's two kernels at 512^3 beside the kernels they are measured against, in one process on
one field: the value pass (k_jp_value), the gradient pass (k_jp_grad), k_jacobian_det (the walk the value pass copies)
and k_ffd_force (the yardstick: the image force of an FFD evaluation), and the cost of one MSD evaluation without and
with the penalty.

The field is the export of a lattice (spacing 8, random, amplitude 1 voxel) added to a rotation of 5 degrees about
(1, 2, 3) through the centre, as in ffd_mi_rate.py; the volumes are affine_refine_rate.py's.  A penalised MSD evaluation
launches what sift3d_hip_ffd_evaluate launches, then what sift3d_hip_ffd_jacobian_gradient launches (the value pass with
a(p), its finish, the gradient pass and the three adjoint passes) on the same field, and a combine with one more operand:
the two entries back to back are that evaluation but for the weight tables' second upload.

Algorithmic bytes per voxel: k_jp_value 12 read (+ 8 written with the gradient), k_jp_grad 12 + 8 read and 24 written,
k_jacobian_det 12 read (statistics only), k_ffd_force 20 read and 24 written; each over 8 TB/s is the floor printed.

Times are HIP events around `reps` back-to-back calls, per call, the minimum of 3 trials after a warm-up, the calls
taking turns trial by trial.  The kernels' own durations come from a kernel trace of a run of their own:

    python3 profiles/microbench/jacobian_penalty_rate.py [--label TEXT] > OUT.txt
    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python3 profiles/microbench/jacobian_penalty_rate.py \\
        --launches
    python3 profiles/microbench/jacobian_penalty_rate.py --report DIR >> OUT.txt

Each of the two GPU commands is one process and is meant to run under a `timeout` of its own (a minute each is ample
at 512^3).  --report needs no GPU.  Registers and occupancy are the compiler's (`hipcc
-Rpass-analysis=kernel-resource-usage`); pass them in --label to keep them with the numbers."""
import argparse
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from affine_refine_rate import _volumes  # noqa: E402
from ffd_mi_rate import _alternate  # noqa: E402
from similarity_rate import _require_built, _rot  # noqa: E402

PEAK_BPS = 8.0e12
SPACING = (8, 8, 8)
# kernel: (name in the trace, algorithmic bytes per voxel)
KERNELS = (("k_jp_value<false>", 12.0), ("k_jp_value<true>", 20.0), ("k_jp_grad", 44.0), ("k_jacobian_det", 12.0),
           ("k_ffd_force", 44.0))


def _setup(n):
    import torch
    from sift3d_amd import hip
    F, M = _volumes(n)
    c = np.full(3, (n - 1) / 2.0)
    R = _rot((1.0, 2.0, 3.0), 5.0)
    A = np.hstack([R, (c - R @ c)[:, None]])
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    lattice = torch.rand(hip.ffd_lattice_shape((n, n, n), SPACING), generator=g, device="cuda") * 2.0 - 1.0
    L = hip.lib()
    ework = torch.empty(L.sift3d_amd_ffd_evaluate_work_bytes(n, n, n, *SPACING), dtype=torch.uint8, device="cuda")
    _, _, field = hip.ffd_evaluate(F, M, lattice, SPACING, A, 0.005, ework)
    jwork = torch.empty(L.sift3d_amd_ffd_jacobian_gradient_work_bytes(n, n, n, *SPACING), dtype=torch.uint8,
                        device="cuda")
    pwork = torch.empty(L.sift3d_amd_jacobian_penalty_work_bytes(n, n, n), dtype=torch.uint8, device="cuda")
    S = torch.empty((3, n, n, n), dtype=torch.float64, device="cuda")
    rec = torch.empty(4, dtype=torch.int64, device="cuda")
    ref = float(np.linalg.det(R))

    def penalty(grad):
        rc = L.sift3d_hip_jacobian_penalty(field.data_ptr(), n, n, n, ref, rec.data_ptr(),
                                           S.data_ptr() if grad else None, pwork.data_ptr(), hip.current_stream())
        assert rc == 0
    calls = [("jacobian_penalty, value", lambda: penalty(False)),
             ("jacobian_penalty, value + gradient", lambda: penalty(True)),
             ("jacobian_det, statistics", lambda: hip.jacobian_det(field)),
             ("ffd_evaluate (msd)", lambda: hip.ffd_evaluate(F, M, lattice, SPACING, A, 0.005, ework)),
             ("ffd_jacobian_gradient", lambda: hip.ffd_jacobian_gradient(field, SPACING, ref, jwork))]
    return calls, (rec, hip)


def run(label, reps, n):
    print("# the Jacobian penalty beside jacobian_det and the MSD evaluation, one field, float32, MI355X (gfx950)%s"
          % (label and "; " + label))
    print("# HIP events around %d back-to-back calls, per call, min of 3 alternating trials [spread]" % reps)
    calls, (rec, hip) = _setup(n)
    t = _alternate([fn for _, fn in calls], reps)
    for (name, _), v in zip(calls, t):
        print("%-6s %-36s %8.4f [%.4f-%.4f]" % ("%d^3" % n, name, min(v), min(v), max(v)))
    ev, jg = min(t[3]), min(t[4])
    print("%-6s %-36s %8.4f = %.3f x the evaluation without" % ("%d^3" % n, "msd evaluation with the penalty", ev + jg,
                                                                  (ev + jg) / ev))
    nonpos, total, rmin, rmax = hip.jacobian_penalty_record(rec)
    print("# the field: P %.6g, nonpos %d, r in [%.4g, %.4g]" % (total / float(n) ** 3, nonpos, rmin, rmax))


def launches(n):
    import torch
    calls, _ = _setup(n)
    for _ in range(6):                                                   # the first round is the warm-up
        for _, fn in calls:
            fn()
    torch.cuda.synchronize()
    print("launches: 1 setup evaluation, then 6 rounds of the five calls")


def report(d, n):
    """the kernels' own durations from a kernel trace of --launches: the last five of each"""
    rows = []
    for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)):
        with open(f) as fh:
            rows += [r for r in csv.DictReader(fh)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    t = {k: [] for k, _ in KERNELS}
    for r in rows:
        name = r["Kernel_Name"]
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
        if "k_jp_value" in name:
            with_a = "<true>" in name or "ILb1E" in name
            t["k_jp_value<true>" if with_a else "k_jp_value<false>"].append(ms)
        elif "k_jp_grad" in name:
            t["k_jp_grad"].append(ms)
        elif "k_jacobian_det" in name:
            t["k_jacobian_det"].append(ms)
        elif "k_ffd_force" in name:
            t["k_ffd_force"].append(ms)
    if not any(t.values()):
        sys.exit("no kernel of %s in %s" % ([k for k, _ in KERNELS], d))
    print("# the kernels' own durations (rocprofv3 --kernel-trace of --launches), ms, min of the last 5 [spread], their "
          "algorithmic bytes over 8 TB/s, and the quotient")
    for k, b in KERNELS:
        v = t[k][-5:]
        floor = b * float(n) ** 3 / PEAK_BPS * 1e3
        print("%-6s %-20s %8.4f [%.4f-%.4f] %5.0f B/voxel %8.4f ms %6.2f x" % ("%d^3" % n, k, min(v), min(v), max(v), b,
                                                                               floor, min(v) / floor))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--label", default="")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--report", default="")
    a = ap.parse_args()
    if a.report:
        return report(a.report, a.size)
    _require_built()
    if a.launches:
        return launches(a.size)
    run(a.label, a.reps, a.size)


if __name__ == "__main__":
    main()
