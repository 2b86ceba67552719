#!/usr/bin/env python3
"""Time of the multi-channel force kernel k_ffd_force_channels (sift3d_hip_ffd_evaluate_channels) at nc = 1, 3 and 12
against two baselines in the same run: nc launches of the single-channel k_ffd_force (sift3d_hip_ffd_evaluate on each
channel in turn, what a caller had to do before), and the bytes model

    (12 + 24 + nc * (4 + gathered)) B / voxel at 8 TB/s,     gathered = 4:

the field read once (12 B), the force written once (24 B, three doubles), and per channel the fixed value (4 B) and the
moving volume, every voxel of which is taken to come from HBM once (4 B; the eight taps of neighbouring outputs overlap
and are served by L1 / L2).  nc launches of k_ffd_force move nc * (12 + 24 + 4 + 4) B / voxel by the same count.

The stacks are float32 noise; the lattice (spacing 8) is random with an amplitude of 1 voxel on top of a rotation of 5
degrees about (1, 2, 3) through the centre, as in ffd_mi_rate.py.  The kernels' own durations come from a kernel trace:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python3 profiles/microbench/ffd_channels_rate.py --launches
    python3 profiles/microbench/ffd_channels_rate.py --report DIR [--label TEXT] > OUT.txt

--launches issues, per size and nc, six rounds (the first is the warm-up) of one channels evaluation and nc
single-channel evaluations.  --report needs no GPU.  Another unroll factor of the channel sweep: build it beside the
library (`make -C sift3d_amd/csrc FFDDEF=-DFFD_CHANNELS_UNROLL=n` into a copy) and name it in SIFT3D_AMD_LIB.  Registers and occupancy are the compiler's
(`hipcc -Rpass-analysis=kernel-resource-usage`); pass them in --label to keep them with the numbers."""
import argparse
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from similarity_rate import _require_built, _rot  # noqa: E402

PEAK_BPS = 8.0e12
SPACING = (8, 8, 8)
CHANNELS = (1, 3, 12)
ROUNDS = 6
GATHERED = 4.0


def model_bytes(nc):
    return 12.0 + 24.0 + nc * (4.0 + GATHERED)


def launches(sizes):
    import torch
    from sift3d_amd import hip
    for n in sizes:
        c = np.full(3, (n - 1) / 2.0)
        R = _rot((1.0, 2.0, 3.0), 5.0)
        A = np.hstack([R, (c - R @ c)[:, None]])
        g = torch.Generator(device="cuda")
        g.manual_seed(3)
        lattice = torch.rand(hip.ffd_lattice_shape((n, n, n), SPACING), generator=g, device="cuda") * 2.0 - 1.0
        work = torch.empty(hip.lib().sift3d_amd_ffd_evaluate_work_bytes(n, n, n, *SPACING) // 4, dtype=torch.float32,
                           device="cuda")
        for nc in CHANNELS:
            F = torch.randn((nc, n, n, n), generator=g, device="cuda")
            M = torch.randn((nc, n, n, n), generator=g, device="cuda")
            for _ in range(ROUNDS):
                hip.ffd_evaluate_channels(F, M, lattice, SPACING, A, 0.005, work)
                for k in range(nc):
                    hip.ffd_evaluate(F[k], M[k], lattice, SPACING, A, 0.005, work)
            torch.cuda.synchronize()
            del F, M
        del lattice, work
    print("launches: sizes %s x nc %s x %d rounds of (1 channels evaluation, nc single-channel evaluations)"
          % (list(sizes), list(CHANNELS), ROUNDS))


def report(d, sizes, label):
    """the two force kernels' durations from a kernel trace of --launches, in the trace's order: per (size, nc) group
    ROUNDS launches of k_ffd_force_channels and ROUNDS * nc of k_ffd_force; the first round is dropped"""
    rows = []
    for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)):
        with open(f) as fh:
            rows += [r for r in csv.DictReader(fh)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    seq = []
    for r in rows:
        name = r["Kernel_Name"]
        if "k_ffd_force_channels" in name:
            kn = "channels"
        elif "k_ffd_force" in name:
            kn = "single"
        else:
            continue
        seq.append((kn, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6))
    want = sum(ROUNDS * (1 + nc) for nc in CHANNELS) * len(sizes)
    if len(seq) != want:
        sys.exit("%d force kernels in %s, expected %d for sizes %s" % (len(seq), d, want, list(sizes)))
    print("# k_ffd_force_channels against nc launches of k_ffd_force and against the bytes model, float32, LINEAR, "
          "MI355X (gfx950)%s" % (label and "; " + label))
    print("# the kernels' own durations (rocprofv3 --kernel-trace of --launches), ms, min of %d rounds [spread]; "
          "model: (36 + 8 nc) B / voxel at 8 TB/s" % (ROUNDS - 1))
    print("%-6s %-3s %28s %28s %9s %10s %9s" % ("size", "nc", "k_ffd_force_channels", "nc x k_ffd_force", "fused/nc x",
                                                "model ms", "/ model"))
    at = 0
    for n in sizes:
        for nc in CHANNELS:
            grp = seq[at:at + ROUNDS * (1 + nc)]
            at += ROUNDS * (1 + nc)
            fused, single = [], []
            for k in range(ROUNDS):
                rnd = grp[k * (1 + nc):(k + 1) * (1 + nc)]
                assert rnd[0][0] == "channels" and all(kn == "single" for kn, _ in rnd[1:]), rnd
                fused.append(rnd[0][1])
                single.append(sum(v for _, v in rnd[1:]))
            fused, single = fused[1:], single[1:]
            model = model_bytes(nc) * float(n) ** 3 / PEAK_BPS * 1e3
            print("%-6s %-3d %10.4f [%.4f-%.4f] %10.4f [%.4f-%.4f] %9.3f %10.4f %9.2f"
                  % ("%d^3" % n, nc, min(fused), min(fused), max(fused), min(single), min(single), max(single),
                     min(fused) / min(single), model, min(fused) / model))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--label", default="")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--report", default="")
    a = ap.parse_args()
    sizes = [int(v) for v in a.sizes.split(",")]
    if a.report:
        return report(a.report, sizes, a.label)
    _require_built()
    if not a.launches:
        sys.exit("--launches (under rocprofv3 --kernel-trace) or --report DIR")
    launches(sizes)


if __name__ == "__main__":
    main()
