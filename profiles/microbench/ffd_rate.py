#!/usr/bin/env python3
"""Time of the free-form deformation kernels at 512^3 and 256^3, spacing 8: the field export (sift3d_hip_ffd_field) and
one evaluation with gradient (sift3d_hip_ffd_evaluate: the field, the force pass, the three adjoint passes, the bending
energy and the gradient), beside k_warp_field (sift3d_hip_warp_field), k_similarity through a field
(sift3d_hip_similarity_field, B = 64) and k_affine_normal (sift3d_hip_affine_normal_eqs) on the same volumes in the
same run, as the yardsticks.

The lattice is random with amplitude 1.5 voxels, so that the gathers leave the regular pattern of the identity.  Model
bytes per voxel: the field export writes 12; an evaluation writes 12 (field) + 24 (force) and reads 12 + 8 (field,
F and M) + 24 (force, once), 80 in all; the yardsticks are 16 read + 4 written (warp), 20 read (similarity through a
field), 8 read (affine normal equations).

Times are HIP events around `reps` back-to-back calls, per call, the minimum of 3 trials after a warm-up.

    python3 profiles/microbench/ffd_rate.py [--label TEXT] > OUT.txt"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from affine_refine_rate import _volumes  # noqa: E402
from similarity_rate import _require_built, _time  # noqa: E402

PEAK_BPS = 8.0e12
SPACING = (8, 8, 8)


def run(label, reps):
    import torch
    from sift3d_amd import hip
    L = hip.lib()
    print("# free-form deformation kernels against their yardsticks, float32, LINEAR, spacing 8, MI355X (gfx950)%s"
          % (label and "; " + label))
    print("# HIP events around %d back-to-back calls, per call, min of 3 trials [spread]; model bytes against 8 TB/s"
          % reps)
    print("%-6s %-22s %26s %9s %8s %8s" % ("size", "call", "ms", "B/voxel", "GB/s", "of peak"))
    for n in (512, 256):
        F, M = _volumes(n)
        shape = hip.ffd_lattice_shape((n, n, n), SPACING)
        g = torch.Generator(device="cuda")
        g.manual_seed(3)
        lat = ((torch.rand(shape, generator=g, device="cuda") - 0.5) * 3.0).contiguous()
        field = torch.empty((3, n, n, n), dtype=torch.float32, device="cuda")
        fwork = torch.empty(L.sift3d_amd_ffd_field_work_bytes(*SPACING), dtype=torch.uint8, device="cuda")
        ework = torch.empty(L.sift3d_amd_ffd_evaluate_work_bytes(n, n, n, *SPACING), dtype=torch.uint8, device="cuda")
        warped = torch.empty_like(F)
        lo, hi = float(min(F.min(), M.min())), float(max(F.max(), M.max()))
        hist = torch.empty((64, 64), dtype=torch.int64, device="cuda")
        swork = torch.empty(hip.SIMILARITY_GRID * 56, dtype=torch.uint8, device="cuda")
        rec = torch.empty(hip.AFFINE_NORMAL_BYTES // 8, dtype=torch.int64, device="cuda")
        awork = torch.empty(hip.affine_normal_work_bytes(), dtype=torch.uint8, device="cuda")
        A = np.eye(3, 4)
        rows = [
            ("ffd_field", 12, lambda: hip.ffd_field(lat, SPACING, field, None, fwork)),
            ("ffd_evaluate", 80, lambda: hip.ffd_evaluate(F, M, lat, SPACING, None, 0.005, ework)),
            ("warp_field", 20, lambda: hip.warp_field(M, warped, field, "linear", 0.0)),
            ("similarity_field B=64", 20, lambda: hip.similarity(F, M, field, 64, (lo, hi), (lo, hi), "linear", hist,
                                                                 swork)),
            ("affine_normal_eqs", 8, lambda: hip.affine_normal_equations(F, M, A, rec, awork, raw=True)),
        ]
        times = {}
        for name, bpv, fn in rows:
            t = _time(fn, reps)
            times[name] = min(t)
            nbytes = float(bpv) * float(n) ** 3
            print("%-6s %-22s %8.4f [%.4f-%.4f] %9d %8.0f %8.3f" % (
                "%d^3" % n, name, min(t), min(t), max(t), bpv, nbytes / min(t) / 1e6,
                nbytes / min(t) / 1e-3 / PEAK_BPS))
        record, _, _ = hip.ffd_evaluate(F, M, lat, SPACING, None, 0.005, ework)
        count, see, R, gmax, _, _ = hip.ffd_record(record, shape)
        assert count > 0 and np.isfinite(see) and R > 0 and gmax > 0
        print("# %d^3: %d of %d voxels counted; msd %.6f; R %.6g; evaluation / (affine_normal_eqs + warp_field) = %.2f"
              % (n, count, n ** 3, see / count, R,
                 times["ffd_evaluate"] / (times["affine_normal_eqs"] + times["warp_field"])))
        del F, M, field, ework


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    _require_built()
    run(a.label, a.reps)


if __name__ == "__main__":
    main()
