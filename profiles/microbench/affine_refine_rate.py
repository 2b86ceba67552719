#!/usr/bin/env python3
"""Time per pass of the affine normal equations (sift3d_hip_affine_normal_eqs: the MSD; and
sift3d_hip_affine_ncc_normal_eqs: the fit under a linear intensity map) at 512^3 and 256^3 beside the similarity pass
(sift3d_hip_similarity_affine, B = 64, LINEAR) on the same volumes and transform, in one run.

Both passes walk the fixed grid and gather the moving volume through the same affine (a rotation of 5 degrees about
(1, 2, 3) through the centre): 8 B read per voxel, nothing written.  The similarity pass commits a histogram and six
double sums; the normal equations add 73 double sums, a few hundred f64 operations per voxel, so they are bound by
f64 VALU issue and registers (profiles/microbench/f64_rate_mi355x.txt: about 4.5 cycles per f64 wave instruction
per SIMD), not by HBM.  Volumes: the lattice with a noise floor of similarity_rate.py.

Times are HIP events around `reps` back-to-back calls, per call, the minimum of 3 trials after a warm-up.

    python3 profiles/microbench/affine_refine_rate.py [--label TEXT] > OUT.txt

SIFT3D_AMD_LIB selects another build of the library: one made with `make AFFDEF=-DSIFT3D_AFFINE_REFINE_NAIVE` times
the direct formulation (72 accumulators updated per voxel) instead of the factored one (tile sums over x, folded
once per tile); one made with `make AFFDEF=-DSIFT3D_AFFINE_NCC_ONE_KERNEL` times the NCC pass as one kernel at one wave
per SIMD instead of two kernels at two and three (H, v, S_mm and the count; then u, w and the other moments).
Registers and occupancy are the compiler's (`hipcc -Rpass-analysis=kernel-resource-usage`); pass
them in --label to keep them with the numbers."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from similarity_rate import _require_built, _rot, _time  # noqa: E402

PEAK_BPS = 8.0e12


def _volumes(n):
    import torch
    from sift3d_amd import hip
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    base = torch.empty((n, n, n), device="cuda")
    hip.synth_lattice(base, 0, 11)
    scale = float(base.abs().max())
    F = base / scale + 0.05 * torch.randn(base.shape, generator=g, device="cuda")
    M = base / scale + 0.05 * torch.randn(base.shape, generator=g, device="cuda")
    return F.contiguous(), M.contiguous()


def run(label, reps):
    import torch
    from sift3d_amd import hip
    print("# affine normal equations against the similarity pass, float32, LINEAR, MI355X (gfx950)%s"
          % (label and "; " + label))
    print("# HIP events around %d back-to-back calls, per call, min of 3 trials [spread]; model bytes 8 B / voxel "
          "against 8 TB/s" % reps)
    print("%-6s %-22s %26s %13s %8s %8s" % ("size", "call", "ms", "/ similarity", "GB/s", "of peak"))
    for n in (512, 256):
        F, M = _volumes(n)
        c = np.full(3, (n - 1) / 2.0)
        R = _rot((1.0, 2.0, 3.0), 5.0)
        A = np.hstack([R, (c - R @ c)[:, None]])
        lo, hi = float(min(F.min(), M.min())), float(max(F.max(), M.max()))
        hist = torch.empty((64, 64), dtype=torch.int64, device="cuda")
        swork = torch.empty(hip.SIMILARITY_GRID * 56, dtype=torch.uint8, device="cuda")
        rec = torch.empty(hip.AFFINE_NORMAL_BYTES // 8, dtype=torch.int64, device="cuda")
        work = torch.empty(hip.affine_normal_work_bytes(), dtype=torch.uint8, device="cuda")
        s = _time(lambda: hip.similarity(F, M, A, 64, (lo, hi), (lo, hi), "linear", hist, swork), reps)
        a = _time(lambda: hip.affine_normal_equations(F, M, A, rec, work, raw=True), reps)
        nrec = torch.empty(hip.AFFINE_NCC_BYTES // 8, dtype=torch.int64, device="cuda")
        nwork = torch.empty(hip.affine_ncc_normal_work_bytes(), dtype=torch.uint8, device="cuda")
        cn = _time(lambda: hip.affine_ncc_normal_equations(F, M, A, nrec, nwork, raw=True), reps)
        nbytes = 8.0 * float(n) ** 3
        for name, t, rel in (("similarity B=64", s, "-"), ("affine_normal_eqs", a, "%.3f" % (min(a) / min(s))),
                             ("affine_ncc_normal_eqs", cn, "%.3f" % (min(cn) / min(s)))):
            print("%-6s %-22s %8.4f [%.4f-%.4f] %13s %8.0f %8.3f" % (
                "%d^3" % n, name, min(t), min(t), max(t), rel, nbytes / min(t) / 1e6,
                nbytes / min(t) / 1e-3 / PEAK_BPS))
        count, see, _, H = hip.affine_normal_record(rec)
        scount, sums = hip.similarity_stats(hip.similarity(F, M, A, 64, (lo, hi), (lo, hi), "linear", hist, swork)[1])
        assert count == scount > 0 and abs(see - sums[5]) <= 1e-9 * see and np.array_equal(H, H.T)
        ncc = hip.affine_ncc_record(nrec)
        assert int(ncc["n"]) == count and np.array_equal(ncc["H"], H) and abs(ncc["S_ff"] - sums[2]) <= 1e-9 * sums[2]
        print("# %d^3: %d of %d voxels counted; msd %.6f; ncc pass / msd pass %.3f"
              % (n, count, n ** 3, see / count, min(cn) / min(a)))
        del F, M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    _require_built()
    run(a.label, a.reps)


if __name__ == "__main__":
    main()
