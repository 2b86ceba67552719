#!/usr/bin/env python3
"""Rate of the rotation-invariant dense descriptor image (sift3d_amd_dense_descriptors_rotate_device).

Cases: 256^3 and 512^3 isotropic at sigma 1.6, 512^3 with units (0.8, 0.8, 2.0) at sigma 1.6,
256^3 isotropic at sigma 3.2 and 128^3 at sigma 5.5 (a window near the accepted limit).  Per case the
device-event time of the orientation stage (R2,
sift3d_hip_dense_orient), the binning stage (R3, sift3d_hip_dense_rotate_bin) and the normalisation,
each the minimum over `reps` back-to-back calls after one warm-up call, and the rate in (voxel, window
voxel) pairs per second.  The window voxel count comes from the same sphere test as the kernels.

    python3 profiles/microbench/dense_rotate_rate.py > profiles/microbench/dense_rotate_rate_mi355x.txt

--cases 0,4 runs only those cases; --profile makes one call of each stage per case with no timing (for
rocprofv3 --kernel-trace --stats, or --pmc passes, in runs of their own).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

TARGET_MS = 250.0       # 512^3, sigma 1.6, isotropic


def cases():
    # (name, n, units, sigma)
    return [
        ("iso_s1.6", 256, (1.0, 1.0, 1.0), 1.6),
        ("iso_s1.6", 512, (1.0, 1.0, 1.0), 1.6),
        ("aniso(0.8,0.8,2)_s1.6", 512, (0.8, 0.8, 2.0), 1.6),
        ("iso_s3.2", 256, (1.0, 1.0, 1.0), 3.2),
        ("iso_s5.5", 128, (1.0, 1.0, 1.0), 5.5),     # 18 815 window voxels, near the 20 000 limit
    ]


def window_voxels(sigma, units):
    import numpy as np
    u = [np.float32(a) for a in units]
    rad = 3.0 * sigma
    m = [int(rad / float(a) + 2.0) for a in u]
    l, j, i = np.meshgrid(*[np.arange(-k, k + 1) for k in m[::-1]], indexing="ij")
    dx, dy, dz = i.astype(np.float32) * u[0], j.astype(np.float32) * u[1], l.astype(np.float32) * u[2]
    sq = dx * dx + dy * dy + dz * dz
    return int((~(sq.astype(np.float64) > rad * rad)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default=None)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    pick = None if args.cases is None else {int(c) for c in args.cases.split(",")}
    import torch
    from sift3d_amd import hip
    L = hip.lib()
    print("# sift3d_amd_dense_descriptors_rotate_device, float32 n^3 -> 12 x n^3, MI355X (gfx950)")
    print("# device events, min of %d calls after one warm-up; pairs = voxels x window voxels, once per stage"
          % args.reps)
    print("# target: 512^3 iso sigma 1.6 in %.0f ms" % TARGET_MS)
    print("%-24s %5s %6s %10s %10s %10s %10s %11s %11s" % ("case", "n", "win", "orient ms", "bin ms", "norm ms",
                                                          "total ms", "R2 Gpair/s", "R3 Gpair/s"))
    for ci, (name, n, units, sigma) in enumerate(cases()):
        if pick is not None and ci not in pick:
            continue
        src = torch.empty((n, n, n), device="cuda")
        hip.synth_lattice(src, 0, 11)
        R = torch.empty((3, 3, n, n, n), device="cuda")
        out = torch.empty((12, n, n, n), device="cuda")
        s = hip.current_stream(refresh=True)
        ux, uy, uz = units

        def orient():
            hip._check(L.sift3d_hip_dense_orient(src.data_ptr(), n, n, n, ux, uy, uz, sigma, R.data_ptr(), None, s),
                       "orient")

        def rbin():
            hip._check(L.sift3d_hip_dense_rotate_bin(src.data_ptr(), n, n, n, ux, uy, uz, sigma, R.data_ptr(),
                                                     out.data_ptr(), s), "rotate_bin")

        def norm():
            hip._check(L.sift3d_hip_dense_normalize(out.data_ptr(), n ** 3, s), "normalize")

        if args.profile:
            for f in (orient, rbin, norm):
                f()
            torch.cuda.synchronize()
            print("%s %d: one call of each stage" % (name, n))
            del src, R, out
            torch.cuda.empty_cache()
            continue
        times = []
        for f in (orient, rbin, norm):
            f()
            torch.cuda.synchronize()
            best = float("inf")
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                b.synchronize()
                best = min(best, a.elapsed_time(b))
            times.append(best)
        win = window_voxels(sigma, units)
        pairs = float(n) ** 3 * win
        print("%-24s %5d %6d %10.2f %10.2f %10.3f %10.2f %11.1f %11.1f" % (
            name, n, win, times[0], times[1], times[2], sum(times), pairs / times[0] * 1e-6,
            pairs / times[1] * 1e-6))
        sys.stdout.flush()
        del src, R, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
