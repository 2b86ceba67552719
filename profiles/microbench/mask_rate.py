#!/usr/bin/env python3
"""Cost of the region-of-interest masks (include/sift3d_amd.h, "Masks") at 256^3: the similarity pass (LINEAR, 64
bins), the normal-equation pass and the FFD evaluation (spacing 8), each unmasked and with both masks set (random
binary, about 60 % in each), in one run.

A masked pass reads per voxel one more coalesced 4 B (W_F beside F) and one more gathered 4 B (W_M at the nearest voxel
of q) on top of F and the eight-corner gather; it counts fewer voxels, so the histogram commits and the accumulating
arithmetic shrink with the mask.  The ratio masked / unmasked is reported, not capped.

Times are HIP events around `reps` back-to-back calls, per call, the minimum of `trials` trials after a warm-up, with
the spread of the trials beside it.  Run it with the device to itself.

    python3 profiles/microbench/mask_rate.py [--label TEXT] [--root CHECKOUT] > OUT.txt

--root imports the package from another checkout (one that is already built): on a checkout without the masked
entries only the unmasked rows are timed, which is how the unmasked figures of two commits are compared in one
session."""
import argparse
import os
import sys

import numpy as np

N = 256
SPACING = 8


def _time(fn, reps, trials):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    ms = []
    for _ in range(trials):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return ms


def _rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def run(label, reps, trials):
    import torch
    from sift3d_amd import hip
    L = hip.lib()
    masked = hasattr(L, "sift3d_hip_similarity_affine_masked")
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    base = torch.empty((N, N, N), device="cuda")
    hip.synth_lattice(base, 0, 11)
    scale = float(base.abs().max())
    F = (base / scale + 0.05 * torch.randn(base.shape, generator=g, device="cuda")).contiguous()
    M = (base / scale + 0.05 * torch.randn(base.shape, generator=g, device="cuda")).contiguous()
    WF = (torch.rand(base.shape, generator=g, device="cuda") < 0.6).float().contiguous()
    WM = (torch.rand(base.shape, generator=g, device="cuda") < 0.6).float().contiguous()
    del base
    c = np.full(3, (N - 1) / 2.0)
    R = _rot((1.0, 2.0, 3.0), 5.0)
    A = np.hstack([R, (c - R @ c)[:, None]])
    lo, hi = float(min(F.min(), M.min())), float(max(F.max(), M.max()))
    hist = torch.empty((64, 64), dtype=torch.int64, device="cuda")
    swork = torch.empty(hip.SIMILARITY_GRID * 56, dtype=torch.uint8, device="cuda")
    rec = torch.empty(hip.AFFINE_NORMAL_BYTES // 8, dtype=torch.int64, device="cuda")
    nwork = torch.empty(hip.affine_normal_work_bytes(), dtype=torch.uint8, device="cuda")
    lattice = (0.5 * torch.randn(hip.ffd_lattice_shape((N, N, N), SPACING), generator=g, device="cuda")).contiguous()
    fwork = torch.empty(L.sift3d_amd_ffd_evaluate_work_bytes(N, N, N, SPACING, SPACING, SPACING), dtype=torch.uint8,
                        device="cuda")
    mk = dict(mask_fixed=WF, mask_moving=WM)
    calls = [("similarity B=64", lambda kw: hip.similarity(F, M, A, 64, (lo, hi), (lo, hi), "linear", hist, swork, **kw)),
             ("normal equations", lambda kw: hip.affine_normal_equations(F, M, A, rec, nwork, True, **kw)),
             ("ffd evaluate", lambda kw: hip.ffd_evaluate(F, M, lattice, SPACING, None, 0.005, fwork, **kw))]
    print("# masks: unmasked against masked passes, %d^3 float32, LINEAR, MI355X (gfx950)%s" % (N, label and "; " + label))
    print("# HIP events around %d back-to-back calls, per call, min of %d trials [min-max of the trials]; both masks "
          "random binary, 60 %% in each" % (reps, trials))
    print("%-18s %-9s %28s %10s" % ("call", "masks", "ms", "/ unmasked"))
    for name, call in calls:
        t0 = _time(lambda: call({}), reps, trials)
        print("%-18s %-9s %9.4f [%.4f-%.4f] %10s" % (name, "none", min(t0), min(t0), max(t0), "-"))
        if masked:
            t1 = _time(lambda: call(mk), reps, trials)
            print("%-18s %-9s %9.4f [%.4f-%.4f] %10.3f" % (name, "both", min(t1), min(t1), max(t1), min(t1) / min(t0)))
    if masked:
        n0 = hip.similarity_stats(hip.similarity(F, M, A, 64, (lo, hi), (lo, hi), "linear", hist, swork)[1])[0]
        n1 = hip.similarity_stats(hip.similarity(F, M, A, 64, (lo, hi), (lo, hi), "linear", hist, swork, **mk)[1])[0]
        print("# counted voxels: %d unmasked, %d masked (%.1f %%)" % (n0, n1, 100.0 * n1 / n0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--label", default="")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    lib = os.environ.get("SIFT3D_AMD_LIB") or os.path.join(os.path.abspath(a.root), "sift3d_amd", "libsift3d_amd.so")
    if not os.path.exists(lib):
        sys.exit("%s is missing -- build first" % lib)
    run(a.label, a.reps, a.trials)


if __name__ == "__main__":
    main()
