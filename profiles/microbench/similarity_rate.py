#!/usr/bin/env python3
"""Rate of the similarity pass (sift3d_hip_similarity_affine / _field) at 512^3 against the warp that does the same
gather, in one run.

Cases: B = 64 and B = 128, LINEAR, through an affine (a rotation of 5 degrees about (1, 2, 3) through the centre) and
through that affine's displacement field; two contents: a lattice volume with a noise floor everywhere (bins spread)
and the same with about 70 % of the voxels (everything outside a centred ball) set to exactly 0 in both volumes, the
masked-volume case, whose waves mostly fall wholly into bin (0, 0).  sift3d_hip_warp_affine / _warp_field (nc = 1,
LINEAR) are timed on the same volumes and transform in the same run: the warp writes 4 B per voxel, the similarity
pass reads 4 B more per voxel and writes nothing.  Target: similarity <= warp x 1.05.

Times are HIP events around `reps` back-to-back calls, per call, the minimum of 3 trials after a warm-up.  Model bytes:
8 B per voxel (+ 12 B of field), against the 8 TB/s HBM peak.

    python3 profiles/microbench/similarity_rate.py [--label TEXT] > OUT.txt

SIFT3D_AMD_LIB selects another build of the library: one made with `make SIMDEF=-DSIFT3D_SIMILARITY_NO_UNIFORM`
times the pass with the wave-uniform commit compiled out."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N = 512
PEAK_BPS = 8.0e12


def _require_built():
    """Building from here (a fork + exec of make) is not allowed once a profiler's preloaded library has initialised
    the GPU.  Build first."""
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


def _volumes(masked):
    """(F, M): a lattice volume plus a noise floor, and a second noise draw on the same lattice; masked: 0 outside a
    centred ball of 30 % of the volume in both"""
    import torch
    from sift3d_amd import hip
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    base = torch.empty((N, N, N), device="cuda")
    hip.synth_lattice(base, 0, 11)
    scale = float(base.abs().max())
    F = base / scale + 0.05 * torch.randn(base.shape, generator=g, device="cuda")
    M = base / scale + 0.05 * torch.randn(base.shape, generator=g, device="cuda")
    del base
    if masked:
        r = (0.3 * 3.0 / (4.0 * np.pi)) ** (1.0 / 3.0) * N
        ax = (torch.arange(N, device="cuda", dtype=torch.float32) - (N - 1) / 2.0) ** 2
        ball = (ax[:, None, None] + ax[None, :, None] + ax[None, None, :]) <= r * r
        F = F * ball
        M = M * ball
        del ball
    return F.contiguous(), M.contiguous()


def _time(fn, reps, trials=3):
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


def run(label, reps):
    import torch
    from sift3d_amd import api, hip
    A = _about_center(_rot((1.0, 2.0, 3.0), 5.0))
    field = api.displacement_field(A, (N, N, N))
    dst = torch.empty((N, N, N), device="cuda")
    work = torch.empty(hip.SIMILARITY_GRID * 56, dtype=torch.uint8, device="cuda")
    vox = float(N) ** 3
    print("# similarity pass against the warp, %d^3 float32, LINEAR, MI355X (gfx950)%s" % (N, label and "; " + label))
    print("# HIP events around %d back-to-back calls, per call, min of 3 trials [spread]; model bytes 8 B / voxel "
          "(+ 12 B of field) against 8 TB/s; target: similarity / warp <= 1.05" % reps)
    print("%-9s %-7s %-22s %26s %9s %8s %8s" % ("content", "map", "call", "ms", "/ warp", "GB/s", "of peak"))
    for content in ("spread", "masked"):
        F, M = _volumes(content == "masked")
        lo, hi = float(min(F.min(), M.min())), float(max(F.max(), M.max()))
        zero = float((F == 0).float().mean())
        for name, T in (("affine", A), ("field", field)):
            if name == "affine":
                w = _time(lambda: hip.warp_affine(M, dst, A, "linear"), reps)
            else:
                w = _time(lambda: hip.warp_field(M, dst, field, "linear"), reps)
            nbytes = vox * (8.0 + (12.0 if name == "field" else 0.0))
            print("%-9s %-7s %-22s %8.4f [%.4f-%.4f] %9s %8.0f %8.3f" % (
                content, name, "warp_" + name, min(w), min(w), max(w), "-", nbytes / min(w) / 1e6,
                nbytes / min(w) / 1e-3 / PEAK_BPS))
            for bins in (64, 128):
                hist = torch.empty((bins, bins), dtype=torch.int64, device="cuda")
                s = _time(lambda: hip.similarity(F, M, T, bins, (lo, hi), (lo, hi), "linear", hist, work), reps)
                count, _ = hip.similarity_stats(hip.similarity(F, M, T, bins, (lo, hi), (lo, hi), "linear", hist, work)[1])
                print("%-9s %-7s %-22s %8.4f [%.4f-%.4f] %9.3f %8.0f %8.3f" % (
                    content, name, "similarity B=%d" % bins, min(s), min(s), max(s), min(s) / min(w),
                    nbytes / min(s) / 1e6, nbytes / min(s) / 1e-3 / PEAK_BPS))
                assert int(hist.sum()) == count > 0
        print("# %s: %.1f %% of F's voxels are exactly 0; %d of %d voxels counted; range (%.3f, %.3f)"
              % (content, 100 * zero, count, int(vox), lo, hi))
        del F, M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    _require_built()
    run(a.label, a.reps)


if __name__ == "__main__":
    main()
