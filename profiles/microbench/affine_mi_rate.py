#!/usr/bin/env python3
"""Time per pass of the two passes of the mutual-information affine refinement (sift3d_hip_parzen_hist_affine: the
Parzen histogram in fixed point; sift3d_hip_affine_mi_normal_eqs: the Fisher-scoring record) at 512^3 beside the
similarity pass (sift3d_hip_similarity_affine, B = 64, LINEAR) and the MSD normal equations
(sift3d_hip_affine_normal_eqs) on the same volumes and transform, in one run.

All four walk the fixed grid and gather the moving volume through the same affine (a rotation of 5 degrees about
(1, 2, 3) through the centre): 8 B read per voxel, nothing written.  The histogram pass commits four 64-bit LDS adds per
voxel into four neighbouring words of one row where the similarity pass commits one 32-bit add; the record pass is the
MSD pass plus the window, four LDS reads of W and five f64 multiplies per voxel.  Two contents:
  lattice  the lattice with a noise floor of similarity_rate.py / affine_refine_rate.py: bins spread within a wave;
  smooth   a sum of eight wide Gaussians (width 0.1 - 0.2 of the grid), scaled to [0, 100]: most lanes of a wave share
           b_f and k0, so their four adds meet in the same four words -- the case nobody had measured.

Times are HIP events around `reps` back-to-back calls, per call, the minimum of 3 trials after a warm-up.

    python3 profiles/microbench/affine_mi_rate.py [--label TEXT] > OUT.txt

Registers and occupancy are the compiler's (`hipcc -Rpass-analysis=kernel-resource-usage`); pass them in --label to
keep them with the numbers."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from affine_refine_rate import _volumes  # noqa: E402
from similarity_rate import _require_built, _rot, _time  # noqa: E402

PEAK_BPS = 8.0e12


def _smooth(n):
    """(F, M): two sums of eight separable Gaussians with the same centres, the moving one mapped by (v - 50)^2 / 25"""
    import torch
    rng = np.random.default_rng(11)
    x = torch.arange(n, device="cuda", dtype=torch.float32)
    F = torch.zeros((n, n, n), device="cuda")
    for _ in range(8):
        c = rng.uniform(0.1, 0.9, 3) * (n - 1)
        s = rng.uniform(0.1, 0.2) * n
        g = [torch.exp(-(x - float(ck)) ** 2 / (2 * s * s)) for ck in c]
        F += float(rng.uniform(0.5, 1.5)) * g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]
    F *= 100.0 / float(F.max())
    M = (F - 50.0) ** 2 / 25.0
    return F.contiguous(), M.contiguous()


def run(label, reps, n):
    import torch
    from sift3d_amd import hip
    print("# the two MI passes against the similarity pass and the MSD normal equations, float32, LINEAR, MI355X "
          "(gfx950)%s" % (label and "; " + label))
    print("# HIP events around %d back-to-back calls, per call, min of 3 trials [spread]; model bytes 8 B / voxel "
          "against 8 TB/s" % reps)
    print("%-8s %-6s %-26s %26s %13s %8s %8s" % ("content", "size", "call", "ms", "/ its sibling", "GB/s", "of peak"))
    c = np.full(3, (n - 1) / 2.0)
    R = _rot((1.0, 2.0, 3.0), 5.0)
    A = np.hstack([R, (c - R @ c)[:, None]])
    for content, make in (("lattice", _volumes), ("smooth", _smooth)):
        F, M = make(n)
        rf, rm = (float(F.min()), float(F.max())), (float(M.min()), float(M.max()))
        hist = torch.empty((64, 64), dtype=torch.int64, device="cuda")
        swork = torch.empty(hip.SIMILARITY_GRID * 56, dtype=torch.uint8, device="cuda")
        rec = torch.empty(hip.AFFINE_NORMAL_BYTES // 8, dtype=torch.int64, device="cuda")
        work = torch.empty(hip.affine_normal_work_bytes(), dtype=torch.uint8, device="cuda")
        s = _time(lambda: hip.similarity(F, M, A, 64, rf, rm, "linear", hist, swork), reps)
        a = _time(lambda: hip.affine_normal_equations(F, M, A, rec, work, raw=True), reps)
        rows = [("similarity B=64", s, "-"), ("affine_normal_eqs", a, "-")]
        notes = []
        for bins in (32, 64):
            ph = torch.empty((bins, bins), dtype=torch.int64, device="cuda")
            h = _time(lambda: hip.parzen_histogram(F, M, A, bins, rf, rm, ph, swork), reps)
            _, count = hip.parzen_histogram(F, M, A, bins, rf, rm, ph, swork)
            me = hip.parzen_mi(ph)
            W = torch.from_numpy(me.W).cuda()
            r = _time(lambda: hip.affine_mi_normal_equations(F, M, A, W, rf, rm, rec, work, raw=True), reps)
            rows += [("parzen_hist B=%d" % bins, h, "%.3f" % (min(h) / min(s))),
                     ("affine_mi_normal_eqs B=%d" % bins, r, "%.3f" % (min(r) / min(a)))]
            k, spp, b, H = hip.affine_normal_record(rec)
            assert k == int(count[0]) > 0 and me.n > 0 and np.array_equal(H, H.T) and spp > 0
            notes.append("B=%d: mi %.6f, %d non-empty bins of %d" % (bins, me.mi, int((me.W != 0).sum()), bins * bins))
        nbytes = 8.0 * float(n) ** 3
        for name, t, rel in rows:
            print("%-8s %-6s %-26s %8.4f [%.4f-%.4f] %13s %8.0f %8.3f" % (
                content, "%d^3" % n, name, min(t), min(t), max(t), rel, nbytes / min(t) / 1e6,
                nbytes / min(t) / 1e-3 / PEAK_BPS))
        print("# %s %d^3: %d of %d voxels counted; %s" % (content, n, k, n ** 3, "; ".join(notes)))
        del F, M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    _require_built()
    run(a.label, a.reps, a.size)


if __name__ == "__main__":
    main()
