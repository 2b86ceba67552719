#!/usr/bin/env python3
"""Rates of the multi-resolution transfers (sift3d_multires.hip k_restrict2, k_field_prolong2) and of a three-level
refine_field at 512^3, each beside its yardstick in the same run:

    field_prolong2           sift3d_hip_field_prolong2, 256^3 -> 512^3 (12 B written per fine voxel, 1.5 B read)
    affine_field             k_affine_field, the tree's other pure field writer (12 B written per voxel)
    compose(2 u_c, p -> p/2) the only prolongation before k_field_prolong2: k_field_compose of the doubled coarse
                             field with the field of p -> p / 2 on the fine grid
    restrict2 nc=12          sift3d_hip_restrict2 of [12, 512^3] (4 B read per source voxel, 0.5 B written)
    copy_ [12, 512^3]        a device-to-device copy of the same source bytes (reads them and writes as many)
    12 x (blur + downsample) the only anti-aliased halving before k_restrict2: per channel the detector's blur
                             (sigma 1: x pass, fused y + z pass) and k_downsample2
    restrict2 nc=3, x 0.5    a field going down
    refine_field             intensity and descriptors, 5 iterations per level, one level against three

Targets, same run: field_prolong2 <= 1.25 x affine_field and < compose; restrict2 nc=12 <= copy_ and < the 12 pairs.

    python3 profiles/microbench/multires_rate.py > profiles/microbench/multires_rate_mi355x.txt

Device events around back-to-back calls, per call; the compared calls alternate within each of 3 trials after one
warm-up, and each keeps its minimum."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N = 512
NC = 12
HBM = 8e12


def run():
    import torch
    from sift3d_amd import api, hip
    from field_algebra_rate import _min_alternating
    from field_rate import _oblique
    vox = float(N) ** 3
    C = N // 2
    print("# multi-resolution transfers, float32, fine grid %d^3, MI355X (gfx950); HIP events around back-to-back "
          "calls, per call, min of 3 alternating trials after one warm-up" % N)
    print("%-46s %10s %9s %10s" % ("call", "ms", "alg GB", "frac 8TB/s"))

    def line(name, ms, nbytes):
        print("%-46s %10.4f %9.3f %10.3f" % (name, ms, nbytes / 1e9, (nbytes / HBM * 1e3) / ms if nbytes else 0.0))

    # ---- prolongation
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    uc = (torch.rand((3, C, C, C), device="cuda", generator=g) - 0.5) * 8.0
    uc2 = uc * 2.0
    fine = torch.empty((3, N, N, N), device="cuda")
    aff = torch.empty_like(fine)
    half = torch.empty_like(fine)
    hip.affine_field(half, np.hstack([0.5 * np.eye(3), np.zeros((3, 1))]))         # p -> p / 2
    out = torch.empty_like(fine)
    A = _oblique()
    t = _min_alternating({
        "prolong": lambda: hip.field_prolong2(uc, fine),
        "affine": lambda: hip.affine_field(aff, A),
        "compose": lambda: hip.field_compose(uc2, half, out, "compose"),
    }, 5)
    line("field_prolong2 (k_field_prolong2)", t["prolong"], 13.5 * vox)
    line("affine_field (k_affine_field)", t["affine"], 12 * vox)
    line("compose_fields(2 u_c, p -> p/2) (parent's way)", t["compose"], 25.5 * vox)
    r1, r2 = t["prolong"] / t["affine"], t["prolong"] / t["compose"]
    print("# target 1: field_prolong2 / affine_field = %.3f (must be <= 1.25): %s" % (r1, "met" if r1 <= 1.25 else "MISSED"))
    print("# target 2: field_prolong2 / compose = %.3f (must be < 1): %s" % (r2, "met" if r2 < 1 else "MISSED"))
    del aff, half, out, uc2
    # ---- restriction of a field
    dc = torch.empty((3, C, C, C), device="cuda")
    t = _min_alternating({"restrict3": lambda: hip.restrict2(fine, dc, 0.5)}, 5)
    line("restrict2 nc=3, scale 0.5 (k_restrict2)", t["restrict3"], 13.5 * vox)
    del fine, dc, uc
    torch.cuda.empty_cache()
    # ---- restriction of a feature stack
    src = torch.rand((NC, N, N, N), device="cuda", generator=g)
    cp = torch.empty_like(src)
    dst = torch.empty((NC, C, C, C), device="cuda")
    tmp, tmp2 = torch.empty((N, N, N), device="cuda"), torch.empty((N, N, N), device="cuda")
    taps = api.gauss_filter(1.0)

    def pairs():
        for c in range(NC):
            hip.fir(src[c], tmp, 0, taps)
            if not hip.fir_yz(tmp, tmp2, taps):
                raise RuntimeError("fir_yz does not cover this case")
            hip.downsample2(tmp2, dst[c])

    t = _min_alternating({
        "restrict": lambda: hip.restrict2(src, dst),
        "copy": lambda: cp.copy_(src),
        "pairs": pairs,
    }, 3)
    line("restrict2 nc=12 (k_restrict2)", t["restrict"], NC * 4.5 * vox)
    line("copy_ [12, 512^3]", t["copy"], NC * 8 * vox)
    line("12 x (blur sigma 1 + downsample2) (parent's way)", t["pairs"], NC * 20.5 * vox)
    r1, r2 = t["restrict"] / t["copy"], t["restrict"] / t["pairs"]
    print("# target 3: restrict2 / copy_ = %.3f (must be <= 1): %s" % (r1, "met" if r1 <= 1 else "MISSED"))
    print("# target 4: restrict2 / 12 pairs = %.3f (must be < 1): %s" % (r2, "met" if r2 < 1 else "MISSED"))
    del src, cp, dst, tmp, tmp2
    torch.cuda.empty_cache()
    # ---- refine_field, one level against three with the same iterations per level
    fixed = torch.empty((N, N, N), device="cuda")
    hip.synth_lattice(fixed, 0, 21)
    moving = torch.roll(fixed, (1, 2, 1), (0, 1, 2)).contiguous()
    K = 5
    for feats in ("intensity", "descriptors"):
        t = _min_alternating({
            "one": lambda: api.refine_field(moving, fixed, None, K, features=feats),
            "three": lambda: api.refine_field(moving, fixed, None, K, features=feats, levels=3),
        }, 1)
        line("refine_field %s, %d iterations, 1 level" % (feats, K), t["one"], 0)
        line("refine_field %s, %d per level, 3 levels" % (feats, K), t["three"], 0)
        print("# three levels / one level = %.3f (1 + 1/8 + 1/64 = 1.141 by voxel count)" % (t["three"] / t["one"]))


if __name__ == "__main__":
    np.seterr(all="ignore")
    run()
