#!/usr/bin/env python3
"""Device seconds of the blind match and of the guided match on the two descriptor stores of `bench.py --register`.

The stores are built as register_bench builds them: two 512^3 lattice-blob volumes, the second the first rotated by 90
degrees about z and shifted, detected and described with the stores keeping their histograms in HBM.  One run prints

  blind         Matcher.match (sift3d_hip_nn2 both ways), its match count and RANSAC inliers at err_thresh = 3
  guided r      Matcher.match_guided at radius 4, 16, 64 and +inf, guided by the blind pass's RANSAC affine:
                device seconds, block pairs visited / in all, matches, RANSAC inliers at err_thresh = 3

Device seconds are Matcher.seconds(): HIP events around the two searches on the matcher's stream, the median of
--reps matches after one warm-up.  The +inf row against the blind row is the price of the gate's epilogue and of
the row-order indirection (nothing is skipped); the other rows show what block skipping buys.

    python3 profiles/microbench/match_guided_rate.py [--size 512] [--reps 5]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def _require_built():
    """Build first: this script only measures (a build from here would compile on the measuring machine)."""
    lib = os.environ.get("SIFT3D_AMD_LIB") or os.path.join(ROOT, "sift3d_amd", "libsift3d_amd.so")
    if not os.path.exists(lib):
        sys.exit("%s is missing -- build first: python3 -c \"from sift3d_amd import _native; "
                 "_native.build()\"" % lib)


def stores(n):
    import torch
    from sift3d_amd import api, hip
    sy, sz = 5, 9
    vol = torch.empty((n + 24, n + 16, n), device="cuda")
    hip.synth_lattice(vol, 0, 21)
    v1 = vol[0:n, 0:n, :].contiguous()
    v2 = vol[sz:sz + n, sy:sy + n, :].transpose(1, 2).flip(1).contiguous()
    del vol
    torch.cuda.synchronize()
    out = []
    for v in (v1, v2):
        det, kp, desc = api.Detector(), api.KeypointStore(), api.DescriptorStore()
        desc.keep_device(True)
        assert det.detect_keypoints_device(v.data_ptr(), n, n, n, kp) == 0
        assert det.extract_descriptors(kp, desc) == 0
        out.append(desc)
    return out


def timed(matcher, call, reps):
    call()
    secs = []
    for _ in range(reps):
        m = call()
        secs.append(matcher.seconds())
    return m, float(np.median(secs))


def ransac(api, da, db, m):
    hit = np.nonzero(m >= 0)[0]
    T, inl = api.ransac_affine(da.xyz()[hit], db.xyz()[m[hit]], err_thresh=3.0, num_iter=500, seed=5)
    return T, len(hit), int(inl.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    _require_built()
    from sift3d_amd import api
    da, db = stores(a.size)
    matcher = api.Matcher()
    print("# match_guided_rate: %d^3 pair, %d x %d descriptors, median of %d" % (a.size, len(da), len(db), a.reps))
    print("%-12s %10s %16s %9s %9s" % ("search", "device ms", "blocks visited", "matches", "inliers"))
    m, s = timed(matcher, lambda: matcher.match(da, db, 0.8), a.reps)
    T, nm, ni = ransac(api, da, db, m)
    print("%-12s %10.3f %16s %9d %9d" % ("blind", 1e3 * s, "-", nm, ni))
    for radius in (4.0, 16.0, 64.0, float("inf")):
        m, s = timed(matcher, lambda: matcher.match_guided(da, db, T, radius, 0.8), a.reps)
        _, nm, ni = ransac(api, da, db, m)
        print("%-12s %10.3f %16s %9d %9d" % ("guided %g" % radius, 1e3 * s, "%d/%d" % matcher.blocks(), nm, ni))


if __name__ == "__main__":
    main()
