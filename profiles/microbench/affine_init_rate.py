#!/usr/bin/env python3
"""Rates behind init_affine (include/sift3d_amd.h, "Initial transforms: moments and candidate search") on 32^3, 64^3 and
128^3 pairs, in one run.

1. The batch entry (sift3d_hip_similarity_affine_batch) at K = 343, the default search, against 343 calls of
   hip.similarity each followed by reading its record back, as a search has to today (a memset, the pass, the finish,
   a copy to the host and a wait per candidate).  Both with 32 bins (MI) and, the batch alone, with bins = 0 (MSD and
   NCC).  The batch's time includes reading all 343 records and histograms back.  The entry is kept only if it beats the
   loop at 32^3 and 64^3, the sizes a search runs at.
2. The moments pass against its read-bound time: 4 B per voxel (8 with a mask) over the 8 TB/s HBM peak.
3. init_affine as a whole (mode "search", MI, levels so that the search runs at 32^3 where the pair allows).

Times are host clocks around work that ends in a device synchronise (both sides of 1. end in one), per call, the
minimum of 5 trials after a warm-up, with the spread.

    python3 profiles/microbench/affine_init_rate.py [--label TEXT] > OUT.txt"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SIZES = (32, 64, 128)
K = 343
BINS = 32
PEAK_BPS = 8.0e12


def _require_built():
    """Building from here (a fork + exec of make) is not allowed once a profiler's preloaded library has initialised
    the GPU.  Build first."""
    lib = os.environ.get("SIFT3D_AMD_LIB") or os.path.join(ROOT, "sift3d_amd", "libsift3d_amd.so")
    if not os.path.exists(lib):
        sys.exit("%s is missing -- build first: python3 -c \"from sift3d_amd import _native; "
                 "_native.build()\"" % lib)


def _pair(n):
    """a blob phantom and its rotated, shifted, inverted copy, zero background, on the device"""
    import torch
    from sift3d_amd import hip
    ax = torch.arange(n, device="cuda", dtype=torch.float32) - (n - 1) / 2.0
    z, y, x = ax[:, None, None], ax[None, :, None], ax[None, None, :]
    r = n / 48.0
    body = ((x / (15 * r)) ** 2 + (y / (10 * r)) ** 2 + (z / (6.5 * r)) ** 2) <= 1.0
    ball = ((x - 10 * r) ** 2 + (y - 5 * r) ** 2 + (z + 4 * r) ** 2) <= (5 * r) ** 2
    F = (body * (0.45 + 0.012 / r * x) + ball * 0.3).contiguous()
    t = np.deg2rad(60.0)
    R = np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]])
    c = np.full(3, (n - 1) / 2.0)
    A = np.hstack([R, (c + [2 * r, -r, r] - R @ c)[:, None]])
    M = torch.empty_like(F)
    hip.warp_affine(F, M, A, "linear")
    M = torch.where(M > 0, 1.25 - M, torch.zeros_like(M)).contiguous()
    return F, M


def _time(fn, trials=5):
    import torch
    fn()
    out = []
    for _ in range(trials):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def _fmt(ms):
    return "%9.3f [%.3f-%.3f]" % (min(ms), min(ms), max(ms))


def run(label):
    import torch
    from sift3d_amd import api, hip
    print("# initial transforms, MI355X (gfx950)%s" % (label and "; " + label))
    print("# host clock around work that ends in a synchronise, ms, min of 5 trials [spread]")
    print("#\n# 1. %d candidates (the default search), LINEAR: one batch call against a loop of single calls" % K)
    print("%-6s %-28s %28s %10s" % ("size", "call", "ms", "loop / it"))
    for n in SIZES:
        F, M = _pair(n)
        rf, rm = (0.0, float(F.max())), (0.0, float(M.max()))
        fr = [hip.moments_frame(hip.moments(V, "binary", 0.0), V.shape) for V in (F, M)]
        A = hip.affine_init_candidates("search", fr[0], fr[1])
        assert len(A) == K
        hist1 = torch.empty((BINS, BINS), dtype=torch.int64, device="cuda")
        work1 = torch.empty(hip.SIMILARITY_GRID * 56, dtype=torch.uint8, device="cuda")

        def loop():
            out = []
            for a in A:
                h, s = hip.similarity(F, M, a, BINS, rf, rm, "linear", hist1, work1)
                out.append((hip.similarity_stats(s), h.cpu()))
            return out

        def batch(bins):
            h, s = hip.similarity_batch(F, M, A, bins, rf, rm)
            return s.cpu(), None if h is None else h.cpu()
        want = loop()
        st, hs = batch(BINS)
        for k in range(K):                                  # the same bytes
            assert int(st[k, 0]) == want[k][0][0] and torch.equal(hs[k], want[k][1])
        t_loop, t_b, t_0 = _time(loop), _time(lambda: batch(BINS)), _time(lambda: batch(0))
        print("%-6s %-28s %28s %10s" % ("%d^3" % n, "343 x similarity + read back", _fmt(t_loop), "-"))
        print("%-6s %-28s %28s %10.1f" % ("%d^3" % n, "batch, 32 bins + read back", _fmt(t_b), min(t_loop) / min(t_b)))
        print("%-6s %-28s %28s %10.1f" % ("%d^3" % n, "batch, no bins + read back", _fmt(t_0), min(t_loop) / min(t_0)))
    print("#\n# 2. the moments pass against its read-bound time (4 B per voxel, 8 with a mask, over 8 TB/s); device events"
          "\n#    around 50 back-to-back calls, per call")
    print("%-6s %-12s %12s %14s %10s" % ("size", "mask", "ms", "read-bound ms", "x bound"))
    for n in SIZES + (512,):
        V = torch.rand((n, n, n), device="cuda")
        W = (torch.rand((n, n, n), device="cuda") < 0.8).float()
        rec = torch.empty(11, dtype=torch.int64, device="cuda")
        work = torch.empty(hip.SIMILARITY_GRID * 88, dtype=torch.uint8, device="cuda")
        for mask in (None, W):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ms = []
            for _ in range(4):
                e0.record()
                for _ in range(50):
                    hip.moments(V, "intensity", 0.25, mask, rec, work, raw=True)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / 50)
            ms = ms[1:]
            bound = n ** 3 * (4.0 if mask is None else 8.0) / PEAK_BPS * 1e3
            print("%-6s %-12s %12.4f %14.5f %10.1f" % ("%d^3" % n, "none" if mask is None else "80 % in", min(ms), bound,
                                                       min(ms) / bound))
        del V, W
    print("#\n# 3. init_affine as a whole: mode \"search\", MI, 343 candidates")
    print("%-6s %-8s %-10s %28s" % ("size", "levels", "search at", "ms"))
    for n in SIZES:
        F, M = _pair(n)
        levels = {32: 1, 64: 2, 128: 3}[n]
        ms = _time(lambda: api.init_affine(M, F, levels=levels))
        print("%-6s %-8d %-10s %28s" % ("%d^3" % n, levels, "%d^3" % (n >> (levels - 1)), _fmt(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    _require_built()
    run(a.label)


if __name__ == "__main__":
    main()
