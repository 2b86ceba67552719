#!/usr/bin/env python3
"""Cost of the discrete displacement search's two large kernels (include/sift3d_amd.h, "Discrete displacement search")
at 128^3 and 256^3, nc in {1, 12}, R in {2, 4, 6}:

    (a) sift3d_hip_cost_volume, warm, no masks: ms, and the time per term (label x voxel x channel: one LDS read, one
        convert, a double subtract, multiply and add), in picoseconds, beside block matching's own measured time per
        candidate x voxel (block_match_rate_mi355x.txt, 256^3, R = 1, 3, 6: the same mapping and the same f64 chain,
        three f64 operations per term there too), and the f64 rate against the part's peak
    (b) sift3d_hip_cost_select on that volume (nc does not enter): ms, and the bytes of d_cost over the time as a
        fraction of the HBM peak

Peaks: 256 CUs x 4 SIMDs x 16 f64 lanes x 2.4 GHz = 39.3e12 f64 operations / s; HBM 8 TB/s.  There is no pass / fail
number: the file is the record.  Times are HIP events around `reps` back-to-back calls, per call, the minimum of
`trials` trials after a warm-up, with the spread beside it.  Every size runs in a process of its own under a time
limit, and the run stops at the first that fails.  Run it with the device to itself.

    python3 profiles/microbench/cost_volume_rate.py [--label TEXT] > OUT.txt

SIFT3D_AMD_LIB selects another build of the library (make CVDEF=-DSIFT3D_CV_TILE=16, 8 or 4: that many blocks per
workgroup at every radius)."""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PEAK_F64 = 256 * 4 * 16 * 2.4e9
PEAK_HBM = 8e12
SIZES, CHANNELS, RADII = (128, 256), (1, 12), (2, 4, 6)
STEP_TIMEOUT = 240                                          # seconds, per size


def _require_built():
    """Building from here (a fork + exec of make) is not allowed once a profiler's preloaded library has initialised
    the GPU.  Build first."""
    lib = os.environ.get("SIFT3D_AMD_LIB") or os.path.join(ROOT, "sift3d_amd", "libsift3d_amd.so")
    if not os.path.exists(lib):
        sys.exit("%s is missing -- build first: python3 -c \"from sift3d_amd import _native; "
                 "_native.build()\"" % lib)


def _time(fn, reps, trials):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(2):
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


def block_match_ps():
    """block matching's measured picoseconds per candidate x voxel at 256^3, per R, from its own record"""
    out = {}
    path = os.path.join(ROOT, "profiles", "microbench", "block_match_rate_mi355x.txt")
    for line in open(path):
        m = re.match(r"block_match \(this build\)\s+R=(\d)\s+([0-9.]+)", line)
        if m:
            r = int(m.group(1))
            out[r] = float(m.group(2)) * 1e-3 / (64 ** 3 * (2 * r + 1) ** 3 * 64) * 1e12
    return out


def size_rows(n, reps, trials):
    import torch
    from sift3d_amd import hip
    hip.lib()
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    nb = (n // 4) ** 3
    for r in RADII:
        K = (2 * r + 1) ** 3
        cost = torch.empty((n // 4, n // 4, n // 4, K), dtype=torch.float32, device="cuda")
        for nc in CHANNELS:
            F = torch.rand((nc, n, n, n), device="cuda", generator=g)
            W = torch.rand((nc, n, n, n), device="cuda", generator=g)
            terms = nb * K * 64 * nc
            k = max(1, min(reps, int(2e11 / terms)))         # about a second of work per trial at the most
            t = _time(lambda: hip.cost_volume(F, W, r, cost=cost), k, trials)
            s = min(t) * 1e-3
            print("%-22s %3d^3 nc=%-2d R=%d %10.4f [%.4f-%.4f]  %7.4f ps/term  %6.2f T f64 op/s = %4.1f %% of peak"
                  % ("cost_volume", n, nc, r, min(t), min(t), max(t), s / terms * 1e12, 3 * terms / s / 1e12,
                     100 * 3 * terms / s / PEAK_F64), flush=True)
            del F, W
        u = torch.zeros((3, n // 4, n // 4, n // 4), device="cuda")
        v, data, stats = hip.cost_select(cost, u, 0.1)
        work = torch.empty(hip.COST_SELECT_WORK_BYTES // 4, dtype=torch.float32, device="cuda")
        t = _time(lambda: hip.cost_select(cost, u, 0.1, v, data, stats, work), reps, trials)
        s = min(t) * 1e-3
        print("%-22s %3d^3       R=%d %10.4f [%.4f-%.4f]  %7.1f MB of d_cost  %6.3f TB/s = %4.1f %% of HBM peak"
              % ("cost_select", n, r, min(t), min(t), max(t), cost.numel() * 4 / 1e6, cost.numel() * 4 / s / 1e12,
                 100 * cost.numel() * 4 / s / PEAK_HBM), flush=True)
        del cost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--label", default="")
    ap.add_argument("--size", type=int, default=None, help="only the rows of this size (a child of the full run)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    _require_built()
    if a.size:
        size_rows(a.size, a.reps, a.trials)
        return
    print("# discrete displacement search: cost volume and selection, float32, MI355X (gfx950)%s"
          % (a.label and "; " + a.label))
    print("# HIP events around up to %d back-to-back calls, per call, min of %d trials [min-max]; ms" % (a.reps, a.trials))
    print("# block matching's own time per candidate x voxel at 256^3 (block_match_rate_mi355x.txt): %s"
          % ", ".join("R=%d %.4f ps" % kv for kv in sorted(block_match_ps().items())))
    sys.stdout.flush()
    for n in SIZES:
        # a fresh process per size, each under its own limit; the first failure ends the run
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--size", str(n), "--reps", str(a.reps),
                             "--trials", str(a.trials)], timeout=STEP_TIMEOUT).returncode
        if rc != 0:
            sys.exit("the rows of %d^3 ended with status %d: nothing more is run" % (n, rc))


if __name__ == "__main__":
    main()
