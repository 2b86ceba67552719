#!/usr/bin/env python3
"""Cost of the MIND-SSC descriptor (include/sift3d_amd.h, "MIND self-similarity descriptors") at 128^3 and 256^3,
radius 1 and 2, dilation 2, in one run:

    (a) descriptor pass     sift3d_hip_mind_ssc writing the 12 channels alone, as api.mind_ssc's second call
    (b) statistics pass     sift3d_hip_mind_ssc writing the 16-byte record alone, as api.mind_ssc's first call
    (c) api.mind_ssc        (b), one host synchronisation, (a), and the allocation of the stack
    (d) dense_descriptors   the dense gradient descriptors of the same volume at sigma 1.6, for scale
    (e) hip.lncc            the statistics pass of local cross-correlation at radius 2 on the same grid, for scale

For (a) the achieved bytes / s over the pass's algorithmic bytes are reported: 4 B read and 48 B written per voxel.
(b)'s share of (a) + (b) is the cost of stating the clamps against the mean of V.  There is no pass / fail number:
the file is the record.

Times are HIP events around `reps` back-to-back calls, per call, the minimum of `trials` trials after a warm-up, with
the spread of the trials beside it.  Run it with the device to itself: the device's busy percentage as its driver
reports it (torch.cuda.utilization) is printed before the first and after the last measurement, so that the record
says whether it was.

    python3 profiles/microbench/mind_rate.py [--label TEXT] > OUT.txt"""
import argparse
import os
import sys

SIZES = (128, 256)


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


def _row(name, t, n, nbytes=None):
    rate = "" if nbytes is None else "%8.2f TB/s over %d B per voxel" % (nbytes * n ** 3 / (min(t) * 1e-3) / 1e12, nbytes)
    print("%-44s %9.4f [%.4f-%.4f] %s" % (name, min(t), min(t), max(t), rate), flush=True)
    return min(t)


def _busy():
    """the device's busy percentage over the driver's last sampling window, or "unknown" where it cannot be read"""
    import torch
    try:
        return "%d %%" % torch.cuda.utilization()
    except Exception as e:                                   # no management library on this machine
        return "unknown (%s)" % type(e).__name__


def run(label, reps, trials):
    import torch
    from sift3d_amd import api, hip
    hip.lib()
    print("# MIND-SSC descriptor, dilation 2, float32, MI355X (gfx950)%s" % (label and "; " + label))
    print("# HIP events around %d back-to-back calls, per call, min of %d trials [min-max of the trials]"
          % (reps, trials))
    torch.cuda.synchronize()
    print("# device busy before the first measurement, with nothing of this process queued: %s" % _busy())
    for n in SIZES:
        shape = (n, n, n)
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        I = torch.rand(shape, device="cuda", generator=g)
        out = torch.empty((12,) + shape, dtype=torch.float32, device="cuda")
        stats = torch.empty(2, dtype=torch.int64, device="cuda")
        work = torch.empty(hip.lib().sift3d_amd_mind_work_bytes(n, n, n) // 8, dtype=torch.int64, device="cuda")
        print("%-44s %9s" % ("call at %d^3" % n, "ms"))
        for r in (1, 2):
            a = _row("descriptor pass r=%d" % r, _time(lambda: hip.mind_ssc(I, out, r, 2, 1e-4, 1e2, work=work),
                                                       reps, trials), n, 52)
            b = _row("statistics pass r=%d" % r, _time(lambda: hip.mind_ssc(I, False, r, 2, stats=stats, work=work),
                                                       reps, trials), n)
            print("# the statistics pass is %.1f %% of the two" % (100.0 * b / (a + b)))
            _row("api.mind_ssc r=%d" % r, _time(lambda: api.mind_ssc(I, r, 2), reps, trials), n)
        del out
        _row("dense_descriptors sigma 1.6", _time(lambda: api.dense_descriptors(I, 1.6), reps, trials), n)
        u = torch.zeros((3,) + shape, dtype=torch.float32, device="cuda")
        coef = torch.empty((4,) + shape, dtype=torch.float64, device="cuda")
        pw = torch.empty(hip.lib().sift3d_amd_lncc_work_bytes(n, n, n) // 8, dtype=torch.int64, device="cuda")
        _row("hip.lncc statistics pass r=2", _time(lambda: hip.lncc(I, I, u, 2, shape, coef=coef, stats=stats, work=pw),
                                                   reps, trials), n, 44)
        del u, coef, pw
        torch.cuda.empty_cache()
    torch.cuda.synchronize()
    print("# device busy after the last measurement (this process's own work included): %s" % _busy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--label", default="")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    lib = os.environ.get("SIFT3D_AMD_LIB") or os.path.join(root, "sift3d_amd", "libsift3d_amd.so")
    if not os.path.exists(lib):
        sys.exit("%s is missing -- build first" % lib)
    sys.path.insert(0, root)
    run(a.label, a.reps, a.trials)


if __name__ == "__main__":
    main()
