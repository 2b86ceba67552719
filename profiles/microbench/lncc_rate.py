#!/usr/bin/env python3
"""Cost of local cross-correlation (include/sift3d_amd.h, "Local cross-correlation") at 256^3, radius 2 and 4, in one
run:

    (a) statistics pass     sift3d_hip_lncc with the coefficient volumes and no map, as the driver calls it
    (b) force pass          sift3d_hip_lncc_force
    (c) normalisation       sift3d_hip_field_normalize
    (d) one whole iteration sift3d_amd_demons_lncc_device: warp, validity, (a), (b), fluid blur, (c), u += phi,
                            diffusion blur, at sigma_fluid 2, sigma_diffusion 1
    (e) one demons iteration, nc = 1, at refine_field's defaults, on the same volumes: of this checkout, and with
        --parent ROOT of another (built) checkout, which is how the parent commit's figure is put beside them

For (a) and (b) the achieved bytes / s over the pass's algorithmic bytes are reported: (a) reads F, W and v (12 B per
voxel) and writes four doubles (32 B): 44 B; (b) reads the four doubles, F, W and v (44 B; W's six neighbours come
from cache) and writes phi (12 B): 56 B.  (Both entries also run the validity kernel, 12 + 4 B per voxel, which the
figure leaves out of the bytes and in the time.)  There is no pass / fail number: the file is the record.

Times are HIP events around `reps` back-to-back calls, per call, the minimum of `trials` trials after a warm-up, with
the spread of the trials beside it; the iteration rows first copy the start field back (3 planes read and written, the
same in every row).  Run it with the device to itself.

    python3 profiles/microbench/lncc_rate.py [--label TEXT] [--parent CHECKOUT] > OUT.txt

SIFT3D_AMD_LIB selects another build of the library (make LNCCDEF=-DSIFT3D_LNCC_ZC=n: another stretch of planes per
tile; LNCCDEF=-DSIFT3D_LNCC_RY=2: the 64 x 8 tile)."""
import argparse
import os
import subprocess
import sys

N = 256


def _require_built(root):
    lib = os.environ.get("SIFT3D_AMD_LIB") or os.path.join(root, "sift3d_amd", "libsift3d_amd.so")
    if not os.path.exists(lib):
        sys.exit("%s is missing -- build first" % lib)


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


def _row(name, t, nbytes=None):
    rate = "" if nbytes is None else "%8.2f TB/s over %d B per voxel" % (nbytes * N ** 3 / (min(t) * 1e-3) / 1e12, nbytes)
    print("%-44s %9.4f [%.4f-%.4f] %s" % (name, min(t), min(t), max(t), rate), flush=True)


def _volumes():
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    shape = (N, N, N)
    F = torch.rand(shape, device="cuda", generator=g)
    M = torch.rand(shape, device="cuda", generator=g)
    u = (torch.rand((3,) + shape, device="cuda", generator=g) - 0.5) * 2.0
    return F, M, u


def demons_row(tag, reps, trials):
    import torch
    from sift3d_amd import api, hip
    hip.lib()
    F, M, u = _volumes()
    uu = torch.empty_like(u)
    work = torch.empty((hip.lib().sift3d_amd_demons_work_floats(N, N, N, 1) + 1) // 2, dtype=torch.float64,
                       device="cuda")

    def it():
        uu.copy_(u)
        hip.demons(F, M, uu, 1, api.DEMONS_ALPHA, api.DEMONS_SIGMA_FLUID, api.DEMONS_SIGMA_DIFFUSION, work)
    _row("demons iteration nc=1 at the defaults (%s)" % tag, _time(it, max(reps // 4, 1), trials))


def run(label, reps, trials):
    import torch
    from sift3d_amd import hip
    hip.lib()
    shape = (N, N, N)
    print("# local cross-correlation: the two passes, the normalisation and one iteration, %d^3 float32, MI355X "
          "(gfx950)%s" % (N, label and "; " + label))
    print("# HIP events around %d back-to-back calls (iterations: %d), per call, min of %d trials [min-max of the "
          "trials]" % (reps, max(reps // 4, 1), trials))
    print("%-44s %9s" % ("call", "ms"))
    F, M, u = _volumes()
    W = torch.empty_like(F)
    hip.warp_field(M, W, u)
    coef = torch.empty((4,) + shape, dtype=torch.float64, device="cuda")
    phi = torch.empty_like(u)
    keep = torch.empty_like(u)
    uu = torch.empty_like(u)
    stats = torch.empty(2, dtype=torch.int64, device="cuda")
    pw = torch.empty(hip.lib().sift3d_amd_lncc_work_bytes(N, N, N) // 8, dtype=torch.int64, device="cuda")
    nw = torch.empty(hip.FIELD_NORMALIZE_WORK_BYTES // 8, dtype=torch.int64, device="cuda")
    work = torch.empty((hip.lib().sift3d_amd_demons_lncc_work_floats(N, N, N, 0, 1) + 1) // 2, dtype=torch.float64,
                       device="cuda")
    for r in (2, 4):
        _row("statistics pass r=%d" % r, _time(lambda: hip.lncc(F, W, u, r, shape, coef=coef, stats=stats, work=pw),
                                              reps, trials), 44)
        n = int(hip.demons_stats(stats)[1][0])
        print("# counted voxels: %d of %d (%.1f %%)" % (n, N ** 3, 100.0 * n / N ** 3))
        _row("force pass r=%d" % r, _time(lambda: hip.lncc_force(F, W, u, coef, phi, r, shape, work=pw), reps, trials), 56)
        keep.copy_(phi)

        def norm():
            phi.copy_(keep)
            hip.field_normalize(phi, 0.5, nw)
        _row("normalisation (and the copy that resets it)", _time(norm, reps, trials))

        def it():
            uu.copy_(u)
            hip.demons_lncc([F], [M], uu, [1], r, 0.5, 2.0, 1.0, work)
        _row("lncc iteration r=%d, sigmas 2 / 1" % r, _time(it, max(reps // 4, 1), trials))
    del coef, phi, keep, work
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--label", default="")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its demons iteration too")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--demons-only", default=None, metavar="TAG", help="only the demons row, under this tag")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    _require_built(root)
    if a.parent:
        _require_built(os.path.abspath(a.parent))
    sys.path.insert(0, root)
    if a.demons_only:
        demons_row(a.demons_only, a.reps, a.trials)
        return
    run(a.label, a.reps, a.trials)
    demons_row("this checkout", a.reps, a.trials)
    if a.parent:
        # a fresh process: one process cannot import the package of two checkouts
        sys.stdout.flush()
        env = dict(os.environ)
        env.pop("SIFT3D_AMD_LIB", None)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--demons-only", "parent commit", "--root",
                        os.path.abspath(a.parent), "--reps", str(a.reps), "--trials", str(a.trials)], check=True,
                       env=env)


if __name__ == "__main__":
    main()
