#!/usr/bin/env python3
"""Cost of the region-of-interest masks in demons (include/sift3d_amd.h, "Masks in demons") at 256^3, nc = 1 and
nc = 12, in one run:

    (a) force, unmasked          sift3d_hip_demons_force
    (b) force, random masks      both masks random binary, about 60 % in each: nothing for the wave-uniform skip to find
    (c) force, ball mask         mask_fixed a centred ball holding 50 % of the voxels, mask_moving None: the waves
                                 wholly outside the ball skip the channel loop
    (d) one whole iteration      warp, force, fluid blur, u += delta, diffusion blur at the defaults, unmasked and with
                                 the masks of (b) and of (c)

The masked force reads per voxel one more coalesced 4 B (W_F beside u) and one more gathered 4 B (W_M at the nearest
voxel of q) on top of 28 B (nc = 1) or 116 B (nc = 12) read and 12 B written.  The ratios (b) / (a) and (c) / (a) are
reported, not capped.

Times are HIP events around `reps` back-to-back calls, per call, the minimum of `trials` trials after a warm-up, with
the spread of the trials beside it; the iteration rows take reps / 4 calls, each of which first copies the start field
back (3 planes read and written, the same in every row).  Run it with the device to itself.

    python3 profiles/microbench/demons_mask_rate.py [--label TEXT] [--root CHECKOUT] > OUT.txt
    python3 profiles/microbench/demons_mask_rate.py --geometry [--n 512] >> OUT.txt

--geometry times the force alone under fixed masks of other geometry (all out, all in, the half spaces along z, y and
x, blocks of two tiles (4 planes) alternating along z): which regions the skip turns into time, and which it does not.

--root imports the package from another checkout (one that is already built): on a checkout without the masked entries
only the unmasked rows are timed, which is how the unmasked figures of two commits are compared in one session.
SIFT3D_AMD_LIB selects another build of the library (make DEMDEF=-DSIFT3D_DEMONS_MASK_SKIP=0: the masked kernel
without its skip)."""
import argparse
import inspect
import os
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


def run(label, reps, trials):
    import torch
    from sift3d_amd import api, hip
    hip.lib()
    print("package: %s" % os.path.dirname(hip.__file__), file=sys.stderr)
    masked = "mask_fixed" in inspect.signature(hip.demons_force).parameters
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    shape = (N, N, N)
    WF = (torch.rand(shape, generator=g, device="cuda") < 0.6).float().contiguous()
    WM = (torch.rand(shape, generator=g, device="cuda") < 0.6).float().contiguous()
    ax = torch.arange(N, device="cuda", dtype=torch.float32) - (N - 1) / 2.0
    r2 = ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2
    radius = (0.375 / 3.141592653589793) ** (1.0 / 3.0) * N              # 4/3 pi r^3 = N^3 / 2
    ball = (r2 <= radius * radius).float().contiguous()
    del r2
    cases = [("none", {}, {})]
    if masked:
        cases += [("random", dict(mask_fixed=WF, mask_moving=WM), dict(mask_fixed=WF, mask_moving=WM)),
                  ("ball", dict(mask_fixed=ball), dict(mask_fixed=ball))]
    print("# masks in demons: the force and one iteration, unmasked against masked, %d^3 float32, MI355X (gfx950)%s"
          % (N, label and "; " + label))
    print("# HIP events around %d back-to-back calls, per call, min of %d trials [min-max of the trials]; random: both "
          "masks random binary, 60 %% in each; ball: mask_fixed a centred ball, mask_moving None" % (reps, trials))
    print("# iteration rows: %d back-to-back calls, each with the copy of the start field (3 planes) that resets it"
          % max(reps // 4, 1))
    print("%-34s %-7s %28s %10s" % ("call", "masks", "ms", "/ unmasked"))
    for nc in (1, 12):
        F = torch.rand((nc,) + shape, device="cuda", generator=g)
        M = torch.rand((nc,) + shape, device="cuda", generator=g)
        W = torch.empty_like(F)
        u = (torch.rand((3,) + shape, device="cuda", generator=g) - 0.5) * 2.0
        uu = torch.empty_like(u)
        step = torch.empty_like(u)
        stats = torch.empty(2, dtype=torch.int64, device="cuda")
        pw = torch.empty(hip.DEMONS_FORCE_WORK_BYTES // 8, dtype=torch.int64, device="cuda")
        work = torch.empty((hip.lib().sift3d_amd_demons_work_floats(N, N, N, nc) + 1) // 2, dtype=torch.float64,
                           device="cuda")
        hip.warp_field(M, W, u)
        base = None
        for name, fkw, _ in cases:
            t = _time(lambda: hip.demons_force(F, W, u, step, 1.0, shape, stats, pw, **fkw), reps, trials)
            base = base or min(t)
            print("%-34s %-7s %9.4f [%.4f-%.4f] %10s" % ("force nc=%d" % nc, name, min(t), min(t), max(t),
                                                         "-" if not fkw else "%.3f" % (min(t) / base)))
            if fkw:
                n = int(hip.demons_stats(hip.demons_force(F, W, u, step, 1.0, shape, stats, pw, **fkw))[1][0])
                print("# counted voxels: %d of %d (%.1f %%)" % (n, N ** 3, 100.0 * n / N ** 3))
        base = None
        for name, _, dkw in cases:
            def it():
                uu.copy_(u)
                hip.demons(F, M, uu, 1, api.DEMONS_ALPHA, api.DEMONS_SIGMA_FLUID, api.DEMONS_SIGMA_DIFFUSION, work,
                           **dkw)
            t = _time(it, max(reps // 4, 1), trials)
            base = base or min(t)
            print("%-34s %-7s %9.4f [%.4f-%.4f] %10s" % ("iteration at the defaults nc=%d" % nc, name, min(t), min(t),
                                                         max(t), "-" if not dkw else "%.3f" % (min(t) / base)))
        del F, M, W, u, uu, step, work
        torch.cuda.empty_cache()


def geometry(n, reps, trials):
    import torch
    from sift3d_amd import hip
    hip.lib()
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    shape = (n, n, n)
    ax = torch.arange(n, device="cuda", dtype=torch.float32) - (n - 1) / 2.0
    r2 = ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2
    radius = (0.375 / 3.141592653589793) ** (1.0 / 3.0) * n
    masks = {"ball": (r2 <= radius * radius).float().contiguous(), "all out": torch.zeros(shape, device="cuda"),
             "all in": torch.ones(shape, device="cuda")}
    del r2
    for name, idx in (("z < N/2", 0), ("y < N/2", 1), ("x < N/2", 2)):
        m = torch.zeros(shape, device="cuda")
        sl = [slice(None)] * 3
        sl[idx] = slice(0, n // 2)
        m[tuple(sl)] = 1.0
        masks[name] = m
    masks["z pairs alternate"] = (torch.arange(n // 4, device="cuda")[:, None, None, None] % 2 == 0).float().expand(
        n // 4, 4, n, n).reshape(shape).contiguous()
    for nc in (1, 12):
        F = torch.rand((nc,) + shape, device="cuda", generator=g)
        W = torch.rand((nc,) + shape, device="cuda", generator=g)
        u = (torch.rand((3,) + shape, device="cuda", generator=g) - 0.5) * 2.0
        step = torch.empty_like(u)
        stats = torch.empty(2, dtype=torch.int64, device="cuda")
        pw = torch.empty(hip.DEMONS_FORCE_WORK_BYTES // 8, dtype=torch.int64, device="cuda")
        t = _time(lambda: hip.demons_force(F, W, u, step, 1.0, shape, stats, pw), reps, trials)
        print("nc=%-2d %-20s %.4f [%.4f-%.4f]" % (nc, "unmasked", min(t), min(t), max(t)), flush=True)
        for name, m in masks.items():
            t = _time(lambda: hip.demons_force(F, W, u, step, 1.0, shape, stats, pw, mask_fixed=m), reps, trials)
            print("nc=%-2d %-20s %.4f [%.4f-%.4f]" % (nc, name, min(t), min(t), max(t)), flush=True)
        del F, W, u, step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--label", default="")
    ap.add_argument("--geometry", action="store_true")
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    _require_built(root)
    sys.path.insert(0, root)
    if a.geometry:
        geometry(a.n, a.reps, a.trials)
    else:
        run(a.label, a.reps, a.trials)


if __name__ == "__main__":
    main()
