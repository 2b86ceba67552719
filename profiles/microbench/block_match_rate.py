#!/usr/bin/env python3
"""Cost of block matching (include/sift3d_amd.h, "Block matching") at 256^3, radius 1, 3 and 6, in one run:

    (a) one sift3d_hip_block_match, warm, no masks
    (b) one driver iteration on one level (sift3d_amd_block_register_device, levels 1, iterations 1, rigid): two
        warps, the match, the copy of the records to the host with its wait, selection and the trimmed fit
    (c) one evaluation of the affine refinement (sift3d_hip_affine_normal_eqs and the read of its record), whose code
        this change does not touch: the parent commit's figure, for orientation only

For (a) the counted work over the time is reported against the part's peaks.  Counted: per block and candidate 64
voxels, each one double add and two double FMAs (3 f64 operations, "DFMA" below) and one 4-byte LDS read; the six
recomputed neighbours and the staging are left out of the count and in the time.  Peaks: 256 CUs x 4 SIMDs x 16 f64
lanes x 2.4 GHz = 39.3e12 f64 operations / s; ds_read_b32 75 TB/s chip-wide.  There is no pass / fail number: the file
is the record.

Times (a) are HIP events around `reps` back-to-back calls, per call, the minimum of `trials` trials after a warm-up,
with the spread beside it.  (b) and (c) wait for the host, so they are wall-clock times around a call that ends with
the stream idle.  Run it with the device to itself.

    python3 profiles/microbench/block_match_rate.py [--label TEXT] [--variants DIR] > OUT.txt

SIFT3D_AMD_LIB selects another build of the library (make BMDEF="-DSIFT3D_BM_J=2": two candidates per lane and pass;
-DSIFT3D_BM_OPAQUE=0: F promoted once per block; -DSIFT3D_BM_TBX/TBY/TBZ=: another tile of blocks per workgroup).
--variants DIR runs (a) once more in a fresh process for every lib_*.so in DIR."""
import argparse
import glob
import os
import subprocess
import sys
import time

N = 256
PEAK_F64 = 256 * 4 * 16 * 2.4e9
PEAK_LDS = 75e12


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


def _wall(fn, trials):
    import torch
    fn()
    ms = []
    for _ in range(trials):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return ms


def _volumes():
    import torch
    from sift3d_amd import hip
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    M = torch.rand((N, N, N), device="cuda", generator=g)
    F = torch.empty_like(M)
    hip.warp_affine(M, F, [[1, 0.01, 0, 0.4], [-0.01, 1, 0, -0.3], [0, 0, 1, 0.2]])
    F.mul_(torch.linspace(0.6, 1.4, N, device="cuda")[None, None, :])
    return F, M


def match_rows(tag, reps, trials):
    from sift3d_amd import hip
    hip.lib()
    F, M = _volumes()
    for r in (1, 3, 6):
        t = _time(lambda: hip.block_match(F, M, r), reps if r < 6 else max(reps // 4, 1), trials)
        work = (N // 4) ** 3 * (2 * r + 1) ** 3 * 64
        s = min(t) * 1e-3
        print("%-34s R=%d %9.4f [%.4f-%.4f]  %6.2f T f64 op/s = %4.1f %% of peak; LDS %6.2f TB/s = %4.1f %%"
              % ("block_match (%s)" % tag, r, min(t), min(t), max(t), 3 * work / s / 1e12,
                 100 * 3 * work / s / PEAK_F64, 4 * work / s / 1e12, 100 * 4 * work / s / PEAK_LDS), flush=True)


def other_rows(trials):
    from sift3d_amd import hip
    F, M = _volumes()
    A = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]
    for r in (1, 3, 6):
        p = hip.block_register_params(levels=1, iterations=1, radius=r)
        t = _wall(lambda: hip.block_register(F, M, A, p), trials)
        print("%-34s R=%d %9.4f [%.4f-%.4f]" % ("driver iteration, rigid (wall)", r, min(t), min(t), max(t)),
              flush=True)
    t = _wall(lambda: hip.affine_normal_equations(F, M, A), trials)
    print("%-38s %9.4f [%.4f-%.4f]" % ("affine refinement evaluation (wall)", min(t), min(t), max(t)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--label", default="")
    ap.add_argument("--variants", default=None, help="a directory of lib_*.so builds: the match rows of each")
    ap.add_argument("--match-only", default=None, metavar="TAG", help="only the match rows, under this tag")
    a = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, root)
    if a.match_only:
        match_rows(a.match_only, a.reps, a.trials)
        return
    print("# block matching at %d^3 float32, MI355X (gfx950)%s" % (N, a.label and "; " + a.label))
    print("# match: HIP events around %d back-to-back calls (R=6: %d), per call, min of %d trials [min-max]; ms"
          % (a.reps, max(a.reps // 4, 1), a.trials))
    match_rows("this build", a.reps, a.trials)
    other_rows(a.trials)
    for lib in sorted(glob.glob(os.path.join(a.variants, "lib_*.so")) if a.variants else []):
        # a fresh process: the library is bound once per process
        sys.stdout.flush()
        env = dict(os.environ, SIFT3D_AMD_LIB=os.path.abspath(lib))
        subprocess.run([sys.executable, os.path.abspath(__file__), "--match-only",
                        os.path.basename(lib)[4:-3], "--reps", str(a.reps), "--trials", str(a.trials)], check=True,
                       env=env, timeout=300)


if __name__ == "__main__":
    main()
