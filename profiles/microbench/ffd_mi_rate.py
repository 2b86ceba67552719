#!/usr/bin/env python3
"""Time of the two new kernels of the mutual-information free-form deformation at 512^3 beside their existing
counterparts, alternating, in one process: the Parzen histogram through a field (sift3d_hip_parzen_hist_field) against
the one through an affine map (sift3d_hip_parzen_hist_affine), and the MI evaluation (sift3d_hip_ffd_mi_evaluate, whose
force pass is k_ffd_mi_force) against the MSD evaluation (sift3d_hip_ffd_evaluate, k_ffd_force), each at B = 32 and 64,
on the two contents of affine_mi_rate.py (the lattice with a noise floor; the sum of wide Gaussians under the hump map).

The histogram pair samples the same points: the field is the export of the affine map (a rotation of 5 degrees about
(1, 2, 3) through the centre), 12 B more read per voxel in the place of the pull map's arithmetic.  The two evaluations
differ in the force kernel alone (and in a factor of the combine pass): they share the field export, the adjoint, the
bending passes and the lattice (spacing 8, random, amplitude 1 voxel, added to the same affine map), so the difference
of their times is the difference of the two force kernels.  The force pass's own traffic is 24 B stored and 20 B read
per voxel: 5.9 GB at 512^3, 0.74 ms at 8 TB/s.

Times are HIP events around `reps` back-to-back calls (a quarter as many of an evaluation), per call, the minimum of 3
trials after a warm-up; a pair's two members alternate trial by trial.  The kernels' own durations come from a kernel trace of a run of their own:

    python3 profiles/microbench/ffd_mi_rate.py [--label TEXT] > OUT.txt
    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python3 profiles/microbench/ffd_mi_rate.py --launches
    python3 profiles/microbench/ffd_mi_rate.py --report DIR >> OUT.txt

--launches issues, per content and B, five alternating calls of each of the four entries after a warm-up.  --report
needs no GPU.  Registers and occupancy are the compiler's (`hipcc -Rpass-analysis=kernel-resource-usage`); pass them in
--label to keep them with the numbers."""
import argparse
import csv
import glob
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from affine_mi_rate import _smooth  # noqa: E402
from affine_refine_rate import _volumes  # noqa: E402
from similarity_rate import _require_built, _rot  # noqa: E402

PEAK_BPS = 8.0e12
SPACING = (8, 8, 8)
KERNELS = ("k_parzen_hist", "k_ffd_force", "k_ffd_mi_force")


def _alternate(fns, reps, trials=3):
    """[ms per call of each fn, one entry per trial]: the fns take turns, trial by trial"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in fns:
        for _ in range(2):
            fn()
    out = [[] for _ in fns]
    for _ in range(trials):
        for k, fn in enumerate(fns):
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) / reps)
    return out


def _setup(n, make):
    """the volumes, the affine map, its exported field, a lattice and the buffers of one content"""
    import torch
    from sift3d_amd import api, hip
    F, M = make(n)
    c = np.full(3, (n - 1) / 2.0)
    R = _rot((1.0, 2.0, 3.0), 5.0)
    A = np.hstack([R, (c - R @ c)[:, None]])
    field = api.displacement_field(A, (n, n, n))
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    lattice = torch.rand(hip.ffd_lattice_shape((n, n, n), SPACING), generator=g, device="cuda") * 2.0 - 1.0
    rf, rm = (float(F.min()), float(F.max())), (float(M.min()), float(M.max()))
    hwork = torch.empty(hip.SIMILARITY_GRID * 8, dtype=torch.uint8, device="cuda")
    ework = torch.empty(hip.lib().sift3d_amd_ffd_evaluate_work_bytes(n, n, n, *SPACING), dtype=torch.uint8,
                        device="cuda")
    return F, M, A, field, lattice, rf, rm, hwork, ework


def _calls(hip, s, bins):
    """the four entries as closures (and the table W of the histogram through the lattice's field)"""
    import torch
    F, M, A, field, lattice, rf, rm, hwork, ework = s
    ph = torch.empty((bins, bins), dtype=torch.int64, device="cuda")
    _, _, lfield = hip.ffd_evaluate(F, M, lattice, SPACING, A, 0.005, ework)
    hip.parzen_histogram_field(F, M, lfield, bins, rf, rm, ph, hwork)
    me = hip.parzen_mi(ph)
    W = torch.from_numpy(me.W).cuda()
    del lfield
    return me, ph, [lambda: hip.parzen_histogram(F, M, A, bins, rf, rm, ph, hwork),
                    lambda: hip.parzen_histogram_field(F, M, field, bins, rf, rm, ph, hwork),
                    lambda: hip.ffd_evaluate(F, M, lattice, SPACING, A, 0.005, ework),
                    lambda: hip.ffd_mi_evaluate(F, M, lattice, SPACING, W, rf, rm, A, 0.005, ework)]


def run(label, reps, n):
    from sift3d_amd import hip
    print("# the field histogram against the affine histogram, the MI evaluation against the MSD evaluation, float32, "
          "LINEAR, MI355X (gfx950)%s" % (label and "; " + label))
    print("# HIP events around %d (histograms) or %d (evaluations) back-to-back calls, per call, min of 3 alternating "
          "trials [spread]; the evaluations share everything but the force kernel" % (reps, max(reps // 4, 2)))
    print("%-8s %-6s %-28s %26s %13s" % ("content", "size", "call", "ms", "/ its sibling"))
    for content, make in (("lattice", _volumes), ("smooth", _smooth)):
        s = _setup(n, make)
        notes = []
        for bins in (32, 64):
            me, ph, (ha, hf, em, ei) = _calls(hip, s, bins)
            ta, tf = _alternate([ha, hf], reps)
            tm, ti = _alternate([em, ei], max(reps // 4, 2))
            _, ca = hip.parzen_histogram(s[0], s[1], s[2], bins, s[5], s[6], ph, s[7])
            ca = int(ca[0])
            _, cf = hip.parzen_histogram_field(s[0], s[1], s[3], bins, s[5], s[6], ph, s[7])
            rows = [("parzen_hist_affine B=%d" % bins, ta, "-"),
                    ("parzen_hist_field B=%d" % bins, tf, "%.3f" % (min(tf) / min(ta))),
                    ("ffd_evaluate (msd)", tm, "-"),
                    ("ffd_mi_evaluate B=%d" % bins, ti, "%.3f" % (min(ti) / min(tm)))]
            for name, t, rel in rows:
                print("%-8s %-6s %-28s %8.4f [%.4f-%.4f] %13s" % (content, "%d^3" % n, name, min(t), min(t), max(t),
                                                                  rel))
            print("%-8s %-6s %-28s %8.4f" % (content, "%d^3" % n, "mi force - msd force B=%d" % bins,
                                             min(ti) - min(tm)))
            notes.append("B=%d: counted %d (affine) %d (field), mi through the lattice %.6f" % (bins, ca, int(cf[0]),
                                                                                              me.mi))
        print("# %s %d^3: %s" % (content, n, "; ".join(notes)))
        del s


def launches(n):
    import torch
    from sift3d_amd import hip
    for content, make in (("lattice", _volumes), ("smooth", _smooth)):
        s = _setup(n, make)
        for bins in (32, 64):
            _, _, fns = _calls(hip, s, bins)
            for _ in range(6):                                           # the first round is the warm-up
                for fn in fns:
                    fn()
            torch.cuda.synchronize()
        del s
    print("launches: 2 contents x B = 32, 64 x (1 + 1 setup, 6 rounds) of the four entries")


def report(d, n):
    """the kernels' own durations from a kernel trace of --launches: in the trace's order the contents and bins follow
    each other, a setup evaluation and histogram first, then six rounds of which the first is dropped"""
    rows = []
    for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)):
        with open(f) as fh:
            rows += [r for r in csv.DictReader(fh)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    seq = []
    for r in rows:
        name = r["Kernel_Name"]
        if "k_ffd_mi_force" in name:
            kn = "k_ffd_mi_force"
        elif "k_ffd_force" in name:
            kn = "k_ffd_force"
        elif "k_parzen_hist" in name and "finish" not in name:           # FIELD is the last template argument
            field = re.search(r"k_parzen_hist<[^>]*true\s*>", name) or re.search(r"k_parzen_histILi\dELb\dELb1E", name)
            kn = "k_parzen_hist<field>" if field else "k_parzen_hist"
        else:
            continue
        seq.append((kn, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6))
    if not seq:
        sys.exit("no kernel of %s in %s" % (KERNELS, d))
    per = len(seq) // 4                                                  # (content, bins) groups
    print("# the kernels' own durations (rocprofv3 --kernel-trace of --launches), ms, min of 5 [spread]; floor of the "
          "force pass's traffic (44 B / voxel at 8 TB/s): %.3f ms" % (44.0 * float(n) ** 3 / PEAK_BPS * 1e3))
    k = 0
    for content in ("lattice", "smooth"):
        for bins in (32, 64):
            grp = seq[k * per:(k + 1) * per]
            k += 1
            names = ("k_parzen_hist", "k_parzen_hist<field>", "k_ffd_force", "k_ffd_mi_force")
            t = {nm: [v for kn, v in grp if kn == nm] for nm in names}
            t = {nm: v[-5:] for nm, v in t.items()}                      # drop setup and warm-up
            for nm, sib in (("k_parzen_hist", None), ("k_parzen_hist<field>", "k_parzen_hist"), ("k_ffd_force", None),
                            ("k_ffd_mi_force", "k_ffd_force")):
                v = t[nm]
                print("%-8s %-6s %-28s %8.4f [%.4f-%.4f] %13s" % (
                    content, "%d^3" % n, "%s B=%d" % (nm, bins), min(v), min(v), max(v),
                    "-" if sib is None else "%.3f" % (min(v) / min(t[sib]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--label", default="")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--report", default="")
    a = ap.parse_args()
    if a.report:
        return report(a.report, a.size)
    _require_built()
    if a.launches:
        return launches(a.size)
    run(a.label, a.reps, a.size)


if __name__ == "__main__":
    main()
