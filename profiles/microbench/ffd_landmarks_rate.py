#!/usr/bin/env python3
"""What the landmark term costs an MSD evaluation of the FFD driver: a 256^3 pair at spacing 8 through
sift3d_amd_ffd_refine_device (the entry a call without landmarks goes to) and through
sift3d_amd_ffd_refine_landmarks_device with m = 256, 4096 and 65536 landmarks at weight 0.01.

The drivers run one level; every evaluation is the field, the force, the adjoint, the bending passes, (the landmarks'
value and adjoint passes,) the combine and one wait for the record, so a driver call of E evaluations costs a + E * t with
a the set-up of the call (the weight tables, the zero lattice, the landmarks' ordering and upload, the final field).  Each
driver is timed at E = 4 and E = 12 with a host clock around the call, which ends in a device synchronise; t = (T12 - T4)
/ 8 and a = T4 - 4 t.  tol is set so small and min_overlap to 0 so that no call stops before its E evaluations (the trail's
length is checked).  After one warm-up call of each, the calls take turns trial by trial; the median of the trials and
their spread are printed.

The volumes are affine_refine_rate.py's; the landmarks are uniform over the grid with Q = P + a smooth displacement of
2 voxels, so that the term has something to pull.

    python3 profiles/microbench/ffd_landmarks_rate.py [--label TEXT] > OUT.txt

One process, meant to run under a `timeout` of its own (two minutes are ample)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from affine_refine_rate import _volumes  # noqa: E402
from similarity_rate import _require_built  # noqa: E402

SPACING = (8, 8, 8)
COUNTS = (256, 4096, 65536)
EVALS = (4, 12)
WEIGHT = 0.01


def _landmarks(m, n):
    rng = np.random.default_rng(m)
    P = rng.uniform(0.0, n - 1.0, (m, 3))
    Q = P + 2.0 * np.sin(2.0 * np.pi * P[:, [1, 2, 0]] / n)
    return P, Q


def run(label, trials, n):
    import torch
    from sift3d_amd import hip
    F, M = _volumes(n)
    L = hip.lib()
    work = torch.empty(L.sift3d_amd_ffd_refine_landmarks_work_bytes(n, n, n, n, n, n, *SPACING, 1, max(COUNTS)),
                       dtype=torch.uint8, device="cuda")

    def params(E):
        return hip.ffd_refine_params(spacing=SPACING, levels=1, max_evaluations=E, tol=1e-30, min_overlap=0.0)

    def plain(E):
        res = hip.ffd_refine(F, M, None, params(E), work)[0]
        assert res.evaluations == E, res.evaluations

    def with_landmarks(E, P, Q):
        res = hip.ffd_refine_landmarks(F, M, P, Q, None, WEIGHT, params=params(E), work=work)[0]
        assert res.evaluations == E, res.evaluations

    calls = [("without landmarks (sift3d_amd_ffd_refine_device)", plain)]
    for m in COUNTS:
        P, Q = _landmarks(m, n)
        calls.append(("m = %d" % m, lambda E, P=P, Q=Q: with_landmarks(E, P, Q)))
    times = {(name, E): [] for name, _ in calls for E in EVALS}
    for name, fn in calls:                                               # the warm-up
        for E in EVALS:
            fn(E)
    for _ in range(trials):
        for name, fn in calls:
            for E in EVALS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(E)
                times[(name, E)].append((time.perf_counter() - t0) * 1e3)
    print("# one MSD evaluation of the FFD driver without and with the landmark term, %d^3, spacing 8, one level, float32, "
          "MI355X (gfx950)%s" % (n, label and "; " + label))
    print("# host clock around a driver call of E = %d and of E = %d evaluations, ms; median of %d alternating trials "
          "[min-max]; per evaluation t = (T%d - T%d) / %d, per call a = T%d - %d t"
          % (EVALS[0], EVALS[1], trials, EVALS[1], EVALS[0], EVALS[1] - EVALS[0], EVALS[0], EVALS[0]))
    base = None
    for name, _ in calls:
        lo, hi = times[(name, EVALS[0])], times[(name, EVALS[1])]
        per = [(b - a) / (EVALS[1] - EVALS[0]) for a, b in zip(lo, hi)]
        t = statistics.median(per)
        a = statistics.median(lo) - EVALS[0] * t
        base = t if base is None else base
        print("%-52s T%d %8.3f [%.3f-%.3f]  T%d %8.3f [%.3f-%.3f]  t %7.3f [%.3f-%.3f]  a %7.3f  t / t(without) %.4f"
              % (name, EVALS[0], statistics.median(lo), min(lo), max(lo), EVALS[1], statistics.median(hi), min(hi),
                 max(hi), t, min(per), max(per), a, t / base))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    _require_built()
    run(a.label, a.trials, a.size)


if __name__ == "__main__":
    main()
