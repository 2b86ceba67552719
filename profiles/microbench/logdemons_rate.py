#!/usr/bin/env python3
"""Rates of log-domain demons (sift3d_field_bracket.hip, sift3d_demons.c) at float32 512^3:

    k_field_bracket       both modes; 36 B/voxel (six planes read, three written)
    k_jacobian_det        the gate's yardstick: 16 B/voxel (three read, one written), the same stencil walk
    k_field_compose       one pass (a squaring of the exponential): 24 B/voxel
    one iteration         diffeomorphic, logdomain (bch 0 and 1), symmetric; nc = 12, the api's defaults, Kv = 5

    python3 profiles/microbench/logdemons_rate.py > profiles/microbench/logdemons_rate_mi355x.txt

Device events around back-to-back calls, per call, min of 3 trials after one warm-up, all in one run.
Gate: k_field_bracket<BRACKET> takes no longer than 36 / 16 of k_jacobian_det, the ratio of their algorithmic bytes."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from demons_rate import HBM, _ms  # noqa: E402
from dense_rate import _require_built  # noqa: E402

N = 512
NC = 12
KV = 5


def run():
    import torch
    from sift3d_amd import api, hip
    vox = float(N) ** 3
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    a = (torch.rand((3, N, N, N), device="cuda", generator=g) - 0.5) * 2.0
    b = (torch.rand((3, N, N, N), device="cuda", generator=g) - 0.5) * 2.0
    out = torch.empty_like(a)
    print("# log-domain demons, float32 %d^3, MI355X (gfx950); HIP events around back-to-back calls, per call, min of "
          "3 trials after one warm-up" % N)
    print("%-48s %10s %9s %10s" % ("call", "ms", "alg GB", "frac 8TB/s"))

    def line(name, ms, nbytes):
        print("%-48s %10.4f %9.3f %10.3f" % (name, ms, nbytes / 1e9, (nbytes / HBM * 1e3) / ms if nbytes else 0.0))

    t_br = _ms(lambda: hip.field_bracket(a, b, out, "bracket"), 5)
    t_bch = _ms(lambda: hip.field_bracket(a, b, out, "bch1"), 5)
    det = torch.empty((N, N, N), device="cuda")
    t_jac = _ms(lambda: hip.jacobian_det(a, det), 5)
    t_cmp = _ms(lambda: hip.field_compose(a, b, out, "compose"), 5)
    line("k_field_bracket<BRACKET>", t_br, 36 * vox)
    line("k_field_bracket<BCH1>", t_bch, 36 * vox)
    line("k_jacobian_det (with its init / finish)", t_jac, 16 * vox)
    line("k_field_compose, one pass, field ~ +-1 voxel", t_cmp, 24 * vox)
    print("# gate: k_field_bracket<BRACKET> / k_jacobian_det (same run) = %.3f (must be <= 36 / 16 = 2.25)"
          % (t_br / t_jac))
    del b, out, det
    torch.cuda.empty_cache()
    F = torch.rand((NC, N, N, N), device="cuda", generator=g)
    M = torch.rand((NC, N, N, N), device="cuda", generator=g)
    al, sf, sd = api.DEMONS_ALPHA, api.DEMONS_SIGMA_FLUID, api.DEMONS_SIGMA_DIFFUSION
    print("# one whole iteration, nc = %d, alpha %g, sigma_fluid %g, sigma_diffusion %g, Kv = %d (diffeomorphic: "
          "squarings %d); the state is cloned inside the timed call" % (NC, al, sf, sd, KV, api.demons_squarings(al)))
    work = torch.empty(hip.lib().sift3d_amd_logdemons_work_floats(N, N, N, NC, 1, 1), device="cuda")
    line("clone of the state (in every line below)", _ms(lambda: a.clone(), 3), 24 * vox)
    line("iteration: diffeomorphic",
         _ms(lambda: hip.demons(F, M, a.clone(), 1, al, sf, sd, work, "diffeomorphic", api.demons_squarings(al)), 3), 0)
    for name, sym, bch in (("logdomain, bch 0", False, 0), ("logdomain, bch 1", False, 1),
                           ("symmetric, bch 0", True, 0), ("symmetric, bch 1", True, 1)):
        line("iteration: " + name,
             _ms(lambda: hip.logdemons([F], [M], a.clone(), [1], al, sf, sd, sym, bch, KV, work), 3), 0)


if __name__ == "__main__":
    _require_built()
    np.seterr(all="ignore")
    run()
