#!/usr/bin/env python3
"""Generate tests/golden/*.npz from the UNMODIFIED reference -- TEST INFRASTRUCTURE ONLY.

Runs only in the build container (needs oracle/_ref/, i.e. /root/reference):

    make -C oracle ref && OMP_NUM_THREADS=1 python oracle/make_golden.py [--big]

Inputs are produced by this repository's own seeded generators (sift3d_amd/csrc/synth.c)
or numpy's PCG64, so only OUTPUTS of the reference are stored.  The fixtures pin the CPU
restatement (oracle/sift3d_oracle.c) and, through it and directly, the HIP path.

Fixture families:
  g1_filters   Gaussian taps for the default bank and a sweep of sigmas
  g2_fir       1-D interpolating FIR per axis, three widths x units 1/2/4 (+ anisotropic)
  g3_*         end-to-end dumps: level digests, small levels in full, dogmax-free
               candidate list, keypoints (R, sd, stale strength), descriptors, sort order
               (g3_spikes64, g3_integer48, g3_subnormal48: zero-background, integer and subnormal inputs)
  g5_*         larger volumes: candidate/keypoint lists, R, descriptor subset + row sums
  g6_abi       the names the reference library exports and its CLI imports (JSON)
  g7_*         describe on caller-made keypoint lists
  g8_*         assign_eig_ori on caller-made candidate lists: status, conf, R per entry
  g9_*         detect_extrema on caller-made DoG levels (ties, thresholds, borders, subnormal and
               overflowing levels, both builds): the recipes and the reference's records
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle import refprobe  # noqa: E402
from oracle import sift3d_oracle as so  # noqa: E402
from tests import pyramid_content  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def desc_projection(h):
    """Every histogram row projected on 8 seeded random unit vectors (N x 8 float64).  Pins ALL
    rows of a large fixture -- which bin the mass of a row sits in, not only its sum
    (reference binning: sift3d/sift.c:1355-1373, 1514-1526) -- in 64 bytes per row.  The
    columns have unit 2-norm, so an elementwise relative error e of the row moves a projection
    by at most e * |row|_2."""
    P = np.random.default_rng(20240768).standard_normal((768, 8))
    P /= np.linalg.norm(P, axis=0, keepdims=True)
    return np.ascontiguousarray(h, np.float64) @ P


def digest(a):
    """sha1 over float32 values with -0.0 folded into +0.0."""
    a = np.ascontiguousarray(a, np.float32) + np.float32(0.0)
    return hashlib.sha1(a.tobytes()).hexdigest()


def g1_filters():
    sigmas = [0.3, 0.5387011637869722, 0.8, 0.9732939207323564, 1.0, 1.2262734984654078,
              1.5450077936447955, 1.9465878414647133, 2.0, 2.4525469969308156, 3.3, 5.0,
              0.0]
    d = {"sigmas": np.array(sigmas)}
    for i, s in enumerate(sigmas):
        d["taps_%d" % i] = refprobe.gauss_filter(s)
    p = refprobe.Probe()
    vol = so.synth_survey(16, nblob=4)
    assert p.detect(vol) == 0
    bank = p.gss()
    d["bank_sigma"] = np.array([s for s, _ in bank])
    for i, (_, t) in enumerate(bank):
        d["bank_%d" % i] = t
    p.close()
    np.savez_compressed(os.path.join(OUT, "g1_filters.npz"), **d)
    return {"g1_filters": len(sigmas)}


def g2_fir():
    rng = np.random.Generator(np.random.PCG64(20240917))
    dims = (21, 13, 9)  # nx, ny, nz ; nz = 9 with the 17-tap filter is the hw ~ n corner
    vol = rng.standard_normal((dims[2], dims[1], dims[0])).astype(np.float32)
    d = {"vol": vol}
    widths = {5: 0.5387011637869722, 9: 1.2262734984654078, 17: 2.4525469969308156}
    cases = []
    for w, sg in widths.items():
        taps = refprobe.gauss_filter(sg)
        assert len(taps) == w
        d["taps_w%d" % w] = taps
        for u in (1.0, 2.0, 4.0):
            for ax in range(3):
                key = "axis%d_w%d_u%g" % (ax, w, u)
                d[key] = refprobe.fir_axis(vol, taps, ax, units=(u, u, u), unit=1.0)
                cases.append(key)
    # asymmetric (non-Gaussian) taps: catches a reversed tap order
    at = rng.standard_normal(7).astype(np.float32)
    d["taps_asym"] = at
    for u in (1.0, 2.0):
        for ax in range(3):
            key = "axis%d_asym_u%g" % (ax, u)
            d[key] = refprobe.fir_axis(vol, at, ax, units=(u, u, u), unit=1.0)
            cases.append(key)
    # full 3-axis application, incl. anisotropic (non-dyadic unit factors) and unit=-1
    vol2 = rng.standard_normal((17, 20, 24)).astype(np.float32)
    d["vol2"] = vol2
    for name, units, unit in (("iso1", (1, 1, 1), 1.0), ("iso2", (2, 2, 2), 1.0),
                              ("iso4", (4, 4, 4), 1.0), ("aniso", (1.0, 1.5, 0.7), 1.0),
                              ("aniso3", (3.0, 0.9, 6.0), 1.0), ("default", (2, 2, 2), -1.0)):
        for w in (5, 17):
            key = "blur_%s_w%d" % (name, w)
            d[key] = refprobe.apply_sep_fir(vol2, d["taps_w%d" % w], units=units, unit=unit)
            cases.append(key)
    d["units_aniso"] = np.array([1.0, 1.5, 0.7])
    d["units_aniso3"] = np.array([3.0, 0.9, 6.0])
    d["down"] = refprobe.downsample(vol2)
    d["down_odd"] = refprobe.downsample(vol)
    # eigen: a few SPD matrices
    As, Qs, Ls = [], [], []
    for _ in range(16):
        m = rng.standard_normal((3, 3))
        A = m @ m.T
        Q, L = refprobe.eigen3(A)
        As.append(A)
        Qs.append(Q)
        Ls.append(L)
    d["eig_A"] = np.array(As)
    d["eig_Q"] = np.array(Qs)
    d["eig_L"] = np.array(Ls)
    np.savez_compressed(os.path.join(OUT, "g2_fir.npz"), **d)
    return {"g2_fir": len(cases)}


def end_to_end(name, vol, units=(1, 1, 1), full_levels_below=17, desc_stride=1, params=None,
               store_levels=True, input_spec=None):
    params = params or {}
    p = refprobe.Probe(**params)
    t0 = time.time()
    assert p.detect(vol, units) == 0
    t_detect = time.time() - t0
    K = params.get("num_kp_levels") or 3
    d = {"units": np.array(units, np.float64), "dims": np.array(vol.shape[::-1], np.int32),
         "input_digest": np.array(digest(vol)), "num_octaves": np.array(p.num_octaves)}
    for k, v in params.items():
        d["param_" + k] = np.array(v)
    dig = {}
    for o in range(p.num_octaves):
        for which, n in ((0, K + 3), (1, K + 2)):
            for s in range(-1, n - 1):
                a, u, sc = p.level(which, o, s)
                key = "%s_o%d_s%d" % ("G" if which == 0 else "D", o, s)
                dig[key] = digest(a)
                d["scale_" + key] = np.array(sc)
                d["lunits_" + key] = u
                if store_levels and max(a.shape) < full_levels_below:
                    d["level_" + key] = a
    a, _, _ = p.level(2, 0, 0)
    dig["IM"] = digest(a)
    d["digests"] = np.array(json.dumps(dig))
    c = p.candidates()
    d["cand_osxyz"] = c["osxyz"]
    d["cand_strength"] = c["strength"]
    d["cand_sd"] = c["sd"]
    k = p.keypoints()
    d["kp_os"] = k["os"]
    d["kp_xyzsd"] = k["xyzsd"]
    d["kp_strength"] = k["strength"]
    d["kp_R"] = k["R"]
    t_desc = 0.0
    if len(k["strength"]):
        d["kp_mat"] = p.kp_mat()
        t0 = time.time()
        assert p.describe() == 0
        t_desc = time.time() - t0
        h, x = p.descriptors()
        d["desc_idx"] = np.arange(0, len(h), desc_stride, dtype=np.int32)
        d["desc_hist"] = h[::desc_stride]
        d["desc_xyzsd"] = x
        d["desc_rowsum"] = h.astype(np.float64).sum(axis=1)
        d["desc_rowsumsq"] = (h.astype(np.float64) ** 2).sum(axis=1)
        d["desc_proj"] = desc_projection(h)
        # sort_by_strength(limit): resulting order expressed as (o,s,x,y,z,strength) rows
        for lim in (0, 10):
            q = refprobe.Probe(**params)
            assert q.detect(vol, units) == 0
            q.sort(lim)
            kk = q.keypoints()
            d["sort%d_os" % lim] = kk["os"]
            d["sort%d_xyzsd" % lim] = kk["xyzsd"]
            d["sort%d_strength" % lim] = kk["strength"]
            q.close()
    if input_spec:
        d["input_spec"] = np.array(json.dumps(input_spec))
    d["ref_time_detect_s"] = np.array(t_detect)
    d["ref_time_describe_s"] = np.array(t_desc)
    p.close()
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **d)
    return {name: dict(cand=int(len(c["sd"])), kp=int(len(k["strength"])),
                       t_detect=round(t_detect, 2), t_describe=round(t_desc, 2))}


def end_to_end_content(case):
    """g3_<case>: a volume of tests/pyramid_content.py (zero background, integers, a subnormal input) with the
    detector parameters that belong to it."""
    vol, kw = pyramid_content.detect_volume(case, so)
    return end_to_end("g3_" + case, vol, params=kw,
                      input_spec=dict(gen="content", case=case, seed=pyramid_content.DETECT_SEED))


def end_to_end_digest(name, vol, stride=97, input_spec=None):
    """Full-size case: the reference's results as sha1 digests plus strided samples (small file)."""
    p = refprobe.Probe()
    t0 = time.time()
    assert p.detect(vol, (1, 1, 1)) == 0
    t_detect = time.time() - t0
    d = {"dims": np.array(vol.shape[::-1], np.int32), "input_digest": np.array(digest(vol)),
         "num_octaves": np.array(p.num_octaves), "stride": np.array(stride)}
    dig = {}
    for o in range(p.num_octaves):
        for which, n in ((0, 6), (1, 5)):
            for s in range(-1, n - 1):
                a, _, _ = p.level(which, o, s)
                dig["%s_o%d_s%d" % ("G" if which == 0 else "D", o, s)] = digest(a)
    c = p.candidates()
    k = p.keypoints()
    d["ncand"] = np.array(len(c["sd"]))
    d["nkp"] = np.array(len(k["strength"]))
    dig["cand_osxyz"] = digest(np.ascontiguousarray(c["osxyz"]))
    dig["kp_os"] = digest(np.ascontiguousarray(k["os"]))
    dig["kp_xyzsd"] = digest(np.ascontiguousarray(k["xyzsd"]))
    dig["kp_strength"] = digest(np.ascontiguousarray(k["strength"]))
    dig["kp_R"] = digest(np.ascontiguousarray(k["R"]))
    d["kp_idx"] = np.arange(0, len(k["strength"]), stride, dtype=np.int32)
    d["kp_os_s"] = k["os"][::stride]
    d["kp_xyzsd_s"] = k["xyzsd"][::stride]
    d["kp_strength_s"] = k["strength"][::stride]
    d["kp_R_s"] = k["R"][::stride]
    t0 = time.time()
    assert p.describe() == 0
    t_desc = time.time() - t0
    h, x = p.descriptors()
    dig["desc_hist"] = digest(np.ascontiguousarray(h))
    d["desc_hist_s"] = h[::stride]
    d["desc_rowsum"] = h.astype(np.float64).sum(axis=1).astype(np.float32)
    d["desc_proj"] = desc_projection(h)
    d["desc_rownorm"] = np.sqrt((h.astype(np.float64) ** 2).sum(axis=1))
    d["digests"] = np.array(json.dumps(dig))
    if input_spec:
        d["input_spec"] = np.array(json.dumps(input_spec))
    d["ref_time_detect_s"] = np.array(t_detect)
    d["ref_time_describe_s"] = np.array(t_desc)
    p.close()
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **d)
    return {name: dict(cand=int(d["ncand"]), kp=int(d["nkp"]), t_detect=round(t_detect, 2),
                       t_describe=round(t_desc, 2))}


def g4_csv():
    """Files written by the reference's own sift3d_keypoint_store_save /
    sift3d_descriptor_store_save (sift.c:1741-1830 via write_Mat_rm, imutil.c:405-479), plain and
    gzip, for the g3_64 volume -- as DATA: the whole keypoint file (a few KB of numbers), sha1 +
    size + first / last rows of the descriptor file, and the records they were written from."""
    import gzip
    import hashlib
    import tempfile
    vol = so.synth_survey(64)
    p = refprobe.Probe()
    assert p.detect(vol) == 0 and p.describe() == 0
    k = p.keypoints()
    h, x = p.descriptors()
    d = {"kp_os": k["os"], "kp_xyzsd": k["xyzsd"], "kp_strength": k["strength"], "kp_R": k["R"],
         "desc_hist": h, "desc_xyzsd": x, "dims": np.array(vol.shape[::-1], np.int32)}
    with tempfile.TemporaryDirectory() as t:
        kp, dp = os.path.join(t, "kp.csv"), os.path.join(t, "desc.csv")
        assert p.save(kp, dp) == 0
        assert p.save(kp + ".gz", dp + ".gz") == 0
        ktxt, dtxt = open(kp, "rb").read(), open(dp, "rb").read()
        assert gzip.open(kp + ".gz", "rb").read() == ktxt and gzip.open(dp + ".gz", "rb").read() == dtxt
    rows = dtxt.split(b"\n")
    d["kp_csv"] = np.frombuffer(ktxt, np.uint8)
    d["desc_csv_sha1"] = np.array(hashlib.sha1(dtxt).hexdigest())
    d["desc_csv_bytes"] = np.array(len(dtxt))
    d["desc_csv_first_row"] = np.frombuffer(rows[0], np.uint8)
    d["desc_csv_last_row"] = np.frombuffer(rows[-2] if rows[-1] == b"" else rows[-1], np.uint8)
    d["desc_csv_ends_with_newline"] = np.array(dtxt.endswith(b"\n"))
    p.close()
    np.savez_compressed(os.path.join(OUT, "g4_csv.npz"), **d)
    return {"g4_csv": dict(kp=int(len(k["strength"])), kp_csv_bytes=len(ktxt), desc_csv_bytes=len(dtxt))}


def _rotation(rng, reflect=False):
    """A random orthonormal matrix (QR of a Gaussian one), det +1, or det -1 with `reflect`."""
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if (np.linalg.det(q) < 0) != reflect:
        q[:, 0] = -q[:, 0]
    return q.astype(np.float32)


def _steps_volume(n, seed):
    """An axis-aligned step volume: plane x = i holds one PCG64 normal value (every gradient of the
    interior points along x)."""
    nx, ny, nz = n
    c = np.random.Generator(np.random.PCG64(seed)).standard_normal(nx).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(c, (nz, ny, nx)), np.float32)


def g7_keypoints(name, vol, input_spec, units=(1, 1, 1), make_lists=None):
    """Describe on CALLER-MADE keypoint lists (sift.c:1171-1212, 1442-1596): the reference's pyramid of `vol`,
    then each list of make_lists(probe, rng) -- {case: (os (n, 2), xyzsd (n, 4), R (n, 3, 3))} -- through its
    own keypoint store.  Stored per case: the list, the reference's verdict (verify_keys), and for accepted
    lists every descriptor row, desc xyzsd and the projections."""
    p = refprobe.Probe()
    assert p.detect(vol, units) == 0
    d = {"units": np.array(units, np.float64), "dims": np.array(vol.shape[::-1], np.int32),
         "input_digest": np.array(digest(vol)), "num_octaves": np.array(p.num_octaves),
         "input_spec": np.array(json.dumps(input_spec))}
    rng = np.random.Generator(np.random.PCG64(int(hashlib.sha1(name.encode()).hexdigest()[:8], 16)))
    lists = make_lists(p, rng)
    info = {}
    for case, (os_, xyzsd, R) in lists.items():
        os_ = np.asarray(os_, np.int32).reshape(-1, 2)
        xyzsd = np.asarray(xyzsd, np.float64).reshape(-1, 4)
        R = np.asarray(R, np.float32).reshape(-1, 3, 3)
        assert p.set_keypoints(os_, xyzsd, R) == 0
        ok = p.describe() == 0
        d[case + "_os"], d[case + "_xyzsd"], d[case + "_R"] = os_, xyzsd, R
        d[case + "_ok"] = np.array(ok)
        if ok:
            h, x = p.descriptors()
            assert len(h) == len(os_)
            d[case + "_hist"] = h
            d[case + "_desc_xyzsd"] = x
            d[case + "_proj"] = desc_projection(h)
        info[case] = int(len(os_)) if ok else "refused"
    d["cases"] = np.array(json.dumps(list(lists)))
    p.close()
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **d)
    return {name: info}


def _level_sd(p, o, s):
    return p.level(0, o, s)[2]


def _level_dims(p, o):
    return [int(v) for v in p.level(0, o, 0)[0].shape[::-1]]


def _g7_survey64_lists(p, rng):
    K = 3
    lists = {}

    def mk(rows, Rs):
        return (np.array([(o, s) for o, s, _, _ in rows]), np.array([list(c) + [sd] for _, _, c, sd in rows]),
                np.array(Rs, np.float32))

    def centre(o, frac, margin=4):
        n = _level_dims(p, o)
        c = [rng.uniform(margin, v - margin) for v in n]
        return [v if frac else float(np.floor(v)) for v in c]

    # sub-voxel centres at the level's own sd: the weights are computed per voxel, fractional bounds
    rows = [(o, s, centre(o, True), _level_sd(p, o, s)) for o in (0, 1) for s in (0, 1, 2) for _ in range(2)]
    lists["subvox"] = mk(rows, [_rotation(rng) for _ in rows])
    # integer centres, sd one ulp off the level's (the table is rejected by the bits alone) -- and on it
    rows = []
    for o in (0, 1):
        for s in (0, 1, 2):
            sd = _level_sd(p, o, s)
            c = centre(o, False)
            rows += [(o, s, c, np.nextafter(sd, np.inf)), (o, s, c, np.nextafter(sd, 0.0)), (o, s, c, sd)]
    lists["ulp"] = mk(rows, [_rotation(rng) for _ in rows])
    # 0.5x and 2x the level's sd; tiny sd (a window of at most one voxel, or none: a zero histogram)
    rows = []
    for o in (0, 1):
        for s in (0, 2):
            sd = _level_sd(p, o, s)
            rows += [(o, s, centre(o, False), 0.5 * sd), (o, s, centre(o, True), 2.0 * sd)]
    rows += [(0, 0, centre(0, False), 0.02), (0, 1, centre(0, True), 0.02), (1, 0, centre(1, False), 1e-3),
             (0, 2, [31.5, 30.5, 29.5], 0.05)]
    lists["scale"] = mk(rows, [_rotation(rng) for _ in rows])
    # every octave, every level s = -1 .. K + 1 (detect only ever describes 0 .. K - 1)
    rows = [(o, s, centre(o, s % 2 == 0, margin=2), _level_sd(p, o, s))
            for o in range(p.num_octaves) for s in range(-1, K + 2)]
    lists["levels"] = mk(rows, [_rotation(rng) for _ in rows])
    # random proper rotations and reflections (det -1)
    rows = [(o, s, centre(o, k % 3 == 0), _level_sd(p, o, s)) for o in (0, 1) for s in (0, 1, 2) for k in range(2)]
    lists["rot"] = mk(rows, [_rotation(rng, reflect=k % 2 == 1) for k in range(len(rows))])
    # non-orthonormal R: scaled, anisotropically scaled and sheared
    Rs = [0.5 * np.eye(3), 2.0 * np.eye(3), 0.7 * _rotation(rng), _rotation(rng) @ np.diag([0.6, 1.0, 1.4]),
          np.diag([0.8, 0.55, 1.0]) @ _rotation(rng)]
    for (i, j) in ((0, 1), (1, 2), (2, 0)):
        S = np.eye(3)
        S[i, j] = 0.5
        Rs.append(S)
        Rs.append(_rotation(rng) @ S)
    rows = [(k % 2, k % 3, centre(k % 2, k % 2 == 1, margin=6), _level_sd(p, k % 2, k % 3)) for k in range(len(Rs))]
    lists["nonortho"] = mk(rows, Rs)
    # borders: xd = 0, xd * 2^o just below nx, windows clipped on all six faces
    rows = []
    for o in (0, 2):
        n = _level_dims(p, o)
        f = 2.0 ** o
        lo = [0.0, 0.0, 0.0]
        hi = [np.nextafter(n[i] * 1.0, 0.0) for i in range(3)]   # xd * 2^o < nx in the octave's voxels
        assert all(h * f < n0 for h, n0 in zip(hi, _level_dims(p, 0)))
        rows += [(o, 0, lo, _level_sd(p, o, 0)), (o, 1, hi, _level_sd(p, o, 1))]
        for ax in range(3):
            c = [v / 2.0 for v in n]
            c[ax] = 1.0
            rows.append((o, 1, list(c), _level_sd(p, o, 1)))
            c = [v / 2.0 + 0.25 for v in n]
            c[ax] = n[ax] - 1.5
            rows.append((o, 2, list(c), _level_sd(p, o, 2)))
    lists["border"] = mk(rows, [_rotation(rng) for _ in rows])
    # refusals (verify_keys): each list is two valid keypoints and one offender in the middle
    nx = _level_dims(p, 0)[0]
    good = [(0, 0, [20.0, 20.0, 20.0], _level_sd(p, 0, 0)), (1, 1, [10.5, 9.0, 11.0], _level_sd(p, 1, 1))]
    bad = {"ref_neg": (0, 0, [-1e-9, 20.0, 20.0], _level_sd(p, 0, 0)),
           "ref_eqnx": (1, 0, [nx / 2.0, 10.0, 10.0], _level_sd(p, 1, 0)),
           "ref_sd0": (0, 1, [20.0, 21.0, 22.0], 0.0),
           "ref_sdneg": (0, 1, [20.0, 21.0, 22.0], -1.0),
           "ref_below_nx": (1, 0, [np.nextafter(nx / 2.0, 0.0), 10.0, 10.0], _level_sd(p, 1, 0))}
    for case, b in bad.items():
        rows = [good[0], b, good[1]]
        lists[case] = mk(rows, [_rotation(rng) for _ in rows])
    return lists


def _g7_aniso_lists(p, rng):
    rows = []
    for o in range(p.num_octaves):
        n = _level_dims(p, o)
        for s in (-1, 0, 1, 2, 3):
            for f in (1.0, 1.3):
                rows.append(((o, s), [rng.uniform(3, v - 3) for v in n] + [f * _level_sd(p, o, s)]))
    return {"aniso": (np.array([r[0] for r in rows]), np.array([r[1] for r in rows]),
                      np.array([_rotation(rng) for _ in rows]))}


def _g7_axis_lists(p, rng):
    # R = I and the axis permutations (det +1 and -1) on the step volume: every rotated interior gradient lies on
    # an icosahedron edge (the x, y, z axes bisect edges of the mesh), so every voxel takes the full face scan
    perms = [np.eye(3)[list(q)] for q in ((0, 1, 2), (1, 2, 0), (2, 0, 1), (1, 0, 2), (0, 2, 1), (2, 1, 0))]
    rows, Rs = [], []
    for k, P in enumerate(perms):
        for o, s, frac in ((0, 0, False), (0, 1, True), (1, 0, k % 2 == 0)):
            n = _level_dims(p, o)
            c = [v / 2.0 + (0.37 if frac else 0.0) for v in n]
            rows.append(((o, s), c + [_level_sd(p, o, s)]))
            Rs.append(P)
    return {"axis": (np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array(Rs, np.float32))}


def _g7_wide_lists(p, rng):
    # one keypoint whose window row spans more than 1024 voxels (sd 64 on a 1300-voxel-wide volume; the box stays
    # below 2048 voxels on every axis), with R = I and a random rotation; and an ordinary one beside them
    sd0 = _level_sd(p, 0, 0)
    rows = [((0, 0), [650.0, 10.0, 10.0, 64.0]), ((0, 1), [649.5, 9.5, 9.75, 60.0]),
            ((0, 0), [100.0, 10.0, 10.0, sd0])]
    return {"wide": (np.array([r[0] for r in rows]), np.array([r[1] for r in rows]),
                     np.array([np.eye(3, dtype=np.float32), _rotation(rng), _rotation(rng)]))}


def _g7_switch_lists(p, rng):
    # level-0/1 keypoints with sd large enough for windows of > 1.9e5 voxels ((20 sd)^3 / (ux uy uz 8^o)), and some
    # just below that, at integer and fractional centres
    rows = []
    for o, s, sd in ((0, 0, 2.5), (0, 0, 3.0), (0, 1, 3.3), (0, 0, 4.0), (0, 1, 6.0), (1, 0, 5.0), (1, 0, 6.4),
                     (1, 1, 8.0), (0, 0, 2.8), (0, 2, 3.5)):
        n = _level_dims(p, o)
        frac = len(rows) % 2 == 1
        rows.append(((o, s), [v / 2.0 + (0.4 if frac else 0.0) for v in n] + [sd]))
    return {"switch": (np.array([r[0] for r in rows]), np.array([r[1] for r in rows]),
                       np.array([_rotation(rng) for _ in rows]))}


def g7_all():
    out = {}
    out.update(g7_keypoints("g7_survey64", so.synth_survey(64), dict(gen="survey", n=64, nblob=200),
                            make_lists=_g7_survey64_lists))
    out.update(g7_keypoints("g7_aniso", so.synth_survey((40, 33, 47)), dict(gen="survey", n=[40, 33, 47]),
                            units=(1.0, 1.5, 0.7), make_lists=_g7_aniso_lists))
    out.update(g7_keypoints("g7_axis", _steps_volume((48, 40, 44), 7), dict(gen="steps", n=[48, 40, 44], seed=7),
                            make_lists=_g7_axis_lists))
    out.update(g7_keypoints("g7_wide", so.synth_survey((1300, 20, 20)), dict(gen="survey", n=[1300, 20, 20]),
                            make_lists=_g7_wide_lists))
    out.update(g7_keypoints("g7_switch", so.synth_survey(96), dict(gen="survey", n=96),
                            make_lists=_g7_switch_lists))
    return out


def noise_volume(n, seed, blur_sigma=0.0):
    """White PCG64 noise, optionally blurred with the oracle's own blur (tests/util.golden_input restates this)."""
    nx, ny, nz = n
    vol = np.random.Generator(np.random.PCG64(seed)).standard_normal((nz, ny, nx)).astype(np.float32)
    return so.blur(vol, so.gauss_taps(blur_sigma)) if blur_sigma else vol


def _g8_voxels(rng, dims, n):
    """n random voxels with 1 <= x <= nx - 2 (and y, z alike): what the extrema stage guarantees."""
    return np.stack([rng.integers(1, d - 1, n) for d in dims], 1)


def _g8_faces(rng, dims, per_face=8):
    """Voxels on the six face-adjacent layers (x = 1, x = nx - 2, ...) and the eight corners (1, 1, 1) ...
    (nx - 2, ny - 2, nz - 2)."""
    out = []
    for ax in range(3):
        for v in (1, dims[ax] - 2):
            p = _g8_voxels(rng, dims, per_face)
            p[:, ax] = v
            out.append(p)
    out.append(np.array([[x, y, z] for z in (1, dims[2] - 2) for y in (1, dims[1] - 2) for x in (1, dims[0] - 2)]))
    return np.concatenate(out)


def _g8_survey_lists(p, rng):
    """Every level s = -1 .. K + 1 of octaves 0 and 1 at the level's own sd: 150 / 40 random voxels per level, and
    the face layers and corners on the finest and the coarsest level."""
    K = 3
    os_, xyz, sd = [], [], []
    for o, n in ((0, 150), (1, 40)):
        dims = _level_dims(p, o)
        for s in range(-1, K + 2):
            v = _g8_voxels(rng, dims, n)
            if (o, s) in ((0, -1), (1, K + 1)):
                v = np.concatenate([v, _g8_faces(rng, dims)])
            os_ += [(o, s)] * len(v)
            xyz.append(v)
            sd += [_level_sd(p, o, s)] * len(v)
    return {"list": (np.array(os_), np.concatenate(xyz), np.array(sd), 1.0)}


def _g8_sd_lists(sds, n=300):
    """The same n voxels of level (0, 0) with each of the scales `sds` (grouped by sd)."""
    def make(p, rng):
        v = _g8_voxels(rng, _level_dims(p, 0), n)
        return {"list": (np.array([(0, 0)] * (n * len(sds))), np.concatenate([v] * len(sds)),
                         np.repeat(np.array(sds, np.float64), n), 1.0)}
    return make


def _g8_faint_lists(p, rng):
    """The same 300 voxels of level (0, 0) at sd 1.6 with the LEVEL multiplied by 1, 1e-5 and 1e-6 (sift.c:997)."""
    v = _g8_voxels(rng, _level_dims(p, 0), 300)
    return {name: (np.array([(0, 0)] * len(v)), v, np.full(len(v), 1.6), f)
            for name, f in (("x1", 1.0), ("x1e-5", 1e-5), ("x1e-6", 1e-6))}


def g8_list(name, vol, input_spec, make_lists, units=(1, 1, 1)):
    """assign_eig_ori (sift.c:926-1085) on CALLER-MADE candidate lists of the reference's own pyramid of `vol`:
    make_lists(probe, rng) -> {case: (os (n, 2), xyz (n, 3), sd (n,), level scale)}.  Stored per case: the list, the
    reference's status (0 success, 1 REJECT), conf and R; and conf_maxdiff, the largest |conf_oracle - conf_ref| over
    the entries both accept (the oracle's eigen routine stands in for LAPACK dsyevd)."""
    p = refprobe.Probe()
    assert p.detect(vol, units) == 0
    o = so.Oracle()
    assert o.detect(vol, units) == 0
    d = {"units": np.array(units, np.float64), "dims": np.array(vol.shape[::-1], np.int32),
         "input_digest": np.array(digest(vol)), "num_octaves": np.array(p.num_octaves),
         "input_spec": np.array(json.dumps(input_spec))}
    rng = np.random.Generator(np.random.PCG64(int(hashlib.sha1(name.encode()).hexdigest()[:8], 16)))
    lists = make_lists(p, rng)
    info, maxdiff = {}, 0.0
    for case, (os_, xyz, sd, scale) in lists.items():
        os_ = np.asarray(os_, np.int32).reshape(-1, 2)
        xyz = np.asarray(xyz, np.int32).reshape(-1, 3)
        sd = np.asarray(sd, np.float64)
        status, conf, R = p.orient(os_, xyz, sd, scale)
        assert set(np.unique(status)) <= {0, 1}, "assign_eig_ori failed"
        for k, v in (("os", os_), ("xyz", xyz), ("sd", sd), ("scale", np.array(scale, np.float32)), ("status", status),
                     ("conf", conf), ("R", R)):
            d["%s_%s" % (case, k)] = v
        # the oracle on its own (bit-identical) levels
        st_o, cf_o = np.zeros_like(status), np.zeros_like(conf)
        for key in sorted(set(map(tuple, os_.tolist()))):
            m = (os_[:, 0] == key[0]) & (os_[:, 1] == key[1])
            lv, lu, _ = o.level(0, *key)
            assert digest(lv) == digest(p.level(0, *key)[0])
            _, _, cf_o[m], st_o[m] = so.orient_conf(lv * np.float32(scale), lu, sd[m], xyz[m])
        bad = np.nonzero(st_o != status)[0]
        assert len(bad) == 0, "status differs at %s of %s/%s" % (bad[:8], name, case)
        ok = status == 0
        if ok.any():
            maxdiff = max(maxdiff, float(np.abs(cf_o - conf)[ok].max()))
        info[case] = dict(n=int(len(os_)), success=int(ok.sum()))
    d["cases"] = np.array(json.dumps(list(lists)))
    d["conf_maxdiff"] = np.array(maxdiff)
    info["conf_maxdiff"] = maxdiff
    print(name, "conf_maxdiff %.3g" % maxdiff, flush=True)
    p.close()
    o.close()
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **d)
    return {name: info}


def g8_orient():
    out = {}
    out.update(g8_list("g8_survey", so.synth_survey(64), dict(gen="survey", n=64, nblob=200), _g8_survey_lists))
    out.update(g8_list("g8_aniso", so.synth_survey((70, 50, 41)), dict(gen="survey", n=[70, 50, 41]),
                       _g8_survey_lists, units=(1.0, 1.5, 0.7)))
    # sd pairs on either side of the weight LUT's limit (sd / u < 3.07) and of the table's quad capacity
    out.update(g8_list("g8_scales", so.synth_survey(40), dict(gen="survey", n=40),
                       _g8_sd_lists((1.5, 1.6, 3.0, 3.2, 4.2, 4.3))))
    out.update(g8_list("g8_noise", noise_volume((40, 40, 40), 8), dict(gen="noise", n=[40, 40, 40], seed=8),
                       _g8_sd_lists((1.6, 2.5))))
    out.update(g8_list("g8_noise_blur", noise_volume((40, 40, 40), 8, 1.5),
                       dict(gen="noise", n=[40, 40, 40], seed=8, blur_sigma=1.5), _g8_sd_lists((1.6, 2.5))))
    out.update(g8_list("g8_faint", so.synth_survey(40), dict(gen="survey", n=40), _g8_faint_lists))
    return out


def g9_names():
    from tests import extrema_cases as xc
    return sorted({f for f, _, _, _, _ in xc.G9})


def g9_fixture(name):
    """detect_extrema (sift.c:735-871) on the caller-made DoG levels of tests/extrema_cases.py (probe_extrema): per
    case of the fixture its recipe (seed, shape, plants -- not the arrays), state, peak_thresh and build, and the
    reference's records as (s, z, y, x) rows and strengths in its own order."""
    from tests import extrema_cases as xc
    d, cases = {}, []
    for f, recipe, state, peak, cuboid in xc.G9:
        if f != name:
            continue
        p = refprobe.Probe(cuboid_extrema=cuboid)
        D, _ = xc.build(recipe, state)
        szyx, strength = p.extrema(D, peak)
        p.close()
        i = len(cases)
        d["case%d_szyx" % i], d["case%d_strength" % i] = szyx.astype(np.int32), strength.astype(np.float32)
        cases.append(dict(recipe=recipe, state=state, peak=peak, cuboid=cuboid, n=int(len(szyx))))
    d["cases"] = np.array(json.dumps(cases))
    return d


def g9_extrema():
    out = {}
    for name in g9_names():
        d = g9_fixture(name)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **d)
        out[name] = {c["recipe"]["name"] + "/state%d/peak%g%s" % (c["state"], c["peak"], "/cuboid" * c["cuboid"]): c["n"]
                     for c in json.loads(str(d["cases"]))}
        print(name, out[name], flush=True)
    return out


def g6_abi():
    """The link-level contract as data, for machines without the reference: the names the unmodified
    reference library exports (libsift3D_ref.so) and the names its own CLI -- cli/kpSift3D.c compiled unchanged
    against include/sift3d by `make -C oracle ref` -- imports from the library (nm -D of both builds)."""
    import subprocess

    def names(path, *flags):
        out = subprocess.check_output(["nm", "-D"] + list(flags) + [path]).decode()
        return sorted({ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("sift3d_")
                       and (" T " in ln or " U " in ln)})

    d = {"library_exports": names(os.path.join(HERE, "_ref", "libsift3D_ref.so"), "--defined-only"),
         "cli_imports": names(os.path.join(HERE, "_ref", "kpSift3D"), "--undefined-only")}
    with open(os.path.join(OUT, "g6_abi.json"), "w") as f:
        json.dump(d, f, indent=1)
        f.write("\n")
    return {"g6_abi": {k: len(v) for k, v in d.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", action="store_true", help="also 128^3 and 256^3 (minutes)")
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    assert refprobe.available(), "run `make -C oracle ref` first (build container only)"
    os.makedirs(OUT, exist_ok=True)
    info = {"omp_threads": os.environ.get("OMP_NUM_THREADS", "unset"),
            "reference": "fatimp/SIFT3D v2.0 @ /root/reference, gcc -O3 -DNDEBUG -fopenmp"}
    jobs = {
        "g1": g1_filters,
        "g2": g2_fir,
        "g3_64": lambda: end_to_end("g3_64", so.synth_survey(64),
                                    input_spec=dict(gen="survey", n=64, nblob=200)),
        "g3_nc": lambda: end_to_end("g3_70x50x41", so.synth_survey((70, 50, 41)),
                                    input_spec=dict(gen="survey", n=[70, 50, 41])),
        "g3_an": lambda: end_to_end("g3_aniso", so.synth_survey((40, 33, 47)),
                                    units=(1.0, 1.5, 0.7),
                                    input_spec=dict(gen="survey", n=[40, 33, 47])),
        "g3_pp": lambda: end_to_end("g3_params", so.synth_survey(32),
                                    params=dict(num_kp_levels=2, sigma0=2.0, sigma_n=1.0,
                                                peak_thresh=0.05, corner_thresh=0.3),
                                    input_spec=dict(gen="survey", n=32)),
        "g3_cub": lambda: end_to_end("g3_cuboid64", so.synth_survey(64),
                                     params=dict(cuboid_extrema=True),
                                     input_spec=dict(gen="survey", n=64, nblob=200)),
        "g3_cubp": lambda: end_to_end("g3_cuboid_params", so.synth_lattice((50, 44, 40), seed=9),
                                      params=dict(cuboid_extrema=True, peak_thresh=0.03,
                                                  corner_thresh=0.2),
                                      input_spec=dict(gen="lattice", n=[50, 44, 40], seed=9)),
        "g3_lat": lambda: end_to_end("g3_lattice48", so.synth_lattice(48, seed=7),
                                     input_spec=dict(gen="lattice", n=48, seed=7)),
        # content the other g3_* never hold: twelve spikes on exact zero (the reference's levels then hold
        # subnormals), CT-like integers with plateaus, a subnormal input that its maximum divides back to order 1
        "g3_spikes64": lambda: end_to_end_content("spikes64"),
        "g3_integer48": lambda: end_to_end_content("integer48"),
        "g3_subnormal48": lambda: end_to_end_content("subnormal48"),
        "g4_csv": g4_csv,
        "g6_abi": g6_abi,
        # describe on caller-made keypoint lists (g7_*)
        "g7": g7_all,
        # orientation (assign_eig_ori) on caller-made candidate lists (g8_*)
        "g8": g8_orient,
        # detect_extrema on caller-made DoG levels (g9_*)
        "g9": g9_extrema,
    }
    if a.big:
        jobs["g5_128"] = lambda: end_to_end(
            "g5_128", so.synth_survey(128), desc_stride=8, store_levels=False,
            input_spec=dict(gen="survey", n=128, nblob=1600))
        jobs["g5_256"] = lambda: end_to_end(
            "g5_256", so.synth_survey(256), desc_stride=64, store_levels=False,
            input_spec=dict(gen="survey", n=256, nblob=12800))
    # descriptors at large sigma0 (sift.c:1453-1456: the window grows with sd^3, a bin receives ~30x
    # the terms it gets at the default 1.6) -- only on request (the reference needs minutes)
    if a.only and "g3_sigma3" in a.only.split(","):
        jobs["g3_sigma3"] = lambda: end_to_end(
            "g3_sigma3", so.synth_lattice(96, seed=13), store_levels=False,
            params=dict(sigma0=3.0, peak_thresh=0.03, corner_thresh=0.3),
            input_spec=dict(gen="lattice", n=96, seed=13))
    if a.only and "g3_sigma5" in a.only.split(","):
        jobs["g3_sigma5"] = lambda: end_to_end(
            "g3_sigma5", so.synth_survey(96), store_levels=False,
            params=dict(sigma0=5.0, peak_thresh=0.02, corner_thresh=0.2),
            input_spec=dict(gen="survey", n=96))
    # Round 5: the descriptor kernel's fast / reference-order switch (sift3d_host.c exact_desc_first_level:
    # windows of more than 1.9e5 voxels take the reference-order kernel).  sigma0 = 2.85: the keypoints of
    # level s = 0 have windows of 1.85e5 voxels -- the LARGEST the fast commit is ever used for --, those of
    # s = 1, 2 take the reference-order kernel.  Anisotropic units (1, 0.8, 0.8) at the default sigma0: the
    # unit product 0.64 pushes the windows of s = 2 (1.31e5 / 0.64 = 2.05e5 voxels) over the switch, s = 0, 1
    # stay below (sift.c:1453-1456, window radius in voxels = rad / unit: sift.c:96-108)
    if a.only and "g3_switch" in a.only.split(","):
        jobs["g3_switch"] = lambda: end_to_end(
            "g3_switch285", so.synth_lattice(96, seed=17), store_levels=False,
            params=dict(sigma0=2.85, peak_thresh=0.03, corner_thresh=0.3),
            input_spec=dict(gen="lattice", n=96, seed=17))
    if a.only and "g3_switch_aniso" in a.only.split(","):
        jobs["g3_switch_aniso"] = lambda: end_to_end(
            "g3_switch_aniso", so.synth_lattice((80, 112, 112), seed=19), units=(1.0, 0.8, 0.8),
            store_levels=False, params=dict(peak_thresh=0.05, corner_thresh=0.3),
            input_spec=dict(gen="lattice", n=[80, 112, 112], seed=19))
    # Round 5: sigma0 = 8 -- the octave filters are 31 ... 75 taps wide (half width ceil(3 sigma),
    # imutil.c:1275-1277), beyond the 65-tap tables of the device's fast kernels: the reference accepts any
    # sigma0 >= 0 (sift.c:553-565) and so must the drop-in
    if a.only and "g3_sigma8" in a.only.split(","):
        jobs["g3_sigma8"] = lambda: end_to_end(
            "g3_sigma8", so.synth_survey(96), store_levels=False,
            params=dict(sigma0=8.0, peak_thresh=0.01, corner_thresh=0.1),
            input_spec=dict(gen="survey", n=96))
    if a.only and "g5_slab8" in a.only.split(","):
        # BASELINE configs[3]'s slab geometry at 1/16 of its voxels: 256 x 256 x 1024 (eight 128-plane
        # Z-slabs, o_shard = 2) -- the sharded GPU tests compare with THIS, not with the single-GPU API
        jobs["g5_slab8"] = lambda: end_to_end_digest(
            "g5_256x256x1024", so.synth_lattice((256, 256, 1024), seed=11), stride=53,
            input_spec=dict(gen="lattice", n=[256, 256, 1024], seed=11))
    if a.only and "g5_512" in a.only.split(","):
        # BASELINE configs[2] (the bench workload): ~10 min of reference CPU time, ~10 GB
        jobs["g5_512"] = lambda: end_to_end_digest(
            "g5_512", so.synth_lattice(512, seed=11), input_spec=dict(gen="lattice", n=512, seed=11))
    for k, fn in jobs.items():
        if a.only and k not in a.only.split(","):
            continue
        t0 = time.time()
        r = fn()
        print(k, r, "%.1fs" % (time.time() - t0), flush=True)
        info.update(r)
    mpath = os.path.join(OUT, "MANIFEST.json")
    old = {}
    if os.path.exists(mpath):
        old = json.load(open(mpath))
    old.update(info)
    json.dump(old, open(mpath, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
