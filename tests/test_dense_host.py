"""CPU (not gpu): the host side of dense descriptors -- the argument checks of
sift3d_amd_dense_descriptors_device / sift3d_amd_image_dense_descriptors and the stage entries, which
refuse bad input before any device call (so they hold on a machine without a GPU, and under the
sanitizer build), and the numpy restatement's binning that the GPU tests compare against."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import dense_restatement as dr


@pytest.fixture(scope="module")
def api():
    from sift3d_amd import api as a
    a.lib()
    return a


def _units(u):
    return (C.c_double * 3)(*u)


def _dense_dev(src, nx, ny, nz, units, sigma, out, work):
    from sift3d_amd import hip
    return hip.lib().sift3d_amd_dense_descriptors_device(src, nx, ny, nz, None if units is None else _units(units),
                                                         sigma, out, work, None)


def test_work_floats(api):
    from sift3d_amd import hip
    L = hip.lib()
    assert L.sift3d_amd_dense_work_floats(5, 6, 7) == 2 * 5 * 6 * 7
    assert L.sift3d_amd_dense_work_floats(576, 576, 544) == 2 * 576 * 576 * 544
    assert L.sift3d_amd_dense_work_floats(0, 6, 7) == 0
    assert L.sift3d_amd_dense_work_floats(5, -1, 7) == 0


def test_device_entry_refuses_bad_arguments_without_device(api):
    from sift3d_amd import hip
    n = 8 * 8 * 8
    # Every case below is refused before any device call.  Without a device the buffers are made-up
    # addresses; with one they are real allocations that cover every range named below.
    bufs = []
    if api.device_available():
        bufs = [hip.lib().sift3d_hip_malloc(4 * n * 40)]
        assert all(bufs)
        base = bufs[0]
    else:
        base = 0x1000000
    S, O, W = base, base + 4 * n * 2, base + 4 * n * 16
    u1 = (1.0, 1.0, 1.0)
    cases = [
        (None, 8, 8, 8, u1, 1.6, O, W),
        (S, 8, 8, 8, u1, 1.6, None, W),
        (S, 8, 8, 8, u1, 1.6, O, None),
        (S, 8, 8, 8, None, 1.6, O, W),
        (S, 0, 8, 8, u1, 1.6, O, W),
        (S, 8, -2, 8, u1, 1.6, O, W),
        (S, 8, 8, 0, u1, 1.6, O, W),
        (S, 8, 8, 8, u1, 0.0, O, W),
        (S, 8, 8, 8, u1, -1.0, O, W),
        (S, 8, 8, 8, u1, math.nan, O, W),
        (S, 8, 8, 8, u1, math.inf, O, W),
        (S, 8, 8, 8, (0.0, 1.0, 1.0), 1.6, O, W),
        (S, 8, 8, 8, (1.0, -1.0, 1.0), 1.6, O, W),
        (S, 8, 8, 8, (1.0, 1.0, math.nan), 1.6, O, W),
        (S, 8, 8, 8, (math.inf, 1.0, 1.0), 1.6, O, W),
        (S, 8, 8, 8, u1, 1.6, S, W),                      # output over the source
        (S, 8, 8, 8, u1, 1.6, S + 4 * (n - 1), W),        # output starts in the source's last voxel
        (O + 4 * 12 * n - 4, 8, 8, 8, u1, 1.6, O, W),     # source starts in the output's last voxel
        (S, 8, 8, 8, u1, 1.6, O, O + 4 * 100),            # work inside the output
        (S, 8, 8, 8, u1, 1.6, W + 4 * (2 * n - 1), W),    # output starts in the work buffer's end
    ]
    try:
        for c in cases:
            assert _dense_dev(*c) == -1, c
    finally:
        for b in bufs:
            hip.lib().sift3d_hip_free(b)


def test_stage_entries_refuse_bad_arguments_without_device(api):
    from sift3d_amd import hip
    L = hip.lib()
    S, O = 0x1000000, 0x2000000
    assert L.sift3d_hip_dense_bin(None, 8, 8, 8, 1.0, 1.0, 1.0, O, None) == -1
    assert L.sift3d_hip_dense_bin(S, 8, 8, 8, 1.0, 1.0, 1.0, None, None) == -1
    assert L.sift3d_hip_dense_bin(S, 8, 0, 8, 1.0, 1.0, 1.0, O, None) == -1
    assert L.sift3d_hip_dense_bin(S, 8, 8, 8, 1.0, 0.0, 1.0, O, None) == -1
    assert L.sift3d_hip_dense_bin(S, 8, 8, 8, 1.0, 1.0, math.nan, O, None) == -1
    assert L.sift3d_hip_dense_bin(S, 8, 8, 8, 1.0, 1.0, 1.0, S + 4, None) == -1
    assert L.sift3d_hip_dense_normalize(None, 10, None) == -1
    assert "NULL" in L.sift3d_hip_last_error().decode()


def test_valid_call_without_device_reports_it(api, capfd):
    from sift3d_amd import hip
    if api.device_available():
        import torch
        src = torch.rand((6, 7, 8), device="cuda")
        out = torch.empty((12, 6, 7, 8), device="cuda")
        work = torch.empty(hip.lib().sift3d_amd_dense_work_floats(8, 7, 6), device="cuda")
        assert _dense_dev(src.data_ptr(), 8, 7, 6, (1.0, 1.0, 1.0), 1.6, out.data_ptr(), work.data_ptr()) == 0
        torch.cuda.synchronize()
        return
    n = 8 * 7 * 6
    assert _dense_dev(0x1000000, 8, 7, 6, (1.0, 1.0, 1.0), 1.6, 0x2000000, 0x2000000 + 4 * 12 * n) == -1
    assert "no HIP device" in capfd.readouterr().err
    im = api.Image.from_array(np.zeros((6, 7, 8), np.float32), (1.0, 1.0, 2.0))
    out = np.zeros(12 * n, np.float32)
    assert api.lib().sift3d_amd_image_dense_descriptors(im.h, 1.6, out) == -1
    assert "no HIP device" in capfd.readouterr().err
    with pytest.raises(RuntimeError):
        api.dense_descriptors(np.zeros((6, 7, 8), np.float32))


def test_image_entry_refuses_bad_arguments_without_device(api, capfd):
    L = api.lib()
    im = api.Image(8, 7, 6)
    out = np.zeros(12 * 8 * 7 * 6, np.float32)
    two = api.Image(8, 7, 6, 2)
    assert L.sift3d_amd_image_dense_descriptors(None, 1.6, out) == -1
    raw = L["sift3d_amd_image_dense_descriptors"]        # (a fresh handle: out may be NULL)
    raw.restype, raw.argtypes = C.c_int, [C.c_void_p, C.c_double, C.c_void_p]
    assert raw(im.h, 1.6, None) == -1
    assert L.sift3d_amd_image_dense_descriptors(two.h, 1.6, np.zeros(2 * out.size, np.float32)) == -1
    for s in (0.0, -0.5, math.nan, math.inf):
        assert L.sift3d_amd_image_dense_descriptors(im.h, s, out) == -1, s
    inf_units = api.Image(8, 7, 6)
    assert L.sift3d_amd_image_set_units(inf_units.h, 1.0, math.inf, 1.0) == 0
    assert L.sift3d_amd_image_dense_descriptors(inf_units.h, 1.6, out) == -1
    err = capfd.readouterr().err
    assert "NULL" in err and "single-channel" in err and "sigma" in err and "units" in err
    assert "no HIP device" not in err
    with pytest.raises(ValueError):
        api.dense_descriptors(two)


def _directions(rng, so_mesh):
    """Random unit directions, plus directions on the icosahedron's vertices and edges (and tiny
    perturbations of them), scaled by magnitudes from 1e-2 to 1e3."""
    v, _ = so_mesh
    verts = v.reshape(-1, 3)
    edges = np.concatenate([v[:, 0] + v[:, 1], v[:, 1] + v[:, 2], v[:, 2] + v[:, 0]])
    centres = v.sum(axis=1)
    special = np.concatenate([verts, edges, centres, -verts, -edges]).astype(np.float64)
    special = np.concatenate([special] + [special + rng.normal(0, s, special.shape) for s in (1e-7, 1e-6, 1e-5)])
    rand = rng.normal(size=(200000, 3))
    d = np.concatenate([special, rand])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= np.exp(rng.uniform(np.log(1e-2), np.log(1e3), (len(d), 1)))
    return d.astype(np.float32)


def test_restatement_binning_picks_one_face_with_unit_barycentrics(oracle_mod):
    m = dr.mesh(oracle_mod)
    d = _directions(np.random.default_rng(3), m)
    g = tuple(np.ascontiguousarray(d[:, k]) for k in range(3))
    face, bary, nacc = dr.face_of(g, m)
    assert np.all(face >= 0)                       # every direction falls in some face
    assert np.all(nacc >= 1)
    # (directions within ~eps of an edge pass on both sides: the first in table order wins)
    assert np.all(nacc[len(d) - 200000:][np.min(np.stack(bary), 0)[len(d) - 200000:] > 2e-5] == 1)
    s = bary[0].astype(np.float64) + bary[1] + bary[2]
    assert np.abs(s - 1.0).max() < 1e-6
    assert np.min(np.stack(bary)) >= -dr.EPS
    # the channels are the geometric vertices: the vertex nearest the direction is one of the face's,
    # and away from the face's medians it carries the largest barycentric
    _, ids = m
    V = dr.vertices(oracle_mod)
    near = np.argmax(d @ V.T, axis=1)
    assert np.all(np.any(ids[face] == near[:, None], axis=1))
    b = np.stack(bary, 1)
    top = np.sort(b, 1)
    clear = top[:, 2] - top[:, 1] > 1e-3
    assert np.all(ids[face, np.argmax(b, 1)][clear] == near[clear])


def test_restatement_mirror_permutes_channels(oracle_mod):
    m = dr.mesh(oracle_mod)
    V = dr.vertices(oracle_mod)
    perm = [int(np.argmin(np.abs(V - V[c] * np.float32([-1, 1, 1])).sum(1))) for c in range(12)]
    assert sorted(perm) == list(range(12))
    vol = oracle_mod.synth_survey((14, 12, 10), seed=4)
    h = dr.dense_bin(vol, m)
    hf = dr.dense_bin(vol[:, :, ::-1], m)
    assert np.abs(hf[perm][:, :, :, ::-1] - h).max() < 1e-5 * max(1.0, float(np.abs(h).max()))


def test_restatement_dense_bin_values(oracle_mod):
    m = dr.mesh(oracle_mod)
    rng = np.random.default_rng(5)
    vol = rng.normal(size=(5, 6, 7)).astype(np.float32)
    vol[:, :, 3:] = 2.0                              # a flat part: zero gradients there
    h = dr.dense_bin(vol, m, (1.0, 1.5, 0.5))
    assert h.shape == (12, 5, 6, 7) and h.dtype == np.float32
    assert np.count_nonzero(h, axis=0).max() <= 3
    assert np.all(h[:, :, :, 5:] == 0) and np.all(np.signbit(h[:, :, :, 5:]) == 0)
    g = dr.gradient(vol, (1.0, 1.5, 0.5))
    mag = np.sqrt(g[0].astype(np.float64) ** 2 + g[1] ** 2 + g[2] ** 2)
    live = mag * mag >= 1.2e-6
    np.testing.assert_allclose(h.astype(np.float64).sum(0)[live], mag[live], rtol=1e-5)
    hn = dr.normalize(h)
    nrm = np.sqrt((hn.astype(np.float64) ** 2).sum(0))
    assert np.abs(nrm[live] - 1).max() < 1e-6 and np.all(hn[:, ~live] == 0)
