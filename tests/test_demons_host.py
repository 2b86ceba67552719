"""CPU (not gpu): the host side of the dense demons refinement -- every refusal of sift3d_hip_demons_force and
sift3d_amd_demons_device, which check their arguments before any device call; the exported symbols; and the
numpy restatement (tests/demons_restatement.py) against itself and Thirion's textbook formula."""
import numpy as np
import pytest

from tests import demons_restatement as dm


@pytest.fixture(scope="module")
def api():
    from sift3d_amd import api as a
    a.lib()
    return a


@pytest.fixture(scope="module")
def bufs(api):
    """made-up addresses without a device; real allocations covering every range named below with one, so
    that a regressed check could not make a kernel touch unmapped memory"""
    from sift3d_amd import hip
    if api.device_available():
        b = [hip.lib().sift3d_hip_malloc(1 << 16) for _ in range(3)]
        assert all(b)
        yield b
        for p in b:
            hip.lib().sift3d_hip_free(p)
    else:
        yield [0x100000, 0x900000, 0x1100000]


EXPORTED = ["sift3d_hip_demons_force", "sift3d_amd_demons_work_floats", "sift3d_amd_demons_device"]


def test_symbols_exported(api):
    from sift3d_amd import _native, hip
    L = _native.load()
    for name in EXPORTED:
        assert hasattr(L, name), name
    hip.lib()
    for name in ("demons_force", "demons", "demons_stats"):
        assert callable(getattr(hip, name))
    for name in ("refine_field", "register_dense"):
        assert callable(getattr(api, name))
    assert api.DemonsRefinement._fields == ("field", "warped", "msd", "jacobian")
    assert api.DenseRegistration._fields == ("A", "tps", "inliers", "num_matches", "field", "warped", "msd",
                                             "jacobian")


def test_work_floats(api):
    from sift3d_amd import hip
    L = hip.lib()
    part = 32768 // 4
    assert L.sift3d_amd_demons_work_floats(8, 8, 8, 1) == part + 6 * 512
    assert L.sift3d_amd_demons_work_floats(37, 29, 23, 12) == part + 17 * 37 * 29 * 23
    for a in ((0, 8, 8, 1), (8, -1, 8, 1), (8, 8, 0, 1), (8, 8, 8, 0), (8, 8, 8, -2)):
        assert L.sift3d_amd_demons_work_floats(*a) == 0


def _force_args(bufs):
    """a well-formed call on 8^3 grids, nc = 1: F, W, u in buffer 0, step and stats in 1, the partials in 2"""
    A, B, W = bufs
    return dict(F=A, nx=8, ny=8, nz=8, W=A + 8192, u=A + 16384, mx=8, my=8, mz=8, nc=1, alpha=1.0, step=B,
                stats=B + 8192, work=W)


def _force(L, a):
    return L.sift3d_hip_demons_force(a["F"], a["nx"], a["ny"], a["nz"], a["W"], a["u"], a["mx"], a["my"], a["mz"],
                                     a["nc"], a["alpha"], a["step"], a["stats"], a["work"], None)


def test_force_refusals(bufs):
    from sift3d_amd import hip
    L = hip.lib()
    base = _force_args(bufs)
    A, B, W = bufs
    changes = [
        dict(F=None), dict(W=None), dict(u=None), dict(step=None), dict(stats=None), dict(work=None),
        dict(nx=0), dict(ny=-1), dict(nz=0), dict(mx=0), dict(my=-3), dict(mz=0),
        dict(nc=0), dict(nc=-1),
        dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=float("nan")), dict(alpha=float("inf")),
        dict(stats=B + 8196), dict(work=W + 4),                           # 8-byte alignment
        dict(F=A + 2), dict(W=A + 8194), dict(u=A + 16385), dict(step=B + 1),
        dict(step=A + 4 * 100),                                           # step inside F
        dict(step=A + 8192 + 4 * 511),                                    # step runs into W ... and u
        dict(step=A + 16384 + 4 * 1000),                                  # step inside u
        dict(stats=A + 8192 + 64),                                        # stats inside W
        dict(stats=B + 4 * 1534),                                         # stats inside step
        dict(work=B + 4 * 1000),                                          # the partials inside step
        dict(work=A),                                                     # the partials over F, W, u
        dict(stats=W + 32768 - 8),                                        # stats inside the partials
        dict(nc=5, step=A + 8192 + 4 * 2300),                             # step inside W's fifth channel
    ]
    for ch in changes:
        a = dict(base)
        a.update(ch)
        assert _force(L, a) == -1, ch


def _drv_args(bufs):
    """F and M in buffer 0, u and stats in 1, the work buffer in 2 (8^3, nc = 1: 11264 floats)"""
    A, B, W = bufs
    return dict(F=A, nx=8, ny=8, nz=8, M=A + 8192, mx=8, my=8, mz=8, nc=1, u=B, it=3, alpha=1.0, sf=1.0, sd=1.0,
                work=W, stats=B + 8192)


def _drv(L, a):
    return L.sift3d_amd_demons_device(a["F"], a["nx"], a["ny"], a["nz"], a["M"], a["mx"], a["my"], a["mz"], a["nc"],
                                      a["u"], a["it"], a["alpha"], a["sf"], a["sd"], a["work"], a["stats"], None)


def test_driver_refusals(bufs):
    from sift3d_amd import hip
    L = hip.lib()
    base = _drv_args(bufs)
    A, B, W = bufs
    changes = [
        dict(F=None), dict(M=None), dict(u=None), dict(work=None), dict(stats=None),
        dict(nx=0), dict(ny=-2), dict(nz=0), dict(mx=-1), dict(my=0), dict(mz=0),
        dict(nc=0), dict(nc=-5), dict(it=-1),
        dict(alpha=0.0), dict(alpha=-0.5), dict(alpha=float("nan")), dict(alpha=float("inf")),
        dict(sf=-0.1), dict(sf=float("nan")), dict(sf=float("inf")),
        dict(sd=-1.0), dict(sd=float("nan")), dict(sd=float("-inf")),
        dict(stats=B + 8196), dict(work=W + 4),                           # 8-byte alignment
        dict(F=A + 2), dict(M=A + 8193), dict(u=B + 2),
        dict(u=A + 4 * 300),                                              # u inside F
        dict(u=A + 8192 + 4 * 100),                                       # u inside M
        dict(u=W + 4 * 9000),                                             # u inside the work buffer
        dict(stats=B + 4 * 1000),                                         # stats inside u
        dict(stats=B + 4 * 1536 - 8),                                     # the first record ends u ... still inside
        dict(stats=A + 4 * 511),                                          # stats inside F
        dict(work=A + 8192 + 4 * 500),                                    # the work buffer runs over M
        dict(work=B),                                                     # the work buffer over u
        dict(stats=W + 4 * 11264 - 16),                                   # stats inside the work buffer
        dict(nc=2, stats=A + 8192 + 4 * 1000),                            # stats inside M's second channel
    ]
    for ch in changes:
        a = dict(base)
        a.update(ch)
        assert _drv(L, a) == -1, ch
    # iterations == 0 is no refusal (nothing is done), but bad arguments still are
    a = dict(base)
    a.update(it=0, alpha=0.0)
    assert _drv(L, a) == -1


def test_python_refusals(api):
    vol = np.zeros((5, 6, 7), np.float32)
    with pytest.raises(ValueError):
        api.refine_field(vol, vol)
    with pytest.raises(ValueError):
        api.register_dense(vol, vol)


# ---- the restatement against itself --------------------------------------------------------------------------
def _rand(shape, seed, scale=1.0):
    return np.random.default_rng(seed).normal(0, scale, shape).astype(np.float32)


def test_restated_equal_images_give_zero():
    for nc in (1, 3, 12):
        F = _rand((nc, 7, 6, 9), nc)
        u = _rand((3, 7, 6, 9), 2, 0.5)
        delta, sd, ins = dm.ref_force(F, F.copy(), u, (7, 6, 9), 1.0)
        assert ins.any() and not ins.all()
        assert not delta.view(np.uint32).any()                         # +0.0 everywhere, no -0.0
        assert dm.ref_stats(sd, ins)[0] == 0.0


def test_restated_zero_denominator_gives_positive_zero():
    F = np.full((2, 4, 5, 6), 3.0, np.float32)
    delta, sd, ins = dm.ref_force(F, F.copy(), np.zeros((3, 4, 5, 6), np.float32), (4, 5, 6), 0.5)
    _, sg, _, _ = dm.force_terms(F, F, np.zeros((3, 4, 5, 6), np.float32), (4, 5, 6))
    assert ins.all() and not sg.any() and not sd.any()
    assert not delta.view(np.uint32).any()


@pytest.mark.parametrize("alpha", [0.25, 1.0, 3.0])
def test_restated_step_is_capped_by_alpha(alpha):
    rng = np.random.default_rng(7)
    for nc in (1, 3, 12):
        shape = (9, 8, 11)
        F = rng.normal(0, 1, (nc,) + shape).astype(np.float32)
        W = (F + rng.normal(0, rng.choice([0.01, 1.0, 30.0]), F.shape)).astype(np.float32)
        u = rng.normal(0, 2, (3,) + shape).astype(np.float32)
        delta, _, ins = dm.ref_force(F, W, u, (10, 7, 12), alpha)
        norm = np.sqrt((delta.astype(np.float64) ** 2).sum(0))
        assert norm.max() <= (1.0 / (2.0 * alpha)) * (1.0 + 2.0 ** -20)
        assert norm[ins].max() > 0


def test_restated_force_is_thirions_formula():
    """nc = 1 and W = F + c exactly (integers plus 0.5): grad W = grad F, so the symmetric gradient is grad F and
    delta = d grad F / (|grad F|^2 + alpha^2 d^2) with d = -c, evaluated here in float64"""
    rng = np.random.default_rng(3)
    shape = (6, 7, 8)
    F = rng.integers(-20, 20, shape).astype(np.float32)
    for c, alpha in ((0.5, 1.0), (-2.5, 0.3), (4.0, 2.0)):
        W = (F + np.float32(c)).astype(np.float32)
        assert np.array_equal(W - F, np.full(shape, c, np.float32))
        delta, _, ins = dm.ref_force(F, W, np.zeros((3,) + shape, np.float32), shape, alpha)
        assert ins.all()
        g = [np.gradient(F.astype(np.float64), axis=a) for a in (2, 1, 0)]
        d = -float(c)
        den = g[0] ** 2 + g[1] ** 2 + g[2] ** 2 + alpha ** 2 * d * d
        want = np.stack([d * ge / den for ge in g])
        np.testing.assert_allclose(delta.astype(np.float64), want, rtol=1e-6, atol=0)


def test_restated_gamma():
    assert dm.gamma(0) == 0.0
    assert abs(dm.gamma(2 ** 20) - 2.0 ** -33) < 2.0 ** -60
