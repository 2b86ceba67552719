"""The seventeen registration wrappers of sift3d_amd/hip.py as wrappers: what they refuse and under which name, the
work size they ask for against the library's own, whose buffer they write, and that absent masks are all-ones masks.
The numbers they compute are held elsewhere (tests/test_affine_*.py, test_ffd*.py, test_masks.py,
test_registration_bytes.py); the volumes here are as small as the entries take, so every case is a handful of launches.

CALLS, inputs, faults, work_bytes and plain are also what a script needs to run two versions of hip.py side by side;
tests/test_calling_contracts.py runs the same calls on a second, larger set of inputs (a Set other than S)."""
import collections
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FSHAPE, MSHAPE = (5, 6, 7), (6, 5, 8)                      # [nz, ny, nx], no two dimensions of a volume alike
SPACING = (3, 2, 4)                                        # (dx, dy, dz)
LEVELS, EVALUATIONS, BINS, CHANNELS = 2, 3, 4, 2
RANGE = (0.0, 1.0)
BENDING, JACOBIAN, LANDMARK_WEIGHT = 0.01, 0.1, 0.05
# what inputs() is built from; S is the set of every test of this file
Set = collections.namedtuple("Set", "fshape mshape spacing levels evaluations bins channels")
S = Set(FSHAPE, MSHAPE, SPACING, LEVELS, EVALUATIONS, BINS, CHANNELS)

CALLS = {
    "affine_normal_equations": lambda h, x, kw: h.affine_normal_equations(x["F"], x["M"], x["A"], raw=True, **kw),
    "affine_ncc_normal_equations":
        lambda h, x, kw: h.affine_ncc_normal_equations(x["F"], x["M"], x["A"], raw=True, **kw),
    "affine_mi_normal_equations":
        lambda h, x, kw: h.affine_mi_normal_equations(x["F"], x["M"], x["A"], x["W"], RANGE, RANGE, raw=True, **kw),
    "parzen_histogram": lambda h, x, kw: h.parzen_histogram(x["F"], x["M"], x["A"], x["bins"], RANGE, RANGE, **kw),
    "parzen_histogram_field":
        lambda h, x, kw: h.parzen_histogram_field(x["F"], x["M"], x["field"], x["bins"], RANGE, RANGE, **kw),
    "affine_refine": lambda h, x, kw: h.affine_refine(x["F"], x["M"], x["A"], x["ap"], **kw),
    "affine_ncc_refine": lambda h, x, kw: h.affine_ncc_refine(x["F"], x["M"], x["A"], x["ap"], **kw),
    "affine_mi_refine":
        lambda h, x, kw: h.affine_mi_refine(x["F"], x["M"], x["A"], x["bins"], RANGE, RANGE, x["ap"], **kw),
    "ffd_evaluate":
        lambda h, x, kw: h.ffd_evaluate(x["F"], x["M"], x["lattice"], x["spacing"], x["A"], BENDING, **kw),
    "ffd_mi_evaluate":
        lambda h, x, kw: h.ffd_mi_evaluate(x["F"], x["M"], x["lattice"], x["spacing"], x["W"], RANGE, RANGE, x["A"],
                                           BENDING, **kw),
    "ffd_evaluate_landmarks":
        lambda h, x, kw: h.ffd_evaluate_landmarks(x["F"], x["M"], x["lattice"], x["spacing"], x["P"], x["Q"], x["w"],
                                                  LANDMARK_WEIGHT, x["A"], BENDING, JACOBIAN, **kw),
    "ffd_evaluate_channels":
        lambda h, x, kw: h.ffd_evaluate_channels(x["Fs"][0], x["Ms"][0], x["lattice"], x["spacing"], x["A"], BENDING,
                                                 **kw),
    "ffd_refine": lambda h, x, kw: h.ffd_refine(x["F"], x["M"], x["A"], x["fp"], **kw),
    "ffd_mi_refine":
        lambda h, x, kw: h.ffd_mi_refine(x["F"], x["M"], x["bins"], RANGE, RANGE, x["A"], x["fp"], **kw),
    "ffd_refine_jacobian":
        lambda h, x, kw: h.ffd_refine_jacobian(x["F"], x["M"], JACOBIAN, x["bins"], RANGE, RANGE, x["A"], x["fp"],
                                               **kw),
    "ffd_refine_landmarks":
        lambda h, x, kw: h.ffd_refine_landmarks(x["F"], x["M"], x["P"], x["Q"], x["w"], LANDMARK_WEIGHT, JACOBIAN,
                                                x["bins"], RANGE, RANGE, x["A"], x["fp"], **kw),
    "ffd_refine_channels": lambda h, x, kw: h.ffd_refine_channels(x["Fs"], x["Ms"], x["A"], x["fp"], **kw),
}
NAMES = sorted(CALLS)
STACKS = {"ffd_evaluate_channels", "ffd_refine_channels"}
RECORD = {"affine_normal_equations": 158, "affine_ncc_normal_equations": 186, "affine_mi_normal_equations": 158}
HIST = {"parzen_histogram", "parzen_histogram_field"}
TABLE = {"affine_mi_normal_equations", "ffd_mi_evaluate"}               # bins come with W
TAKES_BINS = {"parzen_histogram", "parzen_histogram_field", "affine_mi_refine", "ffd_mi_refine",
              "ffd_refine_jacobian", "ffd_refine_landmarks"}
AFFINE_REFINES = {"affine_refine", "affine_ncc_refine", "affine_mi_refine"}
FFD_REFINES = {"ffd_refine", "ffd_mi_refine", "ffd_refine_jacobian", "ffd_refine_landmarks", "ffd_refine_channels"}
EVALUATES = {"ffd_evaluate", "ffd_mi_evaluate", "ffd_evaluate_landmarks", "ffd_evaluate_channels"}
LANDMARKS = {"ffd_evaluate_landmarks", "ffd_refine_landmarks"}
NO_WORK = {"ffd_evaluate_landmarks"}                                     # allocates its own


def call(h, name, x, **kw):
    return CALLS[name](h, x, kw)


def pyramid(h, shape, levels):
    """the grids of `levels` levels under (and with) shape = (nz, ny, nx), each the half of the one above"""
    out = [tuple(shape)]
    while len(out) < levels:
        out.append(h.half_shape(out[-1]))
    return out


def inputs(h, s=S):
    """the one set of inputs of every case (of the set s); nothing in it is written by a call"""
    import torch
    rng = np.random.default_rng(17)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def volume(*shape):
        return dev(rng.random(shape, dtype=np.float32))
    lattice = h.ffd_lattice_shape(s.fshape, s.spacing)
    P = np.array([[1.5, 2.0, 1.0], [4.0, 3.5, 2.5], [5.5, 1.0, 3.0]])   # x, y, z inside S's fixed grid
    return dict(
        set=s, F=volume(*s.fshape), M=volume(*s.mshape), A=np.array([[1, 0, 0, 0.3], [0, 1, 0, -0.2], [0, 0, 1, 0.1]]),
        lattice=dev((rng.random(lattice, dtype=np.float32) - 0.5) * 0.6), spacing=s.spacing,
        field=dev((rng.random((3,) + tuple(s.fshape), dtype=np.float32) - 0.5) * 0.6),
        bins=s.bins, W=np.log(rng.random((s.bins, s.bins)) + 0.5), P=P, Q=P + [0.4, -0.3, 0.2],
        w=np.array([1.0, 2.0, 0.5]),
        Fs=[volume(s.channels, *g) for g in pyramid(h, s.fshape, s.levels)],
        Ms=[volume(s.channels, *g) for g in pyramid(h, s.mshape, s.levels)],
        ap=h.affine_refine_params(levels=s.levels, max_evaluations=s.evaluations),
        fp=h.ffd_refine_params(spacing=s.spacing, levels=s.levels, max_evaluations=s.evaluations))


def mask_kw(h, name, WF, WM, levels=LEVELS):
    """the wrapper's mask arguments from level 0's two masks (None: absent); the coarser levels of the stacks (`levels`
    in all) get ones where level 0 has a mask"""
    import torch
    if name != "ffd_refine_channels":
        return dict(mask_fixed=WF, mask_moving=WM)

    def per_level(W):
        return None if W is None else [W] + [torch.ones(g, dtype=torch.float32, device="cuda")
                                             for g in pyramid(h, W.shape, levels)[1:]]
    return dict(masks_fixed=per_level(WF), masks_moving=per_level(WM))


def some_masks(s=S, seed=23):
    """(WF, WM): masks of 0 and 1 on the two grids of the set s, about four voxels in five in, neither all ones"""
    import torch
    rng = np.random.default_rng(seed)
    out = [torch.from_numpy((rng.random(g) < 0.8).astype(np.float32)).cuda() for g in (s.fshape, s.mshape)]
    assert all(0 < float(W.sum()) < W.numel() for W in out)
    return tuple(out)


MASKED_SIZE = {"affine_refine", "ffd_refine"}       # the drivers with a size function of their own for the masked entry


def work_bytes(h, name, n_landmarks=3, masked=False, s=S):
    """the library's own size of the work buffer for the wrapper's call on inputs(h, s), without masks or (masked) with
    one: the two MSD drivers have their *_masked_work_bytes, every other entry one size for both"""
    L = h.lib()
    f, m, d = tuple(s.fshape)[::-1], tuple(s.mshape)[::-1], s.spacing
    stem = name + "_masked" if masked and name in MASKED_SIZE else name
    if name in AFFINE_REFINES:
        return getattr(L, "sift3d_amd_%s_work_bytes" % stem)(*f, *m, s.levels)
    if name in FFD_REFINES - STACKS:
        return getattr(L, "sift3d_amd_%s_work_bytes" % stem)(*f, *m, *d, s.levels,
                                                             *((n_landmarks,) if name in LANDMARKS else ()))
    return {"affine_normal_equations": lambda: L.sift3d_amd_affine_normal_work_bytes(*f),
            "affine_ncc_normal_equations": lambda: L.sift3d_amd_affine_ncc_normal_work_bytes(*f),
            "affine_mi_normal_equations": lambda: L.sift3d_amd_affine_normal_work_bytes(*f),
            "parzen_histogram": lambda: L.sift3d_amd_parzen_hist_work_bytes(*f),
            "parzen_histogram_field": lambda: L.sift3d_amd_parzen_hist_work_bytes(*f),
            "ffd_evaluate": lambda: L.sift3d_amd_ffd_evaluate_work_bytes(*f, *d),
            "ffd_mi_evaluate": lambda: L.sift3d_amd_ffd_evaluate_work_bytes(*f, *d),
            "ffd_evaluate_channels": lambda: L.sift3d_amd_ffd_evaluate_channels_work_bytes(*f, *d),
            "ffd_refine_channels": lambda: L.sift3d_amd_ffd_refine_channels_work_bytes(*f, *d)}[name]()


def faults(h, name, x):
    """[(what is wrong, inputs, keyword arguments)]: every input that breaks one rule of the wrapper `name`"""
    import torch
    stacks = name in STACKS
    F, M = (x["Fs"][0], x["Ms"][0]) if stacks else (x["F"], x["M"])

    def volumes(F=None, M=None):
        if stacks:
            return dict(x, Fs=[x["Fs"][0] if F is None else F] + x["Fs"][1:],
                        Ms=[x["Ms"][0] if M is None else M] + x["Ms"][1:])
        return dict(x, **{k: v for k, v in (("F", F), ("M", M)) if v is not None})

    def ffd_params(**kw):
        p = h.ffd_refine_params(spacing=SPACING, levels=LEVELS, max_evaluations=EVALUATIONS)
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    strided = torch.zeros(tuple(F.shape[:-1]) + (2 * F.shape[-1],), dtype=torch.float32, device="cuda")[..., ::2]
    wrong_mask = torch.ones(FSHAPE[::-1], dtype=torch.float32, device="cuda")
    out = [("F on the host", volumes(F=F.cpu()), {}), ("M float64", volumes(M=M.double()), {}),
           ("F not contiguous", volumes(F=strided), {}), ("M of the wrong rank", volumes(M=M[0]), {}),
           ("a mask of the wrong shape", x, mask_kw(h, name, wrong_mask, None))]
    if name != "parzen_histogram_field":
        out.append(("A of the wrong shape", dict(x, A=np.zeros((2, 4))), {}))
    if name in TAKES_BINS:
        out += [("bins = %d" % b, dict(x, bins=b), {}) for b in (3, 65)]
    if name in TABLE:
        out += [("W %d x %d" % s, dict(x, W=np.zeros(s)), {}) for s in ((3, 3), (65, 65), (4, 5))]
    if name in RECORD:
        out.append(("a short record", x, dict(record=torch.empty(RECORD[name] - 1, dtype=torch.int64, device="cuda"))))
    if name in HIST:
        out.append(("a hist that is not square", x,
                    dict(hist=torch.empty((BINS, BINS + 1), dtype=torch.int64, device="cuda"))))
    if name in AFFINE_REFINES:
        out.append(("levels = 0", dict(x, ap=h.affine_refine_params(levels=0, max_evaluations=EVALUATIONS)), {}))
    if name in FFD_REFINES:
        out += [("levels = 0", dict(x, fp=ffd_params(levels=0)), {}),
                ("a spacing of 0", dict(x, fp=ffd_params(spacing=(C.c_int * 3)(3, 0, 4))), {})]
    if name in EVALUATES:
        out.append(("a spacing of 0", dict(x, spacing=(3, 0, 4)), {}))
    if name in LANDMARKS:
        out += [("landmark lists of unequal length", dict(x, Q=x["Q"][:2]), {}),
                ("a negative landmark weight", dict(x, w=np.array([1.0, -1.0, 1.0])), {})]
    if name == "ffd_refine_channels":
        out.append(("a level that is not the half", dict(x, Fs=[x["Fs"][0]] * 2, Ms=[x["Ms"][0]] * 2), {}))
    return out


def plain(v):
    """a wrapper's return value as nested lists of bytes and integers: tensors and arrays by their bytes, structures
    field by field with the trail cut at `evaluations`, floats by their bits (a NaN equals itself)"""
    import torch
    if isinstance(v, torch.Tensor):
        return [str(v.dtype), tuple(v.shape), v.cpu().numpy().tobytes()]
    if isinstance(v, np.ndarray):
        return [str(v.dtype), v.shape, v.tobytes()]
    if isinstance(v, C.Structure):
        return [[f[0], plain(getattr(v, f[0])[:v.evaluations] if f[0] == "trail" else getattr(v, f[0]))]
                for f in v._fields_]
    if isinstance(v, (tuple, list, C.Array)):
        return [plain(e) for e in v]
    return np.float64(v).tobytes() if isinstance(v, float) else v


def results(name, out):
    """what of a wrapper's return value two calls must agree on: all of it but ffd_evaluate_channels' work buffer,
    which is scratch"""
    return plain(out[:3] if name == "ffd_evaluate_channels" else out)


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


@pytest.fixture(scope="module")
def x(hip):
    return inputs(hip)


@pytest.mark.parametrize("name", NAMES)
def test_refusals_carry_the_wrappers_name(hip, x, name):
    for label, bad, kw in faults(hip, name, x):
        with pytest.raises(ValueError) as e:
            call(hip, name, bad, **kw)
        assert str(e.value).startswith(name + ": "), (label, str(e.value))


@pytest.mark.parametrize("name", [n for n in NAMES if n not in NO_WORK])
def test_work_is_the_librarys_size(hip, x, name):
    """need - 1 bytes are refused and need accepted, without masks and with two that are not all ones (where the
    masked entry has a size of its own, that one; never less than the unmasked)"""
    import torch
    for masked in (False, True):
        kw = mask_kw(hip, name, *some_masks()) if masked else {}
        need = work_bytes(hip, name, masked=masked)
        assert need >= work_bytes(hip, name) > 0
        if name in MASKED_SIZE:
            assert masked == (need > work_bytes(hip, name))
        with pytest.raises(ValueError) as e:
            call(hip, name, x, work=torch.empty(need - 1, dtype=torch.uint8, device="cuda"), **kw)
        assert str(e.value).startswith(name + ": work "), (masked, str(e.value))
        work = torch.empty(need, dtype=torch.uint8, device="cuda")
        out = call(hip, name, x, work=work, **kw)
        if name == "ffd_evaluate_channels":
            assert out[3] is work


@pytest.mark.parametrize("name", sorted(set(RECORD) | HIST))
def test_callers_buffer_is_the_one_returned(hip, x, name):
    import torch
    if name in RECORD:
        mine = torch.empty(RECORD[name], dtype=torch.int64, device="cuda")
        assert call(hip, name, x, record=mine) is mine
    else:
        mine = torch.empty((BINS, BINS), dtype=torch.int64, device="cuda")
        assert call(hip, name, x, hist=mine)[0] is mine
    fresh = call(hip, name, x)
    assert plain(mine) == plain(fresh[0] if name in HIST else fresh)


@pytest.mark.parametrize("name", NAMES)
def test_absent_masks_are_masks_of_ones(hip, x, name):
    import torch
    WF = torch.ones(FSHAPE, dtype=torch.float32, device="cuda")
    WM = torch.ones(MSHAPE, dtype=torch.float32, device="cuda")
    absent = results(name, call(hip, name, x, **mask_kw(hip, name, None, None)))
    assert absent == results(name, call(hip, name, x, **mask_kw(hip, name, WF, WM)))
