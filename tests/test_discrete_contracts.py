"""GPU: how the entries of "Discrete displacement search" are called, not what they compute (tests/test_discrete.py
holds the numbers): the two contracts of tests/test_calling_contracts.py on the new entries, its helpers restated.

A. d_work holds the library's own *_work_bytes() / *_work_floats() and nothing is assumed of its contents: every
   work-taking wrapper runs on a work view of exactly that size between two guard bands, the whole tensor filled with
   0xFF (NaN as float and double, 2^64 - 1 as a counter) and then with 0x00, twice in a row on each fill without
   refilling.  Both bands must keep the fill and every result must be, byte for byte, that of work=None.  An entry whose
   size is 0 runs on an empty view: the bands then show that it writes nothing at all.
B. everything an entry does is ordered on the caller's stream: every entry runs on a fresh stream on zeroed twins of its
   inputs, into which the real inputs are copied on that stream behind some milliseconds of queued work; the result
   must be that of the default stream, and differ from that of the zeroed inputs."""
import numpy as np
import pytest

from tests.test_discrete_host import smooth_noise

pytestmark = pytest.mark.gpu
F32 = np.float32
MIN_BAND = 65536
SHAPE, NC, R, LEVELS = (13, 13, 21), 2, 2, 2                  # odd sizes: pad4 of every buffer of the driver adds something
THETAS, PASSES = (0.02, 0.3), 2


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


def _g(t):
    return tuple(t.shape[-3:])[::-1]


def _nb(t):
    return tuple(n // 4 for n in t.shape[-3:])[::-1]


def _discrete_register(h, x, kw):
    u = x["field"].clone()
    return u, h.discrete_register(x["Fs"], x["Ms"], u, h.discrete_register_params(R, PASSES, THETAS), x["VF"], x["VM"],
                                  **kw)


# name: (call(h, x, kw), the library's size in bytes of that call's work buffer)
ROWS = {
    "cost_volume": (lambda h, x, kw: h.cost_volume(x["Fs"][0], x["W"], R, x["VF"], x["VW"], **kw),
                    lambda h, x: h.lib().sift3d_amd_cost_volume_work_bytes(*_g(x["W"]), NC, R)),
    "cost_select": (lambda h, x, kw: h.cost_select(x["cost"], x["u"], 0.3, **kw),
                    lambda h, x: h.lib().sift3d_amd_cost_select_work_bytes(*_nb(x["W"]))),
    "block_field_smooth": (lambda h, x, kw: h.block_field_smooth(x["u"], PASSES, **kw),
                           lambda h, x: h.lib().sift3d_amd_block_field_smooth_work_bytes(*_nb(x["W"]), PASSES)),
    "discrete_register": (_discrete_register,
                          lambda h, x: 4 * h.lib().sift3d_amd_discrete_register_work_floats(
                              *_g(x["Fs"][0]), *_g(x["Ms"][0]), NC, LEVELS, R, 1, 1)),
}
STREAM_ONLY = {
    "block_field_expand": lambda h, x, kw: h.block_field_expand(x["u"], tuple(x["W"].shape[-3:])),
}


@pytest.fixture(scope="module")
def data(hip):
    import torch

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a, F32)).cuda()
    rng = np.random.default_rng(31)
    mshape = (13, 18, 19)
    x = {"Fs": [dev(np.stack([smooth_noise(SHAPE, 3 + c) for c in range(NC)]) + 2)],
         "Ms": [dev(np.stack([smooth_noise(mshape, 7 + c) for c in range(NC)]) + 2)]}
    x["Fs"].append(hip.restrict2(x["Fs"][0]))
    x["Ms"].append(hip.restrict2(x["Ms"][0]))
    x["W"] = dev(np.stack([smooth_noise(SHAPE, 11 + c) for c in range(NC)]) + 2)
    VF, VW = np.ones(SHAPE, F32), np.ones(SHAPE, F32)
    VF[1, 2, 3] = 0
    VW[9, 9, 9] = 0
    VM = np.ones(mshape, F32)
    VM[6, 6, 6] = 0
    x["VF"], x["VW"], x["VM"] = dev(VF), dev(VW), dev(VM)
    x["field"] = dev(rng.standard_normal((3,) + SHAPE) * 0.4 + 0.2)
    x["cost"] = hip.cost_volume(x["Fs"][0], x["W"], R, x["VF"], x["VW"])
    x["u"] = dev(rng.standard_normal((3,) + x["cost"].shape[:3]) + 0.3)
    torch.cuda.synchronize()
    return x


@pytest.fixture(scope="module")
def delay():
    """about 2 ms of queued work per 20 in-place multiplies"""
    import torch
    return torch.ones((256, 512, 512), device="cuda")


def tree(v, f):
    """v with f applied to every tensor in its lists, tuples and dicts"""
    import torch
    if isinstance(v, torch.Tensor):
        return f(v)
    if isinstance(v, dict):
        return {k: tree(e, f) for k, e in v.items()}
    if type(v) in (list, tuple):
        return type(v)(tree(e, f) for e in v)
    return v


def tensors(v):
    import torch
    if isinstance(v, torch.Tensor):
        yield v
    elif isinstance(v, dict):
        for k in v:
            yield from tensors(v[k])
    elif type(v) in (list, tuple):
        for e in v:
            yield from tensors(e)


def results(out):
    """the bytes of every tensor a call returns"""
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy().tobytes() for t in tensors(out)]


def guarded(need, fill):
    """(the work view of `need` bytes rounded up to 4, 16-byte aligned; the two bands round it), all filled with the
    byte `fill`"""
    import torch
    size = (need + 3) // 4 * 4
    G = (max(MIN_BAND, size) + 15) // 16 * 16
    whole = torch.full((G + size + G,), fill, dtype=torch.uint8, device="cuda")
    view = whole[G:G + size]
    assert view.data_ptr() % 16 == 0 and view.numel() == size
    return view, (whole[:G], whole[G + size:])


def test_the_set_pads(hip, data):
    """what makes this the padding set, asserted and not assumed"""
    for t in (data["Fs"] + data["Ms"]):
        assert int(np.prod(t.shape[-3:])) % 4 != 0
    nb = int(np.prod(data["cost"].shape[:3]))
    assert nb % 4 != 0 and (3 * nb) % 4 != 0 and (nb * (2 * R + 1) ** 3) % 4 != 0


@pytest.mark.parametrize("name", sorted(ROWS))
def test_work_of_the_librarys_size_guarded_and_poisoned(hip, data, name):
    import torch
    call, size = ROWS[name]
    need = size(hip, data)
    assert need > 0 or name == "cost_volume"                  # (the cost volume needs none: the header says so)
    want = results(call(hip, data, {}))
    if need:
        with pytest.raises(ValueError):
            call(hip, data, dict(work=guarded(need, 0)[0][:-1]))
    for fill in (0xFF, 0x00):
        work, bands = guarded(need, fill)
        for run in ("first", "second"):                      # the second finds what the first left behind
            got = results(call(hip, data, dict(work=work)))
            torch.cuda.synchronize()
            spilt = [int((b != fill).sum()) for b in bands]
            assert spilt == [0, 0], "%s call on work of 0x%02X, %d bytes: bytes written before, behind: %s" % (
                run, fill, need, spilt)
            assert got == want, "%s call on work of 0x%02X differs from work=None" % (run, fill)


@pytest.mark.parametrize("name", sorted(ROWS) + sorted(STREAM_ONLY))
def test_entry_is_ordered_on_the_callers_stream(hip, data, delay, name):
    import torch
    call = ROWS[name][0] if name in ROWS else STREAM_ONLY[name]
    hip.current_stream(refresh=True)
    want = results(call(hip, data, {}))
    twins = tree(data, torch.zeros_like)
    # the premise: on the zeros, which is what any other stream would read, the entry gives something else
    assert results(call(hip, twins, {})) != want, "all-zero inputs give the same bytes"
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    try:
        with torch.cuda.stream(s):
            hip.current_stream(refresh=True)
            for _ in range(20):
                delay.mul_(1.0001)
            for twin, real in zip(tensors(twins), tensors(data)):
                twin.copy_(real)
            got = tree(call(hip, twins, {}), lambda t: t.clone())
        hip.current_stream(refresh=True)
        torch.cuda.current_stream().wait_stream(s)
        assert results(got) == want, "on a stream of its own behind a delayed producer the entry gives other bytes"
    finally:
        hip.current_stream(refresh=True)
