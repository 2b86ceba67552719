"""GPU (-m gpu): the bytes of the registration sum kernels, pinned to the commit before they shared their tile front-end.

Every sum of these kernels has a fixed order and the histograms are integer, so a change that moves code between them
without changing an operation or its order writes the same bytes.  tests/golden/registration_bytes.json holds the sha1
of every output of
  - each MATRIX case (tests/sampling_cases.py; x extents 1, 5, 64 and 70) of the families similarity, msd, ncc, parzen,
    mi and ffd, through the runners of tests/test_sampling_matrix.py, with the case's masks where it has them;
  - the per-instantiation cases of tests/test_ffd_mi.py for k_parzen_hist<., ., true> and k_ffd_mi_force, through that
    file's check_hist and check_record,
as the commit named in the fixture ("parent_commit") computed them on an MI355X.  A digest that differs means that the
order of an operation changed: the code is what is wrong, not the fixture.

To regenerate (only when a pull request changes these bytes on purpose): build the library of the commit BEFORE the
change, and on an MI355X run, in a fresh process,
    SIFT3D_AMD_LIB=<that commit's libsift3d_amd.so> python -m tests.test_registration_bytes <that commit's hash> OUT.json
and commit OUT.json as the fixture.  Never generate it from the library under test."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from tests import sampling_cases as sc
from tests import test_ffd_mi as tfm
from tests import test_sampling_matrix as tsm
from tests import util

pytestmark = pytest.mark.gpu
FAMILIES = ("similarity", "msd", "ncc", "parzen", "mi", "ffd")
FIXTURE = os.path.join(util.GOLDEN, "registration_bytes.json")


def sha1(a):
    if isinstance(a, (int, np.integer)):
        a = np.int64(a).tobytes()
    elif not isinstance(a, bytes):
        a = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).tobytes()
    return hashlib.sha1(a).hexdigest()


def run_matrix(hip, c):
    return [sha1(b) for b in tsm.RUN[c.family](hip, c, sc.build(c))]


def run_hist_field(hip, nx, masked):
    """tests/test_ffd_mi.test_histogram_field_every_instantiation's case and calls"""
    c = sc.case("similarity", (4, 6, 70), (5, 6, nx), field=True, wf=masked, wm=masked, seed=40 + nx + masked)
    d = sc.build(c)
    out = []
    for bins in tfm.SOME_BINS:
        out += [sha1(a) for a in tfm.check_hist(hip, d.F, d.M, d.field, bins, "nx %d masked %s B=%d" % (nx, masked, bins),
                                                WF=d.WF, WM=d.WM)]
    return out


def run_mi_force(hip, nx, masked):
    """tests/test_ffd_mi.test_record_every_instantiation's case through check_record, and the same evaluation once more
    for the outputs that check_record does not return: the record (n, S_pp, R, gmax, Gc, dR), the gradient and the
    field"""
    fshape, mshape, spacing = ((5, 6, 70), (6, 5, 64), (7, 3, 2)) if nx >= 2 else ((4, 6, 64), (5, 6, 1), (5, 2, 3))
    c = sc.case("ffd", fshape, mshape, wf=masked, wm=masked, spacing=spacing, seed=60 + nx + masked)
    d = sc.build(c)
    rec = tfm.check_record(hip, d.F, d.M, d.lattice, spacing, d.A, 19, "nx %d masked %s" % (nx, masked), WF=d.WF,
                           WM=d.WM)[0]
    u = tfm.fr.field(d.lattice, spacing, d.F.shape, d.A)
    W = tfm.am.measures(tfm.fm.histogram_field(d.F, d.M, u, 19, tfm.RF, tfm.RM, d.WF, d.WM)[0]).W      # check_record's
    again = hip.ffd_mi_evaluate(tfm.dev(d.F), tfm.dev(d.M), tfm.dev(d.lattice), spacing, W, tfm.RF, tfm.RM, d.A,
                                bending=0.01, mask_fixed=tfm.opt(d.WF), mask_moving=tfm.opt(d.WM))
    out = [sha1(a) for a in again]
    assert out[0] == sha1(rec)
    return out


def _entries():
    out = [("%s %s" % (c.family, tsm.ident(c)), run_matrix, (c,)) for c in sc.MATRIX if c.family in FAMILIES]
    for masked in (False, True):
        out += [("parzen field nx %d masked %d" % (nx, masked), run_hist_field, (nx, masked)) for nx in (70, 1)]
        out += [("ffd mi nx %d masked %d" % (nx, masked), run_mi_force, (nx, masked)) for nx in (64, 1)]
    return out


ENTRIES = _entries()


@pytest.fixture(scope="module")
def hip():
    from sift3d_amd import hip as h
    h.lib()
    return h


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_every_case(golden):
    assert len(golden["parent_commit"]) == 40
    assert sorted(golden["sha1"]) == sorted(e[0] for e in ENTRIES)


@pytest.mark.parametrize("name, run, args", [pytest.param(*e, id=e[0]) for e in ENTRIES])
def test_bytes_are_the_parent_commits(hip, golden, name, run, args):
    got = run(hip, *args)
    assert got == golden["sha1"][name], name


if __name__ == "__main__":
    from sift3d_amd import hip as h
    h.lib()
    commit, path = sys.argv[1], sys.argv[2]
    assert len(commit) == 40 and os.environ.get("SIFT3D_AMD_LIB"), "the parent commit's hash and its library"
    digests = {name: run(h, *args) for name, run, args in ENTRIES}
    with open(path, "w") as f:
        json.dump({"parent_commit": commit, "device": "MI355X (gfx950)", "sha1": digests}, f, indent=1)
        f.write("\n")
    print("wrote %d entries to %s" % (len(digests), path))
