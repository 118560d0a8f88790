"""The oracle against RECORDED runs of the reference itself (tests/golden/reference_runs/*.npz, written by
make_reference_runs.py from oracle/_ref/libsmref.so): the same requirement as tests/test_reference_pin.py -- bit-equal points
after every iteration, equal nFrozenPoints, residuals equal as printed -- where the reference is not present."""
import glob
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_pin_cases as rp

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_runs")
FILES = sorted(os.path.basename(f) for f in glob.glob(os.path.join(HERE, "*.npz")))


def test_the_fixtures_are_there():
    assert len(FILES) >= 5, FILES


@pytest.mark.parametrize("name", FILES)
def test_oracle_reproduces_the_recorded_reference_run(oracle_lib, name):
    from smoothmesh_amd.mesh import Patch, PolyMesh
    z = np.load(os.path.join(HERE, name))
    patches = [Patch(str(n), str(t), int(s), int(st)) for n, t, s, st in zip(z["patchName"], z["patchType"], z["patchSize"], z["patchStart"])]
    m = PolyMesh(points=z["points"], faceOffsets=z["faceOffsets"], facePoints=z["facePoints"], owner=z["owner"], neighbour=z["neighbour"],
                 patches=patches, nCells=int(z["nCells"]))
    oracle_lib.set_acos_variant("glibc")
    pts, frz, res, _ = rp.oracle_series(oracle_lib, m, rp.args(str(z["options"])), str(z["variant"]))
    assert len(pts) == len(z["ref_points"]) and frz.tolist() == z["ref_nFrozenPoints"].tolist()
    for i, p in enumerate(pts):
        assert np.array_equal(p, z["ref_points"][i]), (name, "iteration", i + 1, rp.first_difference(p, z["ref_points"][i]))
    assert [rp.printed(r) for r in res] == [str(s) for s in z["ref_residuals"]]
