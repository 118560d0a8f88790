"""The CPU restatement of the tangle constraint (tests/tangle_reference.py; DESIGN.md "Mesh quality", 10.12) on the meshes whose
behaviour the design was settled on: the dented block tangles under the reference's own constraints and stays untangled under
this one, passes = 1 and 0 fall back to the full revert, and a mesh that starts tangled keeps its bad cells exempt."""
import numpy as np
import pytest

from tangle_reference import MARGIN, make_oracle, reference_run
from test_gpu_quality_trace import dented_block
from test_quality_reference import cell_faces, quality_reference, tangled_block

DENT = dict(maxStepLength=1.0, minEdgeLength=1e-4)


def _report(oracle_lib, mesh, pts, variant="com"):
    import copy
    m = copy.copy(mesh)
    m.points = np.array(pts)
    o = make_oracle(oracle_lib, m, variant)
    o.phaseA()
    fc, fa, cc = (o.field(k).reshape(-1, 3) for k in ("faceCentres", "faceAreas", "cellCentres"))
    return quality_reference(m, fc, fa, cc, *cell_faces(m))[0]


def _unconstrained(oracle_lib, mesh, n, constraints=False, **over):
    o = make_oracle(oracle_lib, mesh, "com", constraints, **over)
    out = []
    for _ in range(n):
        assert o.iterate(1, 0.0)[0] == 1
        out.append(o.points().copy())
    return out


def test_dented_block_stays_untangled(oracle_lib):
    m = dented_block()
    r = reference_run(oracle_lib, m, 8, passes=2, constraints=False, **DENT)
    assert r["ref"].nExemptCells == 0
    assert [c["iteration"] for c in r["recs"]] == list(range(1, 9))
    assert [c["passes"] for c in r["recs"]] == [1, 0, 1, 1, 1, 1, 2, 2]
    assert [c["nPointsReverted"] for c in r["recs"]] == [9, 0, 9, 9, 9, 9, 18, 18]
    assert [c["fullRevert"] for c in r["recs"]] == [0] * 8
    assert all((c["nBadCells"] > 0) == (c["passes"] > 0) for c in r["recs"])
    for p in r["pts"]:
        q = _report(oracle_lib, m, p)
        assert q["nNonPositiveVolume"] == 0 and q["nWrongOrientedFaces"] == 0
    assert r["ref"].minMargin > MARGIN
    # ... and without the constraint the same run tangles
    free = _unconstrained(oracle_lib, m, 8, **DENT)
    q1, q8 = _report(oracle_lib, m, free[0]), _report(oracle_lib, m, free[7])
    assert (q1["nNonPositiveVolume"], q1["nWrongOrientedFaces"]) == (0, 4)
    assert (q8["nNonPositiveVolume"], q8["nWrongOrientedFaces"]) == (16, 72)


def test_dented_block_fewer_passes(oracle_lib):
    m = dented_block()
    r = reference_run(oracle_lib, m, 8, passes=1, constraints=False, **DENT)
    assert [c["iteration"] for c in r["recs"] if c["fullRevert"]] == [7, 8]
    assert np.array_equal(r["pts"][6], r["pts"][5]) and np.array_equal(r["pts"][7], r["pts"][5])
    r = reference_run(oracle_lib, m, 8, passes=0, constraints=False, **DENT)
    assert all(c["fullRevert"] == 1 and c["passes"] == 0 and c["nBadCells"] > 0 for c in r["recs"])
    assert all(np.array_equal(p, m.points) for p in r["pts"])


def test_the_references_constraints_do_not_prevent_it(oracle_lib):
    m = dented_block()
    r = reference_run(oracle_lib, m, 8, passes=2, constraints=True, **DENT)
    assert r["recs"][0]["nBadCells"] > 0 and r["recs"][0]["passes"] >= 1
    for p in r["pts"]:
        q = _report(oracle_lib, m, p)
        assert q["nNonPositiveVolume"] == 0 and q["nWrongOrientedFaces"] == 0
    free = _unconstrained(oracle_lib, m, 8, constraints=True, **DENT)
    assert _report(oracle_lib, m, free[0])["nWrongOrientedFaces"] == 4
    assert _report(oracle_lib, m, free[7])["nWrongOrientedFaces"] == 12


def test_tangled_block_cells_are_exempt(oracle_lib):
    m = tangled_block()
    r = reference_run(oracle_lib, m, 6, passes=2, constraints=False, maxStepLength=0.01)
    assert r["ref"].nExemptCells == 4
    for k, c in enumerate(r["recs"], start=1):
        assert c == dict(iteration=k, passes=0, fullRevert=0, nBadCells=0, nPointsReverted=0)
    free = _unconstrained(oracle_lib, m, 6, maxStepLength=0.01)
    for a, b in zip(r["pts"], free):
        assert np.array_equal(a, b)
