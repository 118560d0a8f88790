"""The CPU restatement of the quality constraint (tests/quality_constraint_reference.py; DESIGN.md "Mesh quality", 10.14) on the
cases the design was settled on: the reference's constraints off, the .com variant, the parameters of CASES in
tests/test_gpu_tangle.py.  The tuples are (passes, fullRevert, nBadCells, nPointsReverted) per iteration."""
import functools

import numpy as np
import pytest

import tangle_reference
from quality_constraint_reference import FACE_MARGIN, OFF, SHARED, reference_run
from test_gpu_tangle import CASES
from test_quality_reference import tangled_block


@functools.lru_cache(maxsize=None)
def _mesh(name):
    return CASES[name][0]()


@functools.lru_cache(maxsize=None)
def _run(oracle_lib, name, n, passes, limits):
    r = reference_run(oracle_lib, _mesh(name), n, limits={**OFF, **dict(limits)}, passes=passes, constraints=False, **CASES[name][1])
    assert r["ref"].minMargin > tangle_reference.MARGIN and r["ref"].minCosGap > FACE_MARGIN and r["ref"].minSkewGap > FACE_MARGIN
    return r


def _tuples(r):
    return [(c["passes"], c["fullRevert"], c["nBadCells"], c["nPointsReverted"]) for c in r["recs"]]


def _assert_invariant(r):
    ref = r["ref"]
    for p in r["pts"]:
        faces, cells = ref.bad_now(p)
        assert not faces.any() and not cells.any()


Z = (0, 0, 0, 0)


def test_dented_tiles_boundary_skewness(oracle_lib):
    r = _run(oracle_lib, "dented_tiles", 12, 2, (("maxBoundarySkewness", 0.1),))
    assert r["ref"].nExemptFaces == 0 and r["ref"].nExemptCells == 0
    assert _tuples(r) == [Z] + [(1, 0, 4, 10)] * 4 + [(2, 0, 4, 11)] * 2 + [(2, 0, 2, 10), Z] + [(1, 0, 5, 11)] * 3
    assert [c["iteration"] for c in r["recs"]] == list(range(1, 13))
    assert all(c["nTangledCells"] == 0 and c["nNonOrthoFaces"] == 0 for c in r["recs"])
    assert all((c["nSkewFaces"] > 0) == (c["nBadCells"] > 0) for c in r["recs"])
    _assert_invariant(r)


@pytest.mark.parametrize("passes,want", [(2, [Z] + [(1, 0, 4, 10)] * 2 + [(2, 1, 4, 216)] * 9), (1, [Z] + [(1, 0, 4, 10)] * 2 + [(1, 1, 4, 216)] * 9)])
def test_dented_tiles_both_skewness_limits(oracle_lib, passes, want):
    r = _run(oracle_lib, "dented_tiles", 12, passes, (("maxBoundarySkewness", 0.1), ("maxInternalSkewness", 0.4)))
    assert r["ref"].nExemptFaces == 8
    assert _tuples(r) == want
    for k in range(3, 12):                                   # from iteration 4 on the accepted points stay those of iteration 3
        assert np.array_equal(r["pts"][k], r["pts"][2])
    _assert_invariant(r)


def test_dented_tiles_internal_skewness(oracle_lib):
    r = _run(oracle_lib, "dented_tiles", 12, 2, (("maxInternalSkewness", 0.4),))
    assert r["ref"].nExemptFaces == 8
    t = _tuples(r)
    assert t[:5] == [Z] * 5 and t[5] == (1, 0, 4, 9) and t[6:] == [(2, 0, 4, 18)] * 6
    _assert_invariant(r)


CAVITY = (("maxNonOrtho", 40.0), ("maxInternalSkewness", 0.5), ("maxBoundarySkewness", 0.5))


def test_cavity_interface_non_orthogonality(oracle_lib):
    r = _run(oracle_lib, "cavity_interface", 10, 2, CAVITY)
    assert r["ref"].nExemptFaces == 8 and r["ref"].nExemptNonOrtho == 4
    assert _tuples(r) == [Z] * 8 + [(1, 0, 3, 6)] * 2
    assert r["recs"][8]["nNonOrthoFaces"] > 0
    _assert_invariant(r)
    r = _run(oracle_lib, "cavity_interface", 10, 0, CAVITY)
    t = _tuples(r)
    assert t[:8] == [Z] * 8 and all(x[:2] == (0, 1) and x[3] == 2070 for x in t[8:])
    _assert_invariant(r)


@pytest.mark.parametrize("name", ["dented", "cavity_interface"])
def test_all_criteria_off_is_the_tangle_constraint(oracle_lib, name):
    n = CASES[name][2]
    r = _run(oracle_lib, name, n, 2, ())
    t = tangle_reference.reference_run(oracle_lib, _mesh(name), n, passes=2, constraints=False, **CASES[name][1])
    assert r["ref"].nExemptFaces == 0
    assert [{k: c[k] for k in SHARED} for c in r["recs"]] == t["recs"]
    assert all(c["nTangledCells"] == c["nBadCells"] and c["nNonOrthoFaces"] == 0 and c["nSkewFaces"] == 0 for c in r["recs"])
    assert any(c["nBadCells"] > 0 for c in r["recs"])
    for a, b in zip(r["pts"], t["pts"]):
        assert np.array_equal(a, b)
    _assert_invariant(r)


def test_tangled_block_stays_exempt(oracle_lib):
    m = tangled_block()
    r = reference_run(oracle_lib, m, 6, limits=dict(maxNonOrtho=65.0, maxInternalSkewness=4.0, maxBoundarySkewness=20.0), constraints=False, maxStepLength=0.01)
    ref = r["ref"]
    assert ref.nExemptCells == 4 and ref.nExemptFaces > 0
    assert all(c["nTangledCells"] == 0 for c in r["recs"])
    _assert_invariant(r)
