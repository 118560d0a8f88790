"""The CPU restatement of the quality constraint's tet, twist, weight, ratio and determinant limits
(tests/quality_constraint_full_reference.py; DESIGN.md "Mesh quality", 10.16) on the cases the limits were chosen on: the
reference's constraints off, the .com variant, the parameters of CASES in tests/test_gpu_tangle.py.  The limits were chosen on the
CPU with this helper under one condition, asserted here: each criterion, alone and with the three old ones off, gives a non-zero
count in some iteration, with every margin held."""
import functools

import numpy as np
import pytest

import tangle_reference
from quality_constraint_full_reference import FIELDS_FULL, MORE, MORE_MARGIN, QualityConstraintFullReference, reference_run
from quality_constraint_reference import FACE_MARGIN, FIELDS, OFF
from quality_constraint_reference import reference_run as old_reference_run
from test_gpu_tangle import CASES

# name -> (mesh of CASES, the limits; a criterion not named is off).  cavity_interface starts with every value on the good side of
# its limit (lowest values: tet 3.8e-4, twist 0.39, triangle twist 0.42, weight 0.329, ratio 0.1117, determinant 0.0396) and the
# unconstrained run crosses each one; "all" puts the determinant limit above the four lowest cells (0.0396, 0.0914, 0.1227, 0.1227), which are exempt from it.
LIMITS = {
    "tet": ("cavity_interface", dict(minTetQuality=1e-4)),
    "twist": ("cavity_interface", dict(minTwist=0.05)),
    "triangle_twist": ("cavity_interface", dict(minTriangleTwist=0.05)),
    "weight": ("cavity_interface", dict(minFaceWeight=0.32)),
    "ratio": ("cavity_interface", dict(minVolRatio=0.11)),
    "determinant": ("cavity_interface", dict(minDeterminant=0.035)),
    "tiles_weight": ("dented_tiles", dict(minFaceWeight=0.425)),
    "all": ("cavity_interface", dict(maxNonOrtho=40.0, maxInternalSkewness=0.5, minTetQuality=1e-4, minTwist=0.05, minTriangleTwist=0.05, minFaceWeight=0.32,
                                     minVolRatio=0.11, minDeterminant=0.124)),
}


@functools.lru_cache(maxsize=None)
def _mesh(name):
    return CASES[name][0]()


@functools.lru_cache(maxsize=None)
def _run(oracle_lib, case, passes=2):
    name = LIMITS[case][0]
    r = reference_run(oracle_lib, _mesh(name), CASES[name][2], limits={**OFF, **LIMITS[case][1]}, passes=passes, constraints=False, **CASES[name][1])
    ref = r["ref"]
    assert ref.minMargin > tangle_reference.MARGIN and ref.minCosGap > FACE_MARGIN and ref.minSkewGap > FACE_MARGIN
    assert all(g > MORE_MARGIN for g in ref.minGap.values()), ref.minGap
    return r


def _assert_invariant(r):
    for p in r["pts"]:
        faces, cells = r["ref"].bad_now(p)
        assert not faces.any() and not cells.any()


@pytest.mark.parametrize("case", [c for c in LIMITS if c != "all"])
def test_each_criterion_alone_fires_and_keeps_the_invariant(oracle_lib, case):
    r = _run(oracle_lib, case)
    (limit,) = LIMITS[case][1]
    count = MORE[limit][1]
    assert any(c[count] > 0 for c in r["recs"]), "no limit is met: the case tests nothing"
    for c in r["recs"]:
        assert list(c) == list(FIELDS_FULL)
        assert all(c[MORE[k][1]] == 0 for k in MORE if k != limit) and c["nNonOrthoFaces"] == 0 and c["nSkewFaces"] == 0
        assert (c["nBadCells"] > c["nTangledCells"]) == (c[count] > 0)       # a bad element of the criterion makes a cell bad
    assert np.isfinite(r["ref"].minGap[limit])                                 # something was judged
    _assert_invariant(r)


def test_the_chosen_limits_start_on_the_good_side(oracle_lib):
    """no exempt element in the single-criterion cases on cavity_interface: each limit is crossed from the good side"""
    for case, (name, lim) in LIMITS.items():
        if name == "cavity_interface" and case != "all":
            ref = _run(oracle_lib, case)["ref"]
            assert ref.nExemptFaces == 0 and ref.nExemptDeterminantCells == 0, case


def test_all_six_off_is_the_parent_reference(oracle_lib):
    name = "cavity_interface"
    lim = {**OFF, **dict(maxNonOrtho=40.0, maxInternalSkewness=0.5, maxBoundarySkewness=0.5)}
    a = reference_run(oracle_lib, _mesh(name), CASES[name][2], limits={**lim, **{k: None for k in MORE}}, constraints=False, **CASES[name][1])
    b = old_reference_run(oracle_lib, _mesh(name), CASES[name][2], limits=lim, constraints=False, **CASES[name][1])
    assert [{k: c[k] for k in FIELDS} for c in a["recs"]] == b["recs"] and any(c["nBadCells"] > 0 for c in b["recs"])
    assert all(c[MORE[k][1]] == 0 for c in a["recs"] for k in MORE)
    assert all(np.array_equal(x, y) for x, y in zip(a["pts"], b["pts"]))
    assert np.array_equal(a["ref"].exemptFaces, b["ref"].exemptFaces) and a["ref"].nExemptDeterminantCells == 0
    # the off values themselves are off
    c = reference_run(oracle_lib, _mesh(name), CASES[name][2], limits={**lim, **{k: v[0] for k, v in MORE.items()}}, constraints=False, **CASES[name][1])
    assert c["recs"] == a["recs"]


@pytest.mark.parametrize("passes", [2, 0])
def test_all_criteria_together_and_exemption(oracle_lib, passes):
    r = _run(oracle_lib, "all", passes)
    ref = r["ref"]
    # the cells under-determined at enabling are exempt from the determinant criterion only: they never count there ...
    assert ref.nExemptDeterminantCells == 4 and ref.nExemptCells == 0
    c = ref.exemptDet
    assert sum(x["nBadCells"] > 0 for x in r["recs"]) >= 2
    assert all(x["passes"] == 0 and x["fullRevert"] == 1 for x in r["recs"] if x["nBadCells"] > 0) or passes > 0
    _assert_invariant(r)
    # ... and one of them still turns bad through a face that fails a limit
    m = _mesh("cavity_interface")
    twin = QualityConstraintFullReference(tangle_reference.make_oracle(oracle_lib, m, "com", False, **CASES["cavity_interface"][1]), m,
                                          **{**OFF, **LIMITS["all"][1]}, passes=passes)
    hit = False
    for _ in range(CASES["cavity_interface"][2]):
        x = twin.o.points().copy()
        twin.o.iterate(1, 0.0)
        moved = twin.o.points().copy()
        twin.bad_cells(moved, judge=False)
        hit = hit or bool(twin.byFace[c].any())            # (byFace leaves out the determinant verdict of a cell exempt from it)
        twin.o.set_points(x)
        twin.step()
    assert hit, "no determinant-exempt cell ever turns bad through a face: the case tests nothing"
