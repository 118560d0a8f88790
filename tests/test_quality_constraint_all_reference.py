"""The CPU restatement of the quality constraint's last four limits -- maxConcave, minFlatness, minVol, minArea
(tests/quality_constraint_all_reference.py; DESIGN.md "Mesh quality", 10.18) on the cases the limits were chosen on: the reference's
constraints off, the .com variant, the parameters of CASES in tests/test_gpu_tangle.py.  The limits were chosen on the CPU with this
helper under 10.16's condition, asserted here: each criterion, alone and with the other twelve off, gives a non-zero count in some
iteration, with every margin held."""
import functools

import numpy as np
import pytest

import tangle_reference
from quality_constraint_all_reference import FIELDS_ALL, LAST, LAST_MARGIN, LAST_OFF, QualityConstraintAllReference, reference_run
from quality_constraint_full_reference import FIELDS_FULL, MORE, MORE_MARGIN
from quality_constraint_full_reference import reference_run as full_reference_run
from quality_constraint_reference import FACE_MARGIN, OFF
from test_gpu_tangle import CASES
from test_quality_constraint_full_reference import LIMITS as FULL_LIMITS

# name -> (mesh of CASES, the limits; a criterion not named is off).  The single-criterion cases but the last start with every
# value on the good side of their limit (DESIGN.md 10.18 has the values on either side of each crossing).  dented_tiles starts with
# four faces that carry a 90 degree concave corner, which are exempt under maxConcave 40, and four with a 24.4 degree one, which the
# unconstrained run takes from 38.0 to 40.6 degrees in its sixth iteration, two iterations before 10.12 first reverts there (under
# the issue's candidate, maxConcave 80, nothing fired in twelve iterations: the largest non-exempt corner reaches 64.5 degrees).  "all" is the thirteen limits together on
# cavity_interface, the four set so that some elements start beyond them and are exempt (flatness 0.891 x 4, area 2.66e-3 x 2, volume
# 2.05e-4 x 1) and the next ones cross in the first iteration (flatness 0.921 -> 0.904, area 3.9e-3 -> 3.2e-3, volume 2.44e-4 ->
# 2.21e-4), next to the concave corners; the weight limit is 0.2, under which the run moves on (10.16's 0.32 reverts 948 faces in
# every iteration).  "vol_exempt" puts minVol above the smallest cells of cavity_band, which are volume-exempt, and a face limit
# beside it.
LIMITS = {
    "flatness": ("cavity_interface", dict(minFlatness=0.7)),
    "area": ("cavity_interface", dict(minArea=0.002)),
    "concave": ("cavity_interface", dict(maxConcave=60.0)),
    "vol": ("cavity_band", dict(minVol=1.6e-4)),
    "band_concave": ("cavity_band", dict(maxConcave=45.0)),
    "tiles_concave": ("dented_tiles", dict(maxConcave=40.0)),
    "all": ("cavity_interface", dict(**{**FULL_LIMITS["all"][1], "minFaceWeight": 0.2}, maxConcave=60.0, minFlatness=0.91, minVol=2.3e-4, minArea=0.0035)),
    "vol_exempt": ("cavity_band", dict(minVol=2.0e-4, maxConcave=45.0)),
}
SINGLE = [c for c in LIMITS if c not in ("all", "vol_exempt")]


@functools.lru_cache(maxsize=None)
def _mesh(name):
    return CASES[name][0]()


def _check_margins(ref):
    assert ref.minMargin > tangle_reference.MARGIN and ref.minCosGap > FACE_MARGIN and ref.minSkewGap > FACE_MARGIN
    assert all(g > MORE_MARGIN for g in ref.minGap.values()), ref.minGap
    assert all(g > LAST_MARGIN for g in ref.minGapLast.values()), ref.minGapLast


@functools.lru_cache(maxsize=None)
def _run(oracle_lib, case, passes=2):
    name = LIMITS[case][0]
    r = reference_run(oracle_lib, _mesh(name), CASES[name][2], limits={**OFF, **LIMITS[case][1]}, passes=passes, constraints=False, **CASES[name][1])
    _check_margins(r["ref"])
    return r


def _assert_invariant(r):
    for p in r["pts"]:
        faces, cells = r["ref"].bad_now(p)
        assert not faces.any() and not cells.any()


@pytest.mark.parametrize("case", SINGLE)
def test_each_criterion_alone_fires_and_keeps_the_invariant(oracle_lib, case):
    r = _run(oracle_lib, case)
    (limit,) = LIMITS[case][1]
    count = LAST[limit][1]
    print(case, [c[count] for c in r["recs"]], r["ref"].minGapLast)
    assert any(c[count] > 0 for c in r["recs"]), "no limit is met: the case tests nothing"
    for c in r["recs"]:
        assert list(c) == list(FIELDS_ALL)
        assert all(c[LAST[k][1]] == 0 for k in LAST if k != limit) and all(c[MORE[k][1]] == 0 for k in MORE)
        assert c["nNonOrthoFaces"] == 0 and c["nSkewFaces"] == 0
        assert (c["nBadCells"] > c["nTangledCells"]) == (c[count] > 0)       # a bad element of the criterion makes a cell bad
    gaps = ("cornerSin", "cornerSide") if limit == "maxConcave" else (limit,)
    assert all(np.isfinite(r["ref"].minGapLast[g]) for g in gaps)             # something was judged
    _assert_invariant(r)


def test_the_chosen_limits_start_on_the_good_side_or_exempt(oracle_lib):
    for case in SINGLE:
        ref = _run(oracle_lib, case)["ref"]
        if case == "tiles_concave":                                            # four faces start with a 90 degree concave corner
            assert ref.nExemptFaces == 4 and ref.nExemptVolumeCells == 0
        else:
            assert ref.nExemptFaces == 0 and ref.nExemptVolumeCells == 0, case


def test_all_four_off_is_the_parent_reference(oracle_lib):
    name = "cavity_interface"
    lim = {**OFF, **FULL_LIMITS["all"][1]}
    a = reference_run(oracle_lib, _mesh(name), CASES[name][2], limits={**lim, **{k: None for k in LAST}}, constraints=False, **CASES[name][1])
    b = full_reference_run(oracle_lib, _mesh(name), CASES[name][2], limits=lim, constraints=False, **CASES[name][1])
    assert [{k: c[k] for k in FIELDS_FULL} for c in a["recs"]] == b["recs"] and any(c["nBadCells"] > 0 for c in b["recs"])
    assert all(c[LAST[k][1]] == 0 for c in a["recs"] for k in LAST)
    assert all(np.array_equal(x, y) for x, y in zip(a["pts"], b["pts"]))
    assert np.array_equal(a["ref"].exemptFaces, b["ref"].exemptFaces) and np.array_equal(a["ref"].exemptDet, b["ref"].exemptDet)
    assert a["ref"].nExemptVolumeCells == 0
    # the off values themselves are off
    c = reference_run(oracle_lib, _mesh(name), CASES[name][2], limits={**lim, **LAST_OFF}, constraints=False, **CASES[name][1])
    assert c["recs"] == a["recs"]


@pytest.mark.parametrize("passes", [2, 0])
def test_all_thirteen_together(oracle_lib, passes):
    r = _run(oracle_lib, "all", passes)
    print(r["ref"].minGap, r["ref"].minGapLast)
    assert sum(x["nBadCells"] > 0 for x in r["recs"]) >= 2
    assert all(any(x[LAST[k][1]] > 0 for x in r["recs"]) for k in LAST) and any(x[MORE[k][1]] > 0 for x in r["recs"] for k in MORE)
    ref = r["ref"]
    assert ref.nExemptVolumeCells == 1 and ref.nExemptDeterminantCells == 4 and ref.nExemptFaces == 10
    assert all(x["passes"] == 0 and x["fullRevert"] == 1 for x in r["recs"] if x["nBadCells"] > 0) or passes > 0
    _assert_invariant(r)


def test_a_volume_exempt_cell_still_turns_bad_through_a_face(oracle_lib):
    r = _run(oracle_lib, "vol_exempt")
    ref = r["ref"]
    c = ref.exemptVol
    assert ref.nExemptVolumeCells > 0 and ref.nExemptCells == 0
    assert any(x["nConcaveFaces"] > 0 for x in r["recs"])
    _assert_invariant(r)
    # the exempt cells never count under the volume criterion, and one of them turns bad through a concave face
    name = "cavity_band"
    m = _mesh(name)
    twin = QualityConstraintAllReference(tangle_reference.make_oracle(oracle_lib, m, "com", False, **CASES[name][1]), m, **{**OFF, **LIMITS["vol_exempt"][1]})
    hit = False
    for _ in range(CASES[name][2]):
        x = twin.o.points().copy()
        twin.o.iterate(1, 0.0)
        moved = twin.o.points().copy()
        twin.bad_cells(moved, judge=False)
        hit = hit or bool(twin.byLastFace[c].any())
        twin.o.set_points(x)
        twin.step()
    assert hit, "no volume-exempt cell ever turns bad through a face: the case tests nothing"
