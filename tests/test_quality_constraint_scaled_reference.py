"""The CPU restatement of the quality constraint's scaling passes (tests/quality_constraint_scaled_reference.py; DESIGN.md "Mesh
quality", 10.19), pinned: the finding the passes were built for -- on tiles_both the constraint without them ends nine of twelve
iterations in a full revert and freezes the mesh, with S = 2, r = 0.5, n = 1, P = 2 none does --, the two equivalences of the
contract by ==, the failure mode of a form that scales and never reverts, and the invariant through the report.  The figures are
the helper's own, with every margin of the parent references held on every judged evaluation, the scaled ones included."""
import functools

import numpy as np

import tangle_reference
from quality_constraint_all_reference import FIELDS_ALL, LAST_MARGIN
from quality_constraint_all_reference import reference_run as all_reference_run
from quality_constraint_full_reference import MORE_MARGIN
from quality_constraint_reference import FACE_MARGIN, OFF
from quality_constraint_scaled_reference import FIELDS_SCALED, reference_run
from test_gpu_quality_constraint import LIMITS
from test_gpu_tangle import CASES

PROTOTYPE = dict(scalePasses=2, errorReduction=0.5, nSmoothScale=1)


@functools.lru_cache(maxsize=None)
def _mesh(name):
    return CASES[name][0]()


def _check_margins(ref):
    assert ref.minMargin > tangle_reference.MARGIN and ref.minCosGap > FACE_MARGIN and ref.minSkewGap > FACE_MARGIN
    assert all(g > MORE_MARGIN for g in ref.minGap.values()) and all(g > LAST_MARGIN for g in ref.minGapLast.values())


def _run(oracle_lib, case, scaling, passes=2, n=None, variant="com", constraints=False):
    name, lim = LIMITS[case] if case in LIMITS else (case, {})
    r = reference_run(oracle_lib, _mesh(name), n or CASES[name][2], limits={**OFF, **lim}, passes=passes, variant=variant, constraints=constraints,
                      scaling=scaling, **CASES[name][1])
    _check_margins(r["ref"])
    assert all(list(c) == list(FIELDS_SCALED) for c in r["recs"])
    return r


def _col(r, k):
    return [c[k] for c in r["recs"]]


def _assert_invariant(r):
    """the report's measures of every accepted mesh: no bad face and no bad cell that is not exempt"""
    for p in r["pts"]:
        faces, cells = r["ref"].bad_now(p)
        assert not faces.any() and not cells.any()


def test_tiles_both_freezes_without_scaling_and_moves_with_it(oracle_lib):
    today = _run(oracle_lib, "tiles_both", None)
    assert _col(today, "fullRevert") == [0, 0, 0] + [1] * 9
    assert _col(today, "nPointsReverted") == [0, 10, 10] + [216] * 9
    # from iteration 4 on nothing moves any more
    assert all(np.array_equal(today["pts"][k], today["pts"][2]) for k in range(3, 12))
    r = _run(oracle_lib, "tiles_both", PROTOTYPE)
    assert _col(r, "fullRevert") == [0] * 12
    assert _col(r, "nPointsReverted") == [0, 0, 10, 10, 10] + [13] * 7 and max(_col(r, "nPointsReverted")) <= 13
    assert _col(r, "nPointsScaled") == [0, 25, 58, 62, 62, 74, 74, 74, 74, 74, 64, 64]
    assert _col(r, "passes") == [0, 1] + [3] * 10 and _col(r, "nScalePasses") == [0, 1] + [2] * 10
    assert _col(r, "minScale") == [1.0, 0.5] + [0.0] * 10
    assert not any(np.array_equal(r["pts"][k], r["pts"][k - 1]) for k in range(1, 12))
    _assert_invariant(today)
    _assert_invariant(r)


def test_scaling_without_sweeps_still_freezes(oracle_lib):
    """nSmoothScale = 0, factor 0.75: the nine full reverts stay -- the sweeps are part of the contract"""
    r = _run(oracle_lib, "tiles_both", dict(scalePasses=2, errorReduction=0.75, nSmoothScale=0))
    assert _col(r, "fullRevert") == [0, 0, 0] + [1] * 9 and _col(r, "nPointsScaled") == [0] * 12
    assert _col(r, "passes") == [0, 3, 3] + [4] * 9
    _assert_invariant(r)


def test_scale_passes_zero_is_the_parent_reference(oracle_lib):
    for case, variant, constraints in (("tiles_both", "com", False), ("cavity", "org", True)):
        name = LIMITS[case][0]
        a = _run(oracle_lib, case, None, variant=variant, constraints=constraints)
        b = all_reference_run(oracle_lib, _mesh(name), CASES[name][2], limits={**OFF, **LIMITS[case][1]}, variant=variant, constraints=constraints, **CASES[name][1])
        assert [{k: c[k] for k in FIELDS_ALL} for c in a["recs"]] == b["recs"] and any(c["nBadCells"] > 0 for c in b["recs"])
        assert all(np.array_equal(x, y) for x, y in zip(a["pts"], b["pts"]))
        assert all((c["nScalePasses"], c["nPointsScaled"], c["minScale"]) == (0, 0, 0.0) for c in a["recs"])


def test_factor_zero_without_sweeps_is_the_constraint_with_the_passes_added(oracle_lib):
    for case, S, P in (("tiles_both", 2, 2), ("cavity", 1, 1), ("dented", 3, 0)):
        name = LIMITS[case][0]
        a = _run(oracle_lib, case, dict(scalePasses=S, errorReduction=0.0, nSmoothScale=0), passes=P)
        b = all_reference_run(oracle_lib, _mesh(name), CASES[name][2], limits={**OFF, **LIMITS[case][1]}, passes=S + P, constraints=False, **CASES[name][1])
        assert all(np.array_equal(x, y) for x, y in zip(a["pts"], b["pts"]))
        assert [{k: c[k] for k in FIELDS_ALL} for c in a["recs"]] == b["recs"] and any(c["passes"] > 0 for c in b["recs"])
        assert all(c["nScalePasses"] == min(c["passes"], S) and c["nPointsScaled"] == 0 for c in a["recs"])
        assert all(c["minScale"] == (1.0 if c["nBadCells"] == 0 else 0.0) for c in a["recs"])


def test_dented_block_under_the_tangle_criteria_never_ends_in_a_full_revert(oracle_lib):
    """the failure mode of a form that only scales: there every later iteration of dented_block() is a full revert.  Here the
    reverting passes follow the scaling ones"""
    r = _run(oracle_lib, "dented", dict(scalePasses=2, errorReduction=0.75, nSmoothScale=0), n=12)
    pure = reference_run(oracle_lib, _mesh("dented"), 12, limits=dict(OFF), passes=2, constraints=False,
                         scaling=dict(scalePasses=2, errorReduction=0.75, nSmoothScale=0), **CASES["dented"][1])
    _check_margins(pure["ref"])
    for x in (r, pure):
        assert _col(x, "fullRevert") == [0] * 12 and any(c["nBadCells"] > 0 for c in x["recs"])
        _assert_invariant(x)
    assert all(c["nNonOrthoFaces"] == 0 and c["nSkewFaces"] == 0 and c["nBadCells"] == c["nTangledCells"] for c in pure["recs"])
    print(_col(pure, "nPointsReverted"), _col(pure, "nPointsScaled"), _col(pure, "passes"))


def test_cavity_cases_keep_moving(oracle_lib):
    """the issue's other two findings, on the helper's own figures: fewer reverted points on `cavity` (.org, the reference's
    constraints on), and a later first revert on cavity_band under the tangle criteria alone"""
    today = _run(oracle_lib, "cavity", None, variant="org", constraints=True)
    r = _run(oracle_lib, "cavity", PROTOTYPE, variant="org", constraints=True)
    assert _col(today, "nPointsReverted")[3:] == [4, 4, 4, 3, 3, 3, 3] and _col(r, "nPointsReverted")[3:] == [0, 1, 1, 1, 1, 1, 1]
    assert sum(_col(r, "fullRevert")) == 0 and any(c > 0 for c in _col(r, "nPointsScaled"))
    band0, band = _run(oracle_lib, "cavity_band", None), _run(oracle_lib, "cavity_band", PROTOTYPE)
    first = [next(i for i, c in enumerate(_col(x, "nPointsReverted"), start=1) if c > 0) for x in (band0, band)]
    assert first == [4, 7], first
    for x in (today, r, band0, band):
        _assert_invariant(x)


def test_records_describe_the_accepted_state(oracle_lib):
    """nPointsReverted, nPointsScaled and minScale against the scale field the iteration ended with"""
    name = LIMITS["tiles_both"][0]
    ref = reference_run(oracle_lib, _mesh(name), 0, limits={**OFF, **LIMITS["tiles_both"][1]}, constraints=False,
                        scaling=dict(scalePasses=3, errorReduction=0.5, nSmoothScale=2), passes=1, **CASES[name][1])["ref"]
    seen = False
    for _ in range(CASES[name][2]):
        x = ref.o.points().copy()
        cur, rec, _, _ = ref.step()
        s = ref.last_scale
        assert rec["minScale"] == s.min() and ((s >= 0.0) & (s <= 1.0)).all()
        assert np.array_equal(cur[s == 0.0], x[s == 0.0])
        assert rec["nPointsScaled"] <= int(((s > 0.0) & (s < 1.0)).sum()) and rec["nScalePasses"] <= min(rec["passes"], 3)
        seen = seen or (rec["nPointsScaled"] > 0 and rec["nPointsReverted"] > 0)
    assert seen
