"""The CPU restatement of the tangle constraint and the quality constraint over boundary point smoothing
(tests/boundary_revert_reference.py; DESIGN.md "Mesh quality", 10.21), pinned on the three meshes the contract was settled on.
Records are written (nBadCells, passes, fullRevert, nPointsReverted).  Settings: the .com variant, maxStepLength 1,
minEdgeLength 1e-4, every patch a smoothing patch.

Case B as the issue states it -- hex_block(12, 8, 4), the column x = y = 0.5 dented, box_feature_edges(4), box_surface(2) -- first
tangles at iteration 5, its full revert counts 482 points and its smallest margin is 0.0282; the issue's table gives iteration 4, 391
points and 0.0128 for it, which this mesh does not reproduce under any setting tried (its figures for A and C reproduce exactly).
The case is kept as stated and pinned at what it computes."""
import numpy as np
import pytest

import boundary_revert_reference as br
from quality_constraint_all_reference import FIELDS_ALL
from tangle_reference import FIELDS, MARGIN

ZERO = (0, 0, 0, 0)
# the limits of the tiered runs on case C: one face limit and one cell limit (tests/test_gpu_boundary_revert.py takes them from here)
TIER_LIMITS = dict(minTwist=0.9, minVol=0.012)
TIER_COUNTS = {"minTwist": "nLowTwistFaces", "minVol": "nSmallVolumeCells"}


def short(recs):
    return [(r["nBadCells"], r["passes"], r["fullRevert"], r["nPointsReverted"]) for r in recs]


def first_bad(oracle_lib, name, constraints=False):
    """the first iteration (1-based) after which the loop alone has a bad cell, and the counts"""
    free = br.unconstrained_run(oracle_lib, name, br.ITERS[name], constraints=constraints)
    bad = br.bad_counts(oracle_lib, name, free)
    return next(i + 1 for i, b in enumerate(bad) if b), bad


def test_case_a(oracle_lib):
    at, bad = first_bad(oracle_lib, "A")
    assert at == 3 and bad == [0, 0] + [4] * 8
    for passes in (2, 1):
        r = br.reference_run(oracle_lib, "A", passes=passes)
        assert r["ref"].nExemptCells == 0
        assert short(r["recs"]) == [ZERO, ZERO] + [(4, 1, 0, 18)] * 8
        assert [c["iteration"] for c in r["recs"]] == list(range(1, 11))
        assert 0.0268 < r["ref"].minMargin < 0.0270
        # the invariant: no cell is bad at the accepted points (no cell of this mesh is exempt)
        assert br.bad_counts(oracle_lib, "A", r["pts"]) == [0] * 10
    r = br.reference_run(oracle_lib, "A", passes=0)
    assert short(r["recs"]) == [ZERO, ZERO] + [(4, 0, 1, 108)] * 8
    assert all(np.array_equal(p, r["pts"][1]) for p in r["pts"][2:])


def test_case_a_under_the_references_constraints(oracle_lib):
    at, _ = first_bad(oracle_lib, "A", constraints=True)
    assert at == 5
    r = br.reference_run(oracle_lib, "A", passes=2, constraints=True)
    assert short(r["recs"]) == [ZERO] * 4 + [(4, 1, 0, 17)] * 6
    assert 0.0077 < r["ref"].minMargin < 0.0078
    assert br.bad_counts(oracle_lib, "A", r["pts"]) == [0] * 10


def test_case_b_several_tiles(oracle_lib):
    assert br.case("B")[0].nPoints == 585
    at, _ = first_bad(oracle_lib, "B")
    assert at == 5
    r = br.reference_run(oracle_lib, "B", passes=2)
    assert short(r["recs"]) == [ZERO] * 4 + [(4, 1, 0, 18)] * 4
    assert 0.0281 < r["ref"].minMargin < 0.0283
    assert br.bad_counts(oracle_lib, "B", r["pts"]) == [0] * 8
    r = br.reference_run(oracle_lib, "B", passes=0)
    assert short(r["recs"]) == [ZERO] * 4 + [(4, 0, 1, 482)] * 4


def test_case_c_normals_that_move(oracle_lib):
    at, _ = first_bad(oracle_lib, "C")
    assert at == 6
    r = br.reference_run(oracle_lib, "C", passes=2)
    assert short(r["recs"]) == [ZERO] * 5 + [(4, 1, 0, 18)] * 7
    assert 2.4e-3 < r["ref"].minMargin < 2.6e-3
    assert br.bad_counts(oracle_lib, "C", r["pts"]) == [0] * 12
    # the normals are the loop's: every iteration blends them once, those whose points went back included
    n = r["normals"]
    assert all(not np.array_equal(n[k], n[k + 1]) for k in range(11))
    r0 = br.reference_run(oracle_lib, "C", passes=0)
    assert short(r0["recs"]) == [ZERO] * 5 + [(4, 0, 1, 125)] * 7
    assert 1.6e-3 < r0["ref"].minMargin < 1.8e-3
    # a full revert puts every point back and no normal: the points repeat, the normals go on
    assert np.array_equal(r0["pts"][6], r0["pts"][5]) and not np.array_equal(r0["normals"][6], r0["normals"][5])


def test_margins_hold_with_room(oracle_lib):
    for name in "ABC":
        for passes in (0, 1, 2):
            assert br.reference_run(oracle_lib, name, passes=passes)["ref"].minMargin > 1e9 * MARGIN


def test_quality_constraint_all_off_is_the_tangle_reference(oracle_lib):
    for name, constraints in (("C", False), ("A", True)):
        t = br.reference_run(oracle_lib, name, passes=2, constraints=constraints)
        q = br.reference_run(oracle_lib, name, passes=2, constraints=constraints, limits={})
        assert [{k: c[k] for k in FIELDS} for c in q["recs"]] == t["recs"]
        assert all(c["nTangledCells"] == c["nBadCells"] for c in q["recs"])
        assert all(c[k] == 0 for c in q["recs"] for k in FIELDS_ALL if k not in FIELDS and k != "nTangledCells")
        assert all(np.array_equal(a, b) for a, b in zip(q["pts"], t["pts"]))
        assert all(np.array_equal(a, b) for a, b in zip(q["normals"], t["normals"]))


def test_quality_constraint_tiers_fire(oracle_lib):
    """each of the two limits fires in at least three of the 12 iterations in which no cell is tangled: on cells the tangle
    criterion does not flag"""
    r = br.reference_run(oracle_lib, "C", passes=2, limits=TIER_LIMITS)
    ref = r["ref"]
    assert (ref.nExemptCells, ref.nExemptFaces, ref.nExemptVolumeCells) == (0, 28, 4)
    for limit, count in TIER_COUNTS.items():
        fired = [c["iteration"] for c in r["recs"] if c[count] > 0 and c["nTangledCells"] == 0]
        assert len(fired) >= 3, (limit, fired)
    assert [c["nLowTwistFaces"] for c in r["recs"]] == TIER_KNOWN["nLowTwistFaces"]
    assert [c["nSmallVolumeCells"] for c in r["recs"]] == TIER_KNOWN["nSmallVolumeCells"]
    assert short(r["recs"]) == TIER_KNOWN["short"]
    faces, cells = ref.bad_now(r["pts"][-1])
    assert not faces.any() and not cells.any()
    # each limit alone
    for limit, count in TIER_COUNTS.items():
        one = br.reference_run(oracle_lib, "C", passes=2, limits={limit: TIER_LIMITS[limit]})
        assert sum(1 for c in one["recs"] if c[count] > 0 and c["nTangledCells"] == 0) >= 3, limit


TIER_KNOWN = {
    "nLowTwistFaces": [4] + [8] * 11,
    "nSmallVolumeCells": [0] + [3] * 11,
    "short": [(4, 1, 0, 17)] + [(8, 2, 0, 35)] * 11,
}
