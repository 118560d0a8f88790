"""What the oracle alone must say about the inputs of tests/bnd_edge_cases.py, so that no comparison of
test_gpu_boundary_edges.py is vacuous: the families that are meant to hit do, the ones meant to miss do, the knife-edge
families really have both outcomes, the doubled surface really shows which twin won, every short triangle list enables the
boundary smoothing, the long strings are twelve, the other frames classify as the unit block does, and the OpenFOAM.org
geometry moves the points elsewhere than the OpenFOAM.com one."""
import numpy as np
import pytest

import bnd_edge_cases as bec
from conftest import rel_linf

HITTING = ("through_vertex", "through_edge", "huge", "tiny_straddling")
ON_THE_SURFACE = ("end_on_face", "start_on_face", "start_on_edge_outward")      # t about 1, about 0, about 0


@pytest.mark.parametrize("form", bec.BOX_FORMS)
def test_families_meant_to_hit_do(oracle_lib, form):
    res = bec.oracle_hits(oracle_lib, form)
    for fam in HITTING:
        assert res[fam][0].sum() >= 0.9 * bec.N_SEG, (fam, int(res[fam][0].sum()))


@pytest.mark.parametrize("name", bec.BOX_FORMS + ("sphere", "doubled", "degenerate"))
def test_families_meant_to_miss_do(oracle_lib, name):
    res = bec.oracle_hits(oracle_lib, name)
    for fam in ("tiny_missing", "zero_length"):
        assert not res[fam][0].any(), (fam, int(res[fam][0].sum()))


def test_moved_surface_is_a_knife_edge(oracle_lib):
    """1e4 away the last bits of Moller-Trumbore decide whether a segment that starts or ends on a face hits it"""
    res = bec.oracle_hits(oracle_lib, "moved")
    counts = {fam: int(res[fam][0].sum()) for fam in ON_THE_SURFACE}
    assert sum(0.25 * bec.N_SEG <= c <= 0.75 * bec.N_SEG for c in counts.values()) >= 2, counts


def test_end_on_a_face_has_both_outcomes_at_the_origin(oracle_lib):
    n = int(bec.oracle_hits(oracle_lib, "origin")["end_on_face"][0].sum())
    assert 0.1 * bec.N_SEG <= n <= 0.9 * bec.N_SEG, n


def test_doubled_surface_shows_which_twin_won(oracle_lib):
    fwd, rev = bec.oracle_hits(oracle_lib, "doubled"), bec.oracle_hits(oracle_lib, "doubled_reversed")
    hits = differ = 0
    for fam in bec.FAMILIES:
        (hf, pf), (hr, pr) = fwd[fam], rev[fam]
        assert np.array_equal(hf, hr), fam               # the same segments (same seed) against the same triangles
        hits += int(hf.sum())
        differ += int((hf & (pf != pr).any(axis=1)).sum())
    assert hits >= 300 and differ >= 0.1 * hits, (hits, differ)


@pytest.mark.parametrize("n", bec.FIRST_N)
def test_short_triangle_lists_enable_and_are_hit(oracle_lib, n):
    pts, tris = bec.first_triangles(n)
    assert len(tris) == n
    o, _, on = bec.attach(oracle_lib, (pts, tris), engine=False)
    assert on
    hit = bec.oracle_hits(oracle_lib, "first%d" % n)["through_face"][0]
    assert hit[:100].sum() >= 50, int(hit[:100].sum())


def test_degenerate_surface_has_its_zero_area_triangles():
    pts, tris = bec.degenerate_box()
    base = bec.warped_box()[1]
    assert len(tris) == len(base) + bec.N_DEGENERATE
    area = np.linalg.norm(np.cross(pts[tris[:, 1]] - pts[tris[:, 0]], pts[tris[:, 2]] - pts[tris[:, 0]]), axis=1)
    assert (area == 0.0).sum() == bec.N_DEGENERATE
    pos = np.flatnonzero(area == 0.0)
    assert pos.min() < len(tris) // 2 < pos.max()        # spread over the list


def test_near_axis_directions_are_what_they_claim():
    a, b = bec.segments("origin")["near_axis"]
    d = np.abs(b - a)
    small = np.sort(d, axis=1)[:, 1]                      # the middle component: the tiny one
    assert np.all(np.sort(d, axis=1)[:, 0] == 0.0) and np.all(np.abs(d.max(axis=1) - 1.5) <= 4e-16)
    for k, tiny in enumerate(bec.NEAR_AXIS_TINY):
        s = small[k::4]
        assert (s == tiny).sum() >= 2 * len(s) // 3 - 1   # the two exact constructions
        assert np.all((s == tiny) | (s == 0.0) | (np.abs(s - tiny) <= 1.2e-16))


@pytest.mark.parametrize("m,crowded", bec.STRING_SEGMENTS)
def test_long_strings(oracle_lib, m, crowded):
    from bnd_cases import make_pair
    mesh, init, target, surf = bec.long_string_case(m, crowded)
    o, _, _, on = make_pair(mesh, oracle_lib, init, target, surf, engine=False)
    assert on
    f = o.boundary_fields()
    es = f["targetEdgeStrings"]
    strings, counts = np.unique(es, return_counts=True)
    assert len(strings) == 12 and np.all(counts == m)
    feat, corner = f["isFeatureEdgePoint"].astype(bool), f["isCornerPoint"].astype(bool)
    assert feat.sum() == 48 and corner.sum() == 8
    assert np.all(f["pointStrings"][feat] >= 0)
    # which place of its string (ascending edge id, the order of the device's scan) does the edge nearest to a surface
    # neighbour of a feature edge point have?  Beyond 63 means the answer comes from a lane's second trip.
    rank = np.zeros(len(es), int)
    for s in strings:
        rank[es == s] = np.arange(m)
    off, val = o.addressing("pointPoints")
    internal = np.asarray(mesh.find_internal_points(), bool)
    P, (tp, te) = o.points(), target
    a, b = tp[te[:, 0]], tp[te[:, 1]]
    places = []
    for p in np.flatnonzero(feat):
        mine = np.flatnonzero(es == f["pointStrings"][p])
        for q in val[off[p]:off[p + 1]]:
            if internal[q] or feat[q] or corner[q]:
                continue
            s = np.clip(((P[q] - a[mine]) * (b[mine] - a[mine])).sum(1) / ((b[mine] - a[mine]) ** 2).sum(1), 0.0, 1.0)
            d = np.linalg.norm(a[mine] + s[:, None] * (b[mine] - a[mine]) - P[q], axis=1)
            places.append(rank[mine[np.argmin(d)]])
    places = np.array(places)
    assert len(places) >= 48
    if m > 64 and (m, crowded) != (65, False):          # (evenly spaced, the 65th edge of 65 is nearest to nobody: hence the crowded case)
        assert (places >= 64).sum() >= 4, np.sort(places)[-8:]


@pytest.mark.parametrize("warp", [None, 1.03])
@pytest.mark.parametrize("frame", list(bec.OTHER_FRAMES))
def test_other_frames_classify_as_the_unit_block(oracle_lib, frame, warp):
    from bnd_cases import make_pair
    mesh, init, target, surf = bec.framed_case(frame, warp)
    o, _, _, on = make_pair(mesh, oracle_lib, init, target, surf, constraints=True, engine=False)
    assert on
    f = o.boundary_fields()
    assert f["isCornerPoint"].sum() == 8 and f["isFeatureEdgePoint"].sum() == 48
    x0 = o.points().copy()
    n, res, frz = o.iterate(6, 0.0)
    assert n == 6 and np.isfinite(res).all()
    assert np.abs(o.points() - x0).max() > 1e-3 * bec.bbox_diagonal(x0)          # the run moves the mesh


def _org_against_com(run):
    return rel_linf(run("org"), run("com"))


def test_org_geometry_differs_serial(oracle_lib):
    mesh, init, target, surf = bec.org_boundary_case()
    for constraints in (False, True):
        def run(variant):
            o, _, _, on = bec.make_pair_variant(mesh, oracle_lib, init, target, surf, variant, constraints=constraints,
                                                layerPatches=("xmin",), blend=0.4, engine=False)
            assert on
            o.iterate(8, 0.0)
            return o.points()
        assert _org_against_com(run) > 1e-4


def test_org_geometry_differs_layers_alone(oracle_lib):
    mesh = bec.org_layers_case()

    def run(variant):
        o, _, _, on = bec.make_pair_variant(mesh, oracle_lib, None, None, None, variant, layerPatches=("xmin",), engine=False,
                                            layerExpansionRatio=1.2)
        assert on
        o.iterate(10, 0.0)
        return o.points()
    assert _org_against_com(run) > 1e-4


def test_org_geometry_differs_decomposed(oracle_lib):
    def run(variant):
        mo, orcs, subs, hi = bec.decomposed_case(oracle_lib, variant)
        mo.iterate(8, 0.0)
        return np.concatenate([o.points() for o in orcs])
    assert _org_against_com(run) > 1e-4
