"""The boundary point smoothing at its edges, against the CPU oracle BY BITS: np.array_equal on hit points and coordinates,
equal hit flags, equal nFrozenPoints series, equal iteration counts (the residuals keep the 1e-10 relative rule).  The inputs
are tests/bnd_edge_cases.py; tests/test_boundary_edge_inputs.py holds what the oracle alone says about them.

  A. the segment query (kernels_boundary.hpp findLine: float boxes, parameter window, tie rule) against the oracle's test of
     every triangle, on surfaces and segments chosen for the culling's and the triangle test's edges.  (The in-plane segments
     are why the traversal no longer skips boxes entered beyond its best hit: in a triangle's own plane the parameter is a
     quotient of rounding errors and says nothing about where the triangle's box lies on the segment.)
  B. k_bnd_feature on strings of more than 64 target edges (second trip of a lane, reduction over 64 live lanes)
  C. whole runs away from the origin and in other units
  D. the OpenFOAM.org geometry with boundary smoothing and layers (k_geom_tile_bnd<T, true>)

isSharpEdgePoint is not compared after the runs: the engine keeps it as a bit of its per-boundary-point flags and exposes it
neither through debug_field nor through any other entry."""
import numpy as np
import pytest

import bnd_edge_cases as bec
from test_gpu_boundary import _check_setup

pytestmark = pytest.mark.gpu


def _run_both_by_bits(o, e, iters):
    n_o, res_o, frz_o = o.iterate(iters, 0.0)
    n_g, res_g, frz_g = e.iterate(iters, 0.0)
    assert n_o == n_g == iters and np.array_equal(frz_o, frz_g)
    assert np.max(np.abs(res_o - res_g) / np.maximum(res_o, 1e-300)) <= 1e-10
    po, pg = o.points(), e.get_points()
    bad = np.flatnonzero((po != pg).any(axis=1))
    assert np.array_equal(po, pg), "%d points differ, first %d: %r / %r" % (len(bad), bad[0], po[bad[0]], pg[bad[0]])


# ---- A ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(bec.SURFACES))
def test_find_line_at_its_edges(oracle_lib, name):
    """every family of segments on one surface in one launch: the hit flag is the oracle's, and where it hits the point is the
    oracle's bit for bit"""
    want = bec.oracle_hits(oracle_lib, name)
    segs = bec.segments(name)
    o, e, on = bec.attach(oracle_lib, bec.surface(name)[1], engine=True)
    assert on
    a = np.concatenate([segs[f][0] for f in bec.FAMILIES])
    b = np.concatenate([segs[f][1] for f in bec.FAMILIES])
    hit_g, p_g = e.debug_find_line(a, b)
    report = {}
    for k, fam in enumerate(bec.FAMILIES):
        sl = slice(k * bec.N_SEG, (k + 1) * bec.N_SEG)
        hit_o, p_o = want[fam]
        flags = int((hit_o != hit_g[sl]).sum())
        points = int((hit_o & hit_g[sl] & (p_o != p_g[sl]).any(axis=1)).sum())
        print("%-22s oracle hits %3d  flags differ %3d  points differ %3d" % (fam, hit_o.sum(), flags, points))
        if flags or points:
            report[fam] = (flags, points)
    assert not report, "family: (hit flags that differ, hit points that differ) " + repr(report)


# ---- B ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("constraints", [False, True])
@pytest.mark.parametrize("m,crowded", bec.STRING_SEGMENTS)
def test_long_feature_edge_strings(oracle_lib, m, crowded, constraints):
    """strings of m target edges: exactly one wave of lanes, one more (evenly spaced, and crowded so that the
    65th edge is the one nearest to most neighbours: bnd_edge_cases.STRING_SEGMENTS), and two trips plus a remainder.
    A feature edge point cannot reach k_bnd_feature without a string (featString < 0, the scan over all edges): a point is
    only classified as one when initial and target edge mesh have points, boundary.cpp's edgeStrings gives every target edge
    a string, and closestEdge (strict <, from GREAT) always takes some edge when all distances are finite -- so pointStrings
    is >= 0 for every feature edge point whenever the kernel is launched; there is no case to add."""
    from bnd_cases import make_pair
    mesh, init, target, surf = bec.long_string_case(m, crowded)
    o, e, prm, on = make_pair(mesh, oracle_lib, init, target, surf, constraints=constraints)
    assert on and e.boundary_info["nTargetEdgeStrings"] == 12 and e.boundary_info["nFeatureEdgePoints"] == 48
    _check_setup(o, e)
    _run_both_by_bits(o, e, 6)


# ---- C ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warp", [None, 1.03])
@pytest.mark.parametrize("frame", list(bec.OTHER_FRAMES))
def test_other_frames(oracle_lib, frame, warp):
    """mesh, edges and surface moved and scaled together.  By bits: one ulp at 1e5 is 1.5e-11, far above 1e-13 of the mesh's
    diagonal, so a tolerance relative to the coordinates would mean nothing there"""
    from bnd_cases import make_pair
    mesh, init, target, surf = bec.framed_case(frame, warp)
    o, e, prm, on = make_pair(mesh, oracle_lib, init, target, surf, constraints=True)
    assert on
    _check_setup(o, e)
    assert e.boundary_info["nCornerPoints"] == 8 and e.boundary_info["nFeatureEdgePoints"] == 48
    _run_both_by_bits(o, e, 6)


# ---- D ----------------------------------------------------------------------------------------------------------------
ORG_ENV = [{}, {"SMGPU_TILES": "0"}, {"SMGPU_GEOM_T": "128", "SMGPU_SMOOTH_T": "128"}]


@pytest.mark.parametrize("constraints", [False, True])
@pytest.mark.parametrize("env", ORG_ENV, ids=["tiles", "direct", "T128"])
def test_org_geometry_with_boundary_smoothing_and_layers(oracle_lib, monkeypatch, env, constraints):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    mesh, init, target, surf = bec.org_boundary_case()
    o, e, prm, on = bec.make_pair_variant(mesh, oracle_lib, init, target, surf, "org", constraints=constraints, layerPatches=("xmin",),
                                          blend=0.4)
    assert on
    _check_setup(o, e)
    _run_both_by_bits(o, e, 8)


def test_org_geometry_with_layers_alone(oracle_lib):
    o, e, prm, on = bec.make_pair_variant(bec.org_layers_case(), oracle_lib, None, None, None, "org", layerPatches=("xmin",),
                                          layerExpansionRatio=1.2)
    assert on
    _run_both_by_bits(o, e, 10)


def test_org_geometry_decomposed_with_boundary_smoothing_and_layers(oracle_lib):
    from smoothmesh_amd import BoundaryParams, LayerParams
    from smoothmesh_amd.halo import LocalMultiSmoother
    from smoothmesh_amd.surfgen import box_feature_edges, box_surface
    mo, orcs, subs, hi = bec.decomposed_case(oracle_lib, "org")
    prm = mo.params
    ms = LocalMultiSmoother(subs, device=0)
    for st in ms.states:
        st.eng.set_foam_variant("org")
    ms.set_params(prm)
    assert ms.set_layers(LayerParams(layerPatches=("xmin", "zmax")), prm.minEdgeLength)
    infos = ms.set_boundary_smoothing(BoundaryParams(initEdges=box_feature_edges(8, hi=hi), targetSurfaces=box_surface(4, hi=hi),
                                                     internalSmoothingBlendingFraction=0.4), prm.minEdgeLength)
    assert all(i["enabled"] for i in infos)
    for o, i in zip(orcs, infos):
        f = o.boundary_fields()
        assert i["nCornerPoints"] == f["isCornerPoint"].sum() and i["nFeatureEdgePoints"] == f["isFeatureEdgePoint"].sum()
    n_o, res_o, frz_o = mo.iterate(8, 0.0)
    n_g, res_g, frz_g = ms.iterate(8, 0.0)
    assert n_o == n_g == 8 and np.array_equal(frz_o, frz_g)
    assert np.max(np.abs(res_o - res_g) / np.maximum(res_o, 1e-300)) <= 1e-10
    for o, p in zip(orcs, ms.get_points()):
        assert np.array_equal(p, o.points())
