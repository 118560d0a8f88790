"""The tangle constraint, the quality constraint and the quality guard on an engine with boundary point smoothing (include/smgpu.h
smgpu_set_boundary_revert; DESIGN.md "Mesh quality", 10.21) against their CPU restatement (tests/boundary_revert_reference.py, pinned
by tests/test_boundary_revert_reference.py): the accepted points, every record field and the point normals after every iteration,
bit for bit; the tiers of the quality constraint; a constraint that never fires; the switch alone launches nothing; layers; the
guard's restore with its normals; refusals; `smoothMesh -boundaryRevert`."""
import functools
import os
import subprocess

import numpy as np
import pytest

import boundary_revert_reference as br
from quality_constraint_all_reference import FIELDS_ALL
from quality_constraint_reference import OFF
from tangle_reference import FIELDS
from test_boundary_revert_reference import TIER_COUNTS, TIER_LIMITS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "smoothmesh_amd", "bin", "smoothMesh")


@functools.lru_cache(maxsize=None)
def _reference(oracle_lib, name, variant, constraints, passes, limits=None, layerPatches=()):
    """computed once per configuration and shared"""
    return br.reference_run(oracle_lib, name, passes=passes, variant=variant, constraints=constraints,
                            limits=None if limits is None else dict(limits), layerPatches=layerPatches)


def _engine(inputs, variant="com", constraints=False, layerPatches=(), revert=True, **over):
    """an engine with boundary point smoothing (and layers) on inputs = (mesh, initEdges, targetEdges, targetSurfaces), set up as
    bnd_cases.make_pair sets its oracle up; the foam variant in front of any set-up"""
    from smoothmesh_amd import BoundaryParams, LayerParams, SmoothEngine, default_params
    mesh, init, target, surf = inputs
    e = SmoothEngine(mesh)
    e.set_foam_variant(variant)
    prm = default_params(e.mesh_stats()[0], edgeAngleConstraint=constraints, faceAngleConstraint=constraints, **over)
    e.set_params(prm)
    if layerPatches:
        assert e.set_layers(LayerParams(layerPatches=tuple(layerPatches)), prm.minEdgeLength)
    info = e.set_boundary_smoothing(BoundaryParams(initEdges=init, targetSurfaces=surf, targetEdges=target, smoothingPatches=('".*"',)),
                                    prm.minEdgeLength)
    assert info["enabled"]
    if revert:
        e.set_boundary_revert()
    return e


def _case_engine(name, variant="com", constraints=False, layerPatches=(), revert=True):
    return _engine(br.case(name), variant, constraints, layerPatches, revert, **br.PRM)


def _records(recs, fields=FIELDS):
    return [{k: getattr(r, k) for k in fields} for r in recs]


def _normals(e):
    return e.debug_field("layerNormals").reshape(-1, 3)


def _hold_to_reference(e, ref, records, fields):
    """iteration by iteration: the record, the accepted points and the point normals, by bits"""
    for k in range(len(ref["pts"])):
        n, res, frz = e.iterate(1, 0.0)
        assert n == 1
        rec = _records(records(), fields)
        assert rec == [ref["recs"][k]], (k, rec, ref["recs"][k])
        assert np.array_equal(e.get_points(), ref["pts"][k]), k
        assert np.array_equal(_normals(e), ref["normals"][k]), k
        # residual and nFrozenPoints stay the loop's own (10.12)
        assert float(res[0]) == ref["res"][k] and int(frz[0]) == ref["frz"][k], k


# ---- 1. engine = reference, by bits ------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["com", "org"])
@pytest.mark.parametrize("constraints", [False, True])
@pytest.mark.parametrize("passes", [0, 1, 2])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_tangle_constraint_equals_reference_bitwise(oracle_lib, name, passes, constraints, variant):
    ref = _reference(oracle_lib, name, variant, constraints, passes)
    e = _case_engine(name, variant, constraints)
    assert e.boundary_revert()
    e.set_tangle_constraint(passes)
    st = e.tangle_state()
    assert st.on and st.passes == passes and st.nExemptCells == ref["ref"].nExemptCells == 0 and st.iteration == 0
    _hold_to_reference(e, ref, e.tangle_records, FIELDS)
    assert e.tangle_state().iteration == br.ITERS[name]
    if (variant, constraints) == ("com", False):
        assert any(r["nBadCells"] > 0 for r in ref["recs"]), "the mesh does not tangle: the case tests nothing"


@pytest.mark.parametrize("env", [{"SMGPU_GEOM_T": "64"}, {"SMGPU_GEOM_T": "128"}, {"SMGPU_GEOM_T": "256"}, {"SMGPU_TILES": "0"}],
                         ids=["T64", "T128", "T256", "untiled"])
def test_tile_shapes_and_the_untiled_fallback(oracle_lib, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ref = _reference(oracle_lib, "C", "com", False, 2)
    e = _case_engine("C")
    e.set_tangle_constraint(2)
    _hold_to_reference(e, ref, e.tangle_records, FIELDS)


@pytest.mark.parametrize("side", ["0", "1"])
def test_side_stream_and_riding_normals(oracle_lib, monkeypatch, side):
    """the boundary pre-kernels on the side stream (forked behind the passes) and riding in the geometry launch: the same run"""
    monkeypatch.setenv("SMGPU_SIDE_STREAM", side)
    monkeypatch.setenv("SMGPU_BND_IN_GEOM", "0")
    ref = _reference(oracle_lib, "C", "com", False, 2)
    e = _case_engine("C")
    e.set_tangle_constraint(2)
    _hold_to_reference(e, ref, e.tangle_records, FIELDS)


def test_one_call_equals_iteration_by_iteration(oracle_lib):
    ref = _reference(oracle_lib, "C", "com", False, 2)
    e = _case_engine("C")
    e.set_tangle_constraint(2)
    n = br.ITERS["C"]
    assert e.iterate(n, 0.0)[0] == n
    assert _records(e.tangle_records()) == ref["recs"]
    assert np.array_equal(e.get_points(), ref["pts"][-1]) and np.array_equal(_normals(e), ref["normals"][-1])


# ---- 2. the quality constraint's tiers ---------------------------------------------------------------------------------
def test_quality_constraint_limits_equal_reference(oracle_lib):
    lim = {**OFF, **TIER_LIMITS}
    ref = _reference(oracle_lib, "C", "com", False, 2, tuple(sorted(TIER_LIMITS.items())))
    for count in TIER_COUNTS.values():
        assert sum(1 for c in ref["recs"] if c[count] > 0 and c["nTangledCells"] == 0) >= 3
    e = _case_engine("C")
    e.set_quality_constraint(passes=2, **lim)
    st, r = e.quality_constraint_state(), ref["ref"]
    assert (st.nExemptCells, st.nExemptFaces, st.nExemptDeterminantCells, st.nExemptVolumeCells) == (r.nExemptCells, r.nExemptFaces, r.nExemptDeterminantCells,
                                                                                                       r.nExemptVolumeCells)
    _hold_to_reference(e, ref, e.quality_constraint_records, FIELDS_ALL)


@pytest.mark.parametrize("limits", [{}, dict(minTwist=-1.0), dict(minVol=0.0)], ids=["three", "limits", "limits_all"])
def test_quality_constraint_all_off_is_the_tangle_run(oracle_lib, limits):
    """through each of the three serial entries, every limit at its off value"""
    ref = _reference(oracle_lib, "C", "com", False, 2)
    e = _case_engine("C")
    e.set_quality_constraint(passes=2, **{**OFF, **limits})
    for k in range(br.ITERS["C"]):
        assert e.iterate(1, 0.0)[0] == 1
        rec = e.quality_constraint_records()
        assert _records(rec) == [ref["recs"][k]]
        assert rec[0].nTangledCells == rec[0].nBadCells and all(getattr(rec[0], f) == 0 for f in FIELDS_ALL if f not in FIELDS and f != "nTangledCells")
        assert np.array_equal(e.get_points(), ref["pts"][k]) and np.array_equal(_normals(e), ref["normals"][k])


# ---- 3. a constraint that never fires; the switch alone ----------------------------------------------------------------
def _quiet_inputs():
    import bnd_cases
    from smoothmesh_amd.meshgen import hex_block
    return (hex_block(6, jitter=0.2, seed=3),) + bnd_cases.boundary_inputs(6, 3)


@pytest.mark.parametrize("which", ["tangle", "quality"])
def test_constraint_that_never_fires_leaves_the_run_untouched(which):
    runs = []
    for on in (False, True):
        e = _engine(_quiet_inputs(), "com", True, revert=on)
        if on and which == "tangle":
            e.set_tangle_constraint()
        elif on:
            e.set_quality_constraint()
        n, res, frz = e.iterate(10, 0.0)
        assert n == 10
        if on:
            recs = e.tangle_records() if which == "tangle" else e.quality_constraint_records()
            assert _records(recs) == [dict(iteration=k, passes=0, fullRevert=0, nBadCells=0, nPointsReverted=0) for k in range(1, 11)]
        runs.append((res, frz, e.get_points(), _normals(e), e.near_ties(), e.last_near_ties))
    a, b = runs
    assert all(np.array_equal(a[k], b[k]) for k in range(4)) and a[4] == b[4] and np.array_equal(a[5], b[5])


def test_switch_alone_launches_what_a_fresh_engine_launches():
    out = []
    for on in (False, True):
        e = _engine(_quiet_inputs(), "com", True, revert=on)
        assert e.boundary_revert() == on
        e.reset_counters()
        n, res, frz = e.iterate(6, 0.0)
        assert n == 6
        out.append((res, frz, e.get_points(), _normals(e), {c["name"]: c["launches"] for c in e.counters()}))
    a, b = out
    assert all(np.array_equal(a[k], b[k]) for k in range(4)) and a[4] == b[4]


# ---- 4. layers + boundary point smoothing + the tangle constraint ------------------------------------------------------
@pytest.mark.parametrize("variant", ["com", "org"])
def test_layers_with_boundary_smoothing_equal_reference(oracle_lib, variant):
    ref = _reference(oracle_lib, "A", variant, False, 2, None, ("zmin",))
    assert any(r["nBadCells"] > 0 for r in ref["recs"])
    e = _case_engine("A", variant, False, layerPatches=("zmin",))
    e.set_tangle_constraint(2)
    _hold_to_reference(e, ref, e.tangle_records, FIELDS)


# ---- 5. the guard ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [True, False])
def test_guard_restores_points_and_normals(oracle_lib, refine):
    free = br.unconstrained_run(oracle_lib, "A", br.ITERS["A"])
    bad = br.bad_counts(oracle_lib, "A", free)
    lastGood = max(k + 1 for k in range(len(bad)) if not any(bad[:k + 1]))          # = 2
    assert lastGood == 2
    e = _case_engine("A")
    e.set_quality_trace(2)
    e.set_quality_guard(refine=refine)
    n = e.iterate(10, 0.0)[0]
    g = e.quality_guard()
    assert g.tripped and g.trippedIteration == n == 4 and not g.armed
    assert g.restoredIteration == lastGood
    fresh = _case_engine("A", revert=False)
    assert fresh.iterate(lastGood, 0.0)[0] == lastGood
    assert np.array_equal(fresh.get_points(), free[lastGood - 1])
    assert np.array_equal(e.get_points(), fresh.get_points()) and np.array_equal(_normals(e), _normals(fresh))
    # the normals were carried: those the tripped call left behind are others
    for _ in range(3):
        assert e.iterate(1, 0.0)[0] == 1 and fresh.iterate(1, 0.0)[0] == 1
        assert np.array_equal(e.get_points(), fresh.get_points()) and np.array_equal(_normals(e), _normals(fresh))


def test_guard_restore_on_request_carries_the_normals():
    e = _case_engine("C")
    e.set_quality_trace(2)
    e.set_quality_guard()
    assert e.iterate(2, 0.0)[0] == 2
    pts, nrm = e.get_points(), _normals(e)
    assert e.iterate(1, 0.0)[0] == 1
    assert not np.array_equal(_normals(e), nrm)
    e.quality_guard_restore()
    assert e.quality_guard().restoredIteration == 2
    assert np.array_equal(e.get_points(), pts) and np.array_equal(_normals(e), nrm)


def test_guard_does_not_trip_behind_the_constraint():
    e = _case_engine("A")
    e.set_tangle_constraint()
    e.set_quality_trace(1)
    e.set_quality_guard()
    assert e.iterate(10, 0.0)[0] == 10
    g = e.quality_guard()
    assert g.armed and not g.tripped and g.snapshotIteration == 10
    assert any(r.nBadCells > 0 for r in e.tangle_records())


# ---- 6. refusals -------------------------------------------------------------------------------------------------------
def test_refusals():
    from smoothmesh_amd import SmgpuError
    e = _case_engine("A", revert=False)
    assert not e.boundary_revert()
    # the switch off: every refusal as it was
    with pytest.raises(SmgpuError, match="smgpu_set_tangle_constraint: not available on an engine with boundary point smoothing \\(it rewrites the proposals of the "
                                         "boundary points from state that a reverted iteration would leave ahead of the points\\)"):
        e.set_tangle_constraint()
    for kw, api in ((dict(), "smgpu_set_quality_constraint"), (dict(minTwist=0.5), "smgpu_set_quality_constraint_limits"),
                    (dict(minVol=1e-9), "smgpu_set_quality_constraint_limits_all")):
        with pytest.raises(SmgpuError, match=api + ": not available on an engine with boundary point smoothing \\(it rewrites the proposals of the boundary "
                                             "points from state that a reverted iteration would leave ahead of the points\\)"):
            e.set_quality_constraint(**kw)
    with pytest.raises(SmgpuError, match="smgpu_set_quality_constraint_scaling: not available on an engine with boundary point smoothing \\(nor is the quality constraint\\)"):
        e.set_quality_constraint_scaling(2)
    e.set_quality_trace(2)
    with pytest.raises(SmgpuError, match="smgpu_set_quality_guard: not available on an engine with boundary point smoothing \\(its point normals are a running blend "
                                         "across the iterations and its corner lists are host state, neither of which the guard's snapshot holds\\)"):
        e.set_quality_guard()
    # on, then off again with nothing armed: as before
    e.set_boundary_revert()
    e.set_boundary_revert(False)
    with pytest.raises(SmgpuError, match="boundary point smoothing"):
        e.set_tangle_constraint()
    # the switch on: scaling stays refused, through the setter and through scalePasses of the enabling call
    e.set_boundary_revert()
    e.set_quality_constraint()
    new = "scaling passes with boundary point smoothing are not available \\(a scaled boundary point leaves the target surface\\)"
    with pytest.raises(SmgpuError, match="smgpu_set_quality_constraint_scaling: not available on an engine with boundary point smoothing: " + new):
        e.set_quality_constraint_scaling(2)
    assert e.quality_constraint_state().on
    with pytest.raises(SmgpuError, match=new):
        e.set_quality_constraint(scalePasses=2)
    assert not e.quality_constraint_state().on
    # switching it off while armed
    e.set_quality_constraint()
    with pytest.raises(SmgpuError, match="smgpu_set_boundary_revert: the quality constraint is on"):
        e.set_boundary_revert(False)
    e.clear_quality_constraint()
    e.set_tangle_constraint()
    with pytest.raises(SmgpuError, match="smgpu_set_boundary_revert: the tangle constraint is on"):
        e.set_boundary_revert(False)
    e.clear_tangle_constraint()
    e.set_quality_guard()
    with pytest.raises(SmgpuError, match="smgpu_set_boundary_revert: the quality guard is armed"):
        e.set_boundary_revert(False)
    e.set_quality_guard(None)
    e.set_boundary_revert(False)
    assert not e.boundary_revert()


def test_boundary_smoothing_stays_refused_while_a_constraint_is_on():
    from smoothmesh_amd import BoundaryParams, SmgpuError, SmoothEngine, default_params
    mesh, init, target, surf = br.case("A")
    e = SmoothEngine(mesh)
    prm = default_params(e.mesh_stats()[0])
    e.set_params(prm)
    e.set_boundary_revert()                                        # callable before set_boundary_smoothing
    bp = BoundaryParams(initEdges=init, targetSurfaces=surf, targetEdges=target, smoothingPatches=('".*"',))
    e.set_tangle_constraint()
    with pytest.raises(SmgpuError, match="smgpu_set_boundary_smoothing: the tangle constraint is on"):
        e.set_boundary_smoothing(bp, prm.minEdgeLength)
    e.clear_tangle_constraint()
    e.set_quality_constraint()
    with pytest.raises(SmgpuError, match="smgpu_set_boundary_smoothing: the quality constraint is on"):
        e.set_boundary_smoothing(bp, prm.minEdgeLength)
    e.clear_quality_constraint()
    e.set_quality_trace(2)
    e.set_quality_guard()
    with pytest.raises(SmgpuError, match="smgpu_set_boundary_smoothing: the quality guard is armed"):
        e.set_boundary_smoothing(bp, prm.minEdgeLength)
    e.set_quality_guard(None)
    assert e.set_boundary_smoothing(bp, prm.minEdgeLength)["enabled"]
    e.set_tangle_constraint()                                      # the switch was set in front of the set-up
    assert e.tangle_state().on


def test_halo_engine_is_refused():
    import socket
    import torch.distributed as dist
    from smoothmesh_amd import SmgpuError
    from smoothmesh_amd.halo import DistributedSmoother
    from smoothmesh_amd.meshgen import hex_subdomain
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        ds = DistributedSmoother(hex_subdomain((8, 7, 6), (1, 1, 1), 0, jitter=0.3, seed=5), device=0)
        with pytest.raises(SmgpuError, match="smgpu_set_boundary_revert: not available on an engine with a halo"):
            ds.engine.set_boundary_revert()
        assert not ds.engine.boundary_revert()
    finally:
        dist.destroy_process_group()


# ---- 7. front-end ------------------------------------------------------------------------------------------------------
def _write_case_a(path):
    from smoothmesh_amd.polymesh import write_case
    from smoothmesh_amd.surfgen import write_obj_edges, write_obj_surface
    mesh, init, target, surf = br.case("A")
    assert target is None
    write_case(str(path), mesh, binary=True, writeFormat="binary")
    geo = path / "constant" / "geometry"
    os.makedirs(geo)
    write_obj_edges(str(geo / "initEdges.obj"), *init)
    write_obj_surface(str(geo / "targetSurfaces.obj"), *surf)


def _run(case, opts):
    return subprocess.run([BIN, "-case", str(case)] + opts, capture_output=True, text=True, timeout=300)


PLAIN = ["-centroidalIters", "10", "-relTol", "0", "-faceAngleConstraint", "false", "-edgeAngleConstraint", "false", "-maxStepLength", "1",
         "-minEdgeLength", "1e-4"]


def test_front_end(oracle_lib, tmp_path):
    from smoothmesh_amd.engine import TangleRecord
    from smoothmesh_amd.polymesh import read_polymesh
    from smoothmesh_amd.quality import format_tangle_line
    from smoothmesh_amd.surfgen import read_obj_edges, read_obj_surface
    ref = _reference(oracle_lib, "A", "com", False, 2)
    for d in "abc":
        _write_case_a(tmp_path / d)
    # what the front-end reads is what the reference was given
    mesh, init, _, surf = br.case("A")
    geo = tmp_path / "a" / "constant" / "geometry"
    ri, rs = read_obj_edges(str(geo / "initEdges.obj")), read_obj_surface(str(geo / "targetSurfaces.obj"))
    assert np.array_equal(ri[0], init[0]) and np.array_equal(ri[1], init[1]) and np.array_equal(rs[0], surf[0]) and np.array_equal(rs[1], surf[1])
    r = _run(tmp_path / "a", PLAIN + ["-tangleConstraint", "true", "-boundaryRevert", "true"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert "Enabled boundary point smoothing" in r.stdout
    assert lines.count("Boundary revert: on") == 1 and lines.count("Tangle constraint: 0 exempt cells, 2 passes") == 1
    assert lines.index("Boundary revert: on") < lines.index("Tangle constraint: 0 exempt cells, 2 passes") < next(i for i, x in enumerate(lines) if x.startswith("Smoothing iteration="))
    want = []
    for c in ref["recs"]:
        want.append(f"Smoothing iteration={c['iteration']} ")
        if c["nBadCells"] > 0:
            want.append(format_tangle_line(TangleRecord(**c)).rstrip("\n"))
    got = [x for x in lines if x.startswith(("Smoothing iteration=", "    tangle "))]
    assert len(got) == len(want) and all(g == w or (w.endswith(" ") and g.startswith(w)) for g, w in zip(got, want)), got
    assert sum(x.startswith("    tangle ") for x in got) == 8
    pts = read_polymesh(str(tmp_path / "a" / "constant" / "polyMesh"), str(tmp_path / "a" / "10" / "polyMesh")).points
    assert np.array_equal(np.asarray(pts), ref["pts"][-1])
    # the same command without the option dies with today's message, and writes nothing
    r = _run(tmp_path / "b", PLAIN + ["-tangleConstraint", "true"])
    assert r.returncode != 0
    assert ("-tangleConstraint is not available with boundary point smoothing: it rewrites the boundary points from state that a reverted "
            "iteration would leave ahead of the points (run without -smoothingPatches, or without the constraint)") in r.stdout + r.stderr
    assert not any(x.isdigit() and x != "0" for x in os.listdir(tmp_path / "b"))
    # the option alone
    r = _run(tmp_path / "b", PLAIN + ["-boundaryRevert", "true"])
    assert r.returncode != 0 and "-boundaryRevert needs -tangleConstraint true, -qualityConstraint true or -qualityGuard true" in r.stdout + r.stderr
    # the quality constraint and the guard run on the same case
    r = _run(tmp_path / "c", PLAIN + ["-qualityConstraint", "true", "-maxNonOrtho", "180", "-maxInternalSkewness", "0", "-maxBoundarySkewness", "0",
                                       "-checkQuality", "true", "-qualityInterval", "1", "-qualityGuard", "true", "-boundaryRevert", "true"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Boundary revert: on" in r.stdout.splitlines() and "Quality guard" not in r.stdout
    pts = read_polymesh(str(tmp_path / "c" / "constant" / "polyMesh"), str(tmp_path / "c" / "10" / "polyMesh")).points
    assert np.array_equal(np.asarray(pts), ref["pts"][-1])
