"""The tangle constraint (include/smgpu.h smgpu_set_tangle_constraint / smgpu_get_tangle_records / smgpu_get_tangle_state,
csrc/kernels_quality_tangle.hpp, DESIGN.md "Mesh quality" 10.12) against its CPU restatement (tests/tangle_reference.py, pinned by
tests/test_tangle_reference.py): the accepted points of every iteration and every record field, bit for bit; the invariant
through the existing report; a constraint that never fires leaves the run untouched; exemption; numbering across calls; the
trace and the guard behind it; refusals; and the lines of `smoothMesh -tangleConstraint`."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tangle_reference import FIELDS, MARGIN, reference_run
from test_gpu_quality_guard import dented_block_tiles
from test_gpu_quality_trace import _engine, dented_block
from test_quality_reference import tangled_block

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "smoothmesh_amd", "bin", "smoothMesh")


def dented_cavity(xy, newz):
    """cavity_mesh(8) without jitter (3034 points, 2192 cells: a few tiles, polyhedral cells at the refinement interface) with the
    lowest points of the column x, y = xy lifted to z = newz: a valid mesh that unconstrained smoothing tangles (found on the CPU
    with tests/tangle_reference.py -- "interface": at the coarse / fine interface above z = 0.125, 4 bad cells at iteration 10 with
    a step of 0.05; "band": in the refined band under the cavity, 4 bad cells from iteration 4 on)"""
    from smoothmesh_amd.polymesh import cavity_mesh
    m = cavity_mesh(8, jitter=0.0, seed=3)
    assert m.nPoints == 3034 and m.nCells == 2192
    m.points = m.points.copy()
    col = np.where((np.abs(m.points[:, 0] - xy[0]) < 1e-9) & (np.abs(m.points[:, 1] - xy[1]) < 1e-9))[0]
    col = col[np.argsort(m.points[col, 2])]
    for p, z in zip(col, newz):
        m.points[p, 2] = z
    return m


# name -> (mesh, parameters that make it tangle, iterations)
CASES = {
    "dented": (dented_block, dict(maxStepLength=1.0, minEdgeLength=1e-4), 8),                      # one tile, the six-face path
    "dented_tiles": (dented_block_tiles, dict(maxStepLength=0.03, minEdgeLength=1e-4), 12),        # several tiles; first revert at 8
    "cavity_band": (lambda: dented_cavity((0.5, 0.5), (0.1875, 0.2, 0.2125, 0.225)), dict(maxStepLength=0.05, minEdgeLength=1e-4), 8),
    "cavity_interface": (lambda: dented_cavity((0.125, 0.125), (0.27, 0.28, 0.29)), dict(maxStepLength=0.05, minEdgeLength=1e-4), 10),
}
# (variant, constraints, passes, SMGPU_GEOM_T): both variants and the reference's constraints off / on at the defaults; fewer
# passes and the other tile shapes on the unconstrained .com run
SETTINGS = [("com", False, 2, 128), ("com", True, 2, 128), ("org", False, 2, 128), ("org", True, 2, 128),
            ("com", False, 0, 128), ("com", False, 1, 128), ("com", False, 2, 64), ("com", False, 2, 256)]


@functools.lru_cache(maxsize=None)
def _mesh(name):
    return CASES[name][0]()


@functools.lru_cache(maxsize=None)
def _reference(oracle_lib, name, variant, constraints, passes):
    """computed once per configuration and shared: the accepted points and the records of the CPU restatement"""
    _, over, n = CASES[name]
    r = reference_run(oracle_lib, _mesh(name), n, passes=passes, variant=variant, constraints=constraints, **over)
    assert r["ref"].minMargin > MARGIN
    return r


def _records(recs):
    return [{k: getattr(r, k) for k in FIELDS} for r in recs]


def _tangle_engine(name, variant="com", constraints=False, passes=2, **more):
    e = _engine(_mesh(name), variant, constraints, **{**CASES[name][1], **more})
    e.set_tangle_constraint(passes)
    return e


# ---- 1. engine = reference, by bits ------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,constraints,passes,geomT", SETTINGS)
@pytest.mark.parametrize("name", list(CASES))
def test_engine_equals_reference_bitwise(oracle_lib, monkeypatch, name, variant, constraints, passes, geomT):
    monkeypatch.setenv("SMGPU_GEOM_T", str(geomT))
    n = CASES[name][2]
    ref = _reference(oracle_lib, name, variant, constraints, passes)
    e = _tangle_engine(name, variant, constraints, passes)
    st = e.tangle_state()
    assert st.on and st.passes == passes and st.nExemptCells == ref["ref"].nExemptCells and st.iteration == 0
    for k in range(n):
        assert e.iterate(1, 0.0)[0] == 1
        rec = _records(e.tangle_records())
        assert rec == [ref["recs"][k]], (k, rec, ref["recs"][k])
        assert np.array_equal(e.get_points(), ref["pts"][k]), k
    assert e.tangle_state().iteration == n
    if (variant, constraints) == ("com", False):
        assert any(r["nBadCells"] > 0 for r in ref["recs"]), "the mesh does not tangle: the case tests nothing"


@pytest.mark.parametrize("passes", [1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_without_tiles_equals_tiled(monkeypatch, name, passes):
    n = CASES[name][2]

    def run(env):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            e = _tangle_engine(name, passes=passes)
        assert e.iterate(n, 0.0)[0] == n
        return e.get_points(), e.tangle_records(), e.tangle_state()

    tiled, direct = run({}), run({"SMGPU_TILES": "0"})
    assert np.array_equal(tiled[0], direct[0]) and tiled[1] == direct[1] and tiled[2] == direct[2]
    assert any(r.nBadCells > 0 for r in tiled[1])


# ---- 2. the invariant, through the existing report ---------------------------------------------------------------------
@pytest.mark.parametrize("constraints", [False, True])
@pytest.mark.parametrize("name", list(CASES) + ["tangled"])
def test_invariant_through_the_report(oracle_lib, name, constraints):
    from tangle_reference import TangleReference, make_oracle
    if name == "tangled":
        m, over, n = tangled_block(), dict(maxStepLength=0.01), 8
    else:
        m, (_, over, n) = _mesh(name), CASES[name]
    # the exempt cells, from the CPU restatement (the engine reports their number only)
    ref = TangleReference(make_oracle(oracle_lib, m, "com", constraints, **over), m)
    exempt = ref.exempt
    assert exempt.any() == (name == "tangled")
    e = _engine(m, "com", constraints, **over)
    q0 = e.mesh_quality()
    e.set_tangle_constraint()
    assert e.tangle_state().nExemptCells == int(exempt.sum())
    own, nei = m.owner.astype(np.int64), m.neighbour.astype(np.int64)
    for _ in range(n):
        assert e.iterate(1, 0.0)[0] == 1
        q = e.mesh_quality()
        assert q.nNonPositiveVolume <= q0.nNonPositiveVolume and q.nWrongOrientedFaces <= q0.nWrongOrientedFaces
        sets = e.quality_sets()
        assert exempt[sets["zeroVolumeCells"]].all()
        # a face is wrongly oriented exactly when its owner or its neighbour is bad through it: that cell is an exempt one (on a
        # mesh without exempt cells the set is empty)
        for f in sets["wrongOrientedFaces"].tolist():
            assert exempt[own[f]] or (f < m.nInternalFaces and exempt[nei[f]]), f
        # ... and the cell that is bad through it is the exempt one: no other cell is bad at the accepted points, by the contract's
        # own measure on the oracle's geometry of them
        assert not (ref.bad_cells(e.get_points(), judge=False) & ~exempt).any()


# ---- 3. a constraint that never fires leaves the run untouched ---------------------------------------------------------
@pytest.mark.parametrize("mesh", ["hex12", "hex12_layers", "cavity"])
def test_constraint_that_never_fires_leaves_the_run_untouched(mesh):
    from smoothmesh_amd import LayerParams, default_params
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import cavity_mesh
    m = cavity_mesh(16, jitter=0.2, seed=3) if mesh == "cavity" else hex_block(12, 9, 7, jitter=0.3)
    runs = []
    for on in (False, True):
        e = _engine(m)
        if mesh == "hex12_layers":
            prm = default_params(e.mesh_stats()[0])
            assert e.set_layers(LayerParams(layerPatches=("xmin",), layerExpansionRatio=1.2), prm.minEdgeLength)
        if on:
            e.set_tangle_constraint()
            assert e.tangle_state().nExemptCells == 0
        n, res, frz = e.iterate(10, 0.0)
        assert n == 10
        if on:
            recs = e.tangle_records()
            assert _records(recs) == [dict(iteration=k, passes=0, fullRevert=0, nBadCells=0, nPointsReverted=0) for k in range(1, 11)]
        runs.append((res, frz, e.get_points(), e.near_ties(), e.last_near_ties, e.debug_walk_mode()))
    a, b = runs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[3] == b[3] and np.array_equal(a[4], b[4]) and a[5] == b[5]


# ---- 4. exemption ------------------------------------------------------------------------------------------------------
def test_cells_bad_at_enabling_are_exempt():
    m = tangled_block()
    a, b = _engine(m, constraints=False, maxStepLength=0.01), _engine(m, constraints=False, maxStepLength=0.01)
    a.set_tangle_constraint()
    assert a.tangle_state().nExemptCells == 4
    assert a.iterate(6, 0.0)[0] == 6 and b.iterate(6, 0.0)[0] == 6
    assert _records(a.tangle_records()) == [dict(iteration=k, passes=0, fullRevert=0, nBadCells=0, nPointsReverted=0) for k in range(1, 7)]
    assert np.array_equal(a.get_points(), b.get_points())


# ---- 5. numbering and records across calls -----------------------------------------------------------------------------
def test_numbering_and_records_across_calls(oracle_lib):
    import ctypes as C
    from smoothmesh_amd import SmgpuError, _ffi
    ref = _reference(oracle_lib, "dented", "com", False, 2)
    e = _tangle_engine("dented")
    assert e.iterate(3, 0.0)[0] == 3 and e.iterate(5, 0.0)[0] == 5
    n = C.c_int64(0)
    assert e._lib.smgpu_get_tangle_records(e._h, None, 0, C.byref(n)) == 0 and n.value == 8
    buf = (_ffi.TangleRecord * 8)()
    assert e._lib.smgpu_get_tangle_records(e._h, buf, 7, C.byref(n)) != 0          # a short cap is an error ...
    with pytest.raises(SmgpuError, match="cap 7 is below the 8 pending records"):
        e._check(1)
    assert _records(e.tangle_records()) == ref["recs"]                             # ... that clears nothing
    assert e.tangle_records() == []                                                 # a read clears
    assert e.tangle_state().iteration == 8
    assert np.array_equal(e.get_points(), ref["pts"][7])
    # switching it on again restarts the numbering and takes the exempt cells anew
    e.set_tangle_constraint(1)
    assert e.tangle_state().iteration == 0 and e.tangle_state().passes == 1
    assert e.iterate(2, 0.0)[0] == 2
    assert [r.iteration for r in e.tangle_records()] == [1, 2]


def test_stop_by_reltol_leaves_exactly_done_records():
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(12, 9, 7, jitter=0.3)
    r = _engine(m).iterate(24, 0.0)[1]
    ms = [k for k in range(1, len(r)) if r[k] < r[:k].min()]
    assert ms, r
    relTol = 0.5 * (r[ms[0]] + r[:ms[0]].min())
    a, b = _engine(m), _engine(m)
    a.set_tangle_constraint()
    na, resa, _ = a.iterate(ms[0] + 20, relTol)
    nb, resb, _ = b.iterate(ms[0] + 20, relTol)
    assert na == nb == ms[0] + 1 and np.array_equal(resa, resb)
    assert [x.iteration for x in a.tangle_records()] == list(range(1, na + 1))
    assert a.tangle_state().iteration == na
    assert np.array_equal(a.get_points(), b.get_points())


# ---- 6. with the trace and the guard -----------------------------------------------------------------------------------
def test_trace_sees_the_accepted_points(oracle_lib):
    from test_gpu_quality_trace import _assert_record_is_report
    ref = _reference(oracle_lib, "dented_tiles", "com", False, 2)
    n = CASES["dented_tiles"][2]
    e = _tangle_engine("dented_tiles")
    e.set_quality_trace(1)
    assert e.iterate(n, 0.0)[0] == n
    recs = e.quality_trace()
    assert len(recs) == n
    twin = _engine(_mesh("dented_tiles"), "com", False, **CASES["dented_tiles"][1])
    for k, rec in enumerate(recs, start=1):
        twin.set_points(ref["pts"][k - 1])
        _assert_record_is_report(rec, twin.mesh_quality(), k)
        assert rec.nNonPositiveVolume == 0 and rec.nWrongOrientedFaces == 0
    assert _records(e.tangle_records()) == ref["recs"]


def test_guard_does_not_trip_behind_the_constraint():
    over = dict(maxStepLength=0.03, minEdgeLength=1e-4)
    trips = {}
    for on in (True, False):
        e = _engine(dented_block(), "com", False, **over)
        if on:
            e.set_tangle_constraint()
        e.set_quality_trace(1)
        e.set_quality_guard()
        n = e.iterate(14, 0.0)[0]
        g = e.quality_guard()
        trips[on] = g.tripped
        if on:
            assert n == 14 and g.armed and not g.tripped and g.snapshotIteration == 14
            assert any(r.nBadCells > 0 for r in e.tangle_records())
    assert trips == {True: False, False: True}


def test_running_number_goes_back_with_the_guards_rollback():
    from smoothmesh_amd.meshgen import hex_block
    e = _engine(hex_block(12, 9, 7, jitter=0.3))
    e.set_quality_trace(3)
    e.set_quality_guard()
    assert e.iterate(2, 0.0)[0] == 2
    e.set_tangle_constraint()                                  # enabled later than the trace: its number runs 2 behind
    assert e.iterate(7, 0.0)[0] == 7
    assert e.tangle_state().iteration == 7 and e.quality_guard().snapshotIteration == 9
    assert e.iterate(1, 0.0)[0] == 1
    e.quality_guard_restore()                                  # back to the points of trace iteration 9 = tangle iteration 7
    assert e.quality_guard().restoredIteration == 9 and e.tangle_state().iteration == 7
    assert [r.iteration for r in e.tangle_records()] == list(range(1, 9))   # the records of what ran stand, like the trace's
    assert e.iterate(2, 0.0)[0] == 2
    assert [r.iteration for r in e.tangle_records()] == [8, 9] and [r.iteration for r in e.quality_trace()] == [3, 6, 9]


# ---- 7. refusals and the off state -------------------------------------------------------------------------------------
def test_refusals_and_the_off_state():
    from smoothmesh_amd import SmgpuError
    from smoothmesh_amd.meshgen import hex_block
    from test_gpu_quality_guard import _set_boundary_smoothing
    m = hex_block(6, 5, 4, jitter=0.3)
    e = _engine(m)
    st = e.tangle_state()
    assert not st.on and st.nExemptCells == 0 and st.iteration == 0
    assert e.tangle_records() == []
    with pytest.raises(SmgpuError, match="passes < 0"):
        e.set_tangle_constraint(-1)
    assert not e.tangle_state().on
    e.set_tangle_constraint(3)
    assert e.tangle_state().on and e.tangle_state().passes == 3
    empty = np.zeros(0, np.int32)
    with pytest.raises(SmgpuError, match="tangle constraint"):
        e.halo_configure(empty, empty, 0, np.zeros(1, np.int32), empty, 0, 0, 0, 0, 0)
    with pytest.raises(SmgpuError, match="tangle constraint"):
        _set_boundary_smoothing(e)
    assert e.iterate(3, 0.0)[0] == 3
    e.clear_tangle_constraint()
    assert not e.tangle_state().on and e.tangle_records() == []
    # after switching it off: launch for launch and bit for bit a fresh engine's iterations from the same points
    fresh = _engine(m)
    fresh.set_points(e.get_points())
    for x in (e, fresh):
        x.reset_counters()
    ra, rb = e.iterate(4, 0.0), fresh.iterate(4, 0.0)
    assert ra[0] == rb[0] == 4 and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
    assert np.array_equal(e.get_points(), fresh.get_points())
    assert {c["name"]: c["launches"] for c in e.counters()} == {c["name"]: c["launches"] for c in fresh.counters()}
    assert e.tangle_records() == []
    # an engine with boundary point smoothing is refused
    e = _engine(hex_block(6, jitter=0.0))
    _set_boundary_smoothing(e)
    with pytest.raises(SmgpuError, match="boundary point smoothing"):
        e.set_tangle_constraint()


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
        with pytest.raises(SmgpuError, match="not available on an engine with a halo"):
            ds.engine.set_tangle_constraint()
    finally:
        dist.destroy_process_group()


# ---- 8. front-end ------------------------------------------------------------------------------------------------------
def _run(case, opts):
    r = subprocess.run([BIN, "-case", str(case)] + opts, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _strip(out):
    return [x for x in out.splitlines() if not x.startswith(("Case: ", "ClockTime"))]


def test_front_end(tmp_path):
    from smoothmesh_amd.polymesh import read_polymesh, write_case
    from smoothmesh_amd.quality import format_tangle_line
    m = _mesh("dented")
    for d in "abc":
        write_case(str(tmp_path / d), m, binary=True, writeFormat="binary")
    plain = ["-centroidalIters", "8", "-relTol", "0", "-edgeAngleConstraint", "false", "-faceAngleConstraint", "false",
             "-maxStepLength", "1", "-minEdgeLength", "1e-4", "-writeInterval", "3"]
    e = _tangle_engine("dented")
    assert e.iterate(8, 0.0)[0] == 8
    recs = e.tangle_records()
    assert sum(r.nBadCells > 0 for r in recs) >= 2 and any(r.nBadCells == 0 for r in recs)
    out = _run(tmp_path / "a", plain + ["-tangleConstraint", "true"])
    lines = out.splitlines()
    assert lines.count("Tangle constraint: 0 exempt cells, 2 passes") == 1
    assert lines.index("Tangle constraint: 0 exempt cells, 2 passes") < next(i for i, x in enumerate(lines) if x.startswith("Smoothing iteration="))
    # under the iteration line of every iteration with bad cells, and nowhere else, across the chunks of -writeInterval
    want = []
    for r in recs:
        want.append(f"Smoothing iteration={r.iteration} ")
        if r.nBadCells > 0:
            want.append(format_tangle_line(r).rstrip("\n"))
    got = [x for x in lines if x.startswith(("Smoothing iteration=", "    tangle "))]
    assert len(got) == len(want) and all(g == w or (w.endswith(" ") and g.startswith(w)) for g, w in zip(got, want)), got
    pts = read_polymesh(str(tmp_path / "a" / "constant" / "polyMesh"), str(tmp_path / "a" / "8" / "polyMesh")).points
    assert np.array_equal(np.asarray(pts), e.get_points())
    # -tanglePasses
    out = _run(tmp_path / "b", plain + ["-tangleConstraint", "true", "-tanglePasses", "0"])
    assert "Tangle constraint: 0 exempt cells, 0 passes" in out.splitlines()
    assert sum(x.startswith("    tangle ") and x.endswith(" fullRevert") for x in out.splitlines()) == 8
    # without the option: no line of it
    off = _strip(_run(tmp_path / "c", plain))
    assert not any("Tangle constraint" in x or x.startswith("    tangle ") for x in off)


def test_front_end_where_it_never_fires_is_the_output_without_it(tmp_path):
    """a run in which no cell turns bad prints, less the set-up line, exactly what the run without the option prints: every
    iteration line with its frozen count and residual, the reports, everything else"""
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import write_case
    m = hex_block(9, 8, 7, jitter=0.3, seed=4)
    for d in "ab":
        write_case(str(tmp_path / d), m, binary=True, writeFormat="binary")
    opts = ["-centroidalIters", "6", "-relTol", "0", "-checkQuality", "true", "-qualityInterval", "2", "-writeInterval", "4"]
    off = _strip(_run(tmp_path / "a", opts))
    on = _strip(_run(tmp_path / "b", opts + ["-tangleConstraint", "true"]))
    assert on.count("Tangle constraint: 0 exempt cells, 2 passes") == 1
    assert not any(x.startswith("    tangle ") for x in on)
    on.remove("Tangle constraint: 0 exempt cells, 2 passes")
    assert on == off
    assert sum(x.startswith("Smoothing iteration=") for x in off) == 6
