"""The scaling passes of the quality constraint (include/smgpu.h smgpu_set_quality_constraint_scaling / _records_scaled /
_state_scaled, csrc/kernels_quality_scale.hpp, DESIGN.md "Mesh quality" 10.19) against their CPU restatement
(tests/quality_constraint_scaled_reference.py, pinned by tests/test_quality_constraint_scaled_reference.py): the accepted points
of every iteration and every record field, bit for bit; without tiles; scalePasses = 0 is the constraint as it was; a constraint
that never fires; r = 0, n = 0; the invariant through the engine's own report; the trace and the guard behind it; records across
calls; switching; refusals; and the lines of `smoothMesh -scalePasses`.

The meshes are the smallest on which the kernels can still go wrong: dented_block() (125 points: less than one workgroup,
nPoints % 4 = 1, the tail of the last mark word; one tile, the six-face path), dented_block_tiles() (several tiles) and the two
dented cavities (3034 points: ragged pointPoints rows, a partial last workgroup, the general ELL path)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import tangle_reference
from quality_constraint_all_reference import FIELDS_ALL
from quality_constraint_reference import FACE_MARGIN, OFF
from quality_constraint_scaled_reference import FIELDS_SCALED, reference_run
from test_gpu_quality_constraint import LIMITS
from test_gpu_quality_trace import _engine
from test_gpu_tangle import CASES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "smoothmesh_amd", "bin", "smoothMesh")

# case -> (mesh of CASES, the limits): three of tests/test_gpu_quality_constraint.py's LIMITS, and cavity_band with all criteria off
QC = {"tiles_both": LIMITS["tiles_both"], "cavity": LIMITS["cavity"], "dented": LIMITS["dented"], "cavity_band": ("cavity_band", {})}
# (scalePasses, errorReduction, nSmoothScale, passes)
SCALINGS = [(2, 0.5, 1, 2), (2, 0.75, 4, 2), (1, 0.75, 0, 0), (3, 0.5, 2, 1)]
VARIANTS = [("com", False), ("com", True), ("org", False), ("org", True)]
# every case under every scaling, both foam variants, the reference's constraints off and on; the other tile shapes on one case each
RUNS = [(c, v, k, s, 128) for c in QC for (v, k) in VARIANTS for s in SCALINGS] + \
       [("tiles_both", "com", False, SCALINGS[0], 64), ("cavity", "com", False, SCALINGS[1], 256), ("dented", "com", False, SCALINGS[3], 64)]


@functools.lru_cache(maxsize=None)
def _mesh(name):
    return CASES[name][0]()


def _limits(case):
    return {**OFF, **QC[case][1]}


def _scaling(s):
    return dict(scalePasses=s[0], errorReduction=s[1], nSmoothScale=s[2])


@functools.lru_cache(maxsize=None)
def _reference(oracle_lib, case, variant, constraints, s, n=None):
    """computed once per configuration and shared: the accepted points and the records of the CPU restatement (s = None: off)"""
    name = QC[case][0]
    _, over, nCase = CASES[name]
    r = reference_run(oracle_lib, _mesh(name), n or nCase, limits=_limits(case), passes=s[3] if s else 2, variant=variant, constraints=constraints,
                      scaling=_scaling(s) if s else None, **over)
    assert r["ref"].minMargin > tangle_reference.MARGIN and r["ref"].minCosGap > FACE_MARGIN and r["ref"].minSkewGap > FACE_MARGIN
    return r


def _records(recs, fields=FIELDS_SCALED):
    return [{k: getattr(r, k) for k in fields} for r in recs]


def _qc_engine(case, variant="com", constraints=False, s=None, **more):
    name = QC[case][0]
    e = _engine(_mesh(name), variant, constraints, **{**CASES[name][1], **more})
    e.set_quality_constraint(passes=s[3] if s else 2, **_limits(case), **(_scaling(s) if s else {}))
    return e


# ---- 1. engine = reference, by bits ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,variant,constraints,s,geomT", RUNS)
def test_engine_equals_reference_bitwise(oracle_lib, monkeypatch, case, variant, constraints, s, geomT):
    monkeypatch.setenv("SMGPU_GEOM_T", str(geomT))
    n = CASES[QC[case][0]][2]
    ref = _reference(oracle_lib, case, variant, constraints, s)
    e = _qc_engine(case, variant, constraints, s)
    st = e.quality_constraint_state_scaled()
    assert st.on and st.passes == s[3] and (st.scalePasses, st.errorReduction, st.nSmoothScale) == s[:3] and st.iteration == 0
    assert st.nExemptCells == ref["ref"].nExemptCells and st.nExemptFaces == ref["ref"].nExemptFaces
    for k in range(n):
        assert e.iterate(1, 0.0)[0] == 1
        rec = _records(e.quality_constraint_records_scaled())
        assert rec == [ref["recs"][k]], (k, rec, ref["recs"][k])
        assert np.array_equal(e.get_points(), ref["pts"][k]), k
    assert e.quality_constraint_state_scaled().iteration == n
    if (variant, constraints, s) == ("com", False, SCALINGS[0]):
        assert any(r["nPointsScaled"] > 0 for r in ref["recs"]) and any(r["nPointsReverted"] > 0 for r in ref["recs"]), "the case tests nothing"


@pytest.mark.parametrize("case", list(QC))
def test_every_case_scales_and_reverts(oracle_lib, case):
    """a case whose runs never scale a point, or never revert one, tests nothing: over the settings of the bitwise test (which
    holds the engine's records to these) every case does both, and the bitwise test asserts both under the first setting alone"""
    recs = [r for (v, k) in VARIANTS for s in SCALINGS for r in _reference(oracle_lib, case, v, k, s)["recs"]]
    assert any(r["nPointsScaled"] > 0 for r in recs) and any(r["nPointsReverted"] > 0 for r in recs)
    assert any(r["fullRevert"] for r in recs) and any(r["nScalePasses"] < r["passes"] for r in recs)


@pytest.mark.parametrize("case,s", [("tiles_both", SCALINGS[0]), ("cavity", SCALINGS[1]), ("dented", SCALINGS[3]), ("cavity_band", SCALINGS[2])])
def test_without_tiles_equals_tiled(monkeypatch, case, s):
    n = CASES[QC[case][0]][2]

    def run(env):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            e = _qc_engine(case, s=s)
        assert e.iterate(n, 0.0)[0] == n
        return e.get_points(), e.quality_constraint_records_scaled(), e.quality_constraint_state_scaled()

    tiled, direct = run({}), run({"SMGPU_TILES": "0"})
    assert np.array_equal(tiled[0], direct[0]) and tiled[1] == direct[1] and tiled[2] == direct[2]
    assert any(r.nBadCells > 0 for r in tiled[1])


@pytest.mark.parametrize("grid", [1, 3])
def test_several_trips_per_lane_give_the_same_bits(oracle_lib, monkeypatch, grid):
    """the sweep and the apply take a point per lane and trip on a capped grid (8192 workgroups: beyond 2 097 152 points a lane
    makes a second trip); SMGPU_QS_MAX_GRID caps it at 1 and 3 workgroups, so that on 1040 and 3034 points every lane makes
    several trips, the last one partial"""
    monkeypatch.setenv("SMGPU_QS_MAX_GRID", str(grid))
    for case, s in (("tiles_both", SCALINGS[0]), ("cavity", SCALINGS[1])):
        ref = _reference(oracle_lib, case, "com", False, s)
        e = _qc_engine(case, s=s)
        n = CASES[QC[case][0]][2]
        assert e.iterate(n, 0.0)[0] == n
        assert _records(e.quality_constraint_records_scaled()) == ref["recs"] and any(r["nPointsScaled"] > 0 for r in ref["recs"])
        assert np.array_equal(e.get_points(), ref["pts"][-1])


# ---- 2. scalePasses = 0 is the constraint as it was --------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tiles_both", "cavity"])
def test_scale_passes_zero_is_the_constraint_as_it_was(oracle_lib, case):
    """after having been on, and on a fresh engine without the call: points, records (the old getters) and residuals of the
    reference without scaling, which tests/test_gpu_quality_constraint.py holds the parent's run to"""
    n = CASES[QC[case][0]][2]
    ref = _reference(oracle_lib, case, "com", False, None)
    want = [{k: r[k] for k in FIELDS_ALL} for r in ref["recs"]]
    was_on = _qc_engine(case, s=SCALINGS[1])
    was_on.set_quality_constraint_scaling(0)
    assert was_on.quality_constraint_state_scaled().scalePasses == 0
    explicit = _qc_engine(case)
    explicit.set_quality_constraint_scaling(scalePasses=0, errorReduction=0.5, nSmoothScale=1)
    fresh = _qc_engine(case)
    runs = []
    for e in (was_on, explicit, fresh):
        e.reset_counters()
        got, res, frz = e.iterate(n, 0.0)
        assert got == n
        launches = {c["name"]: c["launches"] for c in e.counters()}
        runs.append((e.get_points(), res, frz, _records(e.quality_constraint_records(), FIELDS_ALL), launches))
    for r in runs:
        assert np.array_equal(r[0], ref["pts"][-1]) and r[3] == want
        assert np.array_equal(r[1], runs[2][1]) and np.array_equal(r[2], runs[2][2]) and r[4] == runs[2][4]
        assert np.array_equal(r[2], np.array(ref["frz"]))
    # the scaled getter on a run without scaling: the three fields are 0
    e = _qc_engine(case)
    assert e.iterate(n, 0.0)[0] == n
    recs = e.quality_constraint_records_scaled()
    assert _records(recs, FIELDS_ALL) == want and all((r.nScalePasses, r.nPointsScaled, r.minScale) == (0, 0, 0.0) for r in recs)


# ---- 3. a constraint that never fires ----------------------------------------------------------------------------------
def test_constraint_that_never_fires_leaves_the_run_untouched():
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(6, 5, 4, jitter=0.3)
    runs = []
    for on in (False, True):
        e = _engine(m)
        if on:
            e.set_quality_constraint(scalePasses=2)
            st = e.quality_constraint_state_scaled()
            assert (st.scalePasses, st.errorReduction, st.nSmoothScale) == (2, 0.75, 4) and st.nExemptCells == 0 and st.nExemptFaces == 0
        n, res, frz = e.iterate(10, 0.0)
        assert n == 10
        if on:
            zero = {k: 0 for k in FIELDS_SCALED}
            assert _records(e.quality_constraint_records_scaled()) == [{**zero, "iteration": k, "minScale": 1.0} for k in range(1, 11)]
        runs.append((res, frz, e.get_points()))
    a, b = runs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ---- 4. r = 0, n = 0: the constraint with the passes added -------------------------------------------------------------
@pytest.mark.parametrize("case,S,P", [("tiles_both", 2, 2), ("cavity", 1, 1), ("dented", 3, 0)])
def test_factor_zero_without_sweeps_is_the_constraint_with_the_passes_added(case, S, P):
    n = CASES[QC[case][0]][2]
    a, b = _qc_engine(case, s=(S, 0.0, 0, P)), _qc_engine(case, s=None)
    b.set_quality_constraint(passes=S + P, **_limits(case))
    fired = False
    for k in range(n):
        assert a.iterate(1, 0.0)[0] == 1 and b.iterate(1, 0.0)[0] == 1
        ra, rb = a.quality_constraint_records_scaled(), b.quality_constraint_records()
        assert _records(ra, FIELDS_ALL) == _records(rb, FIELDS_ALL), k
        assert ra[0].nPointsScaled == 0 and ra[0].nScalePasses == min(ra[0].passes, S)
        assert np.array_equal(a.get_points(), b.get_points()), k
        fired = fired or ra[0].passes > 0
    assert fired


# ---- 5. the invariant, through the engine's own report -----------------------------------------------------------------
@pytest.mark.parametrize("case,s", [("tiles_both", SCALINGS[0]), ("cavity", SCALINGS[1])])
def test_invariant_through_the_report(oracle_lib, case, s):
    ref = _reference(oracle_lib, case, "com", False, s)["ref"]
    m, n, lim = _mesh(QC[case][0]), CASES[QC[case][0]][2], _limits(case)
    exemptF, exemptC = ref.exemptFaces, ref.exempt
    e = _qc_engine(case, s=s)
    st = e.quality_constraint_state()
    assert st.nExemptCells == int(exemptC.sum()) and st.nExemptFaces == int(exemptF.sum())
    twin = _engine(m, "com", False, **CASES[QC[case][0]][1])
    q0 = twin.mesh_quality()
    Fi = m.nInternalFaces
    own, nei = m.owner.astype(np.int64), m.neighbour.astype(np.int64)
    scaled = False
    for _ in range(n):
        assert e.iterate(1, 0.0)[0] == 1
        scaled = scaled or e.quality_constraint_records_scaled()[0].nPointsScaled > 0
        si = e.quality_sets(nonOrthThreshold=min(lim["maxNonOrtho"], 180.0), skewThreshold=lim["maxInternalSkewness"])
        sb = e.quality_sets(nonOrthThreshold=min(lim["maxNonOrtho"], 180.0), skewThreshold=lim["maxBoundarySkewness"])
        if lim["maxNonOrtho"] < 180.0:
            assert exemptF[si["nonOrthoFaces"]].all()
        if lim["maxInternalSkewness"] > 0.0:
            f = si["skewFaces"]
            assert exemptF[f[f < Fi]].all()
        if lim["maxBoundarySkewness"] > 0.0:
            f = sb["skewFaces"]
            assert exemptF[f[f >= Fi]].all()
        q = e.mesh_quality()
        assert q.nNonPositiveVolume <= q0.nNonPositiveVolume and q.nWrongOrientedFaces <= q0.nWrongOrientedFaces
        assert exemptC[si["zeroVolumeCells"]].all()
        for f in si["wrongOrientedFaces"].tolist():
            assert exemptC[own[f]] or (f < Fi and exemptC[nei[f]]), f
    assert scaled


# ---- 6. with the trace and the guard -----------------------------------------------------------------------------------
def test_trace_sees_the_accepted_points(oracle_lib):
    from test_gpu_quality_trace import _assert_record_is_report
    s = SCALINGS[0]
    ref = _reference(oracle_lib, "tiles_both", "com", False, s)
    n = CASES["dented_tiles"][2]
    e = _qc_engine("tiles_both", s=s)
    e.set_quality_trace(1)
    assert e.iterate(n, 0.0)[0] == n
    recs = e.quality_trace()
    assert len(recs) == n
    twin = _engine(_mesh("dented_tiles"), "com", False, **CASES["dented_tiles"][1])
    for k, rec in enumerate(recs, start=1):
        twin.set_points(ref["pts"][k - 1])
        _assert_record_is_report(rec, twin.mesh_quality(), k)
        assert rec.nNonPositiveVolume == 0 and rec.nWrongOrientedFaces == 0
    assert _records(e.quality_constraint_records_scaled()) == ref["recs"]


def test_guard_behind_the_scaled_constraint_does_not_trip(oracle_lib):
    s = SCALINGS[1]
    ref = _reference(oracle_lib, "dented", "com", False, s, 12)
    e = _qc_engine("dented", s=s)
    e.set_quality_trace(1)
    e.set_quality_guard()
    assert e.iterate(12, 0.0)[0] == 12
    g = e.quality_guard()
    assert g.armed and not g.tripped and g.snapshotIteration == 12
    recs = e.quality_constraint_records_scaled()
    assert _records(recs) == ref["recs"] and any(r.nPointsScaled > 0 for r in recs)
    assert np.array_equal(e.get_points(), ref["pts"][11])


# ---- 7. records across calls, switching, clearing ----------------------------------------------------------------------
def test_numbering_and_records_across_calls(oracle_lib):
    import ctypes as C
    from smoothmesh_amd import SmgpuError, _ffi
    s = SCALINGS[0]
    ref = _reference(oracle_lib, "dented", "com", False, s)
    e = _qc_engine("dented", s=s)
    assert e.iterate(3, 0.0)[0] == 3 and e.iterate(5, 0.0)[0] == 5
    n = C.c_int64(0)
    assert e._lib.smgpu_get_quality_constraint_records_scaled(e._h, None, 0, C.byref(n)) == 0 and n.value == 8
    buf = (_ffi.QualityConstraintRecordScaled * 8)()
    assert e._lib.smgpu_get_quality_constraint_records_scaled(e._h, buf, 7, C.byref(n)) != 0          # a short cap is an error ...
    with pytest.raises(SmgpuError, match="cap 7 is below the 8 pending records"):
        e._check(1)
    assert _records(e.quality_constraint_records_scaled()) == ref["recs"]                             # ... that clears nothing
    assert e.quality_constraint_records_scaled() == [] and e.quality_constraint_records() == []       # a read clears, for every getter
    assert e.quality_constraint_state_scaled().iteration == 8
    assert np.array_equal(e.get_points(), ref["pts"][7])
    # the narrower getters return the prefix of the same records
    e = _qc_engine("dented", s=s)
    assert e.iterate(8, 0.0)[0] == 8
    assert _records(e.quality_constraint_records(), FIELDS_ALL) == [{k: r[k] for k in FIELDS_ALL} for r in ref["recs"]]


def test_switching_on_off_on_between_calls(oracle_lib):
    """the scale state does not outlive an iteration and the numbering is the constraint's: a run that switches is, call by call,
    the run of two engines that do not, continued from the same points"""
    s = SCALINGS[0]
    e = _qc_engine("tiles_both", s=s)
    on, off = _qc_engine("tiles_both", s=s), _qc_engine("tiles_both", s=(0, 0.75, 4, 2))
    seen = 0
    for call, scaled in enumerate((True, False, True, False)):
        e.set_quality_constraint_scaling(**(_scaling(s) if scaled else dict(scalePasses=0)))
        assert e.quality_constraint_state_scaled().scalePasses == (s[0] if scaled else 0)
        twin = on if scaled else off
        twin.set_points(e.get_points())
        assert e.iterate(3, 0.0)[0] == 3 and twin.iterate(3, 0.0)[0] == 3
        assert np.array_equal(e.get_points(), twin.get_points()), call
        ra, rb = e.quality_constraint_records_scaled(), twin.quality_constraint_records_scaled()
        assert [r.iteration for r in ra] == [3 * call + 1, 3 * call + 2, 3 * call + 3]
        strip = [{k: v for k, v in r.items() if k != "iteration"} for r in _records(ra)]
        assert strip == [{k: v for k, v in r.items() if k != "iteration"} for r in _records(rb)], call
        seen += sum(r.nPointsScaled > 0 for r in ra)
        assert scaled or all(r.nScalePasses == 0 and r.minScale == 0.0 for r in ra)
    assert seen > 0


def test_clearing_the_constraint_switches_scaling_off():
    from smoothmesh_amd import SmgpuError
    e = _qc_engine("dented", s=SCALINGS[0])
    assert e.quality_constraint_state_scaled().scalePasses == 2
    e.clear_quality_constraint()
    st = e.quality_constraint_state_scaled()
    assert not st.on and (st.scalePasses, st.errorReduction, st.nSmoothScale) == (0, 0.75, 4)
    with pytest.raises(SmgpuError, match="the quality constraint is off"):
        e.set_quality_constraint_scaling(2)
    # re-enabling switches it off as well
    e = _qc_engine("dented", s=SCALINGS[0])
    e.set_quality_constraint(**_limits("dented"))
    assert e.quality_constraint_state_scaled().on and e.quality_constraint_state_scaled().scalePasses == 0


# ---- 8. refusals -------------------------------------------------------------------------------------------------------
def test_refusals():
    from smoothmesh_amd import SmgpuError
    from smoothmesh_amd.meshgen import hex_block
    from test_gpu_quality_guard import _set_boundary_smoothing
    e = _engine(hex_block(6, 5, 4, jitter=0.3))
    with pytest.raises(SmgpuError, match="smgpu_set_quality_constraint_scaling: the quality constraint is off"):
        e.set_quality_constraint_scaling(2)
    e.set_tangle_constraint()
    with pytest.raises(SmgpuError, match="the tangle constraint is on .*has no scaling passes"):
        e.set_quality_constraint_scaling(2)
    e.clear_tangle_constraint()
    e.set_quality_constraint()
    for kw, msg in ((dict(scalePasses=-1), "scalePasses < 0"), (dict(scalePasses=2, errorReduction=1.0), "errorReduction is outside"),
                    (dict(scalePasses=2, errorReduction=-0.1), "errorReduction is outside"), (dict(scalePasses=2, errorReduction=float("nan")), "errorReduction is outside"),
                    (dict(scalePasses=2, nSmoothScale=-1), "nSmoothScale < 0")):
        with pytest.raises(SmgpuError, match=msg):
            e.set_quality_constraint_scaling(**kw)
        assert e.quality_constraint_state_scaled().on and e.quality_constraint_state_scaled().scalePasses == 0
    e.set_quality_constraint(passes=2**31 - 2)
    with pytest.raises(SmgpuError, match="scalePasses \\+ passes is above 2147483647"):
        e.set_quality_constraint_scaling(2)
    e.set_quality_constraint()
    # through set_quality_constraint a refused scaling leaves the constraint off
    with pytest.raises(SmgpuError, match="nSmoothScale < 0"):
        e.set_quality_constraint(scalePasses=1, nSmoothScale=-1)
    assert not e.quality_constraint_state_scaled().on
    # an engine with boundary point smoothing
    e = _engine(hex_block(6, jitter=0.0))
    _set_boundary_smoothing(e)
    with pytest.raises(SmgpuError, match="smgpu_set_quality_constraint_scaling: not available on an engine with boundary point smoothing"):
        e.set_quality_constraint_scaling(2)
    with pytest.raises(SmgpuError, match="boundary point smoothing"):
        e.set_quality_constraint(scalePasses=2)


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
        with pytest.raises(SmgpuError, match="smgpu_set_quality_constraint_scaling: not available on an engine with a halo"):
            ds.engine.set_quality_constraint_scaling(2)
        for call in (ds.set_quality_constraint, ds.set_quality_constraint_limits_all):
            with pytest.raises(ValueError, match="scalePasses=2 .*is not available on a decomposed mesh"):
                call(scalePasses=2)
    finally:
        dist.destroy_process_group()


# ---- 9. front-end ------------------------------------------------------------------------------------------------------
def _run(case, opts):
    r = subprocess.run([BIN, "-case", str(case)] + opts, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _strip(out):
    return [x for x in out.splitlines() if not x.startswith(("Case: ", "ClockTime"))]


def test_front_end(tmp_path):
    from smoothmesh_amd.polymesh import read_polymesh, write_case
    from smoothmesh_amd.quality import format_quality_constraint_line, format_quality_constraint_scaling_line
    m = _mesh("dented")
    for d in "abc":
        write_case(str(tmp_path / d), m, binary=True, writeFormat="binary")
    plain = ["-centroidalIters", "8", "-relTol", "0", "-edgeAngleConstraint", "false", "-faceAngleConstraint", "false",
             "-maxStepLength", "1", "-minEdgeLength", "1e-4", "-writeInterval", "3"]
    limits = ["-qualityConstraint", "true", "-maxNonOrtho", "180", "-maxInternalSkewness", "0.4", "-maxBoundarySkewness", "0"]
    scaling = ["-scalePasses", "2", "-errorReduction", "0.5", "-nSmoothScale", "1"]
    e = _qc_engine("dented", s=SCALINGS[0])
    st = e.quality_constraint_state_scaled()
    assert e.iterate(8, 0.0)[0] == 8
    recs = e.quality_constraint_records_scaled()
    assert sum(r.nBadCells > 0 for r in recs) >= 2 and any(r.nPointsScaled > 0 for r in recs)
    lines = _run(tmp_path / "a", plain + limits + scaling).splitlines()
    setup = [f"Quality constraint: maxNonOrtho 180 maxInternalSkewness 0.4 maxBoundarySkewness 0, {st.nExemptCells} exempt cells, {st.nExemptFaces} exempt faces, 2 passes",
             format_quality_constraint_scaling_line(st).rstrip("\n")]
    assert setup[1] == "Quality constraint scaling: scalePasses 2 errorReduction 0.5 nSmoothScale 1"
    at = lines.index(setup[0])
    assert lines[at:at + 2] == setup and lines.count(setup[1]) == 1
    assert at < next(i for i, x in enumerate(lines) if x.startswith("Smoothing iteration="))
    want = []
    for r in recs:
        want.append(f"Smoothing iteration={r.iteration} ")
        if r.nBadCells > 0:
            want.append(format_quality_constraint_line(r, scaled=True).rstrip("\n"))
    got = [x for x in lines if x.startswith(("Smoothing iteration=", "    quality constraint "))]
    assert len(got) == len(want) and all(g == w or (w.endswith(" ") and g.startswith(w)) for g, w in zip(got, want)), got
    assert any(" scalePasses 2 pointsScaled " in x and " minScale " in x for x in got)
    pts = read_polymesh(str(tmp_path / "a" / "constant" / "polyMesh"), str(tmp_path / "a" / "8" / "polyMesh")).points
    assert np.array_equal(np.asarray(pts), e.get_points())
    # without the three options: the output it was, line for line -- the lines of the engine's records without scaling
    e = _qc_engine("dented")
    assert e.iterate(8, 0.0)[0] == 8
    want = []
    for r in e.quality_constraint_records():
        want.append(f"Smoothing iteration={r.iteration} ")
        if r.nBadCells > 0:
            want.append(format_quality_constraint_line(r).rstrip("\n"))
    off = _strip(_run(tmp_path / "b", plain + limits))
    got = [x for x in off if x.startswith(("Smoothing iteration=", "    quality constraint "))]
    assert len(got) == len(want) and all(g == w or (w.endswith(" ") and g.startswith(w)) for g, w in zip(got, want)), got
    assert not any("scaling" in x or "scalePasses" in x or "minScale" in x for x in off)
    # -scalePasses 0 is the run without the option
    zero = _strip(_run(tmp_path / "c", plain + limits + ["-scalePasses", "0"]))
    assert zero == off
