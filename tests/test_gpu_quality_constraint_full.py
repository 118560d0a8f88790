"""The quality constraint's tet, twist, weight, ratio and determinant limits (include/smgpu.h smgpu_set_quality_constraint_limits /
smgpu_get_quality_constraint_records_full / _state_full, csrc/kernels_quality_limits.hpp, DESIGN.md "Mesh quality" 10.16) against
their CPU restatement (tests/quality_constraint_full_reference.py, pinned by tests/test_quality_constraint_full_reference.py): the
accepted points of every iteration by == and every field of the full record; all six off through the new entry is the old entry;
the invariant through the engine's own reports; a constraint that never fires; the two getters; numbering; the guard's rollback;
refusals; and the lines of `smoothMesh -qualityConstraint true -minTwist ...`."""
import functools
import os
import subprocess

import numpy as np
import pytest

import tangle_reference
from quality_constraint_full_reference import FIELDS_FULL, MORE, MORE_MARGIN, reference_run
from quality_constraint_reference import FACE_MARGIN, FIELDS, OFF
from test_gpu_quality_trace import _engine
from test_gpu_tangle import CASES
from test_quality_constraint_full_reference import LIMITS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "smoothmesh_amd", "bin", "smoothMesh")

# (case of LIMITS, variant, constraints, passes, SMGPU_GEOM_T): each criterion alone; all six with two old ones under both variants,
# the reference's constraints off and on, fewer passes and the other tile shapes
RUNS = ([(c, "com", False, 2, 128) for c in LIMITS if c != "all"]
        + [("all", *s) for s in (("com", False, 2, 128), ("com", True, 2, 128), ("org", False, 2, 128), ("org", True, 2, 128),
                                 ("com", False, 0, 128), ("com", False, 1, 128), ("com", False, 2, 64), ("com", False, 2, 256))])


@functools.lru_cache(maxsize=None)
def _mesh(name):
    return CASES[name][0]()


def _limits(case):
    return {**OFF, **LIMITS[case][1]}


@functools.lru_cache(maxsize=None)
def _reference(oracle_lib, case, variant, constraints, passes):
    name = LIMITS[case][0]
    _, over, n = CASES[name]
    r = reference_run(oracle_lib, _mesh(name), n, limits=_limits(case), passes=passes, variant=variant, constraints=constraints, **over)
    ref = r["ref"]
    assert ref.minMargin > tangle_reference.MARGIN and ref.minCosGap > FACE_MARGIN and ref.minSkewGap > FACE_MARGIN
    assert all(g > MORE_MARGIN for g in ref.minGap.values())
    return r


def _records(recs, fields=FIELDS_FULL):
    return [{k: getattr(r, k) for k in fields} for r in recs]


def _qc_engine(case, variant="com", constraints=False, passes=2, **more):
    name = LIMITS[case][0]
    e = _engine(_mesh(name), variant, constraints, **{**CASES[name][1], **more})
    e.set_quality_constraint(passes=passes, **_limits(case))
    return e


# ---- 1. engine = reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,variant,constraints,passes,geomT", RUNS)
def test_engine_equals_reference(oracle_lib, monkeypatch, case, variant, constraints, passes, geomT):
    monkeypatch.setenv("SMGPU_GEOM_T", str(geomT))
    n = CASES[LIMITS[case][0]][2]
    ref = _reference(oracle_lib, case, variant, constraints, passes)
    e = _qc_engine(case, variant, constraints, passes)
    st, lim = e.quality_constraint_state(), _limits(case)
    assert st.on and st.passes == passes and st.iteration == 0
    for k in MORE:
        assert getattr(st, k) == ref["ref"].more[k]
    assert (st.maxNonOrtho, st.maxInternalSkewness, st.maxBoundarySkewness) == (lim["maxNonOrtho"], lim["maxInternalSkewness"], lim["maxBoundarySkewness"])
    assert (st.nExemptCells, st.nExemptFaces, st.nExemptDeterminantCells) == (ref["ref"].nExemptCells, ref["ref"].nExemptFaces, ref["ref"].nExemptDeterminantCells)
    for k in range(n):
        assert e.iterate(1, 0.0)[0] == 1
        rec = _records(e.quality_constraint_records())
        assert rec == [ref["recs"][k]], (k, rec, ref["recs"][k])
        assert np.array_equal(e.get_points(), ref["pts"][k]), k
    assert e.quality_constraint_state().iteration == n
    if case != "all":
        count = MORE[next(iter(LIMITS[case][1]))][1]
        assert any(r[count] > 0 for r in ref["recs"]), "no limit is met: the case tests nothing"
    elif (variant, constraints) == ("com", False):
        assert any(r["nBadCells"] > 0 for r in ref["recs"]), "no limit is met: the case tests nothing"


@pytest.mark.parametrize("case", ["all", "tiles_weight", "determinant"])
def test_without_tiles_equals_tiled(monkeypatch, case):
    n = CASES[LIMITS[case][0]][2]

    def run(env):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            e = _qc_engine(case)
        assert e.iterate(n, 0.0)[0] == n
        return e.get_points(), e.quality_constraint_records(), e.quality_constraint_state()

    tiled, direct = run({}), run({"SMGPU_TILES": "0"})
    assert np.array_equal(tiled[0], direct[0]) and tiled[1] == direct[1] and tiled[2] == direct[2]
    assert any(r.nBadCells > 0 for r in tiled[1])


# ---- 2. all six off through the new entry: the old entry ---------------------------------------------------------------
@pytest.mark.parametrize("name,lim", [("dented_tiles", dict(maxInternalSkewness=0.4, maxBoundarySkewness=0.1)),
                                      ("cavity_interface", dict(maxNonOrtho=40.0, maxInternalSkewness=0.5, maxBoundarySkewness=0.5))])
def test_all_six_off_is_the_old_entry(name, lim):
    import ctypes as C
    from smoothmesh_amd import _ffi
    from smoothmesh_amd.engine import QUALITY_CONSTRAINT_LIMITS_OFF
    _, over, n = CASES[name]
    lim = {**OFF, **lim}
    a, b = _engine(_mesh(name), "com", False, **over), _engine(_mesh(name), "com", False, **over)
    a.set_quality_constraint(**lim, **QUALITY_CONSTRAINT_LIMITS_OFF)          # every new limit given, at its off value
    b.set_quality_constraint(**lim)
    for x in (a, b):
        x.reset_counters()

    def narrow(e):
        cnt = C.c_int64(0)
        assert e._lib.smgpu_get_quality_constraint_records(e._h, None, 0, C.byref(cnt)) == 0
        buf = (_ffi.QualityConstraintRecord * max(1, cnt.value))()
        assert e._lib.smgpu_get_quality_constraint_records(e._h, buf, cnt.value, C.byref(cnt)) == 0
        return [tuple(getattr(r, f) for f in FIELDS) for r in buf[:cnt.value]]

    def old_state(e):
        s = _ffi.QualityConstraintState()
        assert e._lib.smgpu_get_quality_constraint_state(e._h, C.byref(s)) == 0
        return tuple(getattr(s, f) for f, _ in s._fields_)

    assert old_state(a) == old_state(b) and a.quality_constraint_state() == b.quality_constraint_state()
    fired = False
    for k in range(n):
        assert a.iterate(1, 0.0)[0] == 1 and b.iterate(1, 0.0)[0] == 1
        ra, rb = narrow(a), narrow(b)
        assert ra == rb and len(ra) == 1, k
        fired = fired or ra[0][FIELDS.index("nBadCells")] > 0
        assert np.array_equal(a.get_points(), b.get_points()), k
    assert fired and old_state(a) == old_state(b)
    assert {c["name"]: c["launches"] for c in a.counters()} == {c["name"]: c["launches"] for c in b.counters()}


def test_old_entry_leaves_the_six_new_counts_zero():
    """under smgpu_set_quality_constraint one verdict kernel writes the whole slot: drained through the full getter, the six counts
    of 10.16 are exactly 0 in every record, as the zeroed slot's were while only its head was written"""
    name = "dented_tiles"
    _, over, n = CASES[name]
    e = _engine(_mesh(name), "com", False, **over)
    e.set_quality_constraint(**{**OFF, **dict(maxInternalSkewness=0.4, maxBoundarySkewness=0.1)})
    assert e.iterate(n, 0.0)[0] == n
    recs = e.quality_constraint_records()                                       # (smgpu_get_quality_constraint_records_full)
    assert len(recs) == n and any(r.nBadCells > 0 for r in recs)
    assert all(getattr(r, MORE[k][1]) == 0 for r in recs for k in MORE)


# ---- 3. the invariant, through the engine's own reports ----------------------------------------------------------------
@pytest.mark.parametrize("case", ["all", "tiles_weight"])
def test_invariant_through_the_reports(oracle_lib, case):
    from quality_constraint_full_reference import QualityConstraintFullReference
    from tangle_reference import make_oracle
    m, (_, over, n), lim = _mesh(LIMITS[case][0]), CASES[LIMITS[case][0]], _limits(case)
    ref = QualityConstraintFullReference(make_oracle(oracle_lib, m, "com", False, **over), m, **lim)   # the exempt elements
    exemptF, exemptD, on = ref.exemptFaces, ref.exemptDet, ref.on
    e = _engine(m, "com", False, **over)
    e.set_quality_constraint(**lim)
    st = e.quality_constraint_state()
    assert (st.nExemptFaces, st.nExemptDeterminantCells) == (int(exemptF.sum()), int(exemptD.sum()))
    more = ref.more
    for _ in range(n):
        assert e.iterate(1, 0.0)[0] == 1
        sm = e.quality_motion_sets(tetThreshold=more["minTetQuality"], twistThreshold=more["minTwist"], triangleTwistThreshold=more["minTriangleTwist"])
        sg = e.quality_geometry_sets(weightThreshold=more["minFaceWeight"], volRatioThreshold=more["minVolRatio"], determinantThreshold=more["minDeterminant"])
        for k, s, name in (("minTetQuality", sm, "lowQualityTetFaces"), ("minTwist", sm, "twistedFaces"), ("minTriangleTwist", sm, "lowTriangleTwistFaces"),
                           ("minFaceWeight", sg, "lowWeightFaces"), ("minVolRatio", sg, "lowVolRatioFaces")):
            if on[k]:
                assert exemptF[s[name]].all(), (k, s[name])
        if on["minDeterminant"]:
            assert exemptD[sg["underdeterminedCells"]].all()


# ---- 4. a constraint that never fires leaves the run untouched ---------------------------------------------------------
def test_constraint_that_never_fires_leaves_the_run_untouched():
    from smoothmesh_amd.polymesh import cavity_mesh
    m = cavity_mesh(16, jitter=0.2, seed=3)
    runs = []
    for on in (False, True):
        e = _engine(m)
        if on:   # on, and out of reach: tet quality >= -1 by its normalisation, the twists are cosines, the others are >= 0
            e.set_quality_constraint(179.9, 1e9, 1e9, minTetQuality=-1e9, minTwist=-0.999999, minTriangleTwist=-0.999999, minFaceWeight=1e-12,
                                     minVolRatio=1e-12, minDeterminant=1e-12)
            st = e.quality_constraint_state()
            assert st.on and (st.nExemptCells, st.nExemptFaces, st.nExemptDeterminantCells) == (0, 0, 0) and st.minTwist == -0.999999
        n, res, frz = e.iterate(10, 0.0)
        assert n == 10
        if on:
            zero = {k: 0 for k in FIELDS_FULL}
            assert _records(e.quality_constraint_records()) == [{**zero, "iteration": k} for k in range(1, 11)]
        runs.append((res, frz, e.get_points(), e.near_ties(), e.last_near_ties, e.debug_walk_mode()))
    a, b = runs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[3] == b[3] and np.array_equal(a[4], b[4]) and a[5] == b[5]


# ---- 5. the getters, numbering, the guard's rollback, refusals ----------------------------------------------------------
def test_two_getters_drain_one_list_and_numbering(oracle_lib):
    import ctypes as C
    from smoothmesh_amd import SmgpuError, _ffi
    ref = _reference(oracle_lib, "all", "com", False, 2)
    e = _qc_engine("all")
    assert e.iterate(3, 0.0)[0] == 3 and e.iterate(4, 0.0)[0] == 4
    n = C.c_int64(0)
    for getter in ("smgpu_get_quality_constraint_records", "smgpu_get_quality_constraint_records_full"):
        assert getattr(e._lib, getter)(e._h, None, 0, C.byref(n)) == 0 and n.value == 7
    full = (_ffi.QualityConstraintRecordFull * 7)()
    assert e._lib.smgpu_get_quality_constraint_records_full(e._h, full, 6, C.byref(n)) != 0
    with pytest.raises(SmgpuError, match="smgpu_get_quality_constraint_records_full: cap 6 is below the 7 pending records"):
        e._check(1)
    narrow = (_ffi.QualityConstraintRecord * 7)()
    assert e._lib.smgpu_get_quality_constraint_records(e._h, narrow, 7, C.byref(n)) == 0 and n.value == 7      # the heads ...
    assert [{k: getattr(r, k) for k in FIELDS} for r in narrow] == [{k: r[k] for k in FIELDS} for r in ref["recs"][:7]]
    assert e._lib.smgpu_get_quality_constraint_records_full(e._h, None, 0, C.byref(n)) == 0 and n.value == 0   # ... drained the one list
    assert e.iterate(3, 0.0)[0] == 3
    assert _records(e.quality_constraint_records()) == ref["recs"][7:10] and e.quality_constraint_records() == []
    assert e.quality_constraint_state().iteration == 10
    e.set_quality_constraint(passes=1, **_limits("all"))                       # again: the numbering restarts
    assert e.quality_constraint_state().iteration == 0
    assert e.iterate(2, 0.0)[0] == 2 and [r.iteration for r in e.quality_constraint_records()] == [1, 2]


def test_running_number_goes_back_with_the_guards_rollback():
    from smoothmesh_amd.meshgen import hex_block
    e = _engine(hex_block(12, 9, 7, jitter=0.3))
    e.set_quality_trace(3)
    e.set_quality_guard()
    assert e.iterate(2, 0.0)[0] == 2
    e.set_quality_constraint(minTwist=0.0, minDeterminant=1e-6)
    assert e.iterate(7, 0.0)[0] == 7
    assert e.quality_constraint_state().iteration == 7 and e.quality_guard().snapshotIteration == 9
    assert e.iterate(1, 0.0)[0] == 1
    e.quality_guard_restore()
    assert e.quality_guard().restoredIteration == 9 and e.quality_constraint_state().iteration == 7
    assert [r.iteration for r in e.quality_constraint_records()] == list(range(1, 9))
    assert e.iterate(2, 0.0)[0] == 2
    assert [r.iteration for r in e.quality_constraint_records()] == [8, 9]


def test_refusals_and_the_off_state():
    from smoothmesh_amd import SmgpuError
    from smoothmesh_amd.engine import QUALITY_CONSTRAINT_LIMITS_OFF
    from smoothmesh_amd.meshgen import hex_block
    from test_gpu_quality_guard import _set_boundary_smoothing
    m = hex_block(6, 5, 4, jitter=0.3)
    e = _engine(m)
    st = e.quality_constraint_state()
    assert not st.on and st.nExemptDeterminantCells == 0 and [getattr(st, k) for k in MORE] == list(QUALITY_CONSTRAINT_LIMITS_OFF.values())
    with pytest.raises(SmgpuError, match="smgpu_set_quality_constraint_limits: passes < 0"):
        e.set_quality_constraint(passes=-1, minTwist=0.1)
    for k in MORE:
        with pytest.raises(SmgpuError, match="smgpu_set_quality_constraint_limits: a limit is NaN"):
            e.set_quality_constraint(**{k: float("nan")})
    with pytest.raises(SmgpuError, match="a limit is NaN"):
        e.set_quality_constraint(maxNonOrtho=float("nan"), minTwist=0.1)
    assert not e.quality_constraint_state().on
    e.set_tangle_constraint()
    with pytest.raises(SmgpuError, match="smgpu_set_quality_constraint_limits: the tangle constraint is on"):
        e.set_quality_constraint(minTwist=0.1)
    e.clear_tangle_constraint()
    e.set_quality_constraint(60.0, 3.0, 10.0, passes=3, minTwist=0.1, minVolRatio=0.01)
    st = e.quality_constraint_state()
    assert st.on and (st.passes, st.maxNonOrtho, st.minTwist, st.minVolRatio, st.minTetQuality, st.minDeterminant) == (3, 60.0, 0.1, 0.01, -1e30, 0.0)
    with pytest.raises(SmgpuError, match="the quality constraint is on"):
        e.set_tangle_constraint()
    with pytest.raises(SmgpuError, match="quality constraint"):
        _set_boundary_smoothing(e)
    assert e.iterate(3, 0.0)[0] == 3
    e.set_quality_constraint(60.0, 3.0, 10.0)                      # the old entry replaces the new one: its limits are off again
    st = e.quality_constraint_state()
    assert st.on and [getattr(st, k) for k in MORE] == list(QUALITY_CONSTRAINT_LIMITS_OFF.values())
    e.clear_quality_constraint()
    assert not e.quality_constraint_state().on and e.quality_constraint_records() == []
    e = _engine(hex_block(6, jitter=0.0))
    _set_boundary_smoothing(e)
    with pytest.raises(SmgpuError, match="smgpu_set_quality_constraint_limits: not available on an engine with boundary point smoothing"):
        e.set_quality_constraint(minTwist=0.1)


# ---- 6. front-end ------------------------------------------------------------------------------------------------------
def test_front_end(tmp_path):
    from smoothmesh_amd.polymesh import read_polymesh, write_case
    from smoothmesh_amd.quality import format_quality_constraint_limits_line, format_quality_constraint_line
    name = LIMITS["all"][0]
    m, (_, over, n) = _mesh(name), CASES[name]
    for d in "ab":
        write_case(str(tmp_path / d), m, binary=True, writeFormat="binary")
    plain = ["-centroidalIters", str(n), "-relTol", "0", "-edgeAngleConstraint", "false", "-faceAngleConstraint", "false",
             "-maxStepLength", str(over["maxStepLength"]), "-minEdgeLength", str(over["minEdgeLength"]), "-writeInterval", "4"]
    lim = _limits("all")
    opts = ["-qualityConstraint", "true"] + [x for k, v in lim.items() for x in (f"-{k}", repr(v))]
    e = _qc_engine("all")
    st = e.quality_constraint_state()
    assert e.iterate(n, 0.0)[0] == n
    recs = e.quality_constraint_records()
    assert any(r.nBadCells > 0 for r in recs)
    r = subprocess.run([BIN, "-case", str(tmp_path / "a")] + plain + opts, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    first = next(i for i, x in enumerate(lines) if x.startswith("Quality constraint: "))
    assert lines[first].endswith(f", {st.nExemptCells} exempt cells, {st.nExemptFaces} exempt faces, 2 passes")
    assert lines[first + 1] == format_quality_constraint_limits_line(st).rstrip("\n")
    want = []
    for rec in recs:
        want.append(f"Smoothing iteration={rec.iteration} ")
        if rec.nBadCells > 0:
            want.append(format_quality_constraint_line(rec, more=True).rstrip("\n"))
    got = [x for x in lines if x.startswith(("Smoothing iteration=", "    quality constraint "))]
    assert len(got) == len(want) and all(g == w or (w.endswith(" ") and g.startswith(w)) for g, w in zip(got, want)), got
    pts = read_polymesh(str(tmp_path / "a" / "constant" / "polyMesh"), str(tmp_path / "a" / str(n) / "polyMesh")).points
    assert np.array_equal(np.asarray(pts), e.get_points())
    # none of the six given: the parent's lines
    old = ["-qualityConstraint", "true"] + [x for k in OFF for x in (f"-{k}", repr(lim[k]))]
    r = subprocess.run([BIN, "-case", str(tmp_path / "b")] + plain + old, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0
    assert not any(x.startswith("Quality constraint limits:") or " lowTetFaces " in x for x in r.stdout.splitlines())
