"""The quality constraint's last four limits -- maxConcave, minFlatness, minVol, minArea (include/smgpu.h
smgpu_set_quality_constraint_limits_all / smgpu_get_quality_constraint_records_all / _state_all, csrc/kernels_quality_limits.hpp,
DESIGN.md "Mesh quality" 10.18) -- against their CPU restatement (tests/quality_constraint_all_reference.py, pinned by
tests/test_quality_constraint_all_reference.py): the accepted points of every iteration by == and every field of the widest record;
all four off through the new entry is smgpu_set_quality_constraint_limits' run with its launches; the older entries leave the four
counts 0; the invariant through the engine's own reports; a constraint that never fires; the three getters; refusals."""
import functools

import numpy as np
import pytest

import tangle_reference
from quality_constraint_all_reference import FIELDS_ALL, LAST, LAST_MARGIN, LAST_OFF, QualityConstraintAllReference, reference_run
from quality_constraint_full_reference import FIELDS_FULL, MORE, MORE_MARGIN
from quality_constraint_reference import FACE_MARGIN, FIELDS, OFF
from test_gpu_quality_trace import _engine
from test_gpu_tangle import CASES
from test_quality_constraint_all_reference import LIMITS
from test_quality_constraint_full_reference import LIMITS as FULL_LIMITS

pytestmark = pytest.mark.gpu

# (case of LIMITS, variant, constraints, passes, SMGPU_GEOM_T): each criterion alone and the volume-exempt case; all thirteen under
# both variants, the reference's constraints off and on, fewer passes and the other tile shapes
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
    assert all(g > MORE_MARGIN for g in ref.minGap.values()) and all(g > LAST_MARGIN for g in ref.minGapLast.values())
    return r


def _records(recs, fields=FIELDS_ALL):
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
    st, lim, r = e.quality_constraint_state(), _limits(case), ref["ref"]
    assert st.on and st.passes == passes and st.iteration == 0
    for k in MORE:
        assert getattr(st, k) == r.more[k]
    for k in LAST:
        assert getattr(st, k) == r.lastLim[k]
    assert (st.maxNonOrtho, st.maxInternalSkewness, st.maxBoundarySkewness) == (lim["maxNonOrtho"], lim["maxInternalSkewness"], lim["maxBoundarySkewness"])
    assert (st.nExemptCells, st.nExemptFaces, st.nExemptDeterminantCells, st.nExemptVolumeCells) == (r.nExemptCells, r.nExemptFaces, r.nExemptDeterminantCells,
                                                                                                       r.nExemptVolumeCells)
    for k in range(n):
        assert e.iterate(1, 0.0)[0] == 1
        rec = _records(e.quality_constraint_records())
        assert rec == [ref["recs"][k]], (k, rec, ref["recs"][k])
        assert np.array_equal(e.get_points(), ref["pts"][k]), k
    assert e.quality_constraint_state().iteration == n
    if case == "all":
        if (variant, constraints) == ("com", False):
            assert all(any(x[LAST[k][1]] > 0 for x in ref["recs"]) for k in LAST), "a limit is never met: the case tests less than it says"
    elif case == "vol_exempt":
        assert r.nExemptVolumeCells > 0 and any(x["nConcaveFaces"] > 0 for x in ref["recs"])
    else:
        count = LAST[next(iter(LIMITS[case][1]))][1]
        assert any(x[count] > 0 for x in ref["recs"]), "no limit is met: the case tests nothing"


@pytest.mark.parametrize("case", ["all", "tiles_concave", "vol", "flatness"])
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


# ---- 2. all four off through the new entry: smgpu_set_quality_constraint_limits ------------------------------------------
@pytest.mark.parametrize("name,lim", [("dented_tiles", dict(maxInternalSkewness=0.4, maxBoundarySkewness=0.1, minFaceWeight=0.425)),
                                      ("cavity_interface", FULL_LIMITS["all"][1])])
def test_all_four_off_is_the_limits_entry(name, lim):
    import ctypes as C
    from smoothmesh_amd import _ffi
    _, over, n = CASES[name]
    lim = {**OFF, **lim}
    a, b = _engine(_mesh(name), "com", False, **over), _engine(_mesh(name), "com", False, **over)
    a.set_quality_constraint(**lim, **LAST_OFF)                    # every new limit given, at its off value: the new entry
    b.set_quality_constraint(**lim)                                # smgpu_set_quality_constraint_limits
    for x in (a, b):
        x.reset_counters()

    def full(e):
        cnt = C.c_int64(0)
        assert e._lib.smgpu_get_quality_constraint_records_full(e._h, None, 0, C.byref(cnt)) == 0
        buf = (_ffi.QualityConstraintRecordFull * max(1, cnt.value))()
        assert e._lib.smgpu_get_quality_constraint_records_full(e._h, buf, cnt.value, C.byref(cnt)) == 0
        return [tuple(getattr(r, f) for f in FIELDS_FULL) for r in buf[:cnt.value]]

    def full_state(e):
        s = _ffi.QualityConstraintStateFull()
        assert e._lib.smgpu_get_quality_constraint_state_full(e._h, C.byref(s)) == 0
        return tuple(getattr(s, f) for f, _ in s._fields_)

    assert full_state(a) == full_state(b) and a.quality_constraint_state() == b.quality_constraint_state()
    fired = more = False
    for k in range(n):
        assert a.iterate(1, 0.0)[0] == 1 and b.iterate(1, 0.0)[0] == 1
        ra, rb = full(a), full(b)
        assert ra == rb and len(ra) == 1, k
        fired = fired or ra[0][FIELDS_FULL.index("nBadCells")] > 0
        more = more or any(ra[0][FIELDS_FULL.index(MORE[m][1])] > 0 for m in MORE)
        assert np.array_equal(a.get_points(), b.get_points()), k
    assert fired and more and full_state(a) == full_state(b)
    ca, cb = ({c["name"]: c["launches"] for c in e.counters()} for e in (a, b))
    assert ca == cb


def test_older_entries_leave_the_four_new_counts_zero():
    """under the two older entries the one verdict kernel writes the whole slot: drained through the widest getter, the four counts
    of 10.18 are exactly 0 in every record, and the state shows the four limits at their off values"""
    for name, lim in (("dented_tiles", dict(maxInternalSkewness=0.4, maxBoundarySkewness=0.1)), ("cavity_interface", FULL_LIMITS["weight"][1])):
        _, over, n = CASES[name]
        e = _engine(_mesh(name), "com", False, **over)
        e.set_quality_constraint(**{**OFF, **lim})
        st = e.quality_constraint_state()
        assert [getattr(st, k) for k in LAST] == list(LAST_OFF.values()) and st.nExemptVolumeCells == 0
        assert e.iterate(n, 0.0)[0] == n
        recs = e.quality_constraint_records()                                   # (smgpu_get_quality_constraint_records_all)
        assert len(recs) == n and any(r.nBadCells > 0 for r in recs)
        assert all(getattr(r, LAST[k][1]) == 0 for r in recs for k in LAST)


# ---- 3. the invariant, through the engine's own reports ----------------------------------------------------------------
@pytest.mark.parametrize("case", ["all", "tiles_concave", "vol_exempt"])
def test_invariant_through_the_reports(oracle_lib, case):
    from tangle_reference import make_oracle
    m, (_, over, n), lim = _mesh(LIMITS[case][0]), CASES[LIMITS[case][0]], _limits(case)
    ref = QualityConstraintAllReference(make_oracle(oracle_lib, m, "com", False, **over), m, **lim)   # the exempt elements
    exemptF, exemptV, on, last = ref.exemptFaces, ref.exemptVol, ref.onLast, ref.lastLim
    e = _engine(m, "com", False, **over)
    e.set_quality_constraint(**lim)
    st = e.quality_constraint_state()
    assert (st.nExemptFaces, st.nExemptVolumeCells) == (int(exemptF.sum()), int(exemptV.sum()))
    for _ in range(n):
        assert e.iterate(1, 0.0)[0] == 1
        # (thresholds of the criteria that are off: values nothing fails)
        sg = e.quality_geometry_sets(concaveThreshold=last["maxConcave"], flatnessThreshold=last["minFlatness"])
        if on["maxConcave"]:
            assert exemptF[sg["concaveFaces"]].all(), sg["concaveFaces"]
        if on["minFlatness"]:
            assert exemptF[sg["warpedFaces"]].all(), sg["warpedFaces"]
        if on["minVol"]:
            assert exemptV[e.quality_field("cellVolume") < last["minVol"]].all()
        if on["minArea"]:
            q = e.mesh_quality()
            a = e.debug_field("faceAreas").reshape(-1, 3)                          # the report's own S_f of the accepted points
            area = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
            assert area.min() == q.minFaceArea
            assert exemptF[area < last["minArea"]].all()


# ---- 4. a constraint that never fires leaves the run untouched ---------------------------------------------------------
def test_constraint_that_never_fires_leaves_the_run_untouched():
    from smoothmesh_amd.polymesh import cavity_mesh
    m = cavity_mesh(16, jitter=0.2, seed=3)
    runs = []
    for on in (False, True):
        e = _engine(m)
        if on:   # on, and out of reach: sin(90 degrees) is 1, which only a convex right angle's sine reaches; the others are > 0
            e.set_quality_constraint(179.9, 1e9, 1e9, maxConcave=90.0, minFlatness=1e-12, minVol=1e-300, minArea=1e-300)
            st = e.quality_constraint_state()
            assert st.on and (st.nExemptCells, st.nExemptFaces, st.nExemptDeterminantCells, st.nExemptVolumeCells) == (0, 0, 0, 0)
            assert (st.maxConcave, st.minFlatness, st.minVol, st.minArea) == (90.0, 1e-12, 1e-300, 1e-300)
        n, res, frz = e.iterate(10, 0.0)
        assert n == 10
        if on:
            zero = {k: 0 for k in FIELDS_ALL}
            assert _records(e.quality_constraint_records()) == [{**zero, "iteration": k} for k in range(1, 11)]
        runs.append((res, frz, e.get_points(), e.near_ties(), e.last_near_ties, e.debug_walk_mode()))
    a, b = runs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[3] == b[3] and np.array_equal(a[4], b[4]) and a[5] == b[5]


# ---- 5. the getters, refusals ------------------------------------------------------------------------------------------
def test_three_getters_drain_one_list(oracle_lib):
    import ctypes as C
    from smoothmesh_amd import SmgpuError, _ffi
    ref = _reference(oracle_lib, "all", "com", False, 2)
    e = _qc_engine("all")
    getters = {"smgpu_get_quality_constraint_records": (_ffi.QualityConstraintRecord, FIELDS),
               "smgpu_get_quality_constraint_records_full": (_ffi.QualityConstraintRecordFull, FIELDS_FULL),
               "smgpu_get_quality_constraint_records_all": (_ffi.QualityConstraintRecordAll, FIELDS_ALL)}
    n, at = C.c_int64(0), 0
    for getter, (struct, fields) in getters.items():
        assert e.iterate(2, 0.0)[0] == 2
        for g in getters:
            assert getattr(e._lib, g)(e._h, None, 0, C.byref(n)) == 0 and n.value == 2
        buf = (struct * 2)()
        assert getattr(e._lib, getter)(e._h, buf, 1, C.byref(n)) != 0
        with pytest.raises(SmgpuError, match=f"{getter}: cap 1 is below the 2 pending records"):
            e._check(1)
        assert getattr(e._lib, getter)(e._h, buf, 2, C.byref(n)) == 0 and n.value == 2
        assert [{k: getattr(r, k) for k in fields} for r in buf] == [{k: r[k] for k in fields} for r in ref["recs"][at:at + 2]]
        for g in getters:                                                       # ... drained the one list
            assert getattr(e._lib, g)(e._h, None, 0, C.byref(n)) == 0 and n.value == 0
        at += 2
    assert e.quality_constraint_state().iteration == 6


def test_refusals_and_the_off_state():
    from smoothmesh_amd import SmgpuError
    from smoothmesh_amd.meshgen import hex_block
    e = _engine(hex_block(6, 5, 4, jitter=0.3))
    st = e.quality_constraint_state()
    assert not st.on and st.nExemptVolumeCells == 0 and [getattr(st, k) for k in LAST] == list(LAST_OFF.values())
    for k in LAST:
        with pytest.raises(SmgpuError, match="smgpu_set_quality_constraint_limits_all: a limit is NaN"):
            e.set_quality_constraint(**{k: float("nan")})
    with pytest.raises(SmgpuError, match="smgpu_set_quality_constraint_limits_all: a limit is NaN"):
        e.set_quality_constraint(minTwist=float("nan"), minArea=1e-9)
    with pytest.raises(SmgpuError, match="smgpu_set_quality_constraint_limits_all: maxConcave < 0"):
        e.set_quality_constraint(maxConcave=-1.0)
    with pytest.raises(SmgpuError, match="smgpu_set_quality_constraint_limits_all: passes < 0"):
        e.set_quality_constraint(passes=-1, minVol=1e-9)
    assert not e.quality_constraint_state().on
    e.set_tangle_constraint()
    with pytest.raises(SmgpuError, match="smgpu_set_quality_constraint_limits_all: the tangle constraint is on"):
        e.set_quality_constraint(minArea=1e-9)
    e.clear_tangle_constraint()
    e.set_quality_constraint(60.0, 3.0, 10.0, passes=3, minTwist=0.1, maxConcave=80.0, minVol=1e-9)
    st = e.quality_constraint_state()
    assert st.on and (st.passes, st.maxNonOrtho, st.minTwist, st.maxConcave, st.minFlatness, st.minVol, st.minArea) == (3, 60.0, 0.1, 80.0, 0.0, 1e-9, 0.0)
    assert e.iterate(3, 0.0)[0] == 3
    e.set_quality_constraint(60.0, 3.0, 10.0, minTwist=0.1)        # an older entry replaces the new one: its limits are off again
    st = e.quality_constraint_state()
    assert st.on and st.minTwist == 0.1 and [getattr(st, k) for k in LAST] == list(LAST_OFF.values())
    e.clear_quality_constraint()
    assert not e.quality_constraint_state().on and e.quality_constraint_records() == []


# ---- 6. front-end: the four options, and the limits from a meshQualityDict -------------------------------------------------
def _dict_text(limits, extra=""):
    head = "FoamFile\n{\n    version 2.0;\n    format ascii;\n    class dictionary;\n    object meshQualityDict;\n}\n"
    return head + "".join(f"{k} {v!r};\n" for k, v in limits.items()) + extra


def test_front_end(tmp_path):
    import os
    import subprocess
    from smoothmesh_amd.polymesh import read_polymesh, write_case
    from smoothmesh_amd.quality import format_quality_constraint_limits_line, format_quality_constraint_line, read_mesh_quality_dict
    BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "smoothmesh_amd", "bin", "smoothMesh")
    name = LIMITS["all"][0]
    m, (_, over, n) = _mesh(name), CASES[name]
    for d in "abcd":
        write_case(str(tmp_path / d), m, binary=True, writeFormat="binary")
        os.makedirs(tmp_path / d / "system", exist_ok=True)
    plain = ["-centroidalIters", str(n), "-relTol", "0", "-edgeAngleConstraint", "false", "-faceAngleConstraint", "false",
             "-maxStepLength", str(over["maxStepLength"]), "-minEdgeLength", str(over["minEdgeLength"]), "-writeInterval", "4"]
    lim = _limits("all")
    e = _qc_engine("all")
    st = e.quality_constraint_state()
    assert e.iterate(n, 0.0)[0] == n
    recs = e.quality_constraint_records()
    assert any(r.nBadCells > 0 for r in recs)
    want = []
    for rec in recs:
        want.append(f"Smoothing iteration={rec.iteration} ")
        if rec.nBadCells > 0:
            want.append(format_quality_constraint_line(rec, last=True).rstrip("\n"))
    limitsLine = format_quality_constraint_limits_line(st).rstrip("\n")
    assert " maxConcave 60 minFlatness 0.91 minVol 0.00023 minArea 0.0035, 4 determinant-exempt cells, 1 volume-exempt cells" in limitsLine

    def run(case, opts):
        r = subprocess.run([BIN, "-case", str(tmp_path / case)] + plain + ["-qualityConstraint", "true"] + opts, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout.splitlines()

    def check(case, lines, source=None):
        first = next(i for i, x in enumerate(lines) if x.startswith("Quality constraint: "))
        assert lines[first].endswith(f", {st.nExemptCells} exempt cells, {st.nExemptFaces} exempt faces, 2 passes")
        assert lines[first + 1] == limitsLine
        if source is not None:
            assert lines[first + 2] == source
        assert not lines[first + (2 if source is None else 3)].startswith("Quality constraint")
        got = [x for x in lines if x.startswith(("Smoothing iteration=", "    quality constraint "))]
        assert len(got) == len(want) and all(g == w or (w.endswith(" ") and g.startswith(w)) for g, w in zip(got, want)), got
        pts = read_polymesh(str(tmp_path / case / "constant" / "polyMesh"), str(tmp_path / case / str(n) / "polyMesh")).points
        assert np.array_equal(np.asarray(pts), e.get_points())

    # (a) every limit as an option
    check("a", run("a", [x for k, v in lim.items() for x in (f"-{k}", repr(v))]))
    # (b) the limits from <case>/system/meshQualityDict; its minArea would exempt every face, the option on the command line wins
    path = tmp_path / "b" / "system" / "meshQualityDict"
    path.write_text(_dict_text({**lim, "minArea": 1.0}, "nSmoothScale 4;\nerrorReduction 0.75;\nrelaxed\n{\n    maxNonOrtho 75;\n}\n"))
    d = read_mesh_quality_dict(path, etc_dirs=[])
    assert {**d, "minArea": lim["minArea"]} == lim and d.ignored == ("nSmoothScale", "errorReduction", "relaxed")
    check("b", run("b", ["-meshQualityDict", "true", "-minArea", repr(lim["minArea"])]),
          f"Quality constraint: limits from {tmp_path / 'b'}/system/meshQualityDict, ignored: nSmoothScale errorReduction relaxed")
    # ... and the same file, named relative to the case, through the Python call: the engine the options made
    twin = _engine(m, "com", False, **over)
    twin.set_quality_constraint(**{**d, "minArea": lim["minArea"]})
    assert twin.quality_constraint_state() == _qc_engine("all").quality_constraint_state()
    # (c) a dict with none of the four on: the parent's lines, plus the line that names the file
    older = {k: v for k, v in lim.items() if k not in LAST}
    (tmp_path / "c" / "dicts").mkdir()
    (tmp_path / "c" / "dicts" / "mine").write_text(_dict_text({**older, "maxConcave": 180, "minFlatness": -1, "minVol": -1e30, "minArea": -1}))
    withDict = run("c", ["-meshQualityDict", "dicts/mine"])
    parent = run("d", [x for k, v in older.items() for x in (f"-{k}", repr(v))])
    source = f"Quality constraint: limits from {tmp_path / 'c'}/dicts/mine"
    assert source in withDict and not any(x.startswith("Quality constraint: limits from") for x in parent)
    keep = lambda lines: [x for x in lines if x.startswith(("Quality constraint", "Smoothing iteration=", "    quality constraint "))]   # noqa: E731
    assert [x for x in keep(withDict) if x != source] == keep(parent)
    assert not any(" concaveFaces " in x or "volume-exempt" in x for x in withDict) and any(" lowTetFaces " in x for x in withDict)
