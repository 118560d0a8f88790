"""The reductions of the three quality reports under load: ties, thresholds hit exactly, the fold order (DESIGN.md "Mesh quality"
10.1, 10.6, 10.7, 10.10, 10.14).  Everything here is bitwise or exact: a report is a function of the engine's own per-element
fields (tests/quality_fold_reference.py: fold_sum, lowest_extreme, the count predicates written from DESIGN), a set is flatnonzero
of its predicate, a threshold equal to an element's own value counts that element on the strict side only.  No tolerance, no id
exempted.  The fields themselves are held to the numpy references by the tolerance tests of test_gpu_quality*.py.

    a. the reports of jittered, polygonal and tangled meshes against the engine's fields; thresholds that are elements' own values
    b. graded blocks A and B (tests/test_quality_graded_blocks.py): placed ties in and across workgroups, thresholds on the tie value
    c. more than 256 workgroup records (81^3 cells)
    d. the trace's tile-ordered path, where tile order is not id order
    e. the constraint's twin of the face measures (qcFace against qFaceCore), by bits"""
import dataclasses
import functools
import math

import numpy as np
import pytest

from quality_fold_reference import (GEOMETRY_COUNTS, MOTION_COUNTS, QUALITY_COUNTS, SET_OF, SMALL, VSMALL, block_a, flatness_faces, fold_sum,
                                    groups_of, internal_faces, lowest_extreme, members, polygon_faces, same_bits, tied)
from test_quality_geometry_reference import GEOMETRY_DEFAULTS
from test_quality_motion_reference import MOTION_DEFAULTS
from test_quality_reference import DEFAULTS, tangled_block

pytestmark = pytest.mark.gpu

KINDS = {
    "quality": dict(report="mesh_quality", field="quality_field", sets="quality_sets", defaults=DEFAULTS, counts=QUALITY_COUNTS),
    "geometry": dict(report="mesh_quality_geometry", field="quality_geometry_field", sets="quality_geometry_sets", defaults=GEOMETRY_DEFAULTS,
                     counts=GEOMETRY_COUNTS),
    "motion": dict(report="mesh_quality_motion", field="quality_motion_field", sets="quality_motion_sets", defaults=MOTION_DEFAULTS,
                   counts=MOTION_COUNTS),
}
# kind -> (value, id or None, field, domain, min / max, the value of the empty case)
EXTREMES = {
    "quality": (("minVolume", "minVolumeCell", "cellVolume", None, "min", 0.0), ("maxVolume", None, "cellVolume", None, "max", 0.0),
                ("maxNonOrth", "maxNonOrthFace", "faceNonOrthogonality", "internal", "max", 0.0),
                ("maxSkewness", "maxSkewFace", "faceSkewness", None, "max", 0.0), ("maxOpenness", None, "cellOpenness", None, "max", 0.0),
                ("maxAspectRatio", None, "cellAspectRatio", None, "max", 0.0),
                ("minFaceArea", None, "_faceArea", None, "min", 0.0), ("maxFaceArea", None, "_faceArea", None, "max", 0.0)),
    "geometry": (("maxConcaveSin", "maxConcaveFace", "faceConcavity", "concave", "max", 0.0),
                 ("minFlatness", "minFlatnessFace", "faceFlatness", "flatness", "min", 1.0),
                 ("minFaceWeight", "minFaceWeightFace", "faceWeight", "internal", "min", 1.0),
                 ("minVolRatio", "minVolRatioFace", "faceVolumeRatio", "internal", "min", 1.0),
                 ("minDeterminant", "minDeterminantCell", "cellDeterminant", None, "min", 0.0)),
    "motion": (("minTetQuality", "minTetFace", "faceTetQuality", None, "min", 1.0), ("minBaseTetQuality", "minBaseTetFace", "faceBaseTetQuality", None, "min", 1.0),
               ("minTwist", "minTwistFace", "faceTwist", "polygon", "min", 1.0),
               ("minTriangleTwist", "minTriangleTwistFace", "faceTriangleTwist", "polygon", "min", 1.0)),
}
# kind -> (sum or average, field, domain, the value of the empty case or None for a plain sum)
SUMS = {
    "quality": (("totalVolume", "cellVolume", None, None), ("avgNonOrth", "faceNonOrthogonality", "internal", 0.0)),
    "geometry": (("avgFlatness", "faceFlatness", "flatness", 1.0), ("avgFaceWeight", "faceWeight", "internal", 1.0),
                 ("avgVolRatio", "faceVolumeRatio", "internal", 1.0), ("avgDeterminant", "cellDeterminant", None, 0.0)),
    "motion": (("avgTetQuality", "faceTetQuality", None, 1.0), ("avgTwist", "faceTwist", "polygon", 1.0),
               ("avgTriangleTwist", "faceTriangleTwist", "polygon", 1.0)),
}


def _engine(mesh, variant="com"):
    from smoothmesh_amd import SmoothEngine
    e = SmoothEngine(mesh)
    e.set_foam_variant(variant)
    return e


def _face_area(mesh, variant):
    """|S_f| of the engine's own area vectors (the report publishes no field of it): the loop's S_f, then the kernel's mag"""
    from smoothmesh_amd import default_params
    g = _engine(mesh, variant)
    g.set_params(default_params(g.mesh_stats()[0]))
    g.debug_propose()
    a = g.debug_field("faceAreas").reshape(-1, 3)
    g.close()
    return np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])


class Fields:
    """the engine's per-element fields of its current points, fetched once each; "_faceArea" where `area` is given"""

    def __init__(self, e, mesh, area=None):
        self.e, self.mesh, self.got = e, mesh, ({} if area is None else {"_faceArea": area})

    def __contains__(self, name):
        return not name.startswith("_") or name in self.got

    def __call__(self, kind, name):
        if name not in self.got:
            v = getattr(self.e, KINDS[kind]["field"])(name)
            v.setflags(write=False)
            self.got[name] = v
        return self.got[name]

    def domain(self, name):
        if name is None:
            return None
        if name == "internal":
            return internal_faces(self.mesh)
        if name == "polygon":
            return polygon_faces(self.mesh)
        if name == "concave":
            return self("geometry", "faceConcavity") > SMALL
        assert name == "flatness"
        return flatness_faces(self.mesh, self.got["_faceArea"]) if "_faceArea" in self.got else polygon_faces(self.mesh)


def _assert_counts(kind, got, F, thr, sets=None):
    """every count of the report `got` is its predicate on the field under the thresholds thr; with sets: each is flatnonzero of it"""
    for name, row in KINDS[kind]["counts"].items():
        field, dom, _, tname = row
        m = members(row, F(kind, field), F.domain(dom), thr[tname] if tname else None)
        assert got[name] == int(m.sum()), (kind, name, got[name], int(m.sum()), thr)
        if sets is not None:
            ids = sets[SET_OF[name]]
            assert ids.dtype == np.int32 and np.array_equal(ids, np.flatnonzero(m)), (kind, name, thr)


def _assert_report_of_fields(e, F, kinds=KINDS, label=""):
    """(a): values by bits, ids exactly, averages = fold_sum / denominator by bits, counts and sets at the default thresholds"""
    mesh = F.mesh
    for kind in kinds:
        got = dataclasses.asdict(getattr(e, KINDS[kind]["report"])())
        for value, idk, field, dom, how, empty in EXTREMES[kind]:
            if field not in F:
                continue
            v, i = lowest_extreme(F(kind, field), F.domain(dom), how, empty)
            assert same_bits(got[value], v), (label, value, got[value], v)
            if idk:
                assert got[idk] == i, (label, idk, got[idk], i, tied(F(kind, field), F.domain(dom), how)[:8])
        for name, field, dom, empty in SUMS[kind]:
            x, d = F(kind, field), F.domain(dom)
            s = fold_sum(x if d is None else np.where(d, x, 0.0))
            n = x.size if d is None else int(d.sum())
            want = s if empty is None else (s / n if n else empty)
            assert same_bits(got[name], want), (label, name, got[name], want, float(np.sum(x if d is None else x[d])) / max(n, 1))
        if kind == "quality":
            assert (got["nCells"], got["nFaces"], got["nInternalFaces"]) == (mesh.nCells, mesh.nFaces, mesh.nInternalFaces)
            if "_faceArea" in F:
                assert got["nZeroAreaFaces"] == int((F(kind, "_faceArea") <= VSMALL).sum())
        if kind == "geometry":
            assert got["nFlatnessFaces"] == int(F.domain("flatness").sum())
            if got["nConcaveFaces"]:
                assert got["maxConcaveAngle"] > 0.0
            else:
                assert (got["maxConcaveSin"], got["maxConcaveAngle"], got["maxConcaveFace"]) == (0.0, 0.0, -1)
        if kind == "motion":
            assert got["nTwistFaces"] == int(polygon_faces(mesh).sum())
        sets = getattr(e, KINDS[kind]["sets"])()
        _assert_counts(kind, got, F, KINDS[kind]["defaults"], sets)
        if kind == "quality":                                   # the sets without a published field: their size is the report's count
            assert sets["nonOrthoFaces"].size == got["nSevereNonOrth"] + got["nErrorNonOrth"]
            assert sets["wrongOrientedFaces"].size == got["nWrongOrientedFaces"] and sets["zeroAreaFaces"].size == got["nZeroAreaFaces"]
            for s in sets.values():
                assert np.all(np.diff(s) > 0)


def _own_value(v):
    """an element's own value well inside the sorted order: the distinct value next to the median that leaves at least three elements
    on each side; where the field has no such value (it is all but constant), its median"""
    s = np.sort(v)
    u = np.unique(s)
    ok = [x for x in u if (s < x).sum() >= 3 and (s > x).sum() >= 3]
    return float(min(ok, key=lambda x: abs(np.searchsorted(s, x) - s.size // 2))) if ok else float(s[s.size // 2])


def _assert_threshold_hit(e, F, kind, count, t, expect_tied=None, label=""):
    """the report and the sets at threshold t and at the next double on the side that flips the elements equal to t: the two counts
    differ by exactly the number of elements whose bits are t (so the threshold was hit), each count is the predicate on the field,
    each set is flatnonzero of it.  Returns the number of tied elements."""
    K = KINDS[kind]
    row = K["counts"][count]
    field, dom, pred, tname = row
    x, d = F(kind, field), F.domain(dom)
    strict = int(members(row, x, d, t).sum())
    up = bool(pred(np.array([0.0]), 1.0)[0])                     # a "<" predicate: the next double above t takes the ties in
    t2 = float(np.nextafter(t, math.inf if up else -math.inf))
    nTied = int(((x == t) if d is None else (x == t) & d).sum())
    assert nTied >= 1, (label, kind, count, t)
    if expect_tied is not None:
        assert nTied == expect_tied, (label, count, nTied, expect_tied)
    counts = []
    for thr in (t, t2):
        thrs = {**K["defaults"], tname: thr}
        got = dataclasses.asdict(getattr(e, K["report"])(**thrs))
        sets = getattr(e, K["sets"])(**thrs)
        _assert_counts(kind, got, F, thrs, sets)
        counts.append(got[count])
    assert counts[0] == strict and counts[1] - counts[0] == nTied, (label, kind, count, t, counts, nTied)
    return nTied


def _assert_thresholds_on_own_values(e, F, label=""):
    for kind, K in KINDS.items():
        for count, (field, dom, _, tname) in K["counts"].items():
            if tname is None:
                continue
            x, d = F(kind, field), F.domain(dom)
            v = x if d is None else x[d]
            if v.size == 0:
                continue
            t = _own_value(v)
            n = _assert_threshold_hit(e, F, kind, count, t, label=label)
            print(f"    {label} {count}: {tname} = {t!r} hit by {n}")


def _assert_midpoint_thresholds(e, F, label=""):
    """non-orthogonality and concavity take their threshold through a cosine / a sine: a midpoint between two adjacent field values"""
    Fi = F.mesh.nInternalFaces
    th = np.unique(F("quality", "faceNonOrthogonality")[:Fi])
    gaps = np.flatnonzero(np.diff(th) > 1e-9)                   # (a gap the cosine's rounding cannot close)
    if gaps.size:
        k = int(gaps[gaps.size // 2])
        t = 0.5 * (th[k] + th[k + 1])
        m = internal_faces(F.mesh) & (F("quality", "faceNonOrthogonality") > t)
        q = e.mesh_quality(nonOrthThreshold=t)
        assert q.nSevereNonOrth + q.nErrorNonOrth == int(m.sum()) and 0 < int(m.sum()) < Fi, (label, t)
        assert np.array_equal(e.quality_sets(nonOrthThreshold=t)["nonOrthoFaces"], np.flatnonzero(m)), (label, t)
    conc = F("geometry", "faceConcavity")
    s = np.unique(conc[conc > SMALL])
    gaps = np.flatnonzero(np.diff(s) > 1e-9)
    print(f"    {label}: {th.size} distinct non-orthogonality angles, {s.size} distinct concavities")
    if gaps.size:
        k = int(gaps[gaps.size // 2])
        mid = 0.5 * (s[k] + s[k + 1])
        t = math.degrees(math.asin(mid))
        m = conc > mid
        assert 0 < int(m.sum()) < int((conc > SMALL).sum())
        assert e.mesh_quality_geometry(concaveThreshold=t).nConcaveFaces == int(m.sum()), (label, t)
        assert np.array_equal(e.quality_geometry_sets(concaveThreshold=t)["concaveFaces"], np.flatnonzero(m)), (label, t)


# ---- a. a report is a function of the engine's own fields ------------------------------------------------------------------
def _mesh(name):
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import cavity_mesh
    from test_gpu_quality_geometry import bent_block
    return {"block756": lambda: hex_block(12, 9, 7, jitter=0.3), "block2184": lambda: hex_block(14, 13, 12, jitter=0.25),
            "cavity16": lambda: cavity_mesh(16, jitter=0.2, seed=3), "bent": bent_block, "tangled": tangled_block}[name]()


MESHES = ("block756", "block2184", "cavity16", "bent", "tangled")


@pytest.mark.parametrize("variant", ["com", "org"])
@pytest.mark.parametrize("name", MESHES)
def test_report_is_a_function_of_the_fields(name, variant):
    m = _mesh(name)
    e = _engine(m, variant)
    F = Fields(e, m, _face_area(m, variant))
    label = f"{name} {variant}"
    _assert_report_of_fields(e, F, label=label)
    _assert_thresholds_on_own_values(e, F, label)
    _assert_midpoint_thresholds(e, F, label)
    if name == "bent":                                          # the non-zero branches of the counts and the concave maximum
        g = e.mesh_quality_geometry()
        assert g.nConcaveFaces >= 1 and g.nWarpedFaces >= 1 and g.nLowVolRatioFaces >= 1 and e.mesh_quality().nNonPositiveVolume >= 1


# ---- b. placed ties and exact thresholds -------------------------------------------------------------------------------
EXACT_VALUES = {"quality": ("minVolume", "maxVolume", "totalVolume", "minFaceArea", "maxFaceArea", "maxNonOrth", "avgNonOrth", "maxSkewness",
                            "maxOpenness"),
                "geometry": ("minFaceWeight", "minVolRatio", "minFlatness"), "motion": ("minTwist", "minTriangleTwist")}
IDS = {"quality": ("minVolumeCell", "maxNonOrthFace", "maxSkewFace"),
       "geometry": ("maxConcaveFace", "minFlatnessFace", "minFaceWeightFace", "minVolRatioFace", "minDeterminantCell"),
       "motion": ("minTetFace", "minBaseTetFace", "minTwistFace", "minTriangleTwistFace")}


@pytest.mark.parametrize("variant", ["com", "org"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_graded_block_ties_and_exact_thresholds(name, variant):
    from test_quality_graded_blocks import graded_case
    m, ref = graded_case(name, variant)
    e = _engine(m, variant)
    F = Fields(e, m, _face_area(m, variant))
    label = f"block {name} {variant}"
    for kind in KINDS:
        got, rep = dataclasses.asdict(getattr(e, KINDS[kind]["report"])()), ref[kind][0]
        for k in IDS[kind]:                                     # exact ties on both sides: the reference's argmin is the lowest id
            assert got[k] == rep[k], (label, k, got[k], rep[k])
        for k in EXACT_VALUES[kind]:
            assert same_bits(got[k], rep[k]), (label, k, got[k], rep[k])
        for value, idk, field, dom, how, _ in EXTREMES[kind]:
            if idk:
                t = tied(F(kind, field), F.domain(dom), how)
                print(f"    {label} {value}: {got[value]!r} id {got[idk]}, tied on {t.size} in workgroups {groups_of(t)}")
    _assert_report_of_fields(e, F, label=label)               # every id is lowest_extreme of the engine's field, too
    q = e.mesh_quality()
    assert q.maxAspectRatio == 6.0 and q.minVolume == 2.0 ** -15
    # thresholds on the tie value itself
    nAR = int((ref["quality"][1]["cellAspectRatio"] == 6.0).sum())
    assert _assert_threshold_hit(e, F, "quality", "nHighAspectCells", 6.0, label=label) == nAR > 1
    assert _assert_threshold_hit(e, F, "geometry", "nLowWeightFaces", 0.25, expect_tied=216, label=label) == 216
    rmin = float(F("geometry", "faceVolumeRatio")[:m.nInternalFaces].min())
    assert _assert_threshold_hit(e, F, "geometry", "nLowVolRatioFaces", rmin, expect_tied=216, label=label) == 216
    assert e.mesh_quality_geometry(weightThreshold=0.25).nLowWeightFaces == 0 == e.mesh_quality(aspectThreshold=6.0).nHighAspectCells
    assert _assert_threshold_hit(e, F, "quality", "nSkewFaces", 0.0, expect_tied=m.nFaces, label=label) == m.nFaces
    assert e.mesh_quality(skewThreshold=0.0).nSkewFaces == 0 and e.quality_sets(skewThreshold=0.0)["skewFaces"].size == 0


# ---- c. more than 256 workgroup records ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(81, jitter=0.3)                               # 531 441 cells: the smallest cube over 256 * 2048; 783 face records
    e = _engine(m)
    yield e, m
    e.close()


def test_more_than_256_workgroup_records(big):
    e, m = big
    assert m.nCells > 256 * 2048 and m.nFaces > 3 * 256 * 2048
    _assert_report_of_fields(e, Fields(e, m), label="block 81^3")


# ---- d. the trace's tile-ordered path -------------------------------------------------------------------------------------
TRACE_ENV = [{"SMGPU_GEOM_T": "64"}, {"SMGPU_GEOM_T": "128"}, {"SMGPU_TILES": "0"}, {"SMGPU_QUALITY_TRACE_FUSED": "0"}]


def _trace_one(monkeypatch, m, env):
    """(record of one traced iteration, twin engine at the resulting points, residual)"""
    from test_gpu_quality_trace import _assert_record_is_report, _engine as loop_engine
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    a, b = loop_engine(m), loop_engine(m)
    a.set_quality_trace(1)
    n, res, _ = a.iterate(1, 0.0)
    assert n == 1
    (rec,) = a.quality_trace()
    b.set_points(a.get_points())
    _assert_record_is_report(rec, b.mesh_quality(), 1)
    return rec, b, float(res[0])


def _assert_record_ids(rec, F):
    still = 0
    for value, idk, field, dom, how, empty in EXTREMES["quality"]:
        if idk:
            v, i = lowest_extreme(F("quality", field), F.domain(dom), how, empty)
            assert getattr(rec, idk) == i and same_bits(getattr(rec, value), v), (idk, getattr(rec, idk), i)
            still += tied(F("quality", field), F.domain(dom), how).size > 1
    return still


@pytest.mark.parametrize("env", TRACE_ENV, ids=lambda d: "-".join(f"{k[6:]}{v}" for k, v in d.items()))
def test_trace_ids_on_graded_block(monkeypatch, env):
    m = block_a()
    rec, twin, _ = _trace_one(monkeypatch, m, env)
    still = _assert_record_ids(rec, Fields(twin, m))
    print(f"    block A after one iteration, {env}: {still} of 3 extremes with an id are still tied")


@pytest.mark.parametrize("env", TRACE_ENV, ids=lambda d: "-".join(f"{k[6:]}{v}" for k, v in d.items()))
def test_trace_ids_where_every_cell_ties(monkeypatch, env):
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(16, 12, 10, lengths=(1.0, 0.375, 0.625))     # binary spacing: the points do not move, every cell keeps the same bits
    rec, twin, res = _trace_one(monkeypatch, m, env)
    assert res == 0.0 and np.array_equal(twin.get_points(), m.points)
    F = Fields(twin, m)
    assert tied(F("quality", "cellVolume"), None, "min").size == m.nCells
    assert _assert_record_ids(rec, F) == 3
    assert (rec.minVolumeCell, rec.maxNonOrthFace, rec.maxSkewFace) == (0, 0, 0)


# ---- e. the constraint's twin of the face measures -------------------------------------------------------------------------
@pytest.mark.parametrize("tiles", ["1", "0"])
@pytest.mark.parametrize("variant", ["com", "org"])
@pytest.mark.parametrize("name", ["block2184", "cavity16"])
def test_constraint_judges_by_the_reports_own_skewness(monkeypatch, name, variant, tiles):
    from test_gpu_quality_trace import _engine as loop_engine
    monkeypatch.setenv("SMGPU_TILES", tiles)
    m = _mesh(name)
    e = loop_engine(m, variant)
    s = e.quality_field("faceSkewness")
    Fi = m.nInternalFaces
    for lo, hi, limits in ((0, Fi, lambda t: (180.0, t, 0.0)), (Fi, m.nFaces, lambda t: (180.0, 0.0, t))):
        part = s[lo:hi]
        t = _own_value(part)
        assert t > 0.0 and (part < t).sum() >= 3 and (part > t).sum() >= 3
        nTied = int((part == t).sum())
        e.set_quality_constraint(*limits(t), 2)
        assert e.quality_constraint_state().nExemptFaces == int((part > t).sum()), (name, variant, lo, t)
        e.set_quality_constraint(*limits(float(np.nextafter(t, 0.0))), 2)
        assert e.quality_constraint_state().nExemptFaces == int((part > t).sum()) + nTied, (name, variant, lo, t)
        e.clear_quality_constraint()
