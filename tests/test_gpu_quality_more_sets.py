"""smgpu_quality_geometry_sets / smgpu_quality_motion_sets on the MI355X (DESIGN.md "Mesh quality", 10.9): the engine's sets against
the numpy restatements (tests/test_quality_more_sets_reference.py), sizes against the reports' counts, order, repeatability,
compaction across scan tiles and at workgroup boundaries, the interface's refusals, freedom from side effects, and the
-writeSets of the two front-ends with -allGeometry / -meshQuality.

No tolerance anywhere: membership is exact where no reference value lies near its threshold, which the well-posedness
assertions establish on the reference alone."""
import ctypes as C
import dataclasses
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_quality_geometry as TG
import test_gpu_quality_geometry_motion_decomposed as TD
import test_gpu_quality_motion as TM
from test_gpu_quality_sets import _split_between
from test_quality_geometry_reference import GEOMETRY_DEFAULTS, geometry_reference_of, quality_geometry_reference
from test_quality_more_sets_reference import (GEOMETRY_NAMES, MOTION_NAMES, assert_sizes_are_counts, geometry_sets_of_fields,
                                              motion_sets_of_fields)
from test_quality_motion_reference import quality_motion_reference
from test_quality_reference import cell_faces
from test_quality_sets_reference import NAMES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "smoothmesh_amd", "bin", "smoothMesh")
EVERY_G = dict(flatnessThreshold=2.0, weightThreshold=1.0, volRatioThreshold=2.0, determinantThreshold=1e30)
EVERY_M = dict(tetThreshold=2.0, twistThreshold=2.0, triangleTwistThreshold=2.0)


def _engine(mesh, variant="com"):
    from smoothmesh_amd import SmoothEngine
    e = SmoothEngine(mesh)
    e.set_foam_variant(variant)
    return e


def _tables():
    from smoothmesh_amd.quality import QUALITY_GEOMETRY_SETS, QUALITY_MOTION_SETS
    return QUALITY_GEOMETRY_SETS, QUALITY_MOTION_SETS


def _assert_sets(got, want, names):
    assert list(got) == list(names)
    for k in names:
        assert got[k].dtype == np.int32, k
        assert np.all(np.diff(got[k]) > 0), k                       # strictly ascending
        assert np.array_equal(got[k], want[k]), (k, len(got[k]), len(want[k]))


def _check_geometry(e, rep, want, **thr):
    """the engine's sets equal the reference's, ascending int32; sizes equal the engine's and the reference's report counts"""
    got = e.quality_geometry_sets(**thr)
    _assert_sets(got, want, GEOMETRY_NAMES)
    assert_sizes_are_counts(got, dataclasses.asdict(e.mesh_quality_geometry(**thr)), _tables()[0])
    assert_sizes_are_counts(got, rep, _tables()[0])
    return got


def _check_motion(e, rep, want, **thr):
    got = e.quality_motion_sets(**thr)
    _assert_sets(got, want, MOTION_NAMES)
    assert_sizes_are_counts(got, dataclasses.asdict(e.mesh_quality_motion(**thr)), _tables()[1])
    assert_sizes_are_counts(got, rep, _tables()[1])
    return got


# ---- parity with the numpy restatements ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _squashed_bent(variant):
    """test_gpu_quality_geometry's bent block with z scaled by 0.05: flat cells, so that under-determined cells join the other
    four findings at the default thresholds (on the bent block itself the reference's smallest determinant is 0.114, far above
    0.001: no cell is a member there) -> (mesh, reference report, reference fields), computed once and left unchanged"""
    from oracle import oracle_ffi
    oracle_ffi.build()
    m = TG.bent_block()
    m.points = m.points * np.array([1.0, 1.0, 0.05])
    rep, f = geometry_reference_of(oracle_ffi, m, variant)
    for v in f.values():
        v.setflags(write=False)
    return m, rep, f


def _assert_thresholds_well_posed(m, f):
    """TG._assert_well_posed without its distinct-minimum conditions, which concern the report's ids and not set membership"""
    d, Fi = GEOMETRY_DEFAULTS, m.nInternalFaces
    s, side = f["_cornerSin"], f["_cornerSide"]
    sinT = math.sin(math.radians(d["concaveThreshold"]))
    assert np.min(np.abs(s - sinT)) > 1e-9 and np.min(np.abs(side[s >= sinT])) > 1e-9
    assert np.min(np.abs(f["faceFlatness"][f["_summed"]] - d["flatnessThreshold"])) > 1e-9
    assert np.min(np.abs(f["faceWeight"][:Fi] - d["weightThreshold"])) > 1e-9
    assert np.min(np.abs(f["faceVolumeRatio"][:Fi] - d["volRatioThreshold"])) > 1e-9
    assert np.min(np.abs(f["cellDeterminant"] - d["determinantThreshold"])) > 1e-9


@pytest.mark.parametrize("variant", ["com", "org"])
@pytest.mark.parametrize("name", TG.PARITY + ("bent squashed",))
def test_geometry_sets_parity(name, variant):
    """On `bent` the four face sets are non-empty; underdeterminedCells is empty there in the reference itself (smallest
    determinant 0.114 against the threshold 0.001), so the mesh with all five sets non-empty at the default thresholds is the
    squashed one."""
    if name == "bent squashed":
        m, rep, f = _squashed_bent(variant)
        _assert_thresholds_well_posed(m, f)
    else:
        m, rep, f = TG._case(name, variant)
        TG._assert_well_posed(m, rep, f)
    got = _check_geometry(_engine(m, variant), rep, geometry_sets_of_fields(m, f))
    if name.startswith("bent"):
        for k in GEOMETRY_NAMES[:4] if name == "bent" else GEOMETRY_NAMES:
            assert len(got[k]) > 0, k


@pytest.mark.parametrize("variant", ["com", "org"])
@pytest.mark.parametrize("name", TM.PARITY)
def test_motion_sets_parity(name, variant):
    m, rep, f = TM._case(name, variant)
    TM._assert_well_posed(m, rep, f)
    _check_motion(_engine(m, variant), rep, motion_sets_of_fields(f))


@pytest.mark.parametrize("variant", ["com", "org"])
@pytest.mark.parametrize("kind", ["grid", "bfs", "random", "cavity"])
def test_all_nine_sets_at_the_decomposed_tests_thresholds(kind, variant):
    """the undecomposed meshes of the decomposed tests under their thresholds, where every count but (on the hex block) the
    concave one is positive; the polyhedral mesh has concave faces too"""
    m, _, grep, gf, mrep, mf = TD._refs(kind, variant)
    TD._assert_well_posed(m, grep, gf, mf)
    e = _engine(m, variant)
    g = _check_geometry(e, grep, geometry_sets_of_fields(m, gf, **TD.G_THR), **TD.G_THR)
    t = _check_motion(e, mrep, motion_sets_of_fields(mf, **TD.M_THR), **TD.M_THR)
    for k in GEOMETRY_NAMES[1:] + MOTION_NAMES:
        assert len({**g, **t}[k]) > 0, k
    if kind == "cavity":
        assert len(g["concaveFaces"]) > 0                                # all nine


# ---- compaction ---------------------------------------------------------------------------------------------------
def test_every_eligible_element_in_a_set_across_scan_tiles():
    """thresholds that take every eligible element: the 4 x 328 face-workgroup counts span two 1024-entry tiles of the scan"""
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(61, 60, 60, jitter=0.2)
    assert (m.nCells, m.nFaces, m.nInternalFaces) == (219600, 669720, 647880)
    assert m.nCells % 256 and m.nFaces % 256 and m.nInternalFaces % 256
    assert 1024 < 4 * -(-m.nFaces // 2048) <= 2048
    e = _engine(m)
    g = e.quality_geometry_sets(**EVERY_G)
    t = e.quality_motion_sets(**EVERY_M)
    allF, intF = np.arange(m.nFaces, dtype=np.int32), np.arange(m.nInternalFaces, dtype=np.int32)
    assert np.array_equal(g["warpedFaces"], allF)
    assert np.array_equal(g["lowWeightFaces"], intF) and np.array_equal(g["lowVolRatioFaces"], intF)
    assert np.array_equal(g["underdeterminedCells"], np.arange(m.nCells, dtype=np.int32))
    for k in MOTION_NAMES:
        assert np.array_equal(t[k], allF), k
    assert_sizes_are_counts(g, dataclasses.asdict(e.mesh_quality_geometry(**EVERY_G)), _tables()[0])
    assert_sizes_are_counts(t, dataclasses.asdict(e.mesh_quality_motion(**EVERY_M)), _tables()[1])
    assert_sizes_are_counts(e.quality_geometry_sets(), dataclasses.asdict(e.mesh_quality_geometry()), _tables()[0])
    assert_sizes_are_counts(e.quality_motion_sets(), dataclasses.asdict(e.mesh_quality_motion()), _tables()[1])


def _split(v):
    """_split_between's threshold next to the median; where the values from the median up are all alike (the planar boundary
    faces of a small block: flatness and twist 1), the same search from the median down"""
    try:
        return _split_between(v)
    except AssertionError:
        return -_split_between(-v)


@pytest.mark.parametrize("dims", [(3, 2, 2), (7, 5, 3), (17, 11, 13)])
def test_element_counts_off_the_block_sizes(dims):
    """nFaces / nCells no multiples of 256 or 2048, thresholds that take about half of every set's eligible elements; the
    references take the engine's own published geometry (bit-identical to the oracle's: tests/test_gpu_parity.py)"""
    from smoothmesh_amd import default_params
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(*dims, jitter=0.4, seed=sum(dims))
    assert m.nFaces % 256 and m.nCells % 256
    g = _engine(m)
    g.set_params(default_params(g.mesh_stats()[0]))
    g.debug_propose()
    geo = tuple(g.debug_field(k).reshape(-1, 3) for k in ("faceCentres", "faceAreas", "cellCentres"))
    cf = cell_faces(m)
    gf = quality_geometry_reference(m, *geo, *cf)[1]
    mf = quality_motion_reference(m, *geo, *cf)[1]
    Fi, s = m.nInternalFaces, gf["_summed"]
    assert np.array_equal(s, mf["_summed"]) and s.all()
    eligible = dict(flatnessThreshold=gf["faceFlatness"][s], weightThreshold=gf["faceWeight"][:Fi], volRatioThreshold=gf["faceVolumeRatio"][:Fi],
                    determinantThreshold=gf["cellDeterminant"], tetThreshold=mf["faceTetQuality"], twistThreshold=mf["faceTwist"][s],
                    triangleTwistThreshold=mf["faceTriangleTwist"][s])
    thr = {k: _split(v) for k, v in eligible.items()}
    eligible["baseTet"] = mf["faceBaseTetQuality"]                    # (shares tetThreshold)
    for k, v in eligible.items():                                     # well posed: nothing within 1e-9 of its threshold
        assert np.min(np.abs(v - thr["tetThreshold" if k == "baseTet" else k])) > 1e-9, k
    sinT = np.sin(np.radians(10.0))                                   # concaveThreshold stays at its default
    assert np.min(np.abs(gf["_cornerSin"] - sinT)) > 1e-9
    assert not (gf["_cornerSin"] >= sinT).any() or np.min(np.abs(gf["_cornerSide"][gf["_cornerSin"] >= sinT])) > 1e-9
    gt = {k: thr[k] for k in ("flatnessThreshold", "weightThreshold", "volRatioThreshold", "determinantThreshold")}
    mt = {k: thr[k] for k in ("tetThreshold", "twistThreshold", "triangleTwistThreshold")}
    grep, gf2 = quality_geometry_reference(m, *geo, *cf, **gt)
    mrep, mf2 = quality_motion_reference(m, *geo, *cf, **mt)
    e = _engine(m)
    got_g = _check_geometry(e, grep, geometry_sets_of_fields(m, gf2, **gt), **gt)
    got_m = _check_motion(e, mrep, motion_sets_of_fields(mf2, **mt), **mt)
    for k, n in (("warpedFaces", m.nFaces), ("lowWeightFaces", Fi), ("lowVolRatioFaces", Fi), ("underdeterminedCells", m.nCells)):
        assert n // 3 <= len(got_g[k]) <= n - n // 3 + 1, (k, len(got_g[k]), n)
    for k in ("lowQualityTetFaces", "twistedFaces", "lowTriangleTwistFaces"):
        assert m.nFaces // 3 <= len(got_m[k]) <= m.nFaces - m.nFaces // 3 + 1, (k, len(got_m[k]))


# ---- the interface ----------------------------------------------------------------------------------------------------
def _raw(e, kind):
    from smoothmesh_amd import _ffi
    if kind == "geometry":
        thr = TD.G_THR
        return e._lib.smgpu_quality_geometry_sets, _ffi.QualityGeometryParams(*(thr[n] for n, _ in _ffi.QualityGeometryParams._fields_)), 5
    thr = TD.M_THR
    return e._lib.smgpu_quality_motion_sets, _ffi.QualityMotionParams(*(thr[n] for n, _ in _ffi.QualityMotionParams._fields_)), 4


@pytest.mark.parametrize("kind", ["geometry", "motion"])
def test_small_cap_counts_only_and_null_counts(kind):
    from smoothmesh_amd import SmgpuError, _ffi
    from smoothmesh_amd.meshgen import hex_block
    e = _engine(hex_block(9, 8, 7, jitter=0.3, seed=4))
    want = e.quality_geometry_sets(**TD.G_THR) if kind == "geometry" else e.quality_motion_sets(**TD.M_THR)
    names = GEOMETRY_NAMES if kind == "geometry" else MOTION_NAMES
    total = sum(len(v) for v in want.values())
    assert total > 1
    call, p, n = _raw(e, kind)
    counts = (C.c_int64 * n)()
    ids = np.full(total, -7, np.int32)
    rc = call(e._h, C.byref(p), counts, ids.ctypes.data_as(_ffi.c_i32p), total - 1)
    assert rc != 0 and "ids holds" in e._lib.smgpu_last_error().decode()
    assert list(counts) == [len(want[k]) for k in names]
    assert np.all(ids == -7)
    counts2 = (C.c_int64 * n)()
    assert call(e._h, C.byref(p), counts2, None, 0) == 0                               # counts only
    assert list(counts2) == list(counts)
    assert call(e._h, C.byref(p), counts2, ids.ctypes.data_as(_ffi.c_i32p), total) == 0
    assert np.array_equal(ids, np.concatenate([want[k] for k in names]))
    with pytest.raises(SmgpuError, match="null argument"):
        e._check(call(e._h, C.byref(p), None, None, 0))


def test_sets_leave_the_loop_untouched_and_repeat():
    from smoothmesh_amd import default_params
    from smoothmesh_amd.polymesh import cavity_mesh
    m = cavity_mesh(16, jitter=0.2, seed=3)
    runs = []
    for with_sets in (False, True):
        e = _engine(m)
        e.set_params(default_params(e.mesh_stats()[0]))
        if with_sets:
            n1, r1, f1 = e.iterate(5, 0.0)
            walk = e.debug_walk_mode()
            for call, thr in ((e.quality_geometry_sets, TD.G_THR), (e.quality_motion_sets, TD.M_THR)):
                a, b = call(**thr), call(**thr)
                assert all(a[k].tobytes() == b[k].tobytes() for k in a)            # two calls: bitwise equal
                assert sum(len(v) for v in a.values()) > 0
            assert e.debug_walk_mode() == walk
            n2, r2, f2 = e.iterate(5, 0.0)
            n, res, frz = n1 + n2, np.concatenate([r1, r2]), np.concatenate([f1, f2])
        else:
            n, res, frz = e.iterate(10, 0.0)
        runs.append((n, res, frz, e.get_points(), e.near_ties(), e.debug_walk_mode()))
    (na, ra, fa_, pa, ta, wa), (nb, rb, fb, pb, tb, wb) = runs
    assert na == nb == 10
    assert ra.tobytes() == rb.tobytes() and np.array_equal(fa_, fb)
    assert pa.tobytes() == pb.tobytes()
    assert ta == tb and wa == wb


def test_halo_engine_refuses_the_serial_calls():
    import socket
    import torch.distributed as dist
    from smoothmesh_amd import SmgpuError
    from smoothmesh_amd.halo import DistributedSmoother
    from smoothmesh_amd.meshgen import hex_subdomain
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        ds = DistributedSmoother(hex_subdomain((8, 7, 6), (1, 1, 1), 0, jitter=0.3, seed=5), device=0)
        with pytest.raises(SmgpuError, match="halo"):
            ds.engine.quality_geometry_sets()
        with pytest.raises(SmgpuError, match="halo"):
            ds.engine.quality_motion_sets()
        g, t = ds.quality_geometry_sets(**TD.G_THR), ds.quality_motion_sets(**TD.M_THR)   # the coupled form works on the same engine
        assert list(g) == list(GEOMETRY_NAMES) and list(t) == list(MOTION_NAMES)
        assert sum(len(v) for v in g.values()) > 0 and sum(len(v) for v in t.values()) > 0
    finally:
        dist.destroy_process_group()


# ---- the front-ends -----------------------------------------------------------------------------------------------------
def _run(case, opts):
    r = subprocess.run([BIN, "-case", str(case)] + opts, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def _flat_block():
    from smoothmesh_amd.meshgen import hex_block
    return hex_block(12, 10, 3, lengths=(1.0, 1.0, 2e-5), jitter=0.2, seed=6)    # flat: cell determinants far below 0.001


def _expected(mesh):
    """(the engine's sets of all three tables, the names of the non-empty ones in table order, their "<<Writing" lines)"""
    from smoothmesh_amd.quality import QUALITY_SETS
    e = _engine(mesh)
    want = {**e.quality_sets(), **e.quality_geometry_sets(), **e.quality_motion_sets()}
    table = QUALITY_SETS + _tables()[0] + _tables()[1]
    assert list(want) == [n for n, *_ in table]
    names = [n for n, *_ in table if len(want[n])]
    return want, names, [f"    <<Writing {len(want[n])} {w} to set {n}" for n, _, _, w in table if len(want[n])]


def _assert_flat(mesh):
    """on the numpy reference: the flat block's cell determinants sit far below the default threshold"""
    from oracle import oracle_ffi
    from test_quality_geometry_reference import geometry_reference_of
    oracle_ffi.build()
    det = geometry_reference_of(oracle_ffi, mesh)[1]["cellDeterminant"]
    assert det.max() < 1e-6, det.max()


def test_cli_write_sets_with_all_geometry_and_mesh_quality(tmp_path):
    from smoothmesh_amd.polymesh import read_label_list, read_polymesh, write_case
    m = _flat_block()
    for c in ("a", "b"):
        write_case(str(tmp_path / c), m, binary=True, writeFormat="binary")
    opts = ["-centroidalIters", "8", "-relTol", "0", "-checkQuality", "true", "-writeSets", "true"]
    out = _run(tmp_path / "a", opts + ["-allGeometry", "true", "-meshQuality", "true"]).stdout
    sets_dir = tmp_path / "a" / "8" / "polyMesh" / "sets"
    w = read_polymesh(str(tmp_path / "a" / "constant" / "polyMesh"), str(tmp_path / "a" / "8" / "polyMesh"))
    _assert_flat(w)
    want, names, wl = _expected(w)
    assert len(want["underdeterminedCells"]) == w.nCells                 # a new set is non-empty at the default thresholds
    assert sorted(os.listdir(sets_dir)) == sorted(names)
    for k in names:
        assert np.array_equal(read_label_list(str(sets_dir / k)), want[k]), k
    lines = out.splitlines()
    i = lines.index("Mesh quality (final mesh):")
    assert [x for x in lines[:i] if "<<Writing" in x] == []
    assert [x for x in lines[i:] if "<<Writing" in x] == wl              # the seven's, then geometry, then motion
    j = lines.index(wl[0])
    assert lines[j - 1] == "" and lines[j:j + len(wl)] == wl             # one run of lines after the block's blank line
    # the same run without the two options writes and prints the seven only
    out = _run(tmp_path / "b", opts).stdout
    seven = [n for n in names if n in NAMES]
    assert sorted(os.listdir(tmp_path / "b" / "8" / "polyMesh" / "sets")) == sorted(seven)
    assert [x for x in out.splitlines() if "<<Writing" in x] == [x for x in wl if x.rsplit(" ", 1)[1] in NAMES]


def test_check_quality_write_sets_with_all_geometry_and_mesh_quality(tmp_path):
    from smoothmesh_amd.polymesh import read_label_list, write_case
    m = _flat_block()
    _assert_flat(m)
    for c in ("a", "b"):
        write_case(str(tmp_path / c), m, binary=True, writeFormat="binary")
    tool = lambda *a: subprocess.run([sys.executable, "-m", "smoothmesh_amd.check_quality", *a], capture_output=True, text=True,  # noqa: E731
                                     cwd=ROOT, timeout=300)
    want, names, wl = _expected(m)
    assert len(want["underdeterminedCells"]) == m.nCells
    r = tool("-case", str(tmp_path / "a"), "-writeSets", "-allGeometry", "-meshQuality")
    assert r.returncode == 0, r.stderr[-3000:]
    d = tmp_path / "a" / "constant" / "polyMesh" / "sets"
    assert sorted(os.listdir(d)) == sorted(names)
    for k in names:
        assert np.array_equal(read_label_list(str(d / k)), want[k]), k
    lines = r.stdout.splitlines()
    assert [x for x in lines if "<<Writing" in x] == wl
    assert lines[0] == "Mesh quality (mesh):" and lines[lines.index(wl[0]) - 1] == ""
    r = tool("-case", str(tmp_path / "b"), "-writeSets")
    assert r.returncode == 0, r.stderr[-3000:]
    assert sorted(os.listdir(tmp_path / "b" / "constant" / "polyMesh" / "sets")) == sorted(n for n in names if n in NAMES)
    assert [x for x in r.stdout.splitlines() if "<<Writing" in x] == [x for x in wl if x.rsplit(" ", 1)[1] in NAMES]
