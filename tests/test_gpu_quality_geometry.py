"""The checks `checkMesh -allGeometry` adds, on the GPU (include/smgpu.h smgpu_mesh_quality_geometry / smgpu_quality_geometry_field,
csrc/kernels_quality_geom.hpp) against the numpy restatement of their definitions (tests/test_quality_geometry_reference.py), their
freedom from side effects, their repeatability, the refusal on a halo engine and the `-allGeometry` lines of the front-ends.

Tolerances (as tests/test_gpu_quality.py): both sides take the same inputs bit for bit and evaluate the same IEEE operations; only the
order of the sums differs (the area of a face's triangles, the cell volume, the determinant's tensor, the report's averages: a few
ulp of their largest term).  Counts and ids are exact (the meshes are checked to hold no element near a threshold and no second
element near a reported minimum), report values 1e-12 relative, fields 1e-13 relative to max(|ref|, 1).  The determinant's tensor
entries are O(1) (at most the face count of a cell), so cellDeterminant holds to 1e-12 absolute.  maxConcaveAngle = asin(s): the
engine's smacos is within 1.5 ulp, and d asin / ds = 1 / sqrt(1 - s^2) <= 7.1 for s <= 0.99, which the test asserts on its meshes:
1e-10 degrees covers the 1e-12 of s a hundred times over."""
import dataclasses
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from test_quality_geometry_reference import (COUNTS, GEOMETRY_DEFAULTS, cube27, cube27_determinants, dented_slab, geometry_reference_of,
                                             saddle_cell, split_pair)
from test_quality_reference import tangled_block

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "smoothmesh_amd", "bin", "smoothMesh")
FIELDS = ("faceConcavity", "faceFlatness", "faceWeight", "faceVolumeRatio", "cellDeterminant")
EXACT = COUNTS + ("nFlatnessFaces", "maxConcaveFace", "minFlatnessFace", "minFaceWeightFace", "minVolRatioFace", "minDeterminantCell")
VALUES = ("maxConcaveSin", "minFlatness", "avgFlatness", "minFaceWeight", "avgFaceWeight", "minVolRatio", "avgVolRatio")


def _engine(mesh, variant="com"):
    from smoothmesh_amd import SmoothEngine
    e = SmoothEngine(mesh)
    e.set_foam_variant(variant)
    return e


def bent_block():
    """a jittered block with a few points moved by hand, so that every kind of finding is there: an interior point pushed across
    its cell (tangled cells: concave and warped faces, volume ratios <= 0), and a second one moved close to its x-neighbour (a thin
    cell: a low weight)"""
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(9, 8, 7, jitter=0.2, seed=21)
    m.points = m.points.copy()
    inner = m.find_internal_points()

    def nearest(x, y, z):
        p = int(np.argmin(np.abs(m.points - np.array([x, y, z])).sum(axis=1) + np.where(inner, 0.0, 10.0)))
        assert inner[p]
        return p
    m.points[nearest(3 / 9, 3 / 8, 3 / 7)] += np.array([0.17, 0.19, 0.2])
    p = nearest(6 / 9, 5 / 8, 2 / 7)
    q = nearest(7 / 9, 5 / 8, 2 / 7)
    m.points[p] = m.points[q] - np.array([0.004, 0.001, 0.002])
    return m


def _mesh(name):
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import cavity_mesh
    if name == "block756":
        return hex_block(12, 9, 7, jitter=0.3)           # under one 2048-element workgroup of cells, faces over one
    if name == "block2184":
        return hex_block(14, 13, 12, jitter=0.25)        # one full workgroup of cells plus a ragged tail, three of faces
    if name == "cavity54":
        return cavity_mesh(54, jitter=0.2, seed=9)       # polygons with hanging nodes, cells with other than six faces
    assert name == "bent"
    return bent_block()


PARITY = ("block756", "block2184", "cavity54", "bent")


@functools.lru_cache(maxsize=None)
def _case(name, variant):
    """(mesh, reference report, reference fields), computed once and left unchanged"""
    from oracle import oracle_ffi
    oracle_ffi.build()
    m = _mesh(name)
    rep, f = geometry_reference_of(oracle_ffi, m, variant)
    for v in f.values():
        v.setflags(write=False)
    return m, rep, f


def _assert_well_posed(m, rep, f):
    """on the reference alone: nothing within 1e-9 of a threshold, of the concavity tests' two limits, or of a reported minimum"""
    d = GEOMETRY_DEFAULTS
    Fi = m.nInternalFaces
    s, side = f["_cornerSin"], f["_cornerSide"]
    sinT = math.sin(math.radians(d["concaveThreshold"]))
    assert np.min(np.abs(s - sinT)) > 1e-9
    assert np.min(np.abs(side[s >= sinT])) > 1e-9
    flat = f["faceFlatness"][f["_summed"]]
    assert np.min(np.abs(flat - d["flatnessThreshold"])) > 1e-9
    assert np.min(np.abs(f["faceWeight"][:Fi] - d["weightThreshold"])) > 1e-9
    assert np.min(np.abs(f["faceVolumeRatio"][:Fi] - d["volRatioThreshold"])) > 1e-9
    assert np.min(np.abs(f["cellDeterminant"] - d["determinantThreshold"])) > 1e-9
    for v in (flat, f["faceWeight"][:Fi], f["faceVolumeRatio"][:Fi], f["cellDeterminant"]):
        v = np.sort(v)
        assert v[1] - v[0] > 1e-9, v[:2]
    conc = np.sort(f["faceConcavity"][f["faceConcavity"] > 0.0])
    if conc.size > 1:
        assert conc[-1] - conc[-2] > 1e-9
    assert rep["maxConcaveSin"] <= 0.99                        # the condition number the angle's tolerance rests on


def _assert_report(q, rep, tied=(), engine=None, mesh=None):
    """tied: ids of minima that several elements share within rounding (the reference's id is a matter of the last bit): held to the
    lowest id among the elements that share the extreme of the engine's own field"""
    from quality_fold_reference import engine_lowest_id
    got = dataclasses.asdict(q)
    assert sorted(got) == sorted(rep)
    for k in sorted(got):
        print(f"    {k}: engine {got[k]!r} reference {rep[k]!r}")
    for k in EXACT:
        if k in tied:
            assert got[k] == engine_lowest_id(engine, mesh, k), (k, got[k])
            continue
        assert got[k] == rep[k], (k, got[k], rep[k])
    for k in VALUES:
        assert abs(got[k] - rep[k]) <= 1e-12 * abs(rep[k]), (k, got[k], rep[k])
    for k in ("minDeterminant", "avgDeterminant"):
        assert abs(got[k] - rep[k]) <= 1e-12, (k, got[k], rep[k])
    assert abs(got["maxConcaveAngle"] - rep["maxConcaveAngle"]) <= 1e-10, (got["maxConcaveAngle"], rep["maxConcaveAngle"])


def _assert_fields(e, f):
    for name in FIELDS:
        g, r = e.quality_geometry_field(name), f[name]
        assert g.shape == r.shape, name
        err = float(np.max(np.abs(g - r))) if name == "cellDeterminant" else float(np.max(np.abs(g - r) / np.maximum(np.abs(r), 1.0)))
        print(f"    {name}: max error {err:.3e}")
        assert err <= (1e-12 if name == "cellDeterminant" else 1e-13), (name, err)


# ---- known answers -------------------------------------------------------------------------------------------------
def test_uniform_cube(oracle_lib):
    m = cube27()
    rep, f = geometry_reference_of(oracle_lib, m)
    e = _engine(m)
    q = e.mesh_quality_geometry()
    cc = np.array([m.points[np.unique(np.concatenate([m.facePoints[m.faceOffsets[k]:m.faceOffsets[k + 1]] for k in range(m.nFaces)
                                                      if m.owner[k] == c or (k < m.nInternalFaces and m.neighbour[k] == c)]))].mean(axis=0)
                   for c in range(m.nCells)])
    assert np.max(np.abs(e.quality_geometry_field("cellDeterminant") - cube27_determinants(cc))) <= 1e-12
    assert abs(q.minDeterminant - 0.125) <= 1e-12 and abs(q.avgDeterminant - (1 + 6 * 0.5 + 12 * 0.25 + 8 * 0.125) / 27) <= 1e-12
    assert abs(q.minFaceWeight - 0.5) <= 1e-12 and abs(q.avgFaceWeight - 0.5) <= 1e-12
    assert abs(q.minVolRatio - 1.0) <= 1e-12 and abs(q.avgVolRatio - 1.0) <= 1e-12
    assert abs(q.minFlatness - 1.0) <= 1e-12 and abs(q.avgFlatness - 1.0) <= 1e-12 and q.nFlatnessFaces == m.nFaces
    assert (q.nConcaveFaces, q.maxConcaveSin, q.maxConcaveAngle, q.maxConcaveFace) == (0, 0.0, 0.0, -1)
    for k in COUNTS:
        assert getattr(q, k) == 0 == rep[k], k
    from quality_fold_reference import engine_lowest_id
    for k in ("minFlatnessFace", "minFaceWeightFace", "minVolRatioFace", "minDeterminantCell"):   # equal values within rounding: the lowest id
        assert getattr(q, k) == engine_lowest_id(e, m, k), k
    _assert_fields(e, f)


@pytest.mark.parametrize("a", [0.5, 0.05])
def test_split_pair(oracle_lib, a):
    m = split_pair(a)
    rep, f = geometry_reference_of(oracle_lib, m)
    e = _engine(m)
    q = e.mesh_quality_geometry()
    assert abs(q.minFaceWeight - min(a, 2 - a) / 2) <= 1e-12 and abs(q.avgFaceWeight - min(a, 2 - a) / 2) <= 1e-12
    assert abs(q.minVolRatio - min(a, 2 - a) / max(a, 2 - a)) <= 1e-12
    assert q.nLowWeightFaces == (1 if a == 0.05 else 0) and q.nLowVolRatioFaces == 0
    assert q.nUnderdeterminedCells == 2 and q.minDeterminant <= 1e-30
    _assert_report(q, rep, tied=("minFlatnessFace",), engine=e, mesh=m)           # eleven planar faces: flatness 1 within rounding
    _assert_fields(e, f)
    # thresholds are the caller's: a weight of 0.25 is low under 0.3, a ratio of 1/3 under 0.5
    if a == 0.5:
        t = e.mesh_quality_geometry(weightThreshold=0.3, volRatioThreshold=0.5, determinantThreshold=0.0)
        assert (t.nLowWeightFaces, t.nLowVolRatioFaces, t.nUnderdeterminedCells) == (1, 1, 0)


@pytest.mark.parametrize("variant", ["com", "org"])
@pytest.mark.parametrize("h", [0.5, 0.1])
def test_saddle_face(oracle_lib, variant, h):
    m, top = saddle_cell(h)
    rep, f = geometry_reference_of(oracle_lib, m, variant)
    e = _engine(m, variant)
    q = e.mesh_quality_geometry()
    assert abs(e.quality_geometry_field("faceFlatness")[top] - 1.0 / math.sqrt(1.0 + 4.0 * h * h)) <= 1e-12
    assert q.nWarpedFaces == (1 if h == 0.5 else 0) == rep["nWarpedFaces"]
    assert q.minFlatnessFace == top and abs(q.minFlatness - 1.0 / math.sqrt(1.0 + 4.0 * h * h)) <= 1e-12
    # no internal face: weight and ratio are the fields' 1, no id
    assert (q.minFaceWeight, q.avgFaceWeight, q.minFaceWeightFace, q.minVolRatio, q.minVolRatioFace) == (1.0, 1.0, -1, 1.0, -1)
    assert (q.minDeterminant, q.nUnderdeterminedCells, q.minDeterminantCell) == (0.0, 1, 0)
    _assert_fields(e, f)


def test_dented_slab(oracle_lib):
    m, faces = dented_slab()
    rep, f = geometry_reference_of(oracle_lib, m)
    e = _engine(m)
    q = e.mesh_quality_geometry()
    assert q.nConcaveFaces == 2 and q.maxConcaveFace == min(faces)
    assert abs(q.maxConcaveSin - 15.0 / 17.0) <= 1e-12
    assert abs(q.maxConcaveAngle - math.degrees(math.asin(15.0 / 17.0))) <= 1e-10
    conc = e.quality_geometry_field("faceConcavity")
    assert np.all(np.delete(conc, faces) == 0.0) and np.max(np.abs(conc[faces] - 15.0 / 17.0)) <= 1e-12
    # a corner of 61.9 degrees is fine under a threshold of 70
    assert e.mesh_quality_geometry(concaveThreshold=70.0).nConcaveFaces == 0
    _assert_fields(e, f)


def test_tangled_block(oracle_lib):
    m = tangled_block()
    rep, f = geometry_reference_of(oracle_lib, m)
    e = _engine(m)
    q = e.mesh_quality_geometry()
    assert q.minVolRatio <= 0.0 and q.nLowVolRatioFaces >= 1
    for k in COUNTS:
        assert getattr(q, k) == rep[k], k
    _assert_fields(e, f)


# ---- parity with the numpy reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["com", "org"])
@pytest.mark.parametrize("name", PARITY)
def test_parity(name, variant):
    m, rep, f = _case(name, variant)
    _assert_well_posed(m, rep, f)
    if name == "bent":                                         # the non-zero branches of the counts
        assert min(rep[k] for k in ("nConcaveFaces", "nWarpedFaces", "nLowWeightFaces", "nLowVolRatioFaces")) >= 1, rep
    e = _engine(m, variant)
    _assert_report(e.mesh_quality_geometry(), rep)
    _assert_fields(e, f)


# ---- no side effects, repeatability ----------------------------------------------------------------------------------
def test_report_leaves_the_loop_untouched():
    from smoothmesh_amd import default_params
    from smoothmesh_amd.polymesh import cavity_mesh
    m = cavity_mesh(16, jitter=0.2, seed=3)
    runs = []
    for with_report in (False, True):
        e = _engine(m)
        e.set_params(default_params(e.mesh_stats()[0]))            # constraints on: the face-angle walk runs
        if with_report:
            n1, r1, f1 = e.iterate(5, 0.0)
            walk, counters, before = e.debug_walk_mode(), e.counters(), e.mesh_quality()
            e.mesh_quality_geometry()
            for name in FIELDS:
                e.quality_geometry_field(name)
            assert e.debug_walk_mode() == walk
            after = e.counters()
            assert [(k["name"], k["launches"]) for k in after] == [(k["name"], k["launches"]) for k in counters]
            assert e.mesh_quality() == before                      # the existing report: bit-equal before and after
            n2, r2, f2 = e.iterate(5, 0.0)
            n, res, frz = n1 + n2, np.concatenate([r1, r2]), np.concatenate([f1, f2])
        else:
            n, res, frz = e.iterate(10, 0.0)
        runs.append((n, res, frz, e.get_points(), e.near_ties()))
    (na, ra, fa_, pa, ta), (nb, rb, fb, pb, tb) = runs
    assert na == nb == 10
    assert np.array_equal(ra, rb) and np.array_equal(fa_, fb)
    assert np.array_equal(pa, pb)
    assert ta == tb
    assert fa_.max() > 0                                             # the constraints did freeze points


def test_report_needs_no_params_and_is_bitwise_repeatable():
    from smoothmesh_amd.polymesh import cavity_mesh
    m = cavity_mesh(30, jitter=0.2, seed=5)
    e1, e2 = _engine(m), _engine(m)                                  # (no set_params)
    a, b, c = e1.mesh_quality_geometry(), e1.mesh_quality_geometry(), e2.mesh_quality_geometry()
    for k in dataclasses.asdict(a):
        x, y, z = (np.array(getattr(r, k)).tobytes() for r in (a, b, c))
        assert x == y == z, k
    for name in FIELDS:
        x, y, z = e1.quality_geometry_field(name), e1.quality_geometry_field(name), e2.quality_geometry_field(name)
        assert x.tobytes() == y.tobytes() == z.tobytes(), name


def test_unknown_field_is_an_error():
    from smoothmesh_amd import SmgpuError
    e = _engine(cube27())
    with pytest.raises(SmgpuError, match="unknown quality geometry field"):
        e.quality_geometry_field("cellVolume")


# ---- refusal on a halo engine ----------------------------------------------------------------------------------------
def test_halo_engine_refuses():
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
            ds.engine.mesh_quality_geometry()
        with pytest.raises(SmgpuError, match="halo"):
            ds.engine.quality_geometry_field("cellDeterminant")
    finally:
        dist.destroy_process_group()


# ---- command line ----------------------------------------------------------------------------------------------------
def _run(case, opts, check=True):
    r = subprocess.run([BIN, "-case", str(case)] + opts, capture_output=True, text=True, timeout=300)
    if check:
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def _blocks(out):
    """{label: [the block's lines after its heading, up to its blank line]}"""
    lines = out.splitlines()
    blocks = {}
    for i, line in enumerate(lines):
        if line.startswith("Mesh quality (") and line.endswith("):"):
            j = lines.index("", i)
            blocks[line[len("Mesh quality ("):-2]] = lines[i + 1:j]
    return blocks


def test_cli_all_geometry(tmp_path):
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import read_polymesh, write_case
    from smoothmesh_amd.quality import format_geometry_lines, format_report
    m = hex_block(9, 8, 7, jitter=0.3, seed=4)
    for d in "abc":
        write_case(str(tmp_path / d), m, binary=True, writeFormat="binary")
    iters = ["-centroidalIters", "8", "-relTol", "0"]
    out = _run(tmp_path / "a", iters + ["-checkQuality", "true", "-allGeometry", "true"]).stdout
    b = _blocks(out)
    assert list(b) == ["initial mesh", "final mesh"]
    final = read_polymesh(str(tmp_path / "a" / "constant" / "polyMesh"), str(tmp_path / "a" / "8" / "polyMesh"))
    assert final.points.shape == m.points.shape and not np.array_equal(final.points, m.points)
    for label, pts in (("initial mesh", m.points), ("final mesh", final.points)):
        mm = hex_block(9, 8, 7, jitter=0.3, seed=4)
        mm.points = np.ascontiguousarray(pts)
        e = _engine(mm)
        assert len(b[label]) == 13
        assert [w.split()[0] for w in b[label][8:]] == ["faceConcavity", "faceFlatness", "faceWeight", "volumeRatio", "cellDeterminant"]
        assert "\n".join(b[label][8:]) + "\n" == format_geometry_lines(e.mesh_quality_geometry()), label
        assert "Mesh quality (%s):\n" % label + "\n".join(b[label]) + "\n\n" == format_report(e.mesh_quality(), label, e.mesh_quality_geometry())
    # without the option: today's block
    plain = _run(tmp_path / "b", iters + ["-checkQuality", "true"]).stdout
    pb = _blocks(plain)
    assert list(pb) == ["initial mesh", "final mesh"]
    for label in pb:
        assert pb[label] == b[label][:8]
    assert "Mesh quality (initial mesh):\n" + "\n".join(pb["initial mesh"]) + "\n\n" == format_report(_engine(m).mesh_quality(), "initial mesh")
    assert "faceConcavity" not in plain and "cellDeterminant min" not in plain
    # refusals
    r = _run(tmp_path / "c", iters + ["-allGeometry", "true"], check=False)
    assert r.returncode != 0 and "-allGeometry needs -checkQuality" in r.stdout + r.stderr
    r = _run(tmp_path / "c", ["-parallel", "-checkQuality", "true", "-allGeometry", "true"], check=False)
    assert r.returncode != 0
    r = _run(tmp_path / "c", ["-parallel", "-allGeometry", "true"], check=False)
    assert r.returncode != 0 and "-allGeometry is not available with -parallel" in r.stdout + r.stderr
    assert not (tmp_path / "c" / "8").exists()
    # the Python tool: the same five lines, of the case's latest time
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "smoothmesh_amd.check_quality", "-case", str(tmp_path / "a"), "-allGeometry"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert _blocks(r.stdout)["mesh"] == b["final mesh"]
    r = subprocess.run([sys.executable, "-m", "smoothmesh_amd.check_quality", "-case", str(tmp_path / "a"), "-allGeometry", "-parallel"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode != 0 and "neighbour rank's cell volume" in r.stdout + r.stderr
