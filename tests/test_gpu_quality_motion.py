"""The motion criteria on the GPU (include/smgpu.h smgpu_mesh_quality_motion / smgpu_quality_motion_field,
csrc/kernels_quality_motion.hpp) against the numpy restatement of their definitions (tests/test_quality_motion_reference.py), their
freedom from side effects, their repeatability, the refusal on a halo engine and the `-meshQuality` lines of the front-ends.

Tolerances (as tests/test_gpu_quality_geometry.py): both sides take the same inputs bit for bit and evaluate the same IEEE operations
in the same order; only the order of the report's sums differs (the averages: a few ulp of their largest term).  Counts and ids are
exact (the meshes are checked to hold no element near a threshold and no second element near a reported minimum), report values
1e-12 and fields 1e-13, both relative to max(|ref|, 1).  A tet quality divides by the cube of the circumradius, which is itself a
quotient by the tet's volume; both sides form it with the same operations, so the cube amplifies no difference between them."""
import dataclasses
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from test_quality_motion_reference import (COUNTS, CUBE_CENTRE_TET, MOTION_DEFAULTS, concave_quad, cube27, face_base_minima,
                                           motion_reference_of)
from test_quality_geometry_reference import saddle_cell
from test_quality_reference import oracle_geometry, tangled_block

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "smoothmesh_amd", "bin", "smoothMesh")
FIELDS = ("faceTetQuality", "faceBaseTetQuality", "faceTwist", "faceTriangleTwist")
EXACT = COUNTS + ("nTwistFaces", "minTetFace", "minBaseTetFace", "minTwistFace", "minTriangleTwistFace")
VALUES = ("minTetQuality", "avgTetQuality", "minBaseTetQuality", "minTwist", "avgTwist", "minTriangleTwist", "avgTriangleTwist")
MOTION_LINES = ["faceTets", "faceBaseTets", "faceTwist", "triangleTwist"]


def _engine(mesh, variant="com"):
    from smoothmesh_amd import SmoothEngine
    e = SmoothEngine(mesh)
    e.set_foam_variant(variant)
    return e


def bent_block():
    """a jittered block with a few points moved by hand, so that every count is non-zero: an interior point pushed across its cell
    (tangled cells: inverted tets, faces without a valid base point, twisted quadrilaterals), and a second one moved close to its
    x-neighbour (a thin cell).  Seed 23: with 21 and 22 one tet quality of the thin cell lies within 1e-9 of tetThreshold, which
    _assert_well_posed refuses"""
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(9, 8, 7, jitter=0.2, seed=23)
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
        return hex_block(12, 9, 7, jitter=0.3)           # 2523 faces: one 2048-face workgroup and a short second one
    if name == "block2184":
        return hex_block(14, 13, 12, jitter=0.25)        # 7058 faces: three full workgroups plus a ragged tail
    if name == "cavity54":
        return cavity_mesh(54, jitter=0.2, seed=9)       # polygons with hanging nodes: faces of more than four vertices
    assert name == "bent"
    return bent_block()


PARITY = ("block756", "block2184", "cavity54", "bent")


@functools.lru_cache(maxsize=None)
def _case(name, variant):
    """(mesh, reference report, reference fields), computed once and left unchanged"""
    from oracle import oracle_ffi
    oracle_ffi.build()
    m = _mesh(name)
    rep, f = motion_reference_of(oracle_ffi, m, variant)
    for v in f.values():
        v.setflags(write=False)
    return m, rep, f


def _assert_well_posed(m, rep, f):
    """on the reference alone: no element within 1e-9 of a threshold or of a reported minimum"""
    d = MOTION_DEFAULTS
    s = f["_summed"]
    assert s.sum() >= 2
    per = ((f["faceTetQuality"], d["tetThreshold"]), (f["faceBaseTetQuality"], d["tetThreshold"]),
           (f["faceTwist"][s], d["twistThreshold"]), (f["faceTriangleTwist"][s], d["triangleTwistThreshold"]))
    for v, t in per:
        assert np.min(np.abs(v - t)) > 1e-9, t
        v = np.sort(v)
        assert v[1] - v[0] > 1e-9, v[:2]


def _assert_report(q, rep, tied=(), engine=None, mesh=None):
    """tied: ids of minima that several elements share within rounding (the reference's id is a matter of the last bit): held to the
    lowest id among the elements that share the minimum of the engine's own field"""
    from quality_fold_reference import engine_lowest_id
    got = dataclasses.asdict(q)
    assert list(got) == list(rep)
    for k in got:
        print(f"    {k}: engine {got[k]!r} reference {rep[k]!r}")
    for k in EXACT:
        if k in tied:
            assert got[k] == engine_lowest_id(engine, mesh, k), (k, got[k])
            continue
        assert got[k] == rep[k], (k, got[k], rep[k])
    for k in VALUES:
        assert abs(got[k] - rep[k]) <= 1e-12 * max(abs(rep[k]), 1.0), (k, got[k], rep[k])


def _assert_fields(e, f):
    for name in FIELDS:
        g, r = e.quality_motion_field(name), f[name]
        assert g.shape == r.shape, name
        err = float(np.max(np.abs(g - r) / np.maximum(np.abs(r), 1.0)))
        print(f"    {name}: max error {err:.3e}")
        assert err <= 1e-13, (name, err)


TIED_IDS = ("minTetFace", "minBaseTetFace", "minTwistFace", "minTriangleTwistFace")


# ---- known answers -------------------------------------------------------------------------------------------------
def test_uniform_cube(oracle_lib):
    m = cube27()
    rep, f = motion_reference_of(oracle_lib, m)
    e = _engine(m)
    q = e.mesh_quality_motion()
    assert np.max(np.abs(e.quality_motion_field("faceTetQuality") - CUBE_CENTRE_TET)) <= 1e-12
    assert abs(q.minTetQuality - CUBE_CENTRE_TET) <= 1e-12 and abs(q.avgTetQuality - CUBE_CENTRE_TET) <= 1e-12
    assert abs(q.minTwist - 1.0) <= 1e-12 and abs(q.avgTwist - 1.0) <= 1e-12
    assert abs(q.minTriangleTwist - 1.0) <= 1e-12 and abs(q.avgTriangleTwist - 1.0) <= 1e-12
    assert q.nTwistFaces == m.nFaces
    for k in COUNTS:
        assert getattr(q, k) == 0 == rep[k], k
    _assert_report(q, rep, tied=TIED_IDS, engine=e, mesh=m)     # equal faces: the lowest id of the engine's own ties
    _assert_fields(e, f)


@pytest.mark.parametrize("variant", ["com", "org"])
@pytest.mark.parametrize("h", [0.5, 0.1])
def test_saddle_face(oracle_lib, variant, h):
    m, top = saddle_cell(h)
    rep, f = motion_reference_of(oracle_lib, m, variant, triangleTwistThreshold=0.6)
    e = _engine(m, variant)
    q = e.mesh_quality_motion(triangleTwistThreshold=0.6)
    assert abs(e.quality_motion_field("faceTwist")[top] - 1.0 / np.sqrt(1.0 + 4.0 * h * h)) <= 1e-12
    assert abs(e.quality_motion_field("faceTriangleTwist")[top] - 1.0 / (1.0 + 4.0 * h * h)) <= 1e-12
    assert q.minTwistFace == top and abs(q.minTwist - 1.0 / np.sqrt(1.0 + 4.0 * h * h)) <= 1e-12
    assert q.minTriangleTwistFace == top and abs(q.minTriangleTwist - 1.0 / (1.0 + 4.0 * h * h)) <= 1e-12
    assert q.nLowTriangleTwistFaces == (1 if h == 0.5 else 0) == rep["nLowTriangleTwistFaces"]
    assert e.mesh_quality_motion().nLowTriangleTwistFaces == 0          # the default -1: off
    _assert_report(q, rep, tied=("minTetFace", "minBaseTetFace"), engine=e, mesh=m)       # the four side faces are mirror images
    _assert_fields(e, f)


def test_tangled_block(oracle_lib):
    m = tangled_block()
    rep, f = motion_reference_of(oracle_lib, m)
    e = _engine(m)
    q = e.mesh_quality_motion()
    assert q.minTetQuality < 0.0 and q.nLowTetFaces >= 1
    for k in COUNTS:
        assert getattr(q, k) == rep[k], k
    _assert_fields(e, f)


def test_concave_quadrilateral(oracle_lib):
    m, face = concave_quad()
    rep, f = motion_reference_of(oracle_lib, m)
    mb = face_base_minima(m, oracle_geometry(oracle_lib, m)[2], face)
    assert mb.min() < 0.0 < mb.max()
    e = _engine(m)
    got = e.quality_motion_field("faceBaseTetQuality")[face]
    assert got > 0.0 and abs(got - mb.max()) <= 1e-13          # the best base decides, not base 0
    for k in COUNTS:
        assert getattr(e.mesh_quality_motion(), k) == rep[k], k
    _assert_fields(e, f)
    # thresholds are the caller's: every face of the slab is low under a tet threshold of 2, every quadrilateral under a twist of 2
    t = e.mesh_quality_motion(tetThreshold=2.0, twistThreshold=2.0, triangleTwistThreshold=2.0)
    assert (t.nLowTetFaces, t.nNoBasePointFaces, t.nLowTwistFaces, t.nLowTriangleTwistFaces) == (m.nFaces,) * 4


# ---- parity with the numpy reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["com", "org"])
@pytest.mark.parametrize("name", PARITY)
def test_parity(name, variant):
    m, rep, f = _case(name, variant)
    _assert_well_posed(m, rep, f)
    if name == "bent":                                         # the non-zero branches of the counts
        assert rep["nLowTetFaces"] >= 1 and rep["nLowTwistFaces"] >= 1 and rep["nNoBasePointFaces"] >= 1, rep
    if name == "cavity54":
        assert np.diff(m.faceOffsets).max() > 4
    e = _engine(m, variant)
    _assert_report(e.mesh_quality_motion(), rep)
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
            e.mesh_quality_motion()
            for name in FIELDS:
                e.quality_motion_field(name)
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
    a, b, c = e1.mesh_quality_motion(), e1.mesh_quality_motion(), e2.mesh_quality_motion()
    for k in dataclasses.asdict(a):
        x, y, z = (np.array(getattr(r, k)).tobytes() for r in (a, b, c))
        assert x == y == z, k
    for name in FIELDS:
        x, y, z = e1.quality_motion_field(name), e1.quality_motion_field(name), e2.quality_motion_field(name)
        assert x.tobytes() == y.tobytes() == z.tobytes(), name


def test_unknown_field_is_an_error():
    from smoothmesh_amd import SmgpuError
    e = _engine(cube27())
    with pytest.raises(SmgpuError, match="unknown quality motion field"):
        e.quality_motion_field("faceFlatness")


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
            ds.engine.mesh_quality_motion()
        with pytest.raises(SmgpuError, match="halo"):
            ds.engine.quality_motion_field("faceTwist")
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


def test_cli_mesh_quality(tmp_path):
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import read_polymesh, write_case
    from smoothmesh_amd.quality import format_motion_lines, format_report
    m = hex_block(9, 8, 7, jitter=0.3, seed=4)
    for d in "abcd":
        write_case(str(tmp_path / d), m, binary=True, writeFormat="binary")
    iters = ["-centroidalIters", "8", "-relTol", "0"]
    out = _run(tmp_path / "a", iters + ["-checkQuality", "true", "-meshQuality", "true"]).stdout
    b = _blocks(out)
    assert list(b) == ["initial mesh", "final mesh"]
    both = _blocks(_run(tmp_path / "d", iters + ["-checkQuality", "true", "-allGeometry", "true", "-meshQuality", "true"]).stdout)
    final = read_polymesh(str(tmp_path / "a" / "constant" / "polyMesh"), str(tmp_path / "a" / "8" / "polyMesh"))
    assert final.points.shape == m.points.shape and not np.array_equal(final.points, m.points)
    for label, pts in (("initial mesh", m.points), ("final mesh", final.points)):
        mm = hex_block(9, 8, 7, jitter=0.3, seed=4)
        mm.points = np.ascontiguousarray(pts)
        e = _engine(mm)
        assert len(b[label]) == 12
        assert [w.split()[0] for w in b[label][8:]] == MOTION_LINES
        assert "\n".join(b[label][8:]) + "\n" == format_motion_lines(e.mesh_quality_motion()), label
        assert "Mesh quality (%s):\n" % label + "\n".join(b[label]) + "\n\n" == format_report(e.mesh_quality(), label, None, e.mesh_quality_motion())
        # with -allGeometry as well: its five lines first, then these four
        assert len(both[label]) == 17 and both[label][13:] == b[label][8:] and both[label][:8] == b[label][:8]
        assert "Mesh quality (%s):\n" % label + "\n".join(both[label]) + "\n\n" == format_report(e.mesh_quality(), label, e.mesh_quality_geometry(),
                                                                                                 e.mesh_quality_motion())
    # without the option: today's block
    plain = _run(tmp_path / "b", iters + ["-checkQuality", "true"]).stdout
    pb = _blocks(plain)
    assert list(pb) == ["initial mesh", "final mesh"]
    for label in pb:
        assert pb[label] == b[label][:8]
    assert "Mesh quality (initial mesh):\n" + "\n".join(pb["initial mesh"]) + "\n\n" == format_report(_engine(m).mesh_quality(), "initial mesh")
    assert "faceTets" not in plain and "triangleTwist" not in plain
    # refusals
    r = _run(tmp_path / "c", iters + ["-meshQuality", "true"], check=False)
    assert r.returncode != 0 and "-meshQuality needs -checkQuality" in r.stdout + r.stderr
    r = _run(tmp_path / "c", ["-parallel", "-checkQuality", "true", "-meshQuality", "true"], check=False)
    assert r.returncode != 0 and "-checkQuality is not available with -parallel" in r.stdout + r.stderr    # the existing refusal comes first
    r = _run(tmp_path / "c", ["-parallel", "-meshQuality", "true"], check=False)
    assert r.returncode != 0 and "-meshQuality is not available with -parallel" in r.stdout + r.stderr
    assert not (tmp_path / "c" / "8").exists()
    # the Python tool: the same four lines, of the case's latest time
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    tool = [sys.executable, "-m", "smoothmesh_amd.check_quality", "-case", str(tmp_path / "a")]
    r = subprocess.run(tool + ["-meshQuality"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert _blocks(r.stdout)["mesh"] == b["final mesh"]
    r = subprocess.run(tool + ["-meshQuality", "-parallel"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode != 0 and "-meshQuality is not available with -parallel" in r.stdout + r.stderr
