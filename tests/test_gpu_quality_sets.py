"""smgpu_quality_sets on the MI355X (DESIGN.md "Mesh quality", 10.5): the engine's sets against the numpy restatement
(tests/test_quality_sets_reference.py), sizes against the report's counts, order, repeatability, compaction at workgroup
boundaries, refusals, and smoothMesh -writeSets."""
import dataclasses
import math
import os
import subprocess

import numpy as np
import pytest

from test_quality_reference import DEFAULTS, cell_faces, tangled_block, two_cells, uniform_block
from test_quality_sets_reference import NAMES, assert_sizes_are_counts, quality_sets_reference, sets_reference_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "smoothmesh_amd", "bin", "smoothMesh")
OTHER = dict(nonOrthThreshold=25.0, skewThreshold=0.35, closedThreshold=1e-6, aspectThreshold=2.2)


def _engine(mesh, variant="com"):
    from smoothmesh_amd import SmoothEngine
    e = SmoothEngine(mesh)
    e.set_foam_variant(variant)
    return e


def _assert_well_posed(f, nInternal, **thr):
    """no reference element within 1e-9 of a threshold of thr: membership is then well defined"""
    thr = {**DEFAULTS, **thr}
    cosT = math.cos(math.radians(thr["nonOrthThreshold"]))
    o = f["faceOrtho"][:nInternal]
    assert np.min(np.abs(o - cosT)) > 1e-9 and np.min(np.abs(o)) > 1e-9
    assert np.min(np.abs(f["faceSkewness"] - thr["skewThreshold"])) > 1e-9
    assert np.min(np.abs(f["cellOpenness"] - thr["closedThreshold"])) > 1e-9 * thr["closedThreshold"]
    assert np.min(np.abs(f["cellAspectRatio"] - thr["aspectThreshold"])) > 1e-9
    assert np.min(np.abs(f["cellVolume"]) / f["cellAbsPyramids"]) > 1e-9


def _assert_sets(got, want):
    assert list(got) == list(NAMES)
    for k in NAMES:
        assert got[k].dtype == np.int32, k
        assert np.all(np.diff(got[k]) > 0), k                       # strictly ascending
        assert np.array_equal(got[k], want[k]), (k, len(got[k]), len(want[k]))


def _check(e, rep, want, **thr):
    """the engine's sets equal the reference's, ascending; sizes equal the engine's and the reference's report counts"""
    got = e.quality_sets(**thr)
    _assert_sets(got, want)
    q = dataclasses.asdict(e.mesh_quality(**thr))
    assert_sizes_are_counts(got, q)
    assert_sizes_are_counts(got, rep)
    return got


# ---- against the numpy restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["uniform", "two_cells", "tangled"])
def test_known_answers(oracle_lib, which):
    m = {"uniform": uniform_block, "tangled": tangled_block, "two_cells": lambda: two_cells(0.5)}[which]()
    rep, _, want = sets_reference_of(oracle_lib, m)
    got = _check(_engine(m), rep, want)
    if which == "uniform":
        assert all(len(v) == 0 for v in got.values())
    if which == "tangled":
        assert len(got["zeroVolumeCells"]) >= 1 and len(got["wrongOrientedFaces"]) >= 1
    if which == "two_cells":
        theta = math.degrees(math.atan(0.25))
        below = _engine(m).quality_sets(nonOrthThreshold=theta - 1e-6, skewThreshold=0.25 - 1e-9)
        above = _engine(m).quality_sets(nonOrthThreshold=theta + 1e-6, skewThreshold=0.25 + 1e-9)
        assert 0 in below["nonOrthoFaces"] and 0 in below["skewFaces"]
        assert len(above["nonOrthoFaces"]) == 0 and 0 not in above["skewFaces"]    # (boundary faces of the sheared cell stay)


@pytest.mark.parametrize("variant", ["com", "org"])
@pytest.mark.parametrize("thr", ["default", "other"])
@pytest.mark.parametrize("nx,ny,nz,jit,seed", [(8, 8, 8, 0.35, 1), (13, 9, 7, 0.45, 2)])
def test_parity_jittered_blocks(oracle_lib, variant, thr, nx, ny, nz, jit, seed):
    from smoothmesh_amd.meshgen import hex_block
    t = {} if thr == "default" else OTHER
    m = hex_block(nx, ny, nz, jitter=jit, seed=seed)
    rep, f, want = sets_reference_of(oracle_lib, m, variant, **t)
    _assert_well_posed(f, m.nInternalFaces, **t)
    got = _check(_engine(m, variant), rep, want, **t)
    if thr == "other":
        assert len(got["nonOrthoFaces"]) and len(got["skewFaces"])


@pytest.mark.parametrize("variant", ["com", "org"])
@pytest.mark.parametrize("thr", ["default", "other"])
def test_parity_cavity_mesh(oracle_lib, variant, thr):
    from smoothmesh_amd.polymesh import cavity_mesh
    t = {} if thr == "default" else OTHER
    m = cavity_mesh(30, jitter=0.2, seed=9)
    rep, f, want = sets_reference_of(oracle_lib, m, variant, **t)
    _assert_well_posed(f, m.nInternalFaces, **t)
    _check(_engine(m, variant), rep, want, **t)


# ---- compaction at workgroup boundaries ---------------------------------------------------------------------------
def test_every_element_in_a_set_on_a_million_cells():
    """skewThreshold -1 and aspectThreshold 0 put every face / cell in a set: the scan spans hundreds of workgroups"""
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(101, 100, 100, jitter=0.2, seed=7)
    assert m.nCells > 1_000_000 and m.nCells % 256 and m.nFaces % 256
    e = _engine(m)
    got = e.quality_sets(skewThreshold=-1.0, aspectThreshold=0.0)
    assert np.array_equal(got["skewFaces"], np.arange(m.nFaces, dtype=np.int32))
    assert np.array_equal(got["highAspectRatioCells"], np.arange(m.nCells, dtype=np.int32))
    assert_sizes_are_counts(got, dataclasses.asdict(e.mesh_quality(skewThreshold=-1.0, aspectThreshold=0.0)))
    d = e.quality_sets()
    assert_sizes_are_counts(d, dataclasses.asdict(e.mesh_quality()))
    assert all(len(v) == 0 for v in d.values())                       # a mesh where no element qualifies


def _split_between(v):
    """a threshold halfway between the two sorted values around the median that lie more than 1e-6 apart"""
    v = np.sort(v)
    for k in range(len(v) // 2, len(v) - 1):
        if v[k + 1] - v[k] > 1e-6 * max(abs(v[k]), 1.0):
            return float(0.5 * (v[k] + v[k + 1]))
    raise AssertionError("no gap")


@pytest.mark.parametrize("dims", [(3, 2, 2), (7, 5, 3), (17, 11, 13), (21, 20, 19)])
def test_element_counts_off_the_block_sizes(dims):
    """nFaces / nCells not multiples of 256 or 2048, thresholds that take about half of a face set and a cell set; the
    reference takes the engine's own published geometry (bit-identical to the oracle's: tests/test_gpu_parity.py)"""
    from smoothmesh_amd import default_params
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(*dims, jitter=0.4, seed=sum(dims))
    assert m.nFaces % 256 and m.nCells % 256
    g = _engine(m)
    g.set_params(default_params(g.mesh_stats()[0]))
    g.debug_propose()
    geo = tuple(g.debug_field(k).reshape(-1, 3) for k in ("faceCentres", "faceAreas", "cellCentres"))
    _, f = quality_sets_reference(m, *geo, *cell_faces(m))[:2]
    t = dict(skewThreshold=_split_between(f["faceSkewness"]), aspectThreshold=_split_between(f["cellAspectRatio"]),
             nonOrthThreshold=20.0)
    rep, f, want = quality_sets_reference(m, *geo, *cell_faces(m), **t)
    _assert_well_posed(f, m.nInternalFaces, **t)
    got = _check(_engine(m), rep, want, **t)
    assert len(got["skewFaces"]) >= m.nFaces // 3 and len(got["highAspectRatioCells"]) >= m.nCells // 3


# ---- the loop, repeatability, refusals ----------------------------------------------------------------------------
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
            a, b = e.quality_sets(**OTHER), e.quality_sets(**OTHER)
            assert all(a[k].tobytes() == b[k].tobytes() for k in NAMES)
            assert sum(len(v) for v in a.values()) > 0
            assert e.debug_walk_mode() == walk
            n2, r2, f2 = e.iterate(5, 0.0)
            n, res, frz = n1 + n2, np.concatenate([r1, r2]), np.concatenate([f1, f2])
        else:
            n, res, frz = e.iterate(10, 0.0)
        runs.append((n, res, frz, e.get_points(), e.near_ties()))
    (na, ra, fa_, pa, ta), (nb, rb, fb, pb, tb) = runs
    assert na == nb == 10
    assert ra.tobytes() == rb.tobytes() and np.array_equal(fa_, fb)
    assert pa.tobytes() == pb.tobytes()
    assert ta == tb


def test_small_cap_is_refused_with_counts():
    import ctypes as C
    from smoothmesh_amd import SmgpuError, _ffi
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(9, 8, 7, jitter=0.3, seed=4)
    e = _engine(m)
    want = e.quality_sets(**OTHER)
    total = sum(len(v) for v in want.values())
    assert total > 1
    p = _ffi.QualityParams(OTHER["nonOrthThreshold"], OTHER["skewThreshold"], OTHER["closedThreshold"], OTHER["aspectThreshold"])
    counts = (C.c_int64 * 7)()
    ids = np.full(total, -7, np.int32)
    rc = e._lib.smgpu_quality_sets(e._h, C.byref(p), counts, ids.ctypes.data_as(_ffi.c_i32p), total - 1)
    assert rc != 0 and "ids holds" in e._lib.smgpu_last_error().decode()
    assert list(counts) == [len(want[k]) for k in NAMES]
    assert np.all(ids == -7)
    counts2 = (C.c_int64 * 7)()
    assert e._lib.smgpu_quality_sets(e._h, C.byref(p), counts2, None, 0) == 0          # counts only
    assert list(counts2) == list(counts)
    assert e._lib.smgpu_quality_sets(e._h, C.byref(p), counts2, ids.ctypes.data_as(_ffi.c_i32p), total) == 0
    assert np.array_equal(ids, np.concatenate([want[k] for k in NAMES]))
    with pytest.raises(SmgpuError):
        e._check(e._lib.smgpu_quality_sets(e._h, C.byref(p), None, None, 0))


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
            ds.engine.quality_sets()
        sets = ds.quality_sets()                                       # the coupled form works on the same engine
        assert list(sets) == list(NAMES)
    finally:
        dist.destroy_process_group()


# ---- smoothMesh -writeSets ------------------------------------------------------------------------------------------
def _run(case, opts, check=True):
    r = subprocess.run([BIN, "-case", str(case)] + opts, capture_output=True, text=True, timeout=600)
    if check:
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def test_cli_write_sets(tmp_path):
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import read_label_list, read_polymesh, write_case
    from smoothmesh_amd.quality import QUALITY_SETS
    from test_gpu_quality import _parse_blocks
    m = hex_block(12, 10, 3, lengths=(1.0, 1.0, 2e-5), jitter=0.2, seed=6)    # flat: cell aspect ratios near 10 000
    for c in ("a", "b"):
        write_case(str(tmp_path / c), m, binary=True, writeFormat="binary")
    opts = ["-centroidalIters", "8", "-relTol", "0", "-checkQuality", "true"]
    r = _run(tmp_path / "a", opts + ["-writeSets", "true"])
    out = r.stdout
    dirs = [d for d in os.listdir(tmp_path / "a") if d not in ("system", "constant")]
    assert dirs == ["8"], dirs
    assert not os.path.exists(tmp_path / "a" / "constant" / "polyMesh" / "sets")
    sets_dir = tmp_path / "a" / "8" / "polyMesh" / "sets"
    w = read_polymesh(str(tmp_path / "a" / "constant" / "polyMesh"), str(tmp_path / "a" / "8" / "polyMesh"))
    want = _engine(w).quality_sets()
    assert len(want["highAspectRatioCells"]) > 0                        # at least one set is non-empty
    files = sorted(os.listdir(sets_dir))
    assert files == sorted(k for k in NAMES if len(want[k])), files
    for k in files:
        assert np.array_equal(read_label_list(str(sets_dir / k)), want[k]), k
    # the nine-line block stays as it is; the lines follow its blank line
    b = _parse_blocks(out)
    assert list(b) == ["initial mesh", "final mesh"]
    assert b["final mesh"]["nHighAspectCells"] == len(want["highAspectRatioCells"])
    lines = out.splitlines()
    i = lines.index("Mesh quality (final mesh):")
    j = i + 9 + (1 if lines[i + 9].startswith("    ***") else 0)
    assert lines[j] == ""
    desc = {n: d for n, _, _, d in QUALITY_SETS}
    wl = [f"    <<Writing {len(want[k])} {desc[k]} to set {k}" for k in NAMES if len(want[k])]
    assert lines[j + 1:j + 1 + len(wl)] == wl
    # without the option: the same run writes no sets and prints no such line
    plain = _run(tmp_path / "b", opts).stdout
    assert "<<Writing" not in plain
    assert not any("sets" in dn for _, dn, _ in os.walk(tmp_path / "b"))
