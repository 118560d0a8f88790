"""The -allGeometry checks and the motion criteria of a decomposed mesh on the GPU (include/smgpu.h smgpu_quality_coupled_pack_volumes,
smgpu_quality_coupled_geometry_* / _motion_*, smoothmesh_amd/quality.py, DESIGN.md "Mesh quality", 10.8): the combined reports of
the sub-domains equal the serial engine's reports of the undecomposed mesh and the numpy references, through every driver."""
import dataclasses
import functools
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_quality_decomposed import _case, _gather_points, _local
from test_gpu_quality_geometry import FIELDS as GEOMETRY_FIELDS, _engine
from test_gpu_quality_motion import FIELDS as MOTION_FIELDS
from test_quality_geometry_motion_decomposed_reference import (ALLOWED_DIFF, GEOMETRY_EXACT, MOTION_EXACT, NEW_FORMULA_FIELDS,
                                                               NEW_FORMULA_VALUES)
from test_quality_geometry_reference import geometry_reference_of
from test_quality_motion_reference import motion_reference_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# thresholds chosen on the CPU with the numpy references, all but concaveThreshold away from their defaults: every count of both
# reports is positive on these meshes, with processor faces among the counted elements of every face criterion.  concaveThreshold
# keeps its default 10 degrees: the polyhedral "cavity" mesh has concave faces at it, some of them on processor patches
G_THR = dict(concaveThreshold=10.0, flatnessThreshold=0.98, weightThreshold=0.45, volRatioThreshold=0.6, determinantThreshold=0.9)
M_THR = dict(tetThreshold=0.3, twistThreshold=0.95, triangleTwistThreshold=0.9)
G_COUNTS = ("nConcaveFaces", "nWarpedFaces", "nLowWeightFaces", "nLowVolRatioFaces", "nUnderdeterminedCells")
M_COUNTS = ("nLowTetFaces", "nNoBasePointFaces", "nLowTwistFaces", "nLowTriangleTwistFaces")
MARGIN = 1e-9          # well-posedness: far above every comparison tolerance below (ALLOWED_DIFF, 1e-12)


@functools.lru_cache(maxsize=None)
def _refs(kind, variant):
    """(mesh, sub-domains, geometry report, geometry fields, motion report, motion fields) of the numpy references of the
    undecomposed mesh, computed once and left unchanged"""
    from oracle import oracle_ffi
    oracle_ffi.build()
    m, subs = _case(kind)
    grep, gf = geometry_reference_of(oracle_ffi, m, variant, **G_THR)
    mrep, mf = motion_reference_of(oracle_ffi, m, variant, **M_THR)
    for v in list(gf.values()) + list(mf.values()):
        v.setflags(write=False)
    return m, subs, grep, gf, mrep, mf


def _proc_faces(m, subs):
    isProc = np.zeros(m.nFaces, bool)
    for s in subs:
        for p in s.mesh.patches:
            if p.type == "processor":
                isProc[s.faceProcAddressing[p.startFace:p.startFace + p.nFaces]] = True
    return isProc


def _criteria(m, gf, mf):
    """[(values of the elements a criterion covers, their global ids, threshold)] of the eight thresholded criteria"""
    Fi, s, allF = m.nInternalFaces, np.nonzero(gf["_summed"])[0], np.arange(m.nFaces)
    return dict(nWarpedFaces=(gf["faceFlatness"][s], s, G_THR["flatnessThreshold"]),
                nLowWeightFaces=(gf["faceWeight"][:Fi], allF[:Fi], G_THR["weightThreshold"]),
                nLowVolRatioFaces=(gf["faceVolumeRatio"][:Fi], allF[:Fi], G_THR["volRatioThreshold"]),
                nUnderdeterminedCells=(gf["cellDeterminant"], np.arange(m.nCells), G_THR["determinantThreshold"]),
                nLowTetFaces=(mf["faceTetQuality"], allF, M_THR["tetThreshold"]),
                nNoBasePointFaces=(mf["faceBaseTetQuality"], allF, M_THR["tetThreshold"]),
                nLowTwistFaces=(mf["faceTwist"][s], s, M_THR["twistThreshold"]),
                nLowTriangleTwistFaces=(mf["faceTriangleTwist"][s], s, M_THR["triangleTwistThreshold"]))


def _assert_well_posed(m, grep, gf, mf):
    """on the references alone (after _assert_well_posed of the sibling tests): no value within MARGIN of its threshold or of the
    concavity test's two limits, no two candidates for a winning id within MARGIN of each other"""
    for name, (v, _, t) in _criteria(m, gf, mf).items():
        assert np.min(np.abs(v - t)) > MARGIN, name
        v = np.sort(v)
        assert v[1] - v[0] > MARGIN, (name, v[:2])
    s, side = gf["_cornerSin"], gf["_cornerSide"]
    sinT = math.sin(math.radians(G_THR["concaveThreshold"]))
    assert np.min(np.abs(s - sinT)) > MARGIN
    if (s >= sinT).any():
        assert np.min(np.abs(side[s >= sinT])) > MARGIN
    conc = np.sort(gf["faceConcavity"][gf["faceConcavity"] > 0.0])
    if conc.size > 1:
        assert conc[-1] - conc[-2] > MARGIN
    assert grep["maxConcaveSin"] <= 0.99                       # the condition number the angle's tolerance rests on


def _assert_report(q, rep, exact):
    """counts, denominators and ids exact; values at the tolerances of the serial tests' _assert_report (1e-12), the new formulas
    at ALLOWED_DIFF relative to max(|reference|, 1)"""
    got = dataclasses.asdict(q) if dataclasses.is_dataclass(q) else q
    for k, v in rep.items():
        print(f"    {k}: decomposed {got[k]!r} reference {v!r}")
    for k, v in rep.items():
        if k in exact:
            assert got[k] == v, (k, got[k], v)
        elif k in NEW_FORMULA_VALUES:
            assert abs(got[k] - v) <= ALLOWED_DIFF * max(abs(v), 1.0), (k, got[k], v)
        elif k == "maxConcaveAngle":
            assert abs(got[k] - v) <= 1e-10, (k, got[k], v)
        else:
            assert abs(got[k] - v) <= 1e-12 * max(abs(v), 1.0), (k, got[k], v)


@pytest.mark.parametrize("variant", ["com", "org"])
@pytest.mark.parametrize("kind", ["grid", "bfs", "random", "cavity"])
def test_decomposed_reports_equal_serial(kind, variant):
    from smoothmesh_amd.quality import decomposed_mesh_quality_geometry, decomposed_mesh_quality_motion
    m, subs, grep, gf, mrep, mf = _refs(kind, variant)
    _assert_well_posed(m, grep, gf, mf)
    # the counts test something: each is positive here ("cavity" has the concave faces), with processor faces among the counted
    isProc = _proc_faces(m, subs)
    for name, (v, ids, t) in _criteria(m, gf, mf).items():
        assert (grep.get(name) or mrep.get(name)) > 0, name
        if "Cells" not in name:
            assert isProc[ids[v < t]].any(), name
    assert (grep["nConcaveFaces"] > 0) == (kind == "cavity")
    if kind == "cavity":
        assert isProc[gf["faceConcavity"] > 1e-15].any()
    e = _engine(m, variant)
    gser, mser = dataclasses.asdict(e.mesh_quality_geometry(**G_THR)), dataclasses.asdict(e.mesh_quality_motion(**M_THR))
    e.close()
    qg, qm = decomposed_mesh_quality_geometry(subs, foam_variant=variant, **G_THR), decomposed_mesh_quality_motion(subs, foam_variant=variant, **M_THR)
    ge, me = GEOMETRY_EXACT, MOTION_EXACT
    _assert_report(qg, gser, ge)
    _assert_report(qg, grep, ge)
    _assert_report(qm, mser, me)
    _assert_report(qm, mrep, me)
    ms = _local(subs, variant)
    assert dataclasses.asdict(ms.mesh_quality_geometry(**G_THR)) == dataclasses.asdict(qg)     # the same engines' records, the same combine
    assert dataclasses.asdict(ms.mesh_quality_motion(**M_THR)) == dataclasses.asdict(qm)
    # (rank, local id) of every winner leads to its global id
    for q, pairs in ((qg, (("maxConcave", "maxConcaveFace"), ("minFlatness", "minFlatnessFace"), ("minFaceWeight", "minFaceWeightFace"),
                           ("minVolRatio", "minVolRatioFace"), ("minDeterminant", "minDeterminantCell"))),
                     (qm, (("minTet", "minTetFace"), ("minBaseTet", "minBaseTetFace"), ("minTwist", "minTwistFace"),
                           ("minTriangleTwist", "minTriangleTwistFace")))):
        for stem, idName in pairs:
            r, loc, gid = getattr(q, stem + "Rank"), getattr(q, stem + "Local"), getattr(q, idName)
            if gid < 0:
                assert (r, loc) == (-1, -1)
                continue
            addr = subs[r].cellProcAddressing if idName.endswith("Cell") else subs[r].faceProcAddressing
            assert addr[loc] == gid, idName


def test_single_subdomain_is_bitwise_the_serial_report():
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.quality import decomposed_mesh_quality_geometry, decomposed_mesh_quality_motion
    m = hex_block(11, 9, 7, jitter=0.3, seed=5)
    e = _engine(m)
    pairs = ((dataclasses.asdict(e.mesh_quality_geometry(**G_THR)), dataclasses.asdict(decomposed_mesh_quality_geometry([m], **G_THR))),
             (dataclasses.asdict(e.mesh_quality_motion(**M_THR)), dataclasses.asdict(decomposed_mesh_quality_motion([m], **M_THR))))
    for serial, q in pairs:
        for k, v in serial.items():
            assert type(q[k]) is type(v) and (q[k] == v if isinstance(v, int) else q[k].hex() == v.hex()), (k, q[k], v)


def test_coupled_fields_match_serial_fields():
    """all nine fields through the proc addressing: every element once, every processor face twice, both copies the serial value"""
    m, subs = _case("bfs")
    e = _engine(m)
    ms = _local(subs, "com")
    nProc = sum(p.nFaces for s in subs for p in s.mesh.patches if p.type == "processor") // 2
    for name in GEOMETRY_FIELDS + MOTION_FIELDS:
        geo = name in GEOMETRY_FIELDS
        ref = e.quality_geometry_field(name) if geo else e.quality_motion_field(name)
        per = ms.quality_geometry_field(name) if geo else ms.quality_motion_field(name)
        addr = [s.cellProcAddressing if name.startswith("cell") else s.faceProcAddressing for s in subs]
        seen = np.zeros(len(ref), np.int64)
        tol = ALLOWED_DIFF if name in NEW_FORMULA_FIELDS else 1e-13
        worst = 0.0
        for a, v in zip(addr, per):
            assert v.shape == a.shape
            worst = max(worst, float(np.max(np.abs(v - ref[a]) / np.maximum(np.abs(ref[a]), 1.0))))
            np.add.at(seen, a, 1)
        print(f"    {name}: max difference {worst:.3e} (allowed {tol:.1e})")
        assert worst <= tol, (name, worst)
        assert seen.min() == 1
        if name.startswith("face"):
            assert seen.max() == 2 and (seen == 2).sum() == nProc
            if name in ("faceWeight", "faceVolumeRatio"):      # a processor face is an internal face: not the boundary value 1
                assert np.all(ref[seen == 2] < 1.0)


def test_processor_boundary_cell_keeps_its_determinant():
    """the uniform block: a cell with all six faces internal or processor faces has det = 1; the serial-only rule would drop a face"""
    from smoothmesh_amd.decompose import decompose, grid_partition
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(6, 6, 6)
    subs = decompose(m, grid_partition(m, (2, 1, 1)), 2)
    serial = _engine(m).quality_geometry_field("cellDeterminant")
    per = _local(subs, "com").quality_geometry_field("cellDeterminant")
    seen = 0
    for s, det in zip(subs, per):
        sm = s.mesh
        onProc = np.zeros(sm.nCells, bool)
        for p in sm.patches:
            if p.type == "processor":
                onProc[sm.owner[p.startFace:p.startFace + p.nFaces]] = True
        pick = onProc & (np.abs(serial[s.cellProcAddressing] - 1.0) <= 1e-13)
        seen += int(pick.sum())
        assert np.max(np.abs(det[pick] - 1.0)) <= 1e-13
        assert np.max(np.abs(det - serial[s.cellProcAddressing])) <= 1e-13
    assert seen == 32


def test_reports_between_iterations_leave_the_loop_untouched():
    from smoothmesh_amd import default_params
    from smoothmesh_amd.halo import LocalMultiSmoother
    m, subs = _case("grid")
    runs = []
    for with_report in (False, True):
        ms = LocalMultiSmoother(subs, device=0)
        ms.set_params(default_params(ms.global_min_edge()))         # constraints on
        if with_report:
            n1, r1, f1 = ms.iterate(5, 0.0)
            g1, g2 = ms.mesh_quality_geometry(**G_THR), ms.mesh_quality_geometry(**G_THR)
            t1, t2 = ms.mesh_quality_motion(**M_THR), ms.mesh_quality_motion(**M_THR)
            for a, b in ((g1, g2), (t1, t2)):                         # two consecutive reports: bit-equal
                assert all((x.hex() == y.hex()) if isinstance(x, float) else x == y
                           for x, y in zip(dataclasses.astuple(a), dataclasses.astuple(b)))
            e = _engine(m)
            e.set_points(_gather_points(subs, ms.get_points(), m.nPoints))
            for q, ser in ((g1, e.mesh_quality_geometry(**G_THR)), (t1, e.mesh_quality_motion(**M_THR))):
                ser = dataclasses.asdict(ser)
                for k in GEOMETRY_EXACT + MOTION_EXACT:
                    if k in ser and not k.endswith(("Face", "Cell")):
                        assert getattr(q, k) == ser[k], k
            ms.quality_geometry_field("faceVolumeRatio")
            ms.quality_motion_field("faceTwist")
            n2, r2, f2 = ms.iterate(5, 0.0)
            n, res, frz = n1 + n2, np.concatenate([r1, r2]), np.concatenate([f1, f2])
        else:
            n, res, frz = ms.iterate(10, 0.0)
        runs.append((n, res, frz, ms.get_points()))
    (na, ra, fa, pa), (nb, rb, fb, pb) = runs
    assert na == nb == 10
    assert ra.tobytes() == rb.tobytes() and np.array_equal(fa, fb)
    for a, b in zip(pa, pb):
        assert a.tobytes() == b.tobytes()
    assert fa.max() > 0                                               # frozen points present


def test_refusals():
    import torch
    from smoothmesh_amd import SmgpuError, SmoothEngine
    from smoothmesh_amd.quality import local_exchange, paired_offsets
    m, subs = _case("grid")
    engines = [SmoothEngine(s.mesh) for s in subs]
    dev = torch.device("cuda", 0)
    couplings = [e.quality_coupling(r) for r, e in enumerate(engines)]
    e = engines[0]
    with pytest.raises(SmgpuError, match="smgpu_quality_coupled_pack first"):         # nothing packed yet
        e.quality_coupled_motion_report(0)
    recv = local_exchange(engines, couplings, dev)
    with pytest.raises(SmgpuError, match="smgpu_quality_coupled_pack_volumes"):       # the geometry report needs the volumes
        e.quality_coupled_geometry_report(recv[0].data_ptr(), recv[0].data_ptr())
    with pytest.raises(SmgpuError, match="smgpu_quality_coupled_pack_volumes"):
        e.quality_coupled_geometry_field("faceWeight", recv[0].data_ptr(), recv[0].data_ptr())
    e.quality_coupled_motion_report(recv[0].data_ptr())                               # the motion report does not
    recv, recvV = local_exchange(engines, couplings, dev, volumes=True)
    e.quality_coupled_geometry_report(recv[0].data_ptr(), recvV[0].data_ptr())
    with pytest.raises(SmgpuError, match="null recvVc"):
        e.quality_coupled_geometry_report(recv[0].data_ptr(), 0)
    with pytest.raises(SmgpuError, match="unknown quality motion field"):
        e.quality_coupled_motion_field("faceSkewness", recv[0].data_ptr())
    rank, pats = couplings[0]                                                         # a pack with another coupling lays the slots out
    assert len(pats) >= 2                                                             # anew: the volumes of the old one no longer fit
    send = torch.empty((sum(p[1] for p in pats), 3), dtype=torch.float64, device=dev)
    e.quality_coupled_pack(couplings[0], send.data_ptr())                             # (the same coupling again keeps them)
    e.quality_coupled_geometry_report(recv[0].data_ptr(), recvV[0].data_ptr())
    e.quality_coupled_pack((rank, pats[::-1]), send.data_ptr())
    with pytest.raises(SmgpuError, match="smgpu_quality_coupled_pack_volumes"):
        e.quality_coupled_geometry_report(recv[0].data_ptr(), recvV[0].data_ptr())
    with pytest.raises(SmgpuError, match="smgpu_quality_coupled_pack_volumes"):
        e.quality_coupled_geometry_field("faceVolumeRatio", recv[0].data_ptr(), recvV[0].data_ptr())
    e.quality_coupled_pack(couplings[0], send.data_ptr())
    e.quality_coupled_pack_volumes(torch.empty(send.shape[0], dtype=torch.float64, device=dev).data_ptr())
    e.quality_coupled_geometry_report(recv[0].data_ptr(), recvV[0].data_ptr())
    e.set_points(e.get_points())                                                      # the points may have moved: a new pack is due
    for call in (lambda: e.quality_coupled_geometry_report(recv[0].data_ptr(), recvV[0].data_ptr()),
                 lambda: e.quality_coupled_motion_report(recv[0].data_ptr()),
                 lambda: e.quality_coupled_geometry_field("faceWeight", recv[0].data_ptr(), recvV[0].data_ptr()),
                 lambda: e.quality_coupled_motion_field("faceTwist", recv[0].data_ptr()),
                 lambda: e.quality_coupled_pack_volumes(recvV[0].data_ptr())):
        with pytest.raises(SmgpuError, match="smgpu_quality_coupled_pack first"):
            call()
    with pytest.raises(ValueError):                                                   # a mismatched patch pairing
        paired_offsets(couplings[:1])
    rank, pats = couplings[1]
    with pytest.raises(ValueError):
        paired_offsets([couplings[0], (rank, [(s, n - 1, o) for s, n, o in pats])] + couplings[2:])
    for x in engines:
        x.close()


@pytest.mark.parametrize("world", [2, 3])
def test_distributed_reports_equal_local(tmp_path, world):
    from smoothmesh_amd import default_params
    from smoothmesh_amd.decompose import bfs_partition, decompose
    from smoothmesh_amd.halo import LocalMultiSmoother
    from smoothmesh_amd.meshgen import hex_block
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, SMOOTHMESH_SHARE_GPU="1", SMOOTHMESH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "scripts", "check_dist_quality_geometry_motion.py"), str(tmp_path),
                        json.dumps({"geometry": G_THR, "motion": M_THR})], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = hex_block(12, 10, 8, jitter=0.3, seed=31)
    subs = decompose(m, bfs_partition(m, world, seed=2), world)
    ms = LocalMultiSmoother(subs, device=0)
    ms.set_params(default_params(ms.global_min_edge()))
    both = lambda: {"geometry": dataclasses.asdict(ms.mesh_quality_geometry(**G_THR)),  # noqa: E731
                    "motion": dataclasses.asdict(ms.mesh_quality_motion(**M_THR))}
    want = {"before": both()}
    ms.iterate(3, 0.0)
    want["after"] = both()
    want = {k: {w: {n: (v.hex() if isinstance(v, float) else v) for n, v in d.items()} for w, d in r_.items()} for k, r_ in want.items()}
    for rk in range(world):
        with open(tmp_path / f"rank{rk}.json") as f:
            assert json.load(f) == want, rk


def test_decomposed_case_quality(tmp_path):
    from smoothmesh_amd.check_quality import decomposed_case_quality
    from smoothmesh_amd.decompose import decompose, grid_partition
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import write_decomposed_case
    from smoothmesh_amd.quality import format_report
    m = hex_block(10, 9, 8, jitter=0.3, seed=4)
    write_decomposed_case(str(tmp_path / "d"), decompose(m, grid_partition(m, (2, 2, 1)), 4), binary=True)
    q, g, t = decomposed_case_quality(str(tmp_path / "d"), time="constant", all_geometry=True, mesh_quality=True)
    e = _engine(m)
    gs, ts = e.mesh_quality_geometry(), e.mesh_quality_motion()
    _assert_report(g, dataclasses.asdict(gs), GEOMETRY_EXACT)
    _assert_report(t, dataclasses.asdict(ts), MOTION_EXACT)
    lines = format_report(q, "mesh", g, t).splitlines()
    assert [ln.split()[0] for ln in lines[-10:-1]] == ["faceConcavity", "faceFlatness", "faceWeight", "volumeRatio", "cellDeterminant",
                                                         "faceTets", "faceBaseTets", "faceTwist", "triangleTwist"]
    assert decomposed_case_quality(str(tmp_path / "d"), time="constant")[1:] == (None, None)
