"""smgpu_quality_coupled_geometry_sets / _coupled_motion_sets on the MI355X (DESIGN.md "Mesh quality", 10.9): the sets of a
decomposed mesh, rank by rank with local ids, mapped through the addressing, against the numpy restatements of the undecomposed
mesh (tests/test_quality_more_sets_reference.py); the drivers decomposed_quality_geometry_sets / _motion_sets, LocalMultiSmoother
and DistributedSmoother; check_quality.decomposed_case_quality(write_sets=True).  Meshes, decompositions and thresholds are those
of tests/test_gpu_quality_geometry_motion_decomposed.py: every count is positive there, with processor faces among the members."""
import dataclasses
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_quality_decomposed import _local
from test_gpu_quality_geometry import _engine
from test_gpu_quality_geometry_motion_decomposed import G_THR, M_THR, _assert_well_posed, _proc_faces, _refs
from test_quality_more_sets_reference import GEOMETRY_NAMES, MOTION_NAMES, geometry_sets_of_fields, motion_sets_of_fields

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _assert_rank_sets(table, subs, ranks, serial, combined):
    """mapped to global ids the ranks' sets are disjoint and their union is the serial set; ascending local ids; sizes sum to the
    combined report's counts; a processor face is a member only on the side that counts it (the lower rank)"""
    assert len(ranks) == len(subs) and all(list(r) == [n for n, *_ in table] for r in ranks)
    for name, cls, counts, _ in table:
        addr = [s.faceProcAddressing if cls == "faceSet" else s.cellProcAddressing for s in subs]
        mapped = np.concatenate([np.asarray(a)[r[name]] for a, r in zip(addr, ranks)]).astype(np.int64)
        assert len(np.unique(mapped)) == len(mapped), name
        assert np.array_equal(np.sort(mapped), serial[name].astype(np.int64)), name
        for r in ranks:
            assert r[name].dtype == np.int32 and np.all(np.diff(r[name]) > 0), name
        assert sum(len(r[name]) for r in ranks) == sum(combined[c] for c in counts), name
    for s, r in zip(subs, ranks):
        for p in s.mesh.patches:
            if p.type == "processor" and p.neighbProcNo < s.rank:
                for name, cls, _, _ in table:
                    if cls == "faceSet":
                        ids = r[name]
                        assert not np.any((ids >= p.startFace) & (ids < p.startFace + p.nFaces)), (name, s.rank, p.name)


def _tables():
    from smoothmesh_amd.quality import QUALITY_GEOMETRY_SETS, QUALITY_MOTION_SETS
    return QUALITY_GEOMETRY_SETS, QUALITY_MOTION_SETS


@pytest.mark.parametrize("variant", ["com", "org"])
@pytest.mark.parametrize("kind", ["grid", "bfs", "random", "cavity"])
def test_decomposed_sets_equal_serial(kind, variant):
    from smoothmesh_amd.quality import (decomposed_mesh_quality_geometry, decomposed_mesh_quality_motion, decomposed_quality_geometry_sets,
                                        decomposed_quality_motion_sets)
    m, subs, grep, gf, mrep, mf = _refs(kind, variant)
    _assert_well_posed(m, grep, gf, mf)
    want_g, want_m = geometry_sets_of_fields(m, gf, **G_THR), motion_sets_of_fields(mf, **M_THR)
    rg = decomposed_quality_geometry_sets(subs, foam_variant=variant, **G_THR)
    rm = decomposed_quality_motion_sets(subs, foam_variant=variant, **M_THR)
    qg = dataclasses.asdict(decomposed_mesh_quality_geometry(subs, foam_variant=variant, **G_THR))
    qm = dataclasses.asdict(decomposed_mesh_quality_motion(subs, foam_variant=variant, **M_THR))
    _assert_rank_sets(_tables()[0], subs, rg, want_g, qg)
    _assert_rank_sets(_tables()[1], subs, rm, want_m, qm)
    # processor faces among the members: of every thresholded face set on a hex kind, of concaveFaces on the polyhedral mesh
    isProc = _proc_faces(m, subs)
    if kind == "cavity":
        assert isProc[want_g["concaveFaces"]].any()
    else:
        for k in GEOMETRY_NAMES[1:4]:
            assert isProc[want_g[k]].any(), k
        for k in MOTION_NAMES:
            assert isProc[want_m[k]].any(), k
    # the same engines through LocalMultiSmoother: the same bits
    ms = _local(subs, variant)
    for local, ranks in ((ms.quality_geometry_sets(**G_THR), rg), (ms.quality_motion_sets(**M_THR), rm)):
        for a, b in zip(local, ranks):
            assert list(a) == list(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_single_subdomain_gives_the_serial_sets_bitwise():
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.quality import decomposed_quality_geometry_sets, decomposed_quality_motion_sets
    m = hex_block(11, 9, 7, jitter=0.3, seed=5)
    e = _engine(m)
    for serial, ranks in ((e.quality_geometry_sets(**G_THR), decomposed_quality_geometry_sets([m], **G_THR)),
                          (e.quality_motion_sets(**M_THR), decomposed_quality_motion_sets([m], **M_THR))):
        assert len(ranks) == 1 and list(ranks[0]) == list(serial)
        assert sum(len(v) for v in serial.values()) > 0
        for k, v in serial.items():
            assert ranks[0][k].dtype == v.dtype and ranks[0][k].tobytes() == v.tobytes(), k


def test_coupled_sets_refusals():
    import torch
    from smoothmesh_amd import SmgpuError, SmoothEngine
    from smoothmesh_amd.quality import local_exchange
    _, subs = _refs("grid", "com")[:2]
    engines = [SmoothEngine(s.mesh) for s in subs]
    dev = torch.device("cuda", 0)
    couplings = [e.quality_coupling(r) for r, e in enumerate(engines)]
    e = engines[0]
    with pytest.raises(SmgpuError, match="smgpu_quality_coupled_pack first"):         # nothing packed yet
        e.quality_coupled_motion_sets(0)
    recv = local_exchange(engines, couplings, dev)
    with pytest.raises(SmgpuError, match="smgpu_quality_coupled_pack_volumes"):       # the geometry sets need the volumes
        e.quality_coupled_geometry_sets(recv[0].data_ptr(), recv[0].data_ptr())
    assert list(e.quality_coupled_motion_sets(recv[0].data_ptr(), **M_THR)) == list(MOTION_NAMES)      # the motion sets do not
    recv, recvV = local_exchange(engines, couplings, dev, volumes=True)
    assert list(e.quality_coupled_geometry_sets(recv[0].data_ptr(), recvV[0].data_ptr(), **G_THR)) == list(GEOMETRY_NAMES)
    with pytest.raises(SmgpuError, match="null recvVc"):
        e.quality_coupled_geometry_sets(recv[0].data_ptr(), 0)
    e.set_points(e.get_points())                                                      # the points may have moved: a new pack is due
    for call in (lambda: e.quality_coupled_geometry_sets(recv[0].data_ptr(), recvV[0].data_ptr()),
                 lambda: e.quality_coupled_motion_sets(recv[0].data_ptr())):
        with pytest.raises(SmgpuError, match="smgpu_quality_coupled_pack first"):
            call()
    for x in engines:
        x.close()


def test_distributed_sets_equal_local(tmp_path):
    """two gloo ranks: every rank's own sets of both kinds, before and after three iterations, are LocalMultiSmoother's"""
    from smoothmesh_amd import default_params
    from smoothmesh_amd.decompose import bfs_partition, decompose
    from smoothmesh_amd.halo import LocalMultiSmoother
    from smoothmesh_amd.meshgen import hex_block
    world = 2
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, SMOOTHMESH_SHARE_GPU="1", SMOOTHMESH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "scripts", "check_dist_quality_more_sets.py"), str(tmp_path),
                        json.dumps({"geometry": G_THR, "motion": M_THR})], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = hex_block(12, 10, 8, jitter=0.3, seed=31)
    subs = decompose(m, bfs_partition(m, world, seed=2), world)
    ms = LocalMultiSmoother(subs, device=0)
    ms.set_params(default_params(ms.global_min_edge()))
    both = lambda: [{**g, **t} for g, t in zip(ms.quality_geometry_sets(**G_THR), ms.quality_motion_sets(**M_THR))]  # noqa: E731
    before = both()
    ms.iterate(3, 0.0)
    after = both()
    assert all(sum(len(v) for v in b.values()) > 0 for b in before)
    for rk in range(world):
        got = np.load(tmp_path / f"more_sets{rk}.npz")
        for k in GEOMETRY_NAMES + MOTION_NAMES:
            assert got[f"before_{k}"].dtype == np.int32
            assert got[f"before_{k}"].tobytes() == before[rk][k].tobytes(), (rk, k)
            assert got[f"after_{k}"].tobytes() == after[rk][k].tobytes(), (rk, k)


def test_decomposed_case_quality_writes_the_sets(tmp_path):
    from smoothmesh_amd.check_quality import decomposed_case_quality, format_written
    from smoothmesh_amd.decompose import decompose, grid_partition
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import read_label_list, write_decomposed_case
    from smoothmesh_amd.quality import QUALITY_SETS, decomposed_quality_geometry_sets, decomposed_quality_motion_sets, decomposed_quality_sets
    m = hex_block(10, 9, 4, lengths=(1.0, 1.0, 2e-5), jitter=0.3, seed=4)        # flat: every cell under-determined, high aspect ratios
    subs = decompose(m, grid_partition(m, (2, 2, 1)), 4)
    write_decomposed_case(str(tmp_path / "d"), subs, binary=True)
    write_decomposed_case(str(tmp_path / "g"), subs, binary=True)
    (q, g, t), written = decomposed_case_quality(str(tmp_path / "d"), time="constant", all_geometry=True, mesh_quality=True, write_sets=True)
    assert g is not None and t is not None and g.nUnderdeterminedCells == m.nCells
    per = [decomposed_quality_sets(subs), decomposed_quality_geometry_sets(subs), decomposed_quality_motion_sets(subs)]
    tables = (QUALITY_SETS,) + _tables()
    expect = []
    for s in subs:
        d = tmp_path / "d" / f"processor{s.rank}" / "constant" / "polyMesh" / "sets"
        names = []
        for ranks, table in zip(per, tables):
            names += [(n, ranks[s.rank][n]) for n, *_ in table if len(ranks[s.rank][n])]
        assert "underdeterminedCells" in [n for n, _ in names]
        assert sorted(os.listdir(d)) == sorted(n for n, _ in names), s.rank
        for n, ids in names:
            assert np.array_equal(read_label_list(str(d / n)), ids), (s.rank, n)              # local ids
        expect += [(s.rank, n, len(ids)) for n, ids in names]
    assert written == expect                                                             # rank by rank: the seven, geometry, motion
    assert format_written(written).count("<<Writing") == len(expect)
    assert not os.path.exists(tmp_path / "d" / "constant")
    # only the reports asked for; without write_sets the triple alone and no file
    (_, g2, t2), w2 = decomposed_case_quality(str(tmp_path / "g"), time="constant", all_geometry=True, write_sets=True)
    assert g2 is not None and t2 is None
    assert {n for _, n, _ in w2} <= {n for n, *_ in QUALITY_SETS + _tables()[0]} and "underdeterminedCells" in {n for _, n, _ in w2}
    assert len(decomposed_case_quality(str(tmp_path / "g"), time="constant")) == 3
