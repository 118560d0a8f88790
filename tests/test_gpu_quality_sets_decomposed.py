"""smgpu_quality_coupled_sets on the MI355X (DESIGN.md "Mesh quality", 10.5): the sets of a decomposed mesh, rank by rank with
local ids, mapped through the addressing, against the serial engine's sets of the undecomposed mesh; the drivers
decomposed_quality_sets, LocalMultiSmoother and DistributedSmoother; python -m smoothmesh_amd.check_quality -writeSets."""
import dataclasses
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_quality_sets import OTHER, _assert_well_posed, _engine
from test_quality_sets_reference import NAMES, sets_reference_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(kind):
    from smoothmesh_amd.decompose import bfs_partition, decompose, grid_partition, random_partition
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import cavity_mesh
    if kind == "cavity8":
        m = cavity_mesh(30, jitter=0.2, seed=8)
        return m, decompose(m, grid_partition(m, (2, 2, 2)), 8)
    m = hex_block(13, 10, 8, jitter=0.4, seed=31)
    if kind == "grid2":
        return m, decompose(m, grid_partition(m, (2, 1, 1)), 2)
    if kind == "grid4":
        return m, decompose(m, grid_partition(m, (2, 2, 1)), 4)
    if kind == "bfs5":
        return m, decompose(m, bfs_partition(m, 5, seed=2), 5)
    return m, decompose(m, random_partition(m, 4, seed=6), 4)


def _assert_rank_sets(subs, ranks, serial, combined=None):
    """mapped to global ids the ranks' sets are disjoint and their union is the serial set; sizes sum to the combined counts;
    a processor face is a member only on the lower rank"""
    from smoothmesh_amd.quality import QUALITY_SETS
    for name, cls, counts, _ in QUALITY_SETS:
        addr = [s.faceProcAddressing if cls == "faceSet" else s.cellProcAddressing for s in subs]
        mapped = np.concatenate([np.asarray(a)[r[name]] for a, r in zip(addr, ranks)]).astype(np.int64)
        assert len(np.unique(mapped)) == len(mapped), name
        assert np.array_equal(np.sort(mapped), serial[name].astype(np.int64)), name
        for r in ranks:
            assert np.all(np.diff(r[name]) > 0), name
        if combined is not None:
            assert sum(len(r[name]) for r in ranks) == sum(combined[c] for c in counts), name
    for s, r in zip(subs, ranks):
        for p in s.mesh.patches:
            if p.type == "processor" and p.neighbProcNo < s.rank:
                for name, cls, _, _ in QUALITY_SETS[:4]:
                    ids = r[name]
                    assert not np.any((ids >= p.startFace) & (ids < p.startFace + p.nFaces)), (name, s.rank, p.name)


@pytest.mark.parametrize("variant", ["com", "org"])
@pytest.mark.parametrize("thr", ["default", "other"])
@pytest.mark.parametrize("kind", ["grid2", "grid4", "bfs5", "random4", "cavity8"])
def test_decomposed_sets_equal_serial(oracle_lib, kind, thr, variant):
    from smoothmesh_amd.halo import LocalMultiSmoother
    from smoothmesh_amd.quality import decomposed_mesh_quality, decomposed_quality_sets
    t = {} if thr == "default" else OTHER
    m, subs = _case(kind)
    rep, f, want = sets_reference_of(oracle_lib, m, variant, **t)
    _assert_well_posed(f, m.nInternalFaces, **t)
    serial = _engine(m, variant).quality_sets(**t)
    for k in NAMES:
        assert np.array_equal(serial[k], want[k]), k
    ranks = decomposed_quality_sets(subs, foam_variant=variant, **t)
    assert len(ranks) == len(subs) and all(list(r) == list(NAMES) for r in ranks)
    combined = dataclasses.asdict(decomposed_mesh_quality(subs, foam_variant=variant, **t))
    _assert_rank_sets(subs, ranks, serial, combined)
    if thr == "other":
        assert sum(len(r["nonOrthoFaces"]) for r in ranks) > 0
    ms = LocalMultiSmoother(subs, device=0)
    for st in ms.states:
        st.eng.set_foam_variant(variant)
    local = ms.quality_sets(**t)
    for a, b in zip(local, ranks):
        for k in NAMES:
            assert a[k].tobytes() == b[k].tobytes(), k


def test_sets_between_iterations_leave_the_loop_untouched():
    from smoothmesh_amd import default_params
    from smoothmesh_amd.halo import LocalMultiSmoother
    m, subs = _case("grid4")
    runs = []
    for with_sets in (False, True):
        ms = LocalMultiSmoother(subs, device=0)
        ms.set_params(default_params(ms.global_min_edge()))
        if with_sets:
            n1, r1, f1 = ms.iterate(5, 0.0)
            a, b = ms.quality_sets(**OTHER), ms.quality_sets(**OTHER)
            for x, y in zip(a, b):
                assert all(x[k].tobytes() == y[k].tobytes() for k in NAMES)
            n2, r2, f2 = ms.iterate(5, 0.0)
            n, res, frz = n1 + n2, np.concatenate([r1, r2]), np.concatenate([f1, f2])
        else:
            n, res, frz = ms.iterate(10, 0.0)
        runs.append((n, res, frz, ms.get_points()))
    (na, ra, fa, pa), (nb, rb, fb, pb) = runs
    assert na == nb == 10
    assert ra.tobytes() == rb.tobytes() and np.array_equal(fa, fb)
    for x, y in zip(pa, pb):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("world", [2, 4])
def test_distributed_sets_equal_local(tmp_path, world):
    from smoothmesh_amd import default_params
    from smoothmesh_amd.decompose import decompose, grid_partition
    from smoothmesh_amd.halo import LocalMultiSmoother
    from smoothmesh_amd.meshgen import hex_block
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, SMOOTHMESH_SHARE_GPU="1", SMOOTHMESH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "scripts", "check_dist_quality_sets.py"), str(tmp_path)],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    thr = dict(nonOrthThreshold=25.0, skewThreshold=0.35, aspectThreshold=2.2)
    m = hex_block(12, 10, 8, jitter=0.4, seed=31)
    subs = decompose(m, grid_partition(m, (world, 1, 1)), world)
    ms = LocalMultiSmoother(subs, device=0)
    ms.set_params(default_params(ms.global_min_edge()))
    before = ms.quality_sets(**thr)
    ms.iterate(3, 0.0)
    after = ms.quality_sets(**thr)
    assert sum(len(v) for v in before[0].values()) > 0
    for rk in range(world):
        got = np.load(tmp_path / f"sets{rk}.npz")
        for k in NAMES:
            assert got[f"before_{k}"].tobytes() == before[rk][k].tobytes(), (rk, k)
            assert got[f"after_{k}"].tobytes() == after[rk][k].tobytes(), (rk, k)


def test_check_quality_write_sets(tmp_path):
    from smoothmesh_amd.decompose import decompose, grid_partition
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import read_label_list, write_case, write_decomposed_case
    from smoothmesh_amd.quality import QUALITY_SETS, decomposed_quality_sets
    m = hex_block(10, 9, 4, lengths=(1.0, 1.0, 2e-5), jitter=0.3, seed=4)         # flat: high aspect ratio cells
    subs = decompose(m, grid_partition(m, (2, 2, 1)), 4)
    write_case(str(tmp_path / "s"), m, binary=True, writeFormat="binary")
    write_decomposed_case(str(tmp_path / "d"), subs, binary=True)
    tool = lambda *a: subprocess.run([sys.executable, "-m", "smoothmesh_amd.check_quality", *a], capture_output=True, text=True,  # noqa: E731
                                     cwd=ROOT, timeout=300)
    desc = {n: d for n, _, _, d in QUALITY_SETS}
    # serial: into constant/polyMesh/sets, the engine's sets
    r = tool("-case", str(tmp_path / "s"), "-writeSets")
    assert r.returncode == 0, r.stderr[-3000:]
    want = _engine(m).quality_sets()
    assert len(want["highAspectRatioCells"]) > 0
    d = tmp_path / "s" / "constant" / "polyMesh" / "sets"
    assert sorted(os.listdir(d)) == sorted(k for k in NAMES if len(want[k]))
    for k in os.listdir(d):
        assert np.array_equal(read_label_list(str(d / k)), want[k]), k
    lines = r.stdout.splitlines()
    assert lines[9] == "" or lines[10] == ""
    assert [x for x in lines if "<<Writing" in x] == [f"    <<Writing {len(want[k])} {desc[k]} to set {k}" for k in NAMES if len(want[k])]
    # -parallel: into every processorN/constant/polyMesh/sets, local ids
    r = tool("-case", str(tmp_path / "d"), "-parallel", "-writeSets")
    assert r.returncode == 0, r.stderr[-3000:]
    ranks = decomposed_quality_sets(subs)
    n = 0
    for s, rs in zip(subs, ranks):
        d = tmp_path / "d" / f"processor{s.rank}" / "constant" / "polyMesh" / "sets"
        names = sorted(k for k in NAMES if len(rs[k]))
        if names:
            assert sorted(os.listdir(d)) == names, s.rank
        else:
            assert not os.path.exists(d), s.rank
        for k in names:
            assert np.array_equal(read_label_list(str(d / k)), rs[k]), (s.rank, k)
            n += 1
    assert len([x for x in r.stdout.splitlines() if "<<Writing" in x]) == n
    assert not os.path.exists(tmp_path / "d" / "constant")
