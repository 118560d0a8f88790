"""Mesh quality report of a decomposed mesh on the GPU (include/smgpu.h smgpu_quality_coupled_*, smoothmesh_amd/quality.py,
DESIGN.md "Mesh quality", 10.4): the combined report of the sub-domains equals the serial engine's report of the undecomposed
mesh, through every driver (decomposed_mesh_quality, LocalMultiSmoother, DistributedSmoother, check_quality)."""
import dataclasses
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_quality import BIN, FIELDS, _assert_report, _assert_well_posed, _engine, _parse_blocks, _run
from test_quality_reference import reference_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(kind):
    from smoothmesh_amd.decompose import bfs_partition, decompose, grid_partition, random_partition
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import cavity_mesh
    if kind == "cavity":
        m = cavity_mesh(40, jitter=0.2, seed=8)
        return m, decompose(m, grid_partition(m, (2, 2, 2)), 8)
    m = hex_block(12, 10, 8, jitter=0.3, seed=31)
    if kind == "grid":
        return m, decompose(m, grid_partition(m, (2, 2, 1)), 4)
    if kind == "bfs":
        return m, decompose(m, bfs_partition(m, 5, seed=2), 5)
    return m, decompose(m, random_partition(m, 4, seed=6), 4)


def _local(subs, variant):
    from smoothmesh_amd.halo import LocalMultiSmoother
    ms = LocalMultiSmoother(subs, device=0)
    for st in ms.states:
        st.eng.set_foam_variant(variant)
    return ms


@pytest.mark.parametrize("variant", ["com", "org"])
@pytest.mark.parametrize("kind", ["grid", "bfs", "random", "cavity"])
def test_decomposed_report_equals_serial(oracle_lib, kind, variant):
    from smoothmesh_amd.quality import decomposed_mesh_quality
    m, subs = _case(kind)
    rep, f = reference_of(oracle_lib, m, variant)
    _assert_well_posed(rep, f)
    serial = dataclasses.asdict(_engine(m, variant).mesh_quality())
    scale = float(f["cellAbsPyramids"].sum())
    q = decomposed_mesh_quality(subs, foam_variant=variant)
    _assert_report(q, serial, scale)
    _assert_report(q, rep, scale)
    ql = _local(subs, variant).mesh_quality()
    _assert_report(ql, serial, scale)
    assert dataclasses.asdict(ql) == dataclasses.asdict(q)          # the same engines' records, the same combine


def test_single_subdomain_is_bitwise_the_serial_report():
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.quality import decomposed_mesh_quality
    m = hex_block(11, 9, 7, jitter=0.3, seed=5)
    serial = dataclasses.asdict(_engine(m).mesh_quality())
    q = dataclasses.asdict(decomposed_mesh_quality([m]))
    for k, v in serial.items():
        assert type(q[k]) is type(v) and (q[k] == v if isinstance(v, int) else q[k].hex() == v.hex()), (k, q[k], v)


def test_coupled_fields_match_serial_fields():
    m, subs = _case("bfs")
    e = _engine(m)
    ms = _local(subs, "com")
    for name in FIELDS:
        ref = e.quality_field(name)
        per = ms.quality_field(name)
        addr = [s.cellProcAddressing if name.startswith("cell") else s.faceProcAddressing for s in subs]
        seen = np.zeros(len(ref), np.int64)
        for a, v in zip(addr, per):
            assert v.shape == a.shape
            if name == "faceNonOrthogonality":
                # the sub-domain's cell centres differ from the serial ones in the last bits (other face order, reversed processor
                # faces), and acos amplifies that by 1 / sin(theta) near theta = 0: compare the cosines
                err = np.abs(np.cos(np.radians(v)) - np.cos(np.radians(ref[a])))
            else:
                err = np.abs(v - ref[a]) / np.maximum(np.abs(ref[a]), 1.0)
            assert err.max() <= 1e-13, (name, float(err.max()))
            np.add.at(seen, a, 1)
        assert seen.min() == 1
        if name.startswith("face"):            # every processor face on both sides, both copies agree with the serial value
            assert seen.max() == 2 and (seen == 2).sum() == sum(p.nFaces for s in subs for p in s.mesh.patches if p.type == "processor") // 2


def _gather_points(subs, parts, nPoints):
    pts = np.zeros((nPoints, 3))
    for s, p in zip(subs, parts):
        pts[s.pointProcAddressing] = p
    return pts


def test_report_between_iterations_leaves_the_loop_untouched():
    from smoothmesh_amd import default_params
    from smoothmesh_amd.halo import LocalMultiSmoother
    m, subs = _case("grid")
    runs = []
    for with_report in (False, True):
        ms = LocalMultiSmoother(subs, device=0)
        ms.set_params(default_params(ms.global_min_edge()))         # constraints on
        if with_report:
            n1, r1, f1 = ms.iterate(5, 0.0)
            q1, q2 = ms.mesh_quality(), ms.mesh_quality()
            assert dataclasses.asdict(q1) == dataclasses.asdict(q2)
            e = _engine(m)
            e.set_points(_gather_points(subs, ms.get_points(), m.nPoints))
            serial = dataclasses.asdict(e.mesh_quality())
            vol = float(np.sum(np.abs(e.quality_field("cellVolume"))))
            _assert_report(q1, serial, vol)
            for name in FIELDS:
                ms.quality_field(name)
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
    assert fa.max() > 0


@pytest.mark.parametrize("world", [2, 3])
def test_distributed_report_equals_local(tmp_path, world):
    from smoothmesh_amd import default_params
    from smoothmesh_amd.decompose import bfs_partition, decompose
    from smoothmesh_amd.halo import LocalMultiSmoother
    from smoothmesh_amd.meshgen import hex_block
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, SMOOTHMESH_SHARE_GPU="1", SMOOTHMESH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "scripts", "check_dist_quality.py"), str(tmp_path)],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = hex_block(12, 10, 8, jitter=0.3, seed=31)
    subs = decompose(m, bfs_partition(m, world, seed=2), world)
    ms = LocalMultiSmoother(subs, device=0)
    ms.set_params(default_params(ms.global_min_edge()))
    want = {"before": dataclasses.asdict(ms.mesh_quality())}
    ms.iterate(3, 0.0)
    want["after"] = dataclasses.asdict(ms.mesh_quality())
    want = {k: {n: (v.hex() if isinstance(v, float) else v) for n, v in d.items()} for k, d in want.items()}
    for rk in range(world):
        with open(tmp_path / f"rank{rk}.json") as f:
            assert json.load(f) == want, rk


def test_check_quality_tool(tmp_path):
    from smoothmesh_amd.decompose import decompose, grid_partition
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import write_case, write_decomposed_case
    m = hex_block(10, 9, 8, jitter=0.3, seed=4)
    write_case(str(tmp_path / "s"), m, binary=True, writeFormat="binary")
    write_case(str(tmp_path / "c"), m, binary=True, writeFormat="binary")
    write_decomposed_case(str(tmp_path / "d"), decompose(m, grid_partition(m, (2, 2, 1)), 4), binary=True)
    tool = lambda *a: subprocess.run([sys.executable, "-m", "smoothmesh_amd.check_quality", *a], capture_output=True, text=True,  # noqa: E731
                                     cwd=ROOT, timeout=300)
    r = tool("-case", str(tmp_path / "s"))
    assert r.returncode == 0, r.stderr[-3000:]
    cli = _run(tmp_path / "c", ["-centroidalIters", "1", "-relTol", "0", "-checkQuality", "true"]).stdout.splitlines()
    i = cli.index("Mesh quality (initial mesh):")
    got = r.stdout.splitlines()
    assert got[0] == "Mesh quality (mesh):"
    assert got[1:] == cli[i + 1:i + len(got)], (got, cli[i:i + len(got)])
    r = tool("-case", str(tmp_path / "d"), "-parallel", "-time", "constant")
    assert r.returncode == 0, r.stderr[-3000:]
    a, b = _parse_blocks("\n".join(got))["mesh"], _parse_blocks(r.stdout)["mesh"]
    for k, v in a.items():
        if isinstance(v, float):
            assert abs(b[k] - v) <= 1e-8 * max(abs(v), 1e-300) or (k == "maxOpenness" and abs(b[k] - v) <= 1e-14), (k, b[k], v)
        else:
            assert b[k] == v, (k, b[k], v)
    assert os.path.exists(BIN)
