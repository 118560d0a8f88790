"""The set-up leaves the same tables on the device as the commit before its stages were named: per configuration the checksums of
the addressing, the checksums of every tile table and the engine's device bytes (an array adopted twice, or not at all, moves
that count) against tests/golden/setup_checksums.json, which scripts/record_setup_checksums.py wrote from a build of that commit.
Equality, no tolerance."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "setup_checksums.json")
KNOBS = ("SMGPU_DEVICE_TOPOLOGY", "SMGPU_DEVICE_TILES", "SMGPU_TILE_SHARE", "SMGPU_GEOM_T", "SMGPU_SMOOTH_T", "SMGPU_FILTER")

with open(GOLDEN) as _f:
    _golden = json.load(_f)
CASES = _golden["cases"]      # per case: mesh, env, deviceBytes and the indices of its two lists of checksums in "lists"

_made = {}


def mesh_of(name):
    """a jittered hex block of 720 cells, the cavity mesh with hanging nodes, the hedgehog (test_gpu_topology.py's meshes)"""
    if name not in _made:
        from smoothmesh_amd.meshgen import hex_block
        from smoothmesh_amd.polymesh import cavity_mesh
        from test_gpu_topology import _hedgehog
        _made[name] = {"hex": lambda: hex_block(10, 9, 8, jitter=0.2, seed=7), "cavity": lambda: cavity_mesh(16, jitter=0.2, seed=3),
                       "hedgehog": _hedgehog}[name]()
    return _made[name]


def recorded(mesh, **env):
    """the recording of one configuration (also for tests/test_gpu_create_errors.py)"""
    hit = [c for c in CASES if c["mesh"] == mesh and c["env"] == env]
    assert len(hit) == 1, (mesh, env)
    return hit[0]


def measure(mesh):
    from smoothmesh_amd import SmoothEngine
    e = SmoothEngine(mesh_of(mesh))
    got = {"addressing": "".join(f"{x:016x}" for x in e.debug_addressing_checksums()), "tiles": "".join(f"{x:016x}" for x in e.debug_tile_checksums()),
           "deviceBytes": int(e.sizes()["deviceBytes"])}
    e.close()
    return got


def expected(case):
    return {"addressing": _golden["lists"][case["addressing"]], "tiles": _golden["lists"][case["tiles"]], "deviceBytes": case["deviceBytes"]}


def test_the_recording_covers_the_configurations():
    seen = {(c["mesh"], tuple(sorted(c["env"].items()))) for c in CASES}
    for mesh in ("hex", "cavity", "hedgehog"):
        for topo in "10":
            for tiles in "102":
                for share in "10":
                    assert (mesh, (("SMGPU_DEVICE_TILES", tiles), ("SMGPU_DEVICE_TOPOLOGY", topo), ("SMGPU_TILE_SHARE", share))) in seen
    for T in ("64", "128"):
        assert ("hex", (("SMGPU_GEOM_T", T), ("SMGPU_SMOOTH_T", T))) in seen
    assert ("hex", (("SMGPU_FILTER", "0"),)) in seen


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["mesh"] + "-" + "-".join(k[6:].lower() + v for k, v in c["env"].items()))
def test_setup_equals_the_parent(case, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    got, want = measure(case["mesh"]), expected(case)
    for what in ("addressing", "tiles", "deviceBytes"):
        assert got[what] == want[what], (case["mesh"], case["env"], what)
    assert got["tiles"].strip("0") and got["addressing"].strip("0")
