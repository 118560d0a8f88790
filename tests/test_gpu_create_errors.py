"""smgpu_create's ways out on failure: each an ordinary error return with its own text, after which the next create in the same
process succeeds and gives the tables of tests/golden/setup_checksums.json -- and the device memory of a failed create comes back
(a create that fails at the tile shapes has by then adopted the addressing and has an edge-tile task in flight)."""
import ctypes as C

import pytest

from test_gpu_setup_equals_parent import expected, measure, mesh_of, recorded

pytestmark = pytest.mark.gpu

KNOBS = ("SMGPU_TILES", "SMGPU_GEOM_T", "SMGPU_SMOOTH_T", "SMGPU_DEVICE_TOPOLOGY", "SMGPU_DEVICE_TILES", "SMGPU_TILE_SHARE", "SMGPU_FILTER")


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _default_tables():
    return expected(recorded("hex", SMGPU_DEVICE_TOPOLOGY="1", SMGPU_DEVICE_TILES="1", SMGPU_TILE_SHARE="1"))      # (the knobs' defaults)


@pytest.mark.parametrize("knob,text", [("SMGPU_GEOM_T", "SMGPU_GEOM_T must be 64, 128 or 256"), ("SMGPU_SMOOTH_T", "SMGPU_SMOOTH_T must be 64, 128 or 256")])
def test_a_tile_shape_that_does_not_exist(monkeypatch, knob, text):
    from smoothmesh_amd import SmgpuError, SmoothEngine
    monkeypatch.setenv(knob, "100")
    with pytest.raises(SmgpuError, match=text):
        SmoothEngine(mesh_of("hex"))
    monkeypatch.delenv(knob)
    assert measure("hex") == _default_tables()
    monkeypatch.setenv(knob, "100")
    monkeypatch.setenv("SMGPU_TILES", "0")      # without tiles nobody reads the shape
    e = SmoothEngine(mesh_of("hex"))
    assert e.sizes()["deviceBytes"] > 0
    e.close()


def test_invalid_mesh_sizes_through_the_c_abi():
    from smoothmesh_amd import _ffi
    from smoothmesh_amd.engine import make_desc
    lib = _ffi.lib()
    mesh = mesh_of("hex")
    d, keep = make_desc(mesh, mesh.find_internal_points(), None)
    d.nInternalFaces = d.nFaces + 1
    h = C.c_void_p()
    assert lib.smgpu_create(C.byref(d), C.byref(h)) != 0
    assert lib.smgpu_last_error().decode() == "smgpu_create: invalid mesh sizes"
    assert not h.value
    del keep
    assert measure("hex") == _default_tables()


def test_device_ordinal_out_of_range():
    import torch
    from smoothmesh_amd import SmgpuError, SmoothEngine
    for device in (-1, torch.cuda.device_count()):
        with pytest.raises(SmgpuError, match="smgpu_create: device ordinal out of range"):
            SmoothEngine(mesh_of("hex"), device=device)
    assert measure("hex") == _default_tables()


def test_failed_creates_give_their_memory_back(monkeypatch):
    """five failing creates and a successful one may not cost more free memory than ONE engine's device bytes -- a leak of the adopted
    addressing alone, five times over, would be several times that"""
    import torch
    from smoothmesh_amd import SmgpuError, SmoothEngine
    from smoothmesh_amd.meshgen import hex_block
    mesh = hex_block(40, 40, 40, jitter=0.2, seed=5)
    internal = mesh.find_internal_points()

    def failing():
        monkeypatch.setenv("SMGPU_GEOM_T", "100")
        with pytest.raises(SmgpuError, match="SMGPU_GEOM_T must be"):
            SmoothEngine(mesh, internal)
        monkeypatch.delenv("SMGPU_GEOM_T")

    failing()      # (warm-up: what the runtime keeps for itself after a first create)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(5):
        failing()
    e = SmoothEngine(mesh, internal)
    one_engine = e.sizes()["deviceBytes"]
    e.close()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    print(f"free before {free0}, after {free1}, drop {free0 - free1}, one engine {one_engine}")
    assert one_engine > 0 and free0 - free1 < one_engine
