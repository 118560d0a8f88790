"""The host side of the boundary revert switch (DESIGN.md "Mesh quality", 10.21), without a GPU: the two entries in the header, in
the ctypes table and in the library, and what `smoothMesh -boundaryRevert` refuses or lets stand before the engine is created."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "smoothmesh_amd", "bin", "smoothMesh")
OLD = {
    "-tangleConstraint": "-tangleConstraint is not available with boundary point smoothing: it rewrites the boundary points from state that a reverted "
                         "iteration would leave ahead of the points (run without -smoothingPatches, or without the constraint)",
    "-qualityConstraint": "-qualityConstraint is not available with boundary point smoothing: it rewrites the boundary points from state that a reverted "
                          "iteration would leave ahead of the points (run without -smoothingPatches, or without the constraint)",
    "-qualityGuard": "-qualityGuard is not available with boundary point smoothing: the point normals it blends from iteration to iteration and "
                     "its corner lists are not part of the guard's snapshot (run without -smoothingPatches, or without the guard)",
}


def test_prototypes():
    from smoothmesh_amd import _ffi
    from smoothmesh_amd.engine import SmoothEngine
    assert _ffi.SYMBOLS["smgpu_set_boundary_revert"] == (C.c_int, [C.c_void_p, C.c_int32])
    assert _ffi.SYMBOLS["smgpu_get_boundary_revert"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)])
    header = open(os.path.join(ROOT, "include", "smgpu.h")).read()
    assert re.search(r"^int smgpu_set_boundary_revert\(smgpu_handle\* h, int32_t on\);", header, re.M)
    assert re.search(r"^int smgpu_get_boundary_revert\(smgpu_handle\* h, int32_t\* on\);", header, re.M)
    lib = _ffi.lib()                                               # the library exports them
    assert lib.smgpu_set_boundary_revert and lib.smgpu_get_boundary_revert
    assert callable(SmoothEngine.set_boundary_revert) and callable(SmoothEngine.boundary_revert)
    # a null handle is an error, not a crash
    assert lib.smgpu_set_boundary_revert(None, 1) != 0 and lib.smgpu_get_boundary_revert(None, None) != 0


def _case(tmp_path, geometry):
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import write_case
    write_case(str(tmp_path), hex_block(4))
    if geometry:
        geo = tmp_path / "constant" / "geometry"
        geo.mkdir()
        (geo / "targetSurfaces.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
        (geo / "initEdges.obj").write_text("v 0 0 0\nv 1 0 0\nl 1 2\n")

    def run(*opts):
        return subprocess.run([BIN, "-case", str(tmp_path)] + list(opts), capture_output=True, text=True, timeout=120)
    return run


def test_cli_option_parsing(tmp_path):
    run = _case(tmp_path, geometry=False)
    before = sorted(os.listdir(tmp_path))
    r = run("-boundaryRevert", "true")
    assert r.returncode != 0 and "-boundaryRevert needs -tangleConstraint true, -qualityConstraint true or -qualityGuard true" in r.stdout + r.stderr
    r = run("-boundaryRevert", "true", "-tangleConstraint", "false")
    assert r.returncode != 0 and "-boundaryRevert needs -tangleConstraint true" in r.stdout + r.stderr
    r = run("-parallel", "-boundaryRevert", "true", "-tangleConstraint", "true")
    assert r.returncode != 0                                        # (-tangleConstraint's own refusal of -parallel comes first)
    r = run("-boundaryRevert", "perhaps", "-tangleConstraint", "true")
    assert r.returncode != 0 and "-boundaryRevert" in r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path)) == before
    h = subprocess.run([BIN, "-help"], capture_output=True, text=True, timeout=120)
    assert "-boundaryRevert" in h.stdout


def test_cli_without_the_option_every_refusal_stands(tmp_path):
    run = _case(tmp_path, geometry=True)
    trace = ("-checkQuality", "true", "-qualityInterval", "2")
    for opt, text in OLD.items():
        for extra in ((), ("-boundaryRevert", "false")):
            r = run(opt, "true", *(trace if opt == "-qualityGuard" else ()), *extra)
            assert r.returncode != 0 and text in r.stdout + r.stderr, (opt, extra)
    assert not any(x.isdigit() and x != "0" for x in os.listdir(tmp_path))


def test_cli_scaling_passes_stay_refused(tmp_path):
    run = _case(tmp_path, geometry=True)
    r = run("-qualityConstraint", "true", "-boundaryRevert", "true", "-scalePasses", "2")
    assert r.returncode != 0
    assert "scaling passes with boundary point smoothing are not available (a scaled boundary point leaves the target surface)" in r.stdout + r.stderr
    assert not any(x.isdigit() and x != "0" for x in os.listdir(tmp_path))
