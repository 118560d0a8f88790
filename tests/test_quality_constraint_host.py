"""The host side of the quality constraint (DESIGN.md "Mesh quality", 10.14), without a GPU: the ctypes mirrors of
smgpu_quality_constraint_params, _record and _state against the header, the front-end's line, and the refusals of `smoothMesh
-qualityConstraint`, which come before any device work."""
import ctypes as C
import dataclasses
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "smoothmesh_amd", "bin", "smoothMesh")


def test_ctypes_mirrors_have_the_headers_layout(tmp_path):
    from smoothmesh_amd import _ffi
    from smoothmesh_amd.engine import QualityConstraintRecord, QualityConstraintState
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no host C compiler"
    structs = {"smgpu_quality_constraint_params": _ffi.QualityConstraintParams, "smgpu_quality_constraint_record": _ffi.QualityConstraintRecord,
               "smgpu_quality_constraint_state": _ffi.QualityConstraintState, "smgpu_tangle_record": _ffi.TangleRecord}
    body = ""
    for cname, mirror in structs.items():
        body += f'    printf("{cname} size %zu\\n", sizeof({cname}));\n'
        body += "".join(f'    printf("{cname} {n} %zu\\n", offsetof({cname}, {n}));\n' for n, _ in mirror._fields_)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "smgpu.h"\nint main(void) {\n' + body + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, capture_output=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")
    got = {(a, b): int(v) for a, b, v in (line.split() for line in out if line)}
    want = {}
    for cname, mirror in structs.items():
        want[(cname, "size")] = C.sizeof(mirror)
        want.update({(cname, n): getattr(mirror, n).offset for n, _ in mirror._fields_})
    assert got == want
    # the pinned layout: the record begins with smgpu_tangle_record's fields at their offsets, then the three new counts
    rec = "smgpu_quality_constraint_record"
    assert {n: got[(rec, n)] for n, _ in _ffi.QualityConstraintRecord._fields_} == dict(
        iteration=0, passes=8, fullRevert=12, nBadCells=16, nPointsReverted=24, nTangledCells=32, nNonOrthoFaces=40, nSkewFaces=48)
    assert got[(rec, "size")] == 56                                # what the engine allocates per iteration of the longest call
    for n, _ in _ffi.TangleRecord._fields_:
        assert got[(rec, n)] == got[("smgpu_tangle_record", n)]
    assert got[("smgpu_quality_constraint_params", "size")] == 32 and got[("smgpu_quality_constraint_state", "size")] == 56
    assert [f.name for f in dataclasses.fields(QualityConstraintRecord)] == [n for n, _ in _ffi.QualityConstraintRecord._fields_]
    assert [f.name for f in dataclasses.fields(QualityConstraintState)] == [n for n, _ in _ffi.QualityConstraintState._fields_]
    for sym in ("smgpu_set_quality_constraint", "smgpu_get_quality_constraint_records", "smgpu_get_quality_constraint_state"):
        assert sym in _ffi.SYMBOLS
    _ffi.lib()                                                     # the library exports them


def test_format_quality_constraint_line():
    from smoothmesh_amd.engine import QualityConstraintRecord
    from smoothmesh_amd.quality import format_quality_constraint_line
    r = QualityConstraintRecord(iteration=40, passes=1, fullRevert=0, nBadCells=4, nPointsReverted=9, nTangledCells=0, nNonOrthoFaces=2, nSkewFaces=1)
    assert format_quality_constraint_line(r) == "    quality constraint iteration=40 badCells 4 tangled 0 nonOrthoFaces 2 skewFaces 1 passes 1 pointsReverted 9\n"
    r = QualityConstraintRecord(iteration=8, passes=2, fullRevert=1, nBadCells=4, nPointsReverted=216, nTangledCells=1, nNonOrthoFaces=0, nSkewFaces=3)
    assert format_quality_constraint_line(r) == ("    quality constraint iteration=8 badCells 4 tangled 1 nonOrthoFaces 0 skewFaces 3 passes 2 "
                                                 "pointsReverted 216 fullRevert\n")


def test_cli_quality_constraint_refusals(tmp_path):
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import write_case
    write_case(str(tmp_path / "a"), hex_block(3, 3, 3))
    before = sorted(os.listdir(tmp_path / "a"))

    def run(*opts):
        return subprocess.run([BIN, "-case", str(tmp_path / "a")] + list(opts), capture_output=True, text=True, timeout=120)

    for opt, val in (("-maxNonOrtho", "60"), ("-maxInternalSkewness", "3"), ("-maxBoundarySkewness", "10"), ("-qualityConstraintPasses", "1")):
        r = run(opt, val)
        assert r.returncode != 0 and f"{opt} needs -qualityConstraint true" in r.stdout + r.stderr
        r = run("-qualityConstraint", "false", opt, val)
        assert r.returncode != 0 and f"{opt} needs -qualityConstraint true" in r.stdout + r.stderr
    r = run("-parallel", "-qualityConstraint", "true")
    assert r.returncode != 0 and "-qualityConstraint is not available with -parallel" in r.stdout + r.stderr
    r = run("-qualityConstraint", "true", "-tangleConstraint", "true")
    assert r.returncode != 0 and "-qualityConstraint is not available with -tangleConstraint true" in r.stdout + r.stderr
    r = run("-qualityConstraint", "true", "-qualityConstraintPasses", "-1")
    assert r.returncode != 0 and "qualityConstraintPasses must be between 0 and 2147483647" in r.stdout + r.stderr
    r = run("-qualityConstraint", "true", "-maxNonOrtho", "nan")
    assert r.returncode != 0 and "must be numbers" in r.stdout + r.stderr
    r = run("-qualityConstraint", "true", "-maxNonOrtho", "steep")
    assert r.returncode != 0 and "Bad value for option -maxNonOrtho" in r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path / "a")) == before
    h = subprocess.run([BIN, "-help"], capture_output=True, text=True, timeout=120)
    for o in ("-qualityConstraint", "-maxNonOrtho", "-maxInternalSkewness", "-maxBoundarySkewness", "-qualityConstraintPasses"):
        assert o in h.stdout


def test_cli_refuses_boundary_point_smoothing(tmp_path):
    """the refusal comes with the boundary set-up read, before the engine is created: no device work, nothing written"""
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import write_case
    write_case(str(tmp_path), hex_block(4))
    geo = tmp_path / "constant" / "geometry"
    geo.mkdir()
    (geo / "targetSurfaces.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    (geo / "initEdges.obj").write_text("v 0 0 0\nv 1 0 0\nl 1 2\n")
    r = subprocess.run([BIN, "-case", str(tmp_path), "-qualityConstraint", "true"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "-qualityConstraint is not available with boundary point smoothing" in r.stdout + r.stderr
    assert not any(x.isdigit() and x != "0" for x in os.listdir(tmp_path))
