"""The host side of the quality history (DESIGN.md "Mesh quality", 10.10), without a GPU: the ctypes mirror of
smgpu_quality_trace_record against the header, the front-end's line, and the refusals of `smoothMesh -qualityInterval`, which
come before any device work."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "smoothmesh_amd", "bin", "smoothMesh")


def test_ctypes_mirror_has_the_headers_layout(tmp_path):
    from smoothmesh_amd import _ffi
    from smoothmesh_amd.engine import MeshQuality, QualityTraceRecord
    import dataclasses
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no host C compiler"
    names = [n for n, _ in _ffi.QualityTraceRecord._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "smgpu.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(smgpu_quality_trace_record));\n'
                   + "".join(f'    printf("{n} %zu\\n", offsetof(smgpu_quality_trace_record, {n}));\n' for n in names)
                   + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, capture_output=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")
    assert int(out[0]) == C.sizeof(_ffi.QualityTraceRecord)
    got = dict((k, int(v)) for k, v in (line.split() for line in out[1:] if line))
    assert got == {n: getattr(_ffi.QualityTraceRecord, n).offset for n in names}
    # the dataclass carries the same fields: those of MeshQuality, less the sizes and the two order-dependent ones, plus iteration
    assert [f.name for f in dataclasses.fields(QualityTraceRecord)] == names
    left_out = {"nCells", "nFaces", "nInternalFaces", "totalVolume", "avgNonOrth"}
    assert names[1:] == [f.name for f in dataclasses.fields(MeshQuality) if f.name not in left_out]


def _record(**over):
    from smoothmesh_amd.engine import QualityTraceRecord
    import dataclasses
    d = {f.name: (0 if f.type is int else 0.0) for f in dataclasses.fields(QualityTraceRecord)}
    d.update(over)
    return QualityTraceRecord(**d)


def test_format_trace_line():
    from smoothmesh_amd.engine import MeshQuality
    from smoothmesh_amd.quality import format_trace_line, format_trace_warning
    import dataclasses
    r = _record(iteration=40, minVolume=-1.25e-7, nNonPositiveVolume=3, maxNonOrth=61.123456789123, nErrorNonOrth=2, maxSkewness=0.5,
                nWrongOrientedFaces=7, maxOpenness=1.0 / 3.0, maxAspectRatio=1234567.891)
    assert format_trace_line(r) == ("    quality iteration=40 minVolume -1.25e-07 nonPositive 3 maxNonOrth 61.1234568 error 2 maxSkewness 0.5 "
                                    "wrongOriented 7 maxOpenness 0.333333333 maxAspectRatio 1234567.89\n")
    q = MeshQuality(**{f.name: 0 for f in dataclasses.fields(MeshQuality)})
    q.nNonPositiveVolume, q.nWrongOrientedFaces = 1, 4
    assert format_trace_warning(r, q) == "    ***Iteration 40: 3 non-positive volume cells and 7 wrongly oriented faces (initial mesh: 1, 4)\n"


def test_cli_quality_interval_refusals(tmp_path):
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import write_case
    write_case(str(tmp_path / "a"), hex_block(3, 3, 3))
    before = sorted(os.listdir(tmp_path / "a"))

    def run(*opts):
        return subprocess.run([BIN, "-case", str(tmp_path / "a")] + list(opts), capture_output=True, text=True, timeout=120)

    r = run("-qualityInterval", "2")
    assert r.returncode != 0 and "-qualityInterval needs -checkQuality true" in r.stdout + r.stderr
    r = run("-parallel", "-checkQuality", "true", "-qualityInterval", "2")
    assert r.returncode != 0 and "is not available with -parallel" in r.stdout + r.stderr
    r = run("-parallel", "-qualityInterval", "2")
    assert r.returncode != 0 and "-qualityInterval is not available with -parallel" in r.stdout + r.stderr
    for bad in ("0", "-3"):
        r = run("-checkQuality", "true", "-qualityInterval", bad)
        assert r.returncode != 0 and "qualityInterval must be positive" in r.stdout + r.stderr, bad
    r = run("-checkQuality", "true", "-qualityInterval", "often")
    assert r.returncode != 0 and "Bad value for option -qualityInterval" in r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path / "a")) == before
    h = subprocess.run([BIN, "-help"], capture_output=True, text=True, timeout=120)
    assert "-qualityInterval" in h.stdout
