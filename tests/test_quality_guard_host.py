"""The host side of the guard on the quality history (DESIGN.md "Mesh quality", 10.11), without a GPU: the ctypes mirrors of
smgpu_quality_guard_params / smgpu_quality_guard_state against the header, the front-end's two lines, and the refusals of
`smoothMesh -qualityGuard` that come before any device work."""
import ctypes as C
import dataclasses
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "smoothmesh_amd", "bin", "smoothMesh")


def test_ctypes_mirrors_have_the_headers_layout(tmp_path):
    from smoothmesh_amd import _ffi
    from smoothmesh_amd.engine import QUALITY_GUARD_CRITERIA, QualityGuardState
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no host C compiler"
    structs = {"smgpu_quality_guard_params": _ffi.QualityGuardParams, "smgpu_quality_guard_state": _ffi.QualityGuardState}
    src = tmp_path / "layout.c"
    body = ""
    for cname, mirror in structs.items():
        body += f'    printf("{cname} %zu\\n", sizeof({cname}));\n'
        body += "".join(f'    printf("{cname}.{n} %zu\\n", offsetof({cname}, {n}));\n' for n, _ in mirror._fields_)
    body += "".join(f'    printf("{n} %d\\n", (int){n});\n' for n in ("SMGPU_GUARD_NONPOSITIVE_VOLUME", "SMGPU_GUARD_WRONG_ORIENTED",
                                                                        "SMGPU_GUARD_ERROR_NONORTH"))
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "smgpu.h"\nint main(void) {\n' + body + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, capture_output=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout
    got = dict((k, int(v)) for k, v in (line.split() for line in out.split("\n") if line))
    want = {}
    for cname, mirror in structs.items():
        want[cname] = C.sizeof(mirror)
        want.update({f"{cname}.{n}": getattr(mirror, n).offset for n, _ in mirror._fields_})
    want.update(SMGPU_GUARD_NONPOSITIVE_VOLUME=QUALITY_GUARD_CRITERIA["nonPositiveVolume"],
                SMGPU_GUARD_WRONG_ORIENTED=QUALITY_GUARD_CRITERIA["wrongOriented"],
                SMGPU_GUARD_ERROR_NONORTH=QUALITY_GUARD_CRITERIA["errorNonOrth"])
    assert got == want
    # the dataclass carries the fields of the struct
    assert [f.name for f in dataclasses.fields(QualityGuardState)] == [n for n, _ in _ffi.QualityGuardState._fields_]
    # the library exports the three calls (no device is touched by looking them up)
    lib = C.CDLL(os.path.join(ROOT, "smoothmesh_amd", "csrc", "libsmgpu.so"))
    for name in ("smgpu_set_quality_guard", "smgpu_get_quality_guard", "smgpu_quality_guard_restore"):
        assert name in _ffi.SYMBOLS and getattr(lib, name)


def _record(**over):
    from smoothmesh_amd.engine import QualityTraceRecord
    d = {f.name: (0 if f.type is int else 0.0) for f in dataclasses.fields(QualityTraceRecord)}
    d.update(over)
    return QualityTraceRecord(**d)


def test_format_guard_lines():
    from smoothmesh_amd import QualityGuardState
    from smoothmesh_amd.quality import format_guard_lines
    s = QualityGuardState(armed=False, tripped=True, reasons=("wrongOriented",), snapshotIteration=37, trippedIteration=40,
                          restoredIteration=37, baseline=_record(nNonPositiveVolume=1, nWrongOrientedFaces=4),
                          tripRecord=_record(iteration=40, nNonPositiveVolume=1, nWrongOrientedFaces=7))
    assert format_guard_lines(s) == ("    ***Quality guard: iteration 40: 1 non-positive volume cells and 7 wrongly oriented faces (initial mesh: 1, 4)\n"
                                     "    ***Quality guard: restored the mesh of iteration 37, stopping.\n")


def test_cli_quality_guard_refusals(tmp_path):
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import write_case
    write_case(str(tmp_path / "a"), hex_block(3, 3, 3))
    before = sorted(os.listdir(tmp_path / "a"))

    def run(*opts):
        return subprocess.run([BIN, "-case", str(tmp_path / "a")] + list(opts), capture_output=True, text=True, timeout=120)

    r = run("-qualityGuard", "true")
    assert r.returncode != 0 and "-qualityGuard needs -checkQuality true" in r.stdout + r.stderr
    r = run("-checkQuality", "true", "-qualityGuard", "true")
    assert r.returncode != 0 and "-qualityGuard needs -qualityInterval N" in r.stdout + r.stderr
    r = run("-parallel", "-checkQuality", "true", "-qualityInterval", "2", "-qualityGuard", "true")
    assert r.returncode != 0 and "is not available with -parallel" in r.stdout + r.stderr
    r = run("-parallel", "-qualityGuard", "true")
    assert r.returncode != 0 and "is not available with -parallel" in r.stdout + r.stderr
    r = run("-checkQuality", "true", "-qualityInterval", "2", "-qualityGuardRefine", "false")
    assert r.returncode != 0 and "-qualityGuardRefine needs -qualityGuard true" in r.stdout + r.stderr
    r = run("-checkQuality", "true", "-qualityInterval", "2", "-qualityGuard", "perhaps")
    assert r.returncode != 0 and "Bad bool value for option -qualityGuard" in r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path / "a")) == before
    h = subprocess.run([BIN, "-help"], capture_output=True, text=True, timeout=120)
    assert "-qualityGuard b" in h.stdout and "-qualityGuardRefine" in h.stdout
