"""The host side of the quality constraint's tet, twist, weight, ratio and determinant limits (DESIGN.md "Mesh quality", 10.16),
without a GPU: smgpu_quality_constraint_limits, _record_full and _state_full against the header and against the structs they
extend, the ctypes mirrors, the front-end's lines and its refusals (which come before any device work), and the refusal of the
decomposed smoothers."""
import ctypes as C
import dataclasses
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "smoothmesh_amd", "bin", "smoothMesh")
LIMITS = ("minTetQuality", "minTwist", "minTriangleTwist", "minFaceWeight", "minVolRatio", "minDeterminant")
COUNTS = ("nLowTetFaces", "nLowTwistFaces", "nLowTriangleTwistFaces", "nLowWeightFaces", "nLowVolRatioFaces", "nUnderdeterminedCells")


def test_structs_extend_the_old_ones(tmp_path):
    from smoothmesh_amd import _ffi
    from smoothmesh_amd.engine import QualityConstraintRecordFull, QualityConstraintStateFull
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no host C compiler"
    pairs = {"smgpu_quality_constraint_limits": (_ffi.QualityConstraintLimits, "smgpu_quality_constraint_params", _ffi.QualityConstraintParams),
             "smgpu_quality_constraint_record_full": (_ffi.QualityConstraintRecordFull, "smgpu_quality_constraint_record", _ffi.QualityConstraintRecord),
             "smgpu_quality_constraint_state_full": (_ffi.QualityConstraintStateFull, "smgpu_quality_constraint_state", _ffi.QualityConstraintState)}
    structs = {}
    for cname, (mirror, old, oldMirror) in pairs.items():
        structs[cname], structs[old] = mirror, oldMirror
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
    for cname, mirror in structs.items():
        assert got[(cname, "size")] == C.sizeof(mirror)
        assert {n: got[(cname, n)] for n, _ in mirror._fields_} == {n: getattr(mirror, n).offset for n, _ in mirror._fields_}
    # the old struct is the head of the new one, field for field; the new fields follow in the contract's order, 8 bytes each
    for cname, (mirror, old, oldMirror) in pairs.items():
        names = [n for n, _ in mirror._fields_]
        oldNames = [n for n, _ in oldMirror._fields_]
        assert names[:len(oldNames)] == oldNames
        for n in oldNames:
            assert got[(cname, n)] == got[(old, n)]
        start = 32 if old.endswith("params") else got[(old, "size")]          # params: int32 passes, then padding to 8
        assert [got[(cname, n)] for n in names[len(oldNames):]] == [start + 8 * k for k in range(len(names) - len(oldNames))]
    assert [n for n, _ in _ffi.QualityConstraintLimits._fields_][4:] == list(LIMITS)
    assert [n for n, _ in _ffi.QualityConstraintRecordFull._fields_][8:] == list(COUNTS)
    assert [n for n, _ in _ffi.QualityConstraintStateFull._fields_][8:] == list(LIMITS) + ["nExemptDeterminantCells"]
    assert (got[("smgpu_quality_constraint_limits", "size")], got[("smgpu_quality_constraint_record_full", "size")],
            got[("smgpu_quality_constraint_state_full", "size")]) == (80, 104, 112)
    assert [f.name for f in dataclasses.fields(QualityConstraintRecordFull)] == [n for n, _ in _ffi.QualityConstraintRecordFull._fields_]
    assert [f.name for f in dataclasses.fields(QualityConstraintStateFull)] == [n for n, _ in _ffi.QualityConstraintStateFull._fields_]
    for sym in ("smgpu_set_quality_constraint_limits", "smgpu_get_quality_constraint_records_full", "smgpu_get_quality_constraint_state_full"):
        assert sym in _ffi.SYMBOLS
    _ffi.lib()                                                     # the library exports them


def test_python_defaults_are_all_off():
    import inspect
    from smoothmesh_amd import SmoothEngine
    from smoothmesh_amd.engine import QUALITY_CONSTRAINT_LIMITS_OFF, QualityConstraintRecordFull, QualityConstraintStateFull, quality_constraint_limits_on
    sig = inspect.signature(SmoothEngine.set_quality_constraint).parameters
    assert [sig[k].default for k in LIMITS] == [None] * 6 and list(QUALITY_CONSTRAINT_LIMITS_OFF) == list(LIMITS)
    assert list(QUALITY_CONSTRAINT_LIMITS_OFF.values()) == [-1e30, -1.0, -1.0, 0.0, 0.0, 0.0]
    assert quality_constraint_limits_on() == {} and quality_constraint_limits_on(**{k: None for k in LIMITS}) == {}
    assert quality_constraint_limits_on(**QUALITY_CONSTRAINT_LIMITS_OFF) == {}                  # "off when <= the off value"
    assert quality_constraint_limits_on(minTwist=-0.999, minVolRatio=0.0) == {"minTwist": -0.999}
    assert list(quality_constraint_limits_on(minDeterminant=float("nan"))) == ["minDeterminant"]   # a NaN goes on, to be refused
    r = QualityConstraintRecordFull(iteration=1, passes=0, fullRevert=0, nBadCells=0, nPointsReverted=0, nTangledCells=0, nNonOrthoFaces=0, nSkewFaces=0)
    assert [getattr(r, k) for k in COUNTS] == [0] * 6
    s = QualityConstraintStateFull(on=False, passes=2, maxNonOrtho=65.0, maxInternalSkewness=4.0, maxBoundarySkewness=20.0, nExemptCells=0, nExemptFaces=0, iteration=0)
    assert [getattr(s, k) for k in LIMITS] == list(QUALITY_CONSTRAINT_LIMITS_OFF.values()) and s.nExemptDeterminantCells == 0


def test_formatter_lines():
    from smoothmesh_amd.engine import QualityConstraintRecordFull, QualityConstraintStateFull
    from smoothmesh_amd.quality import format_quality_constraint_limits_line, format_quality_constraint_line
    r = QualityConstraintRecordFull(iteration=40, passes=1, fullRevert=0, nBadCells=4, nPointsReverted=9, nTangledCells=0, nNonOrthoFaces=2, nSkewFaces=1,
                                    nLowTetFaces=3, nLowTwistFaces=5, nLowTriangleTwistFaces=6, nLowWeightFaces=7, nLowVolRatioFaces=8, nUnderdeterminedCells=10)
    assert format_quality_constraint_line(r) == "    quality constraint iteration=40 badCells 4 tangled 0 nonOrthoFaces 2 skewFaces 1 passes 1 pointsReverted 9\n"
    assert format_quality_constraint_line(r, more=True) == (
        "    quality constraint iteration=40 badCells 4 tangled 0 nonOrthoFaces 2 skewFaces 1 lowTetFaces 3 twistedFaces 5 lowTriangleTwistFaces 6 "
        "lowWeightFaces 7 lowVolRatioFaces 8 underdeterminedCells 10 passes 1 pointsReverted 9\n")
    r.fullRevert = 1
    assert format_quality_constraint_line(r, more=True).endswith(" underdeterminedCells 10 passes 1 pointsReverted 9 fullRevert\n")
    s = QualityConstraintStateFull(on=True, passes=2, maxNonOrtho=65.0, maxInternalSkewness=4.0, maxBoundarySkewness=20.0, nExemptCells=0, nExemptFaces=3,
                                   iteration=0, minTwist=0.02, minDeterminant=0.001, nExemptDeterminantCells=12)
    assert format_quality_constraint_limits_line(s) == "Quality constraint limits: minTwist 0.02 minDeterminant 0.001, 12 determinant-exempt cells\n"


def test_cli_refusals(tmp_path):
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import write_case
    write_case(str(tmp_path / "a"), hex_block(3, 3, 3))
    before = sorted(os.listdir(tmp_path / "a"))

    def run(*opts):
        return subprocess.run([BIN, "-case", str(tmp_path / "a")] + list(opts), capture_output=True, text=True, timeout=120)

    for k in LIMITS:
        r = run(f"-{k}", "0.01")
        assert r.returncode != 0 and f"-{k} needs -qualityConstraint true" in r.stdout + r.stderr
        r = run("-qualityConstraint", "false", f"-{k}", "0.01")
        assert r.returncode != 0 and f"-{k} needs -qualityConstraint true" in r.stdout + r.stderr
        r = run("-qualityConstraint", "true", f"-{k}", "nan")
        assert r.returncode != 0 and f"-{k} must be a number" in r.stdout + r.stderr
        r = run("-parallel", "-qualityConstraint", "true", f"-{k}", "0.01")
        assert r.returncode != 0 and "-qualityConstraint is not available with -parallel" in r.stdout + r.stderr
    r = run("-qualityConstraint", "true", "-minTwist", "flat")
    assert r.returncode != 0 and "Bad value for option -minTwist" in r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path / "a")) == before
    h = subprocess.run([BIN, "-help"], capture_output=True, text=True, timeout=120)
    for k in LIMITS:
        assert f"-{k}" in h.stdout


@pytest.mark.parametrize("cls", ["LocalMultiSmoother", "DistributedSmoother"])
def test_decomposed_smoothers_refuse_a_new_limit_by_name(cls):
    """the refusal comes first, before the smoother's state is looked at: no device, no process group"""
    from smoothmesh_amd import halo
    smoother = object.__new__(getattr(halo, cls))
    for k in LIMITS:
        with pytest.raises(ValueError, match=k):
            smoother.set_quality_constraint(**{k: 0.5})
    with pytest.raises(ValueError, match="minDeterminant"):
        smoother.set_quality_constraint(60.0, 3.0, 10.0, passes=1, minTwist=None, minDeterminant=1e-3)
    with pytest.raises(TypeError, match="minTwists"):
        smoother.set_quality_constraint(minTwists=0.5)
