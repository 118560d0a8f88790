"""The host side of the quality constraint's last four limits -- maxConcave, minFlatness, minVol, minArea (DESIGN.md "Mesh
quality", 10.18) -- without a GPU: smgpu_quality_constraint_limits_all, _record_all and _state_all against the header and against the
_full structs they extend, the ctypes mirrors, the formatter lines, the front-end's refusals (which come before any device work),
and the decomposed smoothers' ValueError."""
import ctypes as C
import dataclasses
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "smoothmesh_amd", "bin", "smoothMesh")
LIMITS = ("maxConcave", "minFlatness", "minVol", "minArea")
COUNTS = ("nConcaveFaces", "nWarpedFaces", "nSmallAreaFaces", "nSmallVolumeCells")


def test_structs_extend_the_full_ones(tmp_path):
    from smoothmesh_amd import _ffi
    from smoothmesh_amd.engine import QualityConstraintRecordAll, QualityConstraintRecordFull, QualityConstraintStateAll, QualityConstraintStateFull
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no host C compiler"
    pairs = {"smgpu_quality_constraint_limits_all": (_ffi.QualityConstraintLimitsAll, "smgpu_quality_constraint_limits", _ffi.QualityConstraintLimits),
             "smgpu_quality_constraint_record_all": (_ffi.QualityConstraintRecordAll, "smgpu_quality_constraint_record_full", _ffi.QualityConstraintRecordFull),
             "smgpu_quality_constraint_state_all": (_ffi.QualityConstraintStateAll, "smgpu_quality_constraint_state_full", _ffi.QualityConstraintStateFull)}
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
    # the _full struct is the head of the new one, field for field; the new fields follow in the contract's order, 8 bytes each
    for cname, (mirror, old, oldMirror) in pairs.items():
        names = [n for n, _ in mirror._fields_]
        oldNames = [n for n, _ in oldMirror._fields_]
        assert names[:len(oldNames)] == oldNames
        for n in oldNames:
            assert got[(cname, n)] == got[(old, n)]
        assert [got[(cname, n)] for n in names[len(oldNames):]] == [got[(old, "size")] + 8 * k for k in range(len(names) - len(oldNames))]
    assert [n for n, _ in _ffi.QualityConstraintLimitsAll._fields_][10:] == list(LIMITS)
    assert [n for n, _ in _ffi.QualityConstraintRecordAll._fields_][14:] == list(COUNTS)
    assert [n for n, _ in _ffi.QualityConstraintStateAll._fields_][15:] == list(LIMITS) + ["nExemptVolumeCells"]
    assert (got[("smgpu_quality_constraint_limits_all", "size")], got[("smgpu_quality_constraint_record_all", "size")],
            got[("smgpu_quality_constraint_state_all", "size")]) == (112, 136, 152)
    assert [f.name for f in dataclasses.fields(QualityConstraintRecordAll)] == [n for n, _ in _ffi.QualityConstraintRecordAll._fields_]
    assert [f.name for f in dataclasses.fields(QualityConstraintStateAll)] == [n for n, _ in _ffi.QualityConstraintStateAll._fields_]
    assert issubclass(QualityConstraintRecordAll, QualityConstraintRecordFull) and issubclass(QualityConstraintStateAll, QualityConstraintStateFull)
    for sym in ("smgpu_set_quality_constraint_limits_all", "smgpu_set_quality_constraint_limits_all_coupled", "smgpu_get_quality_constraint_records_all",
                "smgpu_get_quality_constraint_state_all"):
        assert sym in _ffi.SYMBOLS
    _ffi.lib()                                                     # the library exports them


def test_python_defaults_are_all_off():
    import inspect
    from smoothmesh_amd import SmoothEngine
    from smoothmesh_amd.engine import QUALITY_CONSTRAINT_LIMITS_ALL_OFF, QualityConstraintRecordAll, QualityConstraintStateAll, quality_constraint_limits_all_on
    from smoothmesh_amd.halo import DistributedSmoother, LocalMultiSmoother
    for fn in (SmoothEngine.set_quality_constraint, SmoothEngine.set_quality_constraint_limits_coupled, LocalMultiSmoother.set_quality_constraint_limits_all,
               DistributedSmoother.set_quality_constraint_limits_all):
        sig = inspect.signature(fn).parameters
        assert [sig[k].default for k in LIMITS] == [None] * 4, fn
    assert list(QUALITY_CONSTRAINT_LIMITS_ALL_OFF.items()) == [("maxConcave", 180.0), ("minFlatness", 0.0), ("minVol", 0.0), ("minArea", 0.0)]
    assert quality_constraint_limits_all_on() == {} and quality_constraint_limits_all_on(**{k: None for k in LIMITS}) == {}
    assert quality_constraint_limits_all_on(**QUALITY_CONSTRAINT_LIMITS_ALL_OFF) == {}
    assert quality_constraint_limits_all_on(maxConcave=200.0, minFlatness=-1.0, minVol=-1e30, minArea=-1.0) == {}    # OpenFOAM's disabling values
    assert quality_constraint_limits_all_on(maxConcave=179.9, minArea=0.0, minVol=1e-300) == {"maxConcave": 179.9, "minVol": 1e-300}
    assert list(quality_constraint_limits_all_on(maxConcave=float("nan"), minFlatness=float("nan"))) == ["maxConcave", "minFlatness"]   # a NaN goes on, to be refused
    with pytest.raises(TypeError, match="minVolume"):
        quality_constraint_limits_all_on(minVolume=1.0)
    r = QualityConstraintRecordAll(iteration=1, passes=0, fullRevert=0, nBadCells=0, nPointsReverted=0, nTangledCells=0, nNonOrthoFaces=0, nSkewFaces=0)
    assert [getattr(r, k) for k in COUNTS] == [0] * 4
    s = QualityConstraintStateAll(on=False, passes=2, maxNonOrtho=65.0, maxInternalSkewness=4.0, maxBoundarySkewness=20.0, nExemptCells=0, nExemptFaces=0, iteration=0)
    assert [getattr(s, k) for k in LIMITS] == list(QUALITY_CONSTRAINT_LIMITS_ALL_OFF.values()) and s.nExemptVolumeCells == 0


def test_formatter_lines():
    from smoothmesh_amd.engine import QualityConstraintRecordAll, QualityConstraintStateAll
    from smoothmesh_amd.quality import format_quality_constraint_limits_line, format_quality_constraint_line
    r = QualityConstraintRecordAll(iteration=40, passes=1, fullRevert=0, nBadCells=4, nPointsReverted=9, nTangledCells=0, nNonOrthoFaces=2, nSkewFaces=1,
                                   nLowTetFaces=3, nLowTwistFaces=5, nLowTriangleTwistFaces=6, nLowWeightFaces=7, nLowVolRatioFaces=8, nUnderdeterminedCells=10,
                                   nConcaveFaces=11, nWarpedFaces=12, nSmallAreaFaces=13, nSmallVolumeCells=14)
    # the parent's two lines, of the wider record
    assert format_quality_constraint_line(r) == "    quality constraint iteration=40 badCells 4 tangled 0 nonOrthoFaces 2 skewFaces 1 passes 1 pointsReverted 9\n"
    assert format_quality_constraint_line(r, more=True) == (
        "    quality constraint iteration=40 badCells 4 tangled 0 nonOrthoFaces 2 skewFaces 1 lowTetFaces 3 twistedFaces 5 lowTriangleTwistFaces 6 "
        "lowWeightFaces 7 lowVolRatioFaces 8 underdeterminedCells 10 passes 1 pointsReverted 9\n")
    # the four counts stand between underdeterminedCells and passes
    assert format_quality_constraint_line(r, last=True) == (
        "    quality constraint iteration=40 badCells 4 tangled 0 nonOrthoFaces 2 skewFaces 1 lowTetFaces 3 twistedFaces 5 lowTriangleTwistFaces 6 "
        "lowWeightFaces 7 lowVolRatioFaces 8 underdeterminedCells 10 concaveFaces 11 warpedFaces 12 smallAreaFaces 13 smallVolumeCells 14 passes 1 "
        "pointsReverted 9\n")
    r.fullRevert = 1
    assert format_quality_constraint_line(r, last=True).endswith(" smallVolumeCells 14 passes 1 pointsReverted 9 fullRevert\n")
    base = dict(on=True, passes=2, maxNonOrtho=65.0, maxInternalSkewness=4.0, maxBoundarySkewness=20.0, nExemptCells=0, nExemptFaces=3, iteration=0)
    s = QualityConstraintStateAll(**base, minTwist=0.02, minDeterminant=0.001, nExemptDeterminantCells=12)
    assert format_quality_constraint_limits_line(s) == "Quality constraint limits: minTwist 0.02 minDeterminant 0.001, 12 determinant-exempt cells\n"   # the parent's
    s = QualityConstraintStateAll(**base, minTwist=0.02, nExemptDeterminantCells=0, maxConcave=75.0, minVol=1e-13, nExemptVolumeCells=5)
    assert format_quality_constraint_limits_line(s) == "Quality constraint limits: minTwist 0.02 maxConcave 75 minVol 1e-13, 0 determinant-exempt cells, 5 volume-exempt cells\n"
    s = QualityConstraintStateAll(**base, minFlatness=0.5, minArea=2e-9)
    assert format_quality_constraint_limits_line(s) == "Quality constraint limits: minFlatness 0.5 minArea 2e-09, 0 determinant-exempt cells, 0 volume-exempt cells\n"


def test_cli_refusals(tmp_path):
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import write_case
    write_case(str(tmp_path / "a"), hex_block(3, 3, 3))
    before = sorted(os.listdir(tmp_path / "a"))

    def run(*opts):
        return subprocess.run([BIN, "-case", str(tmp_path / "a")] + list(opts), capture_output=True, text=True, timeout=120)

    for k in LIMITS + ("meshQualityDict",):
        value = "true" if k == "meshQualityDict" else "0.01"
        r = run(f"-{k}", value)
        assert r.returncode != 0 and f"-{k} needs -qualityConstraint true" in r.stdout + r.stderr
        r = run("-qualityConstraint", "false", f"-{k}", value)
        assert r.returncode != 0 and f"-{k} needs -qualityConstraint true" in r.stdout + r.stderr
    for k in LIMITS:
        r = run("-qualityConstraint", "true", f"-{k}", "nan")
        assert r.returncode != 0 and f"-{k} must be a number" in r.stdout + r.stderr
        r = run("-parallel", "-qualityConstraint", "true", f"-{k}", "0.01")
        assert r.returncode != 0 and "-qualityConstraint is not available with -parallel" in r.stdout + r.stderr
    r = run("-qualityConstraint", "true", "-maxConcave", "-1")
    assert r.returncode != 0 and "-maxConcave must not be negative" in r.stdout + r.stderr
    r = run("-qualityConstraint", "true", "-minVol", "tiny")
    assert r.returncode != 0 and "Bad value for option -minVol" in r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path / "a")) == before
    h = subprocess.run([BIN, "-help"], capture_output=True, text=True, timeout=120)
    for k in LIMITS + ("meshQualityDict",):
        assert f"-{k}" in h.stdout


@pytest.mark.parametrize("cls", ["LocalMultiSmoother", "DistributedSmoother"])
def test_decomposed_smoothers_refuse_a_new_limit_by_name(cls):
    """set_quality_constraint keeps refusing the limits it does not take, the four included; the refusal comes first, before the
    smoother's state is looked at: no device, no process group"""
    from smoothmesh_amd import halo
    smoother = object.__new__(getattr(halo, cls))
    for k in LIMITS:
        with pytest.raises(ValueError, match=f"{k} is not available through set_quality_constraint on a decomposed mesh"):
            smoother.set_quality_constraint(**{k: 0.5})
    for k, off in zip(LIMITS, (180.0, 0.0, 0.0, 0.0)):                  # off, or None: nothing to refuse -- the call goes on to the smoother's state
        with pytest.raises(AttributeError):
            smoother.set_quality_constraint(**{k: off})
    with pytest.raises(TypeError, match="minVolume"):
        smoother.set_quality_constraint(minVolume=0.5)
