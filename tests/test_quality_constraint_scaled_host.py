"""The host side of the quality constraint's scaling passes (DESIGN.md "Mesh quality", 10.19) without a GPU:
smgpu_quality_constraint_scaling, _record_scaled and _state_scaled against the header and against the _all structs they extend,
the ctypes mirrors, the formatter lines, the front-end's refusals (which come before any device work), and the decomposed
smoothers' ValueError."""
import ctypes as C
import dataclasses
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "smoothmesh_amd", "bin", "smoothMesh")
OPTIONS = ("scalePasses", "errorReduction", "nSmoothScale")


def test_structs_extend_the_widest_ones(tmp_path):
    from smoothmesh_amd import _ffi
    from smoothmesh_amd.engine import QualityConstraintRecordAll, QualityConstraintRecordScaled, QualityConstraintStateAll, QualityConstraintStateScaled
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no host C compiler"
    pairs = {"smgpu_quality_constraint_record_scaled": (_ffi.QualityConstraintRecordScaled, "smgpu_quality_constraint_record_all", _ffi.QualityConstraintRecordAll),
             "smgpu_quality_constraint_state_scaled": (_ffi.QualityConstraintStateScaled, "smgpu_quality_constraint_state_all", _ffi.QualityConstraintStateAll)}
    structs = {"smgpu_quality_constraint_scaling": _ffi.QualityConstraintScaling}
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
    # the _all struct is the head of the new one, field for field; the new fields follow it in the contract's order
    for cname, (mirror, old, oldMirror) in pairs.items():
        names = [n for n, _ in mirror._fields_]
        oldNames = [n for n, _ in oldMirror._fields_]
        assert names[:len(oldNames)] == oldNames
        for n in oldNames:
            assert got[(cname, n)] == got[(old, n)]
    assert [n for n, _ in _ffi.QualityConstraintRecordScaled._fields_][18:] == ["nScalePasses", "nPointsScaled", "minScale"]
    assert [got[("smgpu_quality_constraint_record_scaled", n)] for n in ("nScalePasses", "nPointsScaled", "minScale")] == [136, 144, 152]
    assert [n for n, _ in _ffi.QualityConstraintStateScaled._fields_][20:] == ["scalePasses", "nSmoothScale", "errorReduction"]
    assert [got[("smgpu_quality_constraint_state_scaled", n)] for n in ("scalePasses", "nSmoothScale", "errorReduction")] == [152, 156, 160]
    assert [got[("smgpu_quality_constraint_scaling", n)] for n in ("scalePasses", "nSmoothScale", "errorReduction")] == [0, 4, 8]
    assert (got[("smgpu_quality_constraint_scaling", "size")], got[("smgpu_quality_constraint_record_scaled", "size")],
            got[("smgpu_quality_constraint_state_scaled", "size")]) == (16, 160, 168)
    assert [f.name for f in dataclasses.fields(QualityConstraintRecordScaled)] == [n for n, _ in _ffi.QualityConstraintRecordScaled._fields_]
    assert [f.name for f in dataclasses.fields(QualityConstraintStateScaled)] == [n for n, _ in _ffi.QualityConstraintStateScaled._fields_]
    assert issubclass(QualityConstraintRecordScaled, QualityConstraintRecordAll) and issubclass(QualityConstraintStateScaled, QualityConstraintStateAll)
    for sym in ("smgpu_set_quality_constraint_scaling", "smgpu_get_quality_constraint_records_scaled", "smgpu_get_quality_constraint_state_scaled"):
        assert sym in _ffi.SYMBOLS
    _ffi.lib()                                                     # the library exports them


def test_python_defaults_leave_the_call_unchanged():
    import inspect
    from smoothmesh_amd import SmoothEngine
    from smoothmesh_amd.engine import QualityConstraintRecordScaled, QualityConstraintStateScaled
    from smoothmesh_amd.halo import DistributedSmoother, LocalMultiSmoother
    for fn in (SmoothEngine.set_quality_constraint, SmoothEngine.set_quality_constraint_scaling, LocalMultiSmoother.set_quality_constraint_limits_all,
               DistributedSmoother.set_quality_constraint_limits_all):
        sig = inspect.signature(fn).parameters
        assert [sig[k].default for k in OPTIONS] == [0, 0.75, 4], fn
    r = QualityConstraintRecordScaled(iteration=1, passes=0, fullRevert=0, nBadCells=0, nPointsReverted=0, nTangledCells=0, nNonOrthoFaces=0, nSkewFaces=0)
    assert (r.nScalePasses, r.nPointsScaled, r.minScale) == (0, 0, 0.0)
    s = QualityConstraintStateScaled(on=False, passes=2, maxNonOrtho=65.0, maxInternalSkewness=4.0, maxBoundarySkewness=20.0, nExemptCells=0, nExemptFaces=0, iteration=0)
    assert (s.scalePasses, s.errorReduction, s.nSmoothScale) == (0, 0.75, 4)


def test_formatter_lines():
    from smoothmesh_amd.engine import QualityConstraintRecordScaled, QualityConstraintStateScaled
    from smoothmesh_amd.quality import format_quality_constraint_line, format_quality_constraint_scaling_line
    r = QualityConstraintRecordScaled(iteration=40, passes=3, fullRevert=0, nBadCells=4, nPointsReverted=9, nTangledCells=0, nNonOrthoFaces=2, nSkewFaces=1,
                                      nLowTetFaces=3, nLowTwistFaces=5, nLowTriangleTwistFaces=6, nLowWeightFaces=7, nLowVolRatioFaces=8, nUnderdeterminedCells=10,
                                      nConcaveFaces=11, nWarpedFaces=12, nSmallAreaFaces=13, nSmallVolumeCells=14, nScalePasses=2, nPointsScaled=58, minScale=0.5625)
    # scaling off: the lines they were, of the wider record
    assert format_quality_constraint_line(r) == "    quality constraint iteration=40 badCells 4 tangled 0 nonOrthoFaces 2 skewFaces 1 passes 3 pointsReverted 9\n"
    assert format_quality_constraint_line(r, last=True).endswith(" smallAreaFaces 13 smallVolumeCells 14 passes 3 pointsReverted 9\n")
    # the three values stand directly in front of passes, in every form of the line
    assert format_quality_constraint_line(r, scaled=True) == (
        "    quality constraint iteration=40 badCells 4 tangled 0 nonOrthoFaces 2 skewFaces 1 scalePasses 2 pointsScaled 58 minScale 0.5625 passes 3 pointsReverted 9\n")
    assert format_quality_constraint_line(r, more=True, scaled=True).endswith(" underdeterminedCells 10 scalePasses 2 pointsScaled 58 minScale 0.5625 passes 3 pointsReverted 9\n")
    assert format_quality_constraint_line(r, last=True, scaled=True).endswith(" smallVolumeCells 14 scalePasses 2 pointsScaled 58 minScale 0.5625 passes 3 pointsReverted 9\n")
    r.fullRevert, r.minScale, r.nPointsScaled = 1, 0.0, 0
    assert format_quality_constraint_line(r, scaled=True).endswith(" scalePasses 2 pointsScaled 0 minScale 0 passes 3 pointsReverted 9 fullRevert\n")
    s = QualityConstraintStateScaled(on=True, passes=2, maxNonOrtho=65.0, maxInternalSkewness=4.0, maxBoundarySkewness=20.0, nExemptCells=0, nExemptFaces=3, iteration=0,
                                     scalePasses=2, errorReduction=0.75, nSmoothScale=4)
    assert format_quality_constraint_scaling_line(s) == "Quality constraint scaling: scalePasses 2 errorReduction 0.75 nSmoothScale 4\n"


def test_cli_refusals(tmp_path):
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import write_case
    write_case(str(tmp_path / "a"), hex_block(3, 3, 3))
    before = sorted(os.listdir(tmp_path / "a"))

    def run(*opts):
        r = subprocess.run([BIN, "-case", str(tmp_path / "a")] + list(opts), capture_output=True, text=True, timeout=120)
        return r.returncode, r.stdout + r.stderr

    values = dict(scalePasses="2", errorReduction="0.5", nSmoothScale="1")
    for k in OPTIONS:
        for opts in ((f"-{k}", values[k]), ("-qualityConstraint", "false", f"-{k}", values[k])):
            rc, out = run(*opts)
            assert rc != 0 and f"-{k} needs -qualityConstraint true" in out
        rc, out = run("-tangleConstraint", "true", f"-{k}", values[k])
        assert rc != 0 and f"-{k} is not available with -tangleConstraint: the tangle constraint has no scaling passes" in out
        rc, out = run("-parallel", "-qualityConstraint", "true", "-scalePasses", "2", f"-{k}", values[k])
        assert rc != 0 and "-qualityConstraint is not available with -parallel" in out
        rc, out = run("-qualityConstraint", "true", "-tangleConstraint", "true", "-scalePasses", "2", f"-{k}", values[k])
        assert rc != 0 and "-qualityConstraint is not available with -tangleConstraint true" in out
    for k in OPTIONS[1:]:
        for opts in ((), ("-scalePasses", "0")):
            rc, out = run("-qualityConstraint", "true", f"-{k}", values[k], *opts)
            assert rc != 0 and f"-{k} needs -scalePasses > 0" in out
    for bad, msg in ((("-scalePasses", "-1"), "scalePasses must be between 0 and 2147483647"),
                     (("-scalePasses", "2", "-errorReduction", "1"), "errorReduction must be a number with 0 <= errorReduction < 1"),
                     (("-scalePasses", "2", "-errorReduction", "-0.5"), "errorReduction must be a number with 0 <= errorReduction < 1"),
                     (("-scalePasses", "2", "-errorReduction", "nan"), "errorReduction must be a number with 0 <= errorReduction < 1"),
                     (("-scalePasses", "2", "-nSmoothScale", "-1"), "nSmoothScale must be between 0 and 2147483647"),
                     (("-scalePasses", "some"), "Bad value for option -scalePasses")):
        rc, out = run("-qualityConstraint", "true", *bad)
        assert rc != 0 and msg in out, (bad, out[-400:])
    assert sorted(os.listdir(tmp_path / "a")) == before
    h = subprocess.run([BIN, "-help"], capture_output=True, text=True, timeout=120)
    for k in OPTIONS:
        assert f"-{k}" in h.stdout


def test_cli_refuses_boundary_point_smoothing(tmp_path):
    """the refusal comes with the boundary set-up read, before the engine is created: no device work, nothing written"""
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import write_case
    write_case(str(tmp_path), hex_block(4))
    geo = tmp_path / "constant" / "geometry"
    geo.mkdir()
    (geo / "targetSurfaces.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    (geo / "initEdges.obj").write_text("v 0 0 0\nv 1 0 0\nl 1 2\n")
    r = subprocess.run([BIN, "-case", str(tmp_path), "-qualityConstraint", "true", "-scalePasses", "2", "-errorReduction", "0.5", "-nSmoothScale", "1"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "-qualityConstraint is not available with boundary point smoothing" in r.stdout + r.stderr


@pytest.mark.parametrize("cls", ["LocalMultiSmoother", "DistributedSmoother"])
def test_decomposed_smoothers_refuse_the_scaling_keywords_by_name(cls):
    """set_quality_constraint and set_quality_constraint_limits_all of the two smoothers take the three keywords of
    engine.set_quality_constraint and refuse scalePasses > 0 first, before the smoother's state is looked at: no device, no process
    group.  set_quality_constraint_limits keeps the signature tests/test_quality_constraint_full_multi_host.py pins: it does not
    know the keywords, and Python's own TypeError names the one given"""
    from smoothmesh_amd import halo
    smoother = object.__new__(getattr(halo, cls))
    for k in OPTIONS:
        with pytest.raises(TypeError, match=f"unexpected keyword argument '{k}'"):
            smoother.set_quality_constraint_limits(**{k: 1})
    for call in (smoother.set_quality_constraint, smoother.set_quality_constraint_limits_all):
        with pytest.raises(ValueError, match=r"scalePasses=2 \(with errorReduction=0.75, nSmoothScale=4\) is not available on a decomposed mesh"):
            call(scalePasses=2)
        with pytest.raises(ValueError, match=r"scalePasses=1 \(with errorReduction=0.5, nSmoothScale=0\) is not available on a decomposed mesh.*leave scalePasses, errorReduction and nSmoothScale out"):
            call(scalePasses=1, errorReduction=0.5, nSmoothScale=0)
        # off: nothing to refuse -- the call goes on to the smoother's state
        with pytest.raises(AttributeError):
            call(scalePasses=0, errorReduction=0.5, nSmoothScale=1)
    with pytest.raises(TypeError, match="scalePass"):
        smoother.set_quality_constraint(scalePass=2)


def test_every_tiered_struct_is_the_head_of_the_next():
    """The library widens a setter's argument over the head of the widest limits and answers a getter with the head of the widest
    record or state (smoothmesh_amd/csrc/quality_state.hpp asserts the C layouts): in the ctypes mirrors, too, every field of a
    narrower struct has its name, type and offset in the wider one, and the wider one's own fields start where the narrower ends"""
    from smoothmesh_amd import _ffi
    chains = (("QualityConstraintParams", "QualityConstraintLimits", "QualityConstraintLimitsAll"),
              ("QualityConstraintRecord", "QualityConstraintRecordFull", "QualityConstraintRecordAll", "QualityConstraintRecordScaled"),
              ("QualityConstraintState", "QualityConstraintStateFull", "QualityConstraintStateAll", "QualityConstraintStateScaled"),
              ("QualityConstraintHaloDesc", "QualityConstraintHaloDescFull"))
    for chain in chains:
        for narrow, wide in zip(chain, chain[1:]):
            n, w = getattr(_ffi, narrow), getattr(_ffi, wide)
            assert len(w._fields_) > len(n._fields_) and w._fields_[:len(n._fields_)] == n._fields_, (narrow, wide)
            for name, _ in n._fields_:
                assert (getattr(w, name).offset, getattr(w, name).size) == (getattr(n, name).offset, getattr(n, name).size), (narrow, wide, name)
            assert getattr(w, w._fields_[len(n._fields_)][0]).offset == C.sizeof(n), (narrow, wide)


def test_the_constraint_methods_of_the_two_smoothers_have_one_owner():
    """every public method of the tangle and the quality constraint is written once, on the base the two smoothers share: the same
    function and so the same signature, and neither class defines one of its own.  No device, no process group"""
    import inspect
    from smoothmesh_amd.halo import DistributedSmoother, LocalMultiSmoother
    methods = ("set_tangle_constraint", "clear_tangle_constraint", "tangle_state", "tangle_records", "set_quality_constraint",
               "set_quality_constraint_limits", "set_quality_constraint_limits_all", "clear_quality_constraint", "quality_constraint_state",
               "quality_constraint_records")
    shared = [b for b in DistributedSmoother.__mro__[1:] if b in LocalMultiSmoother.__mro__[1:] and b is not object]
    assert shared, "no shared base"
    for m in methods:
        assert inspect.signature(getattr(DistributedSmoother, m)) == inspect.signature(getattr(LocalMultiSmoother, m)), m
        assert m not in vars(DistributedSmoother) and m not in vars(LocalMultiSmoother), m
        assert getattr(DistributedSmoother, m) is getattr(LocalMultiSmoother, m) and any(m in vars(b) for b in shared), m
