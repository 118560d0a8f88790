"""Reading system/meshQualityDict (smoothmesh_amd.quality.read_mesh_quality_dict over include/smhost.h's
smhost_read_mesh_quality_dict, csrc/host/quality_dict.cpp; DESIGN.md "Mesh quality", 10.18) on the hand-written fixtures of
tests/golden/mesh_quality_dicts: a full and a partial file, OpenFOAM's disabling values against the engine's off ranges, a relaxed
block, comments, #include, #includeEtc through etc_dirs, override order, ignored keys, every error of the grammar by file and line;
the answer as keyword arguments of the entries that take it; the front-end's refusals before any device work; and the stand-alone
checker tests/native/dict_reader_check.cpp under AddressSanitizer and UndefinedBehaviorSanitizer.  (The front-end's printed limits
from a dict need the GPU: tests/test_gpu_quality_constraint_all.py.)"""
import inspect
import os
import shutil
import subprocess

import pytest

from smoothmesh_amd.engine import QUALITY_CONSTRAINT_LIMITS_ALL_OFF, QUALITY_CONSTRAINT_LIMITS_OFF, SmoothEngine, quality_constraint_limits_all_on, quality_constraint_limits_on
from smoothmesh_amd.quality import MESH_QUALITY_DICT_KEYS, read_mesh_quality_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "mesh_quality_dicts")
BIN = os.path.join(ROOT, "smoothmesh_amd", "bin", "smoothMesh")
FULL = dict(maxNonOrtho=62.0, maxBoundarySkewness=18.0, maxInternalSkewness=3.5, maxConcave=75.0, minFlatness=0.55, minVol=1e-13, minTetQuality=1e-15,
            minArea=1e-12, minTwist=0.02, minDeterminant=0.001, minFaceWeight=0.05, minVolRatio=0.01, minTriangleTwist=0.03)


def _fix(name):
    return os.path.join(FIX, name)


def test_full_and_partial_dict():
    d = read_mesh_quality_dict(_fix("full"), etc_dirs=[])
    assert dict(d) == FULL and list(d) == list(MESH_QUALITY_DICT_KEYS) and d.path == _fix("full")
    assert d.ignored == ("nSmoothScale", "errorReduction", "relaxed", "minVolCollapseRatio")       # the relaxed block is not read
    p = read_mesh_quality_dict(_fix("partial"), etc_dirs=[])
    assert dict(p) == dict(maxNonOrtho=55.0, minFlatness=0.6, minArea=2e-9) and p.ignored == ()


def test_the_answer_is_keyword_arguments_of_the_entries():
    from smoothmesh_amd.halo import DistributedSmoother, LocalMultiSmoother
    for fn in (SmoothEngine.set_quality_constraint, LocalMultiSmoother.set_quality_constraint_limits_all,
               DistributedSmoother.set_quality_constraint_limits_all):
        assert set(MESH_QUALITY_DICT_KEYS) <= set(inspect.signature(fn).parameters), fn


def test_disabling_values_fall_inside_the_off_ranges():
    """per key: OpenFOAM's disabling value, as the fixture gives it, switches the engine's criterion off"""
    d = read_mesh_quality_dict(_fix("sentinels"), etc_dirs=[])
    assert set(d) == set(MESH_QUALITY_DICT_KEYS)
    assert d["maxNonOrtho"] >= 180.0 and d["maxInternalSkewness"] <= 0.0 and d["maxBoundarySkewness"] <= 0.0     # 10.14's off ranges
    for k in QUALITY_CONSTRAINT_LIMITS_OFF:
        assert quality_constraint_limits_on(**{k: d[k]}) == {}, k
    for k in QUALITY_CONSTRAINT_LIMITS_ALL_OFF:
        assert quality_constraint_limits_all_on(**{k: d[k]}) == {}, k
    # and a value of the full dict switches each on
    f = read_mesh_quality_dict(_fix("full"), etc_dirs=[])
    assert set(quality_constraint_limits_on(**{k: f[k] for k in QUALITY_CONSTRAINT_LIMITS_OFF})) == set(QUALITY_CONSTRAINT_LIMITS_OFF)
    assert set(quality_constraint_limits_all_on(**{k: f[k] for k in QUALITY_CONSTRAINT_LIMITS_ALL_OFF})) == set(QUALITY_CONSTRAINT_LIMITS_ALL_OFF)


def test_includes_and_override_order(monkeypatch):
    d = read_mesh_quality_dict(_fix("with_include"), etc_dirs=[])
    assert dict(d) == dict(minTwist=0.04, maxNonOrtho=50.0, minFlatness=0.6, minArea=2e-9)           # the later entry wins over the include's
    e = read_mesh_quality_dict(_fix("with_etc"), etc_dirs=[_fix("nowhere"), _fix("etc")])
    assert dict(e) == dict(maxNonOrtho=64.0, minFaceWeight=0.02, minVol=1e-14) and e.ignored == ("relaxed",)
    o = read_mesh_quality_dict(_fix("override"), etc_dirs=[])
    assert dict(o) == dict(maxConcave=60.0, minVol=1e-10) and o.ignored == ("someList", "note")
    # etc_dirs=None: $WM_PROJECT_DIR/etc, then $FOAM_ETC
    monkeypatch.delenv("WM_PROJECT_DIR", raising=False)
    monkeypatch.setenv("FOAM_ETC", _fix("etc"))
    assert dict(read_mesh_quality_dict(_fix("with_etc"))) == dict(e)
    monkeypatch.delenv("FOAM_ETC")
    monkeypatch.setenv("WM_PROJECT_DIR", FIX)
    assert dict(read_mesh_quality_dict(_fix("with_etc"))) == dict(e)


ERRORS = [("err_cycle_a", [], ["err_cycle_b:3: ", "include cycle"]),
          ("err_missing_include", [], ["err_missing_include:2: ", "no_such_file"]),
          ("err_etc_missing", ["etc"], ["err_etc_missing:1: ", "caseDicts/noSuchDict", os.path.join(FIX, "etc")]),
          ("with_etc", [], ["with_etc:2: ", "caseDicts/meshQualityDict", "none was given"]),
          ("err_macro", [], ["err_macro:2: ", "$limit"]),
          ("err_brace", [], ["err_brace:3: ", "unterminated {"]),
          ("err_comment", [], ["err_comment:2: ", "unterminated /*"]),
          ("err_semicolon", [], ["err_semicolon:1: ", "missing ;"]),
          ("err_nonnumeric", [], ["err_nonnumeric:2: ", "minFlatness", "'half' is not a number"]),
          ("err_nan", [], ["err_nan:3: ", "minArea is NaN"]),
          ("err_directive", [], ["err_directive:1: ", "#inputMode"]),
          ("no_such_dict", [], ["no_such_dict", "cannot read"])]


@pytest.mark.parametrize("name,etc,pieces", ERRORS, ids=[e[0] for e in ERRORS])
def test_errors_name_file_and_line(name, etc, pieces):
    with pytest.raises(RuntimeError) as err:
        read_mesh_quality_dict(_fix(name), etc_dirs=[_fix(d) for d in etc])
    assert all(p in str(err.value) for p in pieces), str(err.value)


def test_include_depth_is_capped_at_16(tmp_path):
    for depth in (16, 17):
        d = tmp_path / str(depth)
        d.mkdir()
        for k in range(depth + 1):
            (d / f"f{k}").write_text(f'minVol {k};\n#include "f{k + 1}"\n' if k < depth else "maxConcave 33;\n")
        if depth == 16:
            assert dict(read_mesh_quality_dict(d / "f0", etc_dirs=[])) == dict(maxConcave=33.0, minVol=15.0)
        else:
            with pytest.raises(RuntimeError, match="f16:2: includes nested deeper than 16"):
                read_mesh_quality_dict(d / "f0", etc_dirs=[])


def test_front_end_refuses_before_any_device_work(tmp_path):
    """the dict option and a malformed dict end the front-end while it reads its options: no case is read, no device is opened"""
    case = str(tmp_path / "no_case")
    r = subprocess.run([BIN, "-case", case, "-meshQualityDict", "true"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-meshQualityDict needs -qualityConstraint true" in r.stdout
    for name, _, pieces in ERRORS:
        if name in ("with_etc", "err_etc_missing"):
            continue
        r = subprocess.run([BIN, "-case", case, "-qualityConstraint", "true", "-meshQualityDict", _fix(name)], capture_output=True, text=True, timeout=60,
                           env={k: v for k, v in os.environ.items() if k not in ("WM_PROJECT_DIR", "FOAM_ETC")})
        assert r.returncode != 0 and "-meshQualityDict: " in r.stdout and all(p in r.stdout for p in pieces), (name, r.stdout)
    # `true` is <case>/system/meshQualityDict, a relative path is relative to the case
    for value, where in (("true", "system/meshQualityDict"), ("dicts/mine", "dicts/mine")):
        r = subprocess.run([BIN, "-case", case, "-qualityConstraint", "true", "-meshQualityDict", value], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and f"{case}/{where}" in r.stdout and "cannot read" in r.stdout, r.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_reader_is_clean_under_asan_ubsan(tmp_path):
    """host code only: the stand-alone checker with its own main, the fixtures and the malformed inputs it writes itself"""
    exe = str(tmp_path / "dict_reader_check")
    host = os.path.join(ROOT, "smoothmesh_amd", "csrc", "host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", host, "-o", exe, os.path.join(ROOT, "tests", "native", "dict_reader_check.cpp"), os.path.join(host, "quality_dict.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, FIX, str(tmp_path / "scratch")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and "ERROR" not in r.stderr and "runtime error" not in r.stderr
