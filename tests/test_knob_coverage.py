"""Every SMGPU_* setting the native code reads (envInt / getenv under smoothmesh_amd/csrc) is named by a test, by a script a test
runs, or below with the reason it is not.  DESIGN.md section 7 says which knobs the tests hold to what; this keeps that true."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# scripts the suite runs (tests/test_gpu_fuzz.py, tests/test_gpu_multirank.py)
SCRIPTS_RUN_BY_TESTS = ("scripts/fuzz_parity.py", "scripts/check_arrangements.py")

NOT_COVERED = {
    "SMGPU_DUMP_WALK": "diagnostics only: dumps the face-angle walk's inputs to a file",
    "SMGPU_DUMP_WALK_CALL": "diagnostics only: which call SMGPU_DUMP_WALK dumps",
    "SMGPU_WALK_STATS": "diagnostics only: prints walk statistics",
    "SMGPU_WALK_MEMO_STATS": "diagnostics only: prints walk memo statistics",
    "SMGPU_HALO_DEBUG": "changes results by design: a measurement aid that skips the pack role's work or its wait",
    "SMGPU_PUSH_FENCE": "an A/B fence of the peer-store hand-off, not a result",
    "SMGPU_FOAM_VARIANT": "the same setting as SmoothEngine.set_foam_variant, which the tests use",
    "SMGPU_SYNC_VARIANT": "the same setting as the engine's sync-variant call, which the tests use",
}


def _knobs():
    names = {}
    for p in glob.glob(os.path.join(ROOT, "smoothmesh_amd", "csrc", "**", "*"), recursive=True):
        if not p.endswith((".hip", ".hpp", ".cpp", ".h")):
            continue
        with open(p, errors="replace") as f:
            for m in re.finditer(r'\b(?:envInt|getenv)\s*\(\s*"(SMGPU_\w+)"', f.read()):
                names.setdefault(m.group(1), os.path.relpath(p, ROOT))
    return names


def _covering_text():
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))) + [os.path.join(ROOT, s) for s in SCRIPTS_RUN_BY_TESTS]
    out = []
    for p in paths:
        if os.path.basename(p) == os.path.basename(__file__):
            continue
        with open(p) as f:
            out.append(f.read())
    return "\n".join(out)


def test_every_knob_is_tested_or_listed_with_a_reason():
    knobs = _knobs()
    assert len(knobs) > 40 and "SMGPU_GEOM_T" in knobs and "SMGPU_TILE_SEGMENTS" in knobs
    text = _covering_text()
    covered = {k for k in knobs if re.search(r"\b%s\b" % k, text)}
    missing = sorted(set(knobs) - covered - set(NOT_COVERED))
    assert not missing, "read by the native code, named by no test and not listed: " + ", ".join(f"{k} ({knobs[k]})" for k in missing)
    # the list is exactly what stays uncovered: no entry for a knob that is gone or that a test names by now
    assert not sorted(set(NOT_COVERED) - set(knobs)), "listed but no longer read"
    assert not sorted(set(NOT_COVERED) & covered), "listed but named by a test: drop it from NOT_COVERED"
    assert all(r.strip() for r in NOT_COVERED.values())
    # ... and what stays is diagnostics, time-outs and aliases of calls the tests use: nothing waits for a test
    assert not [k for k, r in NOT_COVERED.items() if r.strip().lower().startswith("not yet covered")]


def test_the_tile_shape_knobs_are_named_by_the_tile_tests():
    """the knobs that shape the LDS tiles are exercised where the results are checked (test_gpu_tile_shapes, test_tile_tables)"""
    with open(os.path.join(ROOT, "tests", "test_gpu_tile_shapes.py")) as f:
        gpu = f.read()
    for k in ("SMGPU_GEOM_T", "SMGPU_SMOOTH_T", "SMGPU_GEOM_CELLS", "SMGPU_GEOM_CAPP", "SMGPU_GEOM_CAPF", "SMGPU_GEOM_CAPWEIGHTED",
              "SMGPU_SMOOTH_CAPC", "SMGPU_SMOOTH_CAPN", "SMGPU_SMOOTH_CAPTOTAL", "SMGPU_EDGE_CAPP", "SMGPU_EDGE_CAPF", "SMGPU_EDGE_CAPC",
              "SMGPU_EDGE_CAPTOTAL", "SMGPU_DEFER_FINISH"):
        assert k in gpu, k
    with open(os.path.join(ROOT, "tests", "test_tile_tables.py")) as f:
        assert "SMGPU_TILE_SEGMENTS" in f.read()
