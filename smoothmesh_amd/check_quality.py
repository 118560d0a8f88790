"""python -m smoothmesh_amd.check_quality -case <dir> [-parallel] [-time <t|constant|latestTime>] [-writeSets] [-allGeometry] [-meshQuality]

Prints the mesh quality report of a case in the format of `smoothMesh -checkQuality` (one block, label "mesh"): the serial
case, or with -parallel every processorN/ sub-domain combined into the report of the whole mesh (smoothmesh_amd/quality.py).
Ids are global where the sub-domains carry cellProcAddressing and faceProcAddressing, else -1.  Time selection as smoothMesh:
the latest time directory by default, else constant; the faces from the newest instance at or before it, the points likewise.
-writeSets: then the failing elements as OpenFOAM sets into <points instance>/sets, i.e. <time>/polyMesh/sets
or constant/polyMesh/sets, in every processorN/ with local ids under -parallel; writeFormat and writeCompression from
system/controlDict.  One "<<Writing" line per written set follows the report (with " in processorN" under -parallel).
With -allGeometry and / or -meshQuality on a serial case, -writeSets also writes the non-empty sets of those reports (DESIGN.md
10.9) into the same sets/ directory, their "<<Writing" lines after the seven's: geometry first, then motion.  A decomposed case
gets them through decomposed_case_quality(..., write_sets=True).
-allGeometry: the block also carries the five lines of the checks `checkMesh -allGeometry` adds; serial cases only.
-meshQuality: the block also carries the four lines of the motion criteria, face and base-point tet quality, face twist and triangle
twist, after those of -allGeometry; serial cases only.
"""
import os
import re
import sys

import numpy as np

_NUM = re.compile(r"^[-+]?(\d+\.?\d*|\.\d+)([eE][-+]?\d+)?$")


def _times(root):
    return sorted((float(d), d) for d in os.listdir(root) if _NUM.match(d) and os.path.isdir(os.path.join(root, d)))


def _has(d, name):
    return os.path.exists(os.path.join(d, name)) or os.path.exists(os.path.join(d, name + ".gz"))


def _instance(root, t, name):
    """polyMesh directory holding `name` at time t (None = constant) or the newest time before it, else constant/polyMesh"""
    if t is not None:
        for v, d in reversed(_times(root)):
            if v <= t and _has(os.path.join(root, d, "polyMesh"), name):
                return os.path.join(root, d, "polyMesh")
    return os.path.join(root, "constant", "polyMesh")


def _select_time(root, opt):
    if opt == "constant":
        return None
    if opt in (None, "latestTime"):
        ts = _times(root)
        return ts[-1][0] if ts else None
    return float(opt)


def _read(root, t):
    from .polymesh import read_polymesh
    mesh_dir, pts_dir = _instance(root, t, "faces"), _instance(root, t, "points")
    return read_polymesh(mesh_dir, None if pts_dir == mesh_dir else pts_dir)


def _addressing(root, name):
    from .polymesh import read_label_list
    d = os.path.join(root, "constant", "polyMesh")
    if not _has(d, name):
        return None
    return read_label_list(os.path.join(d, name)).astype(np.int64)


def _control(case):
    """(binary, compressed) from system/controlDict's writeFormat and writeCompression"""
    try:
        with open(os.path.join(case, "system", "controlDict")) as f:
            txt = f.read()
    except OSError:
        return False, False
    fmt = re.search(r"^\s*writeFormat\s+(\w+)\s*;", txt, re.M)
    cmp = re.search(r"^\s*writeCompression\s+(\w+)\s*;", txt, re.M)
    return (fmt is not None and fmt.group(1) == "binary",
            cmp is not None and cmp.group(1) in ("on", "true", "yes", "compressed"))


def _write_sets(pts_dir, root, sets, control, table=None):
    from .polymesh import set_write_compression
    from .quality import QUALITY_SETS, write_quality_sets
    binary, compressed = control
    set_write_compression(compressed)
    try:
        return write_quality_sets(pts_dir, os.path.relpath(pts_dir, root), sets, binary, table or QUALITY_SETS)
    finally:
        set_write_compression(False)


ALL_GEOMETRY_PARALLEL_REFUSAL = ("check_quality: -allGeometry is not available with -parallel: face weight and volume ratio across processor "
                                 "faces need the neighbour rank's cell volume, which the decomposed report does not exchange (run it on the "
                                 "reconstructed case)")


MESH_QUALITY_PARALLEL_REFUSAL = ("check_quality: -meshQuality is not available with -parallel: the tets and the twist of a processor face "
                                 "need the neighbour rank's cell centre, which the decomposed report does not exchange for them (run it on "
                                 "the reconstructed case)")


def _read_subs(case, time):
    """(processor directories [(rank, name)], the selected time, the SubDomain of every processorN/)"""
    from .decompose import SubDomain
    procs = sorted((int(d[9:]), d) for d in os.listdir(case) if re.fullmatch(r"processor\d+", d))
    if not procs or [p[0] for p in procs] != list(range(len(procs))):
        raise SystemExit(f"check_quality: no processor0 .. processorN-1 directories in {case}")
    t = _select_time(os.path.join(case, procs[0][1]), time)
    subs = []
    for r, d in procs:
        root = os.path.join(case, d)
        m = _read(root, t)
        faces = _addressing(root, "faceProcAddressing")
        subs.append(SubDomain(m, r, len(procs), np.zeros(0, np.int64), _addressing(root, "cellProcAddressing"),
                              None if faces is None else np.abs(faces) - 1))          # decomposePar: +-(global face + 1)
    return procs, t, subs


def decomposed_case_quality(case, time=None, device=0, all_geometry=False, mesh_quality=False, write_sets=False):
    """The reports of a decomposed case, every processorN/ combined: (DecomposedMeshQuality,
    DecomposedMeshQualityGeometry or None, DecomposedMeshQualityMotion or None), which format_report(*q) prints as one block.  The
    shell spellings -parallel -allGeometry / -meshQuality keep their refusals; this function is the way in.
    write_sets: also write every processorN/'s sets, local ids, of the reports asked for (the seven, then geometry, then motion:
    DESIGN.md 10.5, 10.9) into its points instance -> (the triple, [(rank, name, size)] in writing order)."""
    from . import quality as Q
    procs, t, subs = _read_subs(case, time)
    q = (Q.decomposed_mesh_quality(subs, device=device),
         Q.decomposed_mesh_quality_geometry(subs, device=device) if all_geometry else None,
         Q.decomposed_mesh_quality_motion(subs, device=device) if mesh_quality else None)
    if not write_sets:
        return q
    control = _control(case)
    kinds = [(Q.decomposed_quality_sets, Q.QUALITY_SETS)]
    if all_geometry:
        kinds.append((Q.decomposed_quality_geometry_sets, Q.QUALITY_GEOMETRY_SETS))
    if mesh_quality:
        kinds.append((Q.decomposed_quality_motion_sets, Q.QUALITY_MOTION_SETS))
    per_kind = [(fn(subs, device=device), table) for fn, table in kinds]
    written = []
    for i, (r, d) in enumerate(procs):
        root = os.path.join(case, d)
        for ranks, table in per_kind:
            written += [(r, n, k) for n, k in _write_sets(_instance(root, t, "points"), root, ranks[i], control, table)]
    return q, written


def case_quality(case, parallel=False, time=None, device=0, write_sets=False, all_geometry=False, mesh_quality=False):
    """MeshQuality of the serial case, or DecomposedMeshQuality of its processorN/ sub-domains.  write_sets: also write the
    failing elements as sets into the points instance (every processorN/ under parallel) -> (quality, [(rank, name, size)]);
    with all_geometry / mesh_quality also the sets of those reports, after the seven.
    all_geometry (serial only): the quality is the pair (MeshQuality, MeshQualityGeometry); mesh_quality (serial only): the triple
    (MeshQuality, MeshQualityGeometry or None, MeshQualityMotion)"""
    if all_geometry and parallel:
        raise SystemExit(ALL_GEOMETRY_PARALLEL_REFUSAL)
    if mesh_quality and parallel:
        raise SystemExit(MESH_QUALITY_PARALLEL_REFUSAL)
    control = _control(case)
    if not parallel:
        from .engine import SmoothEngine
        t = _select_time(case, time)
        e = SmoothEngine(_read(case, t), device=device)
        try:
            q = e.mesh_quality()
            if mesh_quality:
                q = (q, e.mesh_quality_geometry() if all_geometry else None, e.mesh_quality_motion())
            elif all_geometry:
                q = (q, e.mesh_quality_geometry())
            if not write_sets:
                return q
            from .quality import QUALITY_GEOMETRY_SETS, QUALITY_MOTION_SETS
            pts_dir = _instance(case, t, "points")
            written = _write_sets(pts_dir, case, e.quality_sets(), control)
            if all_geometry:
                written += _write_sets(pts_dir, case, e.quality_geometry_sets(), control, QUALITY_GEOMETRY_SETS)
            if mesh_quality:
                written += _write_sets(pts_dir, case, e.quality_motion_sets(), control, QUALITY_MOTION_SETS)
            return q, [(None, n, k) for n, k in written]
        finally:
            e.close()
    from .quality import decomposed_mesh_quality, decomposed_quality_sets
    procs, t, subs = _read_subs(case, time)
    q = decomposed_mesh_quality(subs, device=device)
    if not write_sets:
        return q
    written = []
    for (r, d), sets in zip(procs, decomposed_quality_sets(subs, device=device)):
        root = os.path.join(case, d)
        written += [(r, n, k) for n, k in _write_sets(_instance(root, t, "points"), root, sets, control)]
    return q, written


def format_written(written):
    """the "<<Writing" lines of -writeSets: (rank or None, name, size) in writing order"""
    from .quality import QUALITY_GEOMETRY_SETS, QUALITY_MOTION_SETS, QUALITY_SETS, format_sets_written
    table = QUALITY_SETS + QUALITY_GEOMETRY_SETS + QUALITY_MOTION_SETS
    return "".join(format_sets_written([(n, k)], table).rstrip("\n") + ("" if r is None else f" in processor{r}") + "\n"
                   for r, n, k in written)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m smoothmesh_amd.check_quality", description=__doc__.splitlines()[2])
    ap.add_argument("-case", default=".")
    ap.add_argument("-parallel", action="store_true")
    ap.add_argument("-time", default=None, help="a time, constant or latestTime (default: the latest time, else constant)")
    ap.add_argument("-writeSets", action="store_true", help="write the failing faces and cells as sets into the points instance; with -allGeometry / -meshQuality also "
                    "those reports' sets")
    ap.add_argument("-allGeometry", action="store_true", help="also concavity, flatness, weight, volume ratio, determinant (serial only)")
    ap.add_argument("-meshQuality", action="store_true", help="also face and base-point tet quality, twist, triangle twist (serial only)")
    a = ap.parse_args(argv)
    from .quality import format_report
    if a.allGeometry and a.parallel:
        raise SystemExit(ALL_GEOMETRY_PARALLEL_REFUSAL)
    if a.meshQuality and a.parallel:
        raise SystemExit(MESH_QUALITY_PARALLEL_REFUSAL)
    geo = dict(all_geometry=True) if a.allGeometry else {}
    if a.meshQuality:
        geo["mesh_quality"] = True
    fmt = (lambda q: format_report(q[0], "mesh", *q[1:])) if geo else (lambda q: format_report(q, "mesh"))
    if not a.writeSets:
        sys.stdout.write(fmt(case_quality(a.case, a.parallel, a.time, **geo)))
        return 0
    q, written = case_quality(a.case, a.parallel, a.time, write_sets=True, **geo)
    sys.stdout.write(fmt(q) + format_written(written))
    return 0


if __name__ == "__main__":
    sys.exit(main())
