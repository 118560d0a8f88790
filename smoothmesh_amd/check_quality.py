"""python -m smoothmesh_amd.check_quality -case <dir> [-parallel] [-time <t|constant|latestTime>]

Prints the mesh quality report of a case in the format of `smoothMesh -checkQuality` (one block, label "mesh"): the serial
case, or with -parallel every processorN/ sub-domain combined into the report of the whole mesh (smoothmesh_amd/quality.py).
Ids are global where the sub-domains carry cellProcAddressing and faceProcAddressing, else -1.  Time selection as smoothMesh:
the latest time directory by default, else constant; the faces from the newest instance at or before it, the points likewise.
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


def case_quality(case, parallel=False, time=None, device=0):
    """MeshQuality of the serial case, or DecomposedMeshQuality of its processorN/ sub-domains"""
    if not parallel:
        from .engine import SmoothEngine
        e = SmoothEngine(_read(case, _select_time(case, time)), device=device)
        try:
            return e.mesh_quality()
        finally:
            e.close()
    from .decompose import SubDomain
    from .quality import decomposed_mesh_quality
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
    return decomposed_mesh_quality(subs, device=device)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m smoothmesh_amd.check_quality", description=__doc__.splitlines()[2])
    ap.add_argument("-case", default=".")
    ap.add_argument("-parallel", action="store_true")
    ap.add_argument("-time", default=None, help="a time, constant or latestTime (default: the latest time, else constant)")
    a = ap.parse_args(argv)
    from .quality import format_report
    q = case_quality(a.case, a.parallel, a.time)
    sys.stdout.write(format_report(q, "mesh"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
