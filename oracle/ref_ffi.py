"""ctypes access to oracle/_ref/libsmref.so: the REFERENCE'S OWN program text, compiled against the stand-in OpenFOAM of
oracle/foam_shim/ (oracle/Makefile, target _ref/libsmref.so) and executed in serial.  TEST INFRASTRUCTURE ONLY.

The stand-in mesh takes from the harness everything that OpenFOAM, not the reference, decides: the addressing lists in the
oracle's order (Oracle.addressing(kind)) and the face / cell geometry (a callback into liboracle.so's updateGeometry, in the
.com or the .org form).  Everything else -- arithmetic, control flow, defaults, option handling, log lines -- is the reference's.

The reference keeps function-local statics sized by the first mesh they see, so every run() loads a fresh copy of the library."""
import ctypes as C
import os
import re
import shutil
import tempfile

import numpy as np

from . import oracle_ffi

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
LIBS = {"com": os.path.join(REF_DIR, "libsmref.so"), "org": os.path.join(REF_DIR, "libsmref_org.so")}
REFERENCE_SOURCE = os.environ.get("SMOOTHMESH_REFERENCE", "/root/reference")
ADDRESSING = ("pointCells", "pointPoints", "pointFaces", "pointEdges", "edgeFaces", "edgeCells", "cellPoints")
LINE = re.compile(r"Smoothing iteration=(\d+) nFrozenPoints=(\d+) residual=(\S+)")
CONSTANTS = ("GREAT", "VGREAT", "SMALL", "VSMALL", "ROOTVSMALL")

f64p = C.POINTER(C.c_double)
i32p = C.POINTER(C.c_int32)
GEOMETRY_FN = C.CFUNCTYPE(None, f64p, f64p, f64p, f64p, C.c_void_p)


class ReferenceError_(RuntimeError):
    """the reference ended through FatalError (or the stand-in refused something)"""


def available(variant="com"):
    return os.path.exists(LIBS[variant])


def source_present():
    return os.path.isdir(REFERENCE_SOURCE)


def build():
    """make oracle/_ref/libsmref.so (both variants) if the reference's source is on this machine"""
    import subprocess
    subprocess.check_call(["make", "-C", _HERE, "_ref/libsmref.so"])


def _load(variant):
    """a private copy of the library: its statics serve one run"""
    if not available(variant):
        raise FileNotFoundError(f"{LIBS[variant]} is missing: build it with `make -C oracle _ref/libsmref.so`")
    try:      # next to the library (a temporary directory may forbid loading code from it)
        fd, path = tempfile.mkstemp(prefix=".run_", suffix=".so", dir=REF_DIR)
    except OSError:
        fd, path = tempfile.mkstemp(prefix="libsmref_", suffix=".so")
    os.close(fd)
    try:
        shutil.copyfile(LIBS[variant], path)
        l = C.CDLL(path)
    finally:
        os.unlink(path)
    l.ref_set_mesh.argtypes = [C.c_int] * 4 + [f64p, i32p, i32p, i32p, i32p]
    l.ref_set_patches.argtypes = [C.c_int, C.POINTER(C.c_char_p), i32p, i32p, i32p]
    l.ref_set_edges.argtypes = [C.c_int, i32p]
    l.ref_set_addressing.argtypes = [C.c_char_p, C.c_int, i32p, i32p]
    l.ref_set_geometry.argtypes = [GEOMETRY_FN, C.c_void_p]
    l.ref_run.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    l.ref_run.restype = C.c_int
    for n in ("ref_last_error", "ref_log"):
        getattr(l, n).restype = C.c_char_p
    l.ref_write_name.restype = C.c_char_p
    l.ref_write_name.argtypes = [C.c_int]
    for n in ("ref_points_at", "ref_write_points"):
        getattr(l, n).argtypes = [C.c_int, f64p]
        getattr(l, n).restype = C.c_int
    l.ref_constants.argtypes = [f64p]
    v3 = [f64p, f64p, f64p]
    l.ref_edgeEdgeAngle.argtypes = v3
    l.ref_edgeEdgeAngle.restype = C.c_double
    l.ref_calcEdgeCenterEdgeAngle.argtypes = v3
    l.ref_calcEdgeCenterEdgeAngle.restype = C.c_double
    l.ref_calcARSmoothingRatio.argtypes = v3 + [C.c_int, C.c_int]
    l.ref_calcARSmoothingRatio.restype = C.c_double
    l.ref_isCloserPoint.argtypes = [f64p, f64p]
    l.ref_isSmallerByVectorElements.argtypes = [f64p, f64p]
    l.ref_calcMinMaxFinalProjectedAngle.argtypes = [C.c_int, C.c_int, f64p, f64p, i32p, i32p, f64p]
    l.ref_getMeshStats.argtypes = [f64p]
    return l


def _p(a, t):
    return a.ctypes.data_as(t)


def _v(x):
    a = np.ascontiguousarray(x, dtype=np.float64).reshape(3)
    return a, _p(a, f64p)


class Run:
    """what one execution of the reference's main() left behind"""

    def __init__(self, points, nFrozenPoints, residuals, log, written):
        self.points = points                  # list: the mesh points after every iteration (every mesh.movePoints)
        self.nFrozenPoints = nFrozenPoints    # int64 array, from the "Smoothing iteration=" lines
        self.residuals = residuals            # list of str, as the reference prints them
        self.log = log                        # everything written to Info
        self.written = written                # list of (time name, points) of every mesh.write()

    def __iter__(self):
        return iter((self.points, self.nFrozenPoints, self.residuals, self.log))


class _Session:
    """one loaded copy of the library with a mesh handed over"""

    def __init__(self, mesh, variant="com"):
        self.lib = _load(variant)
        self.mesh = mesh
        self._geo = oracle_ffi.Oracle(mesh)          # serves geometry only; never iterated
        self._geo.set_foam_variant(variant)
        self._keep = []
        o = self._geo
        pts = np.ascontiguousarray(mesh.points, dtype=np.float64)
        self.lib.ref_set_mesh(mesh.nPoints, mesh.nCells, mesh.nFaces, mesh.nInternalFaces, _p(pts, f64p), _p(mesh.faceOffsets, i32p),
                              _p(mesh.facePoints, i32p), _p(mesh.owner, i32p), _p(mesh.neighbour, i32p))
        kinds = {"processor": 1, "empty": 2}
        names = (C.c_char_p * len(mesh.patches))(*[p.name.encode() for p in mesh.patches])
        st = np.array([p.startFace for p in mesh.patches], np.int32)
        sz = np.array([p.nFaces for p in mesh.patches], np.int32)
        kd = np.array([kinds.get(p.type, 0) for p in mesh.patches], np.int32)
        self.lib.ref_set_patches(len(mesh.patches), names, _p(st, i32p), _p(sz, i32p), _p(kd, i32p))
        _, edges = o.addressing("edges")
        edges = np.ascontiguousarray(edges, np.int32)
        self.lib.ref_set_edges(len(edges), _p(edges, i32p))
        for kind in ADDRESSING:
            off, val = o.addressing(kind)
            self.lib.ref_set_addressing(kind.encode(), len(off) - 1, _p(off, i32p), _p(val, i32p))
        nP, nF, nC = mesh.nPoints, mesh.nFaces, mesh.nCells

        def geometry(points, fc, fa, cc, _user):
            o.set_points(np.ctypeslib.as_array(points, shape=(nP * 3,)))
            o.update_geometry()
            np.ctypeslib.as_array(fc, shape=(nF * 3,))[:] = o.field("faceCentres")
            np.ctypeslib.as_array(fa, shape=(nF * 3,))[:] = o.field("faceAreas")
            np.ctypeslib.as_array(cc, shape=(nC * 3,))[:] = o.field("cellCentres")

        self._cb = GEOMETRY_FN(geometry)
        self.lib.ref_set_geometry(self._cb, None)

    def error(self):
        return self.lib.ref_last_error().decode()


def run(mesh, argv, variant="com"):
    """Execute the reference's main() with the option list `argv` (without the program name) on `mesh`.
    Returns a Run: (points per iteration, nFrozenPoints[], residual strings, log) when unpacked."""
    s = _Session(mesh, variant)
    args = [b"smoothMesh"] + [str(a).encode() for a in argv]
    arr = (C.c_char_p * len(args))(*args)
    rc = s.lib.ref_run(len(args), arr)
    log = s.lib.ref_log().decode()
    if rc != 0:
        raise ReferenceError_(s.error() + "\n--- log ---\n" + log[-2000:])
    n3 = mesh.nPoints * 3
    pts = []
    for i in range(s.lib.ref_num_moves()):
        a = np.empty(n3, np.float64)
        assert s.lib.ref_points_at(i, _p(a, f64p)) == n3
        pts.append(a.reshape(-1, 3))
    written = []
    for i in range(s.lib.ref_num_writes()):
        a = np.empty(n3, np.float64)
        assert s.lib.ref_write_points(i, _p(a, f64p)) == n3
        written.append((s.lib.ref_write_name(i).decode(), a.reshape(-1, 3)))
    lines = LINE.findall(log)
    assert [int(a) for a, _, _ in lines] == list(range(1, len(lines) + 1)), "iteration lines out of order"
    return Run(pts, np.array([int(b) for _, b, _ in lines], np.int64), [c for _, _, c in lines], log, written)


def mesh_stats(mesh, variant="com"):
    """the reference's getMeshStats: (minEdgeLength, maxEdgeLength, meshPerimeter)"""
    s = _Session(mesh, variant)
    out = np.zeros(3)
    if s.lib.ref_getMeshStats(_p(out, f64p)) != 0:
        raise ReferenceError_(s.error())
    return tuple(out)


class Functions:
    """single functions of the reference, called with chosen arguments (no mesh needed)"""

    def __init__(self, variant="com"):
        self.lib = _load(variant)

    def constants(self):
        out = np.zeros(5)
        self.lib.ref_constants(_p(out, f64p))
        return dict(zip(CONSTANTS, out.tolist()))

    def edgeEdgeAngle(self, c, p1, p2):
        (a, pa), (b, pb), (d, pd) = _v(c), _v(p1), _v(p2)
        return self.lib.ref_edgeEdgeAngle(pa, pb, pd)

    def calcEdgeCenterEdgeAngle(self, p0, cC, p1):
        (a, pa), (b, pb), (d, pd) = _v(p0), _v(cC), _v(p1)
        return self.lib.ref_calcEdgeCenterEdgeAngle(pa, pb, pd)

    def calcARSmoothingRatio(self, c1, c2, c3, hasCommonCell, isInternalPoint):
        (a, pa), (b, pb), (d, pd) = _v(c1), _v(c2), _v(c3)
        return self.lib.ref_calcARSmoothingRatio(pa, pb, pd, int(hasCommonCell), int(isInternalPoint))

    def isCloserPoint(self, x, y):
        (a, pa), (b, pb) = _v(x), _v(y)
        return bool(self.lib.ref_isCloserPoint(pa, pb))

    def isSmallerByVectorElements(self, x, y):
        (a, pa), (b, pb) = _v(x), _v(y)
        return bool(self.lib.ref_isSmallerByVectorElements(pa, pb))

    def calcMinMaxFinalProjectedAngle(self, pVecs, cVecs, f0Is, f1Is):
        p = np.ascontiguousarray(pVecs, np.float64).reshape(-1, 3)
        c = np.ascontiguousarray(cVecs, np.float64).reshape(-1, 3)
        f0, f1 = np.ascontiguousarray(f0Is, np.int32), np.ascontiguousarray(f1Is, np.int32)
        out = np.zeros(2)
        if self.lib.ref_calcMinMaxFinalProjectedAngle(len(c), len(p), _p(p, f64p), _p(c, f64p), _p(f0, i32p), _p(f1, i32p), _p(out, f64p)) != 0:
            raise ReferenceError_(self.lib.ref_last_error().decode())
        return out[0], out[1]
