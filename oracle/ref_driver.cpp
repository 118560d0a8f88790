// ref_driver.cpp -- runs the REFERENCE's own program text on the stand-in OpenFOAM of oracle/foam_shim/.
// TEST INFRASTRUCTURE ONLY.  This file holds no reference text: the reference's translation unit is pulled in by the
// #include below from $(SMOOTHMESH_REFERENCE)/src at build time (oracle/Makefile, target _ref/libsmref.so), its main()
// renamed to reference_main by -Dmain=reference_main.  The product (smoothmesh_amd/) never links this.
//
// The reference keeps function-local statics that are sized by the first mesh they see, so ONE LOADED COPY OF THIS LIBRARY
// SERVES ONE ref_run: oracle/ref_ffi.py loads a fresh copy for every run.
#include "foam_shim/foamShim.C"

#include "smoothMesh.C"   // the reference: src/smoothMesh.C, which includes its other two source files

#include <cstring>

namespace
{
std::string g_error, g_log;
bool g_ran = false;
int copyOut(const std::vector<double>& v, double* out) { if (out) std::memcpy(out, v.data(), v.size() * sizeof(double)); return int(v.size()); }
template<class F> int guarded(F f)
{
    g_error.clear();
    try { return f(); }
    catch (const std::exception& e) { g_error = e.what(); if (g_error.empty()) g_error = "error"; }
    catch (...) { g_error = "unknown exception"; }
    return -1;
}
Foam::vector V(const double* p) { return Foam::vector(p[0], p[1], p[2]); }
}

extern "C" {

void ref_set_mesh(int nPoints, int nCells, int nFaces, int nInternalFaces, const double* points, const int* faceOffsets,
                  const int* facePoints, const int* owner, const int* neighbour)
{
    Foam::shim::MeshInput& m = Foam::shim::meshInput();
    m.nPoints = nPoints; m.nCells = nCells; m.nFaces = nFaces; m.nInternalFaces = nInternalFaces;
    m.points.assign(points, points + 3 * size_t(nPoints));
    m.faces.assign(size_t(nFaces), std::vector<int>());
    for (int f = 0; f < nFaces; ++f) m.faces[size_t(f)].assign(facePoints + faceOffsets[f], facePoints + faceOffsets[f + 1]);
    m.owner.assign(owner, owner + nFaces);
    m.neighbour.assign(neighbour, neighbour + nInternalFaces);
}
void ref_set_patches(int nPatches, const char* const* names, const int* start, const int* size, const int* kind)
{
    Foam::shim::MeshInput& m = Foam::shim::meshInput();
    m.patchName.assign(names, names + nPatches);
    m.patchStart.assign(start, start + nPatches);
    m.patchSize.assign(size, size + nPatches);
    m.patchKind.assign(kind, kind + nPatches);
}
void ref_set_edges(int nEdges, const int* edges)
{
    Foam::shim::MeshInput& m = Foam::shim::meshInput();
    m.nEdges = nEdges;
    m.edges.assign(edges, edges + 2 * size_t(nEdges));
}
void ref_set_addressing(const char* kind, int rows, const int* offsets, const int* values)
{
    std::vector<std::vector<int> >& a = Foam::shim::meshInput().addressing[kind];
    a.assign(size_t(rows), std::vector<int>());
    for (int r = 0; r < rows; ++r) a[size_t(r)].assign(values + offsets[r], values + offsets[r + 1]);
}
void ref_set_geometry(Foam::shim::GeometryFn fn, void* user)
{
    Foam::shim::meshInput().geometry = fn;
    Foam::shim::meshInput().geometryUser = user;
}

// the reference's whole main(); 0 = it returned normally, -1 = see ref_last_error()
int ref_run(int argc, const char* const* argv)
{
    if (g_ran) { g_error = "ref_run: one loaded copy of this library serves one run (function-local statics of the reference)"; return -1; }
    g_ran = true;
    Foam::argList::clearRegistered();
    std::vector<std::string> store(argv, argv + argc);
    std::vector<char*> av;
    for (size_t i = 0; i < store.size(); ++i) av.push_back(&store[i][0]);
    av.push_back(nullptr);
    const int rc = guarded([&]() { return reference_main(argc, av.data()); });
    Foam::shim::currentTime() = nullptr;
    g_log = Foam::shim::infoBuffer().str();
    return rc;
}
const char* ref_last_error() { return g_error.c_str(); }
const char* ref_log() { g_log = Foam::shim::infoBuffer().str(); return g_log.c_str(); }
int ref_num_moves() { return int(Foam::shim::recorder().moved.size()); }
int ref_points_at(int i, double* out)
{
    const Foam::shim::Recorder& r = Foam::shim::recorder();
    return (i < 0 || i >= int(r.moved.size())) ? -1 : copyOut(r.moved[size_t(i)], out);
}
int ref_num_writes() { return int(Foam::shim::recorder().written.size()); }
const char* ref_write_name(int i)
{
    const Foam::shim::Recorder& r = Foam::shim::recorder();
    return (i < 0 || i >= int(r.writeName.size())) ? "" : r.writeName[size_t(i)].c_str();
}
int ref_write_points(int i, double* out)
{
    const Foam::shim::Recorder& r = Foam::shim::recorder();
    return (i < 0 || i >= int(r.written.size())) ? -1 : copyOut(r.written[size_t(i)], out);
}
// GREAT, VGREAT, SMALL, VSMALL, ROOTVSMALL as the stand-in holds them
void ref_constants(double* out) { out[0] = Foam::GREAT; out[1] = Foam::VGREAT; out[2] = Foam::SMALL; out[3] = Foam::VSMALL; out[4] = Foam::ROOTVSMALL; }
int ref_is_org()
{
#ifdef OPENFOAM_ORG
    return 1;
#else
    return 0;
#endif
}

// ---- single functions of the reference, with chosen arguments
double ref_edgeEdgeAngle(const double* c, const double* p1, const double* p2) { return edgeEdgeAngle(V(c), V(p1), V(p2)); }
double ref_calcEdgeCenterEdgeAngle(const double* p0, const double* cC, const double* p1) { return calcEdgeCenterEdgeAngle(V(p0), V(cC), V(p1)); }
double ref_calcARSmoothingRatio(const double* c1, const double* c2, const double* c3, int hasCommonCell, int isInternalPoint)
{
    return calcARSmoothingRatio(V(c1), V(c2), V(c3), hasCommonCell != 0, isInternalPoint != 0);
}
int ref_isCloserPoint(const double* a, const double* b) { return isCloserPoint(V(a), V(b)) ? 1 : 0; }
int ref_isSmallerByVectorElements(const double* a, const double* b) { return isSmallerByVectorElements(V(a), V(b)) ? 1 : 0; }
// pVecs: nFaces x 3, cVecs: nCells x 3, f0Is / f1Is: nCells; out = {min, max}
int ref_calcMinMaxFinalProjectedAngle(int nCells, int nFaces, const double* pVecs, const double* cVecs, const int* f0Is, const int* f1Is, double* out)
{
    return guarded([&]() {
        Foam::vectorList p(nFaces), c(nCells);
        Foam::labelList faceIs(nFaces, 0), f0(nCells), f1(nCells);
        for (int i = 0; i < nFaces; ++i) p[i] = V(pVecs + 3 * i);
        for (int i = 0; i < nCells; ++i) { c[i] = V(cVecs + 3 * i); f0[i] = f0Is[i]; f1[i] = f1Is[i]; }
        return calcMinMaxFinalProjectedAngle(nCells, p, c, faceIs, f0, f1, out[0], out[1]);
    });
}
// on the mesh handed over by ref_set_*: out = {minEdgeLength, maxEdgeLength, meshPerimeter}
int ref_getMeshStats(double* out)
{
    return guarded([&]() { Foam::fvMesh mesh; return getMeshStats(mesh, out[0], out[1], out[2]); });
}

}  // extern "C"
