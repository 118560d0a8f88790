// tiles.hpp -- LDS staging tables.
//
// The gather kernels of the loop (cell centres from faces from points; per-point sums of cell
// centres and neighbour coordinates) read 24-byte elements through int32 index lists.  Done straight
// from global memory, every wave instruction touches dozens of cache lines and every list walk is a
// chain of dependent loads: the kernels end up latency / L1-line bound, far from HBM.  Instead the
// element range is cut into TILES (consecutive cells / points, one workgroup each).  For every tile
// the host lists, once, the unique source elements the tile needs (ascending ids => coalesced block
// loads into LDS) and rewrites the index lists as 16-bit LDS-local indices in a sliced-ELL layout:
// fixed width per tile, 4 entries (8 bytes) per lane per load, lane-contiguous, so a thread fetches
// its whole adjacency with a couple of independent coalesced loads.  In the kernels all indexed
// access then happens inside LDS and global memory is only streamed.  Arithmetic and summation
// order are unchanged (entries keep the list order, 0xFFFF pads the tail).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "tile_meta.hpp"
#include "topology.hpp"

namespace smgpu {

constexpr uint16_t kEllPad = 0xFFFF;

// The frame of the Z-curve keys of n elements whose coordinates fill the box lo..hi: key = interleave((u64)((x - origin) * scale)).
//  - bounding-box keys: 21 bits per axis of the box's longest side (one isotropic scale).  The octree splits of a 100-cell axis
//    then fall at 50, 25, 12.5, ...: runs of consecutive elements are ragged, not the bricks of the mesh's own lattice.
//  - lattice keys (SMGPU_TILE_LATTICE, default on): the index of the element on a lattice of the mean spacing h, n elements at
//    the nodes of a lattice that fills the box: prod_a (ext_a / h + 1) = n, i.e. h = cbrt(box volume / n) corrected for the
//    half spacing the outermost elements keep from the box (cell centres) -- solved by a fixed-point iteration that starts there.
//    The origin lies h/2 below the box, so that an element on its node sits in the middle of its interval: jitter of up to
//    h/2 leaves the index alone.  Wherever the mesh is locally structured, 2^k consecutive keys are an aligned brick of it.
//    Falls back to the bounding-box keys when h is degenerate or an axis would need more than 21 bits.
// The host (tiles.cpp) and the device (tiles_dev.hip) builds of an order both take their frame from here.
struct MortonFrame { double origin[3]; double scale; int bits; bool lattice; };     // bits: per axis, of the largest index
// SMGPU_TILE_LATTICE where it is set (1 forces lattice keys on any mesh, 0 the bounding-box keys); else the caller's default.  The
// engine's default follows the mesh (tileLatticeDefault): on for meshes of hexahedra alone, off for the others -- on the castellated
// polyhedral mesh lattice keys were measured 0.9 % (constraints off) and 1.4 % (on) SLOWER than bounding-box keys, beyond the 0.4 %
// / 0.2 % run-to-run spread (profiles/tile_lattice_sharing.md, "The polyhedral configurations").  The builders used on their own
// (GeomTiles::latticeKeys etc., mortonOrderOf) default to ON whatever the mesh: that is how the CPU tests hold lattice keys to the
// polyhedral, baffle and fan meshes too.
inline bool tileLatticeKnob(bool dflt = true) { const char* e = std::getenv("SMGPU_TILE_LATTICE"); return e ? std::atoi(e) != 0 : dflt; }
// hexahedra alone, read off the counts: every face a quadrilateral, and six faces per cell (each internal face counts for two cells)
inline bool tileLatticeDefault(int64_t nCells, int64_t nFaces, int64_t nInternalFaces, int64_t nFacePoints) {
    return nFaces > 0 && nFacePoints == 4 * nFaces && nFaces + nInternalFaces == 6 * nCells;
}
inline MortonFrame mortonFrame(int64_t n, const double lo[3], const double hi[3], bool lattice) {
    MortonFrame f{{lo[0], lo[1], lo[2]}, 0.0, 21, false};
    double ext = 0.0, e[3];
    for (int a = 0; a < 3; ++a) { e[a] = hi[a] - lo[a]; ext = std::max(ext, e[a]); }
    f.scale = ext > 0.0 ? 2097151.0 / ext : 0.0;
    if (!lattice || n < 2 || !(ext > 0.0) || !std::isfinite(ext)) return f;
    int k = 0;
    double h = 1.0;
    for (int a = 0; a < 3; ++a) if (e[a] > 0.0) { h *= e[a]; ++k; }
    h = std::pow(h / (double)n, 1.0 / k);
    // (a fixed count, so that every build of an order takes the same h: the map contracts by (h / k) * sum_a 1 / (ext_a + h), about
    // 1 / (elements per axis + 1) -- at most 1/2, for two elements on an axis -- so 16 rounds leave less than 2^-16 of the first
    // guess's error, itself below one spacing: far inside the h/2 an index tolerates)
    for (int it = 0; it < 16; ++it) {
        double v = 1.0;
        for (int a = 0; a < 3; ++a) if (e[a] > 0.0) v *= e[a] + h;
        h = std::pow(v / (double)n, 1.0 / k);
    }
    if (!(h > 0.0) || !std::isfinite(h) || !std::isfinite(1.0 / h) || !(ext / h + 1.0 < 2097151.0)) return f;
    f.lattice = true;
    f.scale = 1.0 / h;
    for (int a = 0; a < 3; ++a) f.origin[a] = lo[a] - 0.5 * h;
    const uint64_t top = (uint64_t)((ext + 0.5 * h) * f.scale) + 1;      // (an index may round one up from the box's own)
    f.bits = 1;
    while (f.bits < 21 && (top >> f.bits)) ++f.bits;
    return f;
}

// Z-curve (Morton) order of n elements given by 3 coordinates each: position -> element id, ties in id order
// (lattice: tileLatticeKnob() of the caller's default)
std::vector<int32_t> mortonOrderOf(int32_t n, const double* xyz, bool lattice = tileLatticeKnob());

// ---- shared topology blocks ----------------------------------------------------------------------------------------------------
// The ELL tables of a tile are written in tile-local indices over ascending-id lists: two tiles that are the same brick of a
// structured region hold the same bytes.  rep[t] = the first tile whose block (the rows at the given bases, `len(t)` entries of
// every array, the widths / counts in `key(t)` part of the identity) equals tile t's entry for entry -- found by hash, verified by
// full comparison.  The kernels address the tables through the bases of their per-tile meta records only, so pointing a
// duplicate's base at rep[t]'s rows leaves what they read unchanged and lets the workgroups of a Morton range re-read one block
// from their L2.  The builders' own arrays (bases ascending, tiles packed in order) stay as they are: the remap goes into the
// meta records.  Lists of global ids (tpIds, tfIds, cellOrder, ...) are never shared.  SMGPU_TILE_SHARE=0: rep[t] = t.
struct TileShare {
    std::vector<int32_t> rep;
    int32_t distinct = 0;
    int32_t remap(const std::vector<int32_t>& base, int32_t t) const { return base[(size_t)rep[(size_t)t]]; }
    // the base tile t reads under an optional share (metaRecords)
    static int32_t baseOf(const TileShare* s, const std::vector<int32_t>& base, int32_t t) { return s && !s->rep.empty() ? s->remap(base, t) : base[(size_t)t]; }
};
inline bool tileShareKnob() { const char* e = std::getenv("SMGPU_TILE_SHARE"); return !e || std::atoi(e) != 0; }
struct GeomTiles; struct SmoothTiles; struct EdgeTiles;
// (the table arrays of a host build; a device build's rows: shareBlocksOnDevice below)
void shareGeomBlocks(const GeomTiles& gt, const uint16_t* faceVerts, const uint16_t* cellFaces, TileShare& fv, TileShare& cf);
void shareSmoothBlocks(const SmoothTiles& st, const uint16_t* pcEll, const uint16_t* ppEll, const uint16_t* pairEll, const uint16_t* pfEll,
                       TileShare& pc, TileShare& pp, TileShare& pf);
void shareEdgeBlocks(const EdgeTiles& et, const uint16_t* efEll, const uint16_t* ecEll, TileShare& ef, TileShare& ec);
// the pass for one array of a device build, run where the rows are (tiles_dev.hip): a = the rows, b = a second array under the same
// bases or NULL; base / len / key per tile.  The same representatives as the host pass.  0 done; 2 a HIP error (why)
int shareBlocksOnDevice(int32_t nTiles, const uint16_t* a, const uint16_t* b, const std::vector<int32_t>& base, const std::vector<int32_t>& len, const std::vector<int32_t>& key,
                        int device, TileShare& out, std::string& why);

// ---- geometry: tile = consecutive cells; LDS holds the tile's points and faces --------------------
struct GeomTiles {
    int32_t nTiles = 0, threads = 0;
    bool latticeKeys = tileLatticeKnob();   // the keys of an order built here (mortonFrame): on unless the knob says otherwise; the engine
                                            // sets its per-mesh default (tileLatticeDefault)
    std::vector<int32_t> cellBeg;   // nTiles+1
    std::vector<int32_t> tpOff;     // nTiles+1 -> tpIds
    std::vector<int32_t> tpIds;     // unique point ids per tile, ascending
    std::vector<int32_t> tfOff;     // nTiles+1 -> tile faces
    std::vector<int32_t> tfIds;     // global face id per tile face (ascending); bit 31 = this tile holds the owner cell
    // face vertices: per tile face, `fw` (= multiple of 4, tile-uniform) LDS-local point indices, padded
    std::vector<int32_t> fvBase;    // nTiles -> offset into faceVerts (units of uint16)
    std::vector<uint8_t> fvWidth;   // nTiles: fw
    std::vector<uint16_t> faceVerts;
    // cell faces: sliced ELL, per tile width cw (multiple of 4); entry (j, t) at cfBase + ((j/4)*threads + t)*4 + j%4
    // value = LDS-local face index | 0x8000 when the cell is the face's neighbour
    std::vector<int32_t> cfBase;    // nTiles
    std::vector<uint8_t> cfWidth;   // nTiles
    std::vector<uint16_t> cellFaces;
    std::vector<uint8_t> tileFlags; // nTiles: bit0 every face of the tile is a quadrilateral, bit1 every cell has 6 faces
                                    // (wave-uniform selection of the unrolled kernel paths)
    int32_t maxPoints = 0, maxFaces = 0;
    // tile order: position -> cell id.  Natural order, or a Morton (Z-curve) order of the cell centres so
    // that a run of consecutive positions is a compact 3-D brick (fewer faces / points shared with other
    // tiles => less duplicated face work, smaller LDS footprint).  Results do not depend on it.
    std::vector<int32_t> order;
    // capWeighted: 3 x points + faceWeight x faces a tile may stage (its LDS footprint in doubles)
    std::string build(const Topology& t, const double* points, bool morton, int32_t threads, int32_t capCells,
                      int32_t capPoints, int32_t capFaces, int32_t capWeighted = 0x7fffffff, int32_t faceWeight = 7);
    // the two halves of build(): tile order + greedy boundaries (host), and the per-tile tables -- which tiles_dev.hip builds on
    // the device from the boundaries where it can (buildGeomTablesOnDevice)
    // cellOrder (optional): the cells' Morton order computed elsewhere (tiles_dev.hip: cellMortonOrderOnDevice, the same order)
    std::string buildBoundaries(const Topology& t, const double* points, bool morton, int32_t threads, int32_t capCells,
                                int32_t capPoints, int32_t capFaces, int32_t capWeighted = 0x7fffffff, int32_t faceWeight = 7,
                                const std::vector<int32_t>* cellOrder = nullptr);
    std::string buildTables(const Topology& t);
    // the tiles' GeomTileMeta records (tile_meta.hpp), kGeomMetaInts ints per tile; a share (the blocks of faceVerts / cellFaces) points
    // a tile's base at the rows of its representative, none or an identity share leaves the tile's own
    std::vector<int> metaRecords(const TileShare* fvShare = nullptr, const TileShare* cfShare = nullptr) const;
};
// the tables of a device build (tiles_dev.hip) that the kernels read where they were built; the caller owns the arrays
struct GeomTilesDev {
    DevArr cellOrder, cellBeg, tpIds, tfIds, faceVerts, cellFaces, meta;
    bool valid = false;
    template <class F> void each(F&& f) { for (DevArr* a : {&cellOrder, &cellBeg, &tpIds, &tfIds, &faceVerts, &cellFaces, &meta}) f(*a); }
};
struct DeviceTopologyArrays;
// 0: built (gt holds the offsets / widths / flags / tfIds / maxima the host reads, `out` the device arrays); 1: not handled there
// (the caller runs gt.buildTables); 2: a HIP error (why)
int cellMortonOrderOnDevice(const DeviceTopologyArrays& td, int32_t nCells, int32_t nPoints, const double* points, int device, std::vector<int32_t>& order, std::string& why,
                            bool lattice = tileLatticeKnob());
int buildGeomTablesOnDevice(GeomTiles& gt, const DeviceTopologyArrays& td, int32_t nCells, int device, GeomTilesDev& out, std::string& why);

// ---- smoothing: tile = consecutive points; LDS holds the cell centres and neighbour points -------
struct SmoothTiles {
    int32_t nTiles = 0, threads = 0;
    bool latticeKeys = tileLatticeKnob();   // (as GeomTiles')
    std::vector<int32_t> ptBeg;     // nTiles+1
    std::vector<int32_t> tcOff;     // nTiles+1 -> tcIds
    std::vector<int32_t> tcIds;     // unique cell ids per tile, ascending
    std::vector<int32_t> tnOff;     // nTiles+1 -> tnIds
    std::vector<int32_t> tnIds;     // unique point ids (the tile's points and their neighbours), ascending
    std::vector<uint16_t> selfLoc;  // per tile position: the point's own LDS-local point index
    // sliced ELL (layout as GeomTiles::cellFaces)
    std::vector<int32_t> pcBase;    // nTiles
    std::vector<uint8_t> pcWidth;
    std::vector<uint16_t> pcEll;    // LDS-local cell index per pointCells entry
    std::vector<int32_t> ppBase;    // nTiles (shared by ppEll and pairEll)
    std::vector<uint8_t> ppWidth;
    std::vector<uint16_t> ppEll;    // LDS-local point index per pointPoints entry (bit 15 is set later for internal neighbours)
    // pairEll entry (p, i): bit j set <=> neighbours i and j of p share a cell (pointNeighPoints
    // membership, SM.C:383); valid while valence <= 16, else the kernel intersects pointCells lists
    std::vector<uint16_t> pairEll;
    // pfEll: per (point, face) the LDS-local indices of the previous and the next vertex of the point in the
    // face (getNeighbourPoints SM.C:793-831), two entries per face, width pfWidth (multiple of 4)
    std::vector<int32_t> pfBase;
    std::vector<uint8_t> pfWidth;
    std::vector<uint16_t> pfEll;
    int32_t maxCells = 0, maxPoints = 0;
    std::vector<int32_t> order;     // tile order: position -> point id (see GeomTiles::order)
    // isInternal (SM.C:40-91) marks bit 15 of the ppEll entries whose neighbour is an internal point (SM.C:294)
    // pointOrder (optional): mortonOrderOf(nPoints, points), computed by the caller (it also serves the edge tiles)
    // subset (optional): tiles over THESE points only, in the given order (multi-rank: the shared points get tiles of their own,
    // smgpu_halo_configure) -- `order`, `selfLoc` and the ELL rows then have subset->size() positions
    // capTotal: cells + points a tile may stage together (what its LDS footprint is made of; the kernels' occupancy is set by it)
    std::string build(const Topology& t, const double* points, const uint8_t* isInternal, bool morton, int32_t threads,
                      int32_t capCells, int32_t capPoints, const std::vector<int32_t>* pointOrder = nullptr,
                      const std::vector<int32_t>* subset = nullptr, int32_t capTotal = 0x7fffffff);
    // the two halves of build(), as GeomTiles'
    std::string buildBoundaries(const Topology& t, const double* points, bool morton, int32_t threads, int32_t capCells, int32_t capPoints,
                                const std::vector<int32_t>* pointOrder = nullptr, const std::vector<int32_t>* subset = nullptr, int32_t capTotal = 0x7fffffff);
    std::string buildTables(const Topology& t, const uint8_t* isInternal, bool subset = false);
    // SmoothTileMeta records, as GeomTiles::metaRecords (shares of pcEll, ppEll + pairEll, pfEll)
    std::vector<int> metaRecords(const TileShare* pcShare = nullptr, const TileShare* ppShare = nullptr, const TileShare* pfShare = nullptr) const;
};
struct SmoothTilesDev {
    DevArr order, ptBeg, tcIds, tnIds, selfLoc, pcEll, ppEll, pairEll, pfEll, meta;
    bool valid = false;
    template <class F> void each(F&& f) { for (DevArr* a : {&order, &ptBeg, &tcIds, &tnIds, &selfLoc, &pcEll, &ppEll, &pairEll, &pfEll, &meta}) f(*a); }
};
// the corner chains of all points computed ahead of the tables (tiles_dev.hip: startCornerChains)
struct CornerChains { int* chPrev = nullptr; int* chNext = nullptr; int* bad = nullptr; int* big = nullptr; void* stream = nullptr; int32_t nPoints = 0; bool started = false; };
int startCornerChains(const DeviceTopologyArrays& td, int32_t nPoints, int device, CornerChains& c, std::string& why);
void releaseCornerChains(CornerChains& c);
// (maxPointPoints: Topology's; the neighbour-pair masks exist while it is <= 16; chains: taken over and freed, or NULL)
int buildSmoothTablesOnDevice(SmoothTiles& st, const DeviceTopologyArrays& td, int32_t nPoints, int32_t maxPointPoints, const uint8_t* isInternal, int device,
                              SmoothTilesDev& out, std::string& why, CornerChains* chains = nullptr);

// ---- face-angle filter: tile = edges (Morton order of the edge midpoints); LDS holds the points, the
// face vertex averages and the cell centres the tile's edges need ------------------------------------------
struct EdgeTiles {
    int32_t nTiles = 0, threads = 0;
    bool latticeKeys = tileLatticeKnob();   // (as GeomTiles')
    std::vector<int32_t> order;     // position -> edge id
    std::vector<int32_t> edgeBeg;   // nTiles+1
    std::vector<int32_t> tpOff, tpIds, tfOff, tfIds, tcOff, tcIds;   // unique points / faces / cells per tile
    std::vector<uint16_t> epLoc;    // 2 per tile position: LDS-local ids of the edge's end points
    std::vector<int32_t> efBase, ecBase;        // nTiles
    std::vector<uint8_t> efWidth, ecWidth;      // multiples of 4
    std::vector<uint16_t> efEll, ecEll;         // ring faces / ring cells (Topology::ringFace/ringCell), sliced ELL;
                                                // an edge without a ring (non-manifold) has an all-pad face row
    int32_t maxPoints = 0, maxFaces = 0, maxCells = 0;
    // pointOrder (optional, with morton): the edges follow the Z-curve of their START points (edges are stored grouped by start
    // point) instead of a sort of their own over the 3x as many edge midpoints -- a tile is still a compact cluster of edges
    std::string build(const Topology& t, const double* points, bool morton, int32_t threads, int32_t capPoints,
                      int32_t capFaces, int32_t capCells, const std::vector<int32_t>* pointOrder = nullptr, int32_t capTotal = 0x7fffffff);
    // the two halves of build(), as GeomTiles'
    std::string buildBoundaries(const Topology& t, const double* points, bool morton, int32_t threads, int32_t capPoints,
                                int32_t capFaces, int32_t capCells, const std::vector<int32_t>* pointOrder = nullptr, int32_t capTotal = 0x7fffffff);
    std::string buildTables(const Topology& t);
    // EdgeTileMeta records, as GeomTiles::metaRecords (shares of efEll, ecEll)
    std::vector<int> metaRecords(const TileShare* efShare = nullptr, const TileShare* ecShare = nullptr) const;
};
struct EdgeTilesDev {
    DevArr order, edgeBeg, tpIds, tfIds, tcIds, epLoc, efEll, ecEll, meta;
    long long nTf = 0;
    bool valid = false;
    template <class F> void each(F&& f) { for (DevArr* a : {&order, &edgeBeg, &tpIds, &tfIds, &tcIds, &epLoc, &efEll, &ecEll, &meta}) f(*a); }
};
// ---- the knobs of the three tile sets, read once per engine (smgpu_create: makeTilePlan, setup_tiles.hpp) ---------------------------
struct TilePlan {
    bool wantTiles = true, wantFilter = true;      // SMGPU_TILES, SMGPU_FILTER
    bool morton = true, latticeKeys = true;        // SMGPU_TILE_MORTON; tileLatticeKnob of the mesh's default
    int deviceTiles = 1;                           // SMGPU_DEVICE_TILES: 0 the tables on the host, 1 on the device where the addressing was built
                                                   // there, 2 as if the device builds handed their tables back (the tests' way into that path)
    bool share = true;                             // tileShareKnob
    int verbose = 0;                               // SMGPU_VERBOSE
    int geomT = 256, smoothT = 256, geomCells = 128;
    int capGeomPoints = 0, capGeomFaces = 0, capGeomWeighted = 0;
    int capSmoothCells = 0, capSmoothNbrs = 0, capSmoothTotal = 0;
    int capEdgePoints = 0, capEdgeFaces = 0, capEdgeCells = 0, capEdgeTotal = 0;
    static bool shapeOk(int T) { return T == 64 || T == 128 || T == 256; }
    bool shapesOk() const { return shapeOk(geomT) && shapeOk(smoothT); }      // (else smgpu_create refuses, once it comes to the tiles)
};

int buildEdgeTablesOnDevice(EdgeTiles& et, const DeviceTopologyArrays& td, int32_t nEdges, int device, EdgeTilesDev& out, std::string& why);
int remapEdgeFaceIdsOnDevice(const int* geomTfIds, long long nGeomTf, int32_t nFaces, int* edgeTfIds, long long nEdgeTf, int device, std::string& why);

}  // namespace smgpu
