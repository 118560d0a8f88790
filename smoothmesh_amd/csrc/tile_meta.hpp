// tile_meta.hpp -- the per-tile records of the three tile sets: one tile's scalars in one record, which the kernels fetch with
// scalar loads (loadGeomMeta / loadSmoothMeta in kernels_tiled.hpp, loadTileMeta in kernels_filter.hpp).  A record is the struct's
// fields in order, one int each: the host writes the structs (tiles.cpp, metaRecords), the kernels read word i into field i.
// The base fields hold the rows a tile READS -- its own, or those of the first tile with the same rows (tiles.hpp, TileShare).
#pragma once

namespace smgpu {

struct GeomTileMeta { int tpOff, nPts, tfOff, nFaces, fvBase, fvWidth, cellBeg, nCells, cfBase, cfWidth, flags, pad; };
struct SmoothTileMeta { int ptBeg, nPts, tcOff, nCells, tnOff, nNbrs, pcBase, pcWidth, ppBase, ppWidth, pfBase, pfWidth; };
struct EdgeTileMeta { int edgeBeg, nEdges, tpOff, nPts, tfOff, nFaces, tcOff, nCells, efBase, efWidth, ecBase, ecWidth; };
constexpr int kGeomMetaInts = sizeof(GeomTileMeta) / sizeof(int);
constexpr int kSmoothMetaInts = sizeof(SmoothTileMeta) / sizeof(int);
constexpr int kEdgeMetaInts = sizeof(EdgeTileMeta) / sizeof(int);
static_assert(kGeomMetaInts == 12 && kSmoothMetaInts == 12 && kEdgeMetaInts == 12, "the kernels read records of 12 ints");

}  // namespace smgpu
