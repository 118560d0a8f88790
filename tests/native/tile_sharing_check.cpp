// tile_sharing_check.cpp -- the lattice Z-curve keys and the shared topology blocks of the LDS tile tables (csrc/tiles.cpp), on the CPU.
//   g++ -O2 -std=c++17 -pthread -I smoothmesh_amd/csrc tests/native/tile_sharing_check.cpp smoothmesh_amd/csrc/topology.cpp smoothmesh_amd/csrc/tiles.cpp
//   tile_sharing_check mesh.bin [T=256]            (mesh.bin: the dump tests/test_tile_tables.py writes)
// For SMGPU_TILE_LATTICE = 1, 0: builds the three tile sets with the caps smgpu.hip derives from T, runs the share pass with
// SMGPU_TILE_SHARE = 0 and 1, expands every tile's rows through the remapped bases and compares them with the tile's own rows
// entry for entry, and holds every tile of several elements to capWeighted / capTotal.  Prints one line per knob combination:
//   "set lattice=L share=S geom tiles=.. fv=.. cf=.. faces_x=.. points_x=.. maxP=.. maxF=.. smooth tiles=.. pc=.. pp=.. pf=.. cells_x=.. nbrs_x=.. edge tiles=.. ef=.. ec=.."
// (fv, cf, ...: distinct blocks; *_x: staged elements per element of the mesh), "FAIL <what>" lines, and "done fails=<n>".
// Under every combination the per-tile meta records (metaRecords, tile_meta.hpp) are held to the tables field by field: counts are
// offset differences, bases are share.remap(base, t), and no share or an identity share gives the tile's own bases.
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "tiles.hpp"
#include "topology.hpp"

using namespace smgpu;

namespace {
int gFails = 0;
void failLine(const std::string& what, int lattice, int share, int tile) {
    if (gFails++ < 20) std::printf("FAIL %s (lattice=%d share=%d tile %d)\n", what.c_str(), lattice, share, tile);
}

struct Mesh {
    int32_t nP = 0, nC = 0, nF = 0, nIF = 0;
    std::vector<double> pts;
    std::vector<int32_t> fo, fp, own, nei;
    std::vector<uint8_t> internal;
};
bool readMesh(const char* path, Mesh& m) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    int32_t hdr[4];
    bool ok = std::fread(hdr, 4, 4, f) == 4;
    m.nP = hdr[0]; m.nC = hdr[1]; m.nF = hdr[2]; m.nIF = hdr[3];
    m.pts.resize(3 * (size_t)m.nP); m.fo.resize((size_t)m.nF + 1); m.own.resize((size_t)m.nF); m.nei.resize((size_t)m.nIF); m.internal.resize((size_t)m.nP);
    ok = ok && std::fread(m.pts.data(), 8, m.pts.size(), f) == m.pts.size();
    ok = ok && std::fread(m.fo.data(), 4, m.fo.size(), f) == m.fo.size();
    if (ok) m.fp.resize((size_t)m.fo[(size_t)m.nF]);
    ok = ok && std::fread(m.fp.data(), 4, m.fp.size(), f) == m.fp.size();
    ok = ok && std::fread(m.own.data(), 4, m.own.size(), f) == m.own.size();
    ok = ok && std::fread(m.nei.data(), 4, m.nei.size(), f) == m.nei.size();
    ok = ok && std::fread(m.internal.data(), 1, m.internal.size(), f) == m.internal.size();
    std::fclose(f);
    return ok;
}

// the rows a tile reads through `base` against the rows it owns
bool sameRows(const std::vector<uint16_t>& v, int32_t own, int32_t via, size_t n) {
    return via >= 0 && (size_t)via + n <= v.size() && std::equal(v.begin() + own, v.begin() + own + (std::ptrdiff_t)n, v.begin() + via);
}
// a representative is an earlier tile (or the tile itself) that represents itself; distinct = the tiles that do
void checkShare(const char* who, const TileShare& s, int32_t nTiles, int lattice, int share) {
    int32_t own = 0;
    if ((int32_t)s.rep.size() != nTiles) { failLine(std::string(who) + ": rep size", lattice, share, -1); return; }
    for (int32_t t = 0; t < nTiles; ++t) {
        const int32_t r = s.rep[(size_t)t];
        if (r < 0 || r > t || s.rep[(size_t)r] != r) failLine(std::string(who) + ": representative is not an earlier tile that stands for itself", lattice, share, t);
        if (!share && r != t) failLine(std::string(who) + ": SMGPU_TILE_SHARE=0 still shares", lattice, share, t);
        own += r == t;
    }
    if (own != s.distinct) failLine(std::string(who) + ": distinct count", lattice, share, -1);
}
// record t of a metaRecords() result as its struct
template <class Meta> Meta recordOf(const std::vector<int>& meta, int32_t t) {
    Meta r;
    std::memcpy(&r, meta.data() + sizeof(Meta) / sizeof(int) * (size_t)t, sizeof(Meta));
    return r;
}
TileShare identityShare(int32_t nTiles) {
    TileShare s;
    s.rep.resize((size_t)nTiles);
    for (int32_t t = 0; t < nTiles; ++t) s.rep[(size_t)t] = t;
    s.distinct = nTiles;
    return s;
}
void checkGeomMeta(const GeomTiles& gt, const TileShare& fv, const TileShare& cf, int lattice, int share) {
    const std::vector<int> meta = gt.metaRecords(&fv, &cf), plain = gt.metaRecords();
    const TileShare id = identityShare(gt.nTiles);
    if (meta.size() != (size_t)kGeomMetaInts * (size_t)gt.nTiles || plain.size() != meta.size()) { failLine("geom meta: size", lattice, share, -1); return; }
    if (gt.metaRecords(&id, &id) != plain || gt.metaRecords(&id, nullptr) != plain) failLine("geom meta: identity share differs from no share", lattice, share, -1);
    if (!share && meta != plain) failLine("geom meta: SMGPU_TILE_SHARE=0 differs from no share", lattice, share, -1);
    for (int32_t t = 0; t < gt.nTiles; ++t) {
        const GeomTileMeta r = recordOf<GeomTileMeta>(meta, t), q = recordOf<GeomTileMeta>(plain, t);
        const size_t i = (size_t)t;
        if (r.tpOff != gt.tpOff[i] || r.nPts != gt.tpOff[i + 1] - gt.tpOff[i] || r.tfOff != gt.tfOff[i] || r.nFaces != gt.tfOff[i + 1] - gt.tfOff[i] ||
            r.cellBeg != gt.cellBeg[i] || r.nCells != gt.cellBeg[i + 1] - gt.cellBeg[i] || r.fvWidth != gt.fvWidth[i] || r.cfWidth != gt.cfWidth[i] ||
            r.flags != gt.tileFlags[i] || r.pad != 0) failLine("geom meta: counts / widths / flags", lattice, share, t);
        if (r.fvBase != fv.remap(gt.fvBase, t) || r.cfBase != cf.remap(gt.cfBase, t)) failLine("geom meta: remapped bases", lattice, share, t);
        if (q.fvBase != gt.fvBase[i] || q.cfBase != gt.cfBase[i]) failLine("geom meta: plain bases", lattice, share, t);
    }
}
void checkSmoothMeta(const SmoothTiles& st, const TileShare& pc, const TileShare& pp, const TileShare& pf, int lattice, int share) {
    const std::vector<int> meta = st.metaRecords(&pc, &pp, &pf), plain = st.metaRecords();
    const TileShare id = identityShare(st.nTiles);
    if (meta.size() != (size_t)kSmoothMetaInts * (size_t)st.nTiles || plain.size() != meta.size()) { failLine("smooth meta: size", lattice, share, -1); return; }
    if (st.metaRecords(&id, &id, &id) != plain || st.metaRecords(nullptr, &id, nullptr) != plain) failLine("smooth meta: identity share differs from no share", lattice, share, -1);
    if (!share && meta != plain) failLine("smooth meta: SMGPU_TILE_SHARE=0 differs from no share", lattice, share, -1);
    for (int32_t t = 0; t < st.nTiles; ++t) {
        const SmoothTileMeta r = recordOf<SmoothTileMeta>(meta, t), q = recordOf<SmoothTileMeta>(plain, t);
        const size_t i = (size_t)t;
        if (r.ptBeg != st.ptBeg[i] || r.nPts != st.ptBeg[i + 1] - st.ptBeg[i] || r.tcOff != st.tcOff[i] || r.nCells != st.tcOff[i + 1] - st.tcOff[i] ||
            r.tnOff != st.tnOff[i] || r.nNbrs != st.tnOff[i + 1] - st.tnOff[i] || r.pcWidth != st.pcWidth[i] || r.ppWidth != st.ppWidth[i] || r.pfWidth != st.pfWidth[i])
            failLine("smooth meta: counts / widths", lattice, share, t);
        if (r.pcBase != pc.remap(st.pcBase, t) || r.ppBase != pp.remap(st.ppBase, t) || r.pfBase != pf.remap(st.pfBase, t)) failLine("smooth meta: remapped bases", lattice, share, t);
        if (q.pcBase != st.pcBase[i] || q.ppBase != st.ppBase[i] || q.pfBase != st.pfBase[i]) failLine("smooth meta: plain bases", lattice, share, t);
    }
}
void checkEdgeMeta(const EdgeTiles& et, const TileShare& ef, const TileShare& ec, int lattice, int share) {
    const std::vector<int> meta = et.metaRecords(&ef, &ec), plain = et.metaRecords();
    const TileShare id = identityShare(et.nTiles);
    if (meta.size() != (size_t)kEdgeMetaInts * (size_t)et.nTiles || plain.size() != meta.size()) { failLine("edge meta: size", lattice, share, -1); return; }
    if (et.metaRecords(&id, &id) != plain || et.metaRecords(nullptr, &id) != plain) failLine("edge meta: identity share differs from no share", lattice, share, -1);
    if (!share && meta != plain) failLine("edge meta: SMGPU_TILE_SHARE=0 differs from no share", lattice, share, -1);
    for (int32_t t = 0; t < et.nTiles; ++t) {
        const EdgeTileMeta r = recordOf<EdgeTileMeta>(meta, t), q = recordOf<EdgeTileMeta>(plain, t);
        const size_t i = (size_t)t;
        if (r.edgeBeg != et.edgeBeg[i] || r.nEdges != et.edgeBeg[i + 1] - et.edgeBeg[i] || r.tpOff != et.tpOff[i] || r.nPts != et.tpOff[i + 1] - et.tpOff[i] ||
            r.tfOff != et.tfOff[i] || r.nFaces != et.tfOff[i + 1] - et.tfOff[i] || r.tcOff != et.tcOff[i] || r.nCells != et.tcOff[i + 1] - et.tcOff[i] ||
            r.efWidth != et.efWidth[i] || r.ecWidth != et.ecWidth[i]) failLine("edge meta: counts / widths", lattice, share, t);
        if (r.efBase != ef.remap(et.efBase, t) || r.ecBase != ec.remap(et.ecBase, t)) failLine("edge meta: remapped bases", lattice, share, t);
        if (q.efBase != et.efBase[i] || q.ecBase != et.ecBase[i]) failLine("edge meta: plain bases", lattice, share, t);
    }
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s mesh.bin [T=256]\n", argv[0]); return 2; }
    Mesh m;
    if (!readMesh(argv[1], m)) { std::printf("error reading %s\n", argv[1]); return 2; }
    int32_t T = 256;
    for (int i = 2; i < argc; ++i) if (!std::strncmp(argv[i], "T=", 2)) T = std::atoi(argv[i] + 2);
    // the defaults smgpu.hip derives from the thread count (as tests/native/tile_tables_check.cpp)
    const int32_t gc = T / 2, gp = std::min(6 * gc, 1400), gf = std::min(4 * gc, 1400), gw = T == 256 ? 3980 : INT_MAX, fw = 6;
    const int32_t sc = std::min(2 * T, 1500), sn = std::min(3 * T, 1500), stot = T == 256 ? 1112 : INT_MAX;
    const int32_t ep = 512, ef = 768, ec = 512, etot = 852;
    Topology topo;
    const std::string te = topo.build(m.nP, m.nC, m.nF, m.nIF, m.fo.data(), m.fp.data(), m.own.data(), m.nei.data());
    if (!te.empty()) { std::printf("error topology: %s\n", te.c_str()); return 1; }
    for (int lattice = 1; lattice >= 0; --lattice) {
        ::setenv("SMGPU_TILE_LATTICE", lattice ? "1" : "0", 1);
        const std::vector<int32_t> pointOrder = mortonOrderOf(m.nP, m.pts.data());
        GeomTiles gt; SmoothTiles st; EdgeTiles et;
        const std::string eg = gt.build(topo, m.pts.data(), true, T, gc, gp, gf, gw, fw);
        const std::string es = st.build(topo, m.pts.data(), m.internal.data(), true, T, sc, sn, &pointOrder, nullptr, stot);
        const std::string ee = et.build(topo, m.pts.data(), true, T, ep, ef, ec, &pointOrder, etot);
        if (!eg.empty() || !es.empty() || !ee.empty()) { std::printf("error build: %s %s %s\n", eg.c_str(), es.c_str(), ee.c_str()); return 1; }
        // the soft caps: a tile of several elements stays under them
        for (int32_t t = 0; t < gt.nTiles; ++t) {
            const long long np = gt.tpOff[(size_t)t + 1] - gt.tpOff[(size_t)t], nf = gt.tfOff[(size_t)t + 1] - gt.tfOff[(size_t)t];
            if (gt.cellBeg[(size_t)t + 1] - gt.cellBeg[(size_t)t] > 1 && 3 * np + fw * nf > gw) failLine("geom: capWeighted", lattice, -1, t);
            if (np > gp || nf > gf) failLine("geom: capPoints / capFaces", lattice, -1, t);
        }
        for (int32_t t = 0; t < st.nTiles; ++t) {
            const long long nc = st.tcOff[(size_t)t + 1] - st.tcOff[(size_t)t], nn = st.tnOff[(size_t)t + 1] - st.tnOff[(size_t)t];
            if (st.ptBeg[(size_t)t + 1] - st.ptBeg[(size_t)t] > 1 && nc + nn > stot) failLine("smooth: capTotal", lattice, -1, t);
            if (nc > sc || nn > sn) failLine("smooth: capCells / capPoints", lattice, -1, t);
        }
        for (int32_t t = 0; t < et.nTiles; ++t) {
            const long long np = et.tpOff[(size_t)t + 1] - et.tpOff[(size_t)t], nf = et.tfOff[(size_t)t + 1] - et.tfOff[(size_t)t], nc = et.tcOff[(size_t)t + 1] - et.tcOff[(size_t)t];
            if (et.edgeBeg[(size_t)t + 1] - et.edgeBeg[(size_t)t] > 1 && np + nf + nc > etot) failLine("edge: capTotal", lattice, -1, t);
        }
        for (int share = 0; share <= 1; ++share) {
            ::setenv("SMGPU_TILE_SHARE", share ? "1" : "0", 1);
            TileShare fv, cf, pc, pp, pf, sef, sec;
            shareGeomBlocks(gt, gt.faceVerts.data(), gt.cellFaces.data(), fv, cf);
            shareSmoothBlocks(st, st.pcEll.data(), st.ppEll.data(), st.pairEll.data(), st.pfEll.data(), pc, pp, pf);
            shareEdgeBlocks(et, et.efEll.data(), et.ecEll.data(), sef, sec);
            checkShare("geom faceVerts", fv, gt.nTiles, lattice, share); checkShare("geom cellFaces", cf, gt.nTiles, lattice, share);
            checkShare("smooth pcEll", pc, st.nTiles, lattice, share); checkShare("smooth ppEll", pp, st.nTiles, lattice, share); checkShare("smooth pfEll", pf, st.nTiles, lattice, share);
            checkShare("edge efEll", sef, et.nTiles, lattice, share); checkShare("edge ecEll", sec, et.nTiles, lattice, share);
            if (gFails) break;
            // expanded through the remapped bases, every tile reads what its own rows hold (the unshared build), entry for entry; widths
            // and counts are the tile's own in both
            for (int32_t t = 0; t < gt.nTiles; ++t) {
                const size_t nf = (size_t)(gt.tfOff[(size_t)t + 1] - gt.tfOff[(size_t)t]);
                const int32_t r1 = fv.rep[(size_t)t], r2 = cf.rep[(size_t)t];
                if (gt.fvWidth[(size_t)r1] != gt.fvWidth[(size_t)t] || !sameRows(gt.faceVerts, gt.fvBase[(size_t)t], fv.remap(gt.fvBase, t), nf * gt.fvWidth[(size_t)t]))
                    failLine("geom: faceVerts through the shared base", lattice, share, t);
                if (gt.cfWidth[(size_t)r2] != gt.cfWidth[(size_t)t] || !sameRows(gt.cellFaces, gt.cfBase[(size_t)t], cf.remap(gt.cfBase, t), (size_t)gt.cfWidth[(size_t)t] * T))
                    failLine("geom: cellFaces through the shared base", lattice, share, t);
            }
            for (int32_t t = 0; t < st.nTiles; ++t) {
                if (!sameRows(st.pcEll, st.pcBase[(size_t)t], pc.remap(st.pcBase, t), (size_t)st.pcWidth[(size_t)t] * T)) failLine("smooth: pcEll through the shared base", lattice, share, t);
                if (!sameRows(st.ppEll, st.ppBase[(size_t)t], pp.remap(st.ppBase, t), (size_t)st.ppWidth[(size_t)t] * T)) failLine("smooth: ppEll through the shared base", lattice, share, t);
                if (!sameRows(st.pairEll, st.ppBase[(size_t)t], pp.remap(st.ppBase, t), (size_t)st.ppWidth[(size_t)t] * T)) failLine("smooth: pairEll through the shared base", lattice, share, t);
                if (!sameRows(st.pfEll, st.pfBase[(size_t)t], pf.remap(st.pfBase, t), (size_t)st.pfWidth[(size_t)t] * T)) failLine("smooth: pfEll through the shared base", lattice, share, t);
            }
            for (int32_t t = 0; t < et.nTiles; ++t) {
                if (!sameRows(et.efEll, et.efBase[(size_t)t], sef.remap(et.efBase, t), (size_t)et.efWidth[(size_t)t] * T)) failLine("edge: efEll through the shared base", lattice, share, t);
                if (!sameRows(et.ecEll, et.ecBase[(size_t)t], sec.remap(et.ecBase, t), (size_t)et.ecWidth[(size_t)t] * T)) failLine("edge: ecEll through the shared base", lattice, share, t);
            }
            checkGeomMeta(gt, fv, cf, lattice, share);
            checkSmoothMeta(st, pc, pp, pf, lattice, share);
            checkEdgeMeta(et, sef, sec, lattice, share);
            std::printf("set lattice=%d share=%d geom tiles=%d fv=%d cf=%d faces_x=%.4f points_x=%.4f maxP=%d maxF=%d smooth tiles=%d pc=%d pp=%d pf=%d cells_x=%.4f nbrs_x=%.4f "
                        "edge tiles=%d ef=%d ec=%d\n", lattice, share, gt.nTiles, fv.distinct, cf.distinct, (double)gt.tfOff.back() / m.nF, (double)gt.tpOff.back() / m.nP,
                        gt.maxPoints, gt.maxFaces, st.nTiles, pc.distinct, pp.distinct, pf.distinct, (double)st.tcOff.back() / m.nP, (double)st.tnOff.back() / m.nP,
                        et.nTiles, sef.distinct, sec.distinct);
        }
    }
    std::printf("done fails=%d\n", gFails);
    return gFails ? 1 : 0;
}
