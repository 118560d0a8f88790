// tile_tables_check.cpp -- decodes the LDS tile tables (csrc/tiles.cpp) back into global ids and holds them to the mesh.
//   g++ -O2 -std=c++17 -pthread -I smoothmesh_amd/csrc tests/native/tile_tables_check.cpp smoothmesh_amd/csrc/topology.cpp smoothmesh_amd/csrc/tiles.cpp
//   tile_tables_check mesh.bin [key=value ...]      (mesh.bin: the dump scripts/native/setup_bench reads; tests/test_tile_tables.py)
// keys: T (threads of all three builders, default 256), morton (1), the caps gc gp gf gw fw / sc sn st / ep ef ec et (default: what
// smgpu.hip derives from T), subset=<seed> (also the shared-point form on a random subset of the points), segs=<n> (the segment count
// the builders cut a large mesh into: the cuts n*sg/segs are tile boundaries and the only boundaries a cap did not force).
// The adjacency the tables are held to is derived here from faces / owner / neighbour alone, not taken from Topology.
// Prints "need ..." (the largest single element's need per cap), "error <builder>: <message>" for a builder that refused, one
// "FAIL <invariant>: n=<count> first: <detail>" line per violated invariant, and "tiles geom=.. smooth=.. edge=.." at the end.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "tiles.hpp"
#include "topology.hpp"

using namespace smgpu;

namespace {

struct Report {
    std::map<std::string, std::pair<long long, std::string>> fails;   // invariant -> (count, first detail)
    void fail(const std::string& what, const std::string& detail) {
        auto& f = fails[what];
        if (f.first++ == 0) f.second = detail;
    }
};
Report R;
#define CHECK(cond, what, ...)                                        \
    do {                                                              \
        if (!(cond)) {                                                \
            char b_[256];                                             \
            std::snprintf(b_, sizeof b_, __VA_ARGS__);                \
            R.fail(what, b_);                                         \
        }                                                             \
    } while (0)

using Rows = std::vector<std::vector<int32_t>>;

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

void sortUnique(std::vector<int32_t>& v) { std::sort(v.begin(), v.end()); v.erase(std::unique(v.begin(), v.end()), v.end()); }

// the adjacency, straight from the mesh
struct Adj {
    Rows cellFaces;      // owned faces ascending, then neighboured faces ascending with bit 31
    Rows cellPoints;     // unique, ascending
    Rows pointCells, pointPoints, pointCorners;   // pointCorners: (prev, next) per face holding the point, flattened
    std::vector<int32_t> pointFaceCount;
    std::vector<std::pair<int32_t, int32_t>> edges;   // (min, max), ascending
    Rows edgeFaces, edgeCells;
};

void buildAdj(const Mesh& m, Adj& a) {
    a.cellFaces.assign((size_t)m.nC, {});
    for (int32_t f = 0; f < m.nF; ++f) a.cellFaces[(size_t)m.own[(size_t)f]].push_back(f);
    for (int32_t f = 0; f < m.nIF; ++f) a.cellFaces[(size_t)m.nei[(size_t)f]].push_back((int32_t)(0x80000000u | (uint32_t)f));
    a.cellPoints.assign((size_t)m.nC, {});
    a.pointCells.assign((size_t)m.nP, {});
    a.pointPoints.assign((size_t)m.nP, {});
    a.pointCorners.assign((size_t)m.nP, {});
    a.pointFaceCount.assign((size_t)m.nP, 0);
    for (int32_t f = 0; f < m.nF; ++f) {
        const int32_t b = m.fo[(size_t)f], n = m.fo[(size_t)f + 1] - b;
        for (int32_t j = 0; j < n; ++j) {
            const int32_t p = m.fp[(size_t)(b + j)], prev = m.fp[(size_t)(b + (j + n - 1) % n)], next = m.fp[(size_t)(b + (j + 1) % n)];
            a.cellPoints[(size_t)m.own[(size_t)f]].push_back(p);
            a.pointCells[(size_t)p].push_back(m.own[(size_t)f]);
            if (f < m.nIF) { a.cellPoints[(size_t)m.nei[(size_t)f]].push_back(p); a.pointCells[(size_t)p].push_back(m.nei[(size_t)f]); }
            a.pointPoints[(size_t)p].push_back(next);
            a.pointPoints[(size_t)p].push_back(prev);
            a.pointCorners[(size_t)p].push_back(prev);
            a.pointCorners[(size_t)p].push_back(next);
            ++a.pointFaceCount[(size_t)p];
            a.edges.push_back({std::min(p, next), std::max(p, next)});
        }
    }
    for (auto& r : a.cellPoints) sortUnique(r);
    for (auto& r : a.pointCells) sortUnique(r);
    for (auto& r : a.pointPoints) sortUnique(r);
    std::sort(a.edges.begin(), a.edges.end());
    a.edges.erase(std::unique(a.edges.begin(), a.edges.end()), a.edges.end());
    a.edgeFaces.assign(a.edges.size(), {});
    a.edgeCells.assign(a.edges.size(), {});
    for (int32_t f = 0; f < m.nF; ++f) {
        const int32_t b = m.fo[(size_t)f], n = m.fo[(size_t)f + 1] - b;
        for (int32_t j = 0; j < n; ++j) {
            const int32_t p = m.fp[(size_t)(b + j)], q = m.fp[(size_t)(b + (j + 1) % n)];
            const auto k = std::lower_bound(a.edges.begin(), a.edges.end(), std::make_pair(std::min(p, q), std::max(p, q))) - a.edges.begin();
            a.edgeFaces[(size_t)k].push_back(f);
            a.edgeCells[(size_t)k].push_back(m.own[(size_t)f]);
            if (f < m.nIF) a.edgeCells[(size_t)k].push_back(m.nei[(size_t)f]);
        }
    }
    for (auto& r : a.edgeFaces) sortUnique(r);
    for (auto& r : a.edgeCells) sortUnique(r);
}

bool isPermutation(const std::vector<int32_t>& v, int32_t n) {
    if ((int64_t)v.size() != n) return false;
    std::vector<uint8_t> seen((size_t)n, 0);
    for (int32_t x : v) { if (x < 0 || x >= n || seen[(size_t)x]) return false; seen[(size_t)x] = 1; }
    return true;
}
bool ascendingUnique(const int32_t* b, const int32_t* e, int32_t mask = 0x7fffffff) {
    for (const int32_t* p = b; p + 1 < e; ++p) if ((p[0] & mask) >= (p[1] & mask)) return false;
    return true;
}
bool intersects(const std::vector<int32_t>& x, const std::vector<int32_t>& y) {   // two ascending lists share an entry
    for (size_t i = 0, j = 0; i < x.size() && j < y.size();) {
        if (x[i] == y[j]) return true;
        if (x[i] < y[j]) ++i; else ++j;
    }
    return false;
}

// boundaries: beg[0] = 0, strictly increasing, beg.back() = n; every cut n*sg/segs among them; returns the set of cuts
std::set<int32_t> checkBoundaries(const char* who, const std::vector<int32_t>& beg, int32_t nTiles, int32_t n, int segs) {
    std::set<int32_t> cuts;
    const std::string w = who;
    CHECK((int32_t)beg.size() == nTiles + 1, w + " boundaries: count", "%zu entries for %d tiles", beg.size(), nTiles);
    if ((int32_t)beg.size() != nTiles + 1 || beg.empty()) return cuts;
    CHECK(beg.front() == 0 && beg.back() == n, w + " boundaries: cover", "first %d last %d of %d", beg.front(), beg.back(), n);
    for (int32_t i = 0; i < nTiles; ++i) CHECK(beg[(size_t)i] < beg[(size_t)i + 1], w + " boundaries: monotone", "tile %d: %d .. %d", i, beg[(size_t)i], beg[(size_t)i + 1]);
    for (int sg = 1; sg < segs; ++sg) {
        const int32_t c = (int32_t)((int64_t)n * sg / segs);
        cuts.insert(c);
        CHECK(std::binary_search(beg.begin(), beg.end(), c), w + " segments: a cut is not a tile boundary", "cut %d of %d at %d", sg, segs, c);
    }
    return cuts;
}

// a sliced-ELL row (j, t) of a tile at base
inline size_t ell(int32_t base, int32_t threads, int32_t j, int32_t t) { return (size_t)base + ((size_t)(j / 4) * threads + t) * 4 + (j % 4); }

// ---------------------------------------------------------------------------------------------------------------------------------
struct GeomCaps { int32_t cells, points, faces, weighted, faceWeight; };

void checkGeom(const Mesh& m, const Adj& a, const GeomTiles& g, int32_t T, const GeomCaps& cap, int segs) {
    CHECK(g.threads == T, "geom: threads", "%d", g.threads);
    CHECK(isPermutation(g.order, m.nC), "geom: order is a permutation of the cells", "%zu entries", g.order.size());
    if (!isPermutation(g.order, m.nC)) return;
    const auto cuts = checkBoundaries("geom", g.cellBeg, g.nTiles, m.nC, segs);
    const int32_t nt = g.nTiles;
    bool sizes = (int32_t)g.tpOff.size() == nt + 1 && (int32_t)g.tfOff.size() == nt + 1 && (int32_t)g.fvBase.size() == nt && (int32_t)g.fvWidth.size() == nt &&
                 (int32_t)g.cfBase.size() == nt && (int32_t)g.cfWidth.size() == nt && (int32_t)g.tileFlags.size() == nt && (int32_t)g.cellBeg.size() == nt + 1 &&
                 g.tpOff.back() == (int32_t)g.tpIds.size() && g.tfOff.back() == (int32_t)g.tfIds.size();
    CHECK(sizes, "geom: table sizes", "nTiles %d", nt);
    if (!sizes) return;
    std::vector<int32_t> cellTile((size_t)m.nC, -1);
    for (int32_t ti = 0; ti < nt; ++ti)
        for (int32_t ci = g.cellBeg[(size_t)ti]; ci < g.cellBeg[(size_t)ti + 1]; ++ci) cellTile[(size_t)g.order[(size_t)ci]] = ti;
    std::vector<int32_t> ownerMarks((size_t)m.nF, 0);
    int32_t maxP = 0, maxF = 0;
    size_t fvNext = 0, cfNext = 0;
    std::vector<int32_t> pts, fcs;
    for (int32_t ti = 0; ti < nt; ++ti) {
        const int32_t cb = g.cellBeg[(size_t)ti], ce = g.cellBeg[(size_t)ti + 1], nc = ce - cb;
        pts.clear(); fcs.clear();
        int32_t longestCell = 0, longestFace = 0;
        bool allHex = true, allQuads = true;
        for (int32_t ci = cb; ci < ce; ++ci) {
            const int32_t c = g.order[(size_t)ci];
            longestCell = std::max(longestCell, (int32_t)a.cellFaces[(size_t)c].size());
            allHex = allHex && a.cellFaces[(size_t)c].size() == 6;
            for (int32_t v : a.cellFaces[(size_t)c]) fcs.push_back(v & 0x7fffffff);
            pts.insert(pts.end(), a.cellPoints[(size_t)c].begin(), a.cellPoints[(size_t)c].end());
        }
        sortUnique(pts); sortUnique(fcs);
        for (int32_t f : fcs) {
            const int32_t n = m.fo[(size_t)f + 1] - m.fo[(size_t)f];
            longestFace = std::max(longestFace, n);
            allQuads = allQuads && n == 4;
        }
        const int32_t* tp = g.tpIds.data() + g.tpOff[(size_t)ti];
        const int32_t* tf = g.tfIds.data() + g.tfOff[(size_t)ti];
        const int32_t np = g.tpOff[(size_t)ti + 1] - g.tpOff[(size_t)ti], nf = g.tfOff[(size_t)ti + 1] - g.tfOff[(size_t)ti];
        CHECK(ascendingUnique(tp, tp + np), "geom: tpIds ascending and unique", "tile %d", ti);
        CHECK(ascendingUnique(tf, tf + nf), "geom: tfIds ascending and unique", "tile %d", ti);
        CHECK(np == (int32_t)pts.size() && std::equal(pts.begin(), pts.end(), tp), "geom: tpIds are the points of the tile's cells", "tile %d: %d listed, %zu expected", ti, np, pts.size());
        bool facesOk = nf == (int32_t)fcs.size();
        for (int32_t k = 0; facesOk && k < nf; ++k) facesOk = (tf[k] & 0x7fffffff) == fcs[(size_t)k];
        CHECK(facesOk, "geom: tfIds are the faces of the tile's cells", "tile %d: %d listed, %zu expected", ti, nf, fcs.size());
        // caps (capWeighted is soft: a one-cell tile may exceed it)
        CHECK(nc <= std::min(cap.cells, T), "geom cap: cells per tile", "tile %d: %d cells, cap %d, threads %d", ti, nc, cap.cells, T);
        CHECK(np <= cap.points, "geom cap: points", "tile %d: %d > %d", ti, np, cap.points);
        CHECK(nf <= cap.faces, "geom cap: faces", "tile %d: %d > %d", ti, nf, cap.faces);
        CHECK(nc == 1 || 3LL * np + (long long)cap.faceWeight * nf <= cap.weighted, "geom cap: weighted (soft) exceeded by a tile of several cells", "tile %d: %d cells, %lld > %d",
              ti, nc, 3LL * np + (long long)cap.faceWeight * nf, cap.weighted);
        // the greedy boundary: a tile closes only where its next cell would break a cap (or at a segment cut)
        if (ti + 1 < nt && !cuts.count(ce)) {
            const int32_t c = g.order[(size_t)ce];
            std::vector<int32_t> p2(pts), f2(fcs);
            p2.insert(p2.end(), a.cellPoints[(size_t)c].begin(), a.cellPoints[(size_t)c].end());
            for (int32_t v : a.cellFaces[(size_t)c]) f2.push_back(v & 0x7fffffff);
            sortUnique(p2); sortUnique(f2);
            const int32_t P2 = (int32_t)p2.size(), F2 = (int32_t)f2.size();
            CHECK(nc + 1 > std::min(cap.cells, T) || P2 > cap.points || F2 > cap.faces || 3LL * P2 + (long long)cap.faceWeight * F2 > cap.weighted,
                  "geom boundary: a tile closed although its next cell fits every cap", "tile %d (%d cells) + cell %d: %d points %d faces", ti, nc, c, P2, F2);
        }
        // owner bit
        for (int32_t k = 0; k < nf; ++k) {
            const int32_t f = tf[k] & 0x7fffffff;
            const bool bit = tf[k] < 0, ownerHere = cellTile[(size_t)m.own[(size_t)f]] == ti;
            CHECK(bit == ownerHere, "geom: tfIds bit 31 = the tile holds the face's owner", "tile %d face %d: bit %d, owner in tile %d", ti, f, (int)bit, (int)ownerHere);
            if (bit) ++ownerMarks[(size_t)f];
        }
        // face vertices
        const int32_t fw = g.fvWidth[(size_t)ti];
        CHECK(fw % 4 == 0 && fw >= longestFace && fw >= 4, "geom: faceVerts width", "tile %d: width %d, longest face %d", ti, fw, longestFace);
        CHECK((size_t)g.fvBase[(size_t)ti] == fvNext, "geom: faceVerts tiles packed in order", "tile %d: base %d, expected %zu", ti, g.fvBase[(size_t)ti], fvNext);
        fvNext = (size_t)g.fvBase[(size_t)ti] + (size_t)nf * fw;
        if (fvNext > g.faceVerts.size()) { CHECK(false, "geom: faceVerts bounds", "tile %d", ti); return; }
        for (int32_t k = 0; k < nf; ++k) {
            const int32_t f = tf[k] & 0x7fffffff, b = m.fo[(size_t)f], n = m.fo[(size_t)f + 1] - b;
            const uint16_t* row = g.faceVerts.data() + g.fvBase[(size_t)ti] + (size_t)k * fw;
            for (int32_t j = 0; j < fw; ++j) {
                if (j < n) CHECK(row[j] < np && tp[row[j]] == m.fp[(size_t)(b + j)], "geom: faceVerts decode to the face's points in order", "tile %d face %d entry %d: %d", ti, f, j, (int)row[j]);
                else CHECK(row[j] == kEllPad, "geom: faceVerts pads after the face's points", "tile %d face %d entry %d: %d", ti, f, j, (int)row[j]);
            }
        }
        // cell faces: sliced ELL over `threads` lanes
        const int32_t cw = g.cfWidth[(size_t)ti];
        CHECK(cw % 4 == 0 && cw >= longestCell && cw >= 4, "geom: cellFaces width", "tile %d: width %d, longest cell %d", ti, cw, longestCell);
        CHECK((size_t)g.cfBase[(size_t)ti] == cfNext, "geom: cellFaces tiles packed in order (stride = threads)", "tile %d: base %d, expected %zu", ti, g.cfBase[(size_t)ti], cfNext);
        cfNext = (size_t)g.cfBase[(size_t)ti] + (size_t)cw * T;
        if (cfNext > g.cellFaces.size()) { CHECK(false, "geom: cellFaces bounds", "tile %d", ti); return; }
        for (int32_t t = 0; t < T; ++t) {
            const std::vector<int32_t>* row = t < nc ? &a.cellFaces[(size_t)g.order[(size_t)(cb + t)]] : nullptr;
            for (int32_t j = 0; j < cw; ++j) {
                const uint16_t v = g.cellFaces[ell(g.cfBase[(size_t)ti], T, j, t)];
                if (row && j < (int32_t)row->size()) {
                    const int32_t want = (*row)[(size_t)j];
                    const int32_t loc = v & 0x7fff;
                    CHECK(loc < nf && (tf[loc] & 0x7fffffff) == (want & 0x7fffffff), "geom: cellFaces decode to the cell's faces in order", "tile %d lane %d entry %d: %d", ti, t, j, (int)v);
                    CHECK(((v & 0x8000) != 0) == (want < 0), "geom: cellFaces 0x8000 exactly where the cell is the neighbour", "tile %d lane %d entry %d", ti, t, j);
                } else CHECK(v == kEllPad, "geom: cellFaces pads after the row and on idle lanes", "tile %d lane %d entry %d: %d", ti, t, j, (int)v);
            }
        }
        CHECK(g.tileFlags[(size_t)ti] == ((allQuads ? 1 : 0) | (allHex ? 2 : 0)), "geom: tileFlags", "tile %d: %d, quads %d hex %d", ti, (int)g.tileFlags[(size_t)ti], (int)allQuads, (int)allHex);
        maxP = std::max(maxP, np); maxF = std::max(maxF, nf);
    }
    CHECK(fvNext == g.faceVerts.size(), "geom: faceVerts size", "%zu, expected %zu", g.faceVerts.size(), fvNext);
    CHECK(cfNext == g.cellFaces.size(), "geom: cellFaces size", "%zu, expected %zu", g.cellFaces.size(), cfNext);
    for (int32_t f = 0; f < m.nF; ++f) CHECK(ownerMarks[(size_t)f] == 1, "geom: one owner bit per face", "face %d: %d", f, ownerMarks[(size_t)f]);
    CHECK(g.maxPoints == maxP && g.maxFaces == maxF, "geom: maxPoints / maxFaces", "%d %d, true %d %d", g.maxPoints, g.maxFaces, maxP, maxF);
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct SmoothCaps { int32_t cells, points, total; };

void checkSmooth(const char* who, const Mesh& m, const Adj& a, const Topology& topo, const SmoothTiles& s, int32_t T, const SmoothCaps& cap,
                 const std::vector<int32_t>* subset, int segs) {
    const std::string w = who;
    const int32_t nPos = subset ? (int32_t)subset->size() : m.nP;
    CHECK(s.threads == T, w + ": threads", "%d", s.threads);
    if (subset) CHECK(s.order == *subset, w + ": order is the subset", "%zu entries", s.order.size());
    else CHECK(isPermutation(s.order, m.nP), w + ": order is a permutation of the points", "%zu entries", s.order.size());
    if ((int32_t)s.order.size() != nPos) return;
    const auto cuts = checkBoundaries(who, s.ptBeg, s.nTiles, nPos, segs);
    const int32_t nt = s.nTiles;
    const bool sizes = (int32_t)s.tcOff.size() == nt + 1 && (int32_t)s.tnOff.size() == nt + 1 && (int32_t)s.selfLoc.size() == nPos &&
                       (int32_t)s.pcBase.size() == nt && (int32_t)s.ppBase.size() == nt && (int32_t)s.pfBase.size() == nt && (int32_t)s.pcWidth.size() == nt &&
                       (int32_t)s.ppWidth.size() == nt && (int32_t)s.pfWidth.size() == nt && s.tcOff.back() == (int32_t)s.tcIds.size() &&
                       s.tnOff.back() == (int32_t)s.tnIds.size() && s.pairEll.size() == s.ppEll.size() && (int32_t)s.ptBeg.size() == nt + 1;
    CHECK(sizes, w + ": table sizes", "nTiles %d", nt);
    if (!sizes) return;
    const bool pairs = topo.maxPointPoints <= 16;
    int32_t maxC = 0, maxN = 0;
    size_t pcNext = 0, ppNext = 0, pfNext = 0;
    std::vector<int32_t> cls, nbs;
    for (int32_t ti = 0; ti < nt; ++ti) {
        const int32_t pb = s.ptBeg[(size_t)ti], pe = s.ptBeg[(size_t)ti + 1], npt = pe - pb;
        cls.clear(); nbs.clear();
        int32_t lc = 0, ln = 0, lf = 0;
        for (int32_t pi = pb; pi < pe; ++pi) {
            const int32_t p = s.order[(size_t)pi];
            cls.insert(cls.end(), a.pointCells[(size_t)p].begin(), a.pointCells[(size_t)p].end());
            nbs.push_back(p);
            nbs.insert(nbs.end(), a.pointPoints[(size_t)p].begin(), a.pointPoints[(size_t)p].end());
            lc = std::max(lc, (int32_t)a.pointCells[(size_t)p].size());
            ln = std::max(ln, (int32_t)a.pointPoints[(size_t)p].size());
            lf = std::max(lf, 2 * a.pointFaceCount[(size_t)p]);
        }
        sortUnique(cls); sortUnique(nbs);
        const int32_t* tc = s.tcIds.data() + s.tcOff[(size_t)ti];
        const int32_t* tn = s.tnIds.data() + s.tnOff[(size_t)ti];
        const int32_t nc = s.tcOff[(size_t)ti + 1] - s.tcOff[(size_t)ti], nn = s.tnOff[(size_t)ti + 1] - s.tnOff[(size_t)ti];
        CHECK(ascendingUnique(tc, tc + nc, -1), w + ": tcIds ascending and unique", "tile %d", ti);
        CHECK(ascendingUnique(tn, tn + nn, -1), w + ": tnIds ascending and unique", "tile %d", ti);
        CHECK(nc == (int32_t)cls.size() && std::equal(cls.begin(), cls.end(), tc), w + ": tcIds are the cells of the tile's points", "tile %d: %d listed, %zu expected", ti, nc, cls.size());
        CHECK(nn == (int32_t)nbs.size() && std::equal(nbs.begin(), nbs.end(), tn), w + ": tnIds are the tile's points and their neighbours", "tile %d: %d listed, %zu expected", ti, nn, nbs.size());
        CHECK(npt <= T, w + " cap: points per tile <= threads", "tile %d: %d", ti, npt);
        CHECK(nc <= cap.cells, w + " cap: cells", "tile %d: %d > %d", ti, nc, cap.cells);
        CHECK(nn <= cap.points, w + " cap: points", "tile %d: %d > %d", ti, nn, cap.points);
        CHECK(npt == 1 || nc + nn <= cap.total, w + " cap: total (soft) exceeded by a tile of several points", "tile %d: %d points, %d > %d", ti, npt, nc + nn, cap.total);
        if (ti + 1 < nt && !cuts.count(pe)) {
            const int32_t p = s.order[(size_t)pe];
            std::vector<int32_t> c2(cls), n2(nbs);
            c2.insert(c2.end(), a.pointCells[(size_t)p].begin(), a.pointCells[(size_t)p].end());
            n2.push_back(p);
            n2.insert(n2.end(), a.pointPoints[(size_t)p].begin(), a.pointPoints[(size_t)p].end());
            sortUnique(c2); sortUnique(n2);
            const int32_t C2 = (int32_t)c2.size(), N2 = (int32_t)n2.size();
            CHECK(npt + 1 > T || C2 > cap.cells || N2 > cap.points || C2 + N2 > cap.total, w + " boundary: a tile closed although its next point fits every cap",
                  "tile %d (%d points) + point %d: %d cells %d points", ti, npt, p, C2, N2);
        }
        const int32_t wc = s.pcWidth[(size_t)ti], wn = s.ppWidth[(size_t)ti], wf = s.pfWidth[(size_t)ti];
        CHECK(wc % 4 == 0 && wc >= std::max(lc, 4), w + ": pcEll width", "tile %d: %d, longest %d", ti, wc, lc);
        CHECK(wn % 4 == 0 && wn >= std::max(ln, 4), w + ": ppEll width", "tile %d: %d, longest %d", ti, wn, ln);
        CHECK(wf % 4 == 0 && wf >= std::max(lf, 4), w + ": pfEll width", "tile %d: %d, longest %d", ti, wf, lf);
        CHECK((size_t)s.pcBase[(size_t)ti] == pcNext, w + ": pcEll tiles packed in order (stride = threads)", "tile %d: base %d, expected %zu", ti, s.pcBase[(size_t)ti], pcNext);
        CHECK((size_t)s.ppBase[(size_t)ti] == ppNext, w + ": ppEll tiles packed in order (stride = threads)", "tile %d: base %d, expected %zu", ti, s.ppBase[(size_t)ti], ppNext);
        CHECK((size_t)s.pfBase[(size_t)ti] == pfNext, w + ": pfEll tiles packed in order (stride = threads)", "tile %d: base %d, expected %zu", ti, s.pfBase[(size_t)ti], pfNext);
        pcNext = (size_t)s.pcBase[(size_t)ti] + (size_t)wc * T;
        ppNext = (size_t)s.ppBase[(size_t)ti] + (size_t)wn * T;
        pfNext = (size_t)s.pfBase[(size_t)ti] + (size_t)wf * T;
        if (pcNext > s.pcEll.size() || ppNext > s.ppEll.size() || pfNext > s.pfEll.size()) { CHECK(false, w + ": ELL bounds", "tile %d", ti); return; }
        for (int32_t t = 0; t < T; ++t) {
            const int32_t p = t < npt ? s.order[(size_t)(pb + t)] : -1;
            if (p >= 0) CHECK(s.selfLoc[(size_t)(pb + t)] < nn && tn[s.selfLoc[(size_t)(pb + t)]] == p, w + ": selfLoc decodes to the point", "tile %d lane %d", ti, t);
            const std::vector<int32_t>* pcr = p >= 0 ? &a.pointCells[(size_t)p] : nullptr;
            const std::vector<int32_t>* ppr = p >= 0 ? &a.pointPoints[(size_t)p] : nullptr;
            for (int32_t j = 0; j < wc; ++j) {
                const uint16_t v = s.pcEll[ell(s.pcBase[(size_t)ti], T, j, t)];
                if (pcr && j < (int32_t)pcr->size()) CHECK(v < nc && tc[v] == (*pcr)[(size_t)j], w + ": pcEll decodes to pointCells in order", "tile %d lane %d entry %d: %d", ti, t, j, (int)v);
                else CHECK(v == kEllPad, w + ": pcEll pads after the row and on idle lanes", "tile %d lane %d entry %d: %d", ti, t, j, (int)v);
            }
            const int32_t val = ppr ? (int32_t)ppr->size() : 0;
            for (int32_t j = 0; j < wn; ++j) {
                const size_t at = ell(s.ppBase[(size_t)ti], T, j, t);
                const uint16_t v = s.ppEll[at], pm = s.pairEll[at];
                if (j < val) {
                    const int32_t q = (*ppr)[(size_t)j], loc = v & 0x7fff;
                    CHECK(loc < nn && tn[loc] == q, w + ": ppEll decodes to pointPoints in order", "tile %d lane %d entry %d: %d", ti, t, j, (int)v);
                    CHECK(((v & 0x8000) != 0) == (m.internal[(size_t)q] != 0), w + ": ppEll bit 15 exactly on internal neighbours", "tile %d point %d neighbour %d", ti, p, q);
                    uint16_t want = 0;
                    if (pairs)
                        for (int32_t i = 0; i < val; ++i) {
                            if (i == j) continue;
                            const auto& A = a.pointCells[(size_t)q];
                            const auto& B = a.pointCells[(size_t)(*ppr)[(size_t)i]];
                            if (intersects(A, B)) want |= (uint16_t)(1u << i);
                        }
                    CHECK(pm == want, pairs ? w + ": pairEll bit i = neighbours j and i share a cell" : w + ": no pairEll bits beyond 16 neighbours",
                          "tile %d point %d neighbour %d: %04x, expected %04x", ti, p, j, (unsigned)pm, (unsigned)want);
                } else {
                    CHECK(v == kEllPad, w + ": ppEll pads after the row and on idle lanes", "tile %d lane %d entry %d: %d", ti, t, j, (int)v);
                    CHECK(pm == 0, w + ": pairEll zero after the row and on idle lanes", "tile %d lane %d entry %d: %04x", ti, t, j, (unsigned)pm);
                }
            }
            // face corners: (previous, next) per face holding the point -- chained into trails, so compared as a multiset of unordered pairs
            std::vector<std::pair<int32_t, int32_t>> want, got;
            const int32_t nfc = p >= 0 ? a.pointFaceCount[(size_t)p] : 0;
            for (int32_t k = 0; k < nfc; ++k) {
                const int32_t x = a.pointCorners[(size_t)p][(size_t)(2 * k)], y = a.pointCorners[(size_t)p][(size_t)(2 * k + 1)];
                want.push_back({std::min(x, y), std::max(x, y)});
            }
            bool decodable = true;
            for (int32_t j = 0; j < wf; ++j) {
                const uint16_t v = s.pfEll[ell(s.pfBase[(size_t)ti], T, j, t)];
                if (j < 2 * nfc) decodable = decodable && v < nn;
                else CHECK(v == kEllPad, w + ": pfEll pads after the corners and on idle lanes", "tile %d lane %d entry %d: %d", ti, t, j, (int)v);
            }
            if (nfc) {
                CHECK(decodable, w + ": pfEll entries are tile-local points", "tile %d lane %d", ti, t);
                if (decodable) {
                    for (int32_t k = 0; k < nfc; ++k) {
                        const int32_t x = tn[s.pfEll[ell(s.pfBase[(size_t)ti], T, 2 * k, t)]], y = tn[s.pfEll[ell(s.pfBase[(size_t)ti], T, 2 * k + 1, t)]];
                        got.push_back({std::min(x, y), std::max(x, y)});
                    }
                    std::sort(want.begin(), want.end()); std::sort(got.begin(), got.end());
                    CHECK(want == got, w + ": pfEll holds the previous / next vertex of the point in each of its faces", "tile %d point %d", ti, p);
                }
            }
        }
        maxC = std::max(maxC, nc); maxN = std::max(maxN, nn);
    }
    CHECK(pcNext == s.pcEll.size() && ppNext == s.ppEll.size() && pfNext == s.pfEll.size(), w + ": ELL sizes", "%zu %zu %zu", s.pcEll.size(), s.ppEll.size(), s.pfEll.size());
    CHECK(s.maxCells == maxC && s.maxPoints == maxN, w + ": maxCells / maxPoints", "%d %d, true %d %d", s.maxCells, s.maxPoints, maxC, maxN);
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct EdgeCaps { int32_t points, faces, cells, total; };

void checkEdges(const Mesh& m, const Adj& a, const Topology& topo, const EdgeTiles& e, int32_t T, const EdgeCaps& cap, int segs) {
    const int32_t nE = (int32_t)a.edges.size();
    CHECK(topo.nEdges == nE, "topology: edge count", "%d, mesh %d", topo.nEdges, nE);
    if (topo.nEdges != nE) return;
    // the edge numbering and the rings the tables encode (Topology's): rings are permutations of the edge's faces / cells, cell i
    // between ring faces i and i + 1
    for (int32_t k = 0; k < nE; ++k) {
        CHECK(topo.edges[2 * (size_t)k] == a.edges[(size_t)k].first && topo.edges[2 * (size_t)k + 1] == a.edges[(size_t)k].second, "topology: edges", "edge %d", k);
        const int32_t fb = topo.edgeFaces.off[(size_t)k], nf = topo.edgeFaces.off[(size_t)k + 1] - fb;
        const int32_t cb = topo.edgeCells.off[(size_t)k], ncl = topo.edgeCells.off[(size_t)k + 1] - cb;
        std::vector<int32_t> rf(topo.ringFace.begin() + fb, topo.ringFace.begin() + fb + nf), rc(topo.ringCell.begin() + cb, topo.ringCell.begin() + cb + ncl);
        if (!topo.edgeRingOk[(size_t)k]) continue;
        for (int32_t i = 0; i < ncl; ++i) {
            const int32_t c = rc[(size_t)i];
            for (int32_t f : {rf[(size_t)i], rf[(size_t)((i + 1) % nf)]})
                CHECK(m.own[(size_t)f] == c || (f < m.nIF && m.nei[(size_t)f] == c), "topology: ring cell between its ring faces", "edge %d cell %d face %d", k, c, f);
        }
        std::sort(rf.begin(), rf.end()); std::sort(rc.begin(), rc.end());
        CHECK(rf == a.edgeFaces[(size_t)k] && rc == a.edgeCells[(size_t)k], "topology: rings are the edge's faces and cells", "edge %d", k);
    }
    CHECK(e.threads == T, "edge: threads", "%d", e.threads);
    CHECK(isPermutation(e.order, nE), "edge: order is a permutation of the edges", "%zu entries", e.order.size());
    if (!isPermutation(e.order, nE)) return;
    const auto cuts = checkBoundaries("edge", e.edgeBeg, e.nTiles, nE, segs);
    const int32_t nt = e.nTiles;
    const bool sizes = (int32_t)e.tpOff.size() == nt + 1 && (int32_t)e.tfOff.size() == nt + 1 && (int32_t)e.tcOff.size() == nt + 1 &&
                       (int32_t)e.efBase.size() == nt && (int32_t)e.ecBase.size() == nt && (int32_t)e.efWidth.size() == nt && (int32_t)e.ecWidth.size() == nt &&
                       e.epLoc.size() == 2 * (size_t)nE && e.tpOff.back() == (int32_t)e.tpIds.size() && e.tfOff.back() == (int32_t)e.tfIds.size() &&
                       e.tcOff.back() == (int32_t)e.tcIds.size() && (int32_t)e.edgeBeg.size() == nt + 1;
    CHECK(sizes, "edge: table sizes", "nTiles %d", nt);
    if (!sizes) return;
    int32_t maxP = 0, maxF = 0, maxC = 0;
    size_t efNext = 0, ecNext = 0;
    std::vector<int32_t> pts, fcs, cls;
    auto addEdge = [&](int32_t k, std::vector<int32_t>& P, std::vector<int32_t>& F, std::vector<int32_t>& C) {
        P.push_back(a.edges[(size_t)k].first); P.push_back(a.edges[(size_t)k].second);
        F.insert(F.end(), a.edgeFaces[(size_t)k].begin(), a.edgeFaces[(size_t)k].end());
        C.insert(C.end(), a.edgeCells[(size_t)k].begin(), a.edgeCells[(size_t)k].end());
    };
    for (int32_t ti = 0; ti < nt; ++ti) {
        const int32_t eb = e.edgeBeg[(size_t)ti], ee = e.edgeBeg[(size_t)ti + 1], ne = ee - eb;
        pts.clear(); fcs.clear(); cls.clear();
        int32_t lf = 0, lc = 0;
        for (int32_t ei = eb; ei < ee; ++ei) {
            const int32_t k = e.order[(size_t)ei];
            addEdge(k, pts, fcs, cls);
            lf = std::max(lf, (int32_t)a.edgeFaces[(size_t)k].size());
            lc = std::max(lc, (int32_t)a.edgeCells[(size_t)k].size());
        }
        sortUnique(pts); sortUnique(fcs); sortUnique(cls);
        const int32_t* tp = e.tpIds.data() + e.tpOff[(size_t)ti];
        const int32_t* tf = e.tfIds.data() + e.tfOff[(size_t)ti];
        const int32_t* tc = e.tcIds.data() + e.tcOff[(size_t)ti];
        const int32_t np = e.tpOff[(size_t)ti + 1] - e.tpOff[(size_t)ti], nf = e.tfOff[(size_t)ti + 1] - e.tfOff[(size_t)ti], nc = e.tcOff[(size_t)ti + 1] - e.tcOff[(size_t)ti];
        CHECK(np == (int32_t)pts.size() && std::equal(pts.begin(), pts.end(), tp), "edge: tpIds are the end points of the tile's edges", "tile %d", ti);
        CHECK(nf == (int32_t)fcs.size() && std::equal(fcs.begin(), fcs.end(), tf), "edge: tfIds are the faces of the tile's edges", "tile %d", ti);
        CHECK(nc == (int32_t)cls.size() && std::equal(cls.begin(), cls.end(), tc), "edge: tcIds are the cells of the tile's edges", "tile %d", ti);
        CHECK(ne <= T, "edge cap: edges per tile <= threads", "tile %d: %d", ti, ne);
        CHECK(np <= cap.points, "edge cap: points", "tile %d: %d > %d", ti, np, cap.points);
        CHECK(nf <= cap.faces, "edge cap: faces", "tile %d: %d > %d", ti, nf, cap.faces);
        CHECK(nc <= cap.cells, "edge cap: cells", "tile %d: %d > %d", ti, nc, cap.cells);
        CHECK(ne == 1 || np + nf + nc <= cap.total, "edge cap: total (soft) exceeded by a tile of several edges", "tile %d: %d edges, %d > %d", ti, ne, np + nf + nc, cap.total);
        if (ti + 1 < nt && !cuts.count(ee)) {
            std::vector<int32_t> P2(pts), F2(fcs), C2(cls);
            addEdge(e.order[(size_t)ee], P2, F2, C2);
            sortUnique(P2); sortUnique(F2); sortUnique(C2);
            const int32_t a2 = (int32_t)P2.size(), b2 = (int32_t)F2.size(), c2 = (int32_t)C2.size();
            CHECK(ne + 1 > T || a2 > cap.points || b2 > cap.faces || c2 > cap.cells || a2 + b2 + c2 > cap.total, "edge boundary: a tile closed although its next edge fits every cap",
                  "tile %d (%d edges): %d points %d faces %d cells", ti, ne, a2, b2, c2);
        }
        const int32_t wf = e.efWidth[(size_t)ti], wc = e.ecWidth[(size_t)ti];
        CHECK(wf % 4 == 0 && wf >= std::max(lf, 4), "edge: efEll width", "tile %d: %d, longest %d", ti, wf, lf);
        CHECK(wc % 4 == 0 && wc >= std::max(lc, 4), "edge: ecEll width", "tile %d: %d, longest %d", ti, wc, lc);
        CHECK((size_t)e.efBase[(size_t)ti] == efNext, "edge: efEll tiles packed in order (stride = threads)", "tile %d", ti);
        CHECK((size_t)e.ecBase[(size_t)ti] == ecNext, "edge: ecEll tiles packed in order (stride = threads)", "tile %d", ti);
        efNext = (size_t)e.efBase[(size_t)ti] + (size_t)wf * T;
        ecNext = (size_t)e.ecBase[(size_t)ti] + (size_t)wc * T;
        if (efNext > e.efEll.size() || ecNext > e.ecEll.size()) { CHECK(false, "edge: ELL bounds", "tile %d", ti); return; }
        for (int32_t t = 0; t < T; ++t) {
            const int32_t k = t < ne ? e.order[(size_t)(eb + t)] : -1;
            if (k >= 0) {
                const uint16_t l0 = e.epLoc[2 * (size_t)(eb + t)], l1 = e.epLoc[2 * (size_t)(eb + t) + 1];
                CHECK(l0 < np && l1 < np && tp[l0] == a.edges[(size_t)k].first && tp[l1] == a.edges[(size_t)k].second, "edge: epLoc decodes to the edge's end points", "tile %d edge %d", ti, k);
            }
            const bool ring = k >= 0 && topo.edgeRingOk[(size_t)k];
            const int32_t fb = k >= 0 ? topo.edgeFaces.off[(size_t)k] : 0, nfe = ring ? topo.edgeFaces.off[(size_t)k + 1] - fb : 0;
            const int32_t cb = k >= 0 ? topo.edgeCells.off[(size_t)k] : 0, nce = ring ? topo.edgeCells.off[(size_t)k + 1] - cb : 0;
            for (int32_t j = 0; j < wf; ++j) {
                const uint16_t v = e.efEll[ell(e.efBase[(size_t)ti], T, j, t)];
                if (j < nfe) CHECK(v < nf && tf[v] == topo.ringFace[(size_t)(fb + j)], "edge: efEll decodes to ringFace in order", "tile %d edge %d entry %d", ti, k, j);
                else CHECK(v == kEllPad, k >= 0 && !ring ? "edge: non-manifold edge has an all-pad face row" : "edge: efEll pads after the row and on idle lanes", "tile %d lane %d entry %d", ti, t, j);
            }
            for (int32_t j = 0; j < wc; ++j) {
                const uint16_t v = e.ecEll[ell(e.ecBase[(size_t)ti], T, j, t)];
                if (j < nce) CHECK(v < nc && tc[v] == topo.ringCell[(size_t)(cb + j)], "edge: ecEll decodes to ringCell in order", "tile %d edge %d entry %d", ti, k, j);
                else CHECK(v == kEllPad, k >= 0 && !ring ? "edge: non-manifold edge has an all-pad cell row" : "edge: ecEll pads after the row and on idle lanes", "tile %d lane %d entry %d", ti, t, j);
            }
        }
        maxP = std::max(maxP, np); maxF = std::max(maxF, nf); maxC = std::max(maxC, nc);
    }
    CHECK(efNext == e.efEll.size() && ecNext == e.ecEll.size(), "edge: ELL sizes", "%zu %zu", e.efEll.size(), e.ecEll.size());
    CHECK(e.maxPoints == maxP && e.maxFaces == maxF && e.maxCells == maxC, "edge: maxPoints / maxFaces / maxCells", "%d %d %d, true %d %d %d", e.maxPoints, e.maxFaces, e.maxCells, maxP, maxF, maxC);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s mesh.bin [key=value ...]\n", argv[0]); return 2; }
    Mesh m;
    if (!readMesh(argv[1], m)) { std::printf("error reading %s\n", argv[1]); return 2; }
    std::map<std::string, long long> kv;
    for (int i = 2; i < argc; ++i) {
        const char* eq = std::strchr(argv[i], '=');
        if (!eq) { std::fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
        kv[std::string(argv[i], (size_t)(eq - argv[i]))] = std::atoll(eq + 1);
    }
    auto opt = [&](const char* k, long long d) { auto it = kv.find(k); return (int32_t)(it == kv.end() ? d : it->second); };
    const int32_t T = opt("T", 256);
    const bool morton = opt("morton", 1) != 0;
    // the defaults smgpu.hip derives from the thread count (smgpu_create; SMGPU_GEOM_WAVES = 5, face stride 6)
    const int32_t gc = opt("gc", T / 2);
    const GeomCaps gcap{gc, opt("gp", std::min(6 * gc, 1400)), opt("gf", std::min(4 * gc, 1400)), opt("gw", T == 256 ? 3980 : INT_MAX), opt("fw", 6)};
    const SmoothCaps scap{opt("sc", std::min(2 * T, 1500)), opt("sn", std::min(3 * T, 1500)), opt("st", T == 256 ? 1112 : INT_MAX)};
    const EdgeCaps ecap{opt("ep", 512), opt("ef", 768), opt("ec", 512), opt("et", 852)};
    const int segsArg = opt("segs", 1);
    const int subsetSeed = opt("subset", 0);

    Adj a;
    buildAdj(m, a);
    {   // the largest single element's need per cap (what a tile of one element stages)
        long long gP = 0, gF = 0, gW = 0, sC = 0, sN = 0, sT = 0, eP = 0, eF = 0, eC = 0, eT = 0;
        for (int32_t c = 0; c < m.nC; ++c) {
            const long long p = (long long)a.cellPoints[(size_t)c].size(), f = (long long)a.cellFaces[(size_t)c].size();
            gP = std::max(gP, p); gF = std::max(gF, f); gW = std::max(gW, 3 * p + gcap.faceWeight * f);
        }
        for (int32_t p = 0; p < m.nP; ++p) {
            const long long c = (long long)a.pointCells[(size_t)p].size(), n = 1 + (long long)a.pointPoints[(size_t)p].size();
            sC = std::max(sC, c); sN = std::max(sN, n); sT = std::max(sT, c + n);
        }
        for (size_t k = 0; k < a.edges.size(); ++k) {
            const long long f = (long long)a.edgeFaces[k].size(), c = (long long)a.edgeCells[k].size();
            eP = 2; eF = std::max(eF, f); eC = std::max(eC, c); eT = std::max(eT, 2 + f + c);
        }
        std::printf("need gp=%lld gf=%lld gw=%lld sc=%lld sn=%lld st=%lld ep=%lld ef=%lld ec=%lld et=%lld\n", gP, gF, gW, sC, sN, sT, eP, eF, eC, eT);
    }

    Topology topo;
    const std::string te = topo.build(m.nP, m.nC, m.nF, m.nIF, m.fo.data(), m.fp.data(), m.own.data(), m.nei.data());
    if (!te.empty()) { std::printf("error topology: %s\n", te.c_str()); return 1; }
    // Topology's lists the tile builders read, against the mesh
    for (int32_t c = 0; c < m.nC; ++c) {
        const auto& r = a.cellFaces[(size_t)c];
        CHECK(std::equal(r.begin(), r.end(), topo.cellFacesGeom.val.begin() + topo.cellFacesGeom.off[(size_t)c]) &&
                  (size_t)(topo.cellFacesGeom.off[(size_t)c + 1] - topo.cellFacesGeom.off[(size_t)c]) == r.size(), "topology: cellFacesGeom", "cell %d", c);
    }
    for (int32_t p = 0; p < m.nP; ++p) {
        const auto& c = a.pointCells[(size_t)p];
        const auto& q = a.pointPoints[(size_t)p];
        CHECK((size_t)(topo.pointCells.off[(size_t)p + 1] - topo.pointCells.off[(size_t)p]) == c.size() &&
                  std::equal(c.begin(), c.end(), topo.pointCells.val.begin() + topo.pointCells.off[(size_t)p]), "topology: pointCells", "point %d", p);
        CHECK((size_t)(topo.pointEdges.off[(size_t)p + 1] - topo.pointEdges.off[(size_t)p]) == q.size() &&
                  std::equal(q.begin(), q.end(), topo.pointPoints.begin() + topo.pointEdges.off[(size_t)p]), "topology: pointPoints", "point %d", p);
    }

    // the engine's calls (smgpu_create): one Z-curve of the points for the smoothing and the edge tiles
    std::vector<int32_t> pointOrder;
    if (morton) pointOrder = mortonOrderOf(m.nP, m.pts.data());
    auto segsFor = [&](int64_t n, int64_t threshold) { return n >= threshold ? segsArg : 1; };
    GeomTiles gt; SmoothTiles st; EdgeTiles et;
    const std::string eg = gt.build(topo, m.pts.data(), morton, T, gcap.cells, gcap.points, gcap.faces, gcap.weighted, gcap.faceWeight);
    const std::string es = st.build(topo, m.pts.data(), m.internal.data(), morton, T, scap.cells, scap.points, morton ? &pointOrder : nullptr, nullptr, scap.total);
    const std::string ee = et.build(topo, m.pts.data(), morton, T, ecap.points, ecap.faces, ecap.cells, morton ? &pointOrder : nullptr, ecap.total);
    if (!eg.empty()) std::printf("error geom: %s\n", eg.c_str());
    else checkGeom(m, a, gt, T, gcap, segsFor(m.nC, 2 << 20));
    if (!es.empty()) std::printf("error smooth: %s\n", es.c_str());
    else checkSmooth("smooth", m, a, topo, st, T, scap, nullptr, segsFor(m.nP, 2 << 20));
    if (!ee.empty()) std::printf("error edge: %s\n", ee.c_str());
    else checkEdges(m, a, topo, et, T, ecap, segsFor((int64_t)a.edges.size(), 4 << 20));
    int subTiles = -1;
    if (subsetSeed) {   // the shared-point form (smgpu.hip, shared-point tiles): a subset of the points in an order of their own
        std::mt19937 rng((unsigned)subsetSeed);
        std::vector<int32_t> sub;
        for (int32_t p = 0; p < m.nP; ++p) if (rng() % 3 == 0) sub.push_back(p);
        std::shuffle(sub.begin(), sub.end(), rng);
        SmoothTiles sh;
        std::vector<double> zeros(3 * (size_t)m.nP, 0.0);
        const std::string eh = sh.build(topo, zeros.data(), m.internal.data(), false, T, scap.cells, scap.points, nullptr, &sub, scap.total);
        if (!eh.empty()) std::printf("error subset: %s\n", eh.c_str());
        else { checkSmooth("subset", m, a, topo, sh, T, scap, &sub, segsFor((int64_t)sub.size(), 2 << 20)); subTiles = sh.nTiles; }
    }
    for (const auto& f : R.fails) std::printf("FAIL %s: n=%lld first: %s\n", f.first.c_str(), f.second.first, f.second.second.c_str());
    int32_t nonManifold = 0;
    for (uint8_t ok : topo.edgeRingOk) nonManifold += ok ? 0 : 1;
    std::printf("tiles geom=%d smooth=%d edge=%d subset=%d cells=%d points=%d edges=%d maxPointPoints=%d nonManifoldEdges=%d\n", eg.empty() ? gt.nTiles : -1,
                es.empty() ? st.nTiles : -1, ee.empty() ? et.nTiles : -1, subTiles, m.nC, m.nP, topo.nEdges, topo.maxPointPoints, nonManifold);
    return R.fails.empty() ? 0 : 1;
}
