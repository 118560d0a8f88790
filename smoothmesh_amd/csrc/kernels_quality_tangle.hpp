// kernels_quality_tangle.hpp -- the tangle constraint (smgpu_set_tangle_constraint: include/smgpu.h, DESIGN.md "Mesh quality",
// 10.12): behind the movePoints of every iteration the points whose move turned a cell bad go back to where the iteration found them.
//
// Per iteration the engine queues, on its own stream and in front of the trace's launches, for k = 0 .. passes
//   1. k_tangle_tile: the geometry tile of the new points (the phases of k_geom_tile, nothing published) and, on the face records
//      the tile holds in LDS, the verdict on every cell -- bad: V_c <= VSMALL with the report's V_c, or an own-side pyramid <= 0
//      against the loop's C_c.  A tile with a bad cell that is not exempt marks the points of the cell's faces, one byte per
//      point id, and adds its count to the device word (one integer atomic per workgroup; no float atomics anywhere);
//   2. k_tangle_verdict: one wave, all values written by one lane: nothing bad -> the "clean" word that turns everything queued
//      behind for this iteration into a no-op; bad and k == passes -> the full revert; else one more marked pass.  Fills the record;
//   3. k_tangle_apply: a streaming pass that restores the marked points (or all of them) from the points the iteration started
//      from, clears the marks and counts the points that changed.
// Every kernel takes the trace's gate (qTraceRan): an iteration that did not run leaves points, marks and record alone.
// Without tiles (SMGPU_TILES=0) step 1 is k_face_geom + k_cell_centres + k_tangle_cells: the same verdicts, marks and records.
#pragma once
#include "kernels_quality_trace.hpp"

namespace smgpu {

struct TangleDev {
    int clean;     // this iteration: an evaluation found no bad cell; what is queued behind it returns at once
    int full;      // this pass restores every point
    int badNow;    // bad cells that are not exempt, counted by the evaluation in flight
    int err;       // 1: a tile's marks do not fit the LDS its points leave free
};

// The thread's cell of the tile, on the face records in LDS: bad or not.  Three bodies in one walk, each a twin of the code that
// defines it -- keep them alike: C_c is geomCell's (kernels_tiled.hpp: the estimate by divExact / divByCount, the clamp of the
// .org variant), V_c is qTileCell's (kernels_quality_trace.hpp: the estimate by a plain division, signed pyramids, no clamp), the
// own-side pyramids are pO / pN of qFaceOne (kernels_quality.hpp) with this cell's C_c.  tflags bit1: every cell has six faces.
template <int T, bool ORG>
__device__ __forceinline__ bool tangleTileCell(const GeomTileView& g, const GeomLds& L, const GeomTileMeta& tm, int tid, unsigned tflags, const GeomCellIn& in) {
    const double *fcx = L.fcx, *fcy = L.fcy, *fcz = L.fcz, *fax = L.fax, *fay = L.fay, *faz = L.faz;
    const int cw4 = tm.cfWidth >> 2;
    const ushort4* row = reinterpret_cast<const ushort4*>(g.cellFaces + tm.cfBase) + tid;
    V3 sum = v3(0, 0, 0), cG, cQ, ctr = v3(0, 0, 0);
    double vol = 0.0, pyr = 0.0;
    bool bad = false;
#define SMGPU_TPYR(E, FC)                                                          \
    {                                                                              \
        const V3 fC = (FC);                                                        \
        const V3 fA = ldsg(fax, fay, faz, kGF * ((E) & 0x7fff));                   \
        double pyr3Vol = dot(fA, fC - cG);                                         \
        pyr3Vol = ((E) & 0x8000) ? -pyr3Vol : pyr3Vol;                             \
        if (ORG) pyr3Vol = (pyr3Vol > SMGPU_VSMALL) ? pyr3Vol : SMGPU_VSMALL;      \
        const V3 pc = (3.0 / 4.0) * fC + (1.0 / 4.0) * cG;                         \
        ctr = ctr + pyr3Vol * pc;                                                  \
        vol += pyr3Vol;                                                            \
    }
#define SMGPU_TOWN(E, FC)                                                          \
    {                                                                              \
        const V3 fC = (FC);                                                        \
        const V3 fA = ldsg(fax, fay, faz, kGF * ((E) & 0x7fff));                   \
        double p = dot(fA, fC - cQ);                                               \
        if ((E) & 0x8000) p = -p;                                                  \
        pyr += p;                                                                  \
        const double own = ((E) & 0x8000) ? dot(fA, ctr - fC) : dot(fA, fC - ctr); \
        bad = bad || own <= 0.0;                                                   \
    }
    if ((tflags & 2u)) {
        const ushort4 qa = in.qa, qb = in.qb;
        const unsigned e0 = qa.x, e1 = qa.y, e2 = qa.z, e3 = qa.w, e4 = qb.x, e5 = qb.y;
        const V3 c0 = ldsg(fcx, fcy, fcz, kGF * (e0 & 0x7fff)), c1 = ldsg(fcx, fcy, fcz, kGF * (e1 & 0x7fff)), c2 = ldsg(fcx, fcy, fcz, kGF * (e2 & 0x7fff)),
                 c3 = ldsg(fcx, fcy, fcz, kGF * (e3 & 0x7fff)), c4 = ldsg(fcx, fcy, fcz, kGF * (e4 & 0x7fff)), c5 = ldsg(fcx, fcy, fcz, kGF * (e5 & 0x7fff));
        sum = sum + c0; sum = sum + c1; sum = sum + c2; sum = sum + c3; sum = sum + c4; sum = sum + c5;
        cG = divExact(sum, 6.0);
        cQ = sum / 6.0;
        SMGPU_TPYR(e0, c0) SMGPU_TPYR(e1, c1) SMGPU_TPYR(e2, c2) SMGPU_TPYR(e3, c3) SMGPU_TPYR(e4, c4) SMGPU_TPYR(e5, c5)
        if (fabs(vol) > SMGPU_VSMALL) ctr = divExact(ctr, vol);
        else ctr = cG;
        SMGPU_TOWN(e0, c0) SMGPU_TOWN(e1, c1) SMGPU_TOWN(e2, c2) SMGPU_TOWN(e3, c3) SMGPU_TOWN(e4, c4) SMGPU_TOWN(e5, c5)
    } else {
        int nFaces = 0;
        SMGPU_ELL_FOREACH(row, cw4, T, {
            sum = sum + ldsg(fcx, fcy, fcz, kGF * (e & 0x7fff));
            nFaces = j + 1;
        })
        cG = divByCount(sum, nFaces);
        cQ = sum / (double)nFaces;
        SMGPU_ELL_FOREACH(row, cw4, T, {
            (void)j;
            const V3 fc = ldsg(fcx, fcy, fcz, kGF * (e & 0x7fff));
            SMGPU_TPYR(e, fc)
        })
        if (fabs(vol) > SMGPU_VSMALL) ctr = divExact(ctr, vol);
        else ctr = cG;
        SMGPU_ELL_FOREACH(row, cw4, T, {
            (void)j;
            const V3 fc = ldsg(fcx, fcy, fcz, kGF * (e & 0x7fff));
            SMGPU_TOWN(e, fc)
        })
    }
#undef SMGPU_TPYR
#undef SMGPU_TOWN
    return bad || (1.0 / 3.0) * pyr <= SMGPU_VSMALL;
}

// The geometry tile of s.ptsCur -- the phases of geomTileBody (kernels_tiled.hpp) without the loop's stop word and deferred finish,
// wantAvg = 0, writeFaces = 0: nothing is published -- then the verdict on the tile's cells and, in a tile that holds a bad one,
// the marks.  pass > 0: a no-op once an earlier evaluation of this iteration found nothing bad.
// exemptOut != NULL (enabling): every cell's verdict goes to exemptOut[c] instead, nothing is marked, the count is the exempt cells'.
// The marks are built in the LDS the tile's points occupied (free behind the face phase): one byte per face slot, then one per
// point slot; the threads then store one byte per marked point id -- plain stores of the same value from every tile that holds the
// point.
template <int T, bool ORG>
__global__ void __launch_bounds__(T) __attribute__((amdgpu_waves_per_eu(4))) k_tangle_tile(MeshView m, State s, GeomTileView g, int nLaunch, int xcdMap,
                                                                                 const uint8_t* __restrict__ exempt, uint8_t* __restrict__ exemptOut,
                                                                                 uint8_t* __restrict__ marks, TangleDev* __restrict__ d, int pass,
                                                                                 const smgpu_iter_stats* gate) {
    if (!qTraceRan(gate) || (pass > 0 && d->clean)) return;
    const int tile = launchTile(nLaunch, xcdMap, (int)blockIdx.x);
    if (tile < 0) return;
    extern __shared__ double lds[];
    const int tid = threadIdx.x;
    const GeomTileMeta tm = loadTileMeta(g, tile);
    const GeomLds L = geomLds(lds, tm);
    int id[2];
    geomLoadIds<T>(g, tm, tid, id);
    const GeomRows r = geomLoadRows<T, ORG>(g, tm, tid);
    V3 v[2];
    geomLoadPoints(s, id, v);
    geomStorePoints<T>(s, g, tm, L, id, v, tid);
    __syncthreads();
    geomFaces<T, ORG>(s, g, L, tm, r, tid, 0, 0);
    __syncthreads();
    const unsigned tflags = (unsigned)tm.flags;
    bool bad = false;
    if (r.cin.mine) {
        bad = tangleTileCell<T, ORG>(g, L, tm, tid, tflags, r.cin);
        if (exemptOut) exemptOut[r.cin.c] = bad ? 1 : 0;
        else bad = bad && !exempt[r.cin.c];
    }
    const int nBad = __syncthreads_count(bad ? 1 : 0);
    if (nBad == 0) return;
    if (tid == 0) atomicAdd(&d->badNow, nBad);
    if (exemptOut) return;
    // the marks, in the points' LDS: face slots first, then point slots, each rounded up to whole words
    const int fBytes = (tm.nFaces + 3) & ~3, pBytes = (tm.nPts + 3) & ~3;
    if (fBytes + pBytes > 24 * tm.nPts) {
        if (tid == 0) d->err = 1;
        return;
    }
    uint8_t* const fFlag = reinterpret_cast<uint8_t*>(lds);
    uint8_t* const pFlag = fFlag + fBytes;
    for (int i = tid; i < ((fBytes + pBytes) >> 2); i += T) reinterpret_cast<unsigned*>(lds)[i] = 0u;
    __syncthreads();
    if (bad) {
        if ((tflags & 2u)) {
            const ushort4 qa = r.cin.qa, qb = r.cin.qb;
            fFlag[qa.x & 0x7fff] = 1; fFlag[qa.y & 0x7fff] = 1; fFlag[qa.z & 0x7fff] = 1; fFlag[qa.w & 0x7fff] = 1;
            fFlag[qb.x & 0x7fff] = 1; fFlag[qb.y & 0x7fff] = 1;
        } else {
            const ushort4* row = reinterpret_cast<const ushort4*>(g.cellFaces + tm.cfBase) + tid;
            SMGPU_ELL_FOREACH(row, tm.cfWidth >> 2, T, {
                (void)j;
                fFlag[e & 0x7fff] = 1;
            })
        }
    }
    __syncthreads();
    const int fw4 = tm.fvWidth >> 2;
    const ushort4* fvTile = reinterpret_cast<const ushort4*>(g.faceVerts + tm.fvBase);
    for (int i = tid; i < tm.nFaces; i += T) {
        if (!fFlag[i]) continue;
        const ushort4* row = fvTile + (size_t)i * fw4;
        SMGPU_ELL_FOREACH(row, fw4, 1, {
            (void)j;
            pFlag[e] = 1;
        })
    }
    __syncthreads();
    const int* ids = g.tpIds + tm.tpOff;
    for (int i = tid; i < tm.nPts; i += T)
        if (pFlag[i]) marks[ids[i]] = 1;
}

// Without tiles: the verdict on cell c from the face values and cell centres k_face_geom / k_cell_centres have just left by id
// (the arithmetic of the tile's cell, so the same bits: V_c as qCellVolume, the own-side pyramids against cellCtr[c]), and the
// marks through the cell's faces and their points.  One thread per cell.
constexpr int kTangleBlock = 256;
__global__ void __launch_bounds__(kTangleBlock) k_tangle_cells(MeshView m, const double* __restrict__ fCtr, const double* __restrict__ fArea,
                                                                const double* __restrict__ cellCtr, const uint8_t* __restrict__ exempt,
                                                                uint8_t* __restrict__ exemptOut, uint8_t* __restrict__ marks, TangleDev* __restrict__ d,
                                                                int pass, const smgpu_iter_stats* gate) {
    if (!qTraceRan(gate) || (pass > 0 && d->clean)) return;
    const int c = blockIdx.x * kTangleBlock + threadIdx.x;
    bool bad = false;
    if (c < m.nCells) {
        const int b = m.cfOff[c], e = m.cfOff[c + 1];
        V3 cEst = v3(0, 0, 0);
        for (int j = b; j < e; ++j) cEst = cEst + ldv(fCtr, m.cfVal[j] & 0x7fffffff);
        cEst = cEst / (double)(e - b);
        const V3 ctr = ldv(cellCtr, c);
        double pyr = 0.0;
        for (int j = b; j < e; ++j) {
            const int ev = m.cfVal[j];
            const int f = ev & 0x7fffffff;
            const V3 Sf = ldv(fArea, f), Cf = ldv(fCtr, f);
            double p = dot(Sf, Cf - cEst);
            if (ev < 0) p = -p;
            pyr += p;
            const double own = (ev < 0) ? dot(Sf, ctr - Cf) : dot(Sf, Cf - ctr);
            bad = bad || own <= 0.0;
        }
        bad = bad || (1.0 / 3.0) * pyr <= SMGPU_VSMALL;
        if (exemptOut) exemptOut[c] = bad ? 1 : 0;
        else bad = bad && !exempt[c];
        if (bad && !exemptOut) {
            for (int j = b; j < e; ++j) {
                const int f = m.cfVal[j] & 0x7fffffff;
                for (int k = m.faceOff[f]; k < m.faceOff[f + 1]; ++k) marks[m.facePts[k]] = 1;
            }
        }
    }
    const int nBad = __syncthreads_count(bad ? 1 : 0);
    if (nBad > 0 && threadIdx.x == 0) atomicAdd(&d->badNow, nBad);
}

// One wave; lane 0 writes everything, in plain C++.  rec: the iteration's slot of the call's record slab (zeroed by the call).
__global__ void __launch_bounds__(64) k_tangle_verdict(TangleDev* __restrict__ d, smgpu_tangle_record* __restrict__ rec, long long number, int pass,
                                                        int passes, const smgpu_iter_stats* gate) {
    if (threadIdx.x != 0) return;
    if (!qTraceRan(gate) || (pass > 0 && d->clean)) return;
    const int nBad = d->badNow;
    d->badNow = 0;
    if (pass == 0) {
        smgpu_tangle_record r;
        r.iteration = number; r.passes = 0; r.fullRevert = 0; r.nBadCells = nBad; r.nPointsReverted = 0;
        *rec = r;
    }
    if (nBad == 0) { d->clean = 1; d->full = 0; return; }
    d->clean = 0;
    if (pass == passes) { d->full = 1; rec->fullRevert = 1; }
    else { d->full = 0; rec->passes += 1; }
}

// A workgroup takes kTanglePts consecutive points; marks: nPoints rounded up to a multiple of 4 bytes, zero past the end.
// Marked mode: the first kTanglePts / 4 lanes read one word of four mark bytes each, and a lane whose word is zero reads nothing
// else; a marked point whose coordinates differ goes back to x.  Full revert: a streaming copy in the style of
// k_quality_guard_snapshot -- 16 bytes per lane per access, consecutive lanes consecutive addresses, every load issued before the
// first store (the workgroup's points are 3 * kTangleBlock double2 of each array, 16-byte aligned: whole allocations) -- that
// also leaves one "differs" byte per double in LDS, from which every lane then counts two points.  The last, partial workgroup
// goes point by point.  nPointsReverted takes the points that changed, one integer atomic per workgroup.
constexpr int kTanglePts = 2 * kTangleBlock;
__global__ void __launch_bounds__(kTangleBlock) k_tangle_apply(const double* __restrict__ x, double* __restrict__ xNew, uint8_t* __restrict__ marks,
                                                                int nPoints, const TangleDev* __restrict__ d, smgpu_tangle_record* __restrict__ rec,
                                                                const smgpu_iter_stats* gate) {
    if (!qTraceRan(gate) || d->clean) return;
    __shared__ uint8_t differs[6 * kTangleBlock];
    const bool full = d->full != 0;
    const int tid = threadIdx.x;
    const long long first = (long long)blockIdx.x * kTanglePts;
    const bool stream = full && first + kTanglePts <= nPoints;
    int changed = 0;
    if (stream) {
        const double2* __restrict__ sp = reinterpret_cast<const double2*>(x + 3 * first);
        double2* __restrict__ dp = reinterpret_cast<double2*>(xNew + 3 * first);
        const double2 a0 = sp[tid], a1 = sp[tid + kTangleBlock], a2 = sp[tid + 2 * kTangleBlock];
        const double2 b0 = dp[tid], b1 = dp[tid + kTangleBlock], b2 = dp[tid + 2 * kTangleBlock];
        dp[tid] = a0; dp[tid + kTangleBlock] = a1; dp[tid + 2 * kTangleBlock] = a2;
        differs[2 * tid] = a0.x != b0.x; differs[2 * tid + 1] = a0.y != b0.y;
        differs[2 * (tid + kTangleBlock)] = a1.x != b1.x; differs[2 * (tid + kTangleBlock) + 1] = a1.y != b1.y;
        differs[2 * (tid + 2 * kTangleBlock)] = a2.x != b2.x; differs[2 * (tid + 2 * kTangleBlock) + 1] = a2.y != b2.y;
        __syncthreads();
        changed = ((differs[3 * tid] | differs[3 * tid + 1] | differs[3 * tid + 2]) ? 1 : 0) +
                  ((differs[3 * (tid + kTangleBlock)] | differs[3 * (tid + kTangleBlock) + 1] | differs[3 * (tid + kTangleBlock) + 2]) ? 1 : 0);
    }
    const long long p0 = first + 4 * tid;
    if (tid < kTanglePts / 4 && p0 < nPoints) {
        unsigned* const mw = reinterpret_cast<unsigned*>(marks) + (p0 >> 2);
        const unsigned w = *mw;
        if (!stream && (full || w)) {
            for (int j = 0; j < 4; ++j) {
                const long long p = p0 + j;
                if (p >= nPoints || !(full || ((w >> (8 * j)) & 0xffu))) continue;
                const V3 a = ldv(x, p), b = ldv(xNew, p);
                if (a.x != b.x || a.y != b.y || a.z != b.z) { stv(xNew, p, a); ++changed; }
            }
        }
        if (w) *mw = 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) changed += __shfl_xor(changed, o, 64);
    __shared__ int waveChanged[kTangleBlock / 64];
    if ((tid & 63) == 0) waveChanged[tid >> 6] = changed;
    __syncthreads();
    if (tid == 0) {
        int sum = 0;
        for (int w = 0; w < kTangleBlock / 64; ++w) sum += waveChanged[w];
        if (sum > 0) atomicAdd(reinterpret_cast<unsigned long long*>(&rec->nPointsReverted), (unsigned long long)sum);
    }
}

// ---- the coupled form (smgpu_set_tangle_constraint_coupled, DESIGN.md "Mesh quality", 10.13): a sub-domain of a decomposed mesh ----
// The evaluation is the one above, ungated (gate = NULL, pass = 0).  The verdict is the host's, on the count summed over the ranks,
// so nothing here reads TangleDev::clean or ::full: the pass and its kind arrive as kernel arguments.

// Exchange T, pack: one lane per send slot, slot -> shared index -> local point -> mark byte, as an int32 (k_halo_packF's shape:
// consecutive lanes read consecutive sendShared entries and store consecutive sendT words).
__global__ void __launch_bounds__(kTangleBlock) k_tangle_pack(int nSend, const int* __restrict__ sendShared, const int* __restrict__ sharedLocal,
                                                               const uint8_t* __restrict__ marks, int* __restrict__ sendT) {
    const int i = blockIdx.x * kTangleBlock + threadIdx.x;
    if (i < nSend) sendT[i] = marks[sharedLocal[sendShared[i]]] ? 1 : 0;
}

// Exchange T, combine: one lane per shared point ORs the other sharers' marks into its own (k_halo_orF's shape).
__global__ void __launch_bounds__(kTangleBlock) k_tangle_combine(int nShared, const int* __restrict__ sharedLocal, const int* __restrict__ combOff,
                                                                  const int* __restrict__ combSlots, const int* __restrict__ recvT,
                                                                  uint8_t* __restrict__ marks) {
    const int i = blockIdx.x * kTangleBlock + threadIdx.x;
    if (i >= nShared) return;
    int any = 0;
    for (int k = combOff[i]; k < combOff[i + 1]; ++k) {
        const int sl = combSlots[k];
        if (sl >= 0) any |= recvT[sl];
    }
    if (any) marks[sharedLocal[i]] = 1;
}

// The revert of the coupled form.  Every lane takes the four points of one word of marks (marks: as k_tangle_apply's), a lane
// whose word is zero reads nothing else unless `full`; a point that goes back and whose coordinates differ is restored from x.
// The revert itself is the same on every rank that holds the point; nPointsReverted takes a shared point on its master only:
// sharedSlot[p] >= 0 names the point's entry of `counted` (one byte per shared point, 0 where a lower rank shares it).
constexpr int kTangleCountedPts = 4 * kTangleBlock;
__global__ void __launch_bounds__(kTangleBlock) k_tangle_apply_counted(const double* __restrict__ x, double* __restrict__ xNew, uint8_t* __restrict__ marks,
                                                                        int nPoints, int full, const int* __restrict__ sharedSlot,
                                                                        const uint8_t* __restrict__ counted, smgpu_tangle_record* __restrict__ rec) {
    const int tid = threadIdx.x;
    const long long p0 = ((long long)blockIdx.x * kTangleBlock + tid) * 4;
    int changed = 0;
    if (p0 < nPoints) {
        unsigned* const mw = reinterpret_cast<unsigned*>(marks) + (p0 >> 2);
        const unsigned w = *mw;
        if (full || w) {
            for (int j = 0; j < 4; ++j) {
                const long long p = p0 + j;
                if (p >= nPoints || !(full || ((w >> (8 * j)) & 0xffu))) continue;
                const V3 a = ldv(x, p), b = ldv(xNew, p);
                if (a.x != b.x || a.y != b.y || a.z != b.z) {
                    stv(xNew, p, a);
                    const int sl = sharedSlot ? sharedSlot[p] : -1;
                    if (sl < 0 || counted[sl]) ++changed;
                }
            }
        }
        if (w) *mw = 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) changed += __shfl_xor(changed, o, 64);
    __shared__ int waveChanged[kTangleBlock / 64];
    if ((tid & 63) == 0) waveChanged[tid >> 6] = changed;
    __syncthreads();
    if (tid == 0) {
        int sum = 0;
        for (int w = 0; w < kTangleBlock / 64; ++w) sum += waveChanged[w];
        if (sum > 0) atomicAdd(reinterpret_cast<unsigned long long*>(&rec->nPointsReverted), (unsigned long long)sum);
    }
}

// Closes the record of an iteration from the host's verdict; one wave, lane 0 writes every word in plain C++ (nPointsReverted is
// the applies': the slot was zeroed before the iteration's first pass).
__global__ void __launch_bounds__(64) k_tangle_close(smgpu_tangle_record* __restrict__ rec, long long number, int passes, int fullRevert, long long nBadCells) {
    if (threadIdx.x != 0) return;
    rec->iteration = number;
    rec->passes = passes;
    rec->fullRevert = fullRevert;
    rec->nBadCells = nBadCells;
}

}  // namespace smgpu
