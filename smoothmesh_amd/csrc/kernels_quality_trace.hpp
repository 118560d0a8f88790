// kernels_quality_trace.hpp -- the quality history of a run (smgpu_set_quality_trace / smgpu_get_quality_trace: include/smgpu.h,
// DESIGN.md "Mesh quality", 10.10).
//
// After every interval-th iteration of smgpu_iterate the engine queues, behind that iteration's movePoints and on its own stream,
//   1. k_quality_geom_tile: the geometry tile of the new points (the phases of k_geom_tile with writeFaces) and, on the face
//      records the tile holds in LDS, the cell measures of the report's cell pass -- one QCell partial per tile;
//   2. k_quality_faces<false>: the report's own face pass, unchanged;
//   3. k_quality_trace_fold: the tile partials, 2048 per workgroup;
//   4. k_quality_trace_final: one workgroup folds both slabs into slot r of the call's record slab.
// A record holds only minima, maxima (ties to the lowest id) and counts: any fold order gives the same record, and every field
// has the bits smgpu_mesh_quality gives for the same points.  With SMGPU_TILES=0 or SMGPU_QUALITY_TRACE_FUSED=0 step 1 is the
// report's geometry launch and cell pass and step 3 falls away.
//
// gate: with relTol > 0 the iterations queued behind the stop are no-ops, but the host has swapped the point buffers for them all
// the same.  k_finish runs in every iteration then and has written stats[i] before the trace of iteration i starts: the kernels
// of this file test its written bit and leave everything as it is when the iteration did not run.  gate == NULL (relTol <= 0:
// nothing can stop the loop, and stats[i] may be written late by the deferred finish): no test.
#pragma once
#include "kernels_quality.hpp"
#include "kernels_tiled.hpp"

namespace smgpu {

__device__ __forceinline__ bool qTraceRan(const smgpu_iter_stats* gate) { return !gate || (gate->nNearTies & kStatsWritten) != 0; }

// the tail of qCellOne: the record of a cell from its volume, the signed sum and the sum of magnitudes of its area vectors
__device__ __forceinline__ void qTileCellRecord(const QualityThresholds& thr, int c, double V, const V3& sumS, const V3& M, QCell& a) {
    const double open = fmax(fmax(fabs(sumS.x) / (M.x + SMGPU_ROOTVSMALL), fabs(sumS.y) / (M.y + SMGPU_ROOTVSMALL)),
                             fabs(sumS.z) / (M.z + SMGPU_ROOTVSMALL));
    const double maxM = fmax(fmax(M.x, M.y), M.z), minM = fmin(fmin(M.x, M.y), M.z);
    const double ar = fmax(maxM / (minM + SMGPU_ROOTVSMALL),
                           ((1.0 / 6.0) * ((M.x + M.y) + M.z)) / pow(fmax(V, SMGPU_ROOTVSMALL), 2.0 / 3.0));
    a.minV = V; a.minVId = c; a.maxV = V; a.sumV = V;
    a.nNonPos = (V <= SMGPU_VSMALL) ? 1 : 0;
    a.maxOpen = open; a.nOpen = (open > thr.closed) ? 1 : 0;
    a.maxAR = ar; a.nHigh = (ar > thr.aspect) ? 1 : 0;
}

// qCellVolume / qCellOne (kernels_quality.hpp) of the thread's cell on the tile's face records in LDS.  The cell's row holds its
// faces in cfVal order (bit 15: the cell is the face's neighbour), and a record in LDS has the bits the tile publishes by face id,
// so every operation below meets the operands of the cell pass in its order: the mean of the face centres by a plain division,
// the signed pyramids without a vSmall clamp under either foam variant, each sum its own chain.  A body of its own, not a
// template shared with qCellOne: the report's kernels stay the code they were (tests/test_gpu_quality_trace.py holds the two
// to the same bits).  tflags bit1: every cell of the tile has six faces (the row is in registers: GeomCellIn).
template <int T>
__device__ __forceinline__ void qTileCell(const GeomTileView& g, const GeomLds& L, const GeomTileMeta& tm, int tid, unsigned tflags, const GeomCellIn& in,
                                          const QualityThresholds& thr, QCell& a) {
    const double *fcx = L.fcx, *fcy = L.fcy, *fcz = L.fcz, *fax = L.fax, *fay = L.fay, *faz = L.faz;
    V3 cEst = v3(0, 0, 0), sumS = v3(0, 0, 0), M = v3(0, 0, 0);
    double pyr = 0.0;
#define SMGPU_QPYR(E, FC)                                                      \
    {                                                                          \
        const V3 Sf = ldsg(fax, fay, faz, kGF * ((E) & 0x7fff));               \
        double p = dot(Sf, (FC) - cEst);                                       \
        if ((E) & 0x8000) { p = -p; sumS = sumS - Sf; }                        \
        else sumS = sumS + Sf;                                                 \
        M = M + v3(fabs(Sf.x), fabs(Sf.y), fabs(Sf.z));                        \
        pyr += p;                                                              \
    }
    if ((tflags & 2u)) {
        const ushort4 qa = in.qa, qb = in.qb;
        const unsigned e0 = qa.x, e1 = qa.y, e2 = qa.z, e3 = qa.w, e4 = qb.x, e5 = qb.y;
        const V3 c0 = ldsg(fcx, fcy, fcz, kGF * (e0 & 0x7fff)), c1 = ldsg(fcx, fcy, fcz, kGF * (e1 & 0x7fff)), c2 = ldsg(fcx, fcy, fcz, kGF * (e2 & 0x7fff)),
                 c3 = ldsg(fcx, fcy, fcz, kGF * (e3 & 0x7fff)), c4 = ldsg(fcx, fcy, fcz, kGF * (e4 & 0x7fff)), c5 = ldsg(fcx, fcy, fcz, kGF * (e5 & 0x7fff));
        cEst = cEst + c0; cEst = cEst + c1; cEst = cEst + c2; cEst = cEst + c3; cEst = cEst + c4; cEst = cEst + c5;
        cEst = cEst / 6.0;
        SMGPU_QPYR(e0, c0) SMGPU_QPYR(e1, c1) SMGPU_QPYR(e2, c2) SMGPU_QPYR(e3, c3) SMGPU_QPYR(e4, c4) SMGPU_QPYR(e5, c5)
    } else {
        const int cw4 = tm.cfWidth >> 2;
        const ushort4* row = reinterpret_cast<const ushort4*>(g.cellFaces + tm.cfBase) + tid;
        int nFaces = 0;
        SMGPU_ELL_FOREACH(row, cw4, T, {
            cEst = cEst + ldsg(fcx, fcy, fcz, kGF * (e & 0x7fff));
            nFaces = j + 1;
        })
        cEst = cEst / (double)nFaces;
        SMGPU_ELL_FOREACH(row, cw4, T, {
            (void)j;
            const V3 fc = ldsg(fcx, fcy, fcz, kGF * (e & 0x7fff));
            SMGPU_QPYR(e, fc)
        })
    }
#undef SMGPU_QPYR
    qTileCellRecord(thr, in.c, (1.0 / 3.0) * pyr, sumS, M, a);
}

// qBlockReduce for a workgroup of T threads (valid in thread 0)
template <int T>
__device__ __forceinline__ QCell qTileReduce(QCell v, QCell* sh /* [T / 64] in LDS */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const QCell w = qShfl(v, o);
        qCombine(v, w);
    }
    if (T > 64) {
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            v = sh[0];
            for (int w = 1; w < T / 64; ++w) qCombine(v, sh[w]);
        }
    }
    return v;
}

// The geometry tile of s.ptsCur with writeFaces -- the phases of geomTileBody (kernels_tiled.hpp), without the loop's stop word
// and deferred finish, wantAvg = 0 -- then the cell measures on the same LDS contents.  Publishes C_f and S_f by face id
// (s.fCtr / s.fArea) and the cell centres (s.cellCtr: the trace's own buffer) for the face pass; part[tile] takes the tile's record.
// Its own launch bounds: the cell phase needs more registers than k_geom_tile's 96 (figures: DESIGN.md 10.10).
template <int T, bool ORG>
__global__ void __launch_bounds__(T) k_quality_geom_tile(MeshView m, State s, GeomTileView g, int nLaunch, int xcdMap, QualityThresholds thr,
                                                          QCell* __restrict__ part, const smgpu_iter_stats* gate) {
    if (!qTraceRan(gate)) return;
    const int tile = launchTile(nLaunch, xcdMap, (int)blockIdx.x);
    if (tile < 0) return;
    extern __shared__ double lds[];
    __shared__ QCell sh[T / 64];
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
    geomFaces<T, ORG>(s, g, L, tm, r, tid, 0, 1);
    __syncthreads();
    geomCell<T, ORG>(s, g, L, tm, tid, (unsigned)tm.flags, r.cin);
    QCell a = qEmpty<QCell>();
    if (r.cin.mine) qTileCell<T>(g, L, tm, tid, (unsigned)tm.flags, r.cin, thr, a);
    a = qTileReduce<T>(a, sh);
    if (tid == 0) part[tile] = a;
}

// the tile partials, kQualityPer * kQualityBlock per workgroup (one workgroup folding one record per tile of the 10 M-cell mesh
// would take as long as a whole iteration: profiles/quality/README.md)
__global__ void __launch_bounds__(kQualityBlock) k_quality_trace_fold(const QCell* __restrict__ in, int n, QCell* __restrict__ out,
                                                                       const smgpu_iter_stats* gate) {
    if (!qTraceRan(gate)) return;
    qPass(n, out, [&](int i, QCell& e) { e = in[i]; });
}

// k_quality_final for a trace record: the same folds and the same rules for an empty mesh; the sums stay out
__global__ void __launch_bounds__(kQualityBlock) k_quality_trace_final(const QFace* __restrict__ fPart, int nFB, const QCell* __restrict__ cPart, int nCB,
                                                                        int nCells, int nFaces, int nInternalFaces, long long iteration,
                                                                        smgpu_quality_trace_record* __restrict__ out, const smgpu_iter_stats* gate) {
    if (!qTraceRan(gate)) return;
    const QFace a = qFold(fPart, nFB);
    const QCell b = qFold(cPart, nCB);
    if (threadIdx.x != 0) return;
    const bool anyCell = nCells > 0, anyFace = nFaces > 0, anyInternal = nInternalFaces > 0;
    smgpu_quality_trace_record q;
    q.iteration = iteration;
    q.minVolume = anyCell ? b.minV : 0.0; q.maxVolume = anyCell ? b.maxV : 0.0;
    q.nNonPositiveVolume = b.nNonPos; q.minVolumeCell = anyCell ? b.minVId : -1;
    q.minFaceArea = anyFace ? a.minA : 0.0; q.maxFaceArea = anyFace ? a.maxA : 0.0; q.nZeroAreaFaces = a.nZero;
    q.maxNonOrth = anyInternal ? a.maxNO : 0.0;
    q.nSevereNonOrth = a.nSev; q.nErrorNonOrth = a.nErr; q.maxNonOrthFace = anyInternal ? a.maxNOId : -1;
    q.maxSkewness = anyFace ? a.maxSk : 0.0; q.nSkewFaces = a.nSkew; q.maxSkewFace = anyFace ? a.maxSkId : -1;
    q.nWrongOrientedFaces = a.nWrong;
    q.maxOpenness = anyCell ? b.maxOpen : 0.0; q.nOpenCells = b.nOpen;
    q.maxAspectRatio = anyCell ? b.maxAR : 0.0; q.nHighAspectCells = b.nHigh;
    *out = q;
}

}  // namespace smgpu
