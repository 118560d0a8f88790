// kernels_quality_constraint.hpp -- the quality constraint (smgpu_set_quality_constraint: include/smgpu.h, DESIGN.md "Mesh quality",
// 10.14): the tangle constraint (kernels_quality_tangle.hpp) with up to three more criteria -- a face's non-orthogonality and its
// skewness against limits of meshQualityDict.  A cell is bad when 10.12 says so or when it is the owner or the neighbour of a bad
// face that is not exempt; the points of its faces go back to where the iteration found them.
//
// Per iteration the engine queues, on its own stream and in front of the trace's launches, for k = 0 .. passes
//   1. k_qc_tile: the geometry tile of the new points with writeFaces (k_quality_geom_tile's phases): C_f, S_f by face id into
//      fCtr / fArea, which no kernel of the tiled loop reads, C_c by cell id into a buffer of the constraint's own, and 10.12's
//      verdict on every cell of the tile that is not exempt (tangleTileCell of kernels_quality_tangle.hpp) as a byte per cell;
//   2. k_qc_faces: one lane per face in polyMesh order: ortho_f and skew_f with k_quality_faces' operands and operation order, the
//      limits and the exempt byte; a bad face stores a byte into the flags of its owner and its neighbour (plain stores of the same
//      value) and counts, one integer atomic per workgroup and criterion;
//   3. k_qc_cells: one lane per cell: the byte of step 1, the flag of step 2 (cleared here), the marks of the points of a bad
//      cell's faces by k_tangle_cells' loop, |B| and the tangled cells, one integer atomic per workgroup each;
//   4. k_qc_verdict: k_tangle_verdict's twin with the wider record, the wider device words and the stop word;
//   5. k_tangle_apply itself: the record and the device words begin with the tangle constraint's (static_asserts below).
// Without tiles (SMGPU_TILES=0) step 1 is k_qc_open + k_face_geom + k_cell_centres on the constraint's cell centres and stop
// word (set while the iteration did not run or a pass was clean), and k_qc_cells forms 10.12's verdict itself with k_tangle_cells'
// arithmetic: identical points and records.
// No float atomics; every store is a plain vector store; every kernel takes the trace's gate (qTraceRan) and the clean word.
// With a limit of 10.16 on (smgpu_set_quality_constraint_limits) kernels_quality_limits.hpp puts a cell pass in front of step 2
// and its own face kernel in the place of step 2; with none on the sequence is the one above.
//
// The coupled form (smgpu_set_quality_constraint_coupled, DESIGN.md "Mesh quality", 10.15 and 10.17): a sub-domain of a decomposed
// mesh.  The kernels are the ones above, instantiated with Coupled = true where a processor face changes a line, and ungated
// (gate = NULL, pass = 0): step 1, then k_quality_pack of the constraint's own cell centres; the host moves them; then
// k_qc_faces<true>, k_qc_cells, k_tangle_pack.  The verdict is the host's, on the count summed over the ranks, as in 10.13:
// k_tangle_combine, k_tangle_apply_counted, k_qc_close.
#pragma once
#include <cstddef>

#include "kernels_quality_tangle.hpp"

namespace smgpu {

// t first: k_tangle_apply reads clean and full through a TangleDev*
struct QcDev {
    TangleDev t;       // clean, full, badNow (|B| of the evaluation in flight), err (unused: no tile holds the marks)
    int tangledNow;    // cells bad by 10.12's definition alone, not exempt
    int nonOrthoNow;   // bad faces, not exempt, by the non-orthogonality limit
    int skewNow;       // ... by a skewness limit
    int facesNow;      // bad faces by any limit (enabling: the exempt faces)
    // 10.16 (kernels_quality_limits.hpp): bad faces, not exempt, by tet quality, twist, triangle twist, weight, volume ratio; cells
    // under the determinant limit, not determinant-exempt (enabling: the determinant-exempt cells).  0 while none of them is on
    int lowTetNow, lowTwistNow, lowTriNow, lowWeightNow, lowRatioNow, underDetNow;
    // 10.18: bad faces, not exempt, by concavity, flatness, area; cells under the volume limit, not volume-exempt (enabling: the
    // volume-exempt cells).  0 while none of them is on
    int concaveNow, warpedNow, smallAreaNow, smallVolNow;
};
static_assert(offsetof(QcDev, t) == 0, "k_tangle_apply takes a QcDev as its TangleDev");
static_assert(offsetof(smgpu_quality_constraint_record, iteration) == offsetof(smgpu_tangle_record, iteration) &&
              offsetof(smgpu_quality_constraint_record, passes) == offsetof(smgpu_tangle_record, passes) &&
              offsetof(smgpu_quality_constraint_record, fullRevert) == offsetof(smgpu_tangle_record, fullRevert) &&
              offsetof(smgpu_quality_constraint_record, nBadCells) == offsetof(smgpu_tangle_record, nBadCells) &&
              offsetof(smgpu_quality_constraint_record, nPointsReverted) == offsetof(smgpu_tangle_record, nPointsReverted),
              "k_tangle_apply adds nPointsReverted through a smgpu_tangle_record*");

static_assert(offsetof(smgpu_quality_constraint_record_full, nSkewFaces) == offsetof(smgpu_quality_constraint_record, nSkewFaces) &&
              offsetof(smgpu_quality_constraint_record_full, nLowTetFaces) == sizeof(smgpu_quality_constraint_record),
              "the narrow record is the head of the full one: smgpu_get_quality_constraint_records copies it out of the full slots");
static_assert(offsetof(smgpu_quality_constraint_record_all, nUnderdeterminedCells) == offsetof(smgpu_quality_constraint_record_full, nUnderdeterminedCells) &&
              offsetof(smgpu_quality_constraint_record_all, nConcaveFaces) == sizeof(smgpu_quality_constraint_record_full),
              "the full record is the head of the widest one, which the slab holds: the narrower getters copy their prefix");

// the limits as the kernels test them; a criterion that is off never fires
struct QcLimits { double cosT, maxInternalSkew, maxBoundarySkew; int nonOrthoOn, internalSkewOn, boundarySkewOn; };

// What a sub-domain changes for a face kernel (QCoupling<true>, kernels_quality.hpp: 10.4's slot table, decoded as qNeighbour
// decodes it, and the neighbour rank's cell centres and volumes in patch order).  qcSlot: -1 for an internal or a physical
// boundary face, else the processor face's place in recvCc / recvVc, | kQualityNotCounted on the side with myRank > neighbRank.
// Serial, it is the constant -1, and what the kernels derive from it folds to the serial lines: `internal` (an internal face of
// the global mesh) is `inner` (both cells are this rank's), every face is counted.
template <bool Coupled>
__device__ __forceinline__ int qcSlot(const MeshView& m, const QCoupling<Coupled>& cp, int f) {
    if constexpr (Coupled) return f < m.nInternalFaces ? -1 : cp.slot[f - m.nInternalFaces];
    else return -1;
}
// C_N of face f, valid where the face is internal to the global mesh: the neighbour cell's, or across a processor face recvCc's
template <bool Coupled>
__device__ __forceinline__ V3 qcNeighbourCentre(const double* __restrict__ cellCtr, const QCoupling<Coupled>& cp, bool inner, int n, int sl) {
    if constexpr (Coupled) return inner ? ldv(cellCtr, n) : (sl >= 0 ? ldv(cp.recvCc, sl & kQualitySlotMask) : v3(0, 0, 0));
    else return inner ? ldv(cellCtr, n) : v3(0, 0, 0);
}

// The geometry tile of s.ptsCur with writeFaces and the cell centres (s.cellCtr: the constraint's own buffer) -- the body of
// k_quality_geom_tile (kernels_quality_trace.hpp) up to geomCell: no stop word of the loop, no deferred finish, wantAvg = 0 -- then
// 10.12's verdict on the thread's cell from the face records in LDS.  tangled[c]: the verdict of a cell that is not exempt.
// exemptOut != NULL (enabling): every cell's verdict goes to exemptOut[c] instead and badNow counts the exempt cells.
template <int T, bool ORG>
__global__ void __launch_bounds__(T) __attribute__((amdgpu_waves_per_eu(4))) k_qc_tile(MeshView m, State s, GeomTileView g, int nLaunch, int xcdMap,
                                                                             const uint8_t* __restrict__ exempt, uint8_t* __restrict__ exemptOut,
                                                                             uint8_t* __restrict__ tangled, QcDev* __restrict__ d, int pass,
                                                                             const smgpu_iter_stats* gate) {
    if (!qTraceRan(gate) || (pass > 0 && d->t.clean)) return;
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
    geomFaces<T, ORG>(s, g, L, tm, r, tid, 0, 1);
    __syncthreads();
    geomCell<T, ORG>(s, g, L, tm, tid, (unsigned)tm.flags, r.cin);
    bool bad = false;
    if (r.cin.mine) {
        bad = tangleTileCell<T, ORG>(g, L, tm, tid, (unsigned)tm.flags, r.cin);
        if (exemptOut) exemptOut[r.cin.c] = bad ? 1 : 0;
        else {
            bad = bad && !exempt[r.cin.c];
            tangled[r.cin.c] = bad ? 1 : 0;
        }
    }
    if (!exemptOut) return;
    const int nBad = __syncthreads_count(bad ? 1 : 0);
    if (nBad > 0 && tid == 0) atomicAdd(&d->t.badNow, nBad);
}

// One wave, lane 0, plain C++: the stop word of the constraint's geometry launches for pass 0 -- set when the iteration did not run
__global__ void __launch_bounds__(64) k_qc_open(Accum* __restrict__ acc, const smgpu_iter_stats* gate) {
    if (threadIdx.x != 0) return;
    acc->stop = qTraceRan(gate) ? 0 : 1;
}

// ortho_f (internal faces) and skew_f of face f: qFaceCore's lines (kernels_quality.hpp), nothing else of it -- keep them alike
__device__ __forceinline__ void qcFace(const MeshView& m, const double* __restrict__ pts, const V3 Cf, const V3 Sf, const V3 CO, bool internal, const V3 CN,
                                       int f, double& ortho, double& skew) {
    const double magSf = mag(Sf);
    const V3 Cpf = Cf - CO;
    V3 d;
    ortho = 1.0;
    if (internal) {
        d = CN - CO;
        ortho = dot(d, Sf) / (mag(d) * magSf + SMGPU_VSMALL);
    } else {
        const V3 n = Sf / (magSf + SMGPU_ROOTVSMALL);
        d = dot(n, Cpf) * n;
    }
    const V3 sv = Cpf - (dot(Sf, Cpf) / (dot(Sf, d) + SMGPU_ROOTVSMALL)) * d;
    const double magSv = mag(sv);
    const V3 sHat = sv / (magSv + SMGPU_ROOTVSMALL);
    double fd = 0.2 * mag(d) + SMGPU_ROOTVSMALL;
    for (int j = m.faceOff[f]; j < m.faceOff[f + 1]; ++j) fd = fmax(fd, fabs(dot(sHat, ldv(pts, m.facePts[j]) - Cf)));
    skew = magSv / fd;
}

// exemptOut != NULL (enabling): every face's verdict goes to exemptOut[f], no cell is flagged, facesNow counts the exempt faces.
// Coupled: a processor face is an internal face of the global mesh: qcFace with internal = true and C_N from recvCc, the two
// internal limits, the flag on its owner (the neighbour cell is the other rank's, which judges the face itself), and the counts
// only on the counted side.  Lanes of internal and physical faces take the serial path.
constexpr int kQcBlock = 256;
template <bool Coupled>
__global__ void __launch_bounds__(kQcBlock) k_qc_faces(MeshView m, const double* __restrict__ pts, const double* __restrict__ fCtr,
                                                        const double* __restrict__ fArea, const double* __restrict__ cellCtr,
                                                        const int* __restrict__ own, const int* __restrict__ nei, QCoupling<Coupled> cp, QcLimits lim,
                                                        const uint8_t* __restrict__ exempt, uint8_t* __restrict__ exemptOut,
                                                        uint8_t* __restrict__ cellFlag, QcDev* __restrict__ d, int pass, const smgpu_iter_stats* gate) {
    if (!qTraceRan(gate) || (pass > 0 && d->t.clean)) return;
    const int f = blockIdx.x * kQcBlock + threadIdx.x;
    bool badNO = false, badSk = false, counted = true;
    if (f < m.nFaces) {
        const bool inner = f < m.nInternalFaces;
        const int sl = qcSlot(m, cp, f);
        const bool internal = inner || sl >= 0;
        const int o = own[f], n = inner ? nei[f] : 0;
        counted = sl < 0 || !(sl & kQualityNotCounted);
        double ortho, skew;
        qcFace(m, pts, ldv(fCtr, f), ldv(fArea, f), ldv(cellCtr, o), internal, qcNeighbourCentre(cellCtr, cp, inner, n, sl), f, ortho, skew);
        badNO = internal && lim.nonOrthoOn && ortho < lim.cosT;
        badSk = internal ? (lim.internalSkewOn && skew > lim.maxInternalSkew) : (lim.boundarySkewOn && skew > lim.maxBoundarySkew);
        if (exemptOut) exemptOut[f] = (badNO || badSk) ? 1 : 0;
        else if (exempt[f]) badNO = badSk = false;
        if ((badNO || badSk) && !exemptOut) {
            cellFlag[o] = 1;
            if (inner) cellFlag[n] = 1;
        }
    }
    const int nNO = __syncthreads_count((badNO && counted) ? 1 : 0), nSk = __syncthreads_count((badSk && counted) ? 1 : 0),
              nAny = __syncthreads_count(((badNO || badSk) && counted) ? 1 : 0);
    if (threadIdx.x == 0) {
        if (nNO > 0) atomicAdd(&d->nonOrthoNow, nNO);
        if (nSk > 0) atomicAdd(&d->skewNow, nSk);
        if (nAny > 0) atomicAdd(&d->facesNow, nAny);
    }
}

// One lane per cell: bad = 10.12's verdict of a cell that is not exempt, or a flag from k_qc_faces -- an exempt cell too is bad
// through a bad face that is not.  Verdict = false (tiles): the verdict is k_qc_tile's byte.  Verdict = true (without tiles): it
// is formed here from the values k_face_geom / k_cell_centres left by id, with k_tangle_cells' arithmetic line for line (keep
// them alike); exemptOut != NULL (enabling): it goes to exemptOut[c], nothing is marked, badNow counts the exempt cells.
template <bool Verdict>
__global__ void __launch_bounds__(kQcBlock) k_qc_cells(MeshView m, const double* __restrict__ fCtr, const double* __restrict__ fArea,
                                                        const double* __restrict__ cellCtr, const uint8_t* __restrict__ exempt,
                                                        uint8_t* __restrict__ exemptOut, const uint8_t* __restrict__ tangledIn,
                                                        uint8_t* __restrict__ cellFlag, uint8_t* __restrict__ marks, QcDev* __restrict__ d, int pass,
                                                        const smgpu_iter_stats* gate) {
    if (!qTraceRan(gate) || (pass > 0 && d->t.clean)) return;
    const int c = blockIdx.x * kQcBlock + threadIdx.x;
    bool tangled = false, bad = false;
    if (c < m.nCells) {
        const int b = m.cfOff[c], e = m.cfOff[c + 1];
        if constexpr (Verdict) {
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
                const double ownSide = (ev < 0) ? dot(Sf, ctr - Cf) : dot(Sf, Cf - ctr);
                tangled = tangled || ownSide <= 0.0;
            }
            tangled = tangled || (1.0 / 3.0) * pyr <= SMGPU_VSMALL;
        } else {
            tangled = tangledIn[c] != 0;
        }
        if (Verdict && exemptOut) {
            exemptOut[c] = tangled ? 1 : 0;
            bad = tangled;
        } else {
            if (Verdict) tangled = tangled && !exempt[c];
            const bool flagged = cellFlag[c] != 0;
            if (flagged) cellFlag[c] = 0;
            bad = tangled || flagged;
            if (bad) {
                for (int j = b; j < e; ++j) {
                    const int f = m.cfVal[j] & 0x7fffffff;
                    for (int k = m.faceOff[f]; k < m.faceOff[f + 1]; ++k) marks[m.facePts[k]] = 1;
                }
            }
        }
    }
    const int nBad = __syncthreads_count(bad ? 1 : 0), nTangled = __syncthreads_count(tangled ? 1 : 0);
    if (threadIdx.x == 0) {
        if (nBad > 0) atomicAdd(&d->t.badNow, nBad);
        if (nTangled > 0) atomicAdd(&d->tangledNow, nTangled);
    }
}

// k_tangle_verdict's twin: one wave, lane 0 writes everything in plain C++.  It also keeps the stop word of the next pass's
// geometry launch.  rec: the iteration's slot of the call's record slab (zeroed by the call).  The six words of 10.16 are 0 while
// none of its limits is on, and so are the record's six counts; likewise the four of 10.18.
__global__ void __launch_bounds__(64) k_qc_verdict(QcDev* __restrict__ d, Accum* __restrict__ acc, smgpu_quality_constraint_record_all* __restrict__ rec,
                                                    long long number, int pass, int passes, const smgpu_iter_stats* gate) {
    if (threadIdx.x != 0) return;
    if (!qTraceRan(gate) || (pass > 0 && d->t.clean)) return;
    const int nBad = d->t.badNow, nTangled = d->tangledNow, nNO = d->nonOrthoNow, nSk = d->skewNow;
    const int nTet = d->lowTetNow, nTw = d->lowTwistNow, nTri = d->lowTriNow, nW = d->lowWeightNow, nR = d->lowRatioNow, nDet = d->underDetNow;
    d->t.badNow = 0; d->tangledNow = 0; d->nonOrthoNow = 0; d->skewNow = 0; d->facesNow = 0;
    const int nConc = d->concaveNow, nWarp = d->warpedNow, nArea = d->smallAreaNow, nVol = d->smallVolNow;
    d->lowTetNow = 0; d->lowTwistNow = 0; d->lowTriNow = 0; d->lowWeightNow = 0; d->lowRatioNow = 0; d->underDetNow = 0;
    d->concaveNow = 0; d->warpedNow = 0; d->smallAreaNow = 0; d->smallVolNow = 0;
    if (pass == 0) {
        smgpu_quality_constraint_record_all r;
        r.iteration = number; r.passes = 0; r.fullRevert = 0; r.nBadCells = nBad; r.nPointsReverted = 0;
        r.nTangledCells = nTangled; r.nNonOrthoFaces = nNO; r.nSkewFaces = nSk;
        r.nLowTetFaces = nTet; r.nLowTwistFaces = nTw; r.nLowTriangleTwistFaces = nTri; r.nLowWeightFaces = nW; r.nLowVolRatioFaces = nR;
        r.nUnderdeterminedCells = nDet;
        r.nConcaveFaces = nConc; r.nWarpedFaces = nWarp; r.nSmallAreaFaces = nArea; r.nSmallVolumeCells = nVol;
        *rec = r;
    }
    if (nBad == 0) { d->t.clean = 1; d->t.full = 0; acc->stop = 1; return; }
    d->t.clean = 0;
    if (pass == passes) { d->t.full = 1; rec->fullRevert = 1; }
    else { d->t.full = 0; rec->passes += 1; }
}

// k_tangle_close's twin: closes the record of an iteration of the coupled form from the host's verdict.  n: the rank's fourteen counts
// at k = 0 in the record's order from nBadCells on, without nPointsReverted (the applies': the slot was zeroed before the
// iteration's first pass).  One wave, lane 0 writes every word in plain C++.
struct QcCounts { long long n[14]; };
__global__ void __launch_bounds__(64) k_qc_close(smgpu_quality_constraint_record_all* __restrict__ rec, long long number, int passes, int fullRevert,
                                                  QcCounts c) {
    if (threadIdx.x != 0) return;
    rec->iteration = number;
    rec->passes = passes;
    rec->fullRevert = fullRevert;
    rec->nBadCells = c.n[0];
    rec->nTangledCells = c.n[1];
    rec->nNonOrthoFaces = c.n[2];
    rec->nSkewFaces = c.n[3];
    rec->nLowTetFaces = c.n[4];
    rec->nLowTwistFaces = c.n[5];
    rec->nLowTriangleTwistFaces = c.n[6];
    rec->nLowWeightFaces = c.n[7];
    rec->nLowVolRatioFaces = c.n[8];
    rec->nUnderdeterminedCells = c.n[9];
    rec->nConcaveFaces = c.n[10];
    rec->nWarpedFaces = c.n[11];
    rec->nSmallAreaFaces = c.n[12];
    rec->nSmallVolumeCells = c.n[13];
}

}  // namespace smgpu
