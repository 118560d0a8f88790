// kernels_quality_geom.hpp -- the checks `checkMesh -allGeometry` adds to the quality report (smgpu_mesh_quality_geometry /
// smgpu_quality_geometry_field: include/smgpu.h): face concavity, face flatness, face interpolation weight, owner / neighbour
// volume ratio, cell determinant.  Definitions: DESIGN.md "Mesh quality", 10.6.
//
// Same inputs and the same layout as kernels_quality.hpp: face centres / area vectors by face id and cell centres by cell id as
// the loop's geometry launch publishes them, kQualityBlock threads, kQualityPer elements per lane (lane t the elements t, t + 256,
// ...), one partial record per workgroup, one folding workgroup at the end, no float atomics.  The cell pass runs first: it leaves
// the signed cell volumes in a scratch array that the face pass reads by owner / neighbour.  For a sub-domain of a decomposed
// mesh (smgpu_quality_coupled_pack_volumes, smgpu_quality_coupled_geometry_*) the *_coupled kernels run: a
// processor face takes the internal-face branch of weight and volume ratio with C_N (recvCc) and V_N (recvVc) of the neighbour
// rank, a cell's determinant runs over its internal and its processor faces, and the volumes are computed before the exchange, by
// k_quality_cell_volumes.  The cell and the face pass stay a serial / coupled pair each, with their own pass loops: sharing their
// bodies (qPass, qNeighbour, qCellVolume) changed the register allocation and cost 0.6 - 1.5 % of kernel time
// (profiles/quality/README.md), so they are the functions that were measured.  Keep each pair alike.
// The findings as sets (smgpu_quality_geometry_sets / _coupled_geometry_sets): the flag passes at the end of this file.
#pragma once
#include "kernels_quality.hpp"

namespace smgpu {

constexpr double kQualitySmall = 1.0e-15;   // OpenFOAM SMALL

// partial record of the face pass ...
struct QGFace {
    double maxSin, minFlat, sumFlat, minW, sumW, minR, sumR;
    int maxSinId, minFlatId, minWId, minRId;
    long long nConcave, nFlat, nWarped, nLowW, nLowR;
};
// ... and of the cell pass
struct QGCell {
    double minDet, sumDet;
    int minDetId;
    long long nUnder;
};

template <> __device__ __forceinline__ QGFace qEmpty<QGFace>() {
    QGFace a;
    a.maxSin = -__builtin_inf(); a.minFlat = __builtin_inf(); a.minW = __builtin_inf(); a.minR = __builtin_inf();
    a.sumFlat = a.sumW = a.sumR = 0.0;
    a.maxSinId = a.minFlatId = a.minWId = a.minRId = kQualityNoId;
    a.nConcave = a.nFlat = a.nWarped = a.nLowW = a.nLowR = 0;
    return a;
}
template <> __device__ __forceinline__ QGCell qEmpty<QGCell>() {
    QGCell a;
    a.minDet = __builtin_inf(); a.sumDet = 0.0; a.minDetId = kQualityNoId; a.nUnder = 0;
    return a;
}
__device__ __forceinline__ void qCombine(QGFace& a, const QGFace& b) {
    qMaxId(a.maxSin, a.maxSinId, b.maxSin, b.maxSinId);
    qMinId(a.minFlat, a.minFlatId, b.minFlat, b.minFlatId);
    qMinId(a.minW, a.minWId, b.minW, b.minWId);
    qMinId(a.minR, a.minRId, b.minR, b.minRId);
    a.sumFlat += b.sumFlat; a.sumW += b.sumW; a.sumR += b.sumR;
    a.nConcave += b.nConcave; a.nFlat += b.nFlat; a.nWarped += b.nWarped; a.nLowW += b.nLowW; a.nLowR += b.nLowR;
}
__device__ __forceinline__ void qCombine(QGCell& a, const QGCell& b) {
    qMinId(a.minDet, a.minDetId, b.minDet, b.minDetId);
    a.sumDet += b.sumDet;
    a.nUnder += b.nUnder;
}
__device__ __forceinline__ QGFace qShfl(const QGFace& a, int o) {
    QGFace r;
    r.maxSin = __shfl_xor(a.maxSin, o, 64); r.minFlat = __shfl_xor(a.minFlat, o, 64); r.sumFlat = __shfl_xor(a.sumFlat, o, 64);
    r.minW = __shfl_xor(a.minW, o, 64); r.sumW = __shfl_xor(a.sumW, o, 64);
    r.minR = __shfl_xor(a.minR, o, 64); r.sumR = __shfl_xor(a.sumR, o, 64);
    r.maxSinId = __shfl_xor(a.maxSinId, o, 64); r.minFlatId = __shfl_xor(a.minFlatId, o, 64);
    r.minWId = __shfl_xor(a.minWId, o, 64); r.minRId = __shfl_xor(a.minRId, o, 64);
    r.nConcave = __shfl_xor(a.nConcave, o, 64); r.nFlat = __shfl_xor(a.nFlat, o, 64); r.nWarped = __shfl_xor(a.nWarped, o, 64);
    r.nLowW = __shfl_xor(a.nLowW, o, 64); r.nLowR = __shfl_xor(a.nLowR, o, 64);
    return r;
}
__device__ __forceinline__ QGCell qShfl(const QGCell& a, int o) {
    QGCell r;
    r.minDet = __shfl_xor(a.minDet, o, 64); r.sumDet = __shfl_xor(a.sumDet, o, 64);
    r.minDetId = __shfl_xor(a.minDetId, o, 64); r.nUnder = __shfl_xor(a.nUnder, o, 64);
    return r;
}

struct QualityGeomThresholds { double sinConcave, flatness, weight, volRatio, determinant; };

// the signed volume of every cell into vol, before the exchange of a decomposed mesh: for the volume pack and the face pass
__global__ void __launch_bounds__(kQualityBlock) k_quality_cell_volumes(MeshView m, const double* __restrict__ fCtr, const double* __restrict__ fArea,
                                                                         double* __restrict__ vol) {
    qEach(m.nCells, [&](int c) { vol[c] = qCellVolume(m, fCtr, fArea, c, [](bool, int, const V3&) {}); });
}
// the owner cell's volume of every processor face, in patch order (the slot order of k_quality_pack): what the neighbour rank
// needs as its V_N.  Lane i stores sendVc[i]: contiguous stores, gathered loads.
__global__ void __launch_bounds__(kQualityBlock) k_quality_pack_volumes(const int* __restrict__ own, const double* __restrict__ vol,
                                                                         const int* __restrict__ procFace, int nProc, double* __restrict__ sendVc) {
    const int i = blockIdx.x * kQualityBlock + threadIdx.x;
    if (i >= nProc) return;
    sendVc[i] = vol[own[procFace[i]]];
}

// cell pass: signed volume (into vol, for the face pass) and determinant of cell c.  outDet: optional per-cell field.
__device__ __forceinline__ void qgCellOne(const MeshView& m, const double* __restrict__ fCtr, const double* __restrict__ fArea,
                                          const QualityGeomThresholds& thr, int c, QGCell& a, double* __restrict__ vol, double* __restrict__ outDet) {
    const int b = m.cfOff[c], e = m.cfOff[c + 1];
    // V_c: the arithmetic of qCellVolume (kernels_quality.hpp) in the same order, so the same bits, written out here because the
    // injected form compiled to a slower kernel (see the head of this file).  Keep the two alike.
    V3 cEst = v3(0, 0, 0);
    for (int j = b; j < e; ++j) cEst = cEst + ldv(fCtr, m.cfVal[j] & 0x7fffffff);
    cEst = cEst / (double)(e - b);
    double pyr = 0.0, sumA = 0.0;
    int nInt = 0;
    for (int j = b; j < e; ++j) {
        const int ev = m.cfVal[j];
        const int f = ev & 0x7fffffff;
        const V3 Sf = ldv(fArea, f);
        double p = dot(Sf, ldv(fCtr, f) - cEst);
        if (ev < 0) p = -p;
        pyr += p;
        if (f < m.nInternalFaces) { sumA += mag(Sf); ++nInt; }     // (the determinant's mean internal face area, same order)
    }
    vol[c] = (1.0 / 3.0) * pyr;
    // determinant of the cell's internal faces: T = sum (S_f / A)(S_f / A)^T, A = mean |S_f|; det_c = |det T| / 8
    double det = 0.0;
    const double avgA = nInt > 0 ? sumA / (double)nInt : 0.0;
    if (nInt > 0 && avgA >= SMGPU_ROOTVSMALL) {
        double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
        for (int j = b; j < e; ++j) {
            const int f = m.cfVal[j] & 0x7fffffff;
            if (f >= m.nInternalFaces) continue;
            const V3 s = ldv(fArea, f) / avgA;
            xx += s.x * s.x; xy += s.x * s.y; xz += s.x * s.z;
            yy += s.y * s.y; yz += s.y * s.z; zz += s.z * s.z;
        }
        det = fabs((xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz)) + xz * (xy * yz - yy * xz)) / 8.0;
    }
    a.minDet = det; a.minDetId = c; a.sumDet = det;
    a.nUnder = (det < thr.determinant) ? 1 : 0;
    if (outDet) outDet[c] = det;
}
__global__ void __launch_bounds__(kQualityBlock) k_quality_geom_cells(MeshView m, const double* __restrict__ fCtr, const double* __restrict__ fArea,
                                                                       QualityGeomThresholds thr, QGCell* __restrict__ part, double* __restrict__ vol,
                                                                       double* __restrict__ outDet) {
    __shared__ QGCell sh[kQualityBlock / 64];
    QGCell a = qEmpty<QGCell>();
    const int base = blockIdx.x * (kQualityPer * kQualityBlock) + threadIdx.x;
    for (int k = 0; k < kQualityPer; ++k) {
        const int c = base + k * kQualityBlock;
        if (c >= m.nCells) break;
        QGCell e = qEmpty<QGCell>();
        qgCellOne(m, fCtr, fArea, thr, c, e, vol, outDet);
        qCombine(a, e);
    }
    a = qBlockReduce(a, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = a;
}

// the determinant of cell c over its internal and its processor faces.  Twin of the determinant part of qgCellOne
// above: the face test "f < nInternalFaces" widened by "or has a slot >= 0", the sums in the same order
// (without processor faces the same bits).  The volumes are k_quality_cell_volumes'.
__device__ __forceinline__ bool qgcCounts(const MeshView& m, const int* __restrict__ slot, int f) {
    return f < m.nInternalFaces || slot[f - m.nInternalFaces] >= 0;
}
__device__ __forceinline__ void qgCellOneCoupled(const MeshView& m, const double* __restrict__ fArea, const int* __restrict__ slot,
                                                 const QualityGeomThresholds& thr, int c, QGCell& a, double* __restrict__ outDet) {
    const int b = m.cfOff[c], e = m.cfOff[c + 1];
    double sumA = 0.0;
    int nInt = 0;
    for (int j = b; j < e; ++j) {
        const int f = m.cfVal[j] & 0x7fffffff;
        if (qgcCounts(m, slot, f)) { sumA += mag(ldv(fArea, f)); ++nInt; }
    }
    double det = 0.0;
    const double avgA = nInt > 0 ? sumA / (double)nInt : 0.0;
    if (nInt > 0 && avgA >= SMGPU_ROOTVSMALL) {
        double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
        for (int j = b; j < e; ++j) {
            const int f = m.cfVal[j] & 0x7fffffff;
            if (!qgcCounts(m, slot, f)) continue;
            const V3 s = ldv(fArea, f) / avgA;
            xx += s.x * s.x; xy += s.x * s.y; xz += s.x * s.z;
            yy += s.y * s.y; yz += s.y * s.z; zz += s.z * s.z;
        }
        det = fabs((xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz)) + xz * (xy * yz - yy * xz)) / 8.0;
    }
    a.minDet = det; a.minDetId = c; a.sumDet = det;
    a.nUnder = (det < thr.determinant) ? 1 : 0;
    if (outDet) outDet[c] = det;
}
__global__ void __launch_bounds__(kQualityBlock) k_quality_geom_cells_coupled(MeshView m, const double* __restrict__ fArea, const int* __restrict__ slot,
                                                                               QualityGeomThresholds thr, QGCell* __restrict__ part,
                                                                               double* __restrict__ outDet) {
    __shared__ QGCell sh[kQualityBlock / 64];
    QGCell a = qEmpty<QGCell>();
    const int base = blockIdx.x * (kQualityPer * kQualityBlock) + threadIdx.x;
    for (int k = 0; k < kQualityPer; ++k) {
        const int c = base + k * kQualityBlock;
        if (c >= m.nCells) break;
        QGCell e = qEmpty<QGCell>();
        qgCellOneCoupled(m, fArea, slot, thr, c, e, outDet);
        qCombine(a, e);
    }
    a = qBlockReduce(a, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = a;
}

// one corner of a face: unit edges in and out (and whether both raw edges are longer than SMALL); returns the corner's sine where
// the corner is concave, else 0
__device__ __forceinline__ double qgCorner(const V3& ePrev, const V3& eNext, bool both, const V3& nHat, double sinConcave) {
    if (!both) return 0.0;
    const V3 c = cross(ePrev, eNext);
    const double s = mag(c);
    if (s < sinConcave) return 0.0;
    return dot(c / s, nHat) < kQualitySmall ? s : 0.0;
}

// face pass: concavity and flatness in one walk over the face's points (each vertex read once: the previous point and the unit
// edge that ends in the current one are carried), weight and volume ratio of an internal face from the two cell centres and the
// two volumes of the cell pass.  out*: optional per-face fields, NULL for the report.
__device__ __forceinline__ void qgFaceOne(const MeshView& m, const double* __restrict__ pts, const double* __restrict__ fCtr, const double* __restrict__ fArea,
                                          const double* __restrict__ cellCtr, const double* __restrict__ vol, const int* __restrict__ own,
                                          const int* __restrict__ nei, const QualityGeomThresholds& thr, int f, QGFace& a,
                                          double* __restrict__ outConc, double* __restrict__ outFlat, double* __restrict__ outW, double* __restrict__ outR) {
    const V3 Cf = ldv(fCtr, f), Sf = ldv(fArea, f);
    const double magSf = mag(Sf);
    const V3 nHat = Sf / (magSf + SMGPU_ROOTVSMALL);
    const int jb = m.faceOff[f], je = m.faceOff[f + 1];
    double conc = 0.0, area = 0.0;
    if (je - jb >= 2) {
        const V3 p0 = ldv(pts, m.facePts[jb]);
        V3 cur = ldv(pts, m.facePts[jb + 1]);
        V3 eRaw = cur - p0;
        double len = mag(eRaw);
        const V3 eFirst = eRaw / (len + SMGPU_ROOTVSMALL);
        const bool okFirst = len > kQualitySmall;
        area = 0.5 * mag(cross(eRaw, Cf - p0));
        V3 ePrev = eFirst;
        bool okPrev = okFirst;
        for (int j = jb + 1; j < je; ++j) {                      // corner j - jb, edge to the next point (cyclic)
            const V3 nxt = (j + 1 < je) ? ldv(pts, m.facePts[j + 1]) : p0;
            eRaw = nxt - cur;
            len = mag(eRaw);
            const V3 eNext = eRaw / (len + SMGPU_ROOTVSMALL);
            const bool okNext = len > kQualitySmall;
            area += 0.5 * mag(cross(eRaw, Cf - cur));
            conc = fmax(conc, qgCorner(ePrev, eNext, okPrev && okNext, nHat, thr.sinConcave));
            ePrev = eNext; okPrev = okNext; cur = nxt;
        }
        conc = fmax(conc, qgCorner(ePrev, eFirst, okPrev && okFirst, nHat, thr.sinConcave));   // corner 0
    }
    if (conc > kQualitySmall) { a.maxSin = conc; a.maxSinId = f; a.nConcave = 1; }
    double flat = 1.0;
    if (je - jb > 3 && magSf > SMGPU_ROOTVSMALL) {
        flat = magSf / (area + SMGPU_ROOTVSMALL);
        a.minFlat = flat; a.minFlatId = f; a.sumFlat = flat; a.nFlat = 1;
        a.nWarped = (flat < thr.flatness) ? 1 : 0;
    }
    double w = 1.0, r = 1.0;
    if (f < m.nInternalFaces) {
        const int o = own[f], n = nei[f];
        const double dO = fabs(dot(Sf, Cf - ldv(cellCtr, o))), dN = fabs(dot(Sf, ldv(cellCtr, n) - Cf));
        w = fmin(dO, dN) / ((dO + dN) + SMGPU_VSMALL);
        const double vO = vol[o], vN = vol[n];
        r = fmin(vO, vN) / (fmax(vO, vN) + SMGPU_VSMALL);
        a.minW = w; a.minWId = f; a.sumW = w; a.nLowW = (w < thr.weight) ? 1 : 0;
        a.minR = r; a.minRId = f; a.sumR = r; a.nLowR = (r < thr.volRatio) ? 1 : 0;
    }
    if (outConc) outConc[f] = conc;
    if (outFlat) outFlat[f] = flat;
    if (outW) outW[f] = w;
    if (outR) outR[f] = r;
}
__global__ void __launch_bounds__(kQualityBlock) k_quality_geom_faces(MeshView m, const double* __restrict__ pts, const double* __restrict__ fCtr,
                                                                       const double* __restrict__ fArea, const double* __restrict__ cellCtr,
                                                                       const double* __restrict__ vol, const int* __restrict__ own,
                                                                       const int* __restrict__ nei, QualityGeomThresholds thr, QGFace* __restrict__ part,
                                                                       double* __restrict__ outConc, double* __restrict__ outFlat,
                                                                       double* __restrict__ outW, double* __restrict__ outR) {
    __shared__ QGFace sh[kQualityBlock / 64];
    QGFace a = qEmpty<QGFace>();
    const int base = blockIdx.x * (kQualityPer * kQualityBlock) + threadIdx.x;
    for (int k = 0; k < kQualityPer; ++k) {
        const int f = base + k * kQualityBlock;
        if (f >= m.nFaces) break;
        QGFace e = qEmpty<QGFace>();
        qgFaceOne(m, pts, fCtr, fArea, cellCtr, vol, own, nei, thr, f, e, outConc, outFlat, outW, outR);
        qCombine(a, e);
    }
    a = qBlockReduce(a, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = a;
}

// k_quality_geom_faces with processor faces.  qgFaceOne gives every face its concavity and flatness (they read the face's own
// points and C_f only) and the internal faces their weight and volume ratio; a processor face then takes the weight / ratio lines
// of qgFaceOne (their twin, keep alike) with C_N = recvCc[slot], V_N = recvVc[slot], and leaves the record where the other side
// counts it.  Its outW / outR entries, which qgFaceOne set to 1, are written again by the same lane.
__global__ void __launch_bounds__(kQualityBlock) k_quality_geom_faces_coupled(MeshView m, const double* __restrict__ pts, const double* __restrict__ fCtr,
                                                                               const double* __restrict__ fArea, const double* __restrict__ cellCtr,
                                                                               const double* __restrict__ vol, const int* __restrict__ own,
                                                                               const int* __restrict__ nei, const int* __restrict__ slot,
                                                                               const double* __restrict__ recvCc, const double* __restrict__ recvVc,
                                                                               QualityGeomThresholds thr, QGFace* __restrict__ part,
                                                                               double* __restrict__ outConc, double* __restrict__ outFlat,
                                                                               double* outW, double* outR) {
    __shared__ QGFace sh[kQualityBlock / 64];
    QGFace a = qEmpty<QGFace>();
    const int base = blockIdx.x * (kQualityPer * kQualityBlock) + threadIdx.x;
    for (int k = 0; k < kQualityPer; ++k) {
        const int f = base + k * kQualityBlock;
        if (f >= m.nFaces) break;
        QGFace e = qEmpty<QGFace>();
        qgFaceOne(m, pts, fCtr, fArea, cellCtr, vol, own, nei, thr, f, e, outConc, outFlat, outW, outR);
        const int sl = f < m.nInternalFaces ? -1 : slot[f - m.nInternalFaces];
        if (sl >= 0) {
            const V3 Cf = ldv(fCtr, f), Sf = ldv(fArea, f);
            const int o = own[f];
            const double dO = fabs(dot(Sf, Cf - ldv(cellCtr, o))), dN = fabs(dot(Sf, ldv(recvCc, sl & kQualitySlotMask) - Cf));
            const double w = fmin(dO, dN) / ((dO + dN) + SMGPU_VSMALL);
            const double vO = vol[o], vN = recvVc[sl & kQualitySlotMask];
            const double r = fmin(vO, vN) / (fmax(vO, vN) + SMGPU_VSMALL);
            e.minW = w; e.minWId = f; e.sumW = w; e.nLowW = (w < thr.weight) ? 1 : 0;
            e.minR = r; e.minRId = f; e.sumR = r; e.nLowR = (r < thr.volRatio) ? 1 : 0;
            if (outW) outW[f] = w;
            if (outR) outR[f] = r;
            if (sl & kQualityNotCounted) e = qEmpty<QGFace>();
        }
        qCombine(a, e);
    }
    a = qBlockReduce(a, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = a;
}

// the serial report of the folded record: the averages in place of the sums
__device__ __forceinline__ void qFinish(const smgpu_quality_geometry_part& q, smgpu_quality_geometry_part* __restrict__ out) { *out = q; }
__device__ __forceinline__ void qFinish(const smgpu_quality_geometry_part& q, smgpu_quality_geometry* __restrict__ out) {
    smgpu_quality_geometry r;
    r.nConcaveFaces = q.nConcaveFaces; r.maxConcaveSin = q.maxConcaveSin; r.maxConcaveAngle = q.maxConcaveAngle; r.maxConcaveFace = q.maxConcaveFace;
    r.minFlatness = q.minFlatness; r.avgFlatness = q.nFlatnessFaces > 0 ? q.sumFlatness / (double)q.nFlatnessFaces : 1.0;
    r.nFlatnessFaces = q.nFlatnessFaces; r.nWarpedFaces = q.nWarpedFaces; r.minFlatnessFace = q.minFlatnessFace;
    r.minFaceWeight = q.minFaceWeight; r.avgFaceWeight = q.nInternalFaces > 0 ? q.sumFaceWeight / (double)q.nInternalFaces : 1.0;
    r.nLowWeightFaces = q.nLowWeightFaces; r.minFaceWeightFace = q.minFaceWeightFace;
    r.minVolRatio = q.minVolRatio; r.avgVolRatio = q.nInternalFaces > 0 ? q.sumVolRatio / (double)q.nInternalFaces : 1.0;
    r.nLowVolRatioFaces = q.nLowVolRatioFaces; r.minVolRatioFace = q.minVolRatioFace;
    r.minDeterminant = q.minDeterminant; r.avgDeterminant = q.nCells > 0 ? q.sumDeterminant / (double)q.nCells : 0.0;
    r.nUnderdeterminedCells = q.nUnderdeterminedCells; r.minDeterminantCell = q.minDeterminantCell;
    *out = r;
}
// one workgroup folds the two slabs (qFold) into the record of sums and denominators.  Out = smgpu_quality_geometry_part: the
// per-rank record (nFaces / nInternalFaces are the counted ones); Out = smgpu_quality_geometry: the serial report.  A rank's own
// maxConcaveAngle is derived here from its maxConcaveSin, so the combine evaluates no acos on the host.
template <class Out>
__global__ void __launch_bounds__(kQualityBlock) k_quality_geom_final(const QGFace* __restrict__ fPart, int nFB, const QGCell* __restrict__ cPart,
                                                                       int nCB, int nCells, int nFaces, int nInternalFaces, Out* __restrict__ out) {
    const QGFace a = qFold(fPart, nFB);
    const QGCell b = qFold(cPart, nCB);
    if (threadIdx.x != 0) return;
    smgpu_quality_geometry_part q;
    q.nCells = nCells; q.nFaces = nFaces; q.nInternalFaces = nInternalFaces;
    const bool anyConcave = a.nConcave > 0, anyFlat = a.nFlat > 0, anyInternal = nInternalFaces > 0, anyCell = nCells > 0;
    q.nConcaveFaces = a.nConcave;
    q.maxConcaveSin = anyConcave ? a.maxSin : 0.0;
    q.maxConcaveAngle = anyConcave ? 90.0 - kRadToDeg * smacos::acosX(fmin(1.0, a.maxSin)) : 0.0;
    q.maxConcaveFace = anyConcave ? a.maxSinId : -1;
    q.minFlatness = anyFlat ? a.minFlat : 1.0; q.sumFlatness = a.sumFlat;
    q.nFlatnessFaces = a.nFlat; q.nWarpedFaces = a.nWarped; q.minFlatnessFace = anyFlat ? a.minFlatId : -1;
    q.minFaceWeight = anyInternal ? a.minW : 1.0; q.sumFaceWeight = a.sumW;
    q.nLowWeightFaces = a.nLowW; q.minFaceWeightFace = anyInternal ? a.minWId : -1;
    q.minVolRatio = anyInternal ? a.minR : 1.0; q.sumVolRatio = a.sumR;
    q.nLowVolRatioFaces = a.nLowR; q.minVolRatioFace = anyInternal ? a.minRId : -1;
    q.minDeterminant = anyCell ? b.minDet : 0.0; q.sumDeterminant = b.sumDet;
    q.nUnderdeterminedCells = b.nUnder; q.minDeterminantCell = anyCell ? b.minDetId : -1;
    qFinish(q, out);
}

// ---- the findings as sets (smgpu_quality_geometry_sets / _coupled_geometry_sets, DESIGN.md "Mesh quality", 10.9) ----------------
// The flag passes of kernels_quality.hpp (qFlagPass: one mask byte per element, member counts per workgroup) over the bodies
// above, with null field outputs: a record's count members become the mask bits, so a set's size is the report's count by
// construction.  The sets then go through k_quality_set_scan / _scatter<4, 1>.  nFlat, the flatness denominator, is no set.
constexpr int kQualityGeomFaceSets = 4;   // concaveFaces, warpedFaces, lowWeightFaces, lowVolRatioFaces
constexpr int kQualityGeomCellSets = 1;   // underdeterminedCells
__device__ __forceinline__ unsigned qgFaceBits(const QGFace& e) {
    return (e.nConcave ? 1u : 0u) | (e.nWarped ? 2u : 0u) | (e.nLowW ? 4u : 0u) | (e.nLowR ? 8u : 0u);
}
// Coupled: what k_quality_geom_faces_coupled does to the record of a processor face (its twin, keep alike): weight and ratio
// again with C_N = recvCc[slot], V_N = recvVc[slot]; no bits where the neighbour rank counts the face
template <bool Coupled>
__global__ void __launch_bounds__(kQualityBlock) k_quality_geom_face_flags(MeshView m, const double* __restrict__ pts, const double* __restrict__ fCtr,
                                                                            const double* __restrict__ fArea, const double* __restrict__ cellCtr,
                                                                            const double* __restrict__ vol, const int* __restrict__ own,
                                                                            const int* __restrict__ nei, QCoupling<Coupled> cp,
                                                                            QualityGeomThresholds thr, uint8_t* __restrict__ mask, int* __restrict__ cnt) {
    qFlagPass<kQualityGeomFaceSets>(m.nFaces, mask, cnt, [&](int f) {
        QGFace e = qEmpty<QGFace>();
        qgFaceOne(m, pts, fCtr, fArea, cellCtr, vol, own, nei, thr, f, e, nullptr, nullptr, nullptr, nullptr);
        if constexpr (Coupled) {
            const int sl = f < m.nInternalFaces ? -1 : cp.slot[f - m.nInternalFaces];
            if (sl >= 0) {
                const V3 Cf = ldv(fCtr, f), Sf = ldv(fArea, f);
                const int o = own[f];
                const double dO = fabs(dot(Sf, Cf - ldv(cellCtr, o))), dN = fabs(dot(Sf, ldv(cp.recvCc, sl & kQualitySlotMask) - Cf));
                const double w = fmin(dO, dN) / ((dO + dN) + SMGPU_VSMALL);
                const double vO = vol[o], vN = cp.recvVc[sl & kQualitySlotMask];
                const double r = fmin(vO, vN) / (fmax(vO, vN) + SMGPU_VSMALL);
                e.nLowW = (w < thr.weight) ? 1 : 0;
                e.nLowR = (r < thr.volRatio) ? 1 : 0;
                if (sl & kQualityNotCounted) e = qEmpty<QGFace>();
            }
        }
        return qgFaceBits(e);
    });
}
// serial: qgCellOne, which also leaves the cell's volume in vol for the face flag pass (launched after this one), as
// k_quality_geom_cells does; coupled: qgCellOneCoupled over internal and processor faces, the volumes are k_quality_cell_volumes'
template <bool Coupled>
__global__ void __launch_bounds__(kQualityBlock) k_quality_geom_cell_flags(MeshView m, const double* __restrict__ fCtr, const double* __restrict__ fArea,
                                                                            QCoupling<Coupled> cp, QualityGeomThresholds thr, double* __restrict__ vol,
                                                                            uint8_t* __restrict__ mask, int* __restrict__ cnt) {
    qFlagPass<kQualityGeomCellSets>(m.nCells, mask, cnt, [&](int c) {
        QGCell e = qEmpty<QGCell>();
        if constexpr (Coupled) qgCellOneCoupled(m, fArea, cp.slot, thr, c, e, nullptr);
        else qgCellOne(m, fCtr, fArea, thr, c, e, vol, nullptr);
        return e.nUnder ? 1u : 0u;
    });
}

}  // namespace smgpu
