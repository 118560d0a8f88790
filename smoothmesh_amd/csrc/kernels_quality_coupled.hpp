// kernels_quality_coupled.hpp -- the -allGeometry checks and the motion criteria for a sub-domain of a decomposed mesh
// (smgpu_quality_coupled_pack_volumes, smgpu_quality_coupled_geometry_* / _motion_*: include/smgpu.h).  Definitions: DESIGN.md
// "Mesh quality", 10.8: a processor face takes the internal-face branch of every criterion with C_N (recvCc) and V_N (recvVc) of
// the neighbour rank, a cell's determinant runs over its internal and processor faces, and a processor face enters the record only
// on the side with myRank < neighbRank.
//
// The layout is that of kernels_quality.hpp: kQualityBlock threads, kQualityPer elements per lane, one partial record per
// workgroup, one folding workgroup, no float atomics.  Nothing of kernels_quality.hpp, kernels_quality_geom.hpp or
// kernels_quality_motion.hpp is changed: their records, reductions and qgFaceOne are used as they are, and where a loop is written
// a second time the comment names its twin.  slot[f - nInternalFaces] is the array smgpu_quality_coupled_pack builds: -1 on a
// physical boundary face, else the face's place in recvCc / recvVc (| kQualityNotCounted on the side that does not count it).
#pragma once
#include "kernels_quality_geom.hpp"
#include "kernels_quality_motion.hpp"

namespace smgpu {

// the signed volume of every cell into vol, for the face pass and the volume pack.  Twin of the V_c loop of qgCellOne
// (kernels_quality_geom.hpp), itself the twin of qCellOne's: the same formula in the same order, so the same bits.  Keep them alike.
__global__ void __launch_bounds__(kQualityBlock) k_quality_cell_volumes(MeshView m, const double* __restrict__ fCtr, const double* __restrict__ fArea,
                                                                         double* __restrict__ vol) {
    const int base = blockIdx.x * (kQualityPer * kQualityBlock) + threadIdx.x;
    for (int k = 0; k < kQualityPer; ++k) {
        const int c = base + k * kQualityBlock;
        if (c >= m.nCells) break;
        const int b = m.cfOff[c], e = m.cfOff[c + 1];
        V3 cEst = v3(0, 0, 0);
        for (int j = b; j < e; ++j) cEst = cEst + ldv(fCtr, m.cfVal[j] & 0x7fffffff);
        cEst = cEst / (double)(e - b);
        double pyr = 0.0;
        for (int j = b; j < e; ++j) {
            const int ev = m.cfVal[j];
            const int f = ev & 0x7fffffff;
            double p = dot(ldv(fArea, f), ldv(fCtr, f) - cEst);
            if (ev < 0) p = -p;
            pyr += p;
        }
        vol[c] = (1.0 / 3.0) * pyr;
    }
}

// the owner cell's volume of every processor face, in patch order (the slot order of k_quality_pack): what the neighbour rank
// needs as its V_N.  Lane i stores sendVc[i]: contiguous stores, gathered loads.
__global__ void __launch_bounds__(kQualityBlock) k_quality_pack_volumes(const int* __restrict__ own, const double* __restrict__ vol,
                                                                         const int* __restrict__ procFace, int nProc, double* __restrict__ sendVc) {
    const int i = blockIdx.x * kQualityBlock + threadIdx.x;
    if (i >= nProc) return;
    sendVc[i] = vol[own[procFace[i]]];
}

// the determinant of cell c over its internal and its processor faces.  Twin of the determinant part of qgCellOne
// (kernels_quality_geom.hpp): the face test "f < nInternalFaces" widened by "or has a slot >= 0", the sums in the same order
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
    QGCell a = qgCellEmpty();
    const int base = blockIdx.x * (kQualityPer * kQualityBlock) + threadIdx.x;
    for (int k = 0; k < kQualityPer; ++k) {
        const int c = base + k * kQualityBlock;
        if (c >= m.nCells) break;
        QGCell e = qgCellEmpty();
        qgCellOneCoupled(m, fArea, slot, thr, c, e, outDet);
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
    QGFace a = qgFaceEmpty();
    const int base = blockIdx.x * (kQualityPer * kQualityBlock) + threadIdx.x;
    for (int k = 0; k < kQualityPer; ++k) {
        const int f = base + k * kQualityBlock;
        if (f >= m.nFaces) break;
        QGFace e = qgFaceEmpty();
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
            if (sl & kQualityNotCounted) e = qgFaceEmpty();
        }
        qCombine(a, e);
    }
    a = qBlockReduce(a, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = a;
}

// k_quality_geom_final for the per-rank record: the sums instead of the averages; nFaces / nInternalFaces are the counted ones.
// The rank's own maxConcaveAngle is derived here from its maxConcaveSin, so the combine evaluates no acos on the host.
__global__ void __launch_bounds__(kQualityBlock) k_quality_geom_part_final(const QGFace* __restrict__ fPart, int nFB, const QGCell* __restrict__ cPart,
                                                                            int nCB, int nCells, int nFaces, int nInternalFaces,
                                                                            smgpu_quality_geometry_part* __restrict__ out) {
    __shared__ QGFace shF[kQualityBlock / 64];
    __shared__ QGCell shC[kQualityBlock / 64];
    QGFace a = qgFaceEmpty();
    for (int i = threadIdx.x; i < nFB; i += kQualityBlock) qCombine(a, fPart[i]);
    QGCell b = qgCellEmpty();
    for (int i = threadIdx.x; i < nCB; i += kQualityBlock) qCombine(b, cPart[i]);
    a = qBlockReduce(a, shF);
    b = qBlockReduce(b, shC);
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
    *out = q;
}

// qmFaceOne (kernels_quality_motion.hpp) with `internal` and C_N given by the caller, so that a processor face takes the
// internal-face branch of the tets and the twist with the neighbour rank's cell centre.  Its twin: the two walks, statement by
// statement; with internal = f < nInternalFaces and C_N = cellCtr[nei[f]] the same bits.  Keep the two alike.
__device__ __forceinline__ void qmFaceOneCoupled(const MeshView& m, const double* __restrict__ pts, const double* __restrict__ fCtr,
                                                 const V3 CO, const bool internal, const V3 CN, const QualityMotionThresholds& thr, int f,
                                                 QMFace& a, double* __restrict__ outTet, double* __restrict__ outBase,
                                                 double* __restrict__ outTw, double* __restrict__ outTri) {
    const V3 Cf = ldv(fCtr, f);
    const int jb = m.faceOff[f], nv = m.faceOff[f + 1] - jb;
    const bool summed = nv > 3;
    double tet = __builtin_inf(), tw = __builtin_inf(), tri = __builtin_inf();
    int nValid = 0;
    if (nv > 0) {
        const V3 dv = sel3(internal, CN, Cf) - CO;
        const V3 nHat = dv / (mag(dv) + SMGPU_VSMALL);
        const V3 p0 = ldv(pts, m.facePts[jb]);
        V3 cur = p0, hFirst = v3(0, 0, 0), hPrev = v3(0, 0, 0);
        for (int i = 0; i < nv; ++i) {
            const V3 nxt = (i + 1 < nv) ? ldv(pts, m.facePts[jb + i + 1]) : p0;
            const V3 u = nxt - cur, v = Cf - cur;
            tet = fmin(tet, qmTetPair(cur, u, v, CO, internal, CN, thr.k));
            if (summed) {
                const V3 t = 0.5 * cross(u, v);
                const double mt = mag(t);
                if (mt > SMGPU_VSMALL) {
                    const V3 h = t / mt;
                    tw = fmin(tw, dot(nHat, h));
                    if (nValid > 0) tri = fmin(tri, dot(hPrev, h));
                    else hFirst = h;
                    hPrev = h;
                    ++nValid;
                }
            }
            cur = nxt;
        }
        if (nValid >= 2) tri = fmin(tri, dot(hPrev, hFirst));
    }
    double base = __builtin_inf();
    for (int b = 0; b < nv; ++b) {
        const V3 pb = ldv(pts, m.facePts[jb + b]);
        int i = b + 1 < nv ? b + 1 : b + 1 - nv;
        V3 u = ldv(pts, m.facePts[jb + i]) - pb;
        double mb = __builtin_inf();
        for (int k = 1; k + 2 <= nv; ++k) {
            i = i + 1 < nv ? i + 1 : 0;
            const V3 v = ldv(pts, m.facePts[jb + i]) - pb;
            mb = fmin(mb, qmTetPair(pb, u, v, CO, internal, CN, thr.k));
            u = v;
        }
        if (b == 0 || mb > base) base = mb;
    }
    a.minTet = tet; a.minTetId = f; a.sumTet = tet; a.nLowTet = (tet < thr.tet) ? 1 : 0;
    a.minBase = base; a.minBaseId = f; a.nNoBase = (base < thr.tet) ? 1 : 0;
    if (nValid < 1) tw = 1.0;
    if (nValid < 2) tri = 1.0;
    if (summed) {
        a.minTw = tw; a.minTwId = f; a.sumTw = tw; a.nTw = 1; a.nLowTw = (tw < thr.twist) ? 1 : 0;
        a.minTri = tri; a.minTriId = f; a.sumTri = tri; a.nLowTri = (tri < thr.triTwist) ? 1 : 0;
    }
    if (outTet) outTet[f] = tet;
    if (outBase) outBase[f] = base;
    if (outTw) outTw[f] = tw;
    if (outTri) outTri[f] = tri;
}
// k_quality_motion_faces with processor faces: one body for the three kinds of face (the slot only selects where C_N comes
// from), so the register budget is that of k_quality_motion_faces plus the slot
__global__ void __launch_bounds__(kQualityBlock) k_quality_motion_faces_coupled(MeshView m, const double* __restrict__ pts, const double* __restrict__ fCtr,
                                                                                 const double* __restrict__ cellCtr, const int* __restrict__ own,
                                                                                 const int* __restrict__ nei, const int* __restrict__ slot,
                                                                                 const double* __restrict__ recvCc, QualityMotionThresholds thr,
                                                                                 QMFace* __restrict__ part, double* __restrict__ outTet,
                                                                                 double* __restrict__ outBase, double* __restrict__ outTw,
                                                                                 double* __restrict__ outTri) {
    __shared__ QMFace sh[kQualityBlock / 64];
    QMFace a = qmFaceEmpty();
    const int base = blockIdx.x * (kQualityPer * kQualityBlock) + threadIdx.x;
    for (int k = 0; k < kQualityPer; ++k) {
        const int f = base + k * kQualityBlock;
        if (f >= m.nFaces) break;
        QMFace e = qmFaceEmpty();
        const int sl = f < m.nInternalFaces ? -1 : slot[f - m.nInternalFaces];
        // C_N by address: the neighbour cell's row of cellCtr, the slot's row of recvCc, or (physical patch, unused) the owner's row
        const double* cnAt = f < m.nInternalFaces ? cellCtr + 3 * (size_t)nei[f]
                                                  : (sl >= 0 ? recvCc + 3 * (size_t)(sl & kQualitySlotMask) : cellCtr + 3 * (size_t)own[f]);
        const bool internal = f < m.nInternalFaces || sl >= 0;
        const V3 CN = internal ? v3(cnAt[0], cnAt[1], cnAt[2]) : v3(0, 0, 0);
        qmFaceOneCoupled(m, pts, fCtr, ldv(cellCtr, own[f]), internal, CN, thr, f, e, outTet, outBase, outTw, outTri);
        if (sl >= 0 && (sl & kQualityNotCounted)) e = qmFaceEmpty();
        qCombine(a, e);
    }
    a = qBlockReduce(a, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = a;
}

// k_quality_motion_final for the per-rank record: the sums instead of the averages; nFaces is the counted one
__global__ void __launch_bounds__(kQualityBlock) k_quality_motion_part_final(const QMFace* __restrict__ fPart, int nFB, int nFaces,
                                                                              smgpu_quality_motion_part* __restrict__ out) {
    __shared__ QMFace sh[kQualityBlock / 64];
    QMFace a = qmFaceEmpty();
    for (int i = threadIdx.x; i < nFB; i += kQualityBlock) qCombine(a, fPart[i]);
    a = qBlockReduce(a, sh);
    if (threadIdx.x != 0) return;
    smgpu_quality_motion_part q;
    q.nFaces = nFaces;
    const bool anyFace = nFaces > 0, anyTw = a.nTw > 0;
    q.minTetQuality = anyFace ? a.minTet : 1.0; q.sumTetQuality = a.sumTet;
    q.nLowTetFaces = a.nLowTet; q.minTetFace = anyFace ? a.minTetId : -1;
    q.minBaseTetQuality = anyFace ? a.minBase : 1.0; q.nNoBasePointFaces = a.nNoBase; q.minBaseTetFace = anyFace ? a.minBaseId : -1;
    q.minTwist = anyTw ? a.minTw : 1.0; q.sumTwist = a.sumTw;
    q.nTwistFaces = a.nTw; q.nLowTwistFaces = a.nLowTw; q.minTwistFace = anyTw ? a.minTwId : -1;
    q.minTriangleTwist = anyTw ? a.minTri : 1.0; q.sumTriangleTwist = a.sumTri;
    q.nLowTriangleTwistFaces = a.nLowTri; q.minTriangleTwistFace = anyTw ? a.minTriId : -1;
    *out = q;
}

}  // namespace smgpu
