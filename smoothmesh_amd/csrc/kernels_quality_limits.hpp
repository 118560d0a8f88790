// kernels_quality_limits.hpp -- the quality constraint's tet, twist, weight, ratio and determinant limits
// (smgpu_set_quality_constraint_limits: include/smgpu.h, DESIGN.md "Mesh quality", 10.16): six more criteria for the loop of
// kernels_quality_constraint.hpp, judged by the reports' own measures (kernels_quality_motion.hpp, kernels_quality_geom.hpp).
//
// Per evaluation, between step 1 (k_qc_tile, or the direct geometry kernels) and k_qc_cells of that file's sequence:
//   a. k_qc_cells_more, queued only when minVolRatio or minDeterminant is on: one lane per cell on the fCtr / fArea step 1
//      published: V_c into a buffer of the constraint's own (qgCellOne's lines, the bits of k_quality_cell_volumes), det_c against
//      the limit and the determinant-exempt byte; a bad cell gets the byte in cellFlag that k_qc_cells reads as "bad through
//      something other than 10.12" and clears; one integer atomic per workgroup;
//   b. k_qc_faces_more in the place of k_qc_faces whenever a new face criterion is on: one lane per face in polyMesh order; ortho_f
//      and skew_f by qcFace's lines, the new values from the same loads of C_f, S_f, C_O, C_N; with Walk the skewness loop and
//      qmFaceOne's first walk are one loop that reads every vertex once (the base-point walk is not in it); with Ratio the two
//      volumes are read.  A criterion that is off costs no loads: which walk and which loads run is a template parameter, which
//      verdicts count an argument uniform over the launch.
// k_qc_cells, k_qc_verdict and k_tangle_apply run as they are.  No float atomics; every store is a plain vector store; every
// kernel takes the trace's gate (qTraceRan) and the clean word.
//
// On a sub-domain of a decomposed mesh (smgpu_set_quality_constraint_limits_coupled, 10.17) the two kernels are instantiated with
// Coupled = true and run ungated (they compile no gate test: pass and gate are the serial form's), in the two halves of 10.15's
// evaluation:
//   first half, behind k_qc_tile (or the direct geometry kernels), in front of the packs: k_qc_cells_more<Det, true>, the
//     determinant over the cell's internal and processor faces (the constraint's own slot table).  The byte it leaves in cellFlag
//     waits for k_qc_cells of the second half, underDetNow for the host's read of QcDev there; then k_quality_pack_volumes
//     (kernels_quality_geom.hpp) of the constraint's own volumes into sendVc, only when minVolRatio is on;
//   second half, behind the host's move of Cc and Vc: k_qc_faces_more<Walk, Ratio, true> in the place of k_qc_faces<true>: a
//     processor face takes the internal branch of every criterion with C_N from recvCc and V_N from recvVc, flags its owner only,
//     and counts only on the counted side.
// Every difference between the two forms is an `if constexpr (Coupled)` of the helpers qcSlot, qcNeighbourCentre
// (kernels_quality_constraint.hpp), qcCounts and qcNeighbourVolume: the serial instantiation compiles the serial lines alone.
//
// The last four limits (smgpu_set_quality_constraint_limits_all, 10.18) ride in the same two kernels behind a template parameter
// of their own, so that an instantiation without them is the one of 10.16, register for register:
//   k_qc_cells_more<.., Vol>: minVol on the V_c it forms; bit 1 of the exemption byte (bit 0: the determinant), smallVolNow;
//   k_qc_faces_more<.., Shape>: 0 none; 1 minArea on |S_f|; 2 also maxConcave and minFlatness by qgFaceOne's lines
//     (kernels_quality_geom.hpp) in the one vertex walk the kernel makes -- Walk's loop, or with Walk off a loop of their own with
//     the skewness line in it.  A processor face is judged on the rank's own vertex order, as 10.8's report does.
#pragma once
#include "kernels_quality_constraint.hpp"
#include "kernels_quality_geom.hpp"
#include "kernels_quality_motion.hpp"

namespace smgpu {

// the limits as the kernels test them; k: the tets' normalisation, formed by the host as the motion report forms it
struct QcMore { double minTet, minTwist, minTri, minWeight, minRatio, minDet, k; int tetOn, twistOn, triOn, weightOn, ratioOn, detOn; };

// the limits of 10.18 as the kernels test them; sinConcave: formed by the host as the geometry report forms its own
struct QcShape { double sinConcave, minFlat, minArea, minVol; int concaveOn, flatOn, areaOn, volOn; };

// does face f enter a cell's determinant: an internal face of the global mesh -- on a sub-domain qgcCounts
// (kernels_quality_geom.hpp), without processor faces the same bits
template <bool Coupled>
__device__ __forceinline__ bool qcCounts(const MeshView& m, const QCoupling<Coupled>& cp, int f) {
    if constexpr (Coupled) return qgcCounts(m, cp.slot, f);
    else return f < m.nInternalFaces;
}
// V_N of a face that is internal to the global mesh: the neighbour cell's, or across a processor face recvVc's
template <bool Coupled>
__device__ __forceinline__ double qcNeighbourVolume(const double* __restrict__ vol, const QCoupling<Coupled>& cp, bool inner, int n, int sl) {
    if constexpr (Coupled) return inner ? vol[n] : cp.recvVc[sl & kQualitySlotMask];
    else return vol[n];
}

// V_c into vol and det_c of cell c: qgCellOne's lines (kernels_quality_geom.hpp), nothing else of it -- keep them alike.
// exemptOut != NULL (enabling): the determinant verdict goes to exemptOut[c], no cell is flagged, underDetNow counts them.
// Vol (10.18): V_c < minVol; the exemption byte is then a bit set -- bit 0 determinant, bit 1 volume -- and smallVolNow counts.
template <bool Det, bool Coupled, bool Vol>
__global__ void __launch_bounds__(kQcBlock) k_qc_cells_more(MeshView m, const double* __restrict__ fCtr, const double* __restrict__ fArea,
                                                             QCoupling<Coupled> cp, QcMore lim, QcShape sh, double* __restrict__ vol, const uint8_t* __restrict__ exempt, uint8_t* __restrict__ exemptOut,
                                                             uint8_t* __restrict__ cellFlag, QcDev* __restrict__ d, int pass, const smgpu_iter_stats* gate) {
    if constexpr (!Coupled) {   // (the coupled form is never gated, and the test cost it 0.05 - 0.2 %: profiles/quality/README.md)
        if (!qTraceRan(gate) || (pass > 0 && d->t.clean)) return;
    }
    const int c = blockIdx.x * kQcBlock + threadIdx.x;
    bool bad = false, badV = false;
    if (c < m.nCells) {
        const int b = m.cfOff[c], e = m.cfOff[c + 1];
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
            if (Det && qcCounts(m, cp, f)) { sumA += mag(Sf); ++nInt; }
        }
        const double Vc = (1.0 / 3.0) * pyr;
        vol[c] = Vc;
        if constexpr (Vol) badV = sh.volOn && Vc < sh.minVol;
        if constexpr (Det) {
            double det = 0.0;
            const double avgA = nInt > 0 ? sumA / (double)nInt : 0.0;
            if (nInt > 0 && avgA >= SMGPU_ROOTVSMALL) {
                double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
                for (int j = b; j < e; ++j) {
                    const int f = m.cfVal[j] & 0x7fffffff;
                    if (!qcCounts(m, cp, f)) continue;
                    const V3 s = ldv(fArea, f) / avgA;
                    xx += s.x * s.x; xy += s.x * s.y; xz += s.x * s.z;
                    yy += s.y * s.y; yz += s.y * s.z; zz += s.z * s.z;
                }
                det = fabs((xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz)) + xz * (xy * yz - yy * xz)) / 8.0;
            }
            bad = det < lim.minDet;
            if constexpr (!Vol) {
                if (exemptOut) exemptOut[c] = bad ? 1 : 0;
                else {
                    bad = bad && !exempt[c];
                    if (bad) cellFlag[c] = 1;
                }
            }
        }
        if constexpr (Vol) {
            if (exemptOut) exemptOut[c] = (uint8_t)((bad ? 1 : 0) | (badV ? 2 : 0));
            else {
                const int ex = exempt[c];
                bad = bad && !(ex & 1);
                badV = badV && !(ex & 2);
                if (bad || badV) cellFlag[c] = 1;
            }
        }
    }
    if constexpr (Det) {
        const int nBad = __syncthreads_count(bad ? 1 : 0);
        if (nBad > 0 && threadIdx.x == 0) atomicAdd(&d->underDetNow, nBad);
    }
    if constexpr (Vol) {
        const int nBadV = __syncthreads_count(badV ? 1 : 0);
        if (nBadV > 0 && threadIdx.x == 0) atomicAdd(&d->smallVolNow, nBadV);
    }
}

// k_qc_faces with the new face criteria.  The lines up to fd are qcFace's, the walk is qmFaceOne's first walk with the skewness
// loop's line in it (both read the vertices in the face's order; fmax and fmin do not depend on it), weight and ratio are
// qgFaceOne's lines: keep each alike.  exemptOut != NULL (enabling): as k_qc_faces.  Coupled: the slot is decoded as k_qc_faces
// decodes it; `internal` is "internal face of the global mesh", `inner` "both cells are this rank's".
// Shape (10.18): 1 the area verdict on magSf; 2 also concavity and flatness, qgFaceOne's lines (kernels_quality_geom.hpp: the unit
// edge that ends in the current point carried, the first kept for corner 0; the triangles' magnitudes summed in ascending i,
// without the twist's mt > VSMALL test) -- keep them alike.  They share Walk's loop; with Walk off the loop is theirs.
template <bool Walk, bool Ratio, bool Coupled, int Shape>
__global__ void __launch_bounds__(kQcBlock) k_qc_faces_more(MeshView m, const double* __restrict__ pts, const double* __restrict__ fCtr,
                                                             const double* __restrict__ fArea, const double* __restrict__ cellCtr,
                                                             const double* __restrict__ vol, const int* __restrict__ own, const int* __restrict__ nei,
                                                             QCoupling<Coupled> cp, QcLimits lim, QcMore more, QcShape sh, const uint8_t* __restrict__ exempt, uint8_t* __restrict__ exemptOut,
                                                             uint8_t* __restrict__ cellFlag, QcDev* __restrict__ d, int pass, const smgpu_iter_stats* gate) {
    if constexpr (!Coupled) {   // (the coupled form is never gated, and the test cost it 0.05 - 0.2 %: profiles/quality/README.md)
        if (!qTraceRan(gate) || (pass > 0 && d->t.clean)) return;
    }
    const int f = blockIdx.x * kQcBlock + threadIdx.x;
    bool badNO = false, badSk = false, badTet = false, badTw = false, badTri = false, badW = false, badR = false, counted = true;
    bool badConc = false, badFlat = false, badArea = false;
    if (f < m.nFaces) {
        const bool inner = f < m.nInternalFaces;
        const int sl = qcSlot(m, cp, f);
        const bool internal = inner || sl >= 0;
        counted = sl < 0 || !(sl & kQualityNotCounted);
        const int o = own[f], n = inner ? nei[f] : 0;
        const V3 Cf = ldv(fCtr, f), Sf = ldv(fArea, f), CO = ldv(cellCtr, o), CN = qcNeighbourCentre(cellCtr, cp, inner, n, sl);
        const double magSf = mag(Sf);
        const V3 Cpf = Cf - CO;
        V3 dd;
        double ortho = 1.0;
        if (internal) {
            dd = CN - CO;
            ortho = dot(dd, Sf) / (mag(dd) * magSf + SMGPU_VSMALL);
        } else {
            const V3 nb = Sf / (magSf + SMGPU_ROOTVSMALL);
            dd = dot(nb, Cpf) * nb;
        }
        const V3 sv = Cpf - (dot(Sf, Cpf) / (dot(Sf, dd) + SMGPU_ROOTVSMALL)) * dd;
        const double magSv = mag(sv);
        const V3 sHat = sv / (magSv + SMGPU_ROOTVSMALL);
        double fd = 0.2 * mag(dd) + SMGPU_ROOTVSMALL;
        const int jb = m.faceOff[f], nv = m.faceOff[f + 1] - jb;
        if constexpr (Walk || Shape == 2) {
            const bool summed = nv > 3;
            double tet = __builtin_inf(), tw = __builtin_inf(), tri = __builtin_inf();
            double conc = 0.0, area = 0.0;
            int nValid = 0;
            if (nv > 0) {
                const V3 dv = sel3(internal, CN, Cf) - CO;
                const V3 nHat = dv / (mag(dv) + SMGPU_VSMALL);
                const V3 nS = Sf / (magSf + SMGPU_ROOTVSMALL);
                const V3 p0 = ldv(pts, m.facePts[jb]);
                V3 cur = p0, hFirst = v3(0, 0, 0), hPrev = v3(0, 0, 0);
                V3 eFirst = v3(0, 0, 0), ePrev = v3(0, 0, 0);
                bool okFirst = false, okPrev = false;
                for (int i = 0; i < nv; ++i) {
                    fd = fmax(fd, fabs(dot(sHat, cur - Cf)));
                    const V3 nxt = (i + 1 < nv) ? ldv(pts, m.facePts[jb + i + 1]) : p0;
                    const V3 u = nxt - cur, v = Cf - cur;
                    if constexpr (Walk) tet = fmin(tet, qmTetPair(cur, u, v, CO, internal, CN, more.k));
                    if constexpr (Shape == 2) {
                        const double len = mag(u);
                        const V3 eNext = u / (len + SMGPU_ROOTVSMALL);
                        const bool okNext = len > kQualitySmall;
                        area += 0.5 * mag(cross(u, v));
                        if (i > 0) conc = fmax(conc, qgCorner(ePrev, eNext, okPrev && okNext, nS, sh.sinConcave));
                        else { eFirst = eNext; okFirst = okNext; }
                        ePrev = eNext; okPrev = okNext;
                    }
                    if (Walk && summed) {
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
                if constexpr (Shape == 2) conc = fmax(conc, qgCorner(ePrev, eFirst, okPrev && okFirst, nS, sh.sinConcave));   // corner 0
            }
            if constexpr (Walk) {
                if (nValid < 1) tw = 1.0;
                if (nValid < 2) tri = 1.0;
                badTet = more.tetOn && tet < more.minTet;
                badTw = summed && more.twistOn && tw < more.minTwist;
                badTri = summed && more.triOn && tri < more.minTri;
            }
            if constexpr (Shape == 2) {
                badConc = sh.concaveOn && conc > kQualitySmall;
                badFlat = sh.flatOn && summed && magSf > SMGPU_ROOTVSMALL && magSf / (area + SMGPU_ROOTVSMALL) < sh.minFlat;
            }
        } else {
            for (int j = jb; j < jb + nv; ++j) fd = fmax(fd, fabs(dot(sHat, ldv(pts, m.facePts[j]) - Cf)));
        }
        if constexpr (Shape >= 1) badArea = sh.areaOn && magSf < sh.minArea;
        const double skew = magSv / fd;
        badNO = internal && lim.nonOrthoOn && ortho < lim.cosT;
        badSk = internal ? (lim.internalSkewOn && skew > lim.maxInternalSkew) : (lim.boundarySkewOn && skew > lim.maxBoundarySkew);
        if (internal) {
            const double dO = fabs(dot(Sf, Cpf)), dN = fabs(dot(Sf, CN - Cf));
            const double w = fmin(dO, dN) / ((dO + dN) + SMGPU_VSMALL);
            badW = more.weightOn && w < more.minWeight;
            if constexpr (Ratio) {
                const double vO = vol[o], vN = qcNeighbourVolume(vol, cp, inner, n, sl);
                const double r = fmin(vO, vN) / (fmax(vO, vN) + SMGPU_VSMALL);
                badR = more.ratioOn && r < more.minRatio;
            }
        }
        const bool any = badNO || badSk || badTet || badTw || badTri || badW || badR || badConc || badFlat || badArea;
        if (exemptOut) exemptOut[f] = any ? 1 : 0;
        else if (exempt[f]) badNO = badSk = badTet = badTw = badTri = badW = badR = badConc = badFlat = badArea = false;
        else if (any) {
            cellFlag[o] = 1;
            if (inner) cellFlag[n] = 1;
        }
    }
    const bool any = badNO || badSk || badTet || badTw || badTri || badW || badR || badConc || badFlat || badArea;
    const int nNO = __syncthreads_count((badNO && counted) ? 1 : 0), nSk = __syncthreads_count((badSk && counted) ? 1 : 0),
              nAny = __syncthreads_count((any && counted) ? 1 : 0);
    int nTet = 0, nTw = 0, nTri = 0, nW = 0, nR = 0, nConc = 0, nFlat = 0, nArea = 0;
    if (Walk && more.tetOn) nTet = __syncthreads_count((badTet && counted) ? 1 : 0);
    if (Walk && more.twistOn) nTw = __syncthreads_count((badTw && counted) ? 1 : 0);
    if (Walk && more.triOn) nTri = __syncthreads_count((badTri && counted) ? 1 : 0);
    if (more.weightOn) nW = __syncthreads_count((badW && counted) ? 1 : 0);
    if (Ratio && more.ratioOn) nR = __syncthreads_count((badR && counted) ? 1 : 0);
    if constexpr (Shape == 2) {
        if (sh.concaveOn) nConc = __syncthreads_count((badConc && counted) ? 1 : 0);
        if (sh.flatOn) nFlat = __syncthreads_count((badFlat && counted) ? 1 : 0);
    }
    if constexpr (Shape >= 1) {
        if (sh.areaOn) nArea = __syncthreads_count((badArea && counted) ? 1 : 0);
    }
    if (threadIdx.x == 0) {
        if (nNO > 0) atomicAdd(&d->nonOrthoNow, nNO);
        if (nSk > 0) atomicAdd(&d->skewNow, nSk);
        if (nAny > 0) atomicAdd(&d->facesNow, nAny);
        if (nTet > 0) atomicAdd(&d->lowTetNow, nTet);
        if (nTw > 0) atomicAdd(&d->lowTwistNow, nTw);
        if (nTri > 0) atomicAdd(&d->lowTriNow, nTri);
        if (nW > 0) atomicAdd(&d->lowWeightNow, nW);
        if (nR > 0) atomicAdd(&d->lowRatioNow, nR);
        if (nConc > 0) atomicAdd(&d->concaveNow, nConc);
        if (nFlat > 0) atomicAdd(&d->warpedNow, nFlat);
        if (nArea > 0) atomicAdd(&d->smallAreaNow, nArea);
    }
}

}  // namespace smgpu
