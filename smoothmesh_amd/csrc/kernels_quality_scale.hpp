// kernels_quality_scale.hpp -- the quality constraint's scaling passes (smgpu_set_quality_constraint_scaling: include/smgpu.h,
// DESIGN.md "Mesh quality", 10.19): before the points of a bad cell go back to where the iteration found them, they keep a
// fraction of their move.  Every point carries a scale s_p (1 at the start of an iteration); the current points are
// x + s (L - x), with L the points the loop produced and x the points it started from.
//
// Per iteration the engine queues, for k = 0 .. S + P, behind the evaluation of 10.14 / 10.16 / 10.18 (unchanged kernels)
//   1. k_qs_verdict: k_qc_verdict's twin with the wider record; it knows S, counts the scaling passes and, in front of every
//      pass that changes the points, resets the three counts that describe the accepted state;
//   2. at k = 0, k_qs_keep: a streaming copy of ptsCur into the constraint's own L (k_quality_guard_snapshot's access pattern)
//      and the fill of the scale field with 1.0;
//   3. k_qs_mark: one lane per word of four mark bytes (k_tangle_apply's read): s *= r, or s = 0, for the marked points (every
//      point in the full revert); clears the marks;
//   4. nSmoothScale times k_qs_sweep: one lane per point and trip, Jacobi, between two fields:
//      s <- min(s, 0.5 s + 0.5 (sum_q s_q) / deg) over the pointPoints row in row order (not in the full revert: all zero);
//   5. k_qs_apply: one lane per point and trip; where s < 1 the point is written from x and L, and counted.
// Every kernel takes the trace's gate (qTraceRan) and the clean word, so a clean iteration moves no bytes.  No float atomics
// (minScale is an integer atomic min on the bits of a non-negative double); every store is a plain vector store.
#pragma once
#include "kernels_quality_constraint.hpp"

namespace smgpu {

static_assert(offsetof(smgpu_quality_constraint_record_scaled, nSmallVolumeCells) == offsetof(smgpu_quality_constraint_record_all, nSmallVolumeCells) &&
              offsetof(smgpu_quality_constraint_record_scaled, nScalePasses) == sizeof(smgpu_quality_constraint_record_all) &&
              sizeof(smgpu_quality_constraint_record_all) == 136 && sizeof(smgpu_quality_constraint_record_scaled) == 160 &&
              offsetof(smgpu_quality_constraint_record_scaled, nPointsScaled) == 144 && offsetof(smgpu_quality_constraint_record_scaled, minScale) == 152,
              "the widest record of 10.18 is the head of the scaled one, which the slab holds: the narrower getters copy their prefix");
static_assert(offsetof(smgpu_quality_constraint_state_scaled, nExemptVolumeCells) == offsetof(smgpu_quality_constraint_state_all, nExemptVolumeCells) &&
              offsetof(smgpu_quality_constraint_state_scaled, scalePasses) == sizeof(smgpu_quality_constraint_state_all) &&
              sizeof(smgpu_quality_constraint_state_all) == 152 && offsetof(smgpu_quality_constraint_state_scaled, nSmoothScale) == 156 &&
              offsetof(smgpu_quality_constraint_state_scaled, errorReduction) == 160 && sizeof(smgpu_quality_constraint_state_scaled) == 168,
              "smgpu_quality_constraint_state_all is the head of smgpu_quality_constraint_state_scaled");
static_assert(sizeof(smgpu_quality_constraint_scaling) == 16 && offsetof(smgpu_quality_constraint_scaling, errorReduction) == 8, "smgpu_quality_constraint_scaling");

constexpr int kQsBlock = 256;
// the sweep and the apply take one point per lane and trip, on a grid of at most kQsMaxGrid workgroups: a launch that returns on
// the clean word costs by its workgroup count (10.19: 10 us at 39.7 k workgroups, 4.7 us at or under 10 k), and a clean iteration
// queues nSmoothScale (S + P) + S + P + 1 of them
constexpr int kQsMaxGrid = 8192;
constexpr unsigned long long kQsOneBits = 0x3ff0000000000000ull;   // 1.0

// k_qc_verdict's twin (keep them alike): total = S + P.  A pass that is not clean changes the points, and k_qs_apply counts the
// accepted state anew: nPointsReverted, nPointsScaled and minScale start over here.
__global__ void __launch_bounds__(64) k_qs_verdict(QcDev* __restrict__ d, Accum* __restrict__ acc, smgpu_quality_constraint_record_scaled* __restrict__ rec,
                                                    long long number, int pass, int scalePasses, int total, const smgpu_iter_stats* gate) {
    if (threadIdx.x != 0) return;
    if (!qTraceRan(gate) || (pass > 0 && d->t.clean)) return;
    const int nBad = d->t.badNow, nTangled = d->tangledNow, nNO = d->nonOrthoNow, nSk = d->skewNow;
    const int nTet = d->lowTetNow, nTw = d->lowTwistNow, nTri = d->lowTriNow, nW = d->lowWeightNow, nR = d->lowRatioNow, nDet = d->underDetNow;
    d->t.badNow = 0; d->tangledNow = 0; d->nonOrthoNow = 0; d->skewNow = 0; d->facesNow = 0;
    const int nConc = d->concaveNow, nWarp = d->warpedNow, nArea = d->smallAreaNow, nVol = d->smallVolNow;
    d->lowTetNow = 0; d->lowTwistNow = 0; d->lowTriNow = 0; d->lowWeightNow = 0; d->lowRatioNow = 0; d->underDetNow = 0;
    d->concaveNow = 0; d->warpedNow = 0; d->smallAreaNow = 0; d->smallVolNow = 0;
    if (pass == 0) {
        smgpu_quality_constraint_record_scaled r;
        r.iteration = number; r.passes = 0; r.fullRevert = 0; r.nBadCells = nBad; r.nPointsReverted = 0;
        r.nTangledCells = nTangled; r.nNonOrthoFaces = nNO; r.nSkewFaces = nSk;
        r.nLowTetFaces = nTet; r.nLowTwistFaces = nTw; r.nLowTriangleTwistFaces = nTri; r.nLowWeightFaces = nW; r.nLowVolRatioFaces = nR;
        r.nUnderdeterminedCells = nDet;
        r.nConcaveFaces = nConc; r.nWarpedFaces = nWarp; r.nSmallAreaFaces = nArea; r.nSmallVolumeCells = nVol;
        r.nScalePasses = 0; r.nPointsScaled = 0; r.minScale = 1.0;
        *rec = r;
    }
    if (nBad == 0) { d->t.clean = 1; d->t.full = 0; acc->stop = 1; return; }
    d->t.clean = 0;
    rec->nPointsReverted = 0; rec->nPointsScaled = 0; rec->minScale = 1.0;
    if (pass == total) { d->t.full = 1; rec->fullRevert = 1; }
    else {
        d->t.full = 0;
        rec->passes += 1;
        if (pass < scalePasses) rec->nScalePasses += 1;
    }
}

// Behind the verdict at k = 0 of an iteration that is not clean: L <- ptsCur (n = 3 nPoints doubles) and scale <- 1.0 (nScale
// doubles, even: the field's allocation is rounded up).  k_quality_guard_snapshot's pattern: 16 bytes per lane per access,
// consecutive lanes at consecutive addresses, kGuardPer accesses per lane in flight, every load issued before the first store; a
// lane past the end loads the last pair again (in bounds) and stores nothing.  The odd double of the tail goes with lane 0.
// nScale / 2 <= n / 2, so the lanes that copy also fill.
__global__ void __launch_bounds__(kGuardBlock) k_qs_keep(const double* __restrict__ src, double* __restrict__ dst, long long n, double* __restrict__ scale,
                                                          long long nScale, const QcDev* __restrict__ d, const smgpu_iter_stats* gate) {
    if (!qTraceRan(gate) || d->t.clean) return;
    const long long nPair = n >> 1, nFill = nScale >> 1;
    const long long base = (long long)blockIdx.x * (kGuardBlock * kGuardPer) + threadIdx.x;
    if (nPair > 0) {
        const double2* __restrict__ s0 = reinterpret_cast<const double2*>(src);
        const long long i0 = base, i1 = base + kGuardBlock, i2 = base + 2 * kGuardBlock, i3 = base + 3 * kGuardBlock, last = nPair - 1;
        const double2 a0 = s0[i0 < nPair ? i0 : last], a1 = s0[i1 < nPair ? i1 : last], a2 = s0[i2 < nPair ? i2 : last], a3 = s0[i3 < nPair ? i3 : last];
        double2* __restrict__ d0 = reinterpret_cast<double2*>(dst);
        if (i0 < nPair) d0[i0] = a0;
        if (i1 < nPair) d0[i1] = a1;
        if (i2 < nPair) d0[i2] = a2;
        if (i3 < nPair) d0[i3] = a3;
        double2* __restrict__ sc = reinterpret_cast<double2*>(scale);
        const double2 one = make_double2(1.0, 1.0);
        if (i0 < nFill) sc[i0] = one;
        if (i1 < nFill) sc[i1] = one;
        if (i2 < nFill) sc[i2] = one;
        if (i3 < nFill) sc[i3] = one;
    }
    static_assert(kGuardPer == 4, "the four accesses are written out");
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1)) dst[n - 1] = src[n - 1];
}

// Mark -> scale.  marks: nPoints rounded up to a multiple of 4 bytes, zero past the end (k_tangle_apply's).  One lane per word; a
// lane whose word is zero reads nothing else.  mode 0: s *= r for the marked points; 1: s = 0 for them; 2 (the full revert):
// s = 0 for every point.  The marks are cleared.
enum : int { kQsScale = 0, kQsZero = 1, kQsFull = 2 };
__global__ void __launch_bounds__(kQsBlock) k_qs_mark(uint8_t* __restrict__ marks, double* __restrict__ scale, int nPoints, double r, int mode,
                                                       const QcDev* __restrict__ d, const smgpu_iter_stats* gate) {
    if (!qTraceRan(gate) || d->t.clean) return;
    const long long p0 = ((long long)blockIdx.x * kQsBlock + threadIdx.x) * 4;
    if (p0 >= nPoints) return;
    unsigned* const mw = reinterpret_cast<unsigned*>(marks) + (p0 >> 2);
    const unsigned w = *mw;
    if (mode == kQsFull || w) {
        for (int j = 0; j < 4; ++j) {
            const long long p = p0 + j;
            if (p >= nPoints) break;
            if (mode == kQsFull) scale[p] = 0.0;
            else if ((w >> (8 * j)) & 0xffu) scale[p] = (mode == kQsZero) ? 0.0 : scale[p] * r;
        }
    }
    if (w) *mw = 0u;
}

// One Jacobi sweep, one lane per point and trip: reads `in`, writes `out`.  The sum is a left fold from 0.0 over the pointPoints row in
// row order, the division one IEEE division (-ffp-contract=off: no contraction); a point with an empty row keeps its value.
__global__ void __launch_bounds__(kQsBlock) k_qs_sweep(MeshView m, const double* __restrict__ in, double* __restrict__ out, const QcDev* __restrict__ d,
                                                        const smgpu_iter_stats* gate) {
    if (!qTraceRan(gate) || d->t.clean) return;
    for (long long p = (long long)blockIdx.x * kQsBlock + threadIdx.x; p < m.nPoints; p += (long long)gridDim.x * kQsBlock) {
        const double s = in[p];
        const int b = m.ppOff[p], e = m.ppOff[p + 1];
        double v = s;
        if (e > b) {
            double sum = 0.0;
            for (int k = b; k < e; ++k) sum += in[m.ppPt[k]];
            const double t = 0.5 * s + 0.5 * (sum / (double)(e - b));
            v = t < s ? t : s;
        }
        out[p] = v;
    }
}

// The accepted points of the pass, one lane per point and trip: where s < 1 the point becomes x (s == 0) or x + s (L - x) per component;
// where s == 1 it is L already, with the loop's own bits (scales only fall within an iteration), and nothing but s is read.
// Counted for the record, which k_qs_verdict has reset: nPointsReverted (the accepted point == x and L != x), nPointsScaled
// (0 < s < 1 and L != x), one integer atomic per workgroup each, folded as k_tangle_apply folds its count; minScale, an integer
// atomic min on the bits of the non-negative double, one per workgroup that holds an s < 1.
__global__ void __launch_bounds__(kQsBlock) k_qs_apply(const double* __restrict__ x, const double* __restrict__ L, double* __restrict__ cur,
                                                        const double* __restrict__ scale, int nPoints, const QcDev* __restrict__ d,
                                                        smgpu_quality_constraint_record_scaled* __restrict__ rec, const smgpu_iter_stats* gate) {
    if (!qTraceRan(gate) || d->t.clean) return;
    const int tid = threadIdx.x;
    int reverted = 0, scaled = 0;
    unsigned long long minBits = kQsOneBits;
    for (long long p = (long long)blockIdx.x * kQsBlock + tid; p < nPoints; p += (long long)gridDim.x * kQsBlock) {
        const double s = scale[p];
        if (s < 1.0) {
            const V3 a = ldv(x, p), l = ldv(L, p);
            const V3 v = (s == 0.0) ? a : v3(a.x + s * (l.x - a.x), a.y + s * (l.y - a.y), a.z + s * (l.z - a.z));
            stv(cur, p, v);
            const bool moved = l.x != a.x || l.y != a.y || l.z != a.z;
            reverted += (moved && v.x == a.x && v.y == a.y && v.z == a.z) ? 1 : 0;
            scaled += (moved && s > 0.0) ? 1 : 0;
            const unsigned long long bits = (unsigned long long)__double_as_longlong(s);
            minBits = bits < minBits ? bits : minBits;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        reverted += __shfl_xor(reverted, o, 64);
        scaled += __shfl_xor(scaled, o, 64);
        const unsigned long long other = __shfl_xor(minBits, o, 64);
        minBits = other < minBits ? other : minBits;
    }
    __shared__ int waveReverted[kQsBlock / 64], waveScaled[kQsBlock / 64];
    __shared__ unsigned long long waveMin[kQsBlock / 64];
    if ((tid & 63) == 0) { waveReverted[tid >> 6] = reverted; waveScaled[tid >> 6] = scaled; waveMin[tid >> 6] = minBits; }
    __syncthreads();
    if (tid == 0) {
        int nR = 0, nS = 0;
        unsigned long long mn = kQsOneBits;
        for (int w = 0; w < kQsBlock / 64; ++w) { nR += waveReverted[w]; nS += waveScaled[w]; mn = waveMin[w] < mn ? waveMin[w] : mn; }
        if (nR > 0) atomicAdd(reinterpret_cast<unsigned long long*>(&rec->nPointsReverted), (unsigned long long)nR);
        if (nS > 0) atomicAdd(reinterpret_cast<unsigned long long*>(&rec->nPointsScaled), (unsigned long long)nS);
        if (mn < kQsOneBits) atomicMin(reinterpret_cast<unsigned long long*>(&rec->minScale), mn);
    }
}

}  // namespace smgpu
