// kernels_quality_guard.hpp -- the guard on the quality history (smgpu_set_quality_guard: include/smgpu.h, DESIGN.md "Mesh
// quality", 10.11): a verdict on every trace record, taken on the device, and a snapshot of the last state that passed.
//
// Behind k_quality_trace_final of every traced iteration the engine queues, on its own stream,
//   1. k_quality_guard_verdict: one wave compares the counts of the record with the baseline's (integers only: the host can repeat
//      every verdict from the records), writes the verdict word and, on a trip, the reasons, the iteration, a copy of the record
//      and the loop's stop word -- every kernel queued behind it is then the no-op the stop by relTol makes it;
//   2. k_quality_guard_snapshot: when the verdict is "good", a streaming copy of the per-point state that an iteration carries to
//      the next one (the points; the layer normals when layers are set) into the guard's own buffers.
// Both take the trace's gate (qTraceRan): an iteration that did not run gets the verdict "none" and leaves the snapshot alone.
#pragma once
#include "kernels_quality_trace.hpp"

namespace smgpu {

enum : int { kGuardNone = 0, kGuardGood = 1, kGuardTripped = 2 };

// the guard's device record
struct GuardDev {
    smgpu_quality_trace_record baseline;   // the trace's record of the points at arming (iteration 0)
    smgpu_quality_trace_record tripRecord;
    long long snapshotIteration, trippedIteration;
    unsigned reasons;
    int verdict;                           // of the latest traced iteration: kGuardNone / kGuardGood / kGuardTripped
    int tripped;
};

__global__ void __launch_bounds__(64) k_quality_guard_verdict(const smgpu_quality_trace_record* __restrict__ rec, GuardDev* __restrict__ g, unsigned criteria,
                                                               int* __restrict__ stop, const smgpu_iter_stats* gate) {
    if (threadIdx.x != 0) return;
    if (!qTraceRan(gate) || g->tripped) { g->verdict = kGuardNone; return; }
    unsigned reasons = 0;
    if ((criteria & SMGPU_GUARD_NONPOSITIVE_VOLUME) && rec->nNonPositiveVolume > g->baseline.nNonPositiveVolume) reasons |= SMGPU_GUARD_NONPOSITIVE_VOLUME;
    if ((criteria & SMGPU_GUARD_WRONG_ORIENTED) && rec->nWrongOrientedFaces > g->baseline.nWrongOrientedFaces) reasons |= SMGPU_GUARD_WRONG_ORIENTED;
    if ((criteria & SMGPU_GUARD_ERROR_NONORTH) && rec->nErrorNonOrth > g->baseline.nErrorNonOrth) reasons |= SMGPU_GUARD_ERROR_NONORTH;
    if (!reasons) { g->verdict = kGuardGood; return; }
    g->verdict = kGuardTripped;
    g->tripped = 1;
    g->reasons = reasons;
    g->trippedIteration = rec->iteration;
    g->tripRecord = *rec;
    *stop = 1;
}

// 16 bytes per lane per access, kGuardPer accesses per lane and array in flight, every load issued before the first store; a lane
// past the end loads the last pair again (in bounds) and stores nothing.  The odd double of the tail goes with lane 0.
constexpr int kGuardBlock = 256;
constexpr int kGuardPer = 4;
// n doubles (src and dst 16-byte aligned: whole allocations) from src0 to dst0 and, with TWO, from src1 to dst1
template <bool TWO>
__global__ void __launch_bounds__(kGuardBlock) k_quality_guard_snapshot(const double* __restrict__ src0, double* __restrict__ dst0, const double* __restrict__ src1,
                                                                         double* __restrict__ dst1, long long n, long long iteration, GuardDev* __restrict__ g,
                                                                         int needGood) {
    if (needGood && g->verdict != kGuardGood) return;
    const long long nPair = n >> 1;
    const long long base = (long long)blockIdx.x * (kGuardBlock * kGuardPer) + threadIdx.x;
    if (nPair > 0) {
        const double2* __restrict__ s0 = reinterpret_cast<const double2*>(src0);
        const double2* __restrict__ s1 = reinterpret_cast<const double2*>(src1);
        double2 a0, a1, a2, a3, b0, b1, b2, b3;
        const long long i0 = base, i1 = base + kGuardBlock, i2 = base + 2 * kGuardBlock, i3 = base + 3 * kGuardBlock, last = nPair - 1;
        a0 = s0[i0 < nPair ? i0 : last]; a1 = s0[i1 < nPair ? i1 : last]; a2 = s0[i2 < nPair ? i2 : last]; a3 = s0[i3 < nPair ? i3 : last];
        if (TWO) { b0 = s1[i0 < nPair ? i0 : last]; b1 = s1[i1 < nPair ? i1 : last]; b2 = s1[i2 < nPair ? i2 : last]; b3 = s1[i3 < nPair ? i3 : last]; }
        double2* __restrict__ d0 = reinterpret_cast<double2*>(dst0);
        double2* __restrict__ d1 = reinterpret_cast<double2*>(dst1);
        if (i0 < nPair) d0[i0] = a0;
        if (i1 < nPair) d0[i1] = a1;
        if (i2 < nPair) d0[i2] = a2;
        if (i3 < nPair) d0[i3] = a3;
        if (TWO) {
            if (i0 < nPair) d1[i0] = b0;
            if (i1 < nPair) d1[i1] = b1;
            if (i2 < nPair) d1[i2] = b2;
            if (i3 < nPair) d1[i3] = b3;
        }
    }
    static_assert(kGuardPer == 4, "the four accesses are written out");
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (n & 1) {
            dst0[n - 1] = src0[n - 1];
            if (TWO) dst1[n - 1] = src1[n - 1];
        }
        if (iteration >= 0) g->snapshotIteration = iteration;
    }
}

}  // namespace smgpu
