// ransac_batch_index.h — the index arithmetic of the batched RANSAC calls (cvFindModelBatch, the essential
// batches, the PnP batches): the check of the offsets, the layout of a call and the plan of one
// hypothesis round. Plain C++ without the HIP runtime: the exports (through batch_host.h's round driver), the
// hooks (mcvHostBatchLayout, mcvHostBatchRound) and the stand-alone sanitizer program
// (tests/asan/ransac_batch_index_asan_main.cpp) read the same copy.
//
// Index spaces of a call:
//   problem  p in [0, B): the caller's; its points are [offsets[p], offsets[p+1]), nothing padded
//   device   d in [0, D): the problems that run on the device (more points than the sample size), in order
//   round    j in [0, n): the device problems still searching, compacted in order; problem j owns the slots
//            [j stride, j stride + hypCount) of the round's buffers, stride = the round's largest hypCount
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace mcv {

// Slots (problem x hypothesis) one round of cvFindModelBatch may hold. 2^21 slots are 151 MB of fundamental
// models (72 B), 64 MB of homography models, 8 MB of counts: B = 1024 problems of the default 2000 iterations
// fit one round. Above it every round gives each problem cap / problems hypotheses (at least one).
static const int64_t kBatchSlotCap = (int64_t)1 << 21;

struct BatchDesc {      // one problem of a hypothesis round, as the kernels read it
    int ptOff, N;            // its points: [ptOff, ptOff + N) of the segmented buffer
    int hypBegin, hypCount;  // its hypotheses of this round
    int64_t slotOff;         // its first slot in the round's model / count buffers
    int64_t rowOff;          // its first row of the sampler table (MCV_FLAG_CV_SAMPLER)
};

// 0: fine; 1: offsets[0] != 0; 2: offsets[*where + 1] < offsets[*where]
inline int batch_check_offsets(const int* offsets, int B, int* where) {
    if (offsets[0] != 0) return 1;
    for (int p = 0; p < B; ++p)
        if (offsets[p + 1] < offsets[p]) {
            *where = p;
            return 2;
        }
    return 0;
}

// The layout of a call (mcvHostBatchLayout exposes it). Problems with more points than the sample size m go
// to the device; they are numbered in order (device index d).
//   slot offset   d * per, 64-bit: problem d's first slot of a round in which every device problem runs
//   row offset    d * iters: its first row of a sampler table with one block of rows per problem
//   per           hypotheses per problem per round = clamp(cap / D, 1, iters); rounds = ceil(iters / per)
struct BatchLayout {
    std::vector<int> dev;             // device problems
    std::vector<int64_t> slotOff, rowOff;   // per problem (-1: not on the device)
    int64_t iters = 1, per = 1, rounds = 0;
};
inline void batch_layout(const int* offsets, int B, int m, int maxIters, int64_t cap, BatchLayout& L) {
    L.dev.clear();
    L.slotOff.assign((size_t)B, -1);
    L.rowOff.assign((size_t)B, -1);
    L.iters = std::max(maxIters, 1);
    for (int p = 0; p < B; ++p)
        if (offsets[p + 1] - offsets[p] > m) L.dev.push_back(p);
    const int64_t D = (int64_t)L.dev.size();
    if (cap < 1) cap = kBatchSlotCap;
    L.per = D ? std::min(std::max<int64_t>(cap / D, 1), L.iters) : L.iters;
    L.rounds = D ? (L.iters + L.per - 1) / L.per : 0;
    for (int64_t d = 0; d < D; ++d) {
        L.slotOff[(size_t)L.dev[(size_t)d]] = d * L.per;
        L.rowOff[(size_t)L.dev[(size_t)d]] = d * L.iters;
    }
}

struct BatchProblem {   // a device problem, for the whole call
    int ptOff, N;
    int64_t rowOff;
};
struct BatchRound { int n, stride; };

// The plan of one round: the hypotheses [begin, begin + size) of every problem of `active` (device indices,
// ascending) that still searches. st[d].niters / st[d].stopped: problem d's replay state (mcvReplayState); a
// stopped problem, or one whose budget ends at or before begin, drops out. desc(j, d) (a BatchDesc&) is entry j
// of the round's table, which describes device problem d; `active` receives the round's device indices.
template <class State, class DescAt>
BatchRound batch_round(const BatchProblem* prob, const State* st, std::vector<int>& active, int64_t begin, int64_t size,
                       DescAt desc) {
    BatchRound R{0, 0};
    for (int d : active) {
        const int64_t left = (int64_t)st[d].niters - begin;
        if (st[d].stopped || left <= 0) continue;
        BatchDesc& X = desc((size_t)R.n, d);
        X.ptOff = prob[d].ptOff;
        X.N = prob[d].N;
        X.hypBegin = (int)begin;
        X.hypCount = (int)std::min(left, size);
        X.rowOff = prob[d].rowOff;
        R.stride = std::max(R.stride, X.hypCount);
        active[(size_t)R.n++] = d;   // in place: R.n never passes the entry being read
    }
    active.resize((size_t)R.n);
    for (int j = 0; j < R.n; ++j) desc((size_t)j, active[(size_t)j]).slotOff = (int64_t)j * R.stride;
    return R;
}

}  // namespace mcv
