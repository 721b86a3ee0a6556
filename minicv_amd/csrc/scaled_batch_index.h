// scaled_batch_index.h — the index arithmetic of the batched findScaled (cvFindScaledPoseBatch): the
// checks of the observation sets' CSR and of setIdx, each problem's place in the row, candidate and
// block spaces, and the sweep's work list. Plain C++ without the HIP runtime: the exports
// (scaled_batch_host.cpp), the kernels (scaled_batch.hip) and the stand-alone sanitizer program
// (tests/asan/scaled_batch_asan_main.cpp) read the same copy.
#pragma once

namespace mcv {

static const int kScaledBatchCands = 64;              // candidate scales per block of the sweep
static const long long kScaledBatchMax = 1ll << 28;   // cap of offsets[S] and of the candidates of a call

// One problem of a batch: observation rows [rowOff, rowOff + N) of its set, candidates
// [candOff, candOff + 2 N) of the per-candidate arrays (the layout of cvFindScaledPoseBatchCosts),
// blocks [blockOff, blockOff + ceil(2 N / kScaledBatchCands)) of the work list.
struct ScaledBatchProb {
    int rowOff, N, candOff, blockOff;
};

// 0: fine; 1: offsets[0] != 0; 2: offsets[*where + 1] < offsets[*where]
inline int scaled_batch_check_offsets(const int* offsets, int S, int* where) {
    if (offsets[0] != 0) return 1;
    for (int s = 0; s < S; ++s)
        if (offsets[s + 1] < offsets[s]) {
            *where = s;
            return 2;
        }
    return 0;
}

// The first problem whose set lies outside [0, S), or -1. A null setIdx means set p: the caller
// has checked S == P.
inline int scaled_batch_check_sets(const int* setIdx, int P, int S) {
    if (!setIdx) return -1;
    for (int p = 0; p < P; ++p)
        if (setIdx[p] < 0 || setIdx[p] >= S) return p;
    return -1;
}

inline int scaled_batch_blocks(int N) { return (int)((2ll * N + kScaledBatchCands - 1) / kScaledBatchCands); }

// Fills probs[P] over checked offsets / setIdx with offsets[S] <= kScaledBatchMax. Returns false, with
// probs partly filled, once the candidates pass kScaledBatchMax (every stored offset still fits an int).
inline bool scaled_batch_layout(const int* offsets, const int* setIdx, int P, ScaledBatchProb* probs,
                                long long* totalCands, long long* totalBlocks, int* nonEmpty) {
    long long cands = 0, blocks = 0;
    int live = 0;
    for (int p = 0; p < P; ++p) {
        const int s = setIdx ? setIdx[p] : p;
        const int N = offsets[s + 1] - offsets[s];
        probs[p].rowOff = offsets[s];
        probs[p].N = N;
        probs[p].candOff = (int)cands;
        probs[p].blockOff = (int)blocks;
        cands += 2ll * N;
        if (cands > kScaledBatchMax) return false;
        blocks += scaled_batch_blocks(N);
        live += N > 0 ? 1 : 0;
    }
    *totalCands = cands;
    *totalBlocks = blocks;
    *nonEmpty = live;
    return true;
}

// blockProb[totalBlocks]: the problem of every block; an empty problem contributes none.
inline void scaled_batch_work_list(const ScaledBatchProb* probs, int P, int* blockProb) {
    for (int p = 0; p < P; ++p) {
        const int nb = scaled_batch_blocks(probs[p].N);
        for (int b = 0; b < nb; ++b) blockProb[probs[p].blockOff + b] = p;
    }
}

}  // namespace mcv
