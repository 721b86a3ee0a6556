// pnp_refine_batch_index.h — the index arithmetic of the batched PnP refinement (cvRefinePnPBatch,
// cvSolvePnPRansacRefineBatch): the check of the problem sizes, each problem's selected rows, its
// place in the compact (gathered) point array, the refusal reasons and the table of the problems that run.
// Plain C++ without the HIP runtime: the exports (ransac_batch_pnp_host.cpp), the layout hook
// (mcvHostRefinePnPBatchLayout) and the stand-alone sanitizer program (tests/asan/pnp_refine_batch_asan_main.cpp)
// read the same copy.
//
// Index spaces of a call:
//   row      [offsets[p], offsets[p+1]) of the caller's segmented arrays and of the mask
//   compact  [compOff[p], compOff[p] + counts[p]) of the gathered array: the selected rows of problem p in
//            index order, the problems in order, nothing padded; compOff[B] = all selected rows
//   job      the problems that run (at least kRefineMinRows selected rows, a usable camera), in order: job j
//            reduces over its problem's compact rows, or over its rows when the call has no mask
#pragma once

#include "ransac_batch_index.h"   // batch_check_offsets: the one check of the offsets

#include <cstdint>

namespace mcv {

static const int kRefineMinRows = 3;   // cvRefinePnPLM / cvRefinePnPVVS refuse fewer

// The check of the offsets under this header's name: batch_check_offsets itself (0 fine, 1 offsets[0] != 0,
// 2 offsets[*where + 1] < offsets[*where]).
inline int refine_batch_check_offsets(const int* offsets, int B, int* where) {
    return batch_check_offsets(offsets, B, where);
}

// The first problem with more than `limit` rows, or -1.
inline int refine_batch_check_sizes(const int* offsets, int B, int limit) {
    for (int p = 0; p < B; ++p)
        if (offsets[p + 1] - offsets[p] > limit) return p;
    return -1;
}

// counts[p] = selected rows of problem p (any non-zero mask byte selects; a null mask selects every row),
// compOff[B + 1] = their exclusive prefix sum. Returns the largest count. Over checked offsets.
inline int refine_batch_layout(const int* offsets, int B, const uint8_t* mask, int* counts, int* compOff) {
    int total = 0, largest = 0;
    for (int p = 0; p < B; ++p) {
        int c = 0;
        if (mask) {
            for (int i = offsets[p]; i < offsets[p + 1]; ++i) c += mask[i] != 0 ? 1 : 0;
        } else {
            c = offsets[p + 1] - offsets[p];
        }
        counts[p] = c;
        compOff[p] = total;
        total += c;   // <= offsets[B]: fits an int
        if (c > largest) largest = c;
    }
    compOff[B] = total;
    return largest;
}

// Why problem p does not run: 0 it runs, 1 fewer than kRefineMinRows selected rows, 2 its camera is refused.
enum { kRefineRuns = 0, kRefineTooFew = 1, kRefineBadCamera = 2 };
inline int refine_batch_reason(int count, bool cameraOk) {
    if (count < kRefineMinRows) return kRefineTooFew;   // the single call checks N before the camera
    return cameraOk ? kRefineRuns : kRefineBadCamera;
}

// The job table: the problems with reason[p] == kRefineRuns, in order. A job reduces over the rows
// [ptOff, ptOff + N) of the array its points sit in: the compact one (gathered: ptOff = compOff[p]) or,
// without a mask, the caller's own rows (ptOff = offsets[p]; then counts[p] is the whole slice).
// Returns nJobs; *largest = the largest job's N (sizes a step's grid).
struct RefineBatchJob {
    int prob, ptOff, N;
};
inline int refine_batch_jobs(const int* offsets, int B, const int* counts, const int* compOff, const int* reason,
                             bool gathered, RefineBatchJob* jobs, int* largest) {
    int n = 0, big = 0;
    for (int p = 0; p < B; ++p) {
        if (reason[p] != kRefineRuns) continue;
        jobs[n].prob = p;
        jobs[n].ptOff = gathered ? compOff[p] : offsets[p];
        jobs[n].N = counts[p];
        if (counts[p] > big) big = counts[p];
        ++n;
    }
    *largest = big;
    return n;
}

}  // namespace mcv
