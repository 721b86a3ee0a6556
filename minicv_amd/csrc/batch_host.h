// batch_host.h — what the RANSAC batches share on the host (host only): their statistics record's counted stream
// calls, the first-failure report, the device-free refusals, OpenCV's sample tables keyed by N and the hypothesis
// round driver. The per-thread, per-device workspace, the timer and the counted calls themselves
// are mcv_runtime.h's, shared with every other host driver; the index arithmetic is ransac_batch_index.h's.
#pragma once

#include "minicv_native.h"
#include "mcv_runtime.h"
#include "plan.h"
#include "ransac_batch_index.h"

#include <chrono>
#include <cstring>
#include <map>
#include <numeric>
#include <string>
#include <vector>

namespace mcv {

// A stream synchronisation / an asynchronous copy of a RANSAC batch, counted in batch_stats().
inline void batch_sync(hipStream_t s) { counted_sync(batch_stats(), s); }
inline void batch_copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    counted_copy(batch_stats(), dst, src, bytes, kind, s);
}

// A call starts its statistics afresh.
inline BatchStats& batch_stats_begin(int B) {
    BatchStats& stats = batch_stats();
    stats = BatchStats();
    stats.problems = B;
    return stats;
}

// A problem that fails returns zero outputs; the call names the first one in the last error.
struct BatchFailures {
    int first = -1;
    std::string msg;
    void note(int p, const std::string& m) {
        if (first < 0 || p < first) { first = p; msg = m; }
    }
    void report(const char* who) const {
        if (first < 0) {
            clear_last_error();
            return;
        }
        char buf[400];
        snprintf(buf, sizeof(buf), "%s: problem %d: %s", who, first, msg.c_str());
        set_last_error(buf);
    }
};

// The refusals every batch shares, none of which touches the device.
inline void check_batch_offsets(const char* who, const int* offsets, int B) {
    if (B < 0) fail("%s: negative B (%d)", who, B);
    int where = 0;
    const int bad = batch_check_offsets(offsets, B, &where);
    if (bad == 1) fail("%s: offsets[0] must be 0 (is %d)", who, offsets[0]);
    if (bad == 2) fail("%s: offsets decrease at problem %d (%d -> %d)", who, where, offsets[where], offsets[where + 1]);
}
// twoD: cvFindModelBatch, which also has LSQ / LMedS single calls to point away from and a 7-point flag
inline void check_batch_config(const char* who, const RansacConfig& cfg, bool twoD = false) {
    check_flags(cfg, who);
    if (cfg.method != MCV_METHOD_RANSAC)
        fail("%s: unsupported method %d (only MCV_METHOD_RANSAC%s)", who, cfg.method,
             twoD ? "; LSQ and LMedS have no batch form" : "");
    if (cfg.flags & MCV_FLAG_FUSED_ERROR) fail("%s: unsupported flag MCV_FLAG_FUSED_ERROR", who);
    if (cfg.flags & MCV_FLAG_FAST_MINIMAL) fail("%s: unsupported flag MCV_FLAG_FAST_MINIMAL", who);
    if (twoD && (cfg.flags & MCV_FLAG_SEVEN_POINT)) fail("%s: unsupported flag MCV_FLAG_SEVEN_POINT", who);
    if (cfg.deviceCount > 1) fail("%s: unsupported deviceCount %d (one GPU per call)", who, cfg.deviceCount);
    if (!(cfg.confidence > 0 && cfg.confidence < 1)) fail("%s: confidence must be in (0,1)", who);
}

// OpenCV's sample stream for a family without checkSubset (essential, PnP): one cv::RNG((uint64)-1) stream per
// problem, as each single call draws, so the rows depend on N alone. One table of `iters` rows of m per distinct N
// goes up in one copy; prob[d].rowOff = problem d's first row. Returns the device table, nullptr without
// MCV_FLAG_CV_SAMPLER (every rowOff stays 0).
inline const int* cv_tables_by_n(int model, const RansacConfig& cfg, std::vector<BatchProblem>& prob, int64_t iters,
                                 int m, PinnedBuf<int>& h_table, DevBuf<int>& table, hipStream_t s) {
    if (!cv_sampler(cfg)) return nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t rowInts = (size_t)iters * m;
    std::map<int, int64_t> byN;
    std::vector<int> rows, all;
    for (BatchProblem& P : prob) {
        auto it = byN.find(P.N);
        if (it == byN.end()) {
            cv_table_build(model, cfg, nullptr, P.N, iters, rows);
            it = byN.emplace(P.N, (int64_t)byN.size() * iters).first;
            all.insert(all.end(), rows.begin(), rows.begin() + (ptrdiff_t)rowInts);
        }
        P.rowOff = it->second;
    }
    h_table.ensure(all.size());
    table.ensure(all.size());
    std::memcpy(h_table.p, all.data(), all.size() * sizeof(int));
    batch_stats().tableUs = us_since(t0);
    batch_copy(table.p, h_table.p, all.size() * sizeof(int), hipMemcpyHostToDevice, s);
    return table.p;
}

// The hypothesis rounds of a RANSAC batch. A round holds the hypotheses [begin, begin + size) of every problem
// still searching (size: firstSize, then per), planned by batch_round; the grouping into rounds never changes a
// result, because the replay reads the counts in order. Per round, in this order: the descriptor table up, the
// family's launches, the counts back, one synchronisation, then per problem the single call's sequential replay
// on the host. st: the replay states, left as the search ended (bestIndex < 0: no model).
//
// A family F (no virtual functions; the driver is instantiated per family) has
//   F.W.h_desc / F.W.desc       the pinned and the device descriptor table, sized here (BatchDesc, or a struct that
//                               holds one: F.desc(j, d) is the BatchDesc of entry j, which describes problem d)
//   F.W.h_counts / F.W.counts   the counts of a round, F.slots per slot, sized by launch()
//   F.slots                     counts per hypothesis (models a minimal sample can yield)
//   F.launch(active, R, s)      sizes the round's buffers, fills and uploads its own tables, generate + sweep
//   F.confidence(d)             device problem d's confidence
//   F.best_changed(changed, s)  after the round's replays, when some problems have a new best: queue what must
//                               leave the round's buffers before the next round reuses them
struct BestChange {   // entry j of the round (device problem d) has a new best: count `slot` of its slots this round
    size_t j;
    int d;
    int64_t slot;
};
template <class Family>
void batch_rounds(Family& F, const std::vector<BatchProblem>& prob, std::vector<mcvReplayState>& st, int maxIters,
                  int64_t firstSize, int64_t per, int m, bool fixed, hipStream_t s) {
    BatchStats& stats = batch_stats();
    st.resize(prob.size());
    for (auto& x : st) mcvReplayInit(&x, maxIters);
    F.W.desc.ensure(prob.size());
    F.W.h_desc.ensure(prob.size());
    std::vector<int> active(prob.size());
    std::iota(active.begin(), active.end(), 0);
    std::vector<BestChange> changed;
    int64_t size = firstSize;
    for (int64_t begin = 0;; begin += size, size = per) {
        const BatchRound R = batch_round(prob.data(), st.data(), active, begin, size,
                                         [&](size_t j, int d) -> BatchDesc& { return F.desc(j, d); });
        if (R.n == 0) break;
        const size_t n = (size_t)R.n;
        batch_copy(F.W.desc.p, F.W.h_desc.p, n * sizeof(*F.W.h_desc.p), hipMemcpyHostToDevice, s);
        F.launch(active, R, s);
        batch_copy(F.W.h_counts.p, F.W.counts.p, n * (size_t)R.stride * F.slots * sizeof(int), hipMemcpyDeviceToHost,
                   s);
        batch_sync(s);
        ++stats.rounds;
        stats.problemRounds += (long long)n;
        changed.clear();
        for (size_t j = 0; j < n; ++j) {
            const int d = active[j];
            const BatchDesc& X = F.desc(j, d);
            const int* counts = F.W.h_counts.p + X.slotOff * F.slots;
            const int64_t before = st[d].bestIndex;
            const double conf = F.confidence(d);
            if (F.slots == 1) mcvReplayChunk(&st[d], counts, begin, X.hypCount, X.N, m, conf, fixed ? 1 : 0);
            else mcvReplayChunkModels(&st[d], counts, begin, X.hypCount, F.slots, X.N, m, conf, fixed ? 1 : 0);
            if (begin + X.hypCount >= st[d].niters) st[d].stopped = 1;
            if (st[d].bestIndex != before) changed.push_back(BestChange{j, d, st[d].bestIndex - begin * F.slots});
        }
        if (!changed.empty()) F.best_changed(changed, s);
    }
}

}  // namespace mcv
