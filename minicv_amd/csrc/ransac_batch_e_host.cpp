// ransac_batch_e_host.cpp — cvFindEssentialMatBatch / cvRecoverPoseBatch: B independent cvFindEssentialMat /
// cvRecoverPose problems in one call whose kernel launches and stream synchronisations do not grow with B
// (DESIGN.md §7f).
//
//   all points -> one segmented buffer of raw pixel pairs, one H2D copy, one batched pack to double4
//                 (x - pp) / focal with each problem's focal and principal point
//   rounds:   the single call's three generate kernels in their batch form (ransac_e5.hip) + the batched
//             sweep over every problem still searching, one copy of the counts back, the single call's
//             sequential replay per problem on the host (mcvReplayChunkModels, its own confidence); the
//             problems whose best model changed get it copied out of their dense region before the next
//             round overwrites it
//   finalize: every winner masked and counted in one launch, one copy back
//   pose:     e_decompose per problem on the host, the cheirality counts of all of them in one launch, one
//             copy back, then e_recover's first-maximum rule per problem
// E has no refit and no refine: the winner is the minimal-sample model as solved, so every problem returns
// the single call's bits. Problems with exactly 5 correspondences take the single export (routed through it).
#include "minicv_native.h"
#include "mcv_runtime.h"
#include "kernels.h"
#include "hyp_essential.h"
#include "plan.h"

#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include <memory>
#include <algorithm>
#include <chrono>

namespace mcv {

namespace {

static const int64_t kBatchEFirstRound = 256;          // hypotheses per problem of an adaptive batch's first round
static const int64_t kBatchEFirstMinHyps = 1 << 16;    // ... from this many hypotheses in a full round on

struct EProblem {   // what differs between the problems of one call
    double focal;
    mcvV2d pp;
    double thrPix;       // threshold in pixels
    double confidence;
};

struct BatchEWs {
    int device = 0;
    hipStream_t stream = nullptr;
    DevBuf<double> raw, pts, best;
    DevBuf<uint8_t> stage, dense, mask;
    DevBuf<int> table, dslot, ndense, counts, found, cnt, good;
    DevBuf<BatchDesc> desc;
    DevBuf<BatchEPack> pack;
    DevBuf<BatchESweep> sweep;
    DevBuf<BatchEFetch> fetch;
    DevBuf<BatchEFin> fin;
    DevBuf<BatchEPose> pose;
    PinnedBuf<double> h_raw, h_best;
    PinnedBuf<uint8_t> h_mask;
    PinnedBuf<int> h_table, h_counts, h_found, h_cnt, h_good;
    PinnedBuf<BatchDesc> h_desc;
    PinnedBuf<BatchEPack> h_pack;
    PinnedBuf<BatchESweep> h_sweep;
    PinnedBuf<BatchEFetch> h_fetch;
    PinnedBuf<BatchEFin> h_fin;
    PinnedBuf<BatchEPose> h_pose;
    ~BatchEWs() {
        if (stream) (void)hipStreamDestroy(stream);
    }
};

BatchEWs& thread_batch_e_ws() {
    int dev = 0;
    MCV_HIP(hipGetDevice(&dev));
    thread_local std::vector<std::unique_ptr<BatchEWs>> all;
    for (auto& w : all)
        if (w->device == dev) return *w;
    all.emplace_back(new BatchEWs());
    all.back()->device = dev;
    MCV_HIP(hipStreamCreateWithFlags(&all.back()->stream, hipStreamNonBlocking));
    return *all.back();
}

long long us_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
}

void batch_e_sync(hipStream_t s) {
    MCV_HIP(hipGetLastError());
    MCV_HIP(hipStreamSynchronize(s));
    ++batch_stats().syncs;
}

// Everything a call can be refused for without touching the device (cfg: one for all problems; the
// per-problem confidences are checked by the caller).
void batch_e_check(const char* who, const int* offsets, int B, const RansacConfig& cfg) {
    if (B < 0) fail("%s: negative B (%d)", who, B);
    if (offsets[0] != 0) fail("%s: offsets[0] must be 0 (is %d)", who, offsets[0]);
    for (int p = 0; p < B; ++p)
        if (offsets[p + 1] < offsets[p])
            fail("%s: offsets decrease at problem %d (%d -> %d)", who, p, offsets[p], offsets[p + 1]);
    check_flags(cfg, who);
    if (cfg.method != MCV_METHOD_RANSAC) fail("%s: unsupported method %d (only MCV_METHOD_RANSAC)", who, cfg.method);
    if (cfg.flags & MCV_FLAG_FUSED_ERROR) fail("%s: unsupported flag MCV_FLAG_FUSED_ERROR", who);
    if (cfg.flags & MCV_FLAG_FAST_MINIMAL) fail("%s: unsupported flag MCV_FLAG_FAST_MINIMAL", who);
    if (cfg.deviceCount > 1) fail("%s: unsupported deviceCount %d (one GPU per call)", who, cfg.deviceCount);
    if (!(cfg.confidence > 0 && cfg.confidence < 1)) fail("%s: confidence must be in (0,1)", who);
}

// The call. pose == false: cvFindEssentialMatBatch (M = E, counts = inliers); pose == true:
// cvRecoverPoseBatch (M = R, t, counts = cvRecoverPose's return). cfg: flags, maxIters, seed for all;
// thresholds and confidences per problem. single(p): the single export on problem p (N == 5).
template <class Single>
int e_batch(const char* who, bool pose, const mcvV2d* a, const mcvV2d* b, const int* offsets, int B,
            const std::vector<EProblem>& pr, const RansacConfig& cfg, mcvM33d* M, mcvV3d* t, uint8_t* mask,
            int* counts, Single single) {
    BatchStats& stats = batch_stats();
    stats = BatchStats();
    stats.problems = B;
    if (B == 0) return 0;
    const int total = offsets[B];
    std::memset(M, 0, (size_t)B * sizeof(mcvM33d));
    if (t) std::memset(t, 0, (size_t)B * sizeof(mcvV3d));
    std::memset(counts, 0, (size_t)B * sizeof(int));
    if (mask) std::memset(mask, 0, (size_t)total);
    require_device();

    const int m = 5, slots = kEModelSlots;
    const bool fixed = (cfg.flags & MCV_FLAG_FIXED_ITERS) != 0;
    const int kind = e_kind(cfg);
    int firstFail = -1;
    std::string firstMsg;
    auto failed = [&](int p, const std::string& msg) {
        if (firstFail < 0 || p < firstFail) { firstFail = p; firstMsg = msg; }
    };
    int ok = 0;

    BatchLayout L;
    batch_layout(offsets, B, m, cfg.maxIters, batch_cap_essential(), L);
    // the problems that never reach the device: too few points, exactly the sample size, a bad focal
    std::vector<int> dev;   // device problems, in order
    for (int p = 0; p < B; ++p) {
        const int N = offsets[p + 1] - offsets[p];
        char buf[200];
        if (N < m) {
            snprintf(buf, sizeof(buf), "need at least %d correspondences (N=%d)", m, N);
            failed(p, buf);
        } else if (N == m) {
            ++stats.single;
            std::string msg;
            if (single(p, msg)) ++ok;
            else {
                failed(p, msg);
                std::memset(M[p].M, 0, sizeof(mcvM33d));
                if (t) std::memset(&t[p], 0, sizeof(mcvV3d));
                counts[p] = 0;
                if (mask) std::memset(mask + offsets[p], 0, (size_t)N);
            }
        } else if (!(pr[(size_t)p].focal != 0) || !std::isfinite(pr[(size_t)p].focal)) {
            snprintf(buf, sizeof(buf), "focal length must be finite and non-zero (got %g)", pr[(size_t)p].focal);
            failed(p, buf);
        } else {
            dev.push_back(p);
        }
    }
    const size_t D = dev.size();
    if (D) {
        BatchEWs& W = thread_batch_e_ws();
        hipStream_t s = W.stream;
        // ---- points: the raw pixel pairs (a then b) in one copy, normalised by one launch
        auto t0 = std::chrono::steady_clock::now();
        W.h_raw.ensure((size_t)total * 4);
        W.raw.ensure((size_t)total * 4);
        W.pts.ensure((size_t)total * 4);
        std::memcpy(W.h_raw.p, a, (size_t)total * sizeof(mcvV2d));
        std::memcpy(W.h_raw.p + 2 * (size_t)total, b, (size_t)total * sizeof(mcvV2d));
        W.h_pack.ensure(D);
        W.pack.ensure(D);
        std::vector<float> thr2(D);
        int maxN = 0;
        for (size_t d = 0; d < D; ++d) {
            const int p = dev[d];
            const EProblem& X = pr[(size_t)p];
            W.h_pack.p[d] = BatchEPack{offsets[p], offsets[p + 1] - offsets[p], X.focal, X.pp.X, X.pp.Y};
            const double thr = X.thrPix / ((X.focal + X.focal) / 2);   // e_find: threshold /= (fx + fy) / 2
            thr2[d] = (float)(thr * thr);
            maxN = std::max(maxN, offsets[p + 1] - offsets[p]);
        }
        stats.packUs = us_since(t0);
        MCV_HIP(hipMemcpyAsync(W.raw.p, W.h_raw.p, (size_t)total * 4 * sizeof(double), hipMemcpyHostToDevice, s));
        MCV_HIP(hipMemcpyAsync(W.pack.p, W.h_pack.p, D * sizeof(BatchEPack), hipMemcpyHostToDevice, s));
        launch_batch_e_pack(W.raw.p, W.raw.p + 2 * (size_t)total, W.pack.p, (int)D, maxN, W.pts.p, s);
        ++stats.launches;
        // ---- OpenCV's sample stream: one cv::RNG((uint64)-1) stream per problem, as each single call draws.
        // EMEstimatorCallback has no checkSubset, so the rows depend on N alone: one table per distinct N.
        const int* d_table = nullptr;
        std::vector<int64_t> rowOff(D, 0);
        if (cv_sampler(cfg)) {
            t0 = std::chrono::steady_clock::now();
            const size_t rowInts = (size_t)L.iters * m;
            std::map<int, int64_t> byN;
            std::vector<int> rows, all;
            for (size_t d = 0; d < D; ++d) {
                const int N = W.h_pack.p[d].N;
                auto it = byN.find(N);
                if (it == byN.end()) {
                    cv_table_build(MCV_MODEL_ESSENTIAL, cfg, nullptr, N, L.iters, rows);
                    it = byN.emplace(N, (int64_t)byN.size() * L.iters).first;
                    all.insert(all.end(), rows.begin(), rows.begin() + (ptrdiff_t)rowInts);
                }
                rowOff[d] = it->second;
            }
            W.h_table.ensure(all.size());
            W.table.ensure(all.size());
            std::memcpy(W.h_table.p, all.data(), all.size() * sizeof(int));
            stats.tableUs = us_since(t0);
            MCV_HIP(hipMemcpyAsync(W.table.p, W.h_table.p, all.size() * sizeof(int), hipMemcpyHostToDevice, s));
            d_table = W.table.p;
        }
        // ---- hypothesis rounds
        std::vector<mcvReplayState> st(D);
        for (auto& x : st) mcvReplayInit(&x, cfg.maxIters);
        std::vector<size_t> active(D);
        for (size_t d = 0; d < D; ++d) active[d] = d;
        std::vector<int> stamp(D, 0);   // the round (1-based) whose fetch holds problem d's best model
        W.desc.ensure(D);
        W.h_desc.ensure(D);
        W.sweep.ensure(D);
        W.h_sweep.ensure(D);
        W.fetch.ensure(D);
        W.h_fetch.ensure(D);
        W.ndense.ensure(D);
        W.best.ensure(D * 9);
        W.h_best.ensure(D * 9);
        W.found.ensure(D);
        W.h_found.ensure(D);
        MCV_HIP(hipMemsetAsync(W.best.p, 0, D * 9 * sizeof(double), s));
        MCV_HIP(hipMemsetAsync(W.found.p, 0, D * sizeof(int), s));
        int round = 0;
        // Adaptive problems at moderate outlier ratios stop after roughly a hundred hypotheses, and the generate
        // is most of the device time, so a large adaptive batch starts with a round of
        // kBatchEFirstRound hypotheses per problem and runs the rest of the budget only for the problems that
        // need it: at most one round more, whatever B is. The replay reads the counts in order, so the grouping
        // into rounds never changes a result. Small batches keep one round: below kBatchEFirstMinHyps
        // hypotheses the generate sits on its latency floor and a second round would only add to it.
        int64_t size = L.per;
        if (!fixed && (int64_t)D * L.per >= kBatchEFirstMinHyps) size = std::min(L.per, kBatchEFirstRound);
        for (int64_t begin = 0; !active.empty(); begin += size, size = L.per) {
            // a round holds the hypotheses [begin, begin + size) of every problem still searching; the
            // problems are compacted, so problem j of the round owns stage columns [j stride, j stride + count)
            std::vector<size_t> run;
            int stride = 0;
            for (size_t d : active) {
                const int64_t left = (int64_t)st[d].niters - begin;
                if (st[d].stopped || left <= 0) continue;
                BatchDesc& X = W.h_desc.p[run.size()];
                X.ptOff = W.h_pack.p[d].ptOff;
                X.N = W.h_pack.p[d].N;
                X.hypBegin = (int)begin;
                X.hypCount = (int)std::min<int64_t>(left, size);
                X.rowOff = rowOff[d];
                stride = std::max(stride, X.hypCount);
                run.push_back(d);
            }
            active.swap(run);
            if (active.empty()) break;
            ++round;
            const size_t n = active.size();
            const size_t cols = n * (size_t)stride;
            for (size_t j = 0; j < n; ++j) {
                BatchDesc& X = W.h_desc.p[j];
                X.slotOff = (int64_t)j * stride;
                W.h_sweep.p[j] = BatchESweep{X.ptOff, X.N, X.slotOff * slots, X.slotOff * slots, thr2[active[j]], 0};
            }
            W.stage.ensure(e5_stage_bytes((int)cols));
            W.dense.ensure(cols * slots * sizeof(EModel));
            W.dslot.ensure(cols * slots);
            W.counts.ensure(cols * slots);
            W.h_counts.ensure(cols * slots);
            MCV_HIP(hipMemcpyAsync(W.desc.p, W.h_desc.p, n * sizeof(BatchDesc), hipMemcpyHostToDevice, s));
            MCV_HIP(hipMemcpyAsync(W.sweep.p, W.h_sweep.p, n * sizeof(BatchESweep), hipMemcpyHostToDevice, s));
            {
                ProfScope pg("batch_e_generate", s);
                stats.launches += launch_e5_batch_generate(W.pts.p, W.desc.p, (int)n, stride, cfg.seed, d_table,
                                                           W.dense.p, W.dslot.p, W.ndense.p, W.counts.p, W.stage.p, s);
            }
            {
                ProfScope ps("batch_e_sweep", s);
                launch_batch_e_sweep(kind, W.pts.p, W.sweep.p, (int)n, stride * slots, W.dense.p, W.dslot.p,
                                     W.ndense.p, W.counts.p, s);
            }
            ++stats.launches;
            MCV_HIP(hipMemcpyAsync(W.h_counts.p, W.counts.p, cols * slots * sizeof(int), hipMemcpyDeviceToHost, s));
            batch_e_sync(s);
            ++stats.rounds;
            stats.problemRounds += (long long)n;
            size_t nFetch = 0;
            for (size_t j = 0; j < n; ++j) {
                const size_t d = active[j];
                const BatchDesc& X = W.h_desc.p[j];
                const int64_t before = st[d].bestIndex;
                mcvReplayChunkModels(&st[d], W.h_counts.p + (size_t)X.slotOff * slots, begin, X.hypCount, slots, X.N, m,
                                     pr[(size_t)dev[d]].confidence, fixed ? 1 : 0);
                if (begin + X.hypCount >= st[d].niters) st[d].stopped = 1;
                if (st[d].bestIndex != before) {
                    stamp[d] = round;
                    W.h_fetch.p[nFetch++] = BatchEFetch{X.slotOff * slots, (int)j,
                                                        (int)(st[d].bestIndex - begin * slots), (int)d, round};
                }
            }
            if (nFetch) {   // in stream order before the next round's generate reuses the dense regions
                MCV_HIP(hipMemcpyAsync(W.fetch.p, W.h_fetch.p, nFetch * sizeof(BatchEFetch), hipMemcpyHostToDevice,
                                       s));
                launch_batch_e_fetch(W.fetch.p, (int)nFetch, W.dense.p, W.dslot.p, W.ndense.p, W.best.p, W.found.p, s);
                ++stats.launches;
                // the next round rewrites h_fetch only after its own synchronisation
            }
        }
        // ---- winners: mask and count, all in one launch
        std::vector<size_t> win;
        int winMaxN = 0;
        W.fin.ensure(D);
        W.h_fin.ensure(D);
        for (size_t d = 0; d < D; ++d) {
            if (st[d].bestIndex < 0) {
                failed(dev[d], "RANSAC found no model with >= 5 inliers");
                continue;
            }
            const BatchEPack& X = W.h_pack.p[d];
            W.h_fin.p[win.size()] = BatchEFin{X.ptOff, X.N, thr2[d], (int)d};
            winMaxN = std::max(winMaxN, X.N);
            win.push_back(d);
        }
        if (!win.empty()) {
            const size_t n = win.size();
            W.cnt.ensure(n);
            W.h_cnt.ensure(n);
            W.mask.ensure((size_t)total);
            W.h_mask.ensure((size_t)total);
            MCV_HIP(hipMemcpyAsync(W.fin.p, W.h_fin.p, n * sizeof(BatchEFin), hipMemcpyHostToDevice, s));
            MCV_HIP(hipMemsetAsync(W.cnt.p, 0, n * sizeof(int), s));
            MCV_HIP(hipMemsetAsync(W.mask.p, 0, (size_t)total, s));
            launch_batch_e_mask(kind, W.pts.p, W.fin.p, (int)n, winMaxN, W.best.p, W.mask.p, W.cnt.p, s);
            ++stats.launches;
            MCV_HIP(hipMemcpyAsync(W.h_best.p, W.best.p, D * 9 * sizeof(double), hipMemcpyDeviceToHost, s));
            MCV_HIP(hipMemcpyAsync(W.h_found.p, W.found.p, D * sizeof(int), hipMemcpyDeviceToHost, s));
            MCV_HIP(hipMemcpyAsync(W.h_cnt.p, W.cnt.p, n * sizeof(int), hipMemcpyDeviceToHost, s));
            MCV_HIP(hipMemcpyAsync(W.h_mask.p, W.mask.p, (size_t)total, hipMemcpyDeviceToHost, s));
            batch_e_sync(s);
            std::vector<size_t> good;   // winners with a model and inliers (indices into win)
            for (size_t k = 0; k < n; ++k) {
                const size_t d = win[k];
                const int p = dev[d];
                if (W.h_found.p[d] != stamp[d]) {
                    char buf[160];
                    snprintf(buf, sizeof(buf), "winning slot %lld has no model", (long long)st[d].bestIndex);
                    failed(p, buf);
                    continue;
                }
                if (W.h_cnt.p[k] <= 0) {   // cannot happen for a replay winner (its sweep count was >= 5): fail closed
                    failed(p, "the winning model has no inliers");
                    continue;
                }
                good.push_back(k);
            }
            if (!pose) {
                for (size_t k : good) {
                    const size_t d = win[k];
                    const int p = dev[d];
                    const BatchEFin& F = W.h_fin.p[k];
                    counts[p] = W.h_cnt.p[k];
                    std::memcpy(M[p].M, W.h_best.p + 9 * d, 9 * sizeof(double));
                    if (mask) std::memcpy(mask + F.ptOff, W.h_mask.p + F.ptOff, (size_t)F.N);
                    ++ok;
                }
            } else if (!good.empty()) {
                // ---- recoverPose: the four (R, +-t) candidates of every winner, one cheirality launch
                const size_t g = good.size();
                W.pose.ensure(g);
                W.h_pose.ensure(g);
                W.good.ensure(4 * g);
                W.h_good.ensure(4 * g);
                int poseMaxN = 0;
                for (size_t i = 0; i < g; ++i) {
                    const size_t k = good[i], d = win[k];
                    const BatchEFin& F = W.h_fin.p[k];
                    BatchEPose& Q = W.h_pose.p[i];
                    Q.ptOff = F.ptOff;
                    Q.N = F.N;
                    double R1[9], R2[9], t0v[3];
                    e_decompose(W.h_best.p + 9 * d, R1, R2, t0v);
                    const double* Rs[4] = {R1, R2, R1, R2};
                    const double sg[4] = {1, 1, -1, -1};
                    for (int c = 0; c < 4; ++c) {
                        for (int j = 0; j < 9; ++j) Q.P[c][j] = Rs[c][j];
                        for (int j = 0; j < 3; ++j) Q.P[c][9 + j] = sg[c] > 0 ? t0v[j] : -t0v[j];
                    }
                    poseMaxN = std::max(poseMaxN, F.N);
                }
                MCV_HIP(hipMemcpyAsync(W.pose.p, W.h_pose.p, g * sizeof(BatchEPose), hipMemcpyHostToDevice, s));
                MCV_HIP(hipMemsetAsync(W.good.p, 0, 4 * g * sizeof(int), s));
                launch_batch_e_cheirality(W.pts.p, W.mask.p, W.pose.p, (int)g, poseMaxN, kCheiralityDist, W.good.p, s);
                ++stats.launches;
                MCV_HIP(hipMemcpyAsync(W.h_good.p, W.good.p, 4 * g * sizeof(int), hipMemcpyDeviceToHost, s));
                batch_e_sync(s);
                for (size_t i = 0; i < g; ++i) {
                    const size_t k = good[i];
                    const int p = dev[win[k]];
                    const BatchEFin& F = W.h_fin.p[k];
                    const BatchEPose& Q = W.h_pose.p[i];
                    const int* gd = W.h_good.p + 4 * i;
                    int pick = 3;   // e_recover's first maximum
                    if (gd[0] >= gd[1] && gd[0] >= gd[2] && gd[0] >= gd[3]) pick = 0;
                    else if (gd[1] >= gd[0] && gd[1] >= gd[2] && gd[1] >= gd[3]) pick = 1;
                    else if (gd[2] >= gd[0] && gd[2] >= gd[1] && gd[2] >= gd[3]) pick = 2;
                    for (int j = 0; j < 9; ++j) M[p].M[j] = Q.P[pick][j];
                    t[p].X = Q.P[pick][9]; t[p].Y = Q.P[pick][10]; t[p].Z = Q.P[pick][11];
                    counts[p] = gd[pick];
                    if (mask) std::memcpy(mask + F.ptOff, W.h_mask.p + F.ptOff, (size_t)F.N);
                    ++ok;
                }
            }
        }
    }
    if (firstFail >= 0) {
        // a problem that failed returns a zero model, count and mask slice; the first one is named
        char buf[400];
        snprintf(buf, sizeof(buf), "%s: problem %d: %s", who, firstFail, firstMsg.c_str());
        set_last_error(buf);
    } else {
        clear_last_error();
    }
    return ok;
}

}  // namespace

}  // namespace mcv

using namespace mcv;

extern "C" MCV_API int cvFindEssentialMatBatch(const mcvV2d* a, const mcvV2d* b, const int* offsets, int B,
                                               const double* focal, const mcvV2d* pp, const RansacConfig* cfgp,
                                               mcvM33d* E, uint8_t* mask, int* counts) {
    MCV_GUARD(-1, {
        const char* who = "cvFindEssentialMatBatch";
        if (!a || !b || !offsets || !focal || !pp || !E || !counts)
            fail("%s: null argument (a, b, offsets, focal, pp, E and counts are required)", who);
        const RansacConfig cfg = e_config(cfgp);
        batch_e_check(who, offsets, B, cfg);
        std::vector<EProblem> pr((size_t)std::max(B, 0));
        for (int p = 0; p < B; ++p) pr[(size_t)p] = EProblem{focal[p], pp[p], cfg.threshold, cfg.confidence};
        auto single = [&](int p, std::string& msg) {
            const int o = offsets[p];
            const int c = cvFindEssentialMat(a + o, b + o, offsets[p + 1] - o, focal[p], pp[p], cfgp, &E[p],
                                             mask ? mask + o : nullptr);
            if (c > 0) { counts[p] = c; return true; }
            msg = mcvGetLastError();
            return false;
        };
        return e_batch(who, false, a, b, offsets, B, pr, cfg, E, nullptr, mask, counts, single);
    })
}

extern "C" MCV_API int cvRecoverPoseBatch(const RecoverPoseConfig* configs, const mcvV2d* pa, const mcvV2d* pb,
                                          const int* offsets, int B, mcvM33d* R, mcvV3d* t, uint8_t* ms, int* good) {
    MCV_GUARD(-1, {
        const char* who = "cvRecoverPoseBatch";
        if (!configs || !pa || !pb || !offsets || !R || !t || !ms || !good)
            fail("%s: null argument (every pointer is required)", who);
        const RansacConfig cfg = e_config((const RansacConfig*)nullptr);   // e_config(RecoverPoseConfig) per problem:
        batch_e_check(who, offsets, B, cfg);                                // OpenCV's stream, 1000 iterations
        std::vector<EProblem> pr((size_t)std::max(B, 0));
        for (int p = 0; p < B; ++p) {
            const RansacConfig c = e_config(&configs[p]);
            if (!(c.confidence > 0 && c.confidence < 1))
                fail("%s: problem %d: confidence must be in (0,1) (Probability = %g)", who, p, c.confidence);
            pr[(size_t)p] = EProblem{configs[p].FocalLength, configs[p].PrincipalPoint, c.threshold, c.confidence};
        }
        auto single = [&](int p, std::string& msg) {
            const int o = offsets[p];
            const int g = cvRecoverPose(&configs[p], offsets[p + 1] - o, pa + o, pb + o, &R[p], &t[p], ms + o);
            const char* e = mcvGetLastError();
            if (g > 0 || !e || !*e) { good[p] = g; return true; }
            msg = e;
            return false;
        };
        return e_batch(who, true, pa, pb, offsets, B, pr, cfg, R, t, ms, good, single);
    })
}

extern "C" MCV_API int mcvTestBatchSweepE(const double* pts4d, const int* offsets, int B, const double* models9,
                                          const int* modelOffsets, const float* thr2, int kind, int* counts) {
    MCV_GUARD(0, {
        if (!pts4d || !offsets || !models9 || !modelOffsets || !thr2 || !counts || B <= 0)
            fail("mcvTestBatchSweepE: null argument or B <= 0");
        if (kind != 0 && kind != 1) fail("mcvTestBatchSweepE: unsupported kind %d (Sampson fused 0, op-by-op 1)", kind);
        if (offsets[0] != 0 || modelOffsets[0] != 0) fail("mcvTestBatchSweepE: offsets must start at 0");
        int maxModels = 0;
        for (int p = 0; p < B; ++p) {
            if (offsets[p + 1] < offsets[p] || modelOffsets[p + 1] < modelOffsets[p])
                fail("mcvTestBatchSweepE: decreasing offsets at problem %d", p);
            maxModels = std::max(maxModels, modelOffsets[p + 1] - modelOffsets[p]);
        }
        const int total = offsets[B], nModels = modelOffsets[B];
        if (nModels <= 0 || total <= 0) fail("mcvTestBatchSweepE: nothing to sweep");
        require_device();
        DevBuf<double> p, mdl;
        DevBuf<int> c, nd;
        DevBuf<BatchESweep> d;
        std::vector<BatchESweep> h((size_t)B);
        std::vector<int> hn((size_t)B);
        for (int k = 0; k < B; ++k) {
            h[(size_t)k] = BatchESweep{offsets[k], offsets[k + 1] - offsets[k], modelOffsets[k], modelOffsets[k],
                                       thr2[k], 0};
            hn[(size_t)k] = modelOffsets[k + 1] - modelOffsets[k];
        }
        p.ensure((size_t)total * 4);
        mdl.ensure((size_t)nModels * 9);
        c.ensure((size_t)nModels);
        nd.ensure((size_t)B);
        d.ensure((size_t)B);
        MCV_HIP(hipMemcpy(p.p, pts4d, (size_t)total * 32, hipMemcpyHostToDevice));
        MCV_HIP(hipMemcpy(mdl.p, models9, (size_t)nModels * 72, hipMemcpyHostToDevice));
        MCV_HIP(hipMemcpy(d.p, h.data(), (size_t)B * sizeof(BatchESweep), hipMemcpyHostToDevice));
        MCV_HIP(hipMemcpy(nd.p, hn.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice));
        MCV_HIP(hipMemset(c.p, 0, (size_t)nModels * 4));
        launch_batch_e_sweep(kind, p.p, d.p, B, maxModels, mdl.p, nullptr, nd.p, c.p, 0);
        MCV_HIP(hipGetLastError());
        MCV_HIP(hipMemcpy(counts, c.p, (size_t)nModels * 4, hipMemcpyDeviceToHost));
        return 1;
    })
}
