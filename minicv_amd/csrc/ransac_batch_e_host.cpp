// ransac_batch_e_host.cpp — cvFindEssentialMatBatch / cvRecoverPoseBatch: B independent cvFindEssentialMat /
// cvRecoverPose problems in one call whose kernel launches and stream synchronisations do not grow with B
// (DESIGN.md §7f).
//
//   all points -> one segmented buffer of raw pixel pairs, one H2D copy, one batched pack to double4
//                 (x - pp) / focal with each problem's focal and principal point
//   rounds:   batch_host.h's driver over the single call's three generate kernels in their batch form
//             (ransac_e5.hip) + the batched sweep, kEModelSlots counts per hypothesis and each problem's own
//             confidence; the problems whose best model changed get it copied out of their dense region
//             before the next round overwrites it; a large adaptive batch starts with a smaller round
//   finalize: every winner masked and counted in one launch, one copy back
//   pose:     e_decompose per problem on the host, the cheirality counts of all of them in one launch, one
//             copy back, then e_recover's first-maximum rule per problem
// E has no refit and no refine: the winner is the minimal-sample model as solved, so every problem returns
// the single call's bits. Problems with exactly 5 correspondences take the single export (routed through it).
#include "kernels.h"
#include "hyp_essential.h"
#include "batch_host.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>

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

struct BatchEWs : DeviceWs {
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
};

// The essential batches' part of a hypothesis round (batch_host.h's batch_rounds): problem j of the round owns
// the stage columns [j stride, j stride + count), kEModelSlots counts per column and a dense region of the
// same capacity.
struct RoundsE {
    BatchEWs& W;
    int kind;
    uint64_t seed;
    const int* d_table;
    const std::vector<float>& thr2;    // per device problem
    const std::vector<double>& conf;
    std::vector<int> stamp;            // the round (1-based) whose fetch holds problem d's best model
    int round = 0;
    static constexpr int slots = kEModelSlots;
    BatchDesc& desc(size_t j, int) { return W.h_desc.p[j]; }
    void launch(const std::vector<int>& active, BatchRound R, hipStream_t s) {
        BatchStats& stats = batch_stats();
        ++round;
        const size_t n = (size_t)R.n, cols = n * (size_t)R.stride;
        for (size_t j = 0; j < n; ++j) {
            const BatchDesc& X = W.h_desc.p[j];
            const int64_t off = X.slotOff * slots;
            W.h_sweep.p[j] = BatchESweep{X.ptOff, X.N, off, off, thr2[(size_t)active[j]], 0};
        }
        W.stage.ensure(e5_stage_bytes((int)cols));
        W.dense.ensure(cols * slots * sizeof(EModel));
        W.dslot.ensure(cols * slots);
        W.counts.ensure(cols * slots);
        W.h_counts.ensure(cols * slots);
        batch_copy(W.sweep.p, W.h_sweep.p, n * sizeof(BatchESweep), hipMemcpyHostToDevice, s);
        {
            ProfScope pg("batch_e_generate", s);
            stats.launches += launch_e5_batch_generate(W.pts.p, W.desc.p, R.n, R.stride, seed, d_table, W.dense.p,
                                                       W.dslot.p, W.ndense.p, W.counts.p, W.stage.p, s);
        }
        {
            ProfScope ps("batch_e_sweep", s);
            launch_batch_e_sweep(kind, W.pts.p, W.sweep.p, R.n, R.stride * slots, W.dense.p, W.dslot.p, W.ndense.p,
                                 W.counts.p, s);
        }
        ++stats.launches;
    }
    double confidence(int d) const { return conf[(size_t)d]; }
    void best_changed(const std::vector<BestChange>& ch, hipStream_t s) {
        for (size_t k = 0; k < ch.size(); ++k) {
            const BestChange& c = ch[k];
            stamp[(size_t)c.d] = round;
            W.h_fetch.p[k] = BatchEFetch{W.h_desc.p[c.j].slotOff * slots, (int)c.j, (int)c.slot, c.d, round};
        }
        // in stream order before the next round's generate reuses the dense regions; the next round rewrites
        // h_fetch only after its own synchronisation
        batch_copy(W.fetch.p, W.h_fetch.p, ch.size() * sizeof(BatchEFetch), hipMemcpyHostToDevice, s);
        launch_batch_e_fetch(W.fetch.p, (int)ch.size(), W.dense.p, W.dslot.p, W.ndense.p, W.best.p, W.found.p, s);
        ++batch_stats().launches;
    }
};

// The call. pose == false: cvFindEssentialMatBatch (M = E, counts = inliers); pose == true:
// cvRecoverPoseBatch (M = R, t, counts = cvRecoverPose's return). cfg: flags, maxIters, seed for all;
// thresholds and confidences per problem. single(p): the single export on problem p (N == 5).
template <class Single>
int e_batch(const char* who, bool pose, const mcvV2d* a, const mcvV2d* b, const int* offsets, int B,
            const std::vector<EProblem>& pr, const RansacConfig& cfg, mcvM33d* M, mcvV3d* t, uint8_t* mask,
            int* counts, Single single) {
    BatchStats& stats = batch_stats_begin(B);
    if (B == 0) return 0;
    const int total = offsets[B];
    std::memset(M, 0, (size_t)B * sizeof(mcvM33d));
    if (t) std::memset(t, 0, (size_t)B * sizeof(mcvV3d));
    std::memset(counts, 0, (size_t)B * sizeof(int));
    if (mask) std::memset(mask, 0, (size_t)total);
    require_device();

    const int m = 5;
    const bool fixed = (cfg.flags & MCV_FLAG_FIXED_ITERS) != 0;
    const int kind = e_kind(cfg);
    BatchFailures fails;
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
            fails.note(p, buf);
        } else if (N == m) {
            ++stats.single;
            std::string msg;
            if (single(p, msg)) ++ok;
            else {
                fails.note(p, msg);
                std::memset(M[p].M, 0, sizeof(mcvM33d));
                if (t) std::memset(&t[p], 0, sizeof(mcvV3d));
                counts[p] = 0;
                if (mask) std::memset(mask + offsets[p], 0, (size_t)N);
            }
        } else if (!(pr[(size_t)p].focal != 0) || !std::isfinite(pr[(size_t)p].focal)) {
            snprintf(buf, sizeof(buf), "focal length must be finite and non-zero (got %g)", pr[(size_t)p].focal);
            fails.note(p, buf);
        } else {
            dev.push_back(p);
        }
    }
    const size_t D = dev.size();
    if (D) {
        BatchEWs& W = thread_device_ws<BatchEWs>();
        hipStream_t s = W.stream();
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
        std::vector<double> conf(D);
        std::vector<BatchProblem> prob(D);
        int maxN = 0;
        for (size_t d = 0; d < D; ++d) {
            const int p = dev[d];
            const EProblem& X = pr[(size_t)p];
            W.h_pack.p[d] = BatchEPack{offsets[p], offsets[p + 1] - offsets[p], X.focal, X.pp.X, X.pp.Y};
            const double thr = X.thrPix / ((X.focal + X.focal) / 2);   // e_find: threshold /= (fx + fy) / 2
            thr2[d] = (float)(thr * thr);
            conf[d] = X.confidence;
            prob[d] = BatchProblem{offsets[p], offsets[p + 1] - offsets[p], 0};
            maxN = std::max(maxN, offsets[p + 1] - offsets[p]);
        }
        stats.packUs = us_since(t0);
        batch_copy(W.raw.p, W.h_raw.p, (size_t)total * 4 * sizeof(double), hipMemcpyHostToDevice, s);
        batch_copy(W.pack.p, W.h_pack.p, D * sizeof(BatchEPack), hipMemcpyHostToDevice, s);
        launch_batch_e_pack(W.raw.p, W.raw.p + 2 * (size_t)total, W.pack.p, (int)D, maxN, W.pts.p, s);
        ++stats.launches;
        // ---- OpenCV's sample stream (EMEstimatorCallback has no checkSubset: one table per distinct N)
        const int* d_table = cv_tables_by_n(MCV_MODEL_ESSENTIAL, cfg, prob, L.iters, m, W.h_table, W.table, s);
        // ---- hypothesis rounds
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
        // Adaptive problems at moderate outlier ratios stop after roughly a hundred hypotheses, and the generate
        // is most of the device time, so a large adaptive batch starts with a round of
        // kBatchEFirstRound hypotheses per problem and runs the rest of the budget only for the problems that
        // need it: at most one round more, whatever B is. The replay reads the counts in order, so the grouping
        // into rounds never changes a result. Small batches keep one round: below kBatchEFirstMinHyps
        // hypotheses the generate sits on its latency floor and a second round would only add to it.
        int64_t first = L.per;
        if (!fixed && (int64_t)D * L.per >= kBatchEFirstMinHyps) first = std::min(L.per, kBatchEFirstRound);
        RoundsE F{W, kind, cfg.seed, d_table, thr2, conf, std::vector<int>(D, 0)};
        std::vector<mcvReplayState> st;
        batch_rounds(F, prob, st, cfg.maxIters, first, L.per, m, fixed, s);
        const std::vector<int>& stamp = F.stamp;
        // ---- winners: mask and count, all in one launch
        std::vector<size_t> win;
        int winMaxN = 0;
        W.fin.ensure(D);
        W.h_fin.ensure(D);
        for (size_t d = 0; d < D; ++d) {
            if (st[d].bestIndex < 0) {
                fails.note(dev[d], "RANSAC found no model with >= 5 inliers");
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
            batch_copy(W.fin.p, W.h_fin.p, n * sizeof(BatchEFin), hipMemcpyHostToDevice, s);
            MCV_HIP(hipMemsetAsync(W.cnt.p, 0, n * sizeof(int), s));
            MCV_HIP(hipMemsetAsync(W.mask.p, 0, (size_t)total, s));
            launch_batch_e_mask(kind, W.pts.p, W.fin.p, (int)n, winMaxN, W.best.p, W.mask.p, W.cnt.p, s);
            ++stats.launches;
            batch_copy(W.h_best.p, W.best.p, D * 9 * sizeof(double), hipMemcpyDeviceToHost, s);
            batch_copy(W.h_found.p, W.found.p, D * sizeof(int), hipMemcpyDeviceToHost, s);
            batch_copy(W.h_cnt.p, W.cnt.p, n * sizeof(int), hipMemcpyDeviceToHost, s);
            batch_copy(W.h_mask.p, W.mask.p, (size_t)total, hipMemcpyDeviceToHost, s);
            batch_sync(s);
            std::vector<size_t> good;   // winners with a model and inliers (indices into win)
            for (size_t k = 0; k < n; ++k) {
                const size_t d = win[k];
                const int p = dev[d];
                if (W.h_found.p[d] != stamp[d]) {
                    char buf[160];
                    snprintf(buf, sizeof(buf), "winning slot %lld has no model", (long long)st[d].bestIndex);
                    fails.note(p, buf);
                    continue;
                }
                if (W.h_cnt.p[k] <= 0) {   // cannot happen for a replay winner (its sweep count was >= 5): fail closed
                    fails.note(p, "the winning model has no inliers");
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
                batch_copy(W.pose.p, W.h_pose.p, g * sizeof(BatchEPose), hipMemcpyHostToDevice, s);
                MCV_HIP(hipMemsetAsync(W.good.p, 0, 4 * g * sizeof(int), s));
                launch_batch_e_cheirality(W.pts.p, W.mask.p, W.pose.p, (int)g, poseMaxN, kCheiralityDist, W.good.p, s);
                ++stats.launches;
                batch_copy(W.h_good.p, W.good.p, 4 * g * sizeof(int), hipMemcpyDeviceToHost, s);
                batch_sync(s);
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
    fails.report(who);   // a problem that failed returns a zero model, count and mask slice; the first one is named
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
        check_batch_offsets(who, offsets, B);
        check_batch_config(who, cfg);
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
        // e_config(RecoverPoseConfig) per problem: OpenCV's stream, 1000 iterations
        const RansacConfig cfg = e_config((const RansacConfig*)nullptr);
        check_batch_offsets(who, offsets, B);
        check_batch_config(who, cfg);
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
