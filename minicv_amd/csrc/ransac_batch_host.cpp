// ransac_batch_host.cpp — cvFindModelBatch: B independent RANSAC problems of one 2-D model family
// (homography, 8-point fundamental, affine, similarity) in one call whose kernel launches and stream
// synchronisations do not grow with B.
//
//   all points -> one segmented float4 buffer, one H2D copy (+ one for OpenCV's sample tables: one block of
//             rows per problem, because checkSubset makes them depend on the points)
//   rounds:   batch_host.h's driver over the batched generate + the batched sweep
//   finalize: every winner re-solved, masked and counted in two launches, one copy back
//   refine:   the B Levenberg-Marquardt solvers in lockstep (lm_solver.h's LmStepper, the controller the
//             single call loops over): each step is one batched reduction over the problems still
//             iterating and one read-back; H runs the batched refit chain first. The sums keep reduce.h's
//             order per problem over the single call's per-point terms, and the host algebra is the single
//             call's own functions (LmStepper, h_refit_from_record, a_to_params / a_from_params), so
//             every problem returns the single call's bits.
// Problems with exactly the sample size take the single export's direct solve (routed through it).
#include "kernels.h"
#include "linalg.h"
#include "mcv_common.h"
#include "hyp_homography.h"
#include "hyp_affine.h"
#include "lm_solver.h"
#include "batch_host.h"

#include <cmath>
#include <cfloat>
#include <climits>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>

namespace mcv {

static int64_t g_batch_cap = kBatchSlotCap;   // a round's slots (ransac_batch_index.h); mcvTestBatchCap
// The essential batches count hypotheses, not slots: one costs 2292 B of five-point stage, 720 B of dense
// models and 80 B of counts and slot indices, ~3.1 KB, so 2^18 of them are 0.8 GB (B = 256 problems of the
// default 1000 iterations fit one round).
// mcvTestBatchCap overrides both: a cap other than the 2-D default holds for this family too.
static const int64_t kBatchHypCapE = (int64_t)1 << 18;
int64_t batch_cap_essential() { return g_batch_cap == kBatchSlotCap ? kBatchHypCapE : g_batch_cap; }
// The PnP batch counts hypotheses too: an EPnP hypothesis holds kEpnpSplitDoubles = 291 doubles of split-solve
// scratch (2328 B), a 96 B pose and a 4 B count, so 2^18 of them are 0.64 GB (B = 1024 problems of the default
// 100 iterations fit one round with room to spare). AP3P rounds hold only the poses and counts.
static const int64_t kBatchHypCapPnp = (int64_t)1 << 18;
int64_t batch_cap_pnp() { return g_batch_cap == kBatchSlotCap ? kBatchHypCapPnp : g_batch_cap; }

static thread_local BatchStats t_stats;
BatchStats& batch_stats() { return t_stats; }

struct BatchWs : DeviceWs {
    DevBuf<float> pts;
    DevBuf<int> table, counts, cnt;
    DevBuf<uint8_t> models, mask;
    DevBuf<BatchDesc> desc;
    DevBuf<BatchFin> fin;
    DevBuf<BatchRed> red;
    DevBuf<BatchOne> one;
    DevBuf<double> par, part, out, rec;
    PinnedBuf<float> h_pts;
    PinnedBuf<int> h_table, h_counts, h_cnt;
    PinnedBuf<uint8_t> h_mask;
    PinnedBuf<BatchDesc> h_desc;
    PinnedBuf<BatchFin> h_fin;
    PinnedBuf<BatchRed> h_red;
    PinnedBuf<BatchOne> h_one;
    PinnedBuf<double> h_par, h_out, h_rec;
};

static const char* batch_model_name(int model) {
    return model == MCV_MODEL_HOMOGRAPHY ? "homography" : model == MCV_MODEL_FUNDAMENTAL ? "fundamental"
           : model == MCV_MODEL_AFFINE   ? "affine" : "similarity";
}

// What a (model, cfg) is refused for; returns the configuration. NULL cfg: the single exports' defaults.
static RansacConfig batch_config(int model, const RansacConfig* cfgp) {
    if (model != MCV_MODEL_HOMOGRAPHY && model != MCV_MODEL_FUNDAMENTAL && !affine_family(model))
        fail("cvFindModelBatch: unsupported model %d (homography, fundamental, affine, similarity)", model);
    const RansacConfig cfg = config_or_default(model, cfgp);
    check_batch_config("cvFindModelBatch", cfg, true);
    return cfg;
}
void batch_check_config(int model, const RansacConfig* cfgp) { (void)batch_config(model, cfgp); }

// Everything a call can be refused for without touching the device.
static RansacConfig batch_check(int model, const mcvV2d* a, const mcvV2d* b, const int* offsets, int B,
                                const RansacConfig* cfgp, const mcvM33d* models, const int* counts) {
    if (!a || !b || !offsets || !models || !counts)
        fail("cvFindModelBatch: null argument (a, b, offsets, models and counts are required)");
    check_batch_offsets("cvFindModelBatch", offsets, B);
    return batch_config(model, cfgp);
}

// The single export on one slice (N == sample size: its direct solve). Returns its count.
static int batch_single(int model, const mcvV2d* a, const mcvV2d* b, int N, const RansacConfig* cfgp, double* M9,
                        uint8_t* mask) {
    ++t_stats.single;
    if (model == MCV_MODEL_HOMOGRAPHY) return cvFindHomography(a, b, N, cfgp, (mcvM33d*)M9, mask);
    if (model == MCV_MODEL_FUNDAMENTAL) return cvFindFundamentalMat(a, b, N, cfgp, (mcvM33d*)M9, mask);
    double A6[6] = {0, 0, 0, 0, 0, 0};
    const int c = model == MCV_MODEL_AFFINE ? cvEstimateAffine2D(a, b, N, cfgp, A6, mask)
                                            : cvEstimateAffinePartial2D(a, b, N, cfgp, A6, mask);
    if (c > 0) {
        for (int k = 0; k < 6; ++k) M9[k] = A6[k];
        M9[6] = 0; M9[7] = 0; M9[8] = 1;
    }
    return c;
}

struct RefineJob { int ptOff, N; double* M9; };   // a winner to refine, its model in place

static void upload_red(BatchWs& W, const std::vector<const RefineJob*>& act, hipStream_t s) {
    const size_t n = act.size();
    W.red.ensure(n);
    W.h_red.ensure(n);
    for (size_t k = 0; k < n; ++k) W.h_red.p[k] = BatchRed{act[k]->ptOff, act[k]->N};
    batch_copy(W.red.p, W.h_red.p, n * sizeof(BatchRed), hipMemcpyHostToDevice, s);
}

// LMSolver(refine callback, 10) of every job in lockstep: per step one batched reduction over the jobs
// still iterating, one read-back, then each job's own host algebra.
template <int LX>
static void batch_lm(BatchWs& W, std::vector<RefineJob>& jobs, int maxN, hipStream_t s) {
    if (jobs.empty()) return;
    std::vector<LmStepper<LX>> st(jobs.size());
    for (size_t j = 0; j < jobs.size(); ++j) {
        double x0[LX];
        if constexpr (LX == 8) std::memcpy(x0, jobs[j].M9, 8 * sizeof(double));   // H[0..7]; H[8] stays
        else a_to_params(LX, jobs[j].M9, x0);
        st[j].begin(x0, 10);
    }
    const size_t per = (size_t)batch_reduce_blocks(maxN);
    for (;;) {
        std::vector<const RefineJob*> act;
        std::vector<size_t> who;
        for (size_t j = 0; j < jobs.size(); ++j)
            if (!st[j].finished()) { act.push_back(&jobs[j]); who.push_back(j); }
        if (act.empty()) break;
        const size_t n = act.size();
        upload_red(W, act, s);
        W.par.ensure(n * 8);
        W.h_par.ensure(n * 8);
        W.out.ensure(n * 45);
        W.h_out.ensure(n * 45);
        W.part.ensure(n * per * 45);
        for (size_t k = 0; k < n; ++k) {
            const double* x = st[who[k]].request();
            for (int i = 0; i < 8; ++i) W.h_par.p[8 * k + i] = i < LX ? x[i] : 0.0;
        }
        batch_copy(W.par.p, W.h_par.p, n * 8 * sizeof(double), hipMemcpyHostToDevice, s);
        t_stats.launches += launch_batch_reduce_lm(LX, W.pts.p, W.mask.p, W.red.p, (int)n, maxN, W.par.p, W.part.p,
                                                   W.out.p, s);
        batch_copy(W.h_out.p, W.out.p, n * 45 * sizeof(double), hipMemcpyDeviceToHost, s);
        batch_sync(s);
        ++t_stats.lmRounds;
        for (size_t k = 0; k < n; ++k) st[who[k]].feed(W.h_out.p + 45 * k);
    }
    for (size_t j = 0; j < jobs.size(); ++j) {
        if constexpr (LX == 8) std::memcpy(jobs[j].M9, st[j].x, 8 * sizeof(double));
        else a_from_params(LX, st[j].x, jobs[j].M9);
    }
}

// HomographyEstimatorCallback::runKernel on every job's inliers: the chained passes for all of them, one
// read-back, h_refit's algebra per job (a job whose refit fails keeps its model, as in h_finalize).
static void batch_h_refit(BatchWs& W, std::vector<RefineJob>& jobs, int maxN, hipStream_t s) {
    if (jobs.empty()) return;
    const size_t n = jobs.size();
    std::vector<const RefineJob*> act;
    for (auto& j : jobs) act.push_back(&j);
    upload_red(W, act, s);
    W.rec.ensure(n * kRefitDoubles);
    W.h_rec.ensure(n * kRefitDoubles);
    W.part.ensure(n * (size_t)batch_reduce_blocks(maxN) * 45);
    t_stats.launches += launch_batch_refit_chain(W.pts.p, W.mask.p, W.red.p, (int)n, maxN, W.part.p, W.rec.p, s);
    batch_copy(W.h_rec.p, W.rec.p, n * kRefitDoubles * sizeof(double), hipMemcpyDeviceToHost, s);
    batch_sync(s);
    for (size_t k = 0; k < n; ++k) {
        double Hr[9];
        if (h_refit_from_record(W.h_rec.p + k * kRefitDoubles, Hr))
            for (int i = 0; i < 9; ++i) jobs[k].M9[i] = Hr[i];
    }
}

// cvFindModelBatch's part of a hypothesis round (batch_host.h's batch_rounds): one model per hypothesis, one
// confidence for all problems; a winner is re-solved from its index, so a new best needs no fetch.
struct Rounds2d {
    BatchWs& W;
    int model, errKind;
    uint64_t seed;
    const int* d_table;
    float thr2;
    double conf;
    static constexpr int slots = 1;
    BatchDesc& desc(size_t j, int) { return W.h_desc.p[j]; }
    void launch(const std::vector<int>&, BatchRound R, hipStream_t s) {
        launch_batch_generate(model, W.pts.p, W.desc.p, R.n, R.stride, seed, d_table, W.models.p, W.counts.p, s);
        launch_batch_sweep(model, errKind, W.pts.p, W.desc.p, R.n, R.stride, W.models.p, W.counts.p, thr2, s);
        batch_stats().launches += 2;
    }
    double confidence(int) const { return conf; }
    void best_changed(const std::vector<BestChange>&, hipStream_t) {}
};

static int find_model_batch(int model, const mcvV2d* a, const mcvV2d* b, const int* offsets, int B,
                            const RansacConfig* cfgp, mcvM33d* models, uint8_t* mask, int* counts) {
    const RansacConfig cfg = batch_check(model, a, b, offsets, B, cfgp, models, counts);
    batch_stats_begin(B);
    if (B == 0) return 0;
    const int total = offsets[B];
    std::memset(models, 0, (size_t)B * sizeof(mcvM33d));
    std::memset(counts, 0, (size_t)B * sizeof(int));
    if (mask) std::memset(mask, 0, (size_t)total);
    require_device();

    const int m = model_points(model);
    const bool fixed = (cfg.flags & MCV_FLAG_FIXED_ITERS) != 0;
    const double t = effective_threshold(cfg);
    const float thr2 = (float)(t * t);
    const int errKind = model == MCV_MODEL_FUNDAMENTAL ? f_error_kind(cfg) : 0;
    BatchFailures fails;
    int ok = 0;

    BatchLayout L;
    batch_layout(offsets, B, m, cfg.maxIters, g_batch_cap, L);
    // the problems that never reach the device: too few points, or exactly the sample size
    for (int p = 0; p < B; ++p) {
        const int N = offsets[p + 1] - offsets[p];
        char buf[160];
        if (N < m) {
            snprintf(buf, sizeof(buf), "need at least %d correspondences (N=%d)", m, N);
            fails.note(p, buf);
        } else if (N == m) {
            const int c = batch_single(model, a + offsets[p], b + offsets[p], N, cfgp, models[p].M,
                                       mask ? mask + offsets[p] : nullptr);
            if (c > 0) { counts[p] = c; ++ok; }
            else {
                fails.note(p, mcvGetLastError());
                std::memset(models[p].M, 0, sizeof(mcvM33d));
                if (mask) std::memset(mask + offsets[p], 0, (size_t)N);
            }
        }
    }
    const size_t D = L.dev.size();
    if (D) {
        BatchWs& W = thread_device_ws<BatchWs>();
        hipStream_t s = W.stream();
        // ---- points: one conversion pass (OpenCV's convertTo(CV_32F)), one copy
        W.h_pts.ensure((size_t)total * 4);
        W.pts.ensure((size_t)total * 4);
        auto t0 = std::chrono::steady_clock::now();
        pack_float4(a, b, total, W.h_pts.p);
        t_stats.packUs = us_since(t0);
        batch_copy(W.pts.p, W.h_pts.p, (size_t)total * 16, hipMemcpyHostToDevice, s);
        // ---- OpenCV's sample stream: one cv::RNG((uint64)-1) stream per problem, as each single call draws
        const int* d_table = nullptr;
        if (cv_sampler(cfg)) {
            const size_t rowInts = (size_t)L.iters * m;
            W.h_table.ensure(D * rowInts);
            W.table.ensure(D * rowInts);
            std::vector<int> rows;
            t0 = std::chrono::steady_clock::now();
            for (size_t d = 0; d < D; ++d) {
                const int p = L.dev[d];
                cv_table_build(model, cfg, W.h_pts.p + 4 * (size_t)offsets[p], offsets[p + 1] - offsets[p], L.iters,
                               rows);
                std::memcpy(W.h_table.p + d * rowInts, rows.data(), rowInts * sizeof(int));
            }
            t_stats.tableUs = us_since(t0);
            batch_copy(W.table.p, W.h_table.p, D * rowInts * sizeof(int), hipMemcpyHostToDevice, s);
            d_table = W.table.p;
        }
        // ---- hypothesis rounds
        std::vector<BatchProblem> prob(D);
        for (size_t d = 0; d < D; ++d) {
            const int p = L.dev[d];
            prob[d] = BatchProblem{offsets[p], offsets[p + 1] - offsets[p], L.rowOff[(size_t)p]};
        }
        const size_t slotsMax = D * (size_t)L.per;
        W.models.ensure(slotsMax * batch_model_bytes(model));
        W.counts.ensure(slotsMax);
        W.h_counts.ensure(slotsMax);
        Rounds2d F{W, model, errKind, cfg.seed, d_table, thr2, cfg.confidence};
        std::vector<mcvReplayState> st;
        batch_rounds(F, prob, st, cfg.maxIters, L.per, L.per, m, fixed, s);
        // ---- winners: re-solve, mask and count, all in two launches
        std::vector<size_t> win;
        int maxN = 0;
        W.fin.ensure(D);
        W.h_fin.ensure(D);
        for (size_t d = 0; d < D; ++d) {
            const int p = L.dev[d];
            if (st[d].bestIndex < 0) {
                char buf[160];
                snprintf(buf, sizeof(buf), "RANSAC found no model with >= %d inliers", m);
                fails.note(p, buf);
                continue;
            }
            BatchFin& F = W.h_fin.p[win.size()];
            F.ptOff = offsets[p];
            F.N = offsets[p + 1] - offsets[p];
            F.rowOff = L.rowOff[(size_t)p];
            F.hyp = st[d].bestIndex;
            maxN = std::max(maxN, F.N);
            win.push_back(d);
        }
        if (!win.empty()) {
            const size_t n = win.size();
            W.one.ensure(n);
            W.h_one.ensure(n);
            W.cnt.ensure(n);
            W.h_cnt.ensure(n);
            W.mask.ensure((size_t)total);
            W.h_mask.ensure((size_t)total);
            batch_copy(W.fin.p, W.h_fin.p, n * sizeof(BatchFin), hipMemcpyHostToDevice, s);
            MCV_HIP(hipMemsetAsync(W.cnt.p, 0, n * sizeof(int), s));
            MCV_HIP(hipMemsetAsync(W.mask.p, 0, (size_t)total, s));
            launch_batch_one(model, W.pts.p, W.fin.p, (int)n, cfg.seed, d_table, W.one.p, s);
            launch_batch_mask(model, errKind, W.pts.p, W.fin.p, (int)n, maxN, W.one.p, thr2, W.mask.p, W.cnt.p, s);
            t_stats.launches += 2;
            batch_copy(W.h_one.p, W.one.p, n * sizeof(BatchOne), hipMemcpyDeviceToHost, s);
            batch_copy(W.h_cnt.p, W.cnt.p, n * sizeof(int), hipMemcpyDeviceToHost, s);
            batch_copy(W.h_mask.p, W.mask.p, (size_t)total, hipMemcpyDeviceToHost, s);
            batch_sync(s);
            std::vector<RefineJob> jobs;
            int jobMaxN = 0;
            for (size_t k = 0; k < n; ++k) {
                const int p = L.dev[win[k]];
                const BatchOne& o = W.h_one.p[k];
                const BatchFin& F = W.h_fin.p[k];
                if (o.status != 1) {
                    char buf[160];
                    snprintf(buf, sizeof(buf), "winning hypothesis %lld has no model (status %d)", (long long)F.hyp,
                             o.status);
                    fails.note(p, buf);
                    continue;
                }
                const int c = W.h_cnt.p[k];
                if (c <= 0) {   // cannot happen for a replay winner (its sweep count was >= m): fail closed
                    fails.note(p, "the winning model has no inliers");
                    continue;
                }
                counts[p] = c;
                double* M = models[p].M;
                if (affine_family(model)) {
                    for (int i = 0; i < 6; ++i) M[i] = o.M[i];
                    M[6] = 0; M[7] = 0; M[8] = 1;
                } else {
                    for (int i = 0; i < 9; ++i) M[i] = o.M[i];
                }
                if (mask) std::memcpy(mask + F.ptOff, W.h_mask.p + F.ptOff, (size_t)F.N);
                ++ok;
                // the single calls' refine conditions (h_finalize, a_finalize_impl); F is not refined
                const bool refine = !(cfg.flags & MCV_FLAG_NO_REFINE) &&
                                    (model == MCV_MODEL_HOMOGRAPHY ? (F.N > 4 && c > 0)
                                                                   : (affine_family(model) && c > m));
                if (refine) {
                    jobs.push_back(RefineJob{F.ptOff, F.N, M});
                    jobMaxN = std::max(jobMaxN, F.N);
                }
            }
            if (model == MCV_MODEL_HOMOGRAPHY) {
                batch_h_refit(W, jobs, jobMaxN, s);
                batch_lm<8>(W, jobs, jobMaxN, s);
            } else if (model == MCV_MODEL_AFFINE) {
                batch_lm<6>(W, jobs, jobMaxN, s);
            } else if (model == MCV_MODEL_SIMILARITY) {
                batch_lm<4>(W, jobs, jobMaxN, s);
            }
        }
    }
    // a problem that failed returns a zero model, count and mask slice; the first one is named
    fails.report((std::string("cvFindModelBatch (") + batch_model_name(model) + ")").c_str());
    return ok;
}

}  // namespace mcv

using namespace mcv;

extern "C" MCV_API int cvFindModelBatch(int model, const mcvV2d* a, const mcvV2d* b, const int* offsets, int B,
                                        const RansacConfig* cfg, mcvM33d* models, uint8_t* mask, int* counts) {
    MCV_GUARD(-1, { return find_model_batch(model, a, b, offsets, B, cfg, models, mask, counts); })
}

extern "C" MCV_API int mcvHostBatchLayout(const int* offsets, int B, int m, int maxIters, long long cap,
                                          long long* desc4, long long* info4) {
    MCV_GUARD(-1, {
        if (!offsets || B < 0 || m < 1 || (B > 0 && !desc4) || !info4) fail("mcvHostBatchLayout: bad argument");
        BatchLayout L;
        batch_layout(offsets, B, m, maxIters, cap, L);
        for (int p = 0; p < B; ++p) {
            desc4[4 * p + 0] = offsets[p];
            desc4[4 * p + 1] = offsets[p + 1] - offsets[p];
            desc4[4 * p + 2] = L.slotOff[(size_t)p];
            desc4[4 * p + 3] = L.rowOff[(size_t)p];
        }
        info4[0] = (long long)L.dev.size();
        info4[1] = L.per;
        info4[2] = L.rounds;
        info4[3] = (long long)L.dev.size() * L.per;
        return (int)L.dev.size();
    })
}

extern "C" MCV_API int mcvHostBatchRound(const int* ptOff, const int* N, const long long* rowOff,
                                         const long long* niters, const int* stopped, int D, const int* active,
                                         int nActive, long long begin, long long size, long long* desc6,
                                         int* activeOut, long long* info2) {
    MCV_GUARD(-1, {
        const char* who = "mcvHostBatchRound";
        if (!info2 || D < 0 || nActive < 0 || nActive > D || (D > 0 && (!ptOff || !N || !niters || !stopped)) ||
            (nActive > 0 && (!active || !desc6 || !activeOut)))
            fail("%s: bad argument", who);
        if (begin < 0 || begin > INT_MAX || size < 1 || size > INT_MAX)
            fail("%s: begin %lld or size %lld outside [0, 2^31) / [1, 2^31)", who, begin, size);
        for (int k = 0; k < nActive; ++k)
            if (active[k] < 0 || active[k] >= D || (k > 0 && active[k] <= active[k - 1]))
                fail("%s: active[%d] = %d is not an ascending index below D = %d", who, k, active[k], D);
        struct State { int64_t niters; int stopped; };
        std::vector<BatchProblem> prob((size_t)D);
        std::vector<State> st((size_t)D);
        for (int d = 0; d < D; ++d) {
            prob[(size_t)d] = BatchProblem{ptOff[d], N[d], rowOff ? rowOff[d] : 0};
            st[(size_t)d] = State{niters[d], stopped[d]};
        }
        std::vector<int> act(active, active + nActive);
        std::vector<BatchDesc> desc((size_t)nActive);
        const BatchRound R = batch_round(prob.data(), st.data(), act, begin, size,
                                         [&](size_t j, int) -> BatchDesc& { return desc[j]; });
        for (int j = 0; j < R.n; ++j) {
            const BatchDesc& X = desc[(size_t)j];
            const long long row[6] = {X.ptOff, X.N, X.hypBegin, X.hypCount, X.slotOff, X.rowOff};
            std::memcpy(desc6 + 6 * j, row, sizeof(row));
            activeOut[j] = act[(size_t)j];
        }
        info2[0] = R.n;
        info2[1] = R.stride;
        return R.n;
    })
}

extern "C" MCV_API long long mcvTestBatchCap(long long cap) {
    const long long prev = g_batch_cap;
    g_batch_cap = cap > 0 ? cap : kBatchSlotCap;
    return prev;
}

extern "C" MCV_API int mcvTestBatchStats(long long* stats16) {
    if (!stats16) return 0;
    const BatchStats& S = t_stats;
    const long long v[16] = {S.launches, S.syncs,  S.rounds,  S.lmRounds,      S.single,
                             S.problems, S.packUs, S.tableUs, S.problemRounds, S.copies};
    std::memcpy(stats16, v, sizeof(v));
    return 1;
}

extern "C" MCV_API int mcvTestBatchSweep(int model, const float* pts4, const int* offsets, int B, const void* models,
                                         const int* modelOffsets, float thr2, int errKind, int* counts) {
    MCV_GUARD(0, {
        if (!pts4 || !offsets || !models || !modelOffsets || !counts || B <= 0)
            fail("mcvTestBatchSweep: null argument or B <= 0");
        if (model != MCV_MODEL_HOMOGRAPHY && model != MCV_MODEL_FUNDAMENTAL && !affine_family(model))
            fail("mcvTestBatchSweep: unsupported model %d", model);
        if (model == MCV_MODEL_FUNDAMENTAL ? (errKind < 0 || errKind > 3) : errKind != 0)
            fail("mcvTestBatchSweep: unsupported errKind %d", errKind);
        if (offsets[0] != 0 || modelOffsets[0] != 0) fail("mcvTestBatchSweep: offsets must start at 0");
        int maxHyp = 0;
        for (int p = 0; p < B; ++p) {
            if (offsets[p + 1] < offsets[p] || modelOffsets[p + 1] < modelOffsets[p])
                fail("mcvTestBatchSweep: decreasing offsets at problem %d", p);
            maxHyp = std::max(maxHyp, modelOffsets[p + 1] - modelOffsets[p]);
        }
        const int total = offsets[B], nModels = modelOffsets[B];
        if (nModels <= 0 || total <= 0) fail("mcvTestBatchSweep: nothing to sweep");
        require_device();
        const size_t mb = batch_model_bytes(model);
        DevBuf<float> p;
        DevBuf<uint8_t> mdl;
        DevBuf<int> c;
        DevBuf<BatchDesc> d;
        std::vector<BatchDesc> h((size_t)B);
        for (int k = 0; k < B; ++k) {
            h[(size_t)k].ptOff = offsets[k];
            h[(size_t)k].N = offsets[k + 1] - offsets[k];
            h[(size_t)k].hypBegin = 0;
            h[(size_t)k].hypCount = modelOffsets[k + 1] - modelOffsets[k];
            h[(size_t)k].slotOff = modelOffsets[k];
            h[(size_t)k].rowOff = 0;
        }
        p.ensure((size_t)total * 4);
        mdl.ensure((size_t)nModels * mb);
        c.ensure((size_t)nModels);
        d.ensure((size_t)B);
        MCV_HIP(hipMemcpy(p.p, pts4, (size_t)total * 16, hipMemcpyHostToDevice));
        MCV_HIP(hipMemcpy(mdl.p, models, (size_t)nModels * mb, hipMemcpyHostToDevice));
        MCV_HIP(hipMemcpy(d.p, h.data(), (size_t)B * sizeof(BatchDesc), hipMemcpyHostToDevice));
        MCV_HIP(hipMemset(c.p, 0, (size_t)nModels * 4));
        launch_batch_sweep(model, errKind, p.p, d.p, B, maxHyp, mdl.p, c.p, thr2, 0);
        MCV_HIP(hipGetLastError());
        MCV_HIP(hipMemcpy(counts, c.p, (size_t)nModels * 4, hipMemcpyDeviceToHost));
        return 1;
    })
}
