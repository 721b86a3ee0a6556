// ransac_host.cpp — host orchestration of the RANSAC hot path behind the C-ABI.
//
// cvFindHomography (new export, conventions of cvRecoverPose, MiniCVNative.cpp:197-215):
//   pack V2d -> float4 on device  ->  [chunks of hypotheses: generate + verify on the GPU,
//   counts back, OpenCV-order sequential replay on the host (adaptive niters)]  ->  finalize:
//   mask of the winner, refit on its inliers (runKernel: GPU reductions + 9x9 Jacobi here),
//   10 Levenberg-Marquardt iterations (GPU reductions + 8x8 solve here)  ->  H, mask.
// Mirrors cv::findHomography(..., RANSAC, thr, mask, maxIters, conf) of OpenCV 4.x
// [ext: calib3d/src/fundam.cpp, ptsetreg.cpp, levmarq.cpp — absent here, SURVEY.md §8c].
#include "minicv_native.h"
#include "mcv_runtime.h"
#include "kernels.h"
#include "linalg.h"
#include "mcv_common.h"
#include "hyp_homography.h"
#include "h_cell_bound.h"
#include "hyp_affine.h"
#include "plan.h"
#include "rank_select.h"
#include "lm_solver.h"

#include <cmath>
#include <cfloat>
#include <cstring>
#include <cstdlib>
#include <vector>
#include <algorithm>
#include <memory>

namespace mcv {

// ------------------------------------------------------------------------------------------
// Sequential replay (RANSACPointSetRegistrator::run loop order + RANSACUpdateNumIters).
// ------------------------------------------------------------------------------------------
int ransac_update_num_iters(double p, double ep, int modelPoints, int64_t maxIters) {
    p = std::max(p, 0.);
    p = std::min(p, 1.);
    ep = std::max(ep, 0.);
    ep = std::min(ep, 1.);
    double num = std::max(1. - p, DBL_MIN);
    double denom = 1. - std::pow(1. - ep, modelPoints);
    if (denom < DBL_MIN) return 0;
    num = std::log(num);
    denom = std::log(denom);
    return (denom >= 0 || -num >= (double)maxIters * (-denom)) ? (int)maxIters : (int)std::lrint(num / denom);
}

}  // namespace mcv

using namespace mcv;

extern "C" MCV_API void mcvReplayInit(mcvReplayState* st, int maxIters) {
    st->niters = std::max(maxIters, 1);
    st->bestIndex = -1;
    st->bestCount = 0;
    st->stopped = 0;
}

namespace mcv {
// One chunk of the RANSACPointSetRegistrator::run loop: hypothesis `it` = one getSubset +
// runKernel; its models (slots) are tried in order, each improvement updates niters; the loop
// condition is checked per hypothesis.
static int replay_chunk(mcvReplayState* st, const int* counts, int64_t hypBegin, int64_t hypCount, int slots, int N,
                        int modelPoints, double confidence, int fixedIters) {
    if (st->stopped) return 1;
    for (int64_t i = 0; i < hypCount; ++i) {
        const int64_t it = hypBegin + i;
        if (it >= st->niters) { st->stopped = 1; return 1; }
        const int* c = counts + i * slots;
        if (c[0] == kStatusNoSample) { st->stopped = 1; return 1; }
        for (int k = 0; k < slots; ++k) {
            if (c[k] < 0) continue;
            if (c[k] > std::max(st->bestCount, modelPoints - 1)) {
                st->bestCount = c[k];
                st->bestIndex = it * slots + k;
                if (!fixedIters)
                    st->niters = ransac_update_num_iters(confidence, (double)(N - c[k]) / N, modelPoints, st->niters);
            }
        }
    }
    if (hypBegin + hypCount >= st->niters) { st->stopped = 1; return 1; }
    return 0;
}
}  // namespace mcv

extern "C" MCV_API int mcvReplayChunk(mcvReplayState* st, const int* counts, int64_t hypBegin, int64_t hypCount,
                                      int N, int modelPoints, double confidence, int fixedIters) {
    return replay_chunk(st, counts, hypBegin, hypCount, 1, N, modelPoints, confidence, fixedIters);
}

extern "C" MCV_API int mcvReplayChunkModels(mcvReplayState* st, const int* counts, int64_t hypBegin,
                                            int64_t hypCount, int slotsPerHyp, int N, int modelPoints,
                                            double confidence, int fixedIters) {
    if (slotsPerHyp < 1) slotsPerHyp = 1;
    return replay_chunk(st, counts, hypBegin, hypCount, slotsPerHyp, N, modelPoints, confidence, fixedIters);
}

namespace mcv {

// ------------------------------------------------------------------------------------------
// Plan
// ------------------------------------------------------------------------------------------
// mcvTestHStaging: 0 automatic, 1 staging regardless of the call's size, 2 never (tests only)
static int g_hstage_mode = 0;
// the plan of the calling thread's last homography evaluate (mcvTestHStaging reads its control block)
static thread_local Plan* t_hstage_plan = nullptr;
// mcvTestHCellMode: the per-cell bound before stage 1: 0 automatic, 1 whenever the sweep is staged, 2 never;
// its two grids
static int g_hcell_mode = 0;
static int g_hcell_G = kHCellG, g_hcell_Gs = kHCellGs;
// mcvTestHMfma: the certified homography sweep's form (kHForm*), and where the calling thread's last
// such sweep left its stats: a plan's device counters, or the values a sweep outside a plan reported
static int g_hmfma_mode = kHFormAuto;
static thread_local Plan* t_hmfma_plan = nullptr;
static thread_local unsigned long long t_hmfma_last[kHMfmaStats] = {0, 0, 0};
int h_mfma_form() { return g_hmfma_mode; }
void h_mfma_set_last(const unsigned long long* stats3) {
    t_hmfma_plan = nullptr;
    for (int i = 0; i < kHMfmaStats; ++i) t_hmfma_last[i] = stats3[i];
}

void Plan::reserve(int n, int64_t hyps) {
    if (n > maxN) maxN = n;
    if (hyps > maxHyps) maxHyps = hyps;
    const size_t slots = (size_t)model_slots(model);
    if (model == MCV_MODEL_ESSENTIAL || model == MCV_MODEL_PNP) {
        ptsd.ensure((size_t)maxN * 4);
        raw.ensure((size_t)maxN * 4);
        dslot.ensure((size_t)maxHyps * slots);
        ndense.ensure(8);
        if (model == MCV_MODEL_ESSENTIAL && maxHyps >= kEStageMinHyps) estage.ensure((size_t)maxHyps * sizeof(EStage));
    } else {
        pts.ensure((size_t)maxN * 4);
    }
    models.ensure((size_t)maxHyps * model_bytes(model));
    if (model == MCV_MODEL_HOMOGRAPHY) h64.ensure((size_t)maxHyps * 9);
    if (affine_family(model)) h64.ensure((size_t)maxHyps * 6);
    counts.ensure((size_t)maxHyps * slots);
    pkey.ensure(512);
    pfail.ensure(512);
    key.ensure(2);
    part.ensure((size_t)kReduceMaxBlocksHost * 64);
    red.ensure(64);
    mask.ensure((size_t)maxN);
    count.ensure(1);
    bbox.ensure(4);
    one.ensure(512);
    h_counts.ensure((size_t)maxHyps * slots);
    h_red.ensure(64);
    if (model != MCV_MODEL_ESSENTIAL && model != MCV_MODEL_PNP) h_pack.ensure((size_t)maxN * 4);
    one.ensure(sizeof(EOneOut));
    h_one.ensure(sizeof(EOneOut));
    h_i.ensure(4);
}

size_t model_bytes(int model) {
    if (model == MCV_MODEL_PNP) return 96;
    if (affine_family(model)) return 24;
    return model == MCV_MODEL_ESSENTIAL ? 72 * kEModelSlots : (model == MCV_MODEL_FUNDAMENTAL ? 80 : 32);
}
int model_slots(int model) { return model == MCV_MODEL_ESSENTIAL ? kEModelSlots : 1; }
static bool f_seven(int model, const RansacConfig& cfg) {
    return model == MCV_MODEL_FUNDAMENTAL && (cfg.flags & MCV_FLAG_SEVEN_POINT) != 0;
}
int model_slots_cfg(int model, const RansacConfig& cfg) { return f_seven(model, cfg) ? kF7Slots : model_slots(model); }

hipStream_t Plan::own_stream() {
    if (!stream) MCV_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    return stream;
}

Plan::~Plan() {
    if (t_hstage_plan == this) t_hstage_plan = nullptr;
    if (t_hmfma_plan == this) t_hmfma_plan = nullptr;
    if (stream) (void)hipStreamDestroy(stream);
}

// Per-thread cached plans for the host-pointer exports (one per device and model).
Plan& thread_plan(int model, int shard) {
    int dev = 0;
    MCV_HIP(hipGetDevice(&dev));
    thread_local std::vector<std::unique_ptr<Plan>> plans;
    for (auto& p : plans)
        if (p->device == dev && p->model == model && p->shard == shard) return *p;
    plans.emplace_back(new Plan());
    plans.back()->device = dev;
    plans.back()->model = model;
    plans.back()->shard = shard;
    return *plans.back();
}

size_t point_bytes(int model, int N) {
    return (size_t)N * (model == MCV_MODEL_ESSENTIAL || model == MCV_MODEL_PNP ? 32 : 16);
}

// Device-resident point buffer of a plan (layout per model) and its size in bytes.
static void* plan_points(Plan& P, int N, size_t* bytes) {
    *bytes = point_bytes(P.model, N);
    return P.model == MCV_MODEL_ESSENTIAL || P.model == MCV_MODEL_PNP ? (void*)P.ptsd.p : (void*)P.pts.p;
}

void mark_chunk(Plan& P, int64_t begin, int64_t count, const Sampler& smp, const void* d_pts, int N, int kind,
                hipStream_t s) {
    P.fp.ensure(2);
    P.h_fp.ensure(2);
    P.last.set(begin, count, smp, d_pts, N, kind);
    launch_fingerprint(d_pts, point_bytes(P.model, N), P.fp.p, s);
}

void queue_chunk_check(Plan& P, const void* d_pts, int N, hipStream_t s) {
    launch_fingerprint(d_pts, point_bytes(P.model, N), P.fp.p + 1, s);
    MCV_HIP(hipMemcpyAsync(P.h_fp.p, P.fp.p, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
}

uint64_t device_fingerprint(Plan& P, const void* d_pts, int N, hipStream_t s) {
    P.fp.ensure(2);
    P.h_fp.ensure(2);
    launch_fingerprint(d_pts, point_bytes(P.model, N), P.fp.p + 1, s);
    MCV_HIP(hipMemcpyAsync(P.h_fp.p + 1, P.fp.p + 1, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    MCV_HIP(hipStreamSynchronize(s));
    return P.h_fp.p[1];
}

void pack_points(Plan& P, const mcvV2d* a, const mcvV2d* b, int N, float* d_dst, hipStream_t s) {
    P.h_pack.ensure((size_t)N * 4);
    float* h = P.h_pack.p;
    for (int i = 0; i < N; ++i) {   // OpenCV: points.convertTo(CV_32F)
        h[4 * i + 0] = (float)a[i].X;
        h[4 * i + 1] = (float)a[i].Y;
        h[4 * i + 2] = (float)b[i].X;
        h[4 * i + 3] = (float)b[i].Y;
    }
    MCV_HIP(hipMemcpyAsync(d_dst, h, (size_t)N * 16, hipMemcpyHostToDevice, s));
    MCV_HIP(hipStreamSynchronize(s));
}

double effective_threshold(const RansacConfig& cfg) { return cfg.threshold > 0 ? cfg.threshold : 3.0; }
bool fused_error(const RansacConfig& cfg) { return (cfg.flags & MCV_FLAG_FUSED_ERROR) != 0; }
bool fast_minimal(const RansacConfig& cfg) { return (cfg.flags & MCV_FLAG_FAST_MINIMAL) != 0; }

// HomographyEstimatorCallback::runKernel over the masked correspondences (mask == NULL: all).
bool h_refit(Plan& P, const float* d_pts, int N, const uint8_t* d_mask, hipStream_t s, double* H) {
    // the three passes (sums -> centroids -> |deviations| -> scales -> LtL) chained on the device,
    // one read-back; the host re-derives c4 / s4 with the same divisions and checks them
    double r[62];
    reduce_to_host(P, s, 62, r, [&](double* part, double* red) { h_refit_chain(d_pts, N, d_mask, part, red, s); });
    const double* sums = r;
    const double count = sums[4];
    if (count <= 0) return false;
    double c4[4] = {sums[0] / count, sums[1] / count, sums[2] / count, sums[3] / count};   // cm.x, cm.y, cM.x, cM.y
    const double* dev = r + 9;
    for (int k = 0; k < 4; ++k)
        if (std::fabs(dev[k]) < DBL_EPSILON) return false;
    double s4[4] = {count / dev[0], count / dev[1], count / dev[2], count / dev[3]};   // sm.x, sm.y, sM.x, sM.y
    const double* ltl = r + 17;
    double A[81], w[9], V[81];
    int o = 0;
    for (int j = 0; j < 9; ++j)
        for (int k = j; k < 9; ++k) { A[j * 9 + k] = ltl[o]; A[k * 9 + j] = ltl[o]; ++o; }
    jacobi_eigen(A, 9, w, V);
    const double* H0 = V + 8 * 9;   // eigenvector of the smallest eigenvalue
    const double invHnorm[9] = {1. / s4[0], 0, c4[0], 0, 1. / s4[1], c4[1], 0, 0, 1};
    const double Hnorm2[9] = {s4[2], 0, -c4[2] * s4[2], 0, s4[3], -c4[3] * s4[3], 0, 0, 1};
    double T[9], R[9];
    mat3_mul(invHnorm, H0, T);
    mat3_mul(T, Hnorm2, R);
    const double sc = 1. / R[8];
    for (int k = 0; k < 9; ++k) {
        H[k] = R[k] * sc;
        if (!std::isfinite(H[k])) return false;
    }
    return true;
}

// LMSolver::create(HomographyRefineCallback(src, dst), 10)->run(H8) — the classic LMSolverImpl
// (Marquardt-Nielsen lambda control, eigen-based solve). The O(N) JtJ / Jtr / |r|^2 sums run on
// the GPU; the 8x8 algebra runs here.
void h_lm_refine(Plan& P, const float* d_pts, int N, const uint8_t* d_mask, hipStream_t s, double* H, int maxIters) {
    auto compute = [&](const double* h, double* Aout, double* vout) -> double {
        double buf[45];
        reduce_to_host(P, s, 45, buf, [&](double* part, double* red) { h_reduce_lm(d_pts, N, d_mask, h, true, part, red, s); });
        return lm_unpack_sums<8>(buf, Aout, vout);
    };
    lm_solver_run<8>(compute, H, maxIters);   // H[0..7]; H[8] stays
}

// Evaluate one chunk of hypotheses on the device (generate + verify [+ best key]).
void evaluate_chunk(Plan& P, const void* d_ptsv, int N, const RansacConfig& cfg, int64_t hypBegin, int hypCount,
                    int* d_counts, uint64_t* d_key, hipStream_t s, bool needCounts) {
    if (P.model == MCV_MODEL_ESSENTIAL) {
        e_evaluate_chunk(P, (const double*)d_ptsv, N, cfg, hypBegin, hypCount, d_counts, s);
        if (d_key)
            launch_best(d_counts, hypCount * kEModelSlots, hypBegin * kEModelSlots, model_points(P.model), P.pkey.p,
                        P.pfail.p, d_key, s);
        MCV_HIP(hipGetLastError());
        return;
    }
    if (P.model == MCV_MODEL_PNP) {
        p_evaluate_chunk(P, d_ptsv, N, cfg, hypBegin, hypCount, d_counts, s);
        if (d_key)
            launch_best(d_counts, hypCount, hypBegin, model_points_cfg(P.model, cfg), P.pkey.p, P.pfail.p, d_key, s);
        MCV_HIP(hipGetLastError());
        return;
    }
    const float* d_pts = (const float*)d_ptsv;
    if (affine_family(P.model)) {
        a_evaluate_chunk(P, d_pts, N, cfg, hypBegin, hypCount, d_counts, s);
        if (d_key) launch_best(d_counts, hypCount, hypBegin, model_points(P.model), P.pkey.p, P.pfail.p, d_key, s);
        MCV_HIP(hipGetLastError());
        return;
    }
    const double t = effective_threshold(cfg);
    const float thr2 = (float)(t * t);
    if (P.model == MCV_MODEL_HOMOGRAPHY) {
        const bool fused = fused_error(cfg);
        P.pairs.ensure((size_t)(N + 1) / 2 * 8);
        launch_h_pair(d_pts, N, P.pairs.p, s);
        if (fused) {
            launch_bbox(d_pts, N, P.bbox.p, s);
        } else {
            P.bb4.ensure(4);
            launch_abs_bound4(d_pts, false, N, P.bb4.p, nullptr, s);
        }
        const Sampler smp = P.sampler(cfg);
        {
            ProfScope pg("h_generate", s);
            if (!fast_minimal(cfg)) P.hgen.ensure(h_gen_scratch_bytes(hypCount));
            launch_h_generate(d_pts, N, smp, hypBegin, hypCount, P.models.p, P.h64.p, d_counts, s,
                              fast_minimal(cfg), fast_minimal(cfg) ? nullptr : P.hgen.p);
        }
        // the winner's models can come straight from this chunk's buffers (h_finalize)
        mark_chunk(P, hypBegin, hypCount, smp, d_pts, N, fast_minimal(cfg) ? 21 : 20, s);
        // Staging decision. The certified sweep may run in self-pruning stages only where nobody reads
        // the per-hypothesis counts: the caller gets the key alone. The key stays exact. B is the full
        // count of one hypothesis with a model before any sampler failure (the candidate), so B <= the
        // winning count. A slot is dropped only when count-so-far + points-left < B: its full count is
        // below B, and so is the partial count it keeps (partial <= full). The candidate and every slot
        // that reaches the winning count are never dropped (the test is inclusive, so ties stay) and end
        // with full counts. The unchanged reduction below therefore packs, for each dropped slot, a key
        // below the candidate's whether it sees the partial or the full count (both < B; both map to key
        // 0 when B itself is below the minimum count), and the true key for every other slot: the same
        // maximum, the same lowest-index tie-break, the same minimum-count rule. Adaptive replay, LMedS,
        // callers that pass d_counts, the fused error and the other models keep the single full sweep.
        // The per-cell bound (h_cell_bound.h) drops slots before stage 1 on the same terms. A slot it drops has
        // a full count of at most UB (every correspondence of a certified cell is an outlier of the slot's
        // model under the op-by-op error: DESIGN.md §4), and UB < B. The count it keeps is its stage-0 partial,
        // at most its full count and so below B. The candidate's own UB is at least its full count B, and a
        // slot that reaches the winning count has UB >= that count >= B: neither is dropped (inclusive test).
        // Everything else above stands as written. Engaged where the size rule itself stages the call and
        // N >= kHCellMinN (kernels.h: the measured rows); forced staging of a small call keeps the plain stages.
        const bool stageable = !fused && d_key != nullptr && !needCounts;
        const bool staged = stageable && g_hstage_mode != 2 &&
                            (g_hstage_mode == 1 || (N >= kHStageMinN && (int64_t)N * hypCount >= kHStageMinEvals));
        P.hstageLast = staged ? 0 : (stageable && g_hstage_mode == 2 ? kHStageForcedOff : kHStageNotApplicable);
        t_hstage_plan = &P;
        const bool sized = N >= kHStageMinN && (int64_t)N * hypCount >= kHStageMinEvals;
        const bool cellBound = staged && g_hcell_mode != 2 && (g_hcell_mode == 1 || (sized && N >= kHCellMinN));
        if (staged) {
            P.hstageCtl.ensure(kHStageCtlInts);
            P.hstageList.ensure(2 * (size_t)hypCount);
            if (cellBound) P.hcells.ensure((size_t)h_cell_count(g_hcell_G, g_hcell_Gs) * kHCellInts);
        }
        // the certified sweep's matrix-core form where the size rule (or mcvTestHMfma) engages it: its
        // point records are written here, beside the pairs
        const int form = g_hmfma_mode;
        P.hmfmaLast = !fused && h_mfma_engages(N, hypCount, form, staged);
        t_hmfma_plan = &P;
        if (P.hmfmaLast) {
            P.hrec.ensure(h_rec_bytes(N));
            P.hmfmaStats.ensure(kHMfmaStats);
            launch_h_rec(d_pts, N, P.hrec.p, s);
        }
        const void* d_rec = P.hmfmaLast ? P.hrec.p : nullptr;
        unsigned long long* d_stats = P.hmfmaLast ? P.hmfmaStats.p : nullptr;
        ProfScope ps("h_verify", s);
        if (staged) {
            launch_h_verify_staged(d_pts, P.pairs.p, N, P.models.p, d_counts, hypCount, hypBegin, thr2, P.bb4.p,
                                   P.hstageCtl.p, P.hstageList.p, P.pkey.p, P.pfail.p, s, d_rec, d_stats, form,
                                   cellBound ? P.hcells.p : nullptr, g_hcell_G, g_hcell_Gs);
        } else if (!fused) {
            // default: OpenCV's op-by-op error, certified division-free sweep
            launch_h_verify_certified(d_pts, P.pairs.p, N, P.models.p, d_counts, hypCount, thr2, P.bb4.p, s, d_rec,
                                      d_stats, form);
        } else {
            launch_h_verify_packed(d_pts, P.pairs.p, N, P.models.p, d_counts, hypCount, thr2, P.bbox.p, s);
        }
    } else if (f_seven(P.model, cfg)) {
        // OpenCV FM_RANSAC: 7-point samples, 3 model slots per hypothesis (slot keys like essential)
        P.last.clear();
        launch_f7_generate(d_pts, N, P.sampler(cfg), hypBegin, hypCount, P.models.p, d_counts, s);
        P.bb4.ensure(4);
        launch_abs_bound4(d_pts, false, N, P.bb4.p, nullptr, s);
        {
            ProfScope ps("f_verify", s);
            launch_f_verify(d_pts, N, P.models.p, d_counts, hypCount * kF7Slots, thr2, f_error_kind(cfg), s, P.bb4.p);
        }
        if (d_key)
            launch_best(d_counts, hypCount * kF7Slots, hypBegin * kF7Slots, 7, P.pkey.p, P.pfail.p, d_key, s);
        MCV_HIP(hipGetLastError());
        return;
    } else {
        const Sampler smp = P.sampler(cfg);
        {
            ProfScope pg("f_generate", s);
            launch_f_generate(d_pts, N, smp, hypBegin, hypCount, P.models.p, d_counts, s, fast_minimal(cfg));
        }
        // the winner's fp64 model can come straight from this chunk's buffer (f_finalize)
        mark_chunk(P, hypBegin, hypCount, smp, d_pts, N, fast_minimal(cfg) ? 11 : 10, s);
        P.bb4.ensure(4);
        launch_abs_bound4(d_pts, false, N, P.bb4.p, nullptr, s);
        ProfScope ps("f_verify", s);
        launch_f_verify(d_pts, N, P.models.p, d_counts, hypCount, thr2, f_error_kind(cfg), s, P.bb4.p);
    }
    if (d_key) launch_best(d_counts, hypCount, hypBegin, model_points(P.model), P.pkey.p, P.pfail.p, d_key, s);
    MCV_HIP(hipGetLastError());
}

int model_points(int model) {
    if (model == MCV_MODEL_AFFINE) return 3;
    if (model == MCV_MODEL_SIMILARITY) return 2;
    return model == MCV_MODEL_FUNDAMENTAL ? 8 : (model == MCV_MODEL_ESSENTIAL ? 5 : 4);
}
// (homography and PnP with the AP3P kernel: 4)
int model_points_cfg(int model, const RansacConfig& cfg) {
    if (f_seven(model, cfg)) return 7;
    return model == MCV_MODEL_PNP && pnp_cfg_epnp(cfg) ? 5 : model_points(model);
}

// Winner -> mask (+ refit + LM). Returns inlier count, 0 on failure. Synchronises s.
int h_finalize(Plan& P, const float* d_pts, int N, const RansacConfig& cfg, int64_t hyp, double* H, uint8_t* d_mask,
               hipStream_t s) {
    const double t = effective_threshold(cfg);
    const float thr2 = (float)(t * t);
    // winner re-solve -> mask from the device-side record -> one read-back of both
    HOneOut* d_one = (HOneOut*)P.one.p;
    const Sampler smp = P.sampler(cfg);
    const bool cached = P.last.covers(hyp, smp, d_pts, N, fast_minimal(cfg) ? 21 : 20);
    if (cached) {
        // the winner's fp64 and fp32 models straight from the last chunk's buffers (the same code
        // produced them) instead of a single-lane eigen re-solve (~0.4 ms); a winner has status 1
        const int64_t local = hyp - P.last.begin;
        MCV_HIP(hipMemcpyAsync(d_one->H, P.h64.p + 9 * local, 9 * sizeof(double), hipMemcpyDeviceToDevice, s));
        MCV_HIP(hipMemcpyAsync(d_one->hf, P.models.p + local * sizeof(HModelF), sizeof(HModelF),
                               hipMemcpyDeviceToDevice, s));
        P.h_i.p[1] = 1;
        MCV_HIP(hipMemcpyAsync(&d_one->status, P.h_i.p + 1, sizeof(int), hipMemcpyHostToDevice, s));
        queue_chunk_check(P, d_pts, N, s);
    } else {
        launch_h_one(d_pts, N, smp, hyp, d_one, s, fast_minimal(cfg));
    }
    MCV_HIP(hipMemsetAsync(P.count.p, 0, sizeof(int), s));
    launch_h_mask_one(d_pts, N, d_one, thr2, fused_error(cfg), d_mask, P.count.p, s);
    MCV_HIP(hipGetLastError());
    HOneOut one;
    MCV_HIP(hipMemcpyAsync(P.h_one.p, d_one, sizeof(HOneOut), hipMemcpyDeviceToHost, s));
    MCV_HIP(hipMemcpyAsync(P.h_i.p, P.count.p, sizeof(int), hipMemcpyDeviceToHost, s));
    MCV_HIP(hipStreamSynchronize(s));
    if (cached && !chunk_fresh(P)) {   // the points changed since the chunk was evaluated: re-solve
        P.last.clear();
        return h_finalize(P, d_pts, N, cfg, hyp, H, d_mask, s);
    }
    std::memcpy(&one, P.h_one.p, sizeof(HOneOut));
    if (one.status != 1) fail("winning hypothesis %lld has no model (status %d)", (long long)hyp, one.status);
    const int count = P.h_i.p[0];
    for (int k = 0; k < 9; ++k) H[k] = one.H[k];
    if (cfg.flags & MCV_FLAG_NO_REFINE) return count;
    if (N > 4 && count > 0) {
        double Hr[9];
        if (h_refit(P, d_pts, N, d_mask, s, Hr))
            for (int k = 0; k < 9; ++k) H[k] = Hr[k];
        h_lm_refine(P, d_pts, N, d_mask, s, H, 10);
    }
    return count;
}

int finalize(Plan& P, const void* d_ptsv, int N, const RansacConfig& cfg, int64_t hyp, double* model9,
             uint8_t* d_mask, hipStream_t s) {
    if (P.model == MCV_MODEL_ESSENTIAL) return e_finalize(P, (const double*)d_ptsv, N, cfg, hyp, model9, d_mask, s);
    if (P.model == MCV_MODEL_PNP) return p_finalize(P, d_ptsv, N, cfg, hyp, model9, d_mask, s);
    const float* d_pts = (const float*)d_ptsv;
    if (P.model == MCV_MODEL_HOMOGRAPHY) return h_finalize(P, d_pts, N, cfg, hyp, model9, d_mask, s);
    if (affine_family(P.model)) return a_finalize(P, d_pts, N, cfg, hyp, model9, d_mask, s);
    return f_finalize(P, d_pts, N, cfg, hyp, model9, d_mask, s);
}

// Full RANSAC on device-resident points with the OpenCV sequential-replay semantics.
// cfg.deviceCount > 1: every chunk is split into that many contiguous hypothesis ranges evaluated
// concurrently by per-shard workspaces on devices 0, 1, ... (round-robin over the visible GPUs;
// points replicated once by peer copy), counts concatenated in order, then the same replay — the
// answer is identical to one device. Returns the best hypothesis (slot) index or -1.
int64_t ransac_search(Plan& P, const void* d_pts, int N, const RansacConfig& cfg, hipStream_t s,
                      const float* h_pts4) {
    const int m = model_points_cfg(P.model, cfg);
    const int slots = model_slots_cfg(P.model, cfg);
    // plans size their slot buffers by model_slots(model): a mode with more slots per hypothesis
    // (7-point F) reserves that many times the hypotheses
    const int64_t slotScale = slots / model_slots(P.model);
    mcvReplayState st;
    mcvReplayInit(&st, cfg.maxIters);
    const bool fixed = (cfg.flags & MCV_FLAG_FIXED_ITERS) != 0;
    int ndev = 1;
    MCV_HIP(hipGetDeviceCount(&ndev));
    const int shards = std::max(1, std::min(cfg.deviceCount, kMaxShards));
    int home = 0;
    MCV_HIP(hipGetDevice(&home));
    // the calling thread's device is restored on every exit, exceptions included (later calls on
    // this thread resolve their plans and allocations by the current device)
    struct DeviceRestore {
        int dev;
        ~DeviceRestore() { (void)hipSetDevice(dev); }
    } restore{home};
    struct Shard { Plan* P; const void* pts; hipStream_t s; int dev; };
    std::vector<Shard> sh;
    sh.push_back({&P, d_pts, s, home});
    // OpenCV's sample stream: the whole budget's subsets up front (niters only shrinks), uploaded to
    // every shard's workspace
    std::vector<int> table;
    uint64_t tableFp = 0;
    const int64_t tableRows = std::max(cfg.maxIters, 1);
    if (cv_sampler(cfg)) {
        std::vector<float> host;
        if (!h_pts4 && P.model != MCV_MODEL_ESSENTIAL && P.model != MCV_MODEL_PNP) {
            host.resize((size_t)N * 4);
            MCV_HIP(hipMemcpyAsync(host.data(), d_pts, (size_t)N * 16, hipMemcpyDeviceToHost, s));
            MCV_HIP(hipStreamSynchronize(s));
            h_pts4 = host.data();
        }
        cv_table_build(P.model, cfg, h_pts4, N, tableRows, table);
        tableFp = cv_table_points_fp(P.model, h_pts4, N);
        cv_table_upload(P, table, m, tableRows, N, tableFp, s);
    }
    if (shards > 1) {
        size_t bytes = 0;
        MCV_HIP(hipStreamSynchronize(s));
        for (int k = 1; k < shards; ++k) {
            const int dev = (home + k) % ndev;
            MCV_HIP(hipSetDevice(dev));
            Plan& Pk = thread_plan(P.model, k);
            Pk.reserve(N, slotScale);
            std::memcpy(Pk.pnpCam, P.pnpCam, sizeof(P.pnpCam));
            void* dst = plan_points(Pk, N, &bytes);
            hipStream_t sk = Pk.own_stream();
            MCV_HIP(hipMemcpyPeerAsync(dst, dev, d_pts, home, bytes, sk));
            if (cv_sampler(cfg)) cv_table_upload(Pk, table, m, tableRows, N, tableFp, sk);
            sh.push_back({&Pk, dst, sk, dev});
        }
        MCV_HIP(hipSetDevice(home));
    }
    int64_t begin = 0;
    // adaptive calls start small (niters shrinks with the first good model); a fixed budget is
    // evaluated in chunks of kChunkMax from the start
    int64_t chunk = std::min<int64_t>(std::max<int64_t>(st.niters, 1), fixed ? kChunkMax : kChunkFirst);
    P.h_keys.ensure(2 * kMaxShards);
    while (!st.stopped) {
        const int64_t remaining = st.niters - begin;
        if (remaining <= 0) break;
        const int cnt = (int)std::min<int64_t>(remaining, chunk);
        P.reserve(N, cnt * slotScale);
        const int nsh = std::min<int>((int)sh.size(), cnt);
        // fixed iterations: the sequential replay's answer is the first maximum over the counts >= m
        // before the first sampler failure, so each shard reduces its range on its own device to the
        // packed key (count << 32 | ~slot) + its first failure and sends 16 B; only a chunk with a
        // sampler failure (degenerate data) falls back to gathering the counts. Adaptive calls gather
        // the counts (4 B per model slot) and replay them in order.
        int64_t off = 0;
        for (int k = 0; k < nsh; ++k) {
            const int ck = (int)(cnt / nsh + (k < cnt % nsh ? 1 : 0));
            Shard& x = sh[k];
            if (k > 0) {
                MCV_HIP(hipSetDevice(x.dev));
                x.P->reserve(N, ck * slotScale);
            }
            // fixed: only the key is read (the counts only after a sampler failure, which unstages the chunk)
            evaluate_chunk(*x.P, x.pts, N, cfg, begin + off, ck, x.P->counts.p, fixed ? x.P->key.p : nullptr, x.s,
                           !fixed);
            if (fixed)
                MCV_HIP(hipMemcpyAsync(P.h_keys.p + 2 * k, x.P->key.p, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost,
                                       x.s));
            else
                MCV_HIP(hipMemcpyAsync(P.h_counts.p + off * slots, x.P->counts.p, (size_t)ck * slots * sizeof(int),
                                       hipMemcpyDeviceToHost, x.s));
            off += ck;
        }
        for (int k = 0; k < nsh; ++k) {
            if (k > 0) MCV_HIP(hipSetDevice(sh[k].dev));
            MCV_HIP(hipStreamSynchronize(sh[k].s));
        }
        bool replayed = false;
        if (fixed) {
            uint64_t best = 0;
            bool failed = false;
            for (int k = 0; k < nsh; ++k) {
                best = std::max(best, P.h_keys.p[2 * k]);
                failed = failed || (int64_t)P.h_keys.p[2 * k + 1] != INT64_MAX;
            }
            if (!failed) {
                const int c = (int)(best >> 32);
                if (best != 0 && c > std::max(st.bestCount, m - 1)) {
                    st.bestCount = c;
                    st.bestIndex = (int64_t)(0xFFFFFFFFull - (best & 0xFFFFFFFFull));
                }
                replayed = true;
            } else {   // a sampler failure inside the chunk: the counts, in order
                off = 0;
                for (int k = 0; k < nsh; ++k) {
                    const int ck = (int)(cnt / nsh + (k < cnt % nsh ? 1 : 0));
                    if (k > 0) MCV_HIP(hipSetDevice(sh[k].dev));
                    MCV_HIP(hipMemcpy(P.h_counts.p + off * slots, sh[k].P->counts.p, (size_t)ck * slots * sizeof(int),
                                      hipMemcpyDeviceToHost));
                    off += ck;
                }
            }
        }
        if (nsh > 1) MCV_HIP(hipSetDevice(home));
        if (!replayed) replay_chunk(&st, P.h_counts.p, begin, cnt, slots, N, m, cfg.confidence, fixed ? 1 : 0);
        begin += cnt;
        if (begin >= st.niters) st.stopped = 1;
        chunk = std::min<int64_t>(chunk * 2, kChunkMax);
    }
    return st.bestIndex;
}

// LMedS (LMeDSPointSetRegistrator::run restated): the whole budget is one chunk (it
// never exceeds maxIters and does not adapt), the medians come back as 4 B per model slot beside the
// statuses, and the scan below is OpenCV's loop: stop at the first sampler failure, first minimum wins.
int64_t lmeds_search(Plan& P, const float* d_pts, int N, const RansacConfig& cfg, hipStream_t s, const float* h_pts4,
                     double* sigma) {
    const int m = model_points_cfg(P.model, cfg);
    const int slots = model_slots_cfg(P.model, cfg);
    const bool fixed = (cfg.flags & MCV_FLAG_FIXED_ITERS) != 0;
    const int64_t niters = fixed ? cfg.maxIters : ransac_update_num_iters(cfg.confidence, 0.45, m, cfg.maxIters);
    if (niters <= 0) fail("LMedS: no hypotheses to evaluate (maxIters=%d)", cfg.maxIters);
    if (niters > kChunkMax) fail("LMedS: %lld hypotheses exceed the one-chunk budget %lld", (long long)niters, (long long)kChunkMax);
    if (N <= m) fail("LMedS: needs more than %d correspondences (N=%d)", m, N);
    const int cnt = (int)niters;
    const int nSlots = cnt * slots;
    P.reserve(N, (int64_t)cnt * (slots / model_slots(P.model)));
    if (cv_sampler(cfg)) cv_table_prepare(P, d_pts, h_pts4, N, cfg, niters, s);
    const Sampler smp = P.sampler(cfg);
    int errKind = 0;
    if (P.model == MCV_MODEL_HOMOGRAPHY) {
        errKind = fused_error(cfg) ? 1 : 0;
        if (!fast_minimal(cfg)) P.hgen.ensure(h_gen_scratch_bytes(cnt));
        launch_h_generate(d_pts, N, smp, 0, cnt, P.models.p, P.h64.p, P.counts.p, s, fast_minimal(cfg),
                          fast_minimal(cfg) ? nullptr : P.hgen.p);
        mark_chunk(P, 0, cnt, smp, d_pts, N, fast_minimal(cfg) ? 21 : 20, s);
    } else if (affine_family(P.model)) {
        errKind = fused_error(cfg) ? 1 : 0;
        P.last.clear();
        launch_a_generate(m, d_pts, N, smp, 0, cnt, P.models.p, P.h64.p, P.counts.p, s);
    } else if (f_seven(P.model, cfg)) {
        errKind = f_error_kind(cfg);
        P.last.clear();
        launch_f7_generate(d_pts, N, smp, 0, cnt, P.models.p, P.counts.p, s);
    } else {
        errKind = f_error_kind(cfg);
        launch_f_generate(d_pts, N, smp, 0, cnt, P.models.p, P.counts.p, s, fast_minimal(cfg));
        mark_chunk(P, 0, cnt, smp, d_pts, N, fast_minimal(cfg) ? 11 : 10, s);
    }
    P.med.ensure((size_t)nSlots);
    P.h_med.ensure((size_t)nSlots);
    {
        ProfScope ps("lmeds_select", s);
        launch_error_rank(P.model, d_pts, N, P.models.p, P.counts.p, nSlots, errKind, N / 2, P.med.p, s);
    }
    MCV_HIP(hipGetLastError());
    MCV_HIP(hipMemcpyAsync(P.h_counts.p, P.counts.p, (size_t)nSlots * sizeof(int), hipMemcpyDeviceToHost, s));
    MCV_HIP(hipMemcpyAsync(P.h_med.p, P.med.p, (size_t)nSlots * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    MCV_HIP(hipStreamSynchronize(s));
    int64_t best = -1;
    uint32_t bestKey = 0;
    for (int h = 0; h < cnt; ++h) {
        const int* c = P.h_counts.p + (size_t)h * slots;
        if (c[0] == kStatusNoSample) {
            if (h == 0) fail("LMedS: the sampler found no valid subset");
            break;
        }
        for (int k = 0; k < slots; ++k) {
            if (c[k] < 0) continue;
            const uint32_t key = P.h_med.p[(size_t)h * slots + k];
            if (best < 0 || key < bestKey) {
                best = (int64_t)h * slots + k;
                bestKey = key;
            }
        }
    }
    if (best < 0) fail("LMedS: no hypothesis gave a model");
    if (bestKey == kRankKeyNaN) fail("LMedS: the best median error is NaN");
    const double med = (double)rank_value(bestKey);
    *sigma = std::max(2.5 * 1.4826 * (1 + 5.0 / (N - m)) * std::sqrt(med), 0.001);
    return best;
}

void require_device() {
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        fail("no HIP device available (hipGetDeviceCount: %s, n=%d); the MI355X path has no CPU fallback",
             hipGetErrorString(e), n);
}

RansacConfig config_or_default(const RansacConfig* cfg) {
    if (cfg) return *cfg;
    RansacConfig c;
    std::memset(&c, 0, sizeof(c));
    c.threshold = 3.0;
    c.confidence = 0.995;
    c.maxIters = 2000;
    c.method = MCV_METHOD_RANSAC;
    c.flags = MCV_FLAG_CV_SAMPLER;   // no seed given: OpenCV's own sample stream
    return c;
}

}  // namespace mcv

// ------------------------------------------------------------------------------------------
// Exports
// ------------------------------------------------------------------------------------------
extern "C" MCV_API int cvFindHomography(const mcvV2d* src, const mcvV2d* dst, const int N, const RansacConfig* cfgp,
                                        mcvM33d* H, uint8_t* mask) {
    MCV_GUARD(0, {
        if (!src || !dst || !H || N < 0) fail("cvFindHomography: null argument or negative N");
        if (mask) std::memset(mask, 0, (size_t)N);
        if (N < 4) fail("cvFindHomography: need at least 4 correspondences (N=%d)", N);
        const RansacConfig cfg = config_or_default(cfgp);
        check_flags(cfg, "cvFindHomography");
        if (cfg.method != MCV_METHOD_RANSAC && cfg.method != MCV_METHOD_LSQ && cfg.method != MCV_METHOD_LMEDS)
            fail("cvFindHomography: unsupported method %d", cfg.method);
        if (cfg.method != MCV_METHOD_LSQ && !(cfg.confidence > 0 && cfg.confidence < 1))
            fail("cvFindHomography: confidence must be in (0,1)");
        require_device();
        Plan& P = thread_plan(MCV_MODEL_HOMOGRAPHY);
        hipStream_t s = P.own_stream();
        P.reserve(N, 1);
        pack_points(P, src, dst, N, P.pts.p, s);
        double Hm[9];
        int count = 0;
        if (cfg.method == MCV_METHOD_LSQ || N == 4) {
            if (!h_refit(P, P.pts.p, N, nullptr, s, Hm)) fail("cvFindHomography: degenerate point set");
            if (N > 4) h_lm_refine(P, P.pts.p, N, nullptr, s, Hm, 10);
            if (mask) std::memset(mask, 1, (size_t)N);
            count = N;
        } else if (cfg.method == MCV_METHOD_LMEDS) {
            // the winner's mask comes from the existing finalize with LMedS' own threshold
            RansacConfig fin = cfg;
            const int64_t best = lmeds_search(P, P.pts.p, N, cfg, s, P.h_pack.p, &fin.threshold);
            count = h_finalize(P, P.pts.p, N, fin, best, Hm, P.mask.p, s);
            if (count < 4) fail("cvFindHomography: LMedS model has %d inliers (< 4)", count);
            if (mask) {
                MCV_HIP(hipMemcpyAsync(mask, P.mask.p, (size_t)N, hipMemcpyDeviceToHost, s));
                MCV_HIP(hipStreamSynchronize(s));
            }
        } else {
            const int64_t best = ransac_search(P, P.pts.p, N, cfg, s, P.h_pack.p);
            if (best < 0) fail("cvFindHomography: RANSAC found no model with >= 4 inliers");
            count = h_finalize(P, P.pts.p, N, cfg, best, Hm, P.mask.p, s);
            if (mask) {
                MCV_HIP(hipMemcpyAsync(mask, P.mask.p, (size_t)N, hipMemcpyDeviceToHost, s));
                MCV_HIP(hipStreamSynchronize(s));
            }
        }
        for (int k = 0; k < 9; ++k) H->M[k] = Hm[k];
        return count;
    })
}

extern "C" MCV_API mcvRansacPlan* mcvRansacPlanCreate(int model, int maxN, int64_t maxHyps) {
    MCV_GUARD(nullptr, {
        if (model < MCV_MODEL_HOMOGRAPHY || model > MCV_MODEL_SIMILARITY)
            fail("unknown model %d", model);
        require_device();
        std::unique_ptr<Plan> p(new Plan());
        MCV_HIP(hipGetDevice(&p->device));
        p->model = model;
        p->reserve(std::max(maxN, 1), std::max<int64_t>(maxHyps, 1));
        return reinterpret_cast<mcvRansacPlan*>(p.release());
    })
}

extern "C" MCV_API void mcvRansacPlanDestroy(mcvRansacPlan* plan) {
    try {
        delete reinterpret_cast<Plan*>(plan);
    } catch (...) {
    }
}

extern "C" MCV_API int mcvPackCorrespondences(const mcvV2d* a, const mcvV2d* b, int N, float* d_pts4, void* stream) {
    MCV_GUARD(0, {
        if (!a || !b || !d_pts4 || N < 0) fail("mcvPackCorrespondences: bad argument");
        require_device();
        Plan& P = thread_plan(MCV_MODEL_HOMOGRAPHY);
        pack_points(P, a, b, N, d_pts4, (hipStream_t)stream);
        return 1;
    })
}

namespace mcv {
// The CV-sampler table of P cannot serve hypotheses [.., rowsNeeded) of a search over these points:
// a search that starts at 0 (begin == 0), too few rows, another sample size, another N, or (H / F,
// whose checkSubset reads the points) other point content. The content check synchronises s.
static bool cv_table_stale(Plan& P, const void* d_pts, int N, const RansacConfig& cfg, int64_t begin,
                           int64_t rowsNeeded, hipStream_t s) {
    if (begin == 0 || P.subsetRows < rowsNeeded || P.subsetM != model_points_cfg(P.model, cfg) || P.subsetN != N)
        return true;
    return cv_table_reads_points(P.model) && device_fingerprint(P, d_pts, N, s) != P.subsetFp;
}
}  // namespace mcv

extern "C" MCV_API int mcvRansacEvaluate(mcvRansacPlan* plan, const void* d_pts4, int N, const RansacConfig* cfg,
                                         int64_t hypBegin, int64_t hypCount, uint64_t* d_key, int* d_counts,
                                         void* stream) {
    MCV_GUARD(0, {
        Plan* P = reinterpret_cast<Plan*>(plan);
        if (!P || !d_pts4 || !cfg || !d_key) fail("mcvRansacEvaluate: null argument");
        if (N < model_points_cfg(P->model, *cfg)) fail("mcvRansacEvaluate: N=%d below the minimal sample", N);
        const int64_t scale = model_slots_cfg(P->model, *cfg) / model_slots(P->model);
        if (hypCount <= 0 || hypCount * scale > P->maxHyps)
            fail("mcvRansacEvaluate: hypCount %lld (x%lld slots) outside plan capacity %lld", (long long)hypCount,
                 (long long)scale, (long long)P->maxHyps);
        if (hypBegin < 0 || (hypBegin + hypCount) * model_slots_cfg(P->model, *cfg) > 0xFFFFFFFFll)
            fail("mcvRansacEvaluate: hypothesis (slot) index beyond 2^32");
        check_flags(*cfg, "mcvRansacEvaluate");
        if (cfg->method == MCV_METHOD_LMEDS)
            fail("mcvRansacEvaluate: LMedS (method 4) has no device-level form; use cvFindHomography / "
                 "cvFindFundamentalMat / cvEstimateAffine2D / cvEstimateAffinePartial2D");
        if (cv_sampler(*cfg) && cv_table_stale(*P, d_pts4, N, *cfg, hypBegin, hypBegin + hypCount, (hipStream_t)stream))
            // a search starts at hypothesis 0, and a table drawn for other points is never reused: the
            // stream is rebuilt from the current points
            cv_table_prepare(*P, d_pts4, nullptr, N, *cfg, std::max<int64_t>(hypBegin + hypCount, cfg->maxIters),
                             (hipStream_t)stream);
        evaluate_chunk(*P, d_pts4, N, *cfg, hypBegin, (int)hypCount, d_counts ? d_counts : P->counts.p, d_key,
                       (hipStream_t)stream, d_counts != nullptr);
        return 1;
    })
}

// Test hook (declared in minicv_native.h). stats[16]: [0] -1 no homography evaluate on this thread yet,
// 0 the stages pruned, else why not (kHStage*); [1] B; [2] stages; [3..9] stage boundaries in points;
// [10..15] slots alive entering each stage. Call after synchronising the evaluate's stream.
extern "C" MCV_API int mcvTestHStaging(int mode, long long* stats) {
    MCV_GUARD(-1, {
        const int prev = g_hstage_mode;
        if (mode >= 0 && mode <= 2) g_hstage_mode = mode;
        if (stats) {
            for (int i = 0; i < 16; ++i) stats[i] = 0;
            const Plan* P = t_hstage_plan;
            stats[0] = P ? P->hstageLast : -1;
            if (P && P->hstageLast == 0) {
                int ctl[kHStageCtlInts];
                MCV_HIP(hipMemcpy(ctl, P->hstageCtl.p, sizeof(ctl), hipMemcpyDeviceToHost));
                const int N = P->last.N;
                stats[0] = ctl[kCtlReason];
                stats[1] = ctl[kCtlB];
                stats[2] = ctl[kCtlStages];
                for (int i = 0; i <= kHStageMax; ++i)
                    stats[3 + i] = std::min<long long>(2LL * ctl[kCtlBound + i], N);
                for (int i = 0; i < kHStageMax; ++i) stats[10 + i] = ctl[kCtlAlive + i];
            }
        }
        return prev;
    })
}

// Test hook (declared in minicv_native.h): the per-cell bound's switch, grids and the last evaluate's figures.
extern "C" MCV_API int mcvTestHCellMode(int mode, int G, int Gs, long long* stats) {
    MCV_GUARD(-1, {
        const int prev = g_hcell_mode;
        if (mode >= 0 && mode <= 2) g_hcell_mode = mode;
        if (G >= 1 && G <= kHCellMaxG) g_hcell_G = G;
        if (Gs >= 1 && Gs <= kHCellMaxGs) g_hcell_Gs = Gs;
        if (stats) {
            for (int i = 0; i < 6; ++i) stats[i] = 0;
            stats[4] = g_hcell_G;
            stats[5] = g_hcell_Gs;
            const Plan* P = t_hstage_plan;
            if (P && P->hstageLast == 0) {
                int ctl[kHStageCtlInts];
                MCV_HIP(hipMemcpy(ctl, P->hstageCtl.p, sizeof(ctl), hipMemcpyDeviceToHost));
                const int cells = ctl[kCtlCells];
                stats[0] = cells > 0;
                stats[2] = ctl[kCtlAlive + 1];
                stats[3] = cells;
                if (cells > 0) {
                    std::vector<int> tab((size_t)cells * kHCellInts);
                    MCV_HIP(hipMemcpy(tab.data(), P->hcells.p, tab.size() * sizeof(int), hipMemcpyDeviceToHost));
                    for (int c = 0; c < cells; ++c) stats[1] += tab[(size_t)c * kHCellInts + kHCellInts - 1] > 0;
                }
            }
        }
        return prev;
    })
}

// Test hook (declared in minicv_native.h): the cell build and the bound on given data, device or host twin.
extern "C" MCV_API int mcvTestHCellBound(const float* pts4, int N, const float* cand8, const float* models8,
                                         int nModels, float thr2, int B, int G, int Gs, int device, int* cellId,
                                         float* boxes, int* sizes, int* ub, unsigned int* bits, int* alive) {
    MCV_GUARD(0, {
        if (!pts4 || !cand8 || !models8 || !cellId || !boxes || !sizes || !ub || !bits || !alive)
            fail("mcvTestHCellBound: null argument");
        if (N <= 0 || nModels <= 0 || G < 1 || G > kHCellMaxG || Gs < 1 || Gs > kHCellMaxGs)
            fail("mcvTestHCellBound: bad sizes");
        if (!device) {
            h_cell_host(pts4, N, cand8, models8, nModels, thr2, B, G, Gs, cellId, boxes, sizes, ub, bits, alive);
            return 1;
        }
        require_device();
        const int cells = h_cell_count(G, Gs), words = (cells + 31) / 32;
        DevBuf<float> p, m, cand;
        DevBuf<double> bb;
        DevBuf<int> ctl, tab, cnt, list, dub, did;
        DevBuf<uint32_t> dbits;
        p.ensure((size_t)N * 4);
        m.ensure((size_t)nModels * 8);
        cand.ensure(8);
        bb.ensure(4);
        ctl.ensure(kHStageCtlInts);
        tab.ensure((size_t)cells * kHCellInts);
        cnt.ensure(nModels);
        list.ensure(nModels);
        dub.ensure(nModels);
        did.ensure(N);
        dbits.ensure((size_t)nModels * words);
        MCV_HIP(hipMemcpy(p.p, pts4, (size_t)N * 16, hipMemcpyHostToDevice));
        MCV_HIP(hipMemcpy(m.p, models8, (size_t)nModels * 32, hipMemcpyHostToDevice));
        MCV_HIP(hipMemcpy(cand.p, cand8, 32, hipMemcpyHostToDevice));
        MCV_HIP(hipMemset(cnt.p, 0, (size_t)nModels * sizeof(int)));
        MCV_HIP(hipMemset(dbits.p, 0, (size_t)nModels * words * sizeof(uint32_t)));
        // a control block that names slot 0 of `cand` as the candidate (key: count 1, hypothesis 0)
        int hctl[kHStageCtlInts] = {0};
        const uint64_t key = (1ull << 32) | 0xFFFFFFFFull;
        memcpy(hctl + kCtlKey, &key, sizeof(key));
        MCV_HIP(hipMemcpy(ctl.p, hctl, sizeof(hctl), hipMemcpyHostToDevice));
        launch_abs_bound4(p.p, false, N, bb.p, nullptr, 0);
        launch_h_stage_count(p.p, N, cand.p, 0, thr2, ctl.p, bb.p, tab.p, G, Gs, did.p, 0);
        MCV_HIP(hipDeviceSynchronize());
        // B as given (the kernel counted the candidate's inliers into the same word)
        MCV_HIP(hipMemcpy(ctl.p + kCtlB, &B, sizeof(int), hipMemcpyHostToDevice));
        launch_h_cell_bound(m.p, cnt.p, nModels, thr2, bb.p, tab.p, G, Gs, ctl.p, list.p, dub.p, dbits.p, 0);
        MCV_HIP(hipGetLastError());
        MCV_HIP(hipDeviceSynchronize());
        std::vector<int> htab((size_t)cells * kHCellInts);
        MCV_HIP(hipMemcpy(htab.data(), tab.p, htab.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int c = 0; c < cells; ++c) {
            for (int j = 0; j < 8; ++j) boxes[8 * c + j] = h_cell_dec(htab[(size_t)c * kHCellInts + j]);
            sizes[c] = htab[(size_t)c * kHCellInts + kHCellInts - 1];
        }
        MCV_HIP(hipMemcpy(cellId, did.p, (size_t)N * sizeof(int), hipMemcpyDeviceToHost));
        MCV_HIP(hipMemcpy(ub, dub.p, (size_t)nModels * sizeof(int), hipMemcpyDeviceToHost));
        MCV_HIP(hipMemcpy(bits, dbits.p, (size_t)nModels * words * sizeof(uint32_t), hipMemcpyDeviceToHost));
        MCV_HIP(hipMemcpy(hctl, ctl.p, sizeof(hctl), hipMemcpyDeviceToHost));
        *alive = hctl[kCtlAlive + 1];
        return 1;
    })
}

// Test hook (declared in minicv_native.h). stats[3]: the undecided rows, the overflowed waves and the
// out-of-domain waves of the
// calling thread's last certified homography sweep. Call after synchronising the sweep's stream.
extern "C" MCV_API int mcvTestHMfma(int mode, long long* stats) {
    MCV_GUARD(-1, {
        const int prev = g_hmfma_mode;
        if (mode >= kHFormAuto && mode <= kHFormMixed) g_hmfma_mode = mode;
        if (stats) {
            unsigned long long v[kHMfmaStats];
            for (int i = 0; i < kHMfmaStats; ++i) v[i] = t_hmfma_last[i];
            const Plan* P = t_hmfma_plan;
            if (P) {
                for (int i = 0; i < kHMfmaStats; ++i) v[i] = 0;
                if (P->hmfmaLast) MCV_HIP(hipMemcpy(v, P->hmfmaStats.p, sizeof(v), hipMemcpyDeviceToHost));
            }
            for (int i = 0; i < kHMfmaStats; ++i) stats[i] = (long long)v[i];
        }
        return prev;
    })
}

extern "C" MCV_API int mcvRansacFinalize(mcvRansacPlan* plan, const void* d_pts4, int N, const RansacConfig* cfg,
                                         int64_t hypIndex, double* model9, uint8_t* d_mask, void* stream) {
    MCV_GUARD(0, {
        Plan* P = reinterpret_cast<Plan*>(plan);
        if (!P || !d_pts4 || !cfg || !model9 || !d_mask) fail("mcvRansacFinalize: null argument");
        if (hypIndex < 0) fail("mcvRansacFinalize: no winning hypothesis");
        check_flags(*cfg, "mcvRansacFinalize");
        P->reserve(N, 1);
        const int64_t hyp = hypIndex / model_slots_cfg(P->model, *cfg);
        if (cv_sampler(*cfg) && cv_table_stale(*P, d_pts4, N, *cfg, 1, hyp + 1, (hipStream_t)stream))
            cv_table_prepare(*P, d_pts4, nullptr, N, *cfg, std::max<int64_t>(hyp + 1, cfg->maxIters),
                             (hipStream_t)stream);
        return finalize(*P, d_pts4, N, *cfg, hypIndex, model9, d_mask, (hipStream_t)stream);
    })
}

extern "C" MCV_API int mcvHostHypothesis(int model, const float* pts4, int N, uint64_t seed, int64_t hyp,
                                         double* model9, float* modelf9, int* sampleIdx) {
    MCV_GUARD(kStatusNoSample - 1, {
        if (!pts4 || !model9 || !modelf9) fail("mcvHostHypothesis: null argument");
        const bool fast = (model & MCV_HOST_FAST_MINIMAL) != 0;
        model &= ~MCV_HOST_FAST_MINIMAL;
        if (model == MCV_MODEL_HOMOGRAPHY) {
            if (N < 4) fail("N < 4");
            HModelF mf;
            for (int k = 0; k < 9; ++k) model9[k] = 0;
            for (int k = 0; k < 8; ++k) mf.h[k] = 0;
            EigWsLocal ws;
            const int st = h_hypothesis(pts4, N, Sampler{seed, nullptr}, (uint64_t)hyp, model9, &mf, sampleIdx, ws,
                                        fast);
            for (int k = 0; k < 8; ++k) modelf9[k] = mf.h[k];
            modelf9[8] = 1.f;
            return st;
        }
        if (affine_family(model)) {
            const int m = model_points(model);
            if (N < m) fail("N < %d", m);
            AModelF mf;
            double A[6];
            for (int k = 0; k < 6; ++k) { A[k] = 0; mf.a[k] = 0; }
            int idx[3] = {-1, -1, -1};
            const Sampler smp{seed, nullptr};
            const int st = m == 3 ? a_hypothesis<3>(pts4, N, smp, (uint64_t)hyp, A, &mf, idx)
                                  : a_hypothesis<2>(pts4, N, smp, (uint64_t)hyp, A, &mf, idx);
            for (int k = 0; k < 6; ++k) { model9[k] = A[k]; modelf9[k] = mf.a[k]; }
            if (sampleIdx) for (int k = 0; k < m; ++k) sampleIdx[k] = idx[k];
            return st;
        }
        return f_host_hypothesis(pts4, N, seed, hyp, model9, modelf9, sampleIdx, fast);
    })
}

extern "C" MCV_API void mcvHostPhilox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                      uint32_t* out4) {
    U4 c;
    c.x = c0; c.y = c1; c.z = c2; c.w = c3;
    const U4 r = philox4x32_10(c, k0, k1);
    out4[0] = r.x; out4[1] = r.y; out4[2] = r.z; out4[3] = r.w;
}

extern "C" MCV_API int cvFindFundamentalMat(const mcvV2d* a, const mcvV2d* b, const int N, const RansacConfig* cfgp,
                                            mcvM33d* F, uint8_t* mask) {
    MCV_GUARD(0, {
        if (!a || !b || !F || N < 0) fail("cvFindFundamentalMat: null argument or negative N");
        if (mask) std::memset(mask, 0, (size_t)N);
        RansacConfig cfg = config_or_default(cfgp);
        if (!cfgp) cfg.confidence = 0.99;
        check_flags(cfg, "cvFindFundamentalMat");
        const bool seven = (cfg.flags & MCV_FLAG_SEVEN_POINT) != 0;
        if (seven && cfg.method == MCV_METHOD_RANSAC && N != 7 && N < 15)
            fail("cvFindFundamentalMat: 7-point FM_RANSAC needs N >= 15 (OpenCV uses LMeDS below that: use method 4; "
                 "N=%d)", N);
        if (!seven && N < 8) fail("cvFindFundamentalMat: need at least 8 correspondences (N=%d)", N);
        if (seven && N < 7) fail("cvFindFundamentalMat: need at least 7 correspondences (N=%d)", N);
        if (cfg.method != MCV_METHOD_RANSAC && cfg.method != MCV_METHOD_LSQ && cfg.method != MCV_METHOD_LMEDS)
            fail("cvFindFundamentalMat: unsupported method %d", cfg.method);
        if (cfg.method != MCV_METHOD_LSQ && !(cfg.confidence > 0 && cfg.confidence < 1))
            fail("cvFindFundamentalMat: confidence must be in (0,1)");
        require_device();
        Plan& P = thread_plan(MCV_MODEL_FUNDAMENTAL);
        hipStream_t s = P.own_stream();
        P.reserve(N, 1);
        pack_points(P, a, b, N, P.pts.p, s);
        double Fm[9];
        int count = 0;
        if (seven && N == 7) {
            // findFundamentalMat with npoints == 7: run7Point once (the first of its models), mask all 1
            launch_f7_direct(P.pts.p, (FOneOut*)P.one.p, s);
            MCV_HIP(hipGetLastError());
            FOneOut one;
            MCV_HIP(hipMemcpyAsync(P.h_one.p, P.one.p, sizeof(FOneOut), hipMemcpyDeviceToHost, s));
            MCV_HIP(hipStreamSynchronize(s));
            std::memcpy(&one, P.h_one.p, sizeof(FOneOut));
            if (one.status <= 0) fail("cvFindFundamentalMat: degenerate 7-point set");
            for (int k = 0; k < 9; ++k) Fm[k] = one.F[k];
            if (mask) std::memset(mask, 1, (size_t)N);
            count = N;
        } else if (cfg.method == MCV_METHOD_LSQ || (N == 8 && !(seven && cfg.method == MCV_METHOD_LMEDS))) {
            count = f_fit_all(P, P.pts.p, N, s, Fm);
            if (count <= 0) fail("cvFindFundamentalMat: degenerate point set");
            if (mask) std::memset(mask, 1, (size_t)N);
        } else if (cfg.method == MCV_METHOD_LMEDS) {
            // 8-point, or 7-point at any N > 7 (the range below 15 is where OpenCV itself runs LMedS)
            RansacConfig fin = cfg;
            const int64_t best = lmeds_search(P, P.pts.p, N, cfg, s, P.h_pack.p, &fin.threshold);
            count = f_finalize(P, P.pts.p, N, fin, best, Fm, P.mask.p, s);
            if (count < (seven ? 7 : 8)) fail("cvFindFundamentalMat: LMedS model has %d inliers (< %d)", count, seven ? 7 : 8);
            if (mask) {
                MCV_HIP(hipMemcpyAsync(mask, P.mask.p, (size_t)N, hipMemcpyDeviceToHost, s));
                MCV_HIP(hipStreamSynchronize(s));
            }
        } else {
            const int64_t best = ransac_search(P, P.pts.p, N, cfg, s, P.h_pack.p);
            if (best < 0) fail("cvFindFundamentalMat: RANSAC found no model with >= %d inliers", seven ? 7 : 8);
            count = f_finalize(P, P.pts.p, N, cfg, best, Fm, P.mask.p, s);
            if (mask) {
                MCV_HIP(hipMemcpyAsync(mask, P.mask.p, (size_t)N, hipMemcpyDeviceToHost, s));
                MCV_HIP(hipStreamSynchronize(s));
            }
        }
        for (int k = 0; k < 9; ++k) F->M[k] = Fm[k];
        return count;
    })
}
