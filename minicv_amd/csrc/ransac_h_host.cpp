// ransac_h_host.cpp — host side of the homography family behind the C-ABI.
//
// cvFindHomography (new export, conventions of cvRecoverPose, MiniCVNative.cpp:197-215):
//   pack V2d -> float4 on device  ->  RANSAC or LMedS of the shared framework (ransac_host.cpp) over
//   h_evaluate (generate + the certified / staged / matrix-core / packed sweep; the decisions and
//   their exactness argument are in it)  ->  h_finalize: mask of the winner, refit on its inliers (runKernel:
//   GPU reductions + 9x9 Jacobi here), 10 Levenberg-Marquardt iterations (GPU reductions + 8x8 solve here).
// Mirrors cv::findHomography(..., RANSAC, thr, mask, maxIters, conf) of OpenCV 4.x
// [ext: calib3d/src/fundam.cpp, ptsetreg.cpp, levmarq.cpp — absent here, SURVEY.md §8c].
// Also here: the homography test hooks (mcvTestHStaging, mcvTestHCellMode, mcvTestHCellBound, mcvTestHCellRel,
// mcvTestHCellPre, mcvTestHCellPreVerdicts, mcvTestHMfma, mcvTestHGenRow, mcvTestHGenerate, mcvHostHGenRow,
// mcvHostHStagePlan, mcvTestHCellSecondPass, mcvTestHListPush).
#include "minicv_native.h"
#include "mcv_runtime.h"
#include "kernels.h"
#include "linalg.h"
#include "mcv_common.h"
#include "hyp_homography.h"
#include "h_cell_bound.h"
#include "h_cell_pre.h"
#include "plan.h"
#include "lm_solver.h"

#include <cmath>
#include <cfloat>
#include <cstring>
#include <vector>
#include <algorithm>

namespace mcv {

// mcvTestHStaging: 0 automatic, 1 staging regardless of the call's size, 2 never (tests only)
static int g_hstage_mode = 0;
// the plan of the calling thread's last homography evaluate (mcvTestHStaging reads its control block)
static thread_local Plan* t_hstage_plan = nullptr;
// mcvTestHCellMode: the per-cell bound before stage 1: 0 automatic, 1 whenever the sweep is staged, 2 never;
// its two grids
static int g_hcell_mode = 0;
static int g_hcell_G = kHCellG, g_hcell_Gs = kHCellGs;
// mcvTestHCellSecondPass: the bound's second pass: 0 the rule (and mcvTestHCellMode's mode 1), 2 never
static int g_hcell_rel_mode = 0;
// mcvTestHCellPre: the box test's fp32 prefilter (h_cell_pre.h): 0 automatic (on), 1 off; and where the calling
// thread's last bound passes left their counters: a plan's device counters, or a hook call's own figures
static int g_hcell_pre_mode = 0;
static bool g_hcell_pre_count = false;   // staged evaluates count only once the hook was called (two atomics a wave)
// mcvTestHStage0Slots: the slots stage 0 sweeps where the bound runs: 0 the rule (kernels.h), else that many
static int g_hstage0_slots = 0;
static thread_local Plan* t_hcell_pre_plan = nullptr;
// mcvTestHGenRow: the generate's certified one-row pass 2: 0 automatic (key-only op-by-op evaluates of the eigen
// solver from kHRowMinHyps hypotheses), 1 wherever it applies, 2 never, 3 as 1 with err times 2^40
static int g_hrow_mode = 0;
static const int kHRowMinHyps = 1 << 14;   // below, pass 2 is a few microseconds either way and the launches count
static thread_local Plan* t_hrow_plan = nullptr;
static thread_local long long t_hcell_pre_last[2] = {0, 0};
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
// Plan::~Plan: no thread-local of this file may outlive the plan it names
void h_plan_forget(const Plan* P) {
    if (t_hstage_plan == P) t_hstage_plan = nullptr;
    if (t_hmfma_plan == P) t_hmfma_plan = nullptr;
    if (t_hcell_pre_plan == P) t_hcell_pre_plan = nullptr;
    if (t_hrow_plan == P) t_hrow_plan = nullptr;
}

// The host half of HomographyEstimatorCallback::runKernel on a refit record (kernels.h kRefit*): the single
// call's and every batched problem's. It re-derives c4 / s4 with the device's divisions and checks them.
bool h_refit_from_record(const double* r, double* H) {
    const double* sums = r + kRefitSums;
    const double count = r[kRefitCount];
    if (count <= 0) return false;
    double c4[4] = {sums[0] / count, sums[1] / count, sums[2] / count, sums[3] / count};   // cm.x, cm.y, cM.x, cM.y
    const double* dev = r + kRefitDev;
    for (int k = 0; k < 4; ++k)
        if (std::fabs(dev[k]) < DBL_EPSILON) return false;
    double s4[4] = {count / dev[0], count / dev[1], count / dev[2], count / dev[3]};   // sm.x, sm.y, sM.x, sM.y
    const double* ltl = r + kRefitLtL;
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

// HomographyEstimatorCallback::runKernel over the masked correspondences (mask == NULL: all): the three
// passes (sums -> centroids -> |deviations| -> scales -> LtL) chained on the device, one read-back.
bool h_refit(Plan& P, const float* d_pts, int N, const uint8_t* d_mask, hipStream_t s, double* H) {
    double r[kRefitDoubles];
    reduce_to_host(P, s, kRefitDoubles, r,
                   [&](double* part, double* red) { h_refit_chain(d_pts, N, d_mask, part, red, s); });
    return h_refit_from_record(r, H);
}

// LMSolver::create(HomographyRefineCallback(src, dst), 10)->run(H8) — the classic LMSolverImpl
// (Marquardt-Nielsen lambda control, eigen-based solve). The O(N) JtJ / Jtr / |r|^2 sums run on
// the GPU; the 8x8 algebra runs here.
void h_lm_refine(Plan& P, const float* d_pts, int N, const uint8_t* d_mask, hipStream_t s, double* H, int maxIters) {
    auto sums = [&](const double* h, double* buf) {
        reduce_to_host(P, s, 45, buf,
                       [&](double* part, double* red) { h_reduce_lm(d_pts, N, d_mask, h, part, red, s); });
    };
    lm_solver_run<8>(sums, H, maxIters);   // H[0..7]; H[8] stays
}

static ChunkSolver h_solver(const RansacConfig& cfg) { return fast_minimal(cfg) ? kSolverHElimination : kSolverHEigen; }

// One chunk of hypotheses: models, statuses, and P.last = this chunk (the winner's models can come straight
// from its buffers: h_finalize). Shared by the RANSAC evaluate below and lmeds_search.
// certifiedRow: the one-row pass 2 (kernels.h). P.h64 then holds only some of the chunk's models; its one reader,
// h_finalize's cached branch, replays the winner from the log the plan still holds (P.hrowLogKept) first.
static void h_generate_chunk(Plan& P, const float* d_pts, int N, const RansacConfig& cfg, int64_t hypBegin,
                             int hypCount, int* d_counts, hipStream_t s, bool certifiedRow) {
    const Sampler smp = P.sampler(cfg);
    certifiedRow = certifiedRow && !fast_minimal(cfg);
    if (!fast_minimal(cfg)) P.hgen.ensure(h_gen_scratch_bytes(hypCount));
    launch_h_generate(d_pts, N, smp, hypBegin, hypCount, P.models.p, P.h64.p, d_counts, s, fast_minimal(cfg),
                      fast_minimal(cfg) ? nullptr : P.hgen.p, certifiedRow);
    P.hrowLast = certifiedRow;
    P.hrowLogKept = certifiedRow && h_gen_row_log_kept(hypCount);
    P.hrowCount = hypCount;
    t_hrow_plan = &P;
    mark_chunk(P, hypBegin, hypCount, smp, d_pts, N, h_solver(cfg), s);
}
void h_generate(Plan& P, const void* d_pts, int N, const RansacConfig& cfg, int64_t hypBegin, int hypCount,
                int* d_counts, hipStream_t s) {
    h_generate_chunk(P, (const float*)d_pts, N, cfg, hypBegin, hypCount, d_counts, s, false);
}

// Generate + verify one chunk of hypotheses. keyOnly: the caller consumes only the chunk's best key
// (evaluate_chunk's reduction over d_counts), never the per-hypothesis counts.
void h_evaluate(Plan& P, const void* d_ptsv, int N, const RansacConfig& cfg, int64_t hypBegin, int hypCount,
                int* d_counts, bool keyOnly, hipStream_t s) {
    const float* d_pts = (const float*)d_ptsv;
    const float thr2 = thr2_of(P, cfg);
    const bool fused = fused_error(cfg);
    P.pairs.ensure((size_t)(N + 1) / 2 * 8);
    launch_h_pair(d_pts, N, P.pairs.p, s);
    if (fused) {
        launch_bbox(d_pts, N, P.bbox.p, s);
    } else {
        P.bb4.ensure(4);
        launch_abs_bound4(d_pts, false, N, P.bb4.p, nullptr, s);
    }
    {
        ProfScope pg("h_generate", s);
        // the certified one-row pass 2 where only the key leaves the evaluate (the staged sweep's own condition)
        const bool row = keyOnly && !fused && !fast_minimal(cfg) && g_hrow_mode != 2 &&
                         (g_hrow_mode != 0 || hypCount >= kHRowMinHyps);
        if (row) h_gen_row_err_scale(g_hrow_mode == 3);
        h_generate_chunk(P, d_pts, N, cfg, hypBegin, hypCount, d_counts, s, row);
    }
    // Staging decision. The certified sweep may run in self-pruning stages only where nobody reads
    // the per-hypothesis counts: the caller gets the key alone. The key stays exact. B is the full
    // count of one hypothesis with a model before any sampler failure (the candidate), so B <= the
    // winning count. A slot is dropped only when count-so-far + points-left < B: its full count is
    // below B, and so is the partial count it keeps (partial <= full). The candidate and every slot
    // that reaches the winning count are never dropped (the test is inclusive, so ties stay) and end
    // with full counts. The unchanged reduction (evaluate_chunk) therefore packs, for each dropped slot, a key
    // below the candidate's whether it sees the partial or the full count (both < B; both map to key
    // 0 when B itself is below the minimum count), and the true key for every other slot: the same
    // maximum, the same lowest-index tie-break, the same minimum-count rule. Adaptive replay, LMedS,
    // callers that pass d_counts, the fused error and the other models keep the single full sweep.
    // The per-cell bound (h_cell_bound.h) drops slots before stage 1 on the same terms. A slot it drops has
    // a full count of at most UB (every correspondence of a certified cell is an outlier of the slot's
    // model under the op-by-op error: DESIGN.md §4), and UB < B. The count it keeps is its stage-0 partial,
    // at most its full count and so below B. The candidate's own UB is at least its full count B, and a
    // slot that reaches the winning count has UB >= that count >= B: neither is dropped (inclusive test).
    // The bound's second pass adds the candidate-relative test on the cells of the candidate's inliers: more
    // certified cells with the same meaning (every correspondence of the cell is an outlier of the slot's model
    // under the op-by-op error), so UB stays an upper bound and the paragraph above holds as it stands. With h
    // = the candidate the relative form is negative, so the candidate certifies none of its own inlier cells.
    // Both passes put a certified fp32 prefilter in front of the box test (h_cell_pre.h): a decided verdict is the
    // fp64 test's, the rest run fp64, so UB, the lists and `left` are the same bits either way.
    // Stage 0 on a leading subset of the slots (with the bound, from kHStage0MinHyps hypotheses or by the hook): its
    // counts go to a scratch buffer and only name the candidate; any slot with a model before the first failure
    // serves, so B is still one hypothesis' full count and B <= the winning count. The counts buffer keeps what
    // the generate wrote (0 or a status) until stage 1, which runs its list from point 0. Dropped slots: a slot the
    // bound drops now holds 0 instead of a stage-0 partial; 0 is at most its full count and below B (a slot is
    // dropped only on UB < B, so B >= 1). B = 0 and the minimum-count rule: with B = 0 nothing has UB < B, nothing
    // is dropped, and a key below the minimum count maps to 0 from 0 as from any partial. Sampler failure: the
    // subset's reduction does not see the other slots' statuses, so one more pass over every status gives the
    // chunk's first failure; the plan takes the earlier of the two, and any failure switches pruning off
    // (kHStageSamplerFailure) with stage 1 running every slot from 0 to the end: full counts for the host's
    // fallback. No candidate among the subset (key 0), and the late-boundary rule: the same, every slot from 0 to
    // the end. Recount marks: kStatusRedo marks of slots outside the subset first appear in stage 1; every
    // compaction reads them (count < 0: not listed) and the recount runs once, behind the last stage, as for the
    // marks stage 1 always could set; a mark stage 0 left in the scratch buffer is set again by stage 1, which
    // tests the same model against the same extents.
    // With the bound the later compactions read points-left per slot: left = the correspondences not yet
    // processed that lie in cells the bound did not certify for the slot's model. The unprocessed points of
    // certified cells are outliers of that model, so only `left` of the N - processed points can still add to
    // the count: full count <= count-so-far + left <= count-so-far + N - processed. A slot dropped on
    // count-so-far + left < B has a full count below B, exactly what the first paragraph needs of a dropped
    // slot; the candidate (full count B) and every slot that reaches the winning count have count-so-far +
    // left >= full count >= B at every boundary and are never dropped (inclusive test, so ties stay).
    // Everything else above stands as written. Engaged where the size rule itself stages the call and
    // N >= kHCellMinN (kernels.h: the measured rows); forced staging of a small call keeps the plain stages.
    // The half boundary (where the bound's second pass runs: one more boundary in the middle of stage 1's range,
    // kernels.h) is one more place where the same test runs, on the same terms: a slot dropped there on
    // count-so-far + left < B has a full count below B, with `left` its own third row of the per-slot figures,
    // built for that boundary exactly as the other two. The sentence above covers "every boundary", so the
    // candidate and the winners pass this one too. Without the second pass `left` is N - processed, with which
    // nothing can be dropped before the first pruning boundary: there the plan keeps its four stages.
    // An empty stage (boundaries that coincide: B near N puts the first pruning boundary on the prefix, a range
    // of one trip puts the half boundary on its start) adds nothing to any count; the compaction behind it
    // applies the test to the unchanged counts and hands the list on. With pruning off on the device
    // (reason != 0) the stage behind boundary 1 runs every slot to the end and every later list stays empty.
    // The test stays in mcv_h_stage_compact: run in the tail of the stage kernel's own waves (one atomic per
    // wave of 6 slots, where the compaction then took one per 64 and now takes one per block of 1024) it was
    // measured slower ("The half boundary").
    const bool stageable = !fused && keyOnly;
    const bool sized = N >= kHStageMinN && (int64_t)N * hypCount >= kHStageMinEvals;
    const bool staged = stageable && g_hstage_mode != 2 && (g_hstage_mode == 1 || sized);
    P.hstageLast = staged ? 0 : (stageable && g_hstage_mode == 2 ? kHStageForcedOff : kHStageNotApplicable);
    t_hstage_plan = &P;
    const bool cellBound = staged && g_hcell_mode != 2 && (g_hcell_mode == 1 || (sized && N >= kHCellMinN));
    // the bound's second pass costs a slot the same whatever N and saves in proportion to N (kernels.h)
    const bool cellRel = cellBound && g_hcell_rel_mode != 2 && (g_hcell_mode == 1 || N >= kHCellRelMinN);
    // stage 0 on a leading subset of the slots, where the bound runs and the chunk is large (or the hook says so)
    int stage0Slots = 0;
    if (cellBound) {
        if (g_hstage0_slots > 0) stage0Slots = g_hstage0_slots;
        else if (hypCount >= kHStage0MinHyps) stage0Slots = std::max(kHStage0MinSlots, hypCount / kHStage0Div);
        if (stage0Slots >= hypCount) stage0Slots = 0;
    }
    if (staged) {
        P.hstageCtl.ensure(kHStageCtlInts);
        P.hstageList.ensure(2 * (size_t)hypCount);
        if (cellBound) {
            const size_t cells = (size_t)h_cell_count(g_hcell_G, g_hcell_Gs);
            P.hcells.ensure(cells * kHCellInts);
            P.hcellRec.ensure(h_cell_rec_ints((int)cells));
            if (stage0Slots) P.hstage0.ensure((size_t)stage0Slots);
            P.hcellPreStats.ensure(2);
            if (cellRel) {
                P.hcellId.ensure((size_t)N);
                P.hcellPref.ensure(cells * kHStageCellLater);
                P.hcellLeft.ensure((size_t)hypCount * kHStageCellLater);
            }
        }
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
    t_hcell_pre_plan = cellBound && g_hcell_pre_count ? &P : nullptr;
    t_hcell_pre_last[0] = t_hcell_pre_last[1] = 0;
    ProfScope ps("h_verify", s);
    if (staged) {
        launch_h_verify_staged(d_pts, P.pairs.p, N, P.models.p, d_counts, hypCount, hypBegin, thr2, P.bb4.p,
                               P.hstageCtl.p, P.hstageList.p, P.pkey.p, P.pfail.p, s, d_rec, d_stats, form,
                               cellBound ? P.hcells.p : nullptr, g_hcell_G, g_hcell_Gs,
                               cellRel ? HCellBufs{P.hcellId.p, P.hcellPref.p, P.hcellLeft.p}
                                       : HCellBufs{nullptr, nullptr, nullptr},
                               cellBound ? HCellPreBufs{P.hcellRec.p, g_hcell_pre_mode == 0,
                                                        g_hcell_pre_count ? P.hcellPreStats.p : nullptr}
                                         : HCellPreBufs{nullptr, 0, nullptr},
                               stage0Slots ? P.hstage0.p : nullptr, stage0Slots);
    } else if (!fused) {
        // default: OpenCV's op-by-op error, certified division-free sweep
        launch_h_verify_certified(d_pts, P.pairs.p, N, P.models.p, d_counts, hypCount, thr2, P.bb4.p, s, d_rec,
                                  d_stats, form);
    } else {
        launch_h_verify_packed(d_pts, P.pairs.p, N, P.models.p, d_counts, hypCount, thr2, P.bbox.p, s);
    }
}

// Winner -> mask (+ refit + LM). Returns inlier count, 0 on failure. Synchronises s.
int h_finalize(Plan& P, const void* d_ptsv, int N, const RansacConfig& cfg, int64_t hyp, double* H, uint8_t* d_mask,
               hipStream_t s) {
    const float* d_pts = (const float*)d_ptsv;
    // winner re-solve -> mask from the device-side record -> one read-back of both
    HOneOut* d_one = (HOneOut*)P.one.p;
    const Sampler smp = P.sampler(cfg);
    bool cached = P.last.covers(hyp, smp, d_pts, N, h_solver(cfg));
    // a chunk of the one-row pass 2 holds the winner's fp64 model only after its exact replay from the chunk's
    // log; where the log is gone (a chunk of more than one piece), the single-lane solve as for a winner outside
    if (cached && P.hrowLast && !P.hrowLogKept) cached = false;
    if (cached) {
        if (P.hrowLast)
            launch_h_gen_v_one(d_pts, P.hrowCount, (int)(hyp - P.last.begin), P.hgen.p, P.models.p, P.h64.p, s);
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
    zero_count(P, s);
    launch_h_mask_one(d_pts, N, d_one, thr2_of(P, cfg), fused_error(cfg), d_mask, P.count.p, s);
    MCV_HIP(hipGetLastError());
    queue_one<HOneOut>(P, s);
    queue_count(P, s);
    MCV_HIP(hipStreamSynchronize(s));
    if (cached && !chunk_fresh(P)) {   // the points changed since the chunk was evaluated: re-solve
        P.last.clear();
        return h_finalize(P, d_pts, N, cfg, hyp, H, d_mask, s);
    }
    const HOneOut one = take_one<HOneOut>(P);
    if (one.status != 1) fail("winning hypothesis %lld has no model (status %d)", (long long)hyp, one.status);
    const int count = take_count(P);
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

int h_host_hypothesis(int, const float* pts4, int N, uint64_t seed, int64_t hyp, double* model9, float* modelf9,
                      int* sampleIdx, bool fast) {
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

// The 2-D entry's direct cases, least squares (method 0) and N == 4: runKernel on all points, then the refine.
bool h_entry_direct(Plan& P, const char* who, int N, const RansacConfig& cfg, hipStream_t s, double* H) {
    if (cfg.method != MCV_METHOD_LSQ && N != 4) return false;
    if (!h_refit(P, P.pts.p, N, nullptr, s, H)) fail("%s: degenerate point set", who);
    if (N > 4) h_lm_refine(P, P.pts.p, N, nullptr, s, H, 10);
    return true;
}

}  // namespace mcv

using namespace mcv;

extern "C" MCV_API int cvFindHomography(const mcvV2d* src, const mcvV2d* dst, const int N, const RansacConfig* cfgp,
                                        mcvM33d* H, uint8_t* mask) {
    MCV_GUARD(0, {
        return find_model_2d(MCV_MODEL_HOMOGRAPHY, "cvFindHomography", src, dst, N, cfgp, H ? H->M : nullptr, mask);
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
        t_hcell_pre_plan = nullptr;
        t_hcell_pre_last[0] = t_hcell_pre_last[1] = 0;
        if (!device) {
            h_cell_host(pts4, N, cand8, models8, nModels, thr2, B, G, Gs, cellId, boxes, sizes, ub, bits, alive,
                        g_hcell_pre_mode == 0, t_hcell_pre_last);
            return 1;
        }
        require_device();
        const int cells = h_cell_count(G, Gs), words = (cells + 31) / 32;
        DevBuf<float> p, m, cand;
        DevBuf<unsigned long long> pst;
        DevBuf<double> bb;
        DevBuf<int> ctl, tab, cnt, list, dub, did, pre;
        DevBuf<uint32_t> dbits;
        pre.ensure(h_cell_rec_ints(cells));
        pst.ensure(2);
        MCV_HIP(hipMemset(pst.p, 0, 2 * sizeof(unsigned long long)));
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
        launch_h_cell_pre(tab.p, G, Gs, thr2, pre.p, 0);
        launch_h_cell_bound(m.p, cnt.p, nModels, thr2, bb.p, tab.p, G, Gs, ctl.p, list.p, dub.p, dbits.p, 0, nullptr,
                            nullptr, 0, 0, HCellPreBufs{pre.p, g_hcell_pre_mode == 0, pst.p});
        MCV_HIP(hipGetLastError());
        MCV_HIP(hipDeviceSynchronize());
        MCV_HIP(hipMemcpy(t_hcell_pre_last, pst.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
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

// Test hook (declared in minicv_native.h): the per-cell bound's second pass (box test + candidate-relative
// test, UB, the `left` figures) on given data and boundaries, device or host twin.
extern "C" MCV_API int mcvTestHCellRel(const float* pts4, int N, const float* cand8, const float* models8, int nModels,
                                       float thr2, int B, int G, int Gs, const int* bounds, int nBounds, int device,
                                       int* cellId, int* ub, unsigned int* bits, int* left, int* alive) {
    MCV_GUARD(0, {
        if (!pts4 || !cand8 || !models8 || !bounds || !cellId || !ub || !bits || !left || !alive)
            fail("mcvTestHCellRel: null argument");
        if (N <= 0 || nModels <= 0 || G < 1 || G > kHCellMaxG || Gs < 1 || Gs > kHCellMaxGs || nBounds < 1 ||
            nBounds > kHCellLater)
            fail("mcvTestHCellRel: bad sizes");
        for (int j = 0; j < nBounds; ++j)
            if (bounds[j] < 0 || bounds[j] > (N + 1) / 2) fail("mcvTestHCellRel: boundary out of range");
        t_hcell_pre_plan = nullptr;
        t_hcell_pre_last[0] = t_hcell_pre_last[1] = 0;
        if (!device) {
            h_cell_rel_host(pts4, N, cand8, models8, nModels, thr2, B, G, Gs, bounds, nBounds, cellId, ub, bits, left,
                            alive, g_hcell_pre_mode == 0, t_hcell_pre_last);
            return 1;
        }
        require_device();
        const int cells = h_cell_count(G, Gs), words = (cells + 31) / 32;
        DevBuf<float> p, m, cand;
        DevBuf<int> pre;
        DevBuf<unsigned long long> pst;
        pre.ensure(h_cell_rec_ints(cells));
        pst.ensure(2);
        MCV_HIP(hipMemset(pst.p, 0, 2 * sizeof(unsigned long long)));
        DevBuf<double> bb;
        DevBuf<int> ctl, tab, list, dub, did, pref, dleft;
        DevBuf<uint32_t> dbits;
        p.ensure((size_t)N * 4);
        m.ensure((size_t)nModels * 8);
        cand.ensure(8);
        bb.ensure(4);
        ctl.ensure(kHStageCtlInts);
        tab.ensure((size_t)cells * kHCellInts);
        list.ensure(nModels);
        dub.ensure(nModels);
        did.ensure(N);
        pref.ensure((size_t)cells * nBounds);
        dleft.ensure((size_t)nModels * nBounds);
        dbits.ensure((size_t)nModels * words);
        MCV_HIP(hipMemcpy(p.p, pts4, (size_t)N * 16, hipMemcpyHostToDevice));
        MCV_HIP(hipMemcpy(m.p, models8, (size_t)nModels * 32, hipMemcpyHostToDevice));
        MCV_HIP(hipMemcpy(cand.p, cand8, 32, hipMemcpyHostToDevice));
        MCV_HIP(hipMemset(dbits.p, 0, (size_t)nModels * words * sizeof(uint32_t)));
        // a control block that names slot 0 of `cand` as the candidate and carries the given boundaries
        int hctl[kHStageCtlInts] = {0};
        const uint64_t key = (1ull << 32) | 0xFFFFFFFFull;
        memcpy(hctl + kCtlKey, &key, sizeof(key));
        for (int j = 0; j < nBounds; ++j) hctl[kCtlBound + 2 + j] = bounds[j];
        MCV_HIP(hipMemcpy(ctl.p, hctl, sizeof(hctl), hipMemcpyHostToDevice));
        launch_abs_bound4(p.p, false, N, bb.p, nullptr, 0);
        launch_h_stage_count(p.p, N, cand.p, 0, thr2, ctl.p, bb.p, tab.p, G, Gs, did.p, 0);
        MCV_HIP(hipDeviceSynchronize());
        MCV_HIP(hipMemcpy(ctl.p + kCtlB, &B, sizeof(int), hipMemcpyHostToDevice));
        launch_h_cell_prefix(did.p, N, ctl.p, nBounds, G, Gs, pref.p, 0);
        launch_h_cell_pre(tab.p, G, Gs, thr2, pre.p, 0);
        launch_h_cell_rel(m.p, cand.p, 0, nModels, thr2, bb.p, tab.p, G, Gs, pref.p, nBounds, ctl.p, nullptr, list.p,
                          dleft.p, dub.p, dbits.p, 0, HCellPreBufs{pre.p, g_hcell_pre_mode == 0, pst.p});
        MCV_HIP(hipGetLastError());
        MCV_HIP(hipDeviceSynchronize());
        MCV_HIP(hipMemcpy(t_hcell_pre_last, pst.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        MCV_HIP(hipMemcpy(cellId, did.p, (size_t)N * sizeof(int), hipMemcpyDeviceToHost));
        MCV_HIP(hipMemcpy(ub, dub.p, (size_t)nModels * sizeof(int), hipMemcpyDeviceToHost));
        MCV_HIP(hipMemcpy(bits, dbits.p, (size_t)nModels * words * sizeof(uint32_t), hipMemcpyDeviceToHost));
        MCV_HIP(hipMemcpy(left, dleft.p, (size_t)nModels * nBounds * sizeof(int), hipMemcpyDeviceToHost));
        MCV_HIP(hipMemcpy(hctl, ctl.p, sizeof(hctl), hipMemcpyDeviceToHost));
        *alive = hctl[kCtlAlive + 1];
        return 1;
    })
}

// Test hook (declared in minicv_native.h): the survivor lists themselves, as the staged sweep's kernels push them.
// The box pass with the second pass behind it (two lists), the second pass over the first pass's list, then two
// compactions on the given counts: one through the stage-1 list with the per-slot `left`, one over every slot with
// the points not yet processed. Every list comes back with its length; entries no kernel wrote read -1.
extern "C" MCV_API int mcvTestHListPush(const float* pts4, int N, const float* cand8, const float* models8, int nModels,
                                        float thr2, int B, int G, int Gs, int boundPairs, const int* counts,
                                        int* lists, int* lens) {
    MCV_GUARD(0, {
        if (!pts4 || !cand8 || !models8 || !counts || !lists || !lens) fail("mcvTestHListPush: null argument");
        if (N <= 0 || nModels <= 0 || G < 1 || G > kHCellMaxG || Gs < 1 || Gs > kHCellMaxGs || boundPairs < 0 ||
            boundPairs > (N + 1) / 2)
            fail("mcvTestHListPush: bad sizes");
        require_device();
        const int cells = h_cell_count(G, Gs);
        DevBuf<float> p, m, cand;
        DevBuf<double> bb;
        DevBuf<int> ctl, tab, cnt, out, did, rec, pref, dleft;
        rec.ensure(h_cell_rec_ints(cells));
        p.ensure((size_t)N * 4);
        m.ensure((size_t)nModels * 8);
        cand.ensure(8);
        bb.ensure(4);
        ctl.ensure(kHStageCtlInts);
        tab.ensure((size_t)cells * kHCellInts);
        cnt.ensure(nModels);
        out.ensure(4 * (size_t)nModels);
        did.ensure(N);
        pref.ensure(cells);
        dleft.ensure(nModels);
        int *dPre = out.p, *dStage1 = out.p + nModels, *dNext = out.p + 2 * (size_t)nModels,
            *dAll = out.p + 3 * (size_t)nModels;
        MCV_HIP(hipMemcpy(p.p, pts4, (size_t)N * 16, hipMemcpyHostToDevice));
        MCV_HIP(hipMemcpy(m.p, models8, (size_t)nModels * 32, hipMemcpyHostToDevice));
        MCV_HIP(hipMemcpy(cand.p, cand8, 32, hipMemcpyHostToDevice));
        MCV_HIP(hipMemcpy(cnt.p, counts, (size_t)nModels * sizeof(int), hipMemcpyHostToDevice));
        MCV_HIP(hipMemset(out.p, 0xFF, 4 * (size_t)nModels * sizeof(int)));
        // a control block that names slot 0 of `cand` as the candidate; stages 2 and 3 both start at the boundary
        int hctl[kHStageCtlInts] = {0};
        const uint64_t key = (1ull << 32) | 0xFFFFFFFFull;
        memcpy(hctl + kCtlKey, &key, sizeof(key));
        hctl[kCtlBound + 2] = hctl[kCtlBound + 3] = boundPairs;
        MCV_HIP(hipMemcpy(ctl.p, hctl, sizeof(hctl), hipMemcpyHostToDevice));
        launch_abs_bound4(p.p, false, N, bb.p, nullptr, 0);
        launch_h_stage_count(p.p, N, cand.p, 0, thr2, ctl.p, bb.p, tab.p, G, Gs, did.p, 0);
        MCV_HIP(hipDeviceSynchronize());
        MCV_HIP(hipMemcpy(ctl.p + kCtlB, &B, sizeof(int), hipMemcpyHostToDevice));
        const HCellPreBufs pre{rec.p, g_hcell_pre_mode == 0, nullptr};
        launch_h_cell_prefix(did.p, N, ctl.p, 1, G, Gs, pref.p, 0);
        launch_h_cell_pre(tab.p, G, Gs, thr2, rec.p, 0);
        launch_h_cell_bound(m.p, cnt.p, nModels, thr2, bb.p, tab.p, G, Gs, ctl.p, dStage1, nullptr, nullptr, 0, dPre,
                            dleft.p, 1, N, pre);
        launch_h_cell_rel(m.p, cand.p, 0, nModels, thr2, bb.p, tab.p, G, Gs, pref.p, 1, ctl.p, dPre, dStage1, dleft.p,
                          nullptr, nullptr, 0, pre);
        launch_h_stage_compact(cnt.p, nModels, N, ctl.p, 2, dStage1, dNext, dleft.p, 0);
        launch_h_stage_compact(cnt.p, nModels, N, ctl.p, 3, nullptr, dAll, nullptr, 0);
        MCV_HIP(hipGetLastError());
        MCV_HIP(hipDeviceSynchronize());
        MCV_HIP(hipMemcpy(lists, out.p, 4 * (size_t)nModels * sizeof(int), hipMemcpyDeviceToHost));
        MCV_HIP(hipMemcpy(hctl, ctl.p, sizeof(hctl), hipMemcpyDeviceToHost));
        lens[0] = hctl[kCtlPre];
        lens[1] = hctl[kCtlAlive + 1];
        lens[2] = hctl[kCtlAlive + 2];
        lens[3] = hctl[kCtlAlive + 3];
        return 1;
    })
}

// Test hook (declared in minicv_native.h): the slots stage 0 sweeps where the per-cell bound runs.
extern "C" MCV_API int mcvTestHStage0Slots(int slots) {
    MCV_GUARD(-1, {
        const int prev = g_hstage0_slots;
        if (slots >= 0) g_hstage0_slots = slots;
        return prev;
    })
}

// Test hook (declared in minicv_native.h): the switch of the per-cell bound's second pass.
extern "C" MCV_API int mcvTestHCellSecondPass(int mode) {
    MCV_GUARD(-1, {
        const int prev = g_hcell_rel_mode;
        if (mode == 0 || mode == 2) g_hcell_rel_mode = mode;
        return prev;
    })
}

// Host hook (declared in minicv_native.h): the stage plan the staged sweep's planner kernel computes, by the same
// function and with the same constants (h_stage_plan_host, ransac_h_stage.hip). No device is touched.
extern "C" MCV_API int mcvHostHStagePlan(int N, int candidate, int failure, int B, int cellBound, int subset,
                                         int* out) {
    MCV_GUARD(-1, {
        if (N < 4 || B < 0 || B > N || cellBound < 0 || cellBound > 2 || !out)
            fail("mcvHostHStagePlan: bad arguments");
        int pa = 0;
        const HStagePlan pl = h_stage_plan_host(N, candidate != 0, failure != 0, B, cellBound != 0, cellBound == 2,
                                                subset != 0, &pa);
        out[0] = pl.reason;
        out[1] = pl.stages;
        out[2] = pa;
        for (int i = 0; i <= kHStageMax; ++i) out[3 + i] = pl.bound[i];
        return pl.stages;
    })
}

// Test hook (declared in minicv_native.h): the prefilter's switch and the counters of the calling thread's last
// bound passes (a staged evaluate: call after synchronising its stream) or hook call.
extern "C" MCV_API int mcvTestHCellPre(int mode, long long* stats) {
    MCV_GUARD(-1, {
        const int prev = g_hcell_pre_mode;
        if (mode == 0 || mode == 1) g_hcell_pre_mode = mode;
        g_hcell_pre_count = true;
        if (stats) {
            unsigned long long v[2] = {(unsigned long long)t_hcell_pre_last[0], (unsigned long long)t_hcell_pre_last[1]};
            const Plan* P = t_hcell_pre_plan;
            if (P) MCV_HIP(hipMemcpy(v, P->hcellPreStats.p, sizeof(v), hipMemcpyDeviceToHost));
            stats[0] = (long long)(v[0] - v[1]);
            stats[1] = (long long)v[1];
        }
        return prev;
    })
}

// Test hook (declared in minicv_native.h): the generate's certified one-row pass 2 and the lane figures of the
// calling thread's last homography generate (read after its stream was synchronised).
extern "C" MCV_API int mcvTestHGenRow(int mode, long long* stats) {
    MCV_GUARD(-1, {
        const int prev = g_hrow_mode;
        if (mode >= 0 && mode <= 3) g_hrow_mode = mode;
        if (stats) {
            int v[2] = {0, 0};
            const Plan* P = t_hrow_plan;
            if (P && P->hrowLast)
                MCV_HIP(hipMemcpy(v, h_gen_row_stats(P->hgen.p, P->hrowCount), sizeof(v), hipMemcpyDeviceToHost));
            stats[0] = v[0];
            stats[1] = v[1];
        }
        return prev;
    })
}

// Test hook (declared in minicv_native.h): the split generate alone on host points, exact or one-row pass 2.
extern "C" MCV_API int mcvTestHGenerate(const float* pts4, int N, uint64_t seed, const int* table, int64_t hypBegin,
                                        int hypCount, int row, float* models8, int* counts, long long* stats) {
    MCV_GUARD(0, {
        if (!pts4 || !models8 || !counts) fail("mcvTestHGenerate: null argument");
        if (N < 4 || hypBegin < 0 || hypCount <= 0 || row < 0 || row > 2) fail("mcvTestHGenerate: bad arguments");
        require_device();
        DevBuf<float> p;
        DevBuf<uint8_t> m, scratch;
        DevBuf<double> h64;
        DevBuf<int> c, tab;
        p.ensure((size_t)N * 4);
        m.ensure((size_t)hypCount * sizeof(HModelF));
        h64.ensure((size_t)hypCount * 9);
        c.ensure((size_t)hypCount);
        scratch.ensure(h_gen_scratch_bytes(hypCount));
        MCV_HIP(hipMemcpy(p.p, pts4, (size_t)N * 16, hipMemcpyHostToDevice));
        if (table) {
            tab.ensure((size_t)(hypBegin + hypCount) * 4);
            MCV_HIP(hipMemcpy(tab.p, table, (size_t)(hypBegin + hypCount) * 16, hipMemcpyHostToDevice));
        }
        // every slot must be written by the generate: a byte pattern no model or status has
        MCV_HIP(hipMemset(m.p, 0xA5, (size_t)hypCount * sizeof(HModelF)));
        MCV_HIP(hipMemset(c.p, 0xA5, (size_t)hypCount * sizeof(int)));
        h_gen_row_err_scale(row == 2);
        launch_h_generate(p.p, N, Sampler{seed, table ? tab.p : nullptr}, hypBegin, hypCount, m.p, h64.p, c.p, 0, false,
                          scratch.p, row != 0);
        MCV_HIP(hipGetLastError());
        MCV_HIP(hipDeviceSynchronize());
        h_gen_row_err_scale(false);
        MCV_HIP(hipMemcpy(models8, m.p, (size_t)hypCount * sizeof(HModelF), hipMemcpyDeviceToHost));
        MCV_HIP(hipMemcpy(counts, c.p, (size_t)hypCount * sizeof(int), hipMemcpyDeviceToHost));
        if (stats) {
            int v[2] = {0, 0};
            if (row) MCV_HIP(hipMemcpy(v, h_gen_row_stats(scratch.p, hypCount), sizeof(v), hipMemcpyDeviceToHost));
            stats[0] = v[0];
            stats[1] = v[1];
        }
        return 1;
    })
}

// Host twin (declared in minicv_native.h): the one-row pass 2 beside the exact solve, hypothesis by hypothesis.
extern "C" MCV_API int mcvHostHGenRow(const float* pts4, int N, uint64_t seed, const int* table, int64_t hypBegin,
                                      int hypCount, int errHuge, float* modelsRow8, float* modelsFwd8, int* statusFwd,
                                      int* decided, double* err, double* dev) {
    MCV_GUARD(0, {
        if (!pts4 || !modelsRow8 || !modelsFwd8 || !statusFwd || !decided || !err || !dev)
            fail("mcvHostHGenRow: null argument");
        if (N < 4 || hypBegin < 0 || hypCount <= 0) fail("mcvHostHGenRow: bad arguments");
        const Sampler smp{seed, table};
        std::vector<EigRot> log(192);
        for (int64_t q = 0; q < hypCount; ++q) {
            const uint64_t hyp = (uint64_t)(hypBegin + q);
            // the exact path: the one-pass solve (the split generate's models are its bits)
            double H[9];
            HModelF mf;
            EigWsLocal ws;
            for (int k = 0; k < 8; ++k) mf.h[k] = 0;
            statusFwd[q] = h_hypothesis(pts4, N, smp, hyp, H, &mf, nullptr, ws);
            for (int k = 0; k < 8; ++k) modelsFwd8[8 * q + k] = statusFwd[q] == 1 ? mf.h[k] : 0.f;
            decided[q] = 0;
            err[q] = dev[q] = 0;
            for (int k = 0; k < 8; ++k) modelsRow8[8 * q + k] = 0.f;
            // pass 1 as mcv_h_gen_aw runs it: the logged solve on the upper triangle and W
            float sx[4], sy[4], dx[4], dy[4];
            int idx[4];
            double nm[8];
            double aw[kEigWs];   // the host form of the logged solve still sends its skipped pairs to the junk slot
            aw[kEigJunk] = 0.0;
            EigWsLane wl{aw};
            if (!h_sample(pts4, N, smp, hyp, sx, sy, dx, dy, idx)) continue;
            if (!h_norm4(sx, sy, dx, dy, nm) || !h_ltl4(sx, sy, dx, dy, nm, wl)) continue;
            double w[9];
            int nrot = 0;
            const int r = eig9_jacobi<EigWsLane, true>(wl, w, 8, &nrot, log.data(), 1, (int)log.size());
            if (nrot < 0) continue;   // log overflow: the one-pass kernel's lane, undecided
            double y[9], e = 0;
            EigWsLane yl{y};
            eig9_replay_row_rev<8>(log.data(), 1, nrot, nrot, r, yl, &e);
            double V[81];
            EigWsLane vl{V};
            eig9_replay(vl, log.data(), 1, nrot);
            for (int k = 0; k < 9; ++k) dev[q] = std::max(dev[q], std::fabs(y[k] - V[9 * r + k]));
            err[q] = e;
            HModelF mr;
            const double (&yr)[9] = y;
            decided[q] = h_model_f_cert(yr, errHuge ? e * 0x1p40 : e, nm, &mr) ? 1 : 0;
            if (decided[q])
                for (int k = 0; k < 8; ++k) modelsRow8[8 * q + k] = mr.h[k];
        }
        return 1;
    })
}

// Test hook (declared in minicv_native.h): the prefilter's three-way verdict for every (model, cell) of the table
// that mcvTestHCellBound builds from the same arguments, device kernel or host twin.
extern "C" MCV_API int mcvTestHCellPreVerdicts(const float* pts4, int N, const float* cand8, const float* models8,
                                               int nModels, float thr2, int B, int G, int Gs, int device, int* cellId,
                                               float* boxes, int* sizes, unsigned char* verdicts) {
    MCV_GUARD(0, {
        if (!pts4 || !cand8 || !models8 || !cellId || !boxes || !sizes || !verdicts)
            fail("mcvTestHCellPreVerdicts: null argument");
        if (N <= 0 || nModels <= 0 || G < 1 || G > kHCellMaxG || Gs < 1 || Gs > kHCellMaxGs)
            fail("mcvTestHCellPreVerdicts: bad sizes");
        const int cells = h_cell_count(G, Gs), words = (cells + 31) / 32;
        if (!device) {
            std::vector<int> ub(nModels);
            std::vector<uint32_t> bits((size_t)nModels * words);
            h_cell_host(pts4, N, cand8, models8, nModels, thr2, B, G, Gs, cellId, boxes, sizes, ub.data(), bits.data(),
                        nullptr, false, nullptr, verdicts);
            return 1;
        }
        require_device();
        DevBuf<float> p, m, cand;
        DevBuf<double> bb;
        DevBuf<int> ctl, tab, did, pre;
        DevBuf<uint8_t> dv;
        p.ensure((size_t)N * 4);
        m.ensure((size_t)nModels * 8);
        cand.ensure(8);
        bb.ensure(4);
        ctl.ensure(kHStageCtlInts);
        tab.ensure((size_t)cells * kHCellInts);
        did.ensure(N);
        dv.ensure((size_t)nModels * cells);
        MCV_HIP(hipMemcpy(p.p, pts4, (size_t)N * 16, hipMemcpyHostToDevice));
        MCV_HIP(hipMemcpy(m.p, models8, (size_t)nModels * 32, hipMemcpyHostToDevice));
        MCV_HIP(hipMemcpy(cand.p, cand8, 32, hipMemcpyHostToDevice));
        int hctl[kHStageCtlInts] = {0};
        const uint64_t key = (1ull << 32) | 0xFFFFFFFFull;   // slot 0 of `cand` is the candidate
        memcpy(hctl + kCtlKey, &key, sizeof(key));
        MCV_HIP(hipMemcpy(ctl.p, hctl, sizeof(hctl), hipMemcpyHostToDevice));
        launch_abs_bound4(p.p, false, N, bb.p, nullptr, 0);
        launch_h_stage_count(p.p, N, cand.p, 0, thr2, ctl.p, bb.p, tab.p, G, Gs, did.p, 0);
        pre.ensure(h_cell_rec_ints(cells));
        launch_h_cell_pre(tab.p, G, Gs, thr2, pre.p, 0);
        launch_h_cell_pre_verdicts(m.p, nModels, thr2, bb.p, tab.p, pre.p, G, Gs, dv.p, 0);
        MCV_HIP(hipGetLastError());
        MCV_HIP(hipDeviceSynchronize());
        std::vector<int> htab((size_t)cells * kHCellInts);
        MCV_HIP(hipMemcpy(htab.data(), tab.p, htab.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int c = 0; c < cells; ++c) {
            for (int j = 0; j < 8; ++j) boxes[8 * c + j] = h_cell_dec(htab[(size_t)c * kHCellInts + j]);
            sizes[c] = htab[(size_t)c * kHCellInts + kHCellInts - 1];
        }
        MCV_HIP(hipMemcpy(cellId, did.p, (size_t)N * sizeof(int), hipMemcpyDeviceToHost));
        MCV_HIP(hipMemcpy(verdicts, dv.p, (size_t)nModels * cells, hipMemcpyDeviceToHost));
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
