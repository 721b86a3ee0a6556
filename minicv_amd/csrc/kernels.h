// kernels.h — host-side launchers of the gfx950 kernels (definitions in *.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "epnp.h"
#include "ransac_batch_index.h"

namespace mcv {

// Hypotheses per wave in the inlier sweep (models live in SGPRs: 8 per hypothesis).
static const int kVerifyHypPerWave = 6;
// Correspondences per lane per trip of the sweep (independent loads in flight).
static const int kVerifyPtsPerLane = 2;
// Upper bound of reduction partial blocks (reduce.h).
static const int kReduceMaxBlocksHost = 1024;

// ---- homography (ransac_h_gen.hip, ransac_h_sweep.hip, ransac_h_mfma.hip, ransac_h_stage.hip,
// ransac_h_refine.hip; the host side: ransac_h_host.cpp)
struct HOneOut {
    double H[9];
    float hf[8];
    int status;
    int idx[4];
};
void launch_h_one(const float* d_pts4, int N, Sampler smp, int64_t hyp, HOneOut* d_out, hipStream_t s, bool fast);
void launch_h_mask_one(const float* d_pts4, int N, const HOneOut* d_one, float thr2, bool fused, uint8_t* d_mask,
                       int* d_count, hipStream_t s);
// d_scratch (h_gen_scratch_bytes(hypCount) bytes): the split eigen generate's rotation log, samples
// and overflow list (ransac_h_gen.hip); nullptr runs the one-pass solve.
void launch_h_generate(const float* d_pts4, int N, Sampler smp, int64_t hypBegin, int hypCount, void* d_models,
                       double* d_h64, int* d_counts, hipStream_t s, bool fast, void* d_scratch = nullptr,
                       bool certifiedRow = false);
size_t h_gen_scratch_bytes(int hypCount);
// certifiedRow (split generate only): pass 2 as the certified one-row replay (mcv_h_gen_r) with the exact
// pass 2 on the lanes it leaves undecided. Same fp32 models and statuses, bit for bit; d_h64 is written only
// for the undecided and the overflow lanes. While the scratch still holds the call's log (a call of one piece:
// h_gen_row_log_kept, and no generate since), launch_h_gen_v_one replays hypothesis `local` of the call
// exactly: its fp32 model and d_h64[9 local ..] as the switch-off generate writes them.
bool h_gen_row_log_kept(int hypCount);
void launch_h_gen_v_one(const float* d_pts4, int hypCount, int local, void* d_scratch, void* d_models, double* d_h64,
                        hipStream_t s);
const int* h_gen_row_stats(const void* d_scratch, int hypCount);   // device: {decided, undecided} lanes of the call
void h_gen_row_err_scale(bool huge);   // mcvTestHGenRow: err times 2^40 (no lane decided)
void launch_h_verify(const float* d_pts4, int N, const void* d_models, int* d_counts, int hypCount, float thr2,
                     bool fused, const float* d_bbox, hipStream_t s);
void launch_bbox(const float* d_pts4, int N, float* d_bbox, hipStream_t s);
// Packed-f32 sweep of the fused error over the paired layout (ransac_h_sweep.hip, HPair: 32 B per 2).
void launch_h_pair(const float* d_pts4, int N, void* d_pairs, hipStream_t s);
void launch_h_verify_packed(const float* d_pts4, const void* d_pairs, int N, const void* d_models, int* d_counts,
                            int hypCount, float thr2, const float* d_bbox, hipStream_t s);
// Certified division-free sweep of the op-by-op error (the default) + exact recount of its redo slots;
// d_bb = launch_abs_bound4 of the float4 points.
// d_rec / d_stats given: the bf16 matrix-core form (mcv_h_verify_mfma) runs where `form` says so.
// form (kHForm*): Auto = the size rule h_mfma_engages, Valu = mcv_h_verify_cert everywhere, Mfma = the
// matrix-core kernel everywhere, Mixed = matrix-core for the full-width launches, VALU for survivor stages.
enum { kHFormAuto = 0, kHFormValu = 1, kHFormMfma = 2, kHFormMixed = 3 };
static const int kHMfmaStats = 3;   // d_stats: undecided rows logged, waves overflowed, waves outside the domain
void launch_h_verify_certified(const float* d_pts4, const void* d_pairs, int N, const void* d_models, int* d_counts,
                               int hypCount, float thr2, const double* d_bb, hipStream_t s,
                               const void* d_rec = nullptr, unsigned long long* d_stats = nullptr,
                               int form = kHFormValu);
// The matrix-core form's point records (h_rec_bytes(N) bytes): per correspondence, padded to a multiple
// of 32, the bf16 pieces of x and y as the MFMA's B fragment words (16 B) and x', y' as f32 (8 B).
size_t h_rec_bytes(int N);
void launch_h_rec(const float* d_pts4, int N, void* d_rec, hipStream_t s);
bool h_mfma_engages(int N, int hypCount, int form, bool staged);
// W, U, V of the matrix-core form for every (model, correspondence): d_wuv[(k * N + i) * 3 + {0, 1, 2}]
void launch_h_mfma_wuv(const void* d_rec, int N, const void* d_models, int nModels, float* d_wuv, hipStream_t s);
// mcvTestHMfma's setting and the stats of a sweep run outside a plan (mcvTestHomographySweep)
int h_mfma_form();
void h_mfma_set_last(const unsigned long long* stats3);
// The certified sweep in self-pruning stages, for callers that consume only the best key (the counts
// of pruned slots stay partial). d_ctl: kHStageCtlInts ints (layout in h_cert.h, read back by
// mcvTestHStaging); d_list: 2 x hypCount ints; d_pkey / d_pfail: launch_best's partials.
static const int kHStageCtlInts = 32;
static const int kCtlB = 0;        // the candidate's full count: a lower bound of the winning count
static const int kCtlReason = 1;   // 0 = pruning engaged, else kHStage* (why everything runs to the end)
static const int kCtlStages = 2;   // stages in use (2 + the later stages)
static const int kCtlCells = 3;    // cell slots of the per-cell bound that ran before stage 1 (0: none)
static const int kCtlBound = 4;    // kHStageMax + 1 boundaries, in pairs
static const int kCtlAlive = 12;   // slots alive entering each stage
static const int kCtlPre = 18;     // slots the per-cell bound's box pass hands to the second pass
static const int kCtlKey = 24;     // the candidate's packed key and the first failure (2 x 64 bit)
static const int kCtlFailAll = 30; // stage 0 on a subset: the chunk's first failure from a pass over every status
                                   // (64 bit; the key that pass packs lands in the two ints before it, unread)
static const int kHStageMax = 6;          // stages: the prefix, the run to the first boundary, <= 4 later ones
static const int kHStagePrefixDiv = 16;   // stage 0 sweeps ~N / 16 points
static const int kHStageSlackDiv = 64;    // first boundary at N - B + N / 64 points
static const int kHStageLater = 2;        // stages after the first boundary
static const int kHStageLatest256 = 192;  // latest first boundary that still prunes: 192 / 256 of the pairs
// the automatic rule: calls with fewer (hypothesis, correspondence) evaluations or fewer
// correspondences than these run unstaged (below them the extra launches cost more
// than the pruning saves)
static const int64_t kHStageMinEvals = (int64_t)1 << 31;
static const int kHStageMinN = 4096;
// why a staged evaluation pruned nothing (control block / mcvTestHStaging stats[0]; 0 = it pruned)
enum { kHStageNoCandidate = 1, kHStageSamplerFailure = 2, kHStageLate = 3, kHStageForcedOff = 4,
       kHStageNotApplicable = 5 };
// Where the per-cell bound's second pass runs, one more boundary halves stage 1's range (the half boundary,
// DESIGN.md §7): stage 1 then runs its list in two launches, and the slots that cannot reach B any more at the
// middle skip the second. Only there: without the per-slot `left` the test at a boundary before the first
// pruning boundary can drop nothing (count + N - processed >= B by that boundary's construction).
// kHStageCellLater: the boundaries behind a list stage there, each with a `left` row.
static const int kHStageCellLater = kHStageLater + 1;
// the per-cell bound's other buffers (with d_cells): cell ids (N ints), prefix table (kHStageCellLater x cells
// ints), per-slot points left in uncertified cells (kHStageCellLater x hypCount ints)
struct HCellBufs {
    int *id, *pref, *left;
};
static const int kHCellLater = kHStageMax - 2;   // the most later boundaries a slot keeps a `left` figure for
static_assert(kHStageCellLater <= kHCellLater && 2 + kHStageCellLater <= kHStageMax, "control block layout");

// The stage boundaries (in pairs) from the candidate's full count B: the arithmetic of mcv_h_stage_plan, which
// the kernel runs on the device and h_stage_plan_host (mcvHostHStagePlan) on the host. The first pruning boundary p1 is the first
// point count at which a slot can fall below the bound (N - B) plus the slack, rounded up to a trip and not
// before the prefix pa; the later stages split the rest evenly. Pruning switches itself off (reason != 0: p1 and
// every later boundary are nPairs, so the stage behind boundary 1 runs every slot to the end and the others are
// empty) without a candidate, with a sampler failure in the chunk and when p1 lies beyond latest/256 of the pairs.
// subset: stage 1 starts at point 0 (boundary 1 is 0), since the counts buffer holds no stage-0 partials.
// half: one more boundary in the middle of stage 1's range [boundary 1, p1), rounded down to a trip so that
// every stage still starts trip-aligned; with one trip or none in the range it collapses onto the range's start
// and the first half is empty. Boundaries are non-decreasing; all but the last are multiples of trip.
struct HStagePlan {
    int reason, stages;
    int bound[kHStageMax + 1];
};
__host__ __device__ inline HStagePlan h_stage_plan(int N, int trip, int later, int slackPts, int latest256,
                                                   bool subset, bool half, bool candidate, bool failure, int B,
                                                   int pa) {
    HStagePlan pl;
    const int nPairs = (N + 1) / 2;
    pl.reason = 0;
    int p1 = nPairs;
    if (!candidate) pl.reason = kHStageNoCandidate;
    else if (failure) pl.reason = kHStageSamplerFailure;
    else {
        const int64_t pts = (int64_t)N - B + slackPts;
        const int64_t pr = ((pts + 1) / 2 + trip - 1) / trip * trip;
        p1 = pr < pa ? pa : (pr > nPairs ? nPairs : (int)pr);
        if ((int64_t)p1 * 256 > (int64_t)nPairs * latest256) pl.reason = kHStageLate;
    }
    if (pl.reason) p1 = nPairs;
    int n = 0;
    pl.bound[n++] = 0;
    const int start = subset ? 0 : pa;
    pl.bound[n++] = start;
    if (half) pl.bound[n++] = pl.reason ? nPairs : start + (p1 - start) / trip / 2 * trip;
    pl.bound[n++] = p1;
    const int trips = (nPairs - p1) / trip;   // whole trips left after the first pruning boundary
    for (int s = 1; s <= later; ++s)
        pl.bound[n++] = s == later ? nPairs : p1 + (int)((int64_t)trips * s / later) * trip;
    pl.stages = n - 1;
    for (; n <= kHStageMax; ++n) pl.bound[n] = 0;
    return pl;
}
// The plan of a staged evaluate of N correspondences on the host, with the constants launch_h_verify_staged
// gives the planner kernel (ransac_h_stage.hip holds both). cellBound: the per-cell bound runs (a shorter stage 0);
// half: its second pass runs too (the half boundary); subset: stage 0 swept a leading subset. pa: stage 0's pairs.
HStagePlan h_stage_plan_host(int N, bool candidate, bool failure, int B, bool cellBound, bool half, bool subset,
                             int* pa);
// what the two bound passes read beside the cell table: the record list of the non-empty cells (h_cell_pre.h:
// h_cell_rec_ints(cells) ints, written by launch_h_cell_pre; always needed), the switch of the box test's fp32
// prefilter (0: fp64 runs alone) and two counters, the (model, cell) tests of the passes and the undecided of
// them (nullptr: not counted)
struct HCellPreBufs {
    int* rec;
    int on;
    unsigned long long* stats;
};
void launch_h_verify_staged(const float* d_pts4, const void* d_pairs, int N, const void* d_models, int* d_counts,
                            int hypCount, int64_t hypBegin, float thr2, const double* d_bb, int* d_ctl, int* d_list,
                            uint64_t* d_pkey, int64_t* d_pfail, hipStream_t s, const void* d_rec = nullptr,
                            unsigned long long* d_stats = nullptr, int form = kHFormValu, int* d_cells = nullptr,
                            int G = 0, int Gs = 0, HCellBufs d_cell = HCellBufs{nullptr, nullptr, nullptr},
                            HCellPreBufs d_pre = HCellPreBufs{nullptr, 0, nullptr}, int* d_s0 = nullptr,
                            int s0Slots = 0);
// Stage 0 on a leading subset of the slots (with the per-cell bound only): stage 0 exists to name a candidate, and
// the first slots name as good a one as all of them. It sweeps the prefix for the first S slots into
// d_s0 (S ints), launch_best over d_s0 names the candidate, and stage 1 runs its list from point 0. The rule:
// S = max(kHStage0MinSlots, hypCount / kHStage0Div) from kHStage0MinHyps hypotheses; mcvTestHStage0Slots forces S.
static const int kHStage0MinHyps = 1 << 18, kHStage0MinSlots = 1 << 14, kHStage0Div = 16;
// The per-cell bound before stage 1 (h_cell_bound.h): the cell table (h_cell_count(G, Gs) x
// kHCellInts ints) is built with the candidate's count, the bound kernel writes the slots that can still
// reach B to d_list and their number to ctl[kCtlAlive + 1]. The automatic rule engages it where the staged
// sweep's own size rule holds and N >= kHCellMinN: the bound costs a slot about what 2200 correspondences of
// the sweep cost, whatever N, and measured it wins at N = 20000 and 100000 from 2^16 / 2^18
// hypotheses and loses at N = 5000 (2^20 hypotheses: 5.96 -> 6.17 ms).
// A second pass over that list (mcv_h_cell_rel) adds the candidate-relative test on the cells of the
// candidate's inliers and writes each kept slot's `left` per later boundary: with d_listPre the first pass
// writes there (length in ctl[kCtlPre]) the slots the relative test can still drop and to d_list the others
// (their `left` in d_left: the points not yet processed), and the second pass appends to d_list.
// d_cellOut / d_ub / d_bits: the test hooks' outputs (nullptr in the sweep, but for the cell ids the prefix
// table is built from).
static const int kHCellMinN = 20000;
// the second pass (candidate-relative test, per-slot `left`) from this many correspondences: it costs a slot
// it visits about what 7000 correspondences of the sweep cost, whatever N, and what it saves grows with N.
// Measured at 2^20 hypotheses: N = 20000 level at 50 % outliers and 1-2 % slower at 70 %;
// N = 35000, 50000, 70000, 100000 faster at 50 % and level at 70 %.
static const int kHCellRelMinN = 35000;
// stage 0 with the bound sweeps ~N / 64 points: every slot still runs stage 0, so with stage 1 listed it is the
// largest full-width cost; cfg3 evaluate 13.00 ms at N / 16, 12.32-12.41 at N / 32, 11.94-12.01 at N / 64 (the
// candidate's B is 50196 at all three)
static const int kHCellPrefixDiv = 64;
void launch_h_stage_count(const float* d_pts4, int N, const void* d_models, int64_t hypBegin, float thr2, int* d_ctl,
                          const double* d_bb, int* d_cells, int G, int Gs, int* d_cellOut, hipStream_t s);
void launch_h_cell_bound(const void* d_models, const int* d_counts, int hypCount, float thr2, const double* d_bb,
                         const int* d_cells, int G, int Gs, int* d_ctl, int* d_list, int* d_ub, uint32_t* d_bits,
                         hipStream_t s, int* d_listPre, int* d_left, int nLater, int N, HCellPreBufs pre);
void launch_h_cell_pre(const int* d_cells, int G, int Gs, float thr2, int* d_rec, hipStream_t s);
// One compaction of the staged sweep: the survivors entering `stage` (>= 2) go from d_src (nullptr: every slot) to
// d_dst, their number to ctl[kCtlAlive + stage]; d_left: the per-slot `left` rows (nullptr: N - processed).
void launch_h_stage_compact(const int* d_counts, int hypCount, int N, int* d_ctl, int stage, const int* d_src,
                            int* d_dst, const int* d_left, hipStream_t s);
// the prefilter's verdict (h_cell_pre.h kHCellPre*) per (model, cell): nModels x cells bytes
void launch_h_cell_pre_verdicts(const void* d_models, int nModels, float thr2, const double* d_bb, const int* d_cells,
                                const int* d_rec, int G, int Gs, uint8_t* d_out, hipStream_t s);
void launch_h_cell_prefix(const int* d_cellId, int N, const int* d_ctl, int nLater, int G, int Gs, int* d_pref,
                          hipStream_t s);
void launch_h_cell_rel(const void* d_models, const void* d_candModels, int64_t hypBegin, int hypCount, float thr2,
                       const double* d_bb, const int* d_cells, int G, int Gs, const int* d_pref, int nLater,
                       int* d_ctl, const int* d_src, int* d_list, int* d_left, int* d_ub, uint32_t* d_bits,
                       hipStream_t s, HCellPreBufs pre);
void h_cell_rel_host(const float* pts4, int N, const float* cand8, const float* models8, int nModels, float thr2,
                     int B, int G, int Gs, const int* bounds, int nBounds, int* cellId, int* ub, uint32_t* bits,
                     int* left, int* alive, bool pre = false, long long* stats = nullptr);
void h_cell_host(const float* pts4, int N, const float* cand8, const float* models8, int nModels, float thr2, int B,
                 int G, int Gs, int* cellId, float* boxes, int* sizes, int* ub, uint32_t* bits, int* alive,
                 bool pre = false, long long* stats = nullptr, uint8_t* verdicts = nullptr);
void h_reduce_sums(const float* d_pts4, int N, const uint8_t* d_mask, double* d_part, double* d_out, hipStream_t s);
// The refit record: what HomographyEstimatorCallback::runKernel's three passes, chained on the device, leave
// per problem (h_refit_chain: one record; launch_batch_refit_chain: one per problem) and what the host half
// (h_refit_from_record, plan.h) reads.
static const int kRefitSums = 0;     // 5: sum dst.x, dst.y, src.x, src.y, count
static const int kRefitCount = 4;    //    the count among them
static const int kRefitC4 = 5;       // 4: centroids cm.x, cm.y, cM.x, cM.y = sums / count
static const int kRefitDev = 9;      // 4: sum |dst - cm|, |src - cM|
static const int kRefitS4 = 13;      // 4: scales sm.x, sm.y, sM.x, sM.y = count / deviation sums
static const int kRefitLtL = 17;     // 45: upper triangle of LtL, row-major
static const int kRefitDoubles = 62;
void h_refit_chain(const float* d_pts4, int N, const uint8_t* d_mask, double* d_part, double* d_red, hipStream_t s);
// d_out = {JtJ upper triangle (36), Jtr (8), |r|^2} of HomographyRefineCallback at h8
void h_reduce_lm(const float* d_pts4, int N, const uint8_t* d_mask, const double* h8, double* d_part, double* d_out,
                 hipStream_t s);

// ---- affine / similarity (ransac_a.hip); m = 3 (affine) or 2 (similarity) point samples, lx = 6 / 4
// refine parameters; both store AModelF (6 floats) per hypothesis
static const int kVerifyAHypPerWave = 8;     // hypotheses per wave of the packed sweep
static const int kVerifyAPairsPerLane = 2;   // HPair loads per lane per trip
struct AOneOut {
    double A[6];
    float af[6];
    int status;
    int idx[3];
};
void launch_a_generate(int m, const float* d_pts4, int N, Sampler smp, int64_t hypBegin, int hypCount, void* d_models,
                       double* d_a64, int* d_counts, hipStream_t s);
// direct: the first m correspondences as they are (the N == m call), no sampler, no subset check
void launch_a_one(int m, const float* d_pts4, int N, Sampler smp, int64_t hyp, AOneOut* d_out, hipStream_t s,
                  bool direct = false);
// d_pairs = launch_h_pair of the float4 points. The counts are final (nothing divides: no recount).
void launch_a_verify(const void* d_pairs, int N, const void* d_models, int* d_counts, int hypCount, float thr2,
                     bool fused, hipStream_t s);
void launch_a_mask_one(const float* d_pts4, int N, const AOneOut* d_one, float thr2, bool fused, uint8_t* d_mask,
                       int* d_count, hipStream_t s);
// d_out = {JtJ upper triangle, Jtr, |r|^2} of the refine callback at h[lx]: 28 (lx 6) or 15 (lx 4) sums
void a_reduce_lm(int lx, const float* d_pts4, int N, const uint8_t* d_mask, const double* h, double* d_part,
                 double* d_out, hipStream_t s);

// ---- fundamental (ransac_f.hip)
static const int kVerifyFHypPerWave = 4;
static const int kVerifyFPtsPerLane = 2;
struct FOneOut {
    double F[9];
    int status;
    int idx[8];
};
void launch_f_generate(const float* d_pts4, int N, Sampler smp, int64_t hypBegin, int hypCount, void* d_models,
                       int* d_counts, hipStream_t s, bool fast);
void launch_f_one(const float* d_pts4, int N, Sampler smp, int64_t hyp, FOneOut* d_out, hipStream_t s, bool fast);
// 7-point (MCV_FLAG_SEVEN_POINT): 3 model slots per hypothesis (models[3h + s], counts[3h + s]).
void launch_f7_generate(const float* d_pts4, int N, Sampler smp, int64_t hypBegin, int hypCount, void* d_models,
                        int* d_counts, hipStream_t s);
void launch_f7_one(const float* d_pts4, int N, Sampler smp, int64_t slot, FOneOut* d_out, hipStream_t s);
void launch_f7_direct(const float* d_pts4, FOneOut* d_out, hipStream_t s);   // N == 7: run7Point, first model
void launch_f_verify(const float* d_pts4, int N, const void* d_models, int* d_counts, int hypCount, float thr2,
                     int kind, hipStream_t s, const double* d_bb = nullptr);
// max |x1|, |y1|, |x2|, |y2| of float4 (fp64 = false) or double4 points -> d_bb[4] (fp64); with
// d_out32 (double4 input) also the float4-rounded copy of the points.
void launch_abs_bound4(const void* d_pts4, bool fp64, int N, double* d_bb, float* d_out32, hipStream_t s);
void launch_f_mask(const float* d_pts4, int N, const double* F9, float thr2, int kind, uint8_t* d_mask, int* d_count,
                   hipStream_t s);
// c4 = {c2x, c2y, c1x, c1y}; d_out = {sum |p2 - c2|, sum |p1 - c1|} (Euclidean).
void f_reduce_eucdev(const float* d_pts4, int N, const uint8_t* d_mask, const double* c4, double* d_part,
                     double* d_out, hipStream_t s);
void f_reduce_ata(const float* d_pts4, int N, const uint8_t* d_mask, const double* c4, const double* s4,
                  double* d_part, double* d_out, hipStream_t s);

// ---- essential (ransac_e.hip)
static const int kVerifyEModelsPerWave = 4;
static const int kEGenLanes = 16;   // lanes per hypothesis of mcv_e_generate_wave (five_point_wave.h)
static const int kVerifyEPtsPerLane = 2;   // correspondences per lane per trip (variant screen)
static const int kEModelSlots = 10;
struct EOneOut {
    double E[10][9];
    int status;    // model count (0 = no model) or -2 (no sample)
    int idx[5];
};
struct EFiveIn { double x1[5], y1[5], x2[5], y2[5]; };
// Five-point solve split at the root finder (mcv_e_stage -> mcv_e_roots): the null basis, B(z) and
// det B(z) of one hypothesis; status 1 = solved up to the roots, 0 = degenerate, -2 = no sample.
struct EStage {
    double nb[4][9];
    double bx[3][4], by[3][4], bc[3][5];
    double det[11];
    int status, pad;
};
static const int kEStageMinHyps = 32768;   // hypCount from which generate takes the split path
static const int kEStageLanes = 16;        // lanes per hypothesis of its matrix phases
static const int kERootLanes = 4;          // lanes per hypothesis of its root finder (1: one lane)
void launch_e_pack(const double* d_ab, int N, double f, double cx, double cy, double* d_pts4, hipStream_t s);
void launch_e_generate(const double* d_pts4, int N, Sampler smp, int64_t hypBegin, int hypCount, void* d_dense,
                       int* d_denseSlot, int* d_nDense, int* d_counts, void* d_stage, hipStream_t s);
void launch_e_verify(const double* d_pts4, int N, const void* d_dense, const int* d_denseSlot, const int* d_nDense,
                     int maxModels, int* d_counts, float thr2, int kind, hipStream_t s, const float* d_pts32 = nullptr,
                     const double* d_bb = nullptr);
// The reference's five-point solver (five_point_ref.h) over a chunk: the default RANSAC generate.
size_t e5_stage_bytes(int hypCount);
void launch_e5_generate(const double* d_pts4, int N, Sampler smp, int64_t hypBegin, int hypCount, void* d_dense,
                        int* d_denseSlot, int* d_nDense, int* d_counts, void* d_stage, hipStream_t s);
void launch_e5_one(const double* d_pts4, int N, Sampler smp, int64_t hyp, EOneOut* d_out, hipStream_t s);
void launch_e_fetch(const void* d_dense, const int* d_denseSlot, const int* d_nDense, int maxModels, int slot,
                    void* d_out, int* d_found, hipStream_t s);
void launch_e_one(const double* d_pts4, int N, Sampler smp, int64_t hyp, EOneOut* d_out, hipStream_t s);
void launch_e_mask(const double* d_pts4, int N, const double* E9, float thr2, int kind, uint8_t* d_mask, int* d_count,
                   hipStream_t s);
void launch_e_cheirality(const double* d_pts4, int N, const uint8_t* d_mask, const double* P4x12, double dist,
                         int* d_good4, hipStream_t s);
void launch_e_fivepoint(const EFiveIn& in, EOneOut* d_out, hipStream_t s);

// ---- PnP (ransac_pnp.hip); cam8 = {fx, fy, cx, cy, k1, k2, p1, p2}
static const int kVerifyPnpPosesPerWave = 3;
struct PnpOneOut {
    double R[9];
    double t[3];
    int status;
    int idx[5];
};
struct Ap3pIn { double mu[3], mv[3], W[3][3], inv_fx, inv_fy, cx_fx, cy_fy; };
struct Ap3pOut {
    double R[4][9];
    double t[4][3];
    int count;
    int cplx;   // the quartic took the complex-pow branch (glibc's clog / exp / cos / atan2, restated)
};
void launch_pnp_pack(const double* d_img, const double* d_world, int N, void* d_pts, hipStream_t s);
// fast (MCV_FLAG_FAST_MINIMAL): the AP3P kernel's real-root-finder quartic instead of the reference's Ferrari
// d_epnpScratch: kEpnpSplitDoubles x min(hypCount, kEpnpPiece) doubles (EPnP's split generate runs over
// sub-ranges of kEpnpPiece hypotheses; unused by AP3P). Round 6: 2^20 (2.4 GB at 2^20 hypotheses): one
// piece per chunk, 27.3-27.5 ms a PnP step against 27.9-28.2 ms with 2^18 pieces (610 MB; each of the
// five kernels per piece drains its slowest waves) and 27.7-27.9 with 2^19, same box alternating.
static const int kEpnpPiece = 1 << 20;
void launch_pnp_generate(const void* d_pts, int N, const double* cam8, Sampler smp, int64_t hypBegin, int hypCount,
                         bool epnp, void* d_models, int* d_counts, double* d_epnpScratch, hipStream_t s,
                         bool fast = false);
// d_ext: 3 doubles of device scratch filled by launch_pnp_extent (the certified sweep's bound);
// d_pairs: kPnpPairFloatsPerPoint x N floats it fills with the sweep's pair layout.
static const int kPnpPairFloatsPerPoint = 6;
void launch_pnp_extent(const void* d_pts, int N, double* d_ext, float* d_pairs, hipStream_t s);
void launch_pnp_verify(const void* d_pts, int N, const double* cam8, const void* d_models, int* d_counts, int hypCount,
                       float thr2, bool fused, const double* d_ext, const float* d_pairs, hipStream_t s);
void launch_pnp_one(const void* d_pts, int N, const double* cam8, Sampler smp, int64_t hyp, bool epnp,
                    PnpOneOut* d_out, hipStream_t s, bool fast = false);
void launch_pnp_solve5(const void* d_pts, const double* cam8, PnpOneOut* d_out, hipStream_t s);
void launch_mask_compact(const uint8_t* d_mask, int N, int* d_idx, int* d_count, hipStream_t s);
// EPnP over n points: d_pts (+ optional index list d_idx) fp32 PnpPoints, or d_img / d_world fp64.
// normalized: d_us = undistortPoints' normalised coordinates (SQPnP) instead of x f + c (EPnP).
// d_n (optional, fp32 points only): the point count on the device (a compaction's output); n is then
// an upper bound that sizes the grid.
void launch_epnp_prep(const void* d_pts, const int* d_idx, const double* d_img, const double* d_world, int n,
                      const double* cam8, double* d_pw, double* d_us, hipStream_t s, bool normalized = false,
                      const int* d_n = nullptr);
// SQPnP passes (sqpnp.h): the 39 computeOmega sums; the positive-depth count of the pose R[0] / t[0].
enum { kEpnpPassSumPw = 0, kEpnpPassPw0 = 1, kEpnpPassMtm = 2, kEpnpPassPc = 3, kEpnpPassAbt = 4, kEpnpPassReproj = 5,
       kEpnpPassSqp = 6, kEpnpPassSqpDepth = 7 };
struct EpnpPassArgs {
    EpnpCtrl C;
    EpnpCam cam;
    double c0[3];            // Pw0: centroid
    double ccs[3][4][3];     // Pc / Abt: sign-fixed control points of N = 1, 2, 3
    double pc0[3][3];        // Abt
    double pw0[3];           // Abt
    double R[3][3][3];       // Reproj
    double t[3][3];
};
// d_n (optional): the point count on the device, n an upper bound; the partials keep the stride of the
// device count's blocks (part[acc * nblk + blk], nblk = ceil(*d_n / kEpnpBlock)). d_prev (optional, Pw0 /
// Abt): the previous pass's partials, from which the pass takes its centroid / pc0 on the device.
void launch_epnp_pass(int mode, const double* d_pw, const double* d_us, int n, const EpnpPassArgs& a, int nacc,
                      double* d_part, hipStream_t s, const int* d_n = nullptr, const double* d_prev = nullptr);
void launch_pnp_solve4(const void* d_pts, const double* cam8, PnpOneOut* d_out, hipStream_t s, bool fast = false);
void launch_pnp_mask(const void* d_pts, int N, const double* cam8, const double* R9, const double* t3, float thr2,
                     bool fused, uint8_t* d_mask, int* d_count, hipStream_t s);
// The same mask for a pose already on the device (a chunk's model slot): no host round trip first.
void launch_pnp_mask_dev(const void* d_pts, int N, const double* cam8, const void* d_pose, float thr2, bool fused,
                         uint8_t* d_mask, int* d_count, hipStream_t s);
void launch_pnp_ap3p(const Ap3pIn& in, Ap3pOut* d_out, hipStream_t s);
void pnp_reduce_lm(const void* d_pts, int N, const uint8_t* d_mask, const double* cam8, const double* R9,
                   const double* t3, const double* dR27, bool wantJ, double* d_part, double* d_out, hipStream_t s);
void pnp_reduce_vvs(const void* d_pts, int N, const uint8_t* d_mask, const double* cam8, const double* R9,
                    const double* t3, double* d_part, double* d_out, hipStream_t s);

// ---- LMedS (lmeds.hip): d_keys[slot] = the order key (rank_select.h) of the rank-`rank` error (0-based,
// ascending) of slot's model over the N correspondences; model = MCV_MODEL_HOMOGRAPHY (HModelF slots,
// errKind = fused 0 / 1), MCV_MODEL_FUNDAMENTAL (FModelD slots, errKind = f_error's kinds) or
// MCV_MODEL_AFFINE / MCV_MODEL_SIMILARITY (AModelF slots, errKind = fused 0 / 1). d_status
// (may be NULL: every slot has a model): slots with a negative status get the NaN class.
void launch_error_rank(int model, const float* d_pts4, int N, const void* d_models, const int* d_status, int nSlots,
                       int errKind, int rank, uint32_t* d_keys, hipStream_t s);

// ---- batched 2-D model RANSAC (ransac_batch.hip): B problems of one family per launch. All problems'
// float4 points sit in one segmented buffer; the tables below name each problem's share of it.
static const int kBatchTile = 1024;          // points staged in LDS per trip of the batched sweep (16 KiB)
// BatchDesc, one problem of a hypothesis round: ransac_batch_index.h
struct BatchFin {       // one problem with a winner
    int ptOff, N;
    int64_t rowOff;
    int64_t hyp;             // the winning hypothesis
};
struct BatchOne {       // the winner in full
    double M[9];             // fp64 model (affine family: 6 values)
    float f[8];              // the sweep's fp32 model (H: 8, affine family: 6; F sweeps M)
    int status, pad;
};
struct BatchRed { int ptOff, N; };   // one problem of a batched reduction
size_t batch_model_bytes(int model);
// maxHyp: the largest hypCount of the table (sizes the grid); d_table: the CV sample rows or nullptr
void launch_batch_generate(int model, const float* d_pts4, const BatchDesc* d_desc, int nDesc, int maxHyp,
                           uint64_t seed, const int* d_table, void* d_models, int* d_counts, hipStream_t s);
// errKind: f_error's kinds (F); 0 for the other families (op-by-op error)
void launch_batch_sweep(int model, int errKind, const float* d_pts4, const BatchDesc* d_desc, int nDesc, int maxHyp,
                        const void* d_models, int* d_counts, float thr2, hipStream_t s);
void launch_batch_one(int model, const float* d_pts4, const BatchFin* d_fin, int nFin, uint64_t seed,
                      const int* d_table, BatchOne* d_one, hipStream_t s);
// d_mask: the segmented mask (written only for winners with a model); d_count[f] += inliers (zeroed by the caller)
void launch_batch_mask(int model, int errKind, const float* d_pts4, const BatchFin* d_fin, int nFin, int maxN,
                       const BatchOne* d_one, float thr2, uint8_t* d_mask, int* d_count, hipStream_t s);
int batch_reduce_blocks(int maxN);   // partial rows per problem (x 45 doubles) of the reductions below
// LM sums of lx = 8 (H), 6 (affine), 4 (similarity) parameters: d_par 8 doubles per problem in,
// d_out 45 doubles per problem out (the single call's order). Both return the kernels launched.
int launch_batch_reduce_lm(int lx, const float* d_pts4, const uint8_t* d_mask, const BatchRed* d_red, int nRed,
                           int maxN, const double* d_par, double* d_part, double* d_out, hipStream_t s);
// h_refit_chain for every problem: d_rec = one refit record (kRefitDoubles) per problem
int launch_batch_refit_chain(const float* d_pts4, const uint8_t* d_mask, const BatchRed* d_red, int nRed, int maxN,
                             double* d_part, double* d_rec, hipStream_t s);

// ---- batched essential-matrix RANSAC (ransac_batch_e.hip; the generate: ransac_e5.hip). All problems'
// double4 normalised points sit in one segmented buffer. A hypothesis round gives problem j of the round
// `stride` columns of the flat five-point stage, 10 stride model slots / counts and a dense region of the
// same capacity at 10 j stride (BatchDesc.slotOff = j stride counts hypotheses).
static const int kBatchETile = 512;          // double4 points staged in LDS per trip of the sweep (16 KiB)
struct BatchEPack {     // one problem of the pack
    int ptOff, N;
    double focal, cx, cy;
};
struct BatchESweep {    // one problem of the sweep
    int ptOff, N;
    int64_t denseOff;        // its first model of the dense buffer
    int64_t countOff;        // its first count: model i's lands at countOff + denseSlot[denseOff + i]
    float thr2;
    int pad;
};
struct BatchEFetch {    // one model to copy out of a dense region
    int64_t denseOff;
    int prob;                // the region's counter: nDense[prob]
    int slot;                // the model's slot within the problem's round: hypothesis * 10 + k
    int outIdx;              // out[outIdx] = the model, found[outIdx] = stamp
    int stamp;
};
struct BatchEFin {      // one winner of the mask
    int ptOff, N;
    float thr2;
    int modelIdx;            // its model: models[modelIdx]
};
struct BatchEPose {     // one winner of the cheirality test: the four [R | t] candidates
    int ptOff, N;
    double P[4][12];
};
// The three kernels of launch_e5_generate over a round (returns the kernels launched); d_stage:
// e5_stage_bytes(nDesc * stride) bytes, d_nDense: nDesc counters.
int launch_e5_batch_generate(const double* d_pts4, const BatchDesc* d_desc, int nDesc, int stride, uint64_t seed,
                             const int* d_table, void* d_dense, int* d_denseSlot, int* d_nDense, int* d_counts,
                             void* d_stage, hipStream_t s);
void launch_batch_e_pack(const double* d_a, const double* d_b, const BatchEPack* d_desc, int nDesc, int maxN,
                         double* d_pts4, hipStream_t s);
// maxModels: the largest dense count possible (sizes the grid); d_denseSlot nullptr: model i counts at countOff + i
void launch_batch_e_sweep(int kind, const double* d_pts4, const BatchESweep* d_desc, int nDesc, int maxModels,
                          const void* d_dense, const int* d_denseSlot, const int* d_nDense, int* d_counts,
                          hipStream_t s);
void launch_batch_e_fetch(const BatchEFetch* d_fetch, int nFetch, const void* d_dense, const int* d_denseSlot,
                          const int* d_nDense, double* d_out9, int* d_found, hipStream_t s);
// d_mask: the segmented mask; d_count[f] += inliers (zeroed by the caller)
void launch_batch_e_mask(int kind, const double* d_pts4, const BatchEFin* d_fin, int nFin, int maxN,
                         const double* d_models9, uint8_t* d_mask, int* d_count, hipStream_t s);
// d_good4[4 f + k] += masked points of winner f passing candidate k's test (zeroed by the caller)
void launch_batch_e_cheirality(const double* d_pts4, const uint8_t* d_mask, const BatchEPose* d_pose, int nPose,
                               int maxN, double dist, int* d_good4, hipStream_t s);

// ---- batched PnP RANSAC (ransac_batch_pnp.hip: sweep, fetch, mask; the batch forms of the generate and of
// the refine passes: ransac_pnp.hip, beside the single forms they share their bodies with). All problems'
// PnpPoint rows sit in one segmented buffer; cams = 8 doubles (cam8) per device problem. A hypothesis round
// gives problem j of the round the slots [j stride, j stride + hypCount) of the pose / count buffers (and of
// the EPnP scratch's columns); the slots past hypCount carry kStatusNoSample and are never read back.
static const int kBatchPnpTile = 512;    // PnpPoint rows (32 B) staged in LDS per workgroup of the sweep (16 KiB)
static const int kBatchPnpWidth = 64;    // lanes = poses per workgroup of the sweep
struct BatchPnpDesc {   // one problem of a hypothesis round
    BatchDesc d;
    int cam, pad;            // its camera: cams + 8 cam
};
struct BatchPnpFetch {  // one pose to copy out of a round's buffer: best[out] = models[slot]
    int64_t slot;
    int out, pad;
};
struct BatchPnpFin {    // one winner of the mask: pose best[pose], camera cams + 8 cam
    int ptOff, N;
    int pose, cam;
};
struct BatchPnpLmJob {  // one job of a batched LM / VVS reduction (the constants of OpPnpLM; OpPnpVVS reads no dR)
    int ptOff, N;
    double cam[8], R[9], t[3], dR[27];
};
struct BatchPnpEpnpJob {   // one job of the batched inlier EPnP
    int ptOff, N;            // its slice of the mask / index / pw / us buffers
    int n, nblk;             // the inlier count once the host knows it (n < 0: read count[job]); ceil(N / kEpnpBlock)
    int64_t partOff;         // its partials: part + partOff, kMtmSums nblk doubles
    double cam[8];
    EpnpPassArgs A;
};
// The AP3P generate / the five EPnP stages over a round: stride slots per problem, table = the CV sample rows
// or nullptr. d_scratch: kEpnpSplitDoubles x (nDesc stride) doubles (EPnP). Returns the kernels launched.
int launch_pnp_batch_generate(const void* d_pts, const BatchPnpDesc* d_desc, int nDesc, int stride, const double* d_cams,
                              uint64_t seed, const int* d_table, bool epnp, void* d_models, int* d_counts,
                              double* d_scratch, hipStream_t s);
// counts[slot] += points of the slot's problem with pnp_error <= thr2 (slots with a negative status untouched)
void launch_batch_pnp_sweep(const void* d_pts, const BatchPnpDesc* d_desc, int nDesc, int maxHyp, int maxN,
                            const double* d_cams, const void* d_models, int* d_counts, float thr2, hipStream_t s);
void launch_batch_pnp_fetch(const BatchPnpFetch* d_fetch, int nFetch, const void* d_models, void* d_best, hipStream_t s);
// d_mask: the segmented mask; d_count[f] += inliers (zeroed by the caller)
void launch_batch_pnp_mask(const void* d_pts, const BatchPnpFin* d_fin, int nFin, int maxN, const double* d_cams,
                           const void* d_best, float thr2, uint8_t* d_mask, int* d_count, hipStream_t s);
// pnp_reduce_lm (wantJ), or with vvs pnp_reduce_vvs (the job's cam, R, t; dR unread), for every job:
// d_part = nJobs x reduce_blocks(maxN) x 28, d_out = nJobs x 28. d_mask: the segmented mask, or nullptr: every
// row of a job counts (the batched refinement's gathered rows). Returns 2.
int launch_pnp_batch_reduce(bool vvs, const void* d_pts, const uint8_t* d_mask, const BatchPnpLmJob* d_jobs,
                            int nJobs, int maxN, double* d_part, double* d_out, hipStream_t s);
// The gather of the batched refinement: mcv_mask_compact's job form over the B problems
// (d_jobs[p].ptOff / .N = problem p's rows; d_idx segmented like the mask, d_count one int per problem), then
// d_out[g] = the g-th selected PnpPoint row of the call, g < total = d_compOff[B] as the host counted it;
// d_rowOff / d_compOff: B + 1 ints each. Returns the kernels launched (2; 0 when nothing is selected).
int launch_pnp_batch_gather(const void* d_pts, const uint8_t* d_mask, const BatchPnpEpnpJob* d_jobs, int B,
                            const int* d_rowOff, const int* d_compOff, int total, int* d_idx, int* d_count,
                            void* d_out, hipStream_t s);
// The inlier EPnP's device steps for every job (grid y = job). compact + prep: d_idx / d_pw / d_us are segmented
// like the mask (idx + ptOff, pw + 3 ptOff, us + 2 ptOff), d_count one int per job. Returns 2.
int launch_pnp_batch_epnp_prep(const void* d_pts, const uint8_t* d_mask, const BatchPnpEpnpJob* d_jobs, int nJobs,
                               int maxN, int* d_idx, int* d_count, double* d_pw, double* d_us, hipStream_t s);
// One pass: job j's partials land at d_part + partOff + regionOff(nblk) as part[acc * nblk + blk], nblk the
// blocks of its inlier count; region: 0 = offset 0, 1 = offset 3 nblkMax (Pw0 beside SumPw), 2 = offset 9 nblk
// (Abt beside Pc). prevRegion >= 0: the pass takes its means from that region's partials (Pw0, Abt).
// Returns the kernels launched (1 up to 65535 jobs, the grid's y limit).
int launch_pnp_batch_epnp_pass(int mode, const BatchPnpEpnpJob* d_jobs, int nJobs, int maxNblk, const int* d_count,
                               const double* d_pw, const double* d_us, int nacc, int region, int prevRegion,
                               double* d_part, hipStream_t s);

// ---- shared (ransac_common.hip)
void launch_best(const int* d_counts, int n, int64_t hypBegin, int minCount, uint64_t* d_pkey, int64_t* d_pfail,
                 uint64_t* d_out, hipStream_t s);
void launch_fill_u8(uint8_t* d, int n, uint8_t v, hipStream_t s);

// ---- point-buffer fingerprints (plan_guard.hip; mcv_common.h fp_term): d_out = the sum, async
void launch_fingerprint(const void* d_buf, size_t bytes, uint64_t* d_out, hipStream_t s);
uint64_t host_fingerprint(const void* h_buf, size_t bytes);

// ---- match -> RANSAC hand-off (match_pipeline.hip)
void launch_match_compact(const int* d_idx, const int* d_di1, const int* d_di2, const float* d_df1,
                          const float* d_df2, const int* d_idxBack, int nq, float ratio, float maxDist,
                          const uint8_t* d_kpA, const uint8_t* d_kpB, int kpStride, uint8_t* d_keep, int* d_cnt,
                          int* d_off, int* d_pairs, float* d_dist, float* d_pts4, hipStream_t s);

// ---- matchers (match_hamming.hip, match_l2.hip, match_l2u8.hip)
static constexpr int kHammingFormGemm = 0, kHammingFormPopcount = 1;
int launch_match_hamming(const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int bytesPerDesc, int* d_idx,
                         int* d_dist, int* d_idx2, int* d_dist2, hipStream_t s, int form = kHammingFormGemm);
int launch_match_l2(const float* d_q, int nq, const float* d_t, int nt, int dim, int* d_idx, float* d_dist,
                    int* d_idx2, float* d_dist2, hipStream_t s);
int hamming_last_query_tiles();
int l2_last_exact_scans();
int l2_last_gemm_form();
int l2_last_scan_chunks();
// uint8 descriptors under L2 on the int8 matrix cores (match_l2u8.hip): exact, the outputs of
// launch_match_l2 on the same bytes as fp32. check_match_l2u8 throws on a dim / nq / nt outside the
// kernel's range (no device needed).
void check_match_l2u8(const char* who, int nq, int nt, int dim);
int launch_match_l2u8(const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int dim, int* d_idx, float* d_dist,
                      int* d_idx2, float* d_dist2, hipStream_t s);

// ---- batched matching (match_batch.hip): B directed problems over one buffer of all images' rows
// A directed problem: queries = rows [qRow, qRow + nq), train = rows [tRow, tRow + nt) of the
// concatenated buffer; its outputs start at outOff of the concatenated idx / dist arrays.
struct MatchBatchProblem {
    int qRow, nq, tRow, nt, outOff;
};
static constexpr int kMatchBatchRowsHamming = 64;   // query rows per workgroup, XOR / popcount form
static constexpr int kMatchBatchRowsL2 = 128;       // the same, int8 matrix-core form
// d_src [rows][dim] -> d_dst [rows][KP] (KP a power of two in [32, 512]); shift: x ^ 0x80 and d_norms.
void launch_match_batch_prep(const uint8_t* d_src, int rows, int dim, int KP, bool shift, uint8_t* d_dst,
                             int* d_norms, hipStream_t s);
// d_wg: nwg x (problem, query tile). W = words per padded row (8 or 16).
void launch_match_batch_hamming(const uint8_t* d_rows, int W, const MatchBatchProblem* d_prob, const int* d_wg,
                                int nwg, int* d_idx, int* d_dist, int* d_idx2, int* d_dist2, hipStream_t s);
void launch_match_batch_l2u8(const uint8_t* d_rows, const int* d_norms, int KP, const MatchBatchProblem* d_prob,
                             const int* d_wg, int nwg, int* d_idx, float* d_dist, int* d_idx2, float* d_dist2,
                             hipStream_t s);
void launch_match_batch_compact(const int* d_idx, const int* d_di1, const int* d_di2, const float* d_df1,
                                const float* d_df2, const MatchBatchProblem* d_prob, const int* d_qStart, int B,
                                bool cross, int totalQ, float ratio, float maxDist, uint8_t* d_keep, int* d_cnt,
                                int* d_off, int* d_pairs, float* d_dist, int* d_offsets, hipStream_t s);

// ---- CameraPose.findScaled (scaled_pose.hip)
struct ScaledSetup;
void launch_scaled(const ScaledSetup& S, const double* d_w3, const double* d_o2, int N, double* d_soa,
                   double* d_scales, uint8_t* d_used, double* d_costs, long long* d_out, hipStream_t s);

// ---- batched CameraPose.findScaled (scaled_batch.hip; the index spaces: scaled_batch_index.h). d_soa: 5
// streams of R rows (all sets' rows, set after set); d_setups / d_probs: one per problem; d_blockProb: the
// work list, the problem of each of the nBlocks blocks of 64 candidates; d_scales / d_costs: every problem's
// 2 N candidates at its candOff, d_used: its N observations at candOff / 2. One launch each.
struct ScaledBatchProb;
void launch_scaled_batch_pack(const double* d_w3, const double* d_o2, int R, double* d_soa, hipStream_t s);
void launch_scaled_batch_candidates(const ScaledSetup* d_setups, const ScaledBatchProb* d_probs,
                                    const int* d_blockProb, int nBlocks, const double* d_soa, int R,
                                    double* d_scales, uint8_t* d_used, hipStream_t s);
void launch_scaled_batch_costs(const ScaledSetup* d_setups, const ScaledBatchProb* d_probs, const int* d_blockProb,
                               int nBlocks, const double* d_soa, int R, const double* d_scales,
                               const uint8_t* d_used, double* d_costs, hipStream_t s);
// d_res: cost[P], scale[P] (doubles), evaluated[P] (64-bit integers) — every problem, the empty ones included
void launch_scaled_batch_best(const ScaledBatchProb* d_probs, int P, const double* d_costs, const double* d_scales,
                              const uint8_t* d_used, double* d_res, hipStream_t s);

// ---- Ray.intersection over many tracks (triangulate.hip)
static const int kTriShortMax = 16;   // tracks of at most this many rays: one lane each; longer: one workgroup each
static const int kTriGrid = 2048;     // blocks of the grid-stride kernels whose length lives on the device
// d_ctr: kTriCtrs counters, zeroed by the caller before the launches below.
//   [0] long tracks queued, [1] tracks with a point, [2] first bad track + 1 (validation), [3] its kind,
//   [4] first bad observation + 1
static const int kTriCtrs = 8;
// Checks the CSR offsets and (d_cameraIdx != nullptr) the camera indices on the device: two launches.
void launch_tri_validate(const int* d_offsets, int T, const int* d_cameraIdx, int nCameras, unsigned int* d_ctr,
                         hipStream_t s);
// Camera.unproject1 of every observation of the T tracks into d_rays (6 doubles each): one launch.
void launch_tri_unproject(const double* d_cameras, const int* d_cameraIdx, const double* d_obs,
                          const int* d_offsets, int T, double* d_rays, hipStream_t s);
// Points and pair counts of T tracks over d_rays: two launches (short tracks and the long-track queue).
void launch_tri_intersect(const double* d_rays, const int* d_offsets, int T, double* d_points, int* d_pairCounts,
                          int* d_longList, unsigned int* d_ctr, hipStream_t s);
// Per-track cost / visible (either may be null, not both): one launch.
void launch_tri_stats(const double* d_cameras, const int* d_cameraIdx, const double* d_obs, const int* d_offsets,
                      int T, const double* d_points, double* d_cost, int* d_visible, hipStream_t s);

// ---- track building: pairwise matches -> track CSR (tracks.hip)
static const int kTrkShortMax = 32;   // components of at most this many nodes: one lane each; longer: one workgroup each
static const int kTrkGrid = 2048;     // blocks of the grid-stride kernels
// d_ctr: kTrkCtrs 64-bit words, zeroed by the caller before launch_build_tracks.
//   [0] oversize, [1] conflicts, [2] short, [3] fail word (a bounded loop gave up),
//   [4] candidates << 32 | their nodes, [5] tracks << 32 | observations, [6] long candidates queued
static const int kTrkCtrs = 8;
static const int kTrkScanItems = 2048;   // nodes per block of the two scans
static const int kTrkScanChunk = 1024;   // block sums per trip (and threads) of the one-block scan over them: it carries between trips
struct TrkDevice {
    const int* edges;        // 2 nEdges node ids
    long long nEdges;
    const int* base;         // nImages + 1
    int nImages, nNodes, minLength;
    int* parent;             // nNodes each: parent, size, cursor, trk
    int* size;
    int* cursor;
    int* trk;
    uint8_t* touched;        // nNodes
    unsigned long long* blockSums;   // ceil(nNodes / kTrkScanItems) + 1
    int slotCap;             // min(2 nEdges, nNodes): the nodes a call can touch
    int* slots;              // slotCap
    int* candList;           // slotCap / 2 + 1
    int* longList;           // slotCap / kTrkShortMax + 1
    int* trackOffsets;       // slotCap / 2 + 1
    int* cameraIdx;          // slotCap
    int* featureIdx;         // slotCap
    int* trackOfFeature;     // nNodes, or null
    unsigned long long* ctr;
};
static const int kTrkLaunches = 13;
// All launches of a call (kTrkLaunches of them, whatever the sizes); the results stay on the device.
void launch_build_tracks(const TrkDevice& D, hipStream_t s);

// ---- bundle adjustment (bundle_adjust.hip)
static const int kBaGrid = 2048;         // blocks of the grid-stride kernels
static const int kBaLongBlocks = 1024;   // blocks (4 waves each) striding over the long-track queue
// The record of one PCG solve, on the device: read back once per chunk of kBaCgChunk iterations.
struct BaCgState {
    double rz, rz0;
    int iter, done, failed, pad;
};
// Cost and flag of one evaluation of the parameters, read back once per trial.
struct BaCostRecord {
    double cost;
    int badz, pad;
};
// d_ctr: [0] long tracks queued, [1] used observations, [2] used tracks, [3] a factorisation of the
// current solve failed, [4] a used observation has pc.z <= 0 in the cost being evaluated
static const int kBaCtrs = 8;
struct BaDevice {
    int nCameras, T, n, nSeg;
    const int *offsets, *cameraIdx, *obsTrack, *camObs, *segCam, *segStart, *segEnd, *camSegPtr;
    const double* obs;          // 2 n
    const uint8_t* fixed;       // nCameras
    double *cams, *pts;         // the current parameters: 14 nCameras, 3 T
    double *cams2, *pts2;       // the trial copy
    uint8_t *used, *trackUsed, *active;   // n, T, nCameras
    double* E;                  // kBaEntry n: A, B, r of every used observation
    double *U, *g, *L, *b;      // per camera: 21, 6, 21, 6
    double *x, *r, *z, *p, *q, *pq;   // per camera: 6 each, pq 1
    double *V, *h, *Vinv, *t, *y;     // per point: 6, 3, 6, 3, 3
    double* part;               // 27 per segment: the segments' partial sums of the pass in flight
    int* longList;              // T
    unsigned int* ctr;
    BaCgState* cg;
    BaCostRecord* rec;
    double lambda, delta, tol2;
    int maxCg;
};
// launches of each stage, whatever the sizes
static const int kBaLaunchesSetup = 3, kBaLaunchesCost = 2, kBaLaunchesLinearize = 4, kBaLaunchesSystem = 4,
                 kBaLaunchesCgIter = 5, kBaLaunchesTrial = 3 + kBaLaunchesCost;
void launch_ba_setup(const BaDevice& D, hipStream_t s);       // the used set, the long-track queue, the active cameras
void launch_ba_cost(const BaDevice& D, const double* d_cams, const double* d_pts, hipStream_t s);   // -> D.rec
void launch_ba_linearize(const BaDevice& D, hipStream_t s);   // E, V, h, U, g at D.cams / D.pts
void launch_ba_system(const BaDevice& D, hipStream_t s);      // Vinv, t, L, b at D.lambda and the PCG start
void launch_ba_cg_iteration(const BaDevice& D, hipStream_t s);
void launch_ba_trial(const BaDevice& D, hipStream_t s);       // cams2 / pts2 from x, and their cost -> D.rec

// ---- bundle adjustment with focal groups (bundle_adjust.hip): what cvBundleAdjustFocal
// keeps beside a BaDevice. d_ctr[5] counts the free groups.
struct BaFocal {
    int fm, nG;                 // focalMode 1 or 2, groups
    const int *camGrp, *grpPtr, *grpCam;   // nCameras, nG + 1, nCameras: a group's cameras in ascending index
    const uint8_t* grpFixed;    // nG
    uint8_t* grpFree;           // nG: not fixed, and a camera of the group has a used observation
    double* Ef;                 // 2 n: the focal block of every used observation
    double* partF;              // kBaFocalPart per segment: the focal sums of the pass in flight
    double *Gd, *gf, *Lf, *bf;  // per group: 2, 2, 3, 2
    double *xf, *rf, *zf, *pf, *qf, *pqf;   // per group: 2 each, pqf 1
};
static const int kBafLaunchesSetup = kBaLaunchesSetup + 1, kBafLaunchesLinearize = 6, kBafLaunchesSystem = 5,
                 kBafLaunchesCgIter = 6, kBafLaunchesTrial = 4 + kBaLaunchesCost;
void launch_baf_setup(const BaDevice& D, const BaFocal& F, hipStream_t s);
void launch_baf_linearize(const BaDevice& D, const BaFocal& F, hipStream_t s);
void launch_baf_system(const BaDevice& D, const BaFocal& F, hipStream_t s);
void launch_baf_cg_iteration(const BaDevice& D, const BaFocal& F, hipStream_t s);
void launch_baf_trial(const BaDevice& D, const BaFocal& F, hipStream_t s);

// ---- SIFT detection (sift.hip; the records are sift_math.h's)
struct SiftParams;
struct SiftKp;
struct SiftRec;
static const int kSiftMaxOctaves = 16;   // round(log2(2 x 8192) - 2) = 12 at the size cap
struct SiftPyramid {
    const float* base;                    // every octave's nl + 3 Gaussian images
    size_t obase[kSiftMaxOctaves];        // float offset of an octave's first image
    int ow[kSiftMaxOctaves], oh[kSiftMaxOctaves];
    int rowBase[kSiftMaxOctaves];         // first bucket of an octave: a bucket is one (octave, layer, row)
};
// bucket of the order stage: rowBase[o] + (layer - 1) oh[o] + r, layer in 1 .. OctaveLayers
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int sift_bucket(const SiftPyramid& Y, int o, int layer, int r) {
    return Y.rowBase[o] + (layer - 1) * Y.oh[o] + r;
}
struct SiftKeyPointOut {   // KeyPoint2d's 28 bytes
    float x, y, size, angle, response;
    int octave, class_id;
};
static const int kSiftRowTile = 256;                        // outputs per block of the row blur
static const int kSiftColTileW = 64, kSiftColTileH = 32;    // outputs per block of the column blur
// d_ctr: [0] candidates, [1] refined, [2] keypoints with orientations, [3] keypoints kept
static const int kSiftCtrs = 4;
// Kernel launches of a cvDetectFeatures call: kSiftLaunchesFixed (grey + doubling, the base blur's two,
// refine, orientation, the order's scan, scatter, rank and compaction, descriptors) + nOctaves x
// (kSiftLaunchesPerBlur x (OctaveLayers + 2) + kSiftLaunchesExtrema) + (nOctaves - 1) x
// kSiftLaunchesDownsample + kSiftLaunchesSelect if FeatureCount > 0. Stream synchronisations, copies and
// memsets are the same for every call that reaches the device with nOctaves > 0.
static const int kSiftLaunchesFixed = 10, kSiftLaunchesPerBlur = 2, kSiftLaunchesExtrema = 1,
                 kSiftLaunchesDownsample = 1, kSiftLaunchesSelect = 1;
static const int kSiftSyncs = 4, kSiftCopies = 7, kSiftMemsets = 1;
void launch_sift_grey_double(const uint8_t* d_img, int w, int h, int ch, float* d_up, hipStream_t s);
// d_out = blur of d_in (rows into d_tmp, then columns); taps[2 R + 1] on the device. Two launches.
void launch_sift_blur(const float* d_in, float* d_out, float* d_tmp, int w, int h, const float* d_taps, int R,
                      hipStream_t s);
void launch_sift_downsample(const float* d_src, int pw, float* d_dst, int w, int h, hipStream_t s);
// Appends (o, layer, r, c) int4 records to d_cand (places >= cap are counted, not written).
void launch_sift_extrema(const float* d_g, int w, int h, int o, int nl, float thr, void* d_cand, unsigned cap,
                         unsigned* d_ctr, hipStream_t s);
void launch_sift_refine(const SiftPyramid& Y, const SiftParams& P, const void* d_cand, int nC, SiftKp* d_kps,
                        unsigned* d_ctr, hipStream_t s);
// d_recs, d_keys, d_starts, d_rkeys: 18 nC each (a candidate has at most 18 orientation peaks); d_bcnt: a
// counter per bucket, zeroed by the caller.
void launch_sift_orient(const SiftPyramid& Y, const void* d_cand, const SiftKp* d_kps, int nC, SiftRec* d_recs,
                        unsigned long long* d_keys, unsigned long long* d_starts, unsigned long long* d_rkeys,
                        unsigned* d_ctr, unsigned* d_bcnt, hipStream_t s);
// The order stage over the n appended records: 4 launches, 5 with featureCount > 0 (sift.hip).
struct SiftOrder {
    int nBuckets;
    unsigned *bcnt, *boff;                                   // nBuckets, nBuckets + 1
    const unsigned long long *keys, *starts, *rkeys;         // as appended
    const SiftRec* recs;
    int *perm, *sortedIdx;                                   // n each
    unsigned long long *skeys, *srkeys;                      // n each: the keys in order
    uint8_t *keepA, *keepB;                                  // n each
    SiftRec* out;                                            // n
    unsigned* count;
};
void launch_sift_order(const SiftPyramid& Y, const SiftOrder& O, int n, int featureCount, hipStream_t s);
void launch_sift_describe(const SiftPyramid& Y, const SiftRec* d_recs, int n, int descType, SiftKeyPointOut* d_kp,
                          uint8_t* d_u8, float* d_f32, hipStream_t s);

// ---- batched SIFT detection (sift_batch.hip): the stages above over (image, tile),
// (image, candidate) and (image, keypoint) grids. The kernels find an image's sizes and offsets in the
// table of SiftBatchImage (sift_batch_plan.h), uploaded once; a block outside its image's extent or
// past its last octave leaves before it touches memory or a barrier.
struct SiftBatchImage;
struct SiftBatchDevice {
    const SiftBatchImage* table;
    int nImages;
    const uint8_t* img;                                      // the staged images
    float *up, *tmp, *pyr;                                   // doubled bases, row-blur scratch, pyramids
    const float* taps;
    // d_ctr as above; icnt: candidates per image; koff: nImages + 1 offsets of the images' kept keypoints;
    // part: kSiftBatchScanBlocks + 1 words of the grid-wide scans
    unsigned *ctr, *icnt, *bcnt, *boff, *koff, *part;
    int nBuckets;
    int4* cand;                                              // (image << 4 | octave, layer, r, c)
    unsigned capC;
};
void launch_sift_batch_grey_double(const SiftBatchDevice& D, int maxW, int maxH, hipStream_t s);
// Blur `blur` (0: the doubled base into image 0 of octave 0; i: image i - 1 into image i) of octave o
// of every image that has it. Two launches, sized by the largest image of that octave.
void launch_sift_batch_blur(const SiftBatchDevice& D, int o, int blur, int tapOff, int R, int maxW, int maxH,
                            hipStream_t s);
void launch_sift_batch_downsample(const SiftBatchDevice& D, int o, int nl, int maxW, int maxH, hipStream_t s);
void launch_sift_batch_extrema(const SiftBatchDevice& D, int o, int nl, float thr, int maxW, int maxH, hipStream_t s);
void launch_sift_batch_refine(const SiftBatchDevice& D, const SiftParams& P, int nC, SiftKp* d_kps, hipStream_t s);
void launch_sift_batch_orient(const SiftBatchDevice& D, const SiftKp* d_kps, int nC, SiftRec* d_recs,
                              unsigned long long* d_keys, unsigned long long* d_starts, unsigned long long* d_rkeys,
                              hipStream_t s);
// The order stage over the n appended records of all images: 10 launches, 11 with featureCount > 0. O as
// for the single call (its nBuckets, bcnt, boff and count are D's); d_pos: n + 1 words.
void launch_sift_batch_order(const SiftBatchDevice& D, const SiftOrder& O, unsigned* d_pos, int n, int featureCount,
                             hipStream_t s);
void launch_sift_batch_describe(const SiftBatchDevice& D, const SiftRec* d_recs, int n, int descType,
                                SiftKeyPointOut* d_kp, uint8_t* d_u8, float* d_f32, hipStream_t s);

}  // namespace mcv
