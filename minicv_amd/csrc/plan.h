// plan.h — device workspace of one RANSAC problem family (homography, fundamental, affine / similarity,
// essential or PnP) on one GPU, and what the shared framework (ransac_host.cpp) and the per-family host
// files declare to each other.
#pragma once

#include "minicv_native.h"
#include "mcv_runtime.h"
#include "mcv_common.h"
#include "ransac_batch_index.h"
#include <stdint.h>
#include <string.h>
#include <vector>

namespace mcv {

// Host-API chunking of the hypothesis stream for the adaptive (sequential-replay) search.
static const int64_t kChunkFirst = 4096;
static const int64_t kChunkMax = 1 << 20;

struct Plan;

// ---- the family table: one record per MCV_MODEL_*, what the shared framework (ransac_host.cpp) needs to know
// about a model family and the family's own code behind one set of hook signatures. family_of(model) returns it.
// The constant part is device-free and constexpr; ransac_host.cpp pins every entry with static_asserts.
struct FamilyShape {
    const char* name;
    int points;           // minimal sample size (a configuration may change it: points_cfg)
    int slots;            // model slots per hypothesis (slots_cfg)
    int modelBytes;       // device model bytes per hypothesis
    bool doublePoints;    // points are 32 B each (essential double4, PnP rows) in Plan::ptsd; else float4 in Plan::pts
    bool defaultThreshold;   // thr2_of: a threshold <= 0 means 3 pixels (the 2-D families); essential / PnP: as given
    double defaultConfidence;   // config_or_default (OpenCV's per function); essential / PnP: e_config, pnp_config
    int h64PerHyp;        // doubles per hypothesis of Plan::h64, the generate's fp64 models (0: the family has none)
};
constexpr FamilyShape kFamilyShapes[] = {
    {"homography", 4, 1, 32, false, true, 0.995, 9},   // MCV_MODEL_HOMOGRAPHY
    {"fundamental", 8, 1, 80, false, true, 0.99, 0},   // MCV_MODEL_FUNDAMENTAL
    {"essential", 5, 10, 720, true, false, 0.999, 0},  // MCV_MODEL_ESSENTIAL
    {"pnp", 4, 1, 96, true, false, 0.99, 0},           // MCV_MODEL_PNP
    {"affine", 3, 1, 24, false, true, 0.99, 6},        // MCV_MODEL_AFFINE
    {"similarity", 2, 1, 24, false, true, 0.99, 6},    // MCV_MODEL_SIMILARITY
};
// The hooks. d_pts is the family's device point buffer (doublePoints tells its layout); a null hook: the family
// has none. generate = one chunk's models, statuses and P.last (shared by the RANSAC evaluate and lmeds_search);
// evaluate = generate + verify into d_counts (keyOnly: nobody reads d_counts beyond the best-key reduction, which
// only the homography sweep exploits); finalize = the winner's model and mask, returns its inlier count.
using ReserveHook = void(Plan& P);
using GenerateHook = void(Plan& P, const void* d_pts, int N, const RansacConfig& cfg, int64_t hypBegin, int hypCount,
                          int* d_counts, hipStream_t s);
using EvaluateHook = void(Plan& P, const void* d_pts, int N, const RansacConfig& cfg, int64_t hypBegin, int hypCount,
                          int* d_counts, bool keyOnly, hipStream_t s);
using FinalizeHook = int(Plan& P, const void* d_pts, int N, const RansacConfig& cfg, int64_t hyp, double* model9,
                         uint8_t* d_mask, hipStream_t s);
using HostHypothesisHook = int(int model, const float* pts4, int N, uint64_t seed, int64_t hyp, double* model9,
                               float* modelf9, int* sampleIdx, bool fast);
using ConfigIntHook = int(const RansacConfig& cfg);
// find_model_2d's family-specific parts. refuse: the refusals that depend on the configuration, the minimal-N
// one included (null: N < points, before the configuration is read). direct: the cases solved on all points
// without a search (count = N, mask all 1); false: not one of them.
using EntryRefuseHook = void(const char* who, int N, const RansacConfig& cfg);
using EntryDirectHook = bool(Plan& P, const char* who, int N, const RansacConfig& cfg, hipStream_t s, double* model9);
struct RansacFamily : FamilyShape {
    ReserveHook* reserve;        // further buffers of its own for P.maxN points / P.maxHyps hypotheses (essential)
    GenerateHook* generate;
    EvaluateHook* evaluate;
    FinalizeHook* finalize;
    HostHypothesisHook* host_hypothesis;
    ConfigIntHook* points_cfg;   // null: points whatever the configuration (PnP with EPnP: 5; 7-point F: 7)
    ConfigIntHook* slots_cfg;    // null: slots (7-point F: 3)
    bool lsq;                    // MCV_METHOD_LSQ is one of the 2-D entry's methods (a direct case)
    EntryRefuseHook* entry_refuse;
    EntryDirectHook* entry_direct;
};
const RansacFamily& family_of(int model);   // throws on a model outside the table
// forwards of the table
size_t model_bytes(int model);
int model_points(int model), model_slots(int model);
int model_points_cfg(int model, const RansacConfig& cfg), model_slots_cfg(int model, const RansacConfig& cfg);
size_t point_bytes(int model, int N);   // device point buffer: 16 N (float4), 32 N (E double4, PnP rows)

// The minimal solver that produced a chunk's models (LastChunk::kind).
enum ChunkSolver : int {
    kSolverNone = -1,
    kSolverHEigen, kSolverHElimination,     // homography: the reference's eigen solve / MCV_FLAG_FAST_MINIMAL
    kSolverF8Exact, kSolverF8Fast,          // 8-point fundamental
    kSolverEReference, kSolverEFast,        // five-point essential
    kSolverAp3p, kSolverEpnp, kSolverAp3pFast,   // PnP
};

// Key of the last evaluated chunk. A winner inside it takes its model from the chunk's buffers
// instead of a re-solve; the key names everything that produced those buffers (the hypothesis
// range, the sample source, the point buffer and N, the minimal solver), and every evaluate replaces
// it, so any other evaluate in between, or a different solver / sampler, invalidates it. The points'
// content is keyed too: the evaluate fingerprints the buffer (Plan::fp[0], mark_chunk), finalize
// fingerprints it again and re-solves the winner when the two differ (a caller that rewrote the
// buffer in place, same pointer and N, between evaluate and finalize).
struct LastChunk {
    int64_t begin = -1, count = 0;
    uint64_t seed = 0;
    const int* table = nullptr;
    const void* pts = nullptr;
    int N = 0;
    ChunkSolver kind = kSolverNone;
    void set(int64_t b, int64_t c, const Sampler& smp, const void* p, int n, ChunkSolver k) {
        begin = b; count = c; seed = smp.seed; table = smp.table; pts = p; N = n; kind = k;
    }
    void clear() { *this = LastChunk(); }
    bool covers(int64_t hyp, const Sampler& smp, const void* p, int n, ChunkSolver k) const {
        return begin >= 0 && hyp >= begin && hyp < begin + count && seed == smp.seed && table == smp.table &&
               pts == p && N == n && kind == k;
    }
};

struct Plan {
    int model = MCV_MODEL_HOMOGRAPHY;
    int device = 0;
    int shard = 0;
    int maxN = 0;
    int64_t maxHyps = 0;
    hipStream_t stream = nullptr;   // only for the host-pointer exports

    DevBuf<float> pts;        // packed float4 correspondences (host-API path)
    DevBuf<uint8_t> models;   // per-hypothesis fp32 models
    DevBuf<int> counts;       // per-hypothesis status / inlier count
    DevBuf<uint64_t> pkey;    // best-key partials
    DevBuf<int64_t> pfail;
    DevBuf<uint64_t> key;
    DevBuf<double> part;      // reduction partials
    DevBuf<double> red;       // reduction result
    DevBuf<uint8_t> mask;
    DevBuf<int> count;
    DevBuf<float> bbox;       // max |x|, max |y| of the source points (fused fast-path bound)
    DevBuf<double> bb4;       // F / E: max |x1|, |y1|, |x2|, |y2| (packed-fp32 Sampson prefilter bound)
    DevBuf<double> h64;       // homography: each hypothesis' fp64 model (finalize takes the winner's);
                              // affine / similarity: the generate's fp64 models (6 per hypothesis)
    DevBuf<uint8_t> hgen;     // homography: the split eigen generate's scratch (rotation log of one piece)
    bool hrowLast = false;    // the last homography generate ran the certified one-row pass 2: h64 holds only the
                              // undecided lanes' models
    bool hrowLogKept = false; // ... and hgen still holds that chunk's log, samples and meta words (one piece)
    int hrowCount = 0;        // the last homography generate's hypotheses (the layout of hgen)
    DevBuf<float> pairs;      // paired point layout of the packed sweeps (homography 8, PnP 12 floats per 2)
    DevBuf<char> hrec;        // homography matrix-core sweep: the bf16 point records (h_rec_bytes(N): 24 B per point)
    DevBuf<unsigned long long> hmfmaStats;   // its undecided rows / overflowed / out-of-domain waves of the last sweep (kHMfmaStats)
    bool hmfmaLast = false;   // the last certified homography sweep ran the matrix-core kernel
    DevBuf<int> hstageList;   // homography staged sweep: the two survivor lists (2 x hypCount slots)
    DevBuf<int> hstageCtl;    // homography staged sweep: the control block (kHStageCtlInts)
    int hstageLast = -1;      // last homography evaluate: 0 staged (the control block tells), else kHStage*
    DevBuf<int> hcells;       // homography staged sweep: the per-cell bound's cell table (kHCellInts ints per cell)
    DevBuf<int> hcellId;      // its cell of every correspondence (N)
    DevBuf<int> hcellPref;    // its prefix table: per later boundary and cell, the cell's points before the boundary
    DevBuf<int> hcellLeft;    // per later boundary and slot: the unprocessed points of the slot's uncertified cells
    DevBuf<int> hstage0;      // stage 0 on a leading subset of the slots: its counts (the subset's slots)
    DevBuf<int> hcellRec;     // the bound passes' record list of the non-empty cells (h_cell_pre.h: h_cell_rec_ints)
    DevBuf<unsigned long long> hcellPreStats;   // its (model, cell) tests and the undecided of them, last bound passes
    DevBuf<uint8_t> one;      // single-hypothesis output record
    DevBuf<double> ptsd;      // essential: double4 normalised correspondences
    DevBuf<double> raw;       // essential: uploaded V2d pairs (a then b)
    DevBuf<int> dslot;        // essential: slot of each dense model
    DevBuf<uint8_t> estage;   // essential: per-hypothesis EStage of the split five-point solve
    DevBuf<int> ndense;       // essential: dense model count, 4 cheirality counters, fetch flag
    double pnpCam[8] = {1, 1, 0, 0, 0, 0, 0, 0};   // PnP: fx, fy, cx, cy, k1, k2, p1, p2
    DevBuf<double> epw;       // PnP: EPnP solve points (world, double)
    DevBuf<double> eus;       // PnP: EPnP solve points (pixels of the undistorted observations)
    DevBuf<int> eidx;         // PnP: inlier indices of the EPnP solve
    DevBuf<double> escratch;  // PnP: the split EPnP generate's per-hypothesis state (kEpnpSplitDoubles each)
    LastChunk last;           // the last evaluated chunk (finalize takes the winner's model from its buffers)
    DevBuf<int> subsets;      // MCV_FLAG_CV_SAMPLER: OpenCV's getSubset stream, subsetM ints per hypothesis
    int64_t subsetRows = 0;   // hypotheses [0, subsetRows) covered by `subsets`
    int subsetM = 0;
    int subsetN = 0;          // the N the table was drawn for (its rows index [0, subsetN))
    uint64_t subsetFp = 0;    // H / F: fingerprint of the points whose checkSubset accepted the rows
    DevBuf<uint64_t> fp;      // [0] the last chunk's points (mark_chunk), [1] the points at finalize / check
    PinnedBuf<uint64_t> h_fp;
    Sampler sampler(const RansacConfig& cfg) const;
    PinnedBuf<int> h_counts;
    PinnedBuf<double> h_red;
    PinnedBuf<float> h_pack;
    PinnedBuf<uint8_t> h_one;
    PinnedBuf<int> h_i;
    PinnedBuf<uint64_t> h_keys;   // per-shard best key + first failure (fixed-iteration searches)
    DevBuf<uint32_t> med;         // LMedS: each model slot's median order key (lmeds.hip)
    PinnedBuf<uint32_t> h_med;

    void reserve(int n, int64_t hyps);
    hipStream_t own_stream();
    ~Plan();
};

Plan& thread_plan(int model, int shard = 0);   // current device; shard > 0: extra per-device workspaces
static const int kMaxShards = 16;

// Sum V doubles over (masked) correspondences: GPU two-stage reduction, result to host.
template <class F>
inline void reduce_to_host(Plan& P, hipStream_t s, int V, double* out, F launch) {
    launch(P.part.p, P.red.p);
    MCV_HIP(hipGetLastError());
    MCV_HIP(hipMemcpyAsync(P.h_red.p, P.red.p, V * sizeof(double), hipMemcpyDeviceToHost, s));
    MCV_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < V; ++i) out[i] = P.h_red.p[i];
}

// The winner's mask (P.mask) to the caller's host buffer, when it wants one. Synchronises s.
inline void mask_to_host(Plan& P, uint8_t* mask, int N, hipStream_t s) {
    if (!mask) return;
    MCV_HIP(hipMemcpyAsync(mask, P.mask.p, (size_t)N, hipMemcpyDeviceToHost, s));
    MCV_HIP(hipStreamSynchronize(s));
}

// The squared inlier threshold the verify and mask kernels take. The 2-D families read a threshold <= 0 as
// 3 pixels (effective_threshold); essential and PnP take the configuration's as given.
double effective_threshold(const RansacConfig& cfg);
inline float thr2_of(const Plan& P, const RansacConfig& cfg) {
    const double t = kFamilyShapes[P.model].defaultThreshold ? effective_threshold(cfg) : cfg.threshold;
    return (float)(t * t);
}

// The winner record (a T at d_src, by default the plan's single-hypothesis record P.one) to the host:
// queue_one enqueues the copy, take_one reads it after the caller's next synchronisation of s (so that a
// finalize can return the record, the count and the freshness words with one synchronisation), fetch_one
// is the two around a synchronisation of its own, after the launch that wrote the record.
template <class T>
inline void queue_one(Plan& P, hipStream_t s, const void* d_src = nullptr) {
    MCV_HIP(hipMemcpyAsync(P.h_one.p, d_src ? d_src : P.one.p, sizeof(T), hipMemcpyDeviceToHost, s));
}
template <class T>
inline T take_one(const Plan& P) {
    T one;
    memcpy(&one, P.h_one.p, sizeof(T));
    return one;
}
template <class T>
inline T fetch_one(Plan& P, hipStream_t s, const void* d_src = nullptr) {
    MCV_HIP(hipGetLastError());
    queue_one<T>(P, s, d_src);
    MCV_HIP(hipStreamSynchronize(s));
    return take_one<T>(P);
}

// The winner's inlier count: a mask kernel adds to P.count, zeroed before it (zero_count); queue_count
// enqueues its copy to the host and take_count reads it after the caller's next synchronisation.
// mask_count is the whole sequence around launch(int* d_count), with a synchronisation of its own.
inline void zero_count(Plan& P, hipStream_t s) { MCV_HIP(hipMemsetAsync(P.count.p, 0, sizeof(int), s)); }
inline void queue_count(Plan& P, hipStream_t s) {
    MCV_HIP(hipMemcpyAsync(P.h_i.p, P.count.p, sizeof(int), hipMemcpyDeviceToHost, s));
}
inline int take_count(const Plan& P) { return P.h_i.p[0]; }
template <class F>
inline int mask_count(Plan& P, hipStream_t s, F launch) {
    zero_count(P, s);
    launch(P.count.p);
    MCV_HIP(hipGetLastError());
    queue_count(P, s);
    MCV_HIP(hipStreamSynchronize(s));
    return take_count(P);
}

// Opt-in kernel timing with HIP events recorded on the launch stream (bench.py's live roofline).
// mcvProfileEnable(n): every n-th launch of each named scope is timed (n = 1: all of them). An event
// pair costs the stream ~3 us each way, 17 % of the 36 us cfg2 Hamming step when every launch is
// timed (scripts/exp/ham_gap.py); a sample keeps the average launch duration and not that cost.
bool prof_enabled();
bool prof_sample(const char* name);   // prof_enabled() and this launch is one of the sampled ones
void prof_record(const char* name, hipEvent_t a, hipEvent_t b);
hipEvent_t prof_event();   // a timing event (reused across mcvProfileReset)
struct ProfScope {
    const char* name;
    hipStream_t s;
    hipEvent_t a = nullptr, b = nullptr;
    ProfScope(const char* n, hipStream_t st) : name(n), s(st) {
        if (prof_sample(n) && (a = prof_event()) && (b = prof_event())) (void)hipEventRecord(a, s);
    }
    ~ProfScope() {
        if (a && b) {
            (void)hipEventRecord(b, s);
            prof_record(name, a, b);
        }
    }
};
// n correspondences a[i] -> b[i] as float4 {a.X, a.Y, b.X, b.Y} (OpenCV: points.convertTo(CV_32F))
inline void pack_float4(const mcvV2d* a, const mcvV2d* b, int n, float* dst) {
    for (int i = 0; i < n; ++i) {
        dst[4 * (size_t)i + 0] = (float)a[i].X;
        dst[4 * (size_t)i + 1] = (float)a[i].Y;
        dst[4 * (size_t)i + 2] = (float)b[i].X;
        dst[4 * (size_t)i + 3] = (float)b[i].Y;
    }
}
void pack_points(Plan& P, const mcvV2d* a, const mcvV2d* b, int N, float* d_dst, hipStream_t s);
// Evaluate side: P.last = this chunk, and the fingerprint of its points -> P.fp[0] (async).
void mark_chunk(Plan& P, int64_t begin, int64_t count, const Sampler& smp, const void* d_pts, int N,
                ChunkSolver kind, hipStream_t s);
// Finalize side, on the cached-model path: the current points' fingerprint -> P.fp[1], both to
// P.h_fp (async; chunk_fresh reads them after the caller's next stream synchronisation).
void queue_chunk_check(Plan& P, const void* d_pts, int N, hipStream_t s);
inline bool chunk_fresh(const Plan& P) { return P.h_fp.p[0] == P.h_fp.p[1]; }
// The device points' fingerprint, synchronously (CV-sampler table checks).
uint64_t device_fingerprint(Plan& P, const void* d_pts, int N, hipStream_t s);
bool cv_sampler(const RansacConfig& cfg);   // MCV_FLAG_CV_SAMPLER
void check_flags(const RansacConfig& cfg, const char* who);   // rejects the retired bit 4
// OpenCV's subset stream (cv_sampler.cpp): rows [0, rows) for P's model / cfg, uploaded to P.subsets.
// h_pts4: host float4 points for the models with a checkSubset (H, F); nullptr = read from d_pts.
void cv_table_build(int model, const RansacConfig& cfg, const float* h_pts4, int N, int64_t rows, std::vector<int>& out);
void cv_table_upload(Plan& P, const std::vector<int>& t, int m, int64_t rows, int N, uint64_t pointsFp,
                     hipStream_t s);
bool cv_table_reads_points(int model);   // the table depends on the points (H / F checkSubset), not only N
// host float4 points -> the fingerprint a table records (0 for the models whose table ignores them)
uint64_t cv_table_points_fp(int model, const float* h_pts4, int N);
void cv_table_prepare(Plan& P, const void* d_pts, const float* h_pts4, int N, const RansacConfig& cfg, int64_t rows,
                      hipStream_t s);
bool fused_error(const RansacConfig& cfg);
bool fast_minimal(const RansacConfig& cfg);   // MCV_FLAG_FAST_MINIMAL
// *cfg, or the 2-D exports' defaults for the model (OpenCV's: threshold 3, 2000 iterations, its own sample stream,
// the family's defaultConfidence)
RansacConfig config_or_default(int model, const RansacConfig* cfg);
int64_t ransac_search(Plan& P, const void* d_pts, int N, const RansacConfig& cfg, hipStream_t s,
                      const float* h_pts4 = nullptr);
// LMedS (method 4) on device-resident H / F / affine-family points: RANSACUpdateNumIters(confidence, 0.45, m, maxIters)
// hypotheses in one chunk, each slot's median error (lmeds.hip), first minimum wins. Returns the winning
// slot and its inlier threshold sigma (cfg.threshold is not read); fails when there is no model.
int64_t lmeds_search(Plan& P, const float* d_pts, int N, const RansacConfig& cfg, hipStream_t s, const float* h_pts4,
                     double* sigma);
int finalize(Plan& P, const void* d_pts, int N, const RansacConfig& cfg, int64_t hyp, double* model9,
             uint8_t* d_mask, hipStream_t s);
// needCounts: the caller reads d_counts (every slot's full count). false: only d_key is consumed, and
// the homography sweep may run in self-pruning stages that leave partial counts in pruned slots.
void evaluate_chunk(Plan& P, const void* d_pts, int N, const RansacConfig& cfg, int64_t hypBegin, int hypCount,
                    int* d_counts, uint64_t* d_key, hipStream_t s, bool needCounts = true);

// The 2-D entry (cvFindHomography, cvFindFundamentalMat, cvEstimateAffine2D, cvEstimateAffinePartial2D): the
// refusals, pack, the family's direct cases, LMedS or RANSAC, finalize, the mask to the host. Returns the count.
int find_model_2d(int model, const char* who, const mcvV2d* a, const mcvV2d* b, int N, const RansacConfig* cfgp,
                  double* model9, uint8_t* mask);

// ---- what the families put into the table (ransac_host.cpp: one row each) and what else other files call
// homography family (ransac_h_*.hip / ransac_h_host.cpp)
GenerateHook h_generate;
EvaluateHook h_evaluate;
FinalizeHook h_finalize;
HostHypothesisHook h_host_hypothesis;
EntryDirectHook h_entry_direct;
// runKernel's host half on one refit record (kernels.h kRefit*) -> H; false: degenerate, H is not a model
bool h_refit_from_record(const double* r, double* H);
void h_plan_forget(const Plan* P);   // ~Plan: drops the test hooks' references to the plan

// fundamental-matrix family (ransac_f.hip / ransac_f_host.cpp)
GenerateHook f_generate;
EvaluateHook f_evaluate;
FinalizeHook f_finalize;
HostHypothesisHook f_host_hypothesis;
ConfigIntHook f_points_cfg, f_slots_cfg;
EntryRefuseHook f_entry_refuse;
EntryDirectHook f_entry_direct;
int f_error_kind(const RansacConfig& cfg);
int f_fit_all(Plan& P, const float* d_pts, int N, hipStream_t s, double* F);

// affine / similarity family (ransac_a.hip / ransac_a_host.cpp)
inline bool affine_family(int model) { return model == MCV_MODEL_AFFINE || model == MCV_MODEL_SIMILARITY; }
GenerateHook a_generate;
EvaluateHook a_evaluate;
FinalizeHook a_finalize;
HostHypothesisHook a_host_hypothesis;
EntryDirectHook a_entry_direct;

// PnP family (ransac_pnp.hip / pnp_host.cpp)
EvaluateHook p_evaluate;
FinalizeHook p_finalize;
ConfigIntHook p_points_cfg;
bool pnp_cfg_epnp(const RansacConfig& cfg);   // minimal sets of 5 for EPnP (solverKind 0/1/3/4)
// cvSolvePnPRansac's configuration: OpenCV's sample stream, RANSAC, the given budget / threshold / kind
RansacConfig pnp_config(int iters, float thr, double conf, int kind);

// essential-matrix family (ransac_e.hip / ransac_e_host.cpp)
ReserveHook e_reserve;
EvaluateHook e_evaluate;
FinalizeHook e_finalize;   // hyp = the winning model slot
// The essential exports' configuration: cvFindEssentialMat's (NULL: its defaults) and cvRecoverPose's; e_check
// throws on what the family does not support (method, confidence, the retired flag bit).
RansacConfig e_config(const RansacConfig* cfg);
RansacConfig e_config(const RecoverPoseConfig* rc);
void e_check(const RansacConfig& cfg, const char* who);
int e_kind(const RansacConfig& cfg);   // f_error's kind of the Sampson error (fused 0, op-by-op 1)
extern const double kCheiralityDist;   // recoverPose's distanceThresh for the focal/pp overload

// ---- the RANSAC batch calls (ransac_batch_host.cpp: cvFindModelBatch; ransac_batch_e_host.cpp: the essential
// batches; ransac_batch_pnp_host.cpp: the PnP batches). Their layout and round plan: ransac_batch_index.h; the
// round driver and the host helpers they share: batch_host.h.
struct BatchStats : CallStats {          // copies: host <-> device, every family; memsets are not counted
    long long rounds = 0, lmRounds = 0, single = 0, problems = 0;
    long long packUs = 0, tableUs = 0;   // host time: point conversion, OpenCV sample tables
    long long problemRounds = 0;         // problems summed over the hypothesis rounds they ran in
};
BatchStats& batch_stats();   // the calling thread's last batch call (mcvTestBatchStats)
// Throws what cvFindModelBatch refuses a (model, cfg) for, with its message; no device needed.
void batch_check_config(int model, const RansacConfig* cfg);
int64_t batch_cap_essential();   // hypotheses a round of the essential batches may hold (mcvTestBatchCap)
int64_t batch_cap_pnp();         // the same for cvSolvePnPRansacBatch

}  // namespace mcv
