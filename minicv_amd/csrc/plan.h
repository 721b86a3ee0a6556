// plan.h — device workspace of one RANSAC problem family (homography, fundamental, affine / similarity,
// essential or PnP) on one GPU, and what the shared framework (ransac_host.cpp) and the per-family host
// files declare to each other.
#pragma once

#include "minicv_native.h"
#include "mcv_runtime.h"
#include "mcv_common.h"
#include "ransac_batch_index.h"
#include <stdint.h>
#include <vector>

namespace mcv {

// Host-API chunking of the hypothesis stream for the adaptive (sequential-replay) search.
static const int64_t kChunkFirst = 4096;
static const int64_t kChunkMax = 1 << 20;

size_t model_bytes(int model);   // device model bytes per hypothesis
int model_points(int model);
int model_points_cfg(int model, const RansacConfig& cfg);   // PnP: 5 with the EPnP kernel; F 7-point: 7
int model_slots_cfg(int model, const RansacConfig& cfg);    // F 7-point: 3 model slots per hypothesis
int model_slots(int model);      // model slots per hypothesis (essential: 10)

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
    int kind = -1;            // H: 20 eigen, 21 elimination; F: 10 / 11; E: 30 / 31; PnP: 1 EPnP, 0 AP3P
    void set(int64_t b, int64_t c, const Sampler& smp, const void* p, int n, int k) {
        begin = b; count = c; seed = smp.seed; table = smp.table; pts = p; N = n; kind = k;
    }
    void clear() { *this = LastChunk(); }
    bool covers(int64_t hyp, const Sampler& smp, const void* p, int n, int k) const {
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
size_t point_bytes(int model, int N);   // device point buffer: 16 N (H / F float4), 32 N (E double4, PnP)
// Evaluate side: P.last = this chunk, and the fingerprint of its points -> P.fp[0] (async).
void mark_chunk(Plan& P, int64_t begin, int64_t count, const Sampler& smp, const void* d_pts, int N, int kind,
                hipStream_t s);
// Finalize side, on the cached-model path: the current points' fingerprint -> P.fp[1], both to
// P.h_fp (async; chunk_fresh reads them after the caller's next stream synchronisation).
void queue_chunk_check(Plan& P, const void* d_pts, int N, hipStream_t s);
inline bool chunk_fresh(const Plan& P) { return P.h_fp.p[0] == P.h_fp.p[1]; }
// The device points' fingerprint, synchronously (CV-sampler table checks).
uint64_t device_fingerprint(Plan& P, const void* d_pts, int N, hipStream_t s);
double effective_threshold(const RansacConfig& cfg);
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
RansacConfig config_or_default(const RansacConfig* cfg);
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

// Per family: *_generate_chunk = one chunk's models, statuses and P.last (shared by the RANSAC evaluate and
// lmeds_search); *_evaluate_chunk = generate + verify into d_counts; *_finalize = the winner's model and mask.

// homography family (ransac_h_*.hip / ransac_h_host.cpp)
void h_generate_chunk(Plan& P, const float* d_pts, int N, const RansacConfig& cfg, int64_t hypBegin, int hypCount,
                      int* d_counts, hipStream_t s, bool certifiedRow = false);
// keyOnly: nobody reads d_counts beyond the best-key reduction, so the sweep may run in self-pruning stages
void h_evaluate_chunk(Plan& P, const float* d_pts, int N, const RansacConfig& cfg, int64_t hypBegin, int hypCount,
                      int* d_counts, bool keyOnly, hipStream_t s);
int h_finalize(Plan& P, const float* d_pts, int N, const RansacConfig& cfg, int64_t hyp, double* H, uint8_t* d_mask,
               hipStream_t s);
int h_host_hypothesis(const float* pts4, int N, uint64_t seed, int64_t hyp, double* model9, float* modelf9,
                      int* sampleIdx, bool fast);
// runKernel's host half on one refit record (kernels.h kRefit*) -> H; false: degenerate, H is not a model
bool h_refit_from_record(const double* r, double* H);
void h_plan_forget(const Plan* P);   // ~Plan: drops the test hooks' references to the plan

// fundamental-matrix family (ransac_f.hip / ransac_f_host.cpp)
bool f_seven(int model, const RansacConfig& cfg);   // fundamental with MCV_FLAG_SEVEN_POINT
int f_error_kind(const RansacConfig& cfg);
void f_generate_chunk(Plan& P, const float* d_pts, int N, const RansacConfig& cfg, int64_t hypBegin, int hypCount,
                      int* d_counts, hipStream_t s);
void f_evaluate_chunk(Plan& P, const float* d_pts, int N, const RansacConfig& cfg, int64_t hypBegin, int hypCount,
                      int* d_counts, hipStream_t s);
int f_finalize(Plan& P, const float* d_pts, int N, const RansacConfig& cfg, int64_t hyp, double* F, uint8_t* d_mask,
               hipStream_t s);
int f_fit_all(Plan& P, const float* d_pts, int N, hipStream_t s, double* F);
int f_host_hypothesis(const float* pts4, int N, uint64_t seed, int64_t hyp, double* F9, float* Ff9, int* sampleIdx,
                      bool fast);

// affine / similarity family (ransac_a.hip / ransac_a_host.cpp)
inline bool affine_family(int model) { return model == MCV_MODEL_AFFINE || model == MCV_MODEL_SIMILARITY; }
void a_generate_chunk(Plan& P, const float* d_pts, int N, const RansacConfig& cfg, int64_t hypBegin, int hypCount,
                      int* d_counts, hipStream_t s);
void a_evaluate_chunk(Plan& P, const float* d_pts, int N, const RansacConfig& cfg, int64_t hypBegin, int hypCount,
                      int* d_counts, hipStream_t s);
int a_host_hypothesis(int model, const float* pts4, int N, uint64_t seed, int64_t hyp, double* model9, float* modelf9,
                      int* sampleIdx);
int a_finalize(Plan& P, const float* d_pts, int N, const RansacConfig& cfg, int64_t hyp, double* model9,
               uint8_t* d_mask, hipStream_t s);

// PnP family (ransac_pnp.hip / pnp_host.cpp)
void p_evaluate_chunk(Plan& P, const void* d_pts, int N, const RansacConfig& cfg, int64_t hypBegin, int hypCount,
                      int* d_counts, hipStream_t s);
int p_finalize(Plan& P, const void* d_pts, int N, const RansacConfig& cfg, int64_t hyp, double* model9,
               uint8_t* d_mask, hipStream_t s);
bool pnp_cfg_epnp(const RansacConfig& cfg);   // minimal sets of 5 for EPnP (solverKind 0/1/3/4)
// cvSolvePnPRansac's configuration: OpenCV's sample stream, RANSAC, the given budget / threshold / kind
RansacConfig pnp_config(int iters, float thr, double conf, int kind);

// essential-matrix family (ransac_e.hip / ransac_e_host.cpp)
void e_evaluate_chunk(Plan& P, const double* d_pts, int N, const RansacConfig& cfg, int64_t hypBegin, int hypCount,
                      int* d_counts, hipStream_t s);
int e_finalize(Plan& P, const double* d_pts, int N, const RansacConfig& cfg, int64_t slot, double* E,
               uint8_t* d_mask, hipStream_t s);
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
struct BatchStats {
    long long launches = 0, syncs = 0, rounds = 0, lmRounds = 0, single = 0, problems = 0;
    long long packUs = 0, tableUs = 0;   // host time: point conversion, OpenCV sample tables
    long long problemRounds = 0;         // problems summed over the hypothesis rounds they ran in
    long long copies = 0;                // host <-> device copies enqueued (every family; memsets are not counted)
};
BatchStats& batch_stats();   // the calling thread's last batch call (mcvTestBatchStats)
// Throws what cvFindModelBatch refuses a (model, cfg) for, with its message; no device needed.
void batch_check_config(int model, const RansacConfig* cfg);
int64_t batch_cap_essential();   // hypotheses a round of the essential batches may hold (mcvTestBatchCap)
int64_t batch_cap_pnp();         // the same for cvSolvePnPRansacBatch

}  // namespace mcv
