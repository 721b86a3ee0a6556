// ransac_host.cpp — the RANSAC framework every model family shares, behind the C-ABI: OpenCV's
// sequential replay (adaptive niters), the Plan workspace, the chunked search over one or several
// devices (ransac_search: generate + verify on the GPU per chunk, counts or the best key back, replay on
// the host), LMedS (lmeds_search) and the device-level mcvRansacEvaluate / mcvRansacFinalize.
// What a chunk's evaluate and a winner's finalize do is each family's own (ransac_h_host.cpp,
// ransac_f_host.cpp, ransac_a_host.cpp, ransac_e_host.cpp, pnp_host.cpp): one table row each (kFamilies), and
// the 2-D exports' common entry (find_model_2d).
#include "minicv_native.h"
#include "mcv_runtime.h"
#include "kernels.h"
#include "mcv_common.h"
#include "plan.h"
#include "rank_select.h"

#include <cmath>
#include <cfloat>
#include <cstring>
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
// The family table (plan.h): one row per MCV_MODEL_*. Columns: shape | reserve, generate, evaluate, finalize,
// host_hypothesis | points_cfg, slots_cfg | lsq, entry_refuse, entry_direct.
static const RansacFamily kFamilies[] = {
    {kFamilyShapes[MCV_MODEL_HOMOGRAPHY], nullptr, h_generate, h_evaluate, h_finalize, h_host_hypothesis,
     nullptr, nullptr, true, nullptr, h_entry_direct},
    {kFamilyShapes[MCV_MODEL_FUNDAMENTAL], nullptr, f_generate, f_evaluate, f_finalize, f_host_hypothesis,
     f_points_cfg, f_slots_cfg, true, f_entry_refuse, f_entry_direct},
    {kFamilyShapes[MCV_MODEL_ESSENTIAL], e_reserve, nullptr, e_evaluate, e_finalize, nullptr,
     nullptr, nullptr, false, nullptr, nullptr},
    {kFamilyShapes[MCV_MODEL_PNP], nullptr, nullptr, p_evaluate, p_finalize, nullptr,
     p_points_cfg, nullptr, false, nullptr, nullptr},
    {kFamilyShapes[MCV_MODEL_AFFINE], nullptr, a_generate, a_evaluate, a_finalize, a_host_hypothesis,
     nullptr, nullptr, false, nullptr, a_entry_direct},
    {kFamilyShapes[MCV_MODEL_SIMILARITY], nullptr, a_generate, a_evaluate, a_finalize, a_host_hypothesis,
     nullptr, nullptr, false, nullptr, a_entry_direct},
};
// a row's sample size, model slots, device model bytes and bytes per point
constexpr bool shape_is(int model, int points, int slots, int modelBytes, int pointBytes) {
    return kFamilyShapes[model].points == points && kFamilyShapes[model].slots == slots &&
           kFamilyShapes[model].modelBytes == modelBytes && (kFamilyShapes[model].doublePoints ? 32 : 16) == pointBytes;
}
static_assert(sizeof(kFamilyShapes) / sizeof(kFamilyShapes[0]) == MCV_MODEL_SIMILARITY + 1, "one row per model");
static_assert(shape_is(MCV_MODEL_HOMOGRAPHY, 4, 1, 32, 16), "homography row");
static_assert(shape_is(MCV_MODEL_FUNDAMENTAL, 8, 1, 80, 16), "fundamental row");
static_assert(shape_is(MCV_MODEL_ESSENTIAL, 5, kEModelSlots, 72 * kEModelSlots, 32), "essential row");
static_assert(shape_is(MCV_MODEL_PNP, 4, 1, 96, 32), "PnP row");
static_assert(shape_is(MCV_MODEL_AFFINE, 3, 1, 24, 16), "affine row");
static_assert(shape_is(MCV_MODEL_SIMILARITY, 2, 1, 24, 16), "similarity row");

const RansacFamily& family_of(int model) {
    if (model < MCV_MODEL_HOMOGRAPHY || model > MCV_MODEL_SIMILARITY) fail("unknown model %d", model);
    return kFamilies[model];
}
size_t model_bytes(int model) { return (size_t)family_of(model).modelBytes; }
int model_slots(int model) { return family_of(model).slots; }
int model_points(int model) { return family_of(model).points; }
int model_slots_cfg(int model, const RansacConfig& cfg) {
    const RansacFamily& f = family_of(model);
    return f.slots_cfg ? f.slots_cfg(cfg) : f.slots;
}
int model_points_cfg(int model, const RansacConfig& cfg) {
    const RansacFamily& f = family_of(model);
    return f.points_cfg ? f.points_cfg(cfg) : f.points;
}
size_t point_bytes(int model, int N) { return (size_t)N * (family_of(model).doublePoints ? 32 : 16); }

void Plan::reserve(int n, int64_t hyps) {
    if (n > maxN) maxN = n;
    if (hyps > maxHyps) maxHyps = hyps;
    const RansacFamily& f = family_of(model);
    if (f.doublePoints) {
        ptsd.ensure((size_t)maxN * 4);
        raw.ensure((size_t)maxN * 4);
    } else {
        pts.ensure((size_t)maxN * 4);
    }
    if (f.reserve) f.reserve(*this);
    models.ensure((size_t)maxHyps * f.modelBytes);
    if (f.h64PerHyp) h64.ensure((size_t)maxHyps * f.h64PerHyp);
    counts.ensure((size_t)maxHyps * f.slots);
    pkey.ensure(512);
    pfail.ensure(512);
    key.ensure(2);
    part.ensure((size_t)kReduceMaxBlocksHost * 64);
    red.ensure(64);
    mask.ensure((size_t)maxN);
    count.ensure(1);
    bbox.ensure(4);
    one.ensure(512);
    h_counts.ensure((size_t)maxHyps * f.slots);
    h_red.ensure(64);
    if (!f.doublePoints) h_pack.ensure((size_t)maxN * 4);
    one.ensure(sizeof(EOneOut));
    h_one.ensure(sizeof(EOneOut));
    h_i.ensure(4);
}

hipStream_t Plan::own_stream() {
    if (!stream) MCV_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    return stream;
}

Plan::~Plan() {
    h_plan_forget(this);
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

void mark_chunk(Plan& P, int64_t begin, int64_t count, const Sampler& smp, const void* d_pts, int N,
                ChunkSolver kind, hipStream_t s) {
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
    pack_float4(a, b, N, P.h_pack.p);
    MCV_HIP(hipMemcpyAsync(d_dst, P.h_pack.p, (size_t)N * 16, hipMemcpyHostToDevice, s));
    MCV_HIP(hipStreamSynchronize(s));
}

double effective_threshold(const RansacConfig& cfg) { return cfg.threshold > 0 ? cfg.threshold : 3.0; }
bool fused_error(const RansacConfig& cfg) { return (cfg.flags & MCV_FLAG_FUSED_ERROR) != 0; }
bool fast_minimal(const RansacConfig& cfg) { return (cfg.flags & MCV_FLAG_FAST_MINIMAL) != 0; }

// Evaluate one chunk of hypotheses on the device (generate + verify [+ best key]).
void evaluate_chunk(Plan& P, const void* d_pts, int N, const RansacConfig& cfg, int64_t hypBegin, int hypCount,
                    int* d_counts, uint64_t* d_key, hipStream_t s, bool needCounts) {
    family_of(P.model).evaluate(P, d_pts, N, cfg, hypBegin, hypCount, d_counts, d_key != nullptr && !needCounts, s);
    // the chunk's best key and first sampler failure over all its model slots
    const int slots = model_slots_cfg(P.model, cfg);
    if (d_key)
        launch_best(d_counts, hypCount * slots, hypBegin * slots, model_points_cfg(P.model, cfg), P.pkey.p, P.pfail.p,
                    d_key, s);
    MCV_HIP(hipGetLastError());
}

int finalize(Plan& P, const void* d_pts, int N, const RansacConfig& cfg, int64_t hyp, double* model9,
             uint8_t* d_mask, hipStream_t s) {
    return family_of(P.model).finalize(P, d_pts, N, cfg, hyp, model9, d_mask, s);
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
        if (!h_pts4 && !family_of(P.model).doublePoints) {   // cv_table_build reads host float4 points
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
        const size_t bytes = point_bytes(P.model, N);
        MCV_HIP(hipStreamSynchronize(s));
        for (int k = 1; k < shards; ++k) {
            const int dev = (home + k) % ndev;
            MCV_HIP(hipSetDevice(dev));
            Plan& Pk = thread_plan(P.model, k);
            Pk.reserve(N, slotScale);
            std::memcpy(Pk.pnpCam, P.pnpCam, sizeof(P.pnpCam));
            void* dst = family_of(P.model).doublePoints ? (void*)Pk.ptsd.p : (void*)Pk.pts.p;
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
    // the rank kernel's error kinds are its own numbering, not a family hook: the fundamental matrix has four
    // (f_error_kind), the other families op-by-op 0 / fused 1
    const int errKind = P.model == MCV_MODEL_FUNDAMENTAL ? f_error_kind(cfg) : (fused_error(cfg) ? 1 : 0);
    // the whole budget as one chunk, by the generate the family's RANSAC evaluate calls
    GenerateHook* generate = family_of(P.model).generate;
    if (!generate) fail("LMedS: model %d has no rank kernel", P.model);
    generate(P, d_pts, N, cfg, 0, cnt, P.counts.p, s);
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

RansacConfig config_or_default(int model, const RansacConfig* cfg) {
    if (cfg) return *cfg;
    RansacConfig c;
    std::memset(&c, 0, sizeof(c));
    c.threshold = 3.0;
    c.confidence = family_of(model).defaultConfidence;
    c.maxIters = 2000;
    c.method = MCV_METHOD_RANSAC;
    c.flags = MCV_FLAG_CV_SAMPLER;   // no seed given: OpenCV's own sample stream
    return c;
}

int find_model_2d(int model, const char* who, const mcvV2d* a, const mcvV2d* b, int N, const RansacConfig* cfgp,
                  double* model9, uint8_t* mask) {
    const RansacFamily& f = family_of(model);
    if (!a || !b || !model9 || N < 0) fail("%s: null argument or negative N", who);
    if (mask) std::memset(mask, 0, (size_t)N);
    if (!f.entry_refuse && N < f.points) fail("%s: need at least %d correspondences (N=%d)", who, f.points, N);
    const RansacConfig cfg = config_or_default(model, cfgp);
    check_flags(cfg, who);
    if (f.entry_refuse) f.entry_refuse(who, N, cfg);
    if (cfg.method != MCV_METHOD_RANSAC && cfg.method != MCV_METHOD_LMEDS && !(f.lsq && cfg.method == MCV_METHOD_LSQ))
        fail("%s: unsupported method %d", who, cfg.method);
    if (cfg.method != MCV_METHOD_LSQ && !(cfg.confidence > 0 && cfg.confidence < 1))
        fail("%s: confidence must be in (0,1)", who);
    require_device();
    Plan& P = thread_plan(model);
    hipStream_t s = P.own_stream();
    P.reserve(N, 1);
    pack_points(P, a, b, N, P.pts.p, s);
    double M[9];
    int count = N;
    if (f.entry_direct(P, who, N, cfg, s, M)) {
        if (mask) std::memset(mask, 1, (size_t)N);
    } else {
        const int m = model_points_cfg(model, cfg);
        RansacConfig fin = cfg;   // LMedS: the winner's mask comes from the finalize with LMedS' own threshold
        int64_t best;
        if (cfg.method == MCV_METHOD_LMEDS) {
            best = lmeds_search(P, P.pts.p, N, cfg, s, P.h_pack.p, &fin.threshold);
        } else {
            best = ransac_search(P, P.pts.p, N, cfg, s, P.h_pack.p);
            if (best < 0) fail("%s: RANSAC found no model with >= %d inliers", who, m);
        }
        count = f.finalize(P, P.pts.p, N, fin, best, M, P.mask.p, s);
        if (cfg.method == MCV_METHOD_LMEDS && count < m) fail("%s: LMedS model has %d inliers (< %d)", who, count, m);
        mask_to_host(P, mask, N, s);
    }
    for (int k = 0; k < 9; ++k) model9[k] = M[k];
    return count;
}

}  // namespace mcv

// ------------------------------------------------------------------------------------------
// Exports
// ------------------------------------------------------------------------------------------
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
        HostHypothesisHook* twin = family_of(model).host_hypothesis;
        if (!twin) fail("mcvHostHypothesis: the %s family has no host twin here", family_of(model).name);
        return twin(model, pts4, N, seed, hyp, model9, modelf9, sampleIdx, fast);
    })
}

extern "C" MCV_API void mcvHostPhilox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                      uint32_t* out4) {
    U4 c;
    c.x = c0; c.y = c1; c.z = c2; c.w = c3;
    const U4 r = philox4x32_10(c, k0, k1);
    out4[0] = r.x; out4[1] = r.y; out4[2] = r.z; out4[3] = r.w;
}
