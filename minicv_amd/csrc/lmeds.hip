// lmeds.hip — the rank-k error of every model slot (LMedS, cv::LMEDS = method 4): for each slot the
// exact element of rank `rank` (0-based, ascending in the order of rank_select.h) of its N fp32
// errors, without an N x slots error matrix.
//
// One workgroup per slot. Radix select over the 32-bit order key in three passes (11 + 11 + 10 bits):
// every pass recomputes the N errors (the points stay in L2, an error is a handful of VALU ops),
// histograms the pass's digit of the keys that match the prefix found so far into 2048 LDS bins, and
// wave 0 scans the bins for the digit that holds the rank and the rank inside it.
//
// Clustered errors (inlier errors share a few exponent bins; a degenerate model makes them all equal)
// would serialise same-address LDS atomics lane by lane. A wave therefore pre-aggregates before it
// touches LDS: up to kRankPeel times it takes the digit of its first pending lane, counts the lanes
// that share it with one ballot, and that lane adds the count with one atomic; what is left after the
// peels (lanes spread over many bins, where atomics do not collide) adds 1 each. All-equal errors cost
// one atomic per wave and trip.
#include "mcv_common.h"
#include "hyp_homography.h"
#include "hyp_fundamental.h"
#include "hyp_affine.h"
#include "rank_select.h"
#include "kernels.h"
#include "plan.h"
#include "minicv_native.h"
#include "mcv_runtime.h"
#include <vector>
#include <cstring>

namespace mcv {

static const int kRankPeel = 4;
static const int kRankThreads = 256;

// Error of one correspondence under a slot's model. MODEL 0: homography (HModelF; KIND 0 op-by-op,
// 1 fused); MODEL 1: fundamental (FModelD; KIND = f_error's kinds 0..3); MODEL 4: affine and
// similarity alike (AModelF, the same 6-float model; KIND 0 op-by-op, 1 fused).
template <int MODEL>
struct RankModel;
template <>
struct RankModel<MCV_MODEL_HOMOGRAPHY> {
    typedef HModelF Stored;
    float h[8];
    MCV_HD void load(const Stored& m) {
        for (int j = 0; j < 8; ++j) h[j] = m.h[j];
    }
    template <int KIND>
    MCV_HD float error(float x, float y, float mx, float my) const {
        return KIND ? h_error_fused(h, x, y, mx, my) : h_error(h, x, y, mx, my);
    }
};
template <>
struct RankModel<MCV_MODEL_FUNDAMENTAL> {
    typedef FModelD Stored;
    double f[9];
    MCV_HD void load(const Stored& m) {
        for (int j = 0; j < 9; ++j) f[j] = m.f[j];
    }
    template <int KIND>
    MCV_HD float error(float x1, float y1, float x2, float y2) const {
        return f_error(KIND, f, x1, y1, x2, y2);
    }
};

template <>
struct RankModel<MCV_MODEL_AFFINE> {
    typedef AModelF Stored;
    float f[6];
    MCV_HD void load(const Stored& m) {
        for (int j = 0; j < 6; ++j) f[j] = m.a[j];
    }
    template <int KIND>
    MCV_HD float error(float x, float y, float X, float Y) const {
        return KIND ? a_error_fused(f, x, y, X, Y) : a_error(f, x, y, X, Y);
    }
};

// One wave adds its lanes' digits to the histogram (see the header comment). Every lane of the wave
// calls it; `active` lanes contribute.
__device__ __forceinline__ void rank_hist_add(uint32_t* hist, bool active, uint32_t digit) {
    const int lane = threadIdx.x & 63;
    uint64_t rem = __builtin_amdgcn_ballot_w64(active);
#pragma unroll 1
    for (int r = 0; r < kRankPeel && rem != 0; ++r) {
        const int leader = __builtin_ctzll(rem);
        const uint32_t d0 = (uint32_t)__shfl((int)digit, leader, 64);
        const uint64_t same = __builtin_amdgcn_ballot_w64(active && digit == d0);
        if (lane == leader) atomicAdd(&hist[d0], (uint32_t)__popcll(same));
        active = active && digit != d0;
        rem &= ~same;
    }
    if (active) atomicAdd(&hist[digit], 1u);
}

template <int MODEL, int KIND>
__global__ __launch_bounds__(kRankThreads) void mcv_error_rank(const float4* __restrict__ pts, int N,
                                                               const typename RankModel<MODEL>::Stored* __restrict__ models,
                                                               const int* __restrict__ status, uint32_t rank,
                                                               uint32_t* __restrict__ keys) {
    __shared__ uint32_t hist[kRankBins];
    __shared__ uint32_t sel[2];   // prefix, rank inside it
    const int slot = blockIdx.x;
    if (status && status[slot] < 0) {   // no model: the NaN class, the status stays
        if (threadIdx.x == 0) keys[slot] = kRankKeyNaN;
        return;
    }
    RankModel<MODEL> m;
    m.load(models[slot]);
    const int lane = threadIdx.x & 63;
    uint32_t prefix = 0, r = rank;
#pragma unroll 1
    for (int pass = 0; pass < kRankPasses; ++pass) {
        for (int b = threadIdx.x; b < kRankBins; b += kRankThreads) hist[b] = 0;
        __syncthreads();
        // uniform trip count: every lane reaches the ballots of rank_hist_add
        for (int base = 0; base < N; base += kRankThreads) {
            const int i = base + (int)threadIdx.x;
            const bool v = i < N;
            const float4 q = pts[v ? i : 0];
            const uint32_t key = rank_key(m.template error<KIND>(q.x, q.y, q.z, q.w));
            rank_hist_add(hist, v && rank_in_prefix(key, prefix, pass), rank_digit(key, pass));
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            // lane l owns bins [l per, l per + per); it reads them rotated by l so that the lanes of one
            // read spread over the LDS banks
            const int per = (1 << rank_width(pass)) / 64;
            uint32_t sum = 0;
            for (int j = 0; j < per; ++j) sum += hist[lane * per + ((j + lane) & (per - 1))];
            uint32_t incl = sum;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t t = (uint32_t)__shfl_up((int)incl, off, 64);
                if (lane >= off) incl += t;
            }
            const uint32_t excl = incl - sum;
            if (excl <= r && (r < incl || lane == 63)) {
                uint32_t rr = r - excl;
                const int d = rank_pick(hist, lane * per, lane * per + per, rr);
                sel[0] = (prefix << rank_width(pass)) | (uint32_t)d;
                sel[1] = rr;
            }
        }
        __syncthreads();
        prefix = sel[0];
        r = sel[1];
    }
    if (threadIdx.x == 0) keys[slot] = prefix;
}

template <int MODEL, int KIND>
static void launch_error_rank_k(const float* d_pts4, int N, const void* d_models, const int* d_status, int nSlots,
                                int rank, uint32_t* d_keys, hipStream_t s) {
    hipLaunchKernelGGL((mcv_error_rank<MODEL, KIND>), dim3(nSlots), dim3(kRankThreads), 0, s, (const float4*)d_pts4, N,
                       (const typename RankModel<MODEL>::Stored*)d_models, d_status, (uint32_t)rank, d_keys);
}

// (model, errKind) -> f(RankCase<MODEL, KIND>()): the one place that names the instantiations, for the device
// launch and the host twin alike.
template <int MODEL, int KIND>
struct RankCase {
    static const int model = MODEL, kind = KIND;
};
template <class F>
static void rank_dispatch(int model, int errKind, F f) {
    if (model == MCV_MODEL_HOMOGRAPHY)
        return errKind ? f(RankCase<MCV_MODEL_HOMOGRAPHY, 1>()) : f(RankCase<MCV_MODEL_HOMOGRAPHY, 0>());
    if (affine_family(model)) return errKind ? f(RankCase<MCV_MODEL_AFFINE, 1>()) : f(RankCase<MCV_MODEL_AFFINE, 0>());
    if (model != MCV_MODEL_FUNDAMENTAL) fail("error rank: model %d has no rank kernel", model);
    switch (errKind) {
        case 0: f(RankCase<MCV_MODEL_FUNDAMENTAL, 0>()); break;
        case 1: f(RankCase<MCV_MODEL_FUNDAMENTAL, 1>()); break;
        case 2: f(RankCase<MCV_MODEL_FUNDAMENTAL, 2>()); break;
        case 3: f(RankCase<MCV_MODEL_FUNDAMENTAL, 3>()); break;
        default: fail("error rank: unknown error kind %d", errKind);
    }
}

void launch_error_rank(int model, const float* d_pts4, int N, const void* d_models, const int* d_status, int nSlots,
                       int errKind, int rank, uint32_t* d_keys, hipStream_t s) {
    if (N <= 0 || nSlots <= 0 || rank < 0 || rank >= N) fail("error rank: bad sizes (N=%d, slots=%d, rank=%d)", N, nSlots, rank);
    rank_dispatch(model, errKind, [&](auto c) {
        launch_error_rank_k<decltype(c)::model, decltype(c)::kind>(d_pts4, N, d_models, d_status, nSlots, rank, d_keys, s);
    });
}

static void check_rank_args(const char* who, int model, const float* pts4, int N, const void* models, int nModels,
                            int errKind, int rank, const float* values) {
    if (!pts4 || !models || !values) fail("%s: null argument", who);
    if (model != MCV_MODEL_HOMOGRAPHY && model != MCV_MODEL_FUNDAMENTAL && !affine_family(model))
        fail("%s: model %d has no rank kernel", who, model);
    if (N <= 0 || nModels <= 0 || rank < 0 || rank >= N) fail("%s: bad sizes (N=%d, models=%d, rank=%d)", who, N, nModels, rank);
    if (errKind < 0 || errKind > (model == MCV_MODEL_FUNDAMENTAL ? 3 : 1)) fail("%s: unknown error kind %d", who, errKind);
}

template <int MODEL, int KIND>
static void host_error_rank(const float* pts4, int N, const void* models, int nModels, int rank, float* values) {
    const typename RankModel<MODEL>::Stored* ms = (const typename RankModel<MODEL>::Stored*)models;
    for (int k = 0; k < nModels; ++k) {
        RankModel<MODEL> m;
        m.load(ms[k]);
        auto err = [&](int i) {
            const float* q = pts4 + 4 * (size_t)i;
            return m.template error<KIND>(q[0], q[1], q[2], q[3]);
        };
        values[k] = rank_value(rank_select_host(err, N, (uint32_t)rank));
    }
}

}  // namespace mcv

using namespace mcv;

// Device self-test: the rank kernel on caller-supplied models (H: 8 floats each, errKind = fused 0 / 1;
// F: 9 doubles each, errKind = f_error's kinds 0..3). values[k] = the rank-`rank` error of model k, NaN
// for the NaN class.
extern "C" MCV_API int mcvTestErrorRank(int model, const float* pts4, int N, const void* models, int nModels,
                                        int errKind, int rank, float* values) {
    MCV_GUARD(0, {
        check_rank_args("mcvTestErrorRank", model, pts4, N, models, nModels, errKind, rank, values);
        require_device();
        const size_t mb = model == MCV_MODEL_HOMOGRAPHY ? sizeof(HModelF)
                                                        : (affine_family(model) ? sizeof(AModelF) : sizeof(FModelD));
        DevBuf<float> p;
        DevBuf<uint8_t> m;
        DevBuf<uint32_t> k;
        p.ensure((size_t)N * 4);
        m.ensure((size_t)nModels * mb);
        k.ensure((size_t)nModels);
        MCV_HIP(hipMemcpy(p.p, pts4, (size_t)N * 16, hipMemcpyHostToDevice));
        MCV_HIP(hipMemcpy(m.p, models, (size_t)nModels * mb, hipMemcpyHostToDevice));
        {
            ProfScope ps("lmeds_select", 0);
            launch_error_rank(model, p.p, N, m.p, nullptr, nModels, errKind, rank, k.p, 0);
        }
        MCV_HIP(hipGetLastError());
        std::vector<uint32_t> h((size_t)nModels);
        MCV_HIP(hipMemcpy(h.data(), k.p, (size_t)nModels * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < nModels; ++i) values[i] = rank_value(h[(size_t)i]);
        return 1;
    })
}

// Host twin: the same three passes, sequentially.
extern "C" MCV_API int mcvHostErrorRank(int model, const float* pts4, int N, const void* models, int nModels,
                                        int errKind, int rank, float* values) {
    MCV_GUARD(0, {
        check_rank_args("mcvHostErrorRank", model, pts4, N, models, nModels, errKind, rank, values);
        rank_dispatch(model, errKind, [&](auto c) {
            host_error_rank<decltype(c)::model, decltype(c)::kind>(pts4, N, models, nModels, rank, values);
        });
        return 1;
    })
}
