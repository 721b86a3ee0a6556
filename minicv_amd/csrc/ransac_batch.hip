// ransac_batch.hip — gfx950 kernels of cvFindModelBatch: B independent RANSAC problems of one model family
// (homography, 8-point fundamental, affine, similarity) in launches whose number does not depend on B.
// All problems' float4 correspondences sit in one segmented buffer; a descriptor table (BatchDesc) names
// each problem's slice, its hypotheses of the round, its slots and its sampler rows. Every kernel indexes
// the grid as (block within problem, problem).
//
//   mcv_batch_generate<MODEL>  one lane per (problem, hypothesis): the single call's per-hypothesis code
//                              (h_hypothesis / f_hypothesis / a_hypothesis<M>, one-pass solvers) -> the
//                              sweep's model + status, as the single generate kernels store them.
//   mcv_batch_sweep<MODEL, K>  the inlier sweep, transposed against the single call's: a workgroup
//                              belongs to one problem, each LANE holds one hypothesis' model in registers,
//                              the problem's points are staged through LDS in tiles of kBatchTile, and
//                              every lane walks the tile reading the same address (an LDS broadcast: no
//                              bank conflict) and counts in a register — no ballot, no atomics. The single
//                              sweeps put points on lanes and models in SGPRs, which is right for 100k
//                              points and leaves most of a wave idle at N = 100. The error is the defining
//                              function itself (h_error with its IEEE division, f_error, a_error), so each
//                              count is by construction the number of points with error <= thr2 (NaN: no).
//   mcv_batch_one<MODEL>       one lane per finishing problem: the winner re-solved in full (fp64 model,
//                              fp32 model, status) by the same code.
//   mcv_batch_mask<MODEL, K>   every winner's inlier mask and count in one launch.
//   mcv_batch_reduce_*         reduce.h's two-stage fixed-order reduction over many problems at once:
//                              problem r's partials are those of reduce_blocks(N_r) blocks of 256 threads
//                              strided by its own grid, reduced by block_sum and summed in block order by
//                              reduce_final's pattern, over the per-point terms the single call's functors
//                              use (a_lm_terms, h_refine_terms.h) — the single call's sums bit for bit.
#include <algorithm>
#include "mcv_common.h"
#include "hyp_homography.h"
#include "hyp_fundamental.h"
#include "hyp_affine.h"
#include "h_refine_terms.h"
#include "jacobi_eig.h"
#include "reduce.h"
#include "kernels.h"
#include "minicv_native.h"

namespace mcv {

// ---- per-model traits: the sweep's model record, the sample size, the error
template <int MODEL> struct BatchModel;
template <> struct BatchModel<MCV_MODEL_HOMOGRAPHY> {
    typedef HModelF Rec;
    static constexpr bool kEig = true;
    template <int KIND>
    static __device__ __forceinline__ float error(const Rec& m, const float4& q) {
        return h_error(m.h, q.x, q.y, q.z, q.w);
    }
};
template <> struct BatchModel<MCV_MODEL_FUNDAMENTAL> {
    typedef FModelD Rec;
    static constexpr bool kEig = true;
    template <int KIND>
    static __device__ __forceinline__ float error(const Rec& m, const float4& q) {
        return f_error(KIND, m.f, q.x, q.y, q.z, q.w);
    }
};
template <> struct BatchModel<MCV_MODEL_AFFINE> {
    typedef AModelF Rec;
    static constexpr bool kEig = false;
    template <int KIND>
    static __device__ __forceinline__ float error(const Rec& m, const float4& q) {
        return a_error(m.a, q.x, q.y, q.z, q.w);
    }
};
template <> struct BatchModel<MCV_MODEL_SIMILARITY> : BatchModel<MCV_MODEL_AFFINE> {};

// One hypothesis of problem d through the single call's code. ws: the eigen-solve's LDS slice (H / F).
template <int MODEL, class WS>
__device__ __forceinline__ int batch_hypothesis(const float* pts4, int N, const Sampler& smp, uint64_t hyp,
                                                double* M9, typename BatchModel<MODEL>::Rec* rec, WS& ws) {
    if constexpr (MODEL == MCV_MODEL_HOMOGRAPHY) {
        return h_hypothesis(pts4, N, smp, hyp, M9, rec, nullptr, ws);
    } else if constexpr (MODEL == MCV_MODEL_FUNDAMENTAL) {
        const int st = f_hypothesis(pts4, N, smp, hyp, M9, nullptr, ws);
#pragma unroll
        for (int j = 0; j < 9; ++j) rec->f[j] = M9[j];
        return st;
    } else {
        constexpr int M = MODEL == MCV_MODEL_AFFINE ? 3 : 2;
        return a_hypothesis<M>(pts4, N, smp, hyp, M9, rec, nullptr);
    }
}

// The model a slot without one carries (its count is never written): the single generates' zero model
// (H, affine) or dummy model (F).
template <int MODEL>
__device__ __forceinline__ void batch_no_model(typename BatchModel<MODEL>::Rec* rec) {
    if constexpr (MODEL == MCV_MODEL_HOMOGRAPHY) {
#pragma unroll
        for (int j = 0; j < 8; ++j) rec->h[j] = 0.f;
    } else if constexpr (MODEL == MCV_MODEL_FUNDAMENTAL) {
#pragma unroll
        for (int j = 0; j < 9; ++j) rec->f[j] = f_dummy_model(j);
    } else {
#pragma unroll
        for (int j = 0; j < 6; ++j) rec->a[j] = 0.f;
    }
}

template <int MODEL>
static constexpr int batch_gen_lanes() { return BatchModel<MODEL>::kEig ? kEigLanes : 256; }

template <int MODEL>
static constexpr int batch_sample_size() {
    return MODEL == MCV_MODEL_HOMOGRAPHY ? 4 : MODEL == MCV_MODEL_FUNDAMENTAL ? 8 : MODEL == MCV_MODEL_AFFINE ? 3 : 2;
}

template <int MODEL>
__device__ __forceinline__ Sampler batch_sampler(uint64_t seed, const int* table, int64_t rowOff) {
    Sampler smp;
    smp.seed = seed;
    smp.table = table ? table + rowOff * batch_sample_size<MODEL>() : nullptr;
    return smp;
}

// ------------------------------------------------------------------------------------------
// Generate. Grid: blocksPer x nDesc blocks of batch_gen_lanes<MODEL>() lanes.
// ------------------------------------------------------------------------------------------
template <int MODEL>
__global__ __launch_bounds__(batch_gen_lanes<MODEL>()) void mcv_batch_generate(
    const float* __restrict__ pts4, const BatchDesc* __restrict__ desc, int blocksPer, uint64_t seed,
    const int* __restrict__ table, typename BatchModel<MODEL>::Rec* __restrict__ models, int* __restrict__ counts) {
    constexpr int L = batch_gen_lanes<MODEL>();
    const BatchDesc D = desc[blockIdx.x / blocksPer];
    const int i = (blockIdx.x % blocksPer) * L + threadIdx.x;
    if (i >= D.hypCount) return;
    const float* p = pts4 + 4 * (int64_t)D.ptOff;
    const Sampler smp = batch_sampler<MODEL>(seed, table, D.rowOff);
    double M9[9];
    typename BatchModel<MODEL>::Rec rec;
    int st;
    if constexpr (BatchModel<MODEL>::kEig) {
        __shared__ double lds[kEigWs * L];
        EigWsLane ws{lds + threadIdx.x * kEigWs};
        st = batch_hypothesis<MODEL>(p, D.N, smp, (uint64_t)(D.hypBegin + i), M9, &rec, ws);
    } else {
        EigWsLocal unused;
        st = batch_hypothesis<MODEL>(p, D.N, smp, (uint64_t)(D.hypBegin + i), M9, &rec, unused);
    }
    if (st != 1) batch_no_model<MODEL>(&rec);
    models[D.slotOff + i] = rec;
    counts[D.slotOff + i] = st == 1 ? 0 : st;
}

// ------------------------------------------------------------------------------------------
// Inlier sweep: lanes = hypotheses, points broadcast from LDS. Grid: blocksPer x nDesc blocks of 256.
// kBatchTile float4 points = 16 KiB of LDS per workgroup: eight workgroups (the CU's 32 waves) take
// 128 KiB of the 160 KiB, so LDS never lowers the occupancy below what the registers allow.
// ------------------------------------------------------------------------------------------
template <int MODEL, int KIND>
__global__ __launch_bounds__(256) void mcv_batch_sweep(const float4* __restrict__ pts,
                                                       const BatchDesc* __restrict__ desc, int blocksPer,
                                                       const typename BatchModel<MODEL>::Rec* __restrict__ models,
                                                       int* __restrict__ counts, float thr2) {
    __shared__ float4 tile[kBatchTile];
    const BatchDesc D = desc[blockIdx.x / blocksPer];
    const int i0 = (blockIdx.x % blocksPer) * 256;
    if (i0 >= D.hypCount) return;   // uniform over the workgroup
    const int i = i0 + threadIdx.x;
    const bool mine = i < D.hypCount;
    // lanes past the problem's hypotheses re-read its last slot and write nothing
    const int64_t slot = D.slotOff + (mine ? i : D.hypCount - 1);
    const typename BatchModel<MODEL>::Rec m = models[slot];
    const bool valid = mine && counts[slot] >= 0;
    const float4* p = pts + D.ptOff;
    int cnt = 0;
    for (int base = 0; base < D.N; base += kBatchTile) {
        const int n = min(kBatchTile, D.N - base);
        if (base) __syncthreads();   // the previous tile has been read by every lane
        for (int j = threadIdx.x; j < n; j += 256) tile[j] = p[base + j];
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const float4 q = tile[j];
            cnt += BatchModel<MODEL>::template error<KIND>(m, q) <= thr2 ? 1 : 0;
        }
    }
    if (valid) counts[slot] = cnt;
}

// ------------------------------------------------------------------------------------------
// Winners: re-solve (one lane per finishing problem), then mask + count.
// ------------------------------------------------------------------------------------------
template <int MODEL>
__global__ __launch_bounds__(batch_gen_lanes<MODEL>()) void mcv_batch_one(const float* __restrict__ pts4,
                                                                          const BatchFin* __restrict__ fin, int nFin,
                                                                          uint64_t seed, const int* __restrict__ table,
                                                                          BatchOne* __restrict__ out) {
    constexpr int L = batch_gen_lanes<MODEL>();
    const int f = blockIdx.x * L + threadIdx.x;
    if (f >= nFin) return;
    const BatchFin D = fin[f];
    const float* p = pts4 + 4 * (int64_t)D.ptOff;
    const Sampler smp = batch_sampler<MODEL>(seed, table, D.rowOff);
    BatchOne o;
    typename BatchModel<MODEL>::Rec rec;
    for (int j = 0; j < 9; ++j) o.M[j] = 0;
    for (int j = 0; j < 8; ++j) o.f[j] = 0;
    batch_no_model<MODEL>(&rec);
    if constexpr (BatchModel<MODEL>::kEig) {
        __shared__ double lds[kEigWs * L];
        EigWsLane ws{lds + threadIdx.x * kEigWs};
        o.status = batch_hypothesis<MODEL>(p, D.N, smp, (uint64_t)D.hyp, o.M, &rec, ws);
    } else {
        EigWsLocal unused;
        o.status = batch_hypothesis<MODEL>(p, D.N, smp, (uint64_t)D.hyp, o.M, &rec, unused);
    }
    if constexpr (MODEL == MCV_MODEL_HOMOGRAPHY) {
        for (int j = 0; j < 8; ++j) o.f[j] = rec.h[j];
    } else if constexpr (MODEL != MCV_MODEL_FUNDAMENTAL) {
        for (int j = 0; j < 6; ++j) o.f[j] = rec.a[j];
    }
    o.pad = 0;
    out[f] = o;
}

// Grid: blocksPer x nFin blocks of 256; block b of problem f masks points [256 b, 256 b + 256).
template <int MODEL, int KIND>
__global__ __launch_bounds__(256) void mcv_batch_mask(const float4* __restrict__ pts, const BatchFin* __restrict__ fin,
                                                      int blocksPer, const BatchOne* __restrict__ one, float thr2,
                                                      uint8_t* __restrict__ mask, int* __restrict__ count) {
    const int f = blockIdx.x / blocksPer;
    const BatchFin D = fin[f];
    const int i = (blockIdx.x % blocksPer) * 256 + threadIdx.x;
    if ((blockIdx.x % blocksPer) * 256 >= D.N || one[f].status != 1) return;   // uniform over the workgroup
    typename BatchModel<MODEL>::Rec m;
    if constexpr (MODEL == MCV_MODEL_HOMOGRAPHY) {
#pragma unroll
        for (int j = 0; j < 8; ++j) m.h[j] = one[f].f[j];
    } else if constexpr (MODEL == MCV_MODEL_FUNDAMENTAL) {
#pragma unroll
        for (int j = 0; j < 9; ++j) m.f[j] = one[f].M[j];
    } else {
#pragma unroll
        for (int j = 0; j < 6; ++j) m.a[j] = one[f].f[j];
    }
    bool in = false;
    if (i < D.N) {
        const float4 q = pts[D.ptOff + i];
        in = BatchModel<MODEL>::template error<KIND>(m, q) <= thr2;
        mask[D.ptOff + i] = in ? 1 : 0;
    }
    const uint64_t b = __ballot(in);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(count + f, (int)__popcll(b));
}

// ------------------------------------------------------------------------------------------
// Batched fixed-order reductions. Grid of the pass: blocksPer x nRed blocks of kReduceThreads
// (blocksPer = reduce_blocks(largest N)); the blocks past a problem's own reduce_blocks(N_r) leave.
// ------------------------------------------------------------------------------------------
// Op: init(pts, mask, par) once per thread, then operator()(i, acc) as reduce.h's functors.
template <int V, class Op>
__global__ __launch_bounds__(kReduceThreads) void mcv_batch_reduce_pass(const float4* __restrict__ pts,
                                                                        const uint8_t* __restrict__ mask,
                                                                        const BatchRed* __restrict__ red,
                                                                        int blocksPer, const double* __restrict__ par,
                                                                        int parStride, double* __restrict__ partials) {
    const int r = blockIdx.x / blocksPer, b = blockIdx.x % blocksPer;
    const BatchRed D = red[r];
    const int nb = reduce_blocks(D.N);
    if (b >= nb) return;   // uniform over the workgroup
    Op op;
    op.init(pts + D.ptOff, mask + D.ptOff, par + (int64_t)r * parStride);
    double acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0;
    for (int i = b * kReduceThreads + threadIdx.x; i < D.N; i += nb * kReduceThreads) op(i, acc);
    block_sum<V>(acc, partials + ((size_t)r * blocksPer + b) * V);
}

template <int V>
__global__ __launch_bounds__(kReduceThreads) void mcv_batch_reduce_final(const BatchRed* __restrict__ red,
                                                                         int blocksPer,
                                                                         const double* __restrict__ partials,
                                                                         double* __restrict__ out, int outStride) {
    const int r = blockIdx.x;
    const int nb = reduce_blocks(red[r].N);
    const double* part = partials + (size_t)r * blocksPer * V;
    double acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0;
    for (int b = threadIdx.x; b < nb; b += kReduceThreads) {
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] += part[(size_t)b * V + v];
    }
    block_sum<V>(acc, out + (size_t)r * outStride);
}

// The functors of the single call's refine passes (ransac_a.hip OpALM; ransac_h_refine.hip OpSums, OpAbsDev,
// OpLtL, OpLM) over the same per-point terms (a_lm_terms, h_refine_terms.h): here the constants come from the
// problem's parameter row and the mask is always present.
template <int LX>
struct BOpALM {
    const float4* pts; const uint8_t* mask; double h[LX];
    __device__ void init(const float4* p, const uint8_t* m, const double* par) {
        pts = p; mask = m;
#pragma unroll
        for (int j = 0; j < LX; ++j) h[j] = par[j];
    }
    __device__ void operator()(int i, double (&a)[a_lm_values(LX)]) const {
        if (!mask[i]) return;
        const float4 q = pts[i];
        a_lm_terms<LX>(h, (double)q.x, (double)q.y, (double)q.z, (double)q.w, a);
    }
};
struct BOpSums {   // 5: sum dst.x, dst.y, src.x, src.y, count
    const float4* pts; const uint8_t* mask;
    __device__ void init(const float4* p, const uint8_t* m, const double*) { pts = p; mask = m; }
    __device__ void operator()(int i, double (&a)[5]) const {
        if (!mask[i]) return;
        const float4 q = pts[i];
        h_sums_terms((double)q.x, (double)q.y, (double)q.z, (double)q.w, a);
    }
};
struct BOpAbsDev {  // 4: sum |dst - cm|, |src - cM|; par = the problem's refit record
    const float4* pts; const uint8_t* mask; const double* c4;
    __device__ void init(const float4* p, const uint8_t* m, const double* par) {
        pts = p; mask = m; c4 = par + kRefitC4;
    }
    __device__ void operator()(int i, double (&a)[4]) const {
        if (!mask[i]) return;
        const float4 q = pts[i];
        h_absdev_terms(c4, (double)q.x, (double)q.y, (double)q.z, (double)q.w, a);
    }
};
struct BOpLtL {     // 45: upper triangle of LtL; par = the problem's refit record
    const float4* pts; const uint8_t* mask; const double* c4; const double* s4;
    __device__ void init(const float4* p, const uint8_t* m, const double* par) {
        pts = p; mask = m; c4 = par + kRefitC4; s4 = par + kRefitS4;
    }
    __device__ void operator()(int i, double (&a)[45]) const {
        if (!mask[i]) return;
        const float4 q = pts[i];
        h_ltl_terms(c4, s4, (double)q.x, (double)q.y, (double)q.z, (double)q.w, a);
    }
};
struct BOpHLM {     // 45: JtJ upper triangle (36), Jtr (8), |r|^2 (1)
    const float4* pts; const uint8_t* mask; double h[8];
    __device__ void init(const float4* p, const uint8_t* m, const double* par) {
        pts = p; mask = m;
#pragma unroll
        for (int j = 0; j < 8; ++j) h[j] = par[j];
    }
    __device__ void operator()(int i, double (&a)[45]) const {
        if (!mask[i]) return;
        const float4 q = pts[i];
        h_lm_terms(h, (double)q.x, (double)q.y, (double)q.z, (double)q.w, a);
    }
};

// The step between the chained passes (h_refine_terms.h) on every problem's record: 4 lanes per record.
__global__ void mcv_batch_refit_stats(double* __restrict__ rec, int nRed, int stage) {
    const int r = blockIdx.x * 64 + (threadIdx.x >> 2), k = threadIdx.x & 3;
    if (r >= nRed) return;
    refit_stats_step(rec + (size_t)r * kRefitDoubles, k, stage);
}

// ------------------------------------------------------------------------------------------
// Launchers
// ------------------------------------------------------------------------------------------
#define MCV_BATCH_MODEL_SWITCH(model, CALL)                                  \
    switch (model) {                                                         \
        case MCV_MODEL_HOMOGRAPHY: CALL(MCV_MODEL_HOMOGRAPHY); break;        \
        case MCV_MODEL_FUNDAMENTAL: CALL(MCV_MODEL_FUNDAMENTAL); break;      \
        case MCV_MODEL_AFFINE: CALL(MCV_MODEL_AFFINE); break;                \
        default: CALL(MCV_MODEL_SIMILARITY); break;                          \
    }

size_t batch_model_bytes(int model) {
    return model == MCV_MODEL_HOMOGRAPHY ? sizeof(HModelF) : model == MCV_MODEL_FUNDAMENTAL ? sizeof(FModelD)
                                                                                            : sizeof(AModelF);
}

template <int MODEL>
static void batch_generate_m(const float* d_pts4, const BatchDesc* d_desc, int nDesc, int maxHyp, uint64_t seed,
                             const int* d_table, void* d_models, int* d_counts, hipStream_t s) {
    constexpr int L = batch_gen_lanes<MODEL>();
    const int per = (maxHyp + L - 1) / L;
    hipLaunchKernelGGL(mcv_batch_generate<MODEL>, dim3((unsigned)per * nDesc), dim3(L), 0, s, d_pts4, d_desc, per, seed,
                       d_table, (typename BatchModel<MODEL>::Rec*)d_models, d_counts);
}

void launch_batch_generate(int model, const float* d_pts4, const BatchDesc* d_desc, int nDesc, int maxHyp,
                           uint64_t seed, const int* d_table, void* d_models, int* d_counts, hipStream_t s) {
#define CALL(M) batch_generate_m<M>(d_pts4, d_desc, nDesc, maxHyp, seed, d_table, d_models, d_counts, s)
    MCV_BATCH_MODEL_SWITCH(model, CALL)
#undef CALL
}

template <int MODEL, int KIND>
static void batch_sweep_mk(const float* d_pts4, const BatchDesc* d_desc, int nDesc, int maxHyp, const void* d_models,
                           int* d_counts, float thr2, hipStream_t s) {
    const int per = (maxHyp + 255) / 256;
    hipLaunchKernelGGL((mcv_batch_sweep<MODEL, KIND>), dim3((unsigned)per * nDesc), dim3(256), 0, s,
                       (const float4*)d_pts4, d_desc, per, (const typename BatchModel<MODEL>::Rec*)d_models, d_counts,
                       thr2);
}

void launch_batch_sweep(int model, int errKind, const float* d_pts4, const BatchDesc* d_desc, int nDesc, int maxHyp,
                        const void* d_models, int* d_counts, float thr2, hipStream_t s) {
    if (model == MCV_MODEL_FUNDAMENTAL) {
        switch (errKind) {
            case 0: batch_sweep_mk<MCV_MODEL_FUNDAMENTAL, 0>(d_pts4, d_desc, nDesc, maxHyp, d_models, d_counts, thr2, s); break;
            case 1: batch_sweep_mk<MCV_MODEL_FUNDAMENTAL, 1>(d_pts4, d_desc, nDesc, maxHyp, d_models, d_counts, thr2, s); break;
            case 2: batch_sweep_mk<MCV_MODEL_FUNDAMENTAL, 2>(d_pts4, d_desc, nDesc, maxHyp, d_models, d_counts, thr2, s); break;
            default: batch_sweep_mk<MCV_MODEL_FUNDAMENTAL, 3>(d_pts4, d_desc, nDesc, maxHyp, d_models, d_counts, thr2, s); break;
        }
    } else if (model == MCV_MODEL_HOMOGRAPHY) {
        batch_sweep_mk<MCV_MODEL_HOMOGRAPHY, 0>(d_pts4, d_desc, nDesc, maxHyp, d_models, d_counts, thr2, s);
    } else {
        batch_sweep_mk<MCV_MODEL_AFFINE, 0>(d_pts4, d_desc, nDesc, maxHyp, d_models, d_counts, thr2, s);
    }
}

template <int MODEL>
static void batch_one_m(const float* d_pts4, const BatchFin* d_fin, int nFin, uint64_t seed, const int* d_table,
                        BatchOne* d_one, hipStream_t s) {
    constexpr int L = batch_gen_lanes<MODEL>();
    hipLaunchKernelGGL(mcv_batch_one<MODEL>, dim3((nFin + L - 1) / L), dim3(L), 0, s, d_pts4, d_fin, nFin, seed,
                       d_table, d_one);
}

void launch_batch_one(int model, const float* d_pts4, const BatchFin* d_fin, int nFin, uint64_t seed,
                      const int* d_table, BatchOne* d_one, hipStream_t s) {
#define CALL(M) batch_one_m<M>(d_pts4, d_fin, nFin, seed, d_table, d_one, s)
    MCV_BATCH_MODEL_SWITCH(model, CALL)
#undef CALL
}

template <int MODEL, int KIND>
static void batch_mask_mk(const float* d_pts4, const BatchFin* d_fin, int nFin, int maxN, const BatchOne* d_one,
                          float thr2, uint8_t* d_mask, int* d_count, hipStream_t s) {
    const int per = (maxN + 255) / 256;
    hipLaunchKernelGGL((mcv_batch_mask<MODEL, KIND>), dim3((unsigned)per * nFin), dim3(256), 0, s,
                       (const float4*)d_pts4, d_fin, per, d_one, thr2, d_mask, d_count);
}

void launch_batch_mask(int model, int errKind, const float* d_pts4, const BatchFin* d_fin, int nFin, int maxN,
                       const BatchOne* d_one, float thr2, uint8_t* d_mask, int* d_count, hipStream_t s) {
    if (model == MCV_MODEL_FUNDAMENTAL) {
        switch (errKind) {
            case 0: batch_mask_mk<MCV_MODEL_FUNDAMENTAL, 0>(d_pts4, d_fin, nFin, maxN, d_one, thr2, d_mask, d_count, s); break;
            case 1: batch_mask_mk<MCV_MODEL_FUNDAMENTAL, 1>(d_pts4, d_fin, nFin, maxN, d_one, thr2, d_mask, d_count, s); break;
            case 2: batch_mask_mk<MCV_MODEL_FUNDAMENTAL, 2>(d_pts4, d_fin, nFin, maxN, d_one, thr2, d_mask, d_count, s); break;
            default: batch_mask_mk<MCV_MODEL_FUNDAMENTAL, 3>(d_pts4, d_fin, nFin, maxN, d_one, thr2, d_mask, d_count, s); break;
        }
    } else if (model == MCV_MODEL_HOMOGRAPHY) {
        batch_mask_mk<MCV_MODEL_HOMOGRAPHY, 0>(d_pts4, d_fin, nFin, maxN, d_one, thr2, d_mask, d_count, s);
    } else {
        batch_mask_mk<MCV_MODEL_AFFINE, 0>(d_pts4, d_fin, nFin, maxN, d_one, thr2, d_mask, d_count, s);
    }
}

int batch_reduce_blocks(int maxN) { return reduce_blocks(maxN); }

template <int V, class Op>
static void batch_reduce(const float* d_pts4, const uint8_t* d_mask, const BatchRed* d_red, int nRed, int maxN,
                         const double* d_par, int parStride, double* d_part, double* d_out, int outStride,
                         hipStream_t s) {
    const int per = reduce_blocks(maxN);
    hipLaunchKernelGGL((mcv_batch_reduce_pass<V, Op>), dim3((unsigned)per * nRed), dim3(kReduceThreads), 0, s,
                       (const float4*)d_pts4, d_mask, d_red, per, d_par, parStride, d_part);
    hipLaunchKernelGGL((mcv_batch_reduce_final<V>), dim3(nRed), dim3(kReduceThreads), 0, s, d_red, per, d_part, d_out,
                       outStride);
}

int launch_batch_reduce_lm(int lx, const float* d_pts4, const uint8_t* d_mask, const BatchRed* d_red, int nRed,
                           int maxN, const double* d_par, double* d_part, double* d_out, hipStream_t s) {
    if (lx == 8) batch_reduce<45, BOpHLM>(d_pts4, d_mask, d_red, nRed, maxN, d_par, 8, d_part, d_out, 45, s);
    else if (lx == 6)
        batch_reduce<a_lm_values(6), BOpALM<6>>(d_pts4, d_mask, d_red, nRed, maxN, d_par, 8, d_part, d_out, 45, s);
    else batch_reduce<a_lm_values(4), BOpALM<4>>(d_pts4, d_mask, d_red, nRed, maxN, d_par, 8, d_part, d_out, 45, s);
    return 2;
}

int launch_batch_refit_chain(const float* d_pts4, const uint8_t* d_mask, const BatchRed* d_red, int nRed, int maxN,
                             double* d_part, double* d_rec, hipStream_t s) {
    const int R = kRefitDoubles;
    const int sb = (nRed + 63) / 64;
    batch_reduce<5, BOpSums>(d_pts4, d_mask, d_red, nRed, maxN, d_rec, R, d_part, d_rec + kRefitSums, R, s);
    hipLaunchKernelGGL(mcv_batch_refit_stats, dim3(sb), dim3(256), 0, s, d_rec, nRed, 0);
    batch_reduce<4, BOpAbsDev>(d_pts4, d_mask, d_red, nRed, maxN, d_rec, R, d_part, d_rec + kRefitDev, R, s);
    hipLaunchKernelGGL(mcv_batch_refit_stats, dim3(sb), dim3(256), 0, s, d_rec, nRed, 1);
    batch_reduce<45, BOpLtL>(d_pts4, d_mask, d_red, nRed, maxN, d_rec, R, d_part, d_rec + kRefitLtL, R, s);
    return 8;
}

}  // namespace mcv
