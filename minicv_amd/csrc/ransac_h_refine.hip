// ransac_h_refine.hip — what follows the homography search on gfx950: the winner's inlier mask
// (mcv_h_mask_one, the same fp32 error as the sweep)                      [SURVEY §2 K4, mask]
// and the fixed-order fp64 reductions over the inliers (reduce.h): centroid, mean |dev| and the 9x9 LtL
// of runKernel chained on the device (h_refit_chain), and the 8x8 JtJ / Jtr / |r|^2 of the LM refine
// (h_reduce_lm). h_reduce_sums also serves the fundamental fit (ransac_f_host.cpp). The per-point terms of
// the four sums are h_refine_terms.h's, shared with the batched call (ransac_batch.hip).
#include "mcv_common.h"
#include "hyp_homography.h"
#include "h_refine_terms.h"
#include "reduce.h"
#include "kernels.h"

namespace mcv {

// ------------------------------------------------------------------------------------------
// Inlier mask of one model (count via per-wave ballot + one atomic per wave), the model read from
// the winner record mcv_h_one wrote (no host round trip).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mcv_h_mask_one(const float4* __restrict__ pts, int N,
                                                      const HOneOut* __restrict__ one, float thr2, int fused,
                                                      uint8_t* __restrict__ mask, int* __restrict__ count) {
    HModelF m;
#pragma unroll
    for (int j = 0; j < 8; ++j) m.h[j] = one->hf[j];
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool in = false;
    if (i < N) {
        const float4 q = pts[i];
        const float e = fused ? h_error_fused(m.h, q.x, q.y, q.z, q.w) : h_error(m.h, q.x, q.y, q.z, q.w);
        in = e <= thr2;
        mask[i] = in ? 1 : 0;
    }
    const uint64_t b = __ballot(in);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, (int)__popcll(b));
}

// ------------------------------------------------------------------------------------------
// Refit (HomographyEstimatorCallback::runKernel over the inliers) and LM
// (HomographyRefineCallback::compute) reductions.
// ------------------------------------------------------------------------------------------
struct OpSums {   // 5: sum dst.x, dst.y, src.x, src.y, count
    const float4* pts; const uint8_t* mask;
    __device__ void operator()(int i, double (&a)[5]) const {
        if (mask && !mask[i]) return;
        const float4 q = pts[i];
        h_sums_terms((double)q.x, (double)q.y, (double)q.z, (double)q.w, a);
    }
};
struct OpAbsDev {  // 4: sum |dst - cm|, |src - cM|, the centroids read from the refit record
    const float4* pts; const uint8_t* mask; const double* c4;
    __device__ void operator()(int i, double (&a)[4]) const {
        if (mask && !mask[i]) return;
        const float4 q = pts[i];
        h_absdev_terms(c4, (double)q.x, (double)q.y, (double)q.z, (double)q.w, a);
    }
};
struct OpLtL {     // 45: upper triangle of LtL, centroids and scales read from the refit record
    const float4* pts; const uint8_t* mask; const double* c4; const double* s4;
    __device__ void operator()(int i, double (&a)[45]) const {
        // read ahead of the mask test: unconditional, so the eight loads leave the pass's loop
        const double c[4] = {c4[0], c4[1], c4[2], c4[3]}, sc[4] = {s4[0], s4[1], s4[2], s4[3]};
        if (mask && !mask[i]) return;
        const float4 q = pts[i];
        h_ltl_terms(c, sc, (double)q.x, (double)q.y, (double)q.z, (double)q.w, a);
    }
};
struct OpLM {      // 45: JtJ upper triangle (36), Jtr (8), |r|^2 (1)
    const float4* pts; const uint8_t* mask; double h[8];
    __device__ void operator()(int i, double (&a)[45]) const {
        if (mask && !mask[i]) return;
        const float4 q = pts[i];
        h_lm_terms(h, (double)q.x, (double)q.y, (double)q.z, (double)q.w, a);
    }
};

void launch_h_mask_one(const float* d_pts4, int N, const HOneOut* d_one, float thr2, bool fused, uint8_t* d_mask,
                       int* d_count, hipStream_t s) {
    hipLaunchKernelGGL(mcv_h_mask_one, dim3((N + 255) / 256), dim3(256), 0, s, (const float4*)d_pts4, N, d_one, thr2,
                       fused ? 1 : 0, d_mask, d_count);
}

void h_reduce_sums(const float* d_pts4, int N, const uint8_t* d_mask, double* d_part, double* d_out, hipStream_t s) {
    OpSums op{(const float4*)d_pts4, d_mask};
    run_reduce<5>(N, op, d_part, d_out, s);
}

// The step between the chained passes on the one record (h_refine_terms.h)
__global__ void mcv_refit_stats(double* __restrict__ red, int stage) {
    if (threadIdx.x >= 4) return;
    refit_stats_step(red, threadIdx.x, stage);
}

// HomographyEstimatorCallback::runKernel's three passes chained on the device (no host round trip) into
// the refit record d_red (kernels.h kRefit*).
void h_refit_chain(const float* d_pts4, int N, const uint8_t* d_mask, double* d_part, double* d_red, hipStream_t s) {
    const float4* p = (const float4*)d_pts4;
    run_reduce<5>(N, OpSums{p, d_mask}, d_part, d_red + kRefitSums, s);
    hipLaunchKernelGGL(mcv_refit_stats, dim3(1), dim3(64), 0, s, d_red, 0);
    run_reduce<4>(N, OpAbsDev{p, d_mask, d_red + kRefitC4}, d_part, d_red + kRefitDev, s);
    hipLaunchKernelGGL(mcv_refit_stats, dim3(1), dim3(64), 0, s, d_red, 1);
    run_reduce<45>(N, OpLtL{p, d_mask, d_red + kRefitC4, d_red + kRefitS4}, d_part, d_red + kRefitLtL, s);
}

void h_reduce_lm(const float* d_pts4, int N, const uint8_t* d_mask, const double* h8, double* d_part, double* d_out,
                 hipStream_t s) {
    OpLM op{(const float4*)d_pts4, d_mask, {h8[0], h8[1], h8[2], h8[3], h8[4], h8[5], h8[6], h8[7]}};
    run_reduce<45>(N, op, d_part, d_out, s);
}

}  // namespace mcv
