// ransac_h_refine.hip — what follows the homography search on gfx950: the winner's inlier mask
// (mcv_h_mask_one, the same fp32 error as the sweep)                      [SURVEY §2 K4, mask]
// and the fixed-order fp64 reductions over the inliers (reduce.h): centroid, mean |dev| and the 9x9 LtL
// of runKernel chained on the device (h_refit_chain), and the 8x8 JtJ / Jtr / |r|^2 of the LM refine
// (h_reduce_lm). h_reduce_sums also serves the fundamental fit (ransac_f_host.cpp).
#include "mcv_common.h"
#include "hyp_homography.h"
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
        a[0] += (double)q.z; a[1] += (double)q.w; a[2] += (double)q.x; a[3] += (double)q.y; a[4] += 1.0;
    }
};
struct OpAbsDevD {  // 4: sum |dst - cm|, |src - cM|, the centroids read from device memory (chained refit)
    const float4* pts; const uint8_t* mask; const double* c4;
    __device__ void operator()(int i, double (&a)[4]) const {
        if (mask && !mask[i]) return;
        const float4 q = pts[i];
        a[0] += fabs((double)q.z - c4[0]); a[1] += fabs((double)q.w - c4[1]);
        a[2] += fabs((double)q.x - c4[2]); a[3] += fabs((double)q.y - c4[3]);
    }
};
struct OpLtL {     // 45: upper triangle of LtL, row-major
    const float4* pts; const uint8_t* mask; double cmx, cmy, cMx, cMy, smx, smy, sMx, sMy;
    __device__ void operator()(int i, double (&a)[45]) const {
        if (mask && !mask[i]) return;
        const float4 q = pts[i];
        const double x = ((double)q.z - cmx) * smx, y = ((double)q.w - cmy) * smy;
        const double X = ((double)q.x - cMx) * sMx, Y = ((double)q.y - cMy) * sMy;
        const double Lx[9] = {X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x};
        const double Ly[9] = {0, 0, 0, X, Y, 1, -y * X, -y * Y, -y};
        int o = 0;
#pragma unroll
        for (int j = 0; j < 9; ++j)
#pragma unroll
            for (int k = j; k < 9; ++k) a[o++] += Lx[j] * Lx[k] + Ly[j] * Ly[k];
    }
};
struct OpLM {      // 45: JtJ upper triangle (36), Jtr (8), |r|^2 (1)
    const float4* pts; const uint8_t* mask; double h[8];
    __device__ void operator()(int i, double (&a)[45]) const {
        if (mask && !mask[i]) return;
        const float4 q = pts[i];
        const double Mx = q.x, My = q.y;
        double ww = h[6] * Mx + h[7] * My + 1.;
        ww = fabs(ww) > kDblEpsilon ? 1. / ww : 0;
        const double xi = (h[0] * Mx + h[1] * My + h[2]) * ww;
        const double yi = (h[3] * Mx + h[4] * My + h[5]) * ww;
        const double rx = xi - (double)q.z, ry = yi - (double)q.w;
        const double Jx[8] = {Mx * ww, My * ww, ww, 0, 0, 0, -Mx * ww * xi, -My * ww * xi};
        const double Jy[8] = {0, 0, 0, Mx * ww, My * ww, ww, -Mx * ww * yi, -My * ww * yi};
        int o = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int k = j; k < 8; ++k) a[o++] += Jx[j] * Jx[k] + Jy[j] * Jy[k];
#pragma unroll
        for (int j = 0; j < 8; ++j) a[36 + j] += Jx[j] * rx + Jy[j] * ry;
        a[44] += rx * rx + ry * ry;
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
struct OpLtLD {    // OpLtL with centroids / scales read from device memory (chained refit)
    const float4* pts; const uint8_t* mask; const double* c4; const double* s4;
    __device__ void operator()(int i, double (&a)[45]) const {
        OpLtL op{pts, mask, c4[0], c4[1], c4[2], c4[3], s4[0], s4[1], s4[2], s4[3]};
        op(i, a);
    }
};

// refit statistics between the chained passes: c4 = sums / count, s4 = count / absdev (the same
// IEEE divisions the host performs, so the passes see bit-identical constants)
__global__ void mcv_refit_stats(double* __restrict__ red, int stage) {
    if (threadIdx.x >= 4) return;
    const int k = threadIdx.x;
    if (stage == 0) red[5 + k] = red[k] / red[4];
    else red[13 + k] = red[4] / red[9 + k];
}

// HomographyEstimatorCallback::runKernel's three passes chained on the device (no host round trip):
// red[0..4] = sums, red[5..8] = centroids, red[9..12] = |dev| sums, red[13..16] = scales,
// red[17..61] = LtL.
void h_refit_chain(const float* d_pts4, int N, const uint8_t* d_mask, double* d_part, double* d_red, hipStream_t s) {
    const float4* p = (const float4*)d_pts4;
    run_reduce<5>(N, OpSums{p, d_mask}, d_part, d_red, s);
    hipLaunchKernelGGL(mcv_refit_stats, dim3(1), dim3(64), 0, s, d_red, 0);
    run_reduce<4>(N, OpAbsDevD{p, d_mask, d_red + 5}, d_part, d_red + 9, s);
    hipLaunchKernelGGL(mcv_refit_stats, dim3(1), dim3(64), 0, s, d_red, 1);
    run_reduce<45>(N, OpLtLD{p, d_mask, d_red + 5, d_red + 13}, d_part, d_red + 17, s);
}

void h_reduce_lm(const float* d_pts4, int N, const uint8_t* d_mask, const double* h8, double* d_part, double* d_out,
                 hipStream_t s) {
    OpLM op{(const float4*)d_pts4, d_mask, {h8[0], h8[1], h8[2], h8[3], h8[4], h8[5], h8[6], h8[7]}};
    run_reduce<45>(N, op, d_part, d_out, s);
}

}  // namespace mcv
