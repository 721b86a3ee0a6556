// ransac_a.hip — gfx950 kernels of the 2-D affine family (estimateAffine2D, M = 3 point samples;
// estimateAffinePartial2D, M = 2): both store the same 6-float model, so only the generate and the
// refine sums know which of the two they serve.
//
//   mcv_a_generate<M>  one lane per hypothesis: Philox sample or table row -> subset check -> closed
//                      form (fp64) -> fp32 model (24 B) + fp64 model + status.
//   mcv_a_verify_pk    the inlier sweep in packed f32 over the homography's HPair layout (mcv_h_pair):
//                      K hypotheses per wave, coefficients in SGPR pairs broadcast by op_sel, NP point
//                      pairs per lane per trip, ballot + popcount counts.
//   mcv_a_one / mcv_a_mask_one / OpALM   the winner: re-solve, mask + count, refine sums (reduce.h).
//
// The error divides nothing, so the packed sweep evaluates computeError itself, operation by operation:
//   op by op (default)   T0 = F0 * x;  T1 = F1 * y;  S = T0 + T1;  S = S + F2;  A = S - X    (b likewise)
//                        E = A * A + B * B        — v_pk_mul_f32 / v_pk_add_f32 only, no fma
//   fused                A = fma(F0, x, fma(F1, y, F2)) - X;  E = fma(A, A, B * B)   — v_pk_fma_f32
// Each packed op rounds like its scalar form (the default kernel mode keeps f32 subnormals), so the
// counts are final: no certificate, no bounding-box precondition, no kStatusRedo, no recount.
#include <algorithm>
#include "mcv_common.h"
#include "hyp_affine.h"
#include "pk_pair.h"
#include "reduce.h"
#include "kernels.h"
#include "minicv_native.h"

namespace mcv {

template <int M>
__global__ __launch_bounds__(256) void mcv_a_generate(const float* __restrict__ pts4, int N, Sampler smp,
                                                      int64_t hypBegin, int hypCount, AModelF* __restrict__ models,
                                                      double* __restrict__ a64, int* __restrict__ counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= hypCount) return;
    double A[6];
    AModelF mf;
    const int st = a_hypothesis<M>(pts4, N, smp, (uint64_t)(hypBegin + i), A, &mf, nullptr);
    if (st != 1) {
        // the zero model (err = X^2 + Y^2) keeps the sweep's slot finite; its count is never written
#pragma unroll
        for (int j = 0; j < 6; ++j) { mf.a[j] = 0.f; A[j] = 0.0; }
    }
    models[i] = mf;
#pragma unroll
    for (int j = 0; j < 6; ++j) a64[6 * (int64_t)i + j] = A[j];
    counts[i] = st == 1 ? 0 : st;
}

// One hypothesis in full (finalize path, and the N == M direct solve).
template <int M>
__global__ void mcv_a_one(const float* __restrict__ pts4, int N, Sampler smp, int64_t hyp, AOneOut* __restrict__ out,
                          bool direct) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    AOneOut o;
    AModelF mf;
    for (int j = 0; j < 6; ++j) { o.A[j] = 0; mf.a[j] = 0; }
    for (int j = 0; j < 3; ++j) o.idx[j] = -1;
    o.status = a_hypothesis<M>(pts4, N, smp, (uint64_t)hyp, o.A, &mf, o.idx, direct);
    for (int j = 0; j < 6; ++j) o.af[j] = mf.a[j];
    *out = o;
}

// ------------------------------------------------------------------------------------------
// Packed-f32 inlier sweep. Layout and conventions of mcv_h_verify_pk (ransac_h_sweep.hip): HPair p holds
// correspondences (2p, 2p + 1) as {x, y, X, Y} pairs; an odd N is padded with {0, 0, NaN, NaN}, whose
// error is NaN (never an inlier). Wave w owns hypotheses [w K, w K + K): (F0,F1) (F2,F3) (F4,F5) as
// three SGPR pairs each. A VOP3P op reads one SGPR pair (constant-bus limit), so the addends F2 / F5,
// which sit beside an SGPR multiplier in the fused form's inner fma, live in one VGPR pair per
// hypothesis, as h2 / h5 do in the homography sweep. K = 8, NP = 2: 48 SGPRs of coefficients, 16 VGPRs
// of addends, 16 of points — the homography's packed shape, kept as the first form that is exact.
// ------------------------------------------------------------------------------------------
template <int K, int NP, bool FUSED, bool PRED>
__device__ __forceinline__ void a_pk_trip(const f2 (&ap)[K][3], const f2 (&ac)[K], const HPair (&q)[NP],
                                          const bool (&v)[NP], float thr2, uint32_t (&cnt)[K]) {
    auto vote = [&](int j, bool pred) -> uint32_t {
        if constexpr (PRED)
            return (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(v[j] && pred));
        else
            return (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(pred));
    };
#pragma unroll
    for (int k = 0; k < K; ++k) {
        // re-define the pairs in the trip (no instruction), so that every broadcast folds into op_sel
        // instead of being hoisted as a splat pair (see h_pk_trip)
        f2 p0 = ap[k][0], p1 = ap[k][1], p2 = ap[k][2];   // (F0,F1) (F2,F3) (F4,F5)
        f2 c = ac[k];                                      // (F2, F5)
        asm volatile("" : "+s"(p0), "+s"(p1), "+s"(p2), "+v"(c));
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            f2 A, B, E;
            if constexpr (FUSED) {
                A = pk_fma(lo(p0), q[j].x, pk_fma(hi(p0), q[j].y, lo(c))) - q[j].mx;
                B = pk_fma(hi(p1), q[j].x, pk_fma(lo(p2), q[j].y, hi(c))) - q[j].my;
                E = pk_fma(A, A, B * B);
            } else {
                A = ((lo(p0) * q[j].x + hi(p0) * q[j].y) + lo(c)) - q[j].mx;
                B = ((hi(p1) * q[j].x + lo(p2) * q[j].y) + hi(c)) - q[j].my;
                E = A * A + B * B;
            }
            cnt[k] += vote(j, E.x <= thr2) + vote(j, E.y <= thr2);
        }
    }
}

template <int K, int NP, bool FUSED>
__global__ __launch_bounds__(256) void mcv_a_verify_pk(const HPair* __restrict__ pairs, int nPairs,
                                                       const AModelF* __restrict__ models, int* __restrict__ counts,
                                                       int hypCount, float thr2) {
    const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * 256u + threadIdx.x) >> 6));
    const int lane = threadIdx.x & 63;
    const int h0 = wave * K;
    if (h0 >= hypCount) return;

    // every slot below hypCount holds a model (the zero model for a failed hypothesis); slots past
    // hypCount re-read the last one and are never written
    f2 ap[K][3], ac[K];
    bool valid[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int hk = h0 + k;
        valid[k] = (hk < hypCount) && (counts[hk] >= 0);
        const f2* mp = (const f2*)&models[hk < hypCount ? hk : hypCount - 1];
#pragma unroll
        for (int j = 0; j < 3; ++j) ap[k][j] = mp[j];
        ac[k] = f2{ap[k][1].x, ap[k][2].y};
        asm volatile("" : "+v"(ac[k]));
    }
    uint32_t cnt[K];
#pragma unroll
    for (int k = 0; k < K; ++k) cnt[k] = 0;

    constexpr int TRIP = 64 * NP;
    const int nFull = nPairs / TRIP * TRIP;
    bool vt[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) vt[j] = true;
    for (int base = 0; base < nFull; base += TRIP) {
        HPair q[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) q[j] = pairs[base + 64 * j + lane];
        a_pk_trip<K, NP, FUSED, false>(ap, ac, q, vt, thr2, cnt);
    }
    if (nFull < nPairs) {
        HPair q[NP];
        bool v[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int p = nFull + 64 * j + lane;
            v[j] = p < nPairs;
            q[j] = pairs[v[j] ? p : 0];
        }
        a_pk_trip<K, NP, FUSED, true>(ap, ac, q, v, thr2, cnt);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (valid[k]) counts[h0 + k] = (int)cnt[k];
    }
}

// Inlier mask of the winner record (count via per-wave ballot + one atomic per wave).
__global__ __launch_bounds__(256) void mcv_a_mask_one(const float4* __restrict__ pts, int N,
                                                      const AOneOut* __restrict__ one, float thr2, int fused,
                                                      uint8_t* __restrict__ mask, int* __restrict__ count) {
    float f[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) f[j] = one->af[j];
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool in = false;
    if (i < N) {
        const float4 q = pts[i];
        const float e = fused ? a_error_fused(f, q.x, q.y, q.z, q.w) : a_error(f, q.x, q.y, q.z, q.w);
        in = e <= thr2;
        mask[i] = in ? 1 : 0;
    }
    const uint64_t b = __ballot(in);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, (int)__popcll(b));
}

// Refine sums (Affine2DRefineCallback / AffinePartial2DRefineCallback::compute): JtJ upper triangle,
// Jtr, |r|^2 over the inliers, in reduce.h's fixed block order.
template <int LX>
struct OpALM {
    const float4* pts; const uint8_t* mask; double h[LX];
    __device__ void operator()(int i, double (&a)[a_lm_values(LX)]) const {
        if (mask && !mask[i]) return;
        const float4 q = pts[i];
        a_lm_terms<LX>(h, (double)q.x, (double)q.y, (double)q.z, (double)q.w, a);
    }
};

// ------------------------------------------------------------------------------------------
// Launchers
// ------------------------------------------------------------------------------------------
void launch_a_generate(int m, const float* d_pts4, int N, Sampler smp, int64_t hypBegin, int hypCount, void* d_models,
                       double* d_a64, int* d_counts, hipStream_t s) {
    const dim3 grid((hypCount + 255) / 256), block(256);
    if (m == 3)
        hipLaunchKernelGGL(mcv_a_generate<3>, grid, block, 0, s, d_pts4, N, smp, hypBegin, hypCount,
                           (AModelF*)d_models, d_a64, d_counts);
    else
        hipLaunchKernelGGL(mcv_a_generate<2>, grid, block, 0, s, d_pts4, N, smp, hypBegin, hypCount,
                           (AModelF*)d_models, d_a64, d_counts);
}

void launch_a_one(int m, const float* d_pts4, int N, Sampler smp, int64_t hyp, AOneOut* d_out, hipStream_t s,
                  bool direct) {
    if (m == 3) hipLaunchKernelGGL(mcv_a_one<3>, dim3(1), dim3(64), 0, s, d_pts4, N, smp, hyp, d_out, direct);
    else hipLaunchKernelGGL(mcv_a_one<2>, dim3(1), dim3(64), 0, s, d_pts4, N, smp, hyp, d_out, direct);
}

void launch_a_verify(const void* d_pairs, int N, const void* d_models, int* d_counts, int hypCount, float thr2,
                     bool fused, hipStream_t s) {
    constexpr int K = kVerifyAHypPerWave, NP = kVerifyAPairsPerLane;
    const int waves = (hypCount + K - 1) / K;
    const int blocks = (waves + 3) / 4;
    if (fused)
        hipLaunchKernelGGL((mcv_a_verify_pk<K, NP, true>), dim3(blocks), dim3(256), 0, s, (const HPair*)d_pairs,
                           (N + 1) / 2, (const AModelF*)d_models, d_counts, hypCount, thr2);
    else
        hipLaunchKernelGGL((mcv_a_verify_pk<K, NP, false>), dim3(blocks), dim3(256), 0, s, (const HPair*)d_pairs,
                           (N + 1) / 2, (const AModelF*)d_models, d_counts, hypCount, thr2);
}

void launch_a_mask_one(const float* d_pts4, int N, const AOneOut* d_one, float thr2, bool fused, uint8_t* d_mask,
                       int* d_count, hipStream_t s) {
    hipLaunchKernelGGL(mcv_a_mask_one, dim3((N + 255) / 256), dim3(256), 0, s, (const float4*)d_pts4, N, d_one, thr2,
                       fused ? 1 : 0, d_mask, d_count);
}

void a_reduce_lm(int lx, const float* d_pts4, int N, const uint8_t* d_mask, const double* h, double* d_part,
                 double* d_out, hipStream_t s) {
    if (lx == 6) {
        OpALM<6> op{(const float4*)d_pts4, d_mask, {h[0], h[1], h[2], h[3], h[4], h[5]}};
        run_reduce<a_lm_values(6)>(N, op, d_part, d_out, s);
    } else {
        OpALM<4> op{(const float4*)d_pts4, d_mask, {h[0], h[1], h[2], h[3]}};
        run_reduce<a_lm_values(4)>(N, op, d_part, d_out, s);
    }
}

}  // namespace mcv
