// ransac_a_host.cpp — host side of the 2-D affine family: cvEstimateAffine2D (MCV_MODEL_AFFINE, 3-point
// samples, 6 refine parameters) and cvEstimateAffinePartial2D (MCV_MODEL_SIMILARITY, 2-point samples, 4
// refine parameters). Mirrors cv::estimateAffine2D / cv::estimateAffinePartial2D of OpenCV 4.x
// [ext: calib3d/src/ptsetreg.cpp, levmarq.cpp — absent here, DESIGN.md §3 / §7d]:
//   pack V2d -> float4  ->  RANSAC (ransac_search) or LMedS (lmeds_search) over the shared framework  ->
//   finalize: the winner's re-solve and mask, then LMSolver(refine callback, 10) on the inliers when
//   there are more of them than the sample size (no runKernel refit first)  ->  the 2x3 matrix, mask.
#include "minicv_native.h"
#include "mcv_runtime.h"
#include "kernels.h"
#include "mcv_common.h"
#include "hyp_affine.h"
#include "lm_solver.h"
#include "plan.h"

#include <cstring>
#include <vector>

namespace mcv {

// One chunk of hypotheses; the winner is re-solved from its sample (a closed form: nothing to cache).
// Shared by the RANSAC evaluate below and lmeds_search.
void a_generate(Plan& P, const void* d_pts, int N, const RansacConfig& cfg, int64_t hypBegin, int hypCount,
                int* d_counts, hipStream_t s) {
    P.last.clear();
    launch_a_generate(model_points(P.model), (const float*)d_pts, N, P.sampler(cfg), hypBegin, hypCount, P.models.p,
                      P.h64.p, d_counts, s);
}

void a_evaluate(Plan& P, const void* d_pts, int N, const RansacConfig& cfg, int64_t hypBegin, int hypCount,
                int* d_counts, bool, hipStream_t s) {
    P.pairs.ensure((size_t)(N + 1) / 2 * 8);
    launch_h_pair((const float*)d_pts, N, P.pairs.p, s);
    {
        ProfScope pg("a_generate", s);
        a_generate(P, d_pts, N, cfg, hypBegin, hypCount, d_counts, s);
    }
    ProfScope ps("a_verify", s);
    launch_a_verify(P.pairs.p, N, P.models.p, d_counts, hypCount, thr2_of(P, cfg), fused_error(cfg), s);
}

// LMSolver::create(Affine2DRefineCallback / AffinePartial2DRefineCallback, 10)->run: the sums over the
// inliers on the GPU (reduce.h's block order), the solver on the host (lm_solver.h).
template <int LX>
static void a_lm_refine(Plan& P, const float* d_pts, int N, const uint8_t* d_mask, hipStream_t s, double* A) {
    double h[LX];
    a_to_params(LX, A, h);
    auto sums = [&](const double* x, double* buf) {
        reduce_to_host(P, s, a_lm_values(LX), buf,
                       [&](double* part, double* red) { a_reduce_lm(LX, d_pts, N, d_mask, x, part, red, s); });
    };
    lm_solver_run<LX>(sums, h, 10);
    a_from_params(LX, h, A);
}

// The same refine with sequential sums on the host (mcvHostAffineRefine).
template <int LX>
static int a_lm_refine_host(const float* pts4, int N, const uint8_t* mask, double* A) {
    double h[LX];
    a_to_params(LX, A, h);
    int used = 0;
    for (int i = 0; i < N; ++i) used += (!mask || mask[i]) ? 1 : 0;
    auto sums = [&](const double* x, double* buf) {
        for (int k = 0; k < a_lm_values(LX); ++k) buf[k] = 0;
        for (int i = 0; i < N; ++i) {
            if (mask && !mask[i]) continue;
            const float* q = pts4 + 4 * (size_t)i;
            a_lm_terms<LX>(x, (double)q[0], (double)q[1], (double)q[2], (double)q[3], buf);
        }
    };
    lm_solver_run<LX>(sums, h, 10);
    a_from_params(LX, h, A);
    return used;
}

// Winner -> mask (+ LM). direct: the N == m solve on all points. Returns the inlier count. Synchronises s.
static int a_finalize_impl(Plan& P, const float* d_pts, int N, const RansacConfig& cfg, int64_t hyp, double* model9,
                           uint8_t* d_mask, hipStream_t s, bool direct) {
    const int m = model_points(P.model);
    AOneOut* d_one = (AOneOut*)P.one.p;
    launch_a_one(m, d_pts, N, P.sampler(cfg), hyp, d_one, s, direct);
    if (!direct) {   // the record and the count come back with one synchronisation
        zero_count(P, s);
        launch_a_mask_one(d_pts, N, d_one, thr2_of(P, cfg), fused_error(cfg), d_mask, P.count.p, s);
        queue_count(P, s);
    }
    MCV_HIP(hipGetLastError());
    queue_one<AOneOut>(P, s);
    MCV_HIP(hipStreamSynchronize(s));
    const AOneOut one = take_one<AOneOut>(P);
    if (one.status != 1) {
        if (direct) fail("degenerate point set (no finite model from the %d correspondences)", m);
        fail("winning hypothesis %lld has no model (status %d)", (long long)hyp, one.status);
    }
    const int count = direct ? N : take_count(P);
    double A[6];
    for (int k = 0; k < 6; ++k) A[k] = one.A[k];
    if (!direct && !(cfg.flags & MCV_FLAG_NO_REFINE) && count > m) {
        if (m == 3) a_lm_refine<6>(P, d_pts, N, d_mask, s, A);
        else a_lm_refine<4>(P, d_pts, N, d_mask, s, A);
    }
    for (int k = 0; k < 6; ++k) model9[k] = A[k];
    model9[6] = 0; model9[7] = 0; model9[8] = 1;
    return count;
}

int a_finalize(Plan& P, const void* d_pts, int N, const RansacConfig& cfg, int64_t hyp, double* model9,
               uint8_t* d_mask, hipStream_t s) {
    return a_finalize_impl(P, (const float*)d_pts, N, cfg, hyp, model9, d_mask, s, false);
}

// The 2-D entry's direct case: N == the sample size, one solve on all points.
bool a_entry_direct(Plan& P, const char*, int N, const RansacConfig& cfg, hipStream_t s, double* model9) {
    if (N != model_points(P.model)) return false;
    a_finalize_impl(P, P.pts.p, N, cfg, 0, model9, P.mask.p, s, true);
    return true;
}

int a_host_hypothesis(int model, const float* pts4, int N, uint64_t seed, int64_t hyp, double* model9, float* modelf9,
                      int* sampleIdx, bool) {
    const int m = model_points(model);
    if (N < m) fail("N < %d", m);
    AModelF mf;
    double A[6];
    for (int k = 0; k < 6; ++k) { A[k] = 0; mf.a[k] = 0; }
    int idx[3] = {-1, -1, -1};
    const Sampler smp{seed, nullptr};
    const int st = m == 3 ? a_hypothesis<3>(pts4, N, smp, (uint64_t)hyp, A, &mf, idx)
                          : a_hypothesis<2>(pts4, N, smp, (uint64_t)hyp, A, &mf, idx);
    for (int k = 0; k < 6; ++k) { model9[k] = A[k]; modelf9[k] = mf.a[k]; }
    if (sampleIdx) for (int k = 0; k < m; ++k) sampleIdx[k] = idx[k];
    return st;
}

// The exports' 2 x 3 result: the first six of find_model_2d's nine.
static int estimate_affine(int model, const char* who, const mcvV2d* from, const mcvV2d* to, int N,
                           const RansacConfig* cfgp, double* A6, uint8_t* mask) {
    double model9[9];
    const int count = find_model_2d(model, who, from, to, N, cfgp, A6 ? model9 : nullptr, mask);
    for (int k = 0; k < 6; ++k) A6[k] = model9[k];
    return count;
}

}  // namespace mcv

using namespace mcv;

extern "C" MCV_API int cvEstimateAffine2D(const mcvV2d* from, const mcvV2d* to, const int N, const RansacConfig* cfg,
                                          double* A6, uint8_t* mask) {
    MCV_GUARD(0, { return estimate_affine(MCV_MODEL_AFFINE, "cvEstimateAffine2D", from, to, N, cfg, A6, mask); })
}

extern "C" MCV_API int cvEstimateAffinePartial2D(const mcvV2d* from, const mcvV2d* to, const int N,
                                                 const RansacConfig* cfg, double* A6, uint8_t* mask) {
    MCV_GUARD(0, {
        return estimate_affine(MCV_MODEL_SIMILARITY, "cvEstimateAffinePartial2D", from, to, N, cfg, A6, mask);
    })
}

extern "C" MCV_API int mcvTestAffineSweep(const float* pts4, int N, const float* models6, int nModels, float thr2,
                                          int fused, int* counts) {
    MCV_GUARD(0, {
        if (!pts4 || !models6 || !counts) fail("mcvTestAffineSweep: null argument");
        if (N <= 0 || nModels <= 0) fail("mcvTestAffineSweep: bad sizes (N=%d, models=%d)", N, nModels);
        require_device();
        DevBuf<float> p, m, pairs;
        DevBuf<int> c;
        p.ensure((size_t)N * 4);
        m.ensure((size_t)nModels * 6);
        pairs.ensure((size_t)(N + 1) / 2 * 8);
        c.ensure((size_t)nModels);
        MCV_HIP(hipMemcpy(p.p, pts4, (size_t)N * 16, hipMemcpyHostToDevice));
        MCV_HIP(hipMemcpy(m.p, models6, (size_t)nModels * 24, hipMemcpyHostToDevice));
        MCV_HIP(hipMemset(c.p, 0, (size_t)nModels * 4));
        launch_h_pair(p.p, N, pairs.p, 0);
        {
            ProfScope ps("a_verify", 0);
            launch_a_verify(pairs.p, N, m.p, c.p, nModels, thr2, fused != 0, 0);
        }
        MCV_HIP(hipGetLastError());
        MCV_HIP(hipMemcpy(counts, c.p, (size_t)nModels * 4, hipMemcpyDeviceToHost));
        return 1;
    })
}

extern "C" MCV_API int mcvHostAffineRefine(int model, const float* pts4, int N, const uint8_t* mask, double* A6) {
    MCV_GUARD(-1, {
        if (!pts4 || !A6 || N <= 0) fail("mcvHostAffineRefine: bad argument");
        if (!affine_family(model)) fail("mcvHostAffineRefine: model %d is not affine / similarity", model);
        return model == MCV_MODEL_AFFINE ? a_lm_refine_host<6>(pts4, N, mask, A6)
                                         : a_lm_refine_host<4>(pts4, N, mask, A6);
    })
}
