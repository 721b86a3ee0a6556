// ransac_f_host.cpp — host side of the fundamental-matrix family: cvFindFundamentalMat (new export;
// OpenCV 4.x cv::findFundamentalMat(points1, points2, FM_RANSAC / FM_8POINT, thr, conf, maxIters, mask)
// semantics, restated [ext]): the RANSAC result is the best hypothesis' model (OpenCV does not
// refit F on the inliers); FM_8POINT (method 0 here) fits all points. The search is the shared
// framework's (ransac_host.cpp); a chunk's generate + verify (8-point and 7-point) and the winner's
// finalize are here.
#include "minicv_native.h"
#include "mcv_runtime.h"
#include "kernels.h"
#include "linalg.h"
#include "hyp_fundamental.h"
#include "hyp_f7.h"
#include "sampson_pk.h"
#include "plan.h"

#include <cmath>
#include <cfloat>
#include <cstring>

namespace mcv {

int f_error_kind(const RansacConfig& cfg) {
    const int e = cfg.errorKind == MCV_FERR_EPIPOLAR ? 1 : 0;
    return e * 2 + ((cfg.flags & MCV_FLAG_FUSED_ERROR) ? 0 : 1);
}

// MCV_FLAG_SEVEN_POINT: 7-point samples (OpenCV's FM_RANSAC / FM_LMEDS), up to 3 models each
static bool f_seven(const RansacConfig& cfg) { return (cfg.flags & MCV_FLAG_SEVEN_POINT) != 0; }
int f_points_cfg(const RansacConfig& cfg) { return f_seven(cfg) ? 7 : 8; }
int f_slots_cfg(const RansacConfig& cfg) { return f_seven(cfg) ? kF7Slots : 1; }
static ChunkSolver f_solver(const RansacConfig& cfg) { return fast_minimal(cfg) ? kSolverF8Fast : kSolverF8Exact; }

// One chunk of hypotheses. 8-point: P.last = this chunk (the winner's fp64 model can come straight from
// its buffer: f_finalize). 7-point (OpenCV FM_RANSAC): 3 model slots per hypothesis (slot keys like
// essential), nothing cached. Shared by the RANSAC evaluate below and lmeds_search.
void f_generate(Plan& P, const void* d_ptsv, int N, const RansacConfig& cfg, int64_t hypBegin, int hypCount,
                int* d_counts, hipStream_t s) {
    const float* d_pts = (const float*)d_ptsv;
    const Sampler smp = P.sampler(cfg);
    if (f_seven(cfg)) {
        P.last.clear();
        launch_f7_generate(d_pts, N, smp, hypBegin, hypCount, P.models.p, d_counts, s);
        return;
    }
    launch_f_generate(d_pts, N, smp, hypBegin, hypCount, P.models.p, d_counts, s, fast_minimal(cfg));
    mark_chunk(P, hypBegin, hypCount, smp, d_pts, N, f_solver(cfg), s);
}

void f_evaluate(Plan& P, const void* d_ptsv, int N, const RansacConfig& cfg, int64_t hypBegin, int hypCount,
                int* d_counts, bool, hipStream_t s) {
    const float* d_pts = (const float*)d_ptsv;
    if (f_seven(cfg)) {
        f_generate(P, d_pts, N, cfg, hypBegin, hypCount, d_counts, s);
    } else {
        ProfScope pg("f_generate", s);
        f_generate(P, d_pts, N, cfg, hypBegin, hypCount, d_counts, s);
    }
    P.bb4.ensure(4);
    launch_abs_bound4(d_pts, false, N, P.bb4.p, nullptr, s);
    ProfScope ps("f_verify", s);
    const int nSlots = hypCount * f_slots_cfg(cfg);
    launch_f_verify(d_pts, N, P.models.p, d_counts, nSlots, thr2_of(P, cfg), f_error_kind(cfg), s, P.bb4.p);
}

int f_finalize(Plan& P, const void* d_ptsv, int N, const RansacConfig& cfg, int64_t hyp, double* F, uint8_t* d_mask,
               hipStream_t s) {
    const float* d_pts = (const float*)d_ptsv;
    FOneOut one;
    const Sampler smp = P.sampler(cfg);
    if (!f_seven(cfg) && P.last.covers(hyp, smp, d_pts, N, f_solver(cfg))) {
        // the winner's model straight from the last chunk's buffer (the same code produced it) instead
        // of a single-lane re-solve (the eigen-solve's ~0.5 ms latency)
        queue_one<FModelD>(P, s, (const FModelD*)P.models.p + (hyp - P.last.begin));
        queue_chunk_check(P, d_pts, N, s);
        MCV_HIP(hipStreamSynchronize(s));
        if (!chunk_fresh(P)) {   // the points changed since the chunk was evaluated: re-solve
            P.last.clear();
            return f_finalize(P, d_pts, N, cfg, hyp, F, d_mask, s);
        }
        std::memcpy(one.F, P.h_one.p, sizeof(FModelD));
        one.status = 1;
    } else {
        if (f_seven(cfg)) launch_f7_one(d_pts, N, smp, hyp, (FOneOut*)P.one.p, s);   // hyp = model slot
        else launch_f_one(d_pts, N, smp, hyp, (FOneOut*)P.one.p, s, fast_minimal(cfg));
        one = fetch_one<FOneOut>(P, s);
    }
    if (one.status != 1) fail("winning hypothesis %lld has no model (status %d)", (long long)hyp, one.status);
    for (int k = 0; k < 9; ++k) F[k] = one.F[k];
    return mask_count(P, s, [&](int* d_count) {
        launch_f_mask(d_pts, N, one.F, thr2_of(P, cfg), f_error_kind(cfg), d_mask, d_count, s);
    });
}

// run8Point over all correspondences: GPU fp64 sums (centroids, Euclidean distances, A^T A), then the
// 9x9 eigen-solve (JacobiImpl_), rank 2 (JacobiSVD) and de-normalisation here. Returns N, or 0 if
// degenerate (a mean distance below FLT_EPSILON, or one of the 8 largest eigenvalues below
// DBL_EPSILON).
int f_fit_all(Plan& P, const float* d_pts, int N, hipStream_t s, double* F) {
    double sums[5];
    reduce_to_host(P, s, 5, sums, [&](double* part, double* red) { h_reduce_sums(d_pts, N, nullptr, part, red, s); });
    const double n = sums[4];
    const double t = 1. / n;
    double c4[4] = {sums[0] * t, sums[1] * t, sums[2] * t, sums[3] * t};   // c2x, c2y, c1x, c1y
    double dev[2];
    reduce_to_host(P, s, 2, dev, [&](double* part, double* red) { f_reduce_eucdev(d_pts, N, nullptr, c4, part, red, s); });
    double scale2 = dev[0] * t, scale1 = dev[1] * t;
    if (scale1 < FLT_EPSILON || scale2 < FLT_EPSILON) return 0;
    scale1 = std::sqrt(2.) / scale1;
    scale2 = std::sqrt(2.) / scale2;
    double s4[4] = {scale2, scale2, scale1, scale1};
    double ata[45];
    reduce_to_host(P, s, 45, ata, [&](double* part, double* red) { f_reduce_ata(d_pts, N, nullptr, c4, s4, part, red, s); });
    double A[81], w[9], V[81];
    int o = 0;
    for (int j = 0; j < 9; ++j)
        for (int k = j; k < 9; ++k) { A[j * 9 + k] = ata[o]; A[k * 9 + j] = ata[o]; ++o; }
    jacobi_eigen(A, 9, w, V);
    int i = 0;
    for (; i < 9; ++i)
        if (std::fabs(w[i]) < DBL_EPSILON) break;
    if (i < 8) return 0;
    double F0[9];
    for (int k = 0; k < 9; ++k) F0[k] = V[8 * 9 + k];
    f_rank2(F0);
    if (!f_denormalize(F0, c4[2], c4[3], s4[2], s4[3], c4[0], c4[1], s4[0], s4[1], F)) return 0;
    return N;
}

int f_host_hypothesis(int, const float* pts4, int N, uint64_t seed, int64_t hyp, double* F9, float* Ff9,
                      int* sampleIdx, bool fast) {
    if (N < 8) fail("N < 8");
    for (int k = 0; k < 9; ++k) F9[k] = 0;
    EigWsLocal ws;
    const int st = f_hypothesis(pts4, N, Sampler{seed, nullptr}, (uint64_t)hyp, F9, sampleIdx, ws, fast);
    for (int k = 0; k < 9; ++k) Ff9[k] = (float)F9[k];
    return st;
}

// The 2-D entry's refusals that depend on the configuration: the sample size is 7 or 8.
void f_entry_refuse(const char* who, int N, const RansacConfig& cfg) {
    if (f_seven(cfg) && cfg.method == MCV_METHOD_RANSAC && N != 7 && N < 15)
        fail("%s: 7-point FM_RANSAC needs N >= 15 (OpenCV uses LMeDS below that: use method 4; N=%d)", who, N);
    if (N < f_points_cfg(cfg)) fail("%s: need at least %d correspondences (N=%d)", who, f_points_cfg(cfg), N);
}

// The 2-D entry's direct cases. 7-point at N == 7: run7Point once (the first of its models). FM_8POINT (method
// 0), and N == 8 unless it is 7-point LMedS (7-point at any N > 7 searches; the range below 15 is where
// OpenCV itself runs LMedS): run8Point on all points.
bool f_entry_direct(Plan& P, const char* who, int N, const RansacConfig& cfg, hipStream_t s, double* F) {
    if (f_seven(cfg) && N == 7) {
        launch_f7_direct(P.pts.p, (FOneOut*)P.one.p, s);
        const FOneOut one = fetch_one<FOneOut>(P, s);
        if (one.status <= 0) fail("%s: degenerate 7-point set", who);
        for (int k = 0; k < 9; ++k) F[k] = one.F[k];
        return true;
    }
    if (cfg.method != MCV_METHOD_LSQ && !(N == 8 && !(f_seven(cfg) && cfg.method == MCV_METHOD_LMEDS))) return false;
    if (f_fit_all(P, P.pts.p, N, s, F) <= 0) fail("%s: degenerate point set", who);
    return true;
}

}  // namespace mcv

using namespace mcv;

extern "C" MCV_API int cvFindFundamentalMat(const mcvV2d* a, const mcvV2d* b, const int N, const RansacConfig* cfgp,
                                            mcvM33d* F, uint8_t* mask) {
    MCV_GUARD(0, {
        return find_model_2d(MCV_MODEL_FUNDAMENTAL, "cvFindFundamentalMat", a, b, N, cfgp, F ? F->M : nullptr, mask);
    })
}

// Host build of one 7-point hypothesis (f7_hypothesis): F27 = up to 3 models, idx7 = the sample.
extern "C" MCV_API int mcvHostF7(const float* pts4, int N, uint64_t seed, int64_t hyp, double* F27, int* idx7) {
    MCV_GUARD(kStatusNoSample - 1, {
        if (!pts4 || !F27 || N < 7) fail("mcvHostF7: bad argument");
        double F[kF7Slots][9];
        for (int s = 0; s < kF7Slots; ++s)
            for (int k = 0; k < 9; ++k) F[s][k] = 0.0;
        const int n = f7_hypothesis(pts4, N, Sampler{seed, nullptr}, (uint64_t)hyp, F, idx7);
        for (int s = 0; s < kF7Slots; ++s)
            for (int k = 0; k < 9; ++k) F27[9 * s + k] = F[s][k];
        return n;
    })
}

// Host twin of the certified Sampson prefilter (sampson_pk.h) for one fp64 model over host float4 points
// {x1, y1, x2, y2}: decision[i] = 1 certified inlier, 0 certified outlier, -1 undecided; exact[i] = the
// fp64 test f_error(kind, ...) <= thr2 (kind 0 fused / 1 op-by-op Sampson). The point-set bound is the
// sweep's (max |coordinate| per column). Returns the number of decided points that differ from the
// exact test (must be 0).
extern "C" MCV_API int mcvHostSampsonCert(const float* pts4, int N, const double* F9, float thr2, int kind,
                                          int* decision, int* exact) {
    double bb[4] = {0, 0, 0, 0};
    for (int i = 0; i < N; ++i)
        for (int c = 0; c < 4; ++c) {
            const double v = pts4[4 * i + c];
            bb[c] = std::isfinite(v) ? std::fmax(bb[c], std::fabs(v)) : INFINITY;
        }
    const SampsonPkCut cut = sampson_pk_cut_host(sampson_cut(thr2));
    double Dm;
    const SampsonPkBound b = sampson_pk_bound(F9, bb[0], bb[1], bb[2], bb[3], &Dm);
    const SpkCut1 k = spk_cut1(b, Dm, cut.L32, cut.H32);
    float f[9];
    for (int j = 0; j < 9; ++j) f[j] = (float)F9[j];
    int bad = 0;
    for (int i = 0; i < N; ++i) {
        const float* q = pts4 + 4 * (size_t)i;
        const int d = spk_decide_host(f, k, q[0], q[1], q[2], q[3]);
        const int e = f_error(kind, F9, q[0], q[1], q[2], q[3]) <= thr2 ? 1 : 0;
        decision[i] = d;
        exact[i] = e;
        if (d >= 0 && d != e) ++bad;
    }
    return bad;
}
