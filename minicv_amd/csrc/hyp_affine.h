// hyp_affine.h — one RANSAC hypothesis of the 2-D affine family: sample M correspondences, check the
// subset, solve the closed form, emit the fp32 model the inlier sweep uses. M = 3: the 6-DoF affine
// transform (cv::estimateAffine2D); M = 2: the 4-DoF similarity (cv::estimateAffinePartial2D). Compiled
// for gfx950 (ransac_a.hip) and for the host (mcvHostHypothesis, mcvHostAffineRefine). Built with
// -ffp-contract=off: every expression rounds as written, so host and device agree bit for bit.
//
// Semantics restated from OpenCV 4.x calib3d/src/ptsetreg.cpp (not present here, version unpinned;
// DESIGN.md §3, §7d):
//   * subset check   = Affine2DEstimatorCallback::checkSubset (inherited by the partial callback):
//                      haveCollinearPoints on both point sets (have_collinear_last<M>; vacuous for M = 2);
//   * minimal solver = the closed forms below, fp64 on the float inputs promoted to double, sums left to
//                      right; a non-finite model counts as no model (its errors would all be NaN);
//   * error          = computeError: fp32, model cast to float, a = F0 x + F1 y + F2 - X,
//                      b = F3 x + F4 y + F5 - Y, err = a a + b b; inlier iff err <= (float)thr^2.
#pragma once

#include "mcv_common.h"
#include "hyp_fundamental.h"   // have_collinear_last

namespace mcv {

struct AModelF { float a[6]; };   // 2x3 row-major; the similarity is stored as [S0 -S1 S2; S1 S0 S3]

template <int M>
MCV_HD bool a_check_subset(const float* sx, const float* sy, const float* dx, const float* dy) {
    return !have_collinear_last<M>(sx, sy) && !have_collinear_last<M>(dx, dy);
}

// Affine2DEstimatorCallback::runKernel on 3 correspondences (x_i, y_i) -> (X_i, Y_i).
MCV_HD void a_solve3(const float* sx, const float* sy, const float* dx, const float* dy, double* A) {
    const double x1 = sx[0], y1 = sy[0], x2 = sx[1], y2 = sy[1], x3 = sx[2], y3 = sy[2];
    const double y23 = y2 - y3, y31 = y3 - y1, y12 = y1 - y2;
    const double x32 = x3 - x2, x13 = x1 - x3, x21 = x2 - x1;
    const double c1 = x2 * y3 - x3 * y2, c2 = x3 * y1 - x1 * y3, c3 = x1 * y2 - x2 * y1;
    const double d = 1. / (x1 * y23 + x2 * y31 + x3 * y12);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 2; ++r) {
        const float* t = r == 0 ? dx : dy;
        const double X1 = t[0], X2 = t[1], X3 = t[2];
        A[3 * r + 0] = d * (X1 * y23 + X2 * y31 + X3 * y12);
        A[3 * r + 1] = d * (X1 * x32 + X2 * x13 + X3 * x21);
        A[3 * r + 2] = d * (X1 * c1 + X2 * c2 + X3 * c3);
    }
}

// AffinePartial2DEstimatorCallback::runKernel on 2 correspondences.
MCV_HD void a_solve2(const float* sx, const float* sy, const float* dx, const float* dy, double* A) {
    const double x1 = sx[0], y1 = sy[0], x2 = sx[1], y2 = sy[1];
    const double X1 = dx[0], Y1 = dy[0], X2 = dx[1], Y2 = dy[1];
    const double ex = x1 - x2, ey = y1 - y2, eX = X1 - X2, eY = Y1 - Y2;
    const double c = x1 * y2 - x2 * y1;
    const double d = 1. / (ex * ex + ey * ey);
    const double S0 = d * (eX * ex + eY * ey);
    const double S1 = d * (eY * ex - eX * ey);
    const double S2 = d * (eY * c - (X1 * y2 - X2 * y1) * ey - (X1 * x2 - X2 * x1) * ex);
    const double S3 = d * (-eX * c - (Y1 * x2 - Y2 * x1) * ex - (Y1 * y2 - Y2 * y1) * ey);
    A[0] = S0; A[1] = -S1; A[2] = S2;
    A[3] = S1; A[4] = S0; A[5] = S3;
}

// The fp32 sweep model; false when an entry of either form is not finite.
MCV_HD bool a_model_f(const double* A, AModelF* mf) {
    bool ok = true;
    for (int i = 0; i < 6; ++i) {
        mf->a[i] = (float)A[i];
        ok = ok && isfinite(A[i]) && isfinite(mf->a[i]);
    }
    return ok;
}

template <int M>
MCV_HD bool a_solve(const float* sx, const float* sy, const float* dx, const float* dy, double* A, AModelF* mf) {
    if constexpr (M == 3) a_solve3(sx, sy, dx, dy, A);
    else a_solve2(sx, sy, dx, dy, A);
    return a_model_f(A, mf);
}

// The sample search: getSubset attempts with the subset check (none for a tabled sampler). False = the
// sampler is exhausted (OpenCV's `break`).
template <int M>
MCV_HD bool a_sample(const float* pts4, int N, const Sampler& smp, uint64_t hyp, float* sx, float* sy, float* dx,
                     float* dy, int* idx) {
    SubsetSrc<M> src(smp, hyp);
    for (int attempt = 0; attempt < kMaxAttempts; ++attempt) {
        const int got = src.next(N, *reinterpret_cast<int(*)[M]>(idx));
        if (got < 0) break;
        if (got == 0) continue;
        for (int i = 0; i < M; ++i) {
            const float* p = pts4 + 4 * (int64_t)idx[i];
            sx[i] = p[0]; sy[i] = p[1]; dx[i] = p[2]; dy[i] = p[3];
        }
        if (!src.tabled() && !a_check_subset<M>(sx, sy, dx, dy)) continue;
        return true;
    }
    return false;
}

// One hypothesis: 1 (model written), kStatusNoModel, or kStatusNoSample. pts4: N packed {x, y, X, Y}.
// direct: the first M correspondences as they are (the N == M call: one runKernel, no subset check).
template <int M>
MCV_HD int a_hypothesis(const float* pts4, int N, const Sampler& smp, uint64_t hyp, double* A, AModelF* mf,
                        int* idx_out, bool direct = false) {
    float sx[M], sy[M], dx[M], dy[M];
    int idx[M];
    if (direct) {
        for (int i = 0; i < M; ++i) {
            idx[i] = i;
            sx[i] = pts4[4 * i]; sy[i] = pts4[4 * i + 1]; dx[i] = pts4[4 * i + 2]; dy[i] = pts4[4 * i + 3];
        }
    } else if (!a_sample<M>(pts4, N, smp, hyp, sx, sy, dx, dy, idx)) {
        return kStatusNoSample;
    }
    if (idx_out) for (int i = 0; i < M; ++i) idx_out[i] = idx[i];
    return a_solve<M>(sx, sy, dx, dy, A, mf) ? 1 : kStatusNoModel;
}

// computeError for one correspondence, two bit-level definitions (as for the homography, hyp_homography.h):
//   op by op (default): a = ((F0 x + F1 y) + F2) - X, b likewise, e = a a + b b, every operation rounded;
//   fused (MCV_FLAG_FUSED_ERROR): a = fma(F0, x, fma(F1, y, F2)) - X; b = fma(F3, x, fma(F4, y, F5)) - Y;
//                                 e = fma(a, a, b * b).
// Nothing divides: the packed sweep (ransac_a.hip) evaluates either form exactly, operation by operation.
MCV_HD float a_error(const float* f, float x, float y, float X, float Y) {
    const float a = f[0] * x + f[1] * y + f[2] - X;
    const float b = f[3] * x + f[4] * y + f[5] - Y;
    return a * a + b * b;
}

MCV_HD float a_error_fused(const float* f, float x, float y, float X, float Y) {
    const float a = fmaf(f[0], x, fmaf(f[1], y, f[2])) - X;
    const float b = fmaf(f[3], x, fmaf(f[4], y, f[5])) - Y;
    return fmaf(a, a, b * b);
}

// Refine callbacks (Affine2DRefineCallback: 6 parameters h0..h5; AffinePartial2DRefineCallback: 4
// parameters a, b, tx, ty): one correspondence's terms of JtJ (upper triangle, row-major), Jtr and
// |r|^2, added to acc[LX (LX + 1) / 2 + LX + 1] in that order.
template <int LX>
MCV_HD void a_lm_terms(const double* h, double x, double y, double X, double Y, double* acc) {
    double Jx[LX], Jy[LX], rx, ry;
    if constexpr (LX == 6) {
        rx = h[0] * x + h[1] * y + h[2] - X;
        ry = h[3] * x + h[4] * y + h[5] - Y;
        Jx[0] = x; Jx[1] = y; Jx[2] = 1; Jx[3] = 0; Jx[4] = 0; Jx[5] = 0;
        Jy[0] = 0; Jy[1] = 0; Jy[2] = 0; Jy[3] = x; Jy[4] = y; Jy[5] = 1;
    } else {
        rx = h[0] * x - h[1] * y + h[2] - X;
        ry = h[1] * x + h[0] * y + h[3] - Y;
        Jx[0] = x; Jx[1] = -y; Jx[2] = 1; Jx[3] = 0;
        Jy[0] = y; Jy[1] = x; Jy[2] = 0; Jy[3] = 1;
    }
    int o = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < LX; ++j)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int k = j; k < LX; ++k) acc[o++] += Jx[j] * Jx[k] + Jy[j] * Jy[k];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < LX; ++j) acc[o++] += Jx[j] * rx + Jy[j] * ry;
    acc[o] += rx * rx + ry * ry;
}

MCV_HD constexpr int a_lm_values(int lx) { return lx * (lx + 1) / 2 + lx + 1; }   // 28 (affine), 15 (similarity)

// 2x3 matrix <-> the refine's parameters (similarity: a, b, tx, ty of [a -b tx; b a ty]); host side.
inline void a_to_params(int lx, const double* A, double* h) {
    if (lx == 6) for (int i = 0; i < 6; ++i) h[i] = A[i];
    else { h[0] = A[0]; h[1] = A[3]; h[2] = A[2]; h[3] = A[5]; }
}
inline void a_from_params(int lx, const double* h, double* A) {
    if (lx == 6) for (int i = 0; i < 6; ++i) A[i] = h[i];
    else { A[0] = h[0]; A[1] = -h[1]; A[2] = h[2]; A[3] = h[1]; A[4] = h[0]; A[5] = h[3]; }
}

}  // namespace mcv
