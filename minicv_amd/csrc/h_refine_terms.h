// h_refine_terms.h — one correspondence's terms of the homography refine's four fixed-order sums, and the
// step between the refit's chained passes. The single call's functors (ransac_h_refine.hip) and the batched
// call's (ransac_batch.hip) differ only in how the points, the mask and the constants reach them; the
// arithmetic is here, once, so a problem of a batch sums what its single call sums.
// Built with -ffp-contract=off: every expression rounds as written wherever it is inlined.
//
// A correspondence is (Mx, My) -> (mx, my): src -> dst, the float4 point's x, y -> z, w, promoted to double.
// Semantics restated from OpenCV 4.x calib3d/src/fundam.cpp [ext]: HomographyEstimatorCallback::runKernel
// (sums, deviations, LtL) and HomographyRefineCallback::compute (LM).
#pragma once

#include "mcv_common.h"
#include "kernels.h"

namespace mcv {

// a[5] += dst.x, dst.y, src.x, src.y, 1
MCV_HD void h_sums_terms(double Mx, double My, double mx, double my, double* a) {
    a[0] += mx; a[1] += my; a[2] += Mx; a[3] += My; a[4] += 1.0;
}

// a[4] += |dst - cm|, |src - cM|; c4 = cm.x, cm.y, cM.x, cM.y
MCV_HD void h_absdev_terms(const double* c4, double Mx, double My, double mx, double my, double* a) {
    a[0] += fabs(mx - c4[0]); a[1] += fabs(my - c4[1]);
    a[2] += fabs(Mx - c4[2]); a[3] += fabs(My - c4[3]);
}

// a[45] += the upper triangle of LtL, row-major; s4 = sm.x, sm.y, sM.x, sM.y
MCV_HD void h_ltl_terms(const double* c4, const double* s4, double Mx, double My, double mx, double my, double* a) {
    const double cmx = c4[0], cmy = c4[1], cMx = c4[2], cMy = c4[3];
    const double smx = s4[0], smy = s4[1], sMx = s4[2], sMy = s4[3];
    const double x = (mx - cmx) * smx, y = (my - cmy) * smy;
    const double X = (Mx - cMx) * sMx, Y = (My - cMy) * sMy;
    const double Lx[9] = {X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x};
    const double Ly[9] = {0, 0, 0, X, Y, 1, -y * X, -y * Y, -y};
    int o = 0;
#pragma unroll
    for (int j = 0; j < 9; ++j)
#pragma unroll
        for (int k = j; k < 9; ++k) a[o++] += Lx[j] * Lx[k] + Ly[j] * Ly[k];
}

// a[45] += JtJ upper triangle (36), Jtr (8), |r|^2 (1) at the parameters h[8]
MCV_HD void h_lm_terms(const double* h, double Mx, double My, double mx, double my, double* a) {
    double ww = h[6] * Mx + h[7] * My + 1.;
    ww = fabs(ww) > kDblEpsilon ? 1. / ww : 0;
    const double xi = (h[0] * Mx + h[1] * My + h[2]) * ww;
    const double yi = (h[3] * Mx + h[4] * My + h[5]) * ww;
    const double rx = xi - mx, ry = yi - my;
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

// Between the refit's chained passes, on one record (kernels.h kRefit*), lane k of 4: stage 0 the centroids
// after the sums, stage 1 the scales after the deviation sums. The same IEEE divisions the host half performs
// (h_refit_from_record), so the passes see bit-identical constants.
MCV_HD void refit_stats_step(double* red, int k, int stage) {
    if (stage == 0) red[kRefitC4 + k] = red[kRefitSums + k] / red[kRefitCount];
    else red[kRefitS4 + k] = red[kRefitCount] / red[kRefitDev + k];
}

}  // namespace mcv
