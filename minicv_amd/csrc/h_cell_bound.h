// h_cell_bound.h — the certified per-cell inlier upper bound of the staged homography sweep. Compiled
// for gfx950 (mcv_h_stage_count's cell build, mcv_h_cell_bound) and for the host (the twin behind
// mcvTestHCellBound). Plain fp64, every operation rounded as written (-ffp-contract=off), so host and
// device agree bit for bit.
//
// The correspondences are partitioned into cells; a cell keeps the box of its points in the source
// plane, the box of their destinations and its size. For one model h and one cell, with
// w = h6 x + h7 y + 1, u = h0 x + h1 y + h2, v = h3 x + h4 y + h5 (real numbers of the fp32 model and
// coordinates): when w keeps one sign s over the source box with |w| >= 2^-10 Bw, and for one side of the
// destination box, e.g. the right one,
//     s (u - (x'max + kappa) w) > beta_x      at the four corners of the source box,
// then the op-by-op fp32 h_error of every correspondence of the cell exceeds thr2 (derivation: DESIGN.md §4,
// "The per-cell bound"). The form is affine in (x, y), so its minimum over the corners is the minimum
// over the box, and it is taken per coordinate: c + min(a xmin, a xmax) + min(b ymin, b ymax).
//   kappa^2 = (d - a_in) (1 + 2^-6)^2            a_in, d: the certified sweep's slopes (h_cert_slopes_host)
//   beta    = sqrt(b_x) (1 + 2^-6) + 8 u (G + kappa Bw)   b_x, G, Bw: h_cert_offsets' (restated below in
//             fp64 with the float round-ups bounded from above); the last term covers the 3.01 u G between
//             the sweep's fp32 DX and the real u - x' w, and the fp64 rounding of the evaluation here
//             (< 2^-48 (G + kappa Bw)).
// Nothing is certified for a model or point set outside h_cert_offsets' domain (that includes NaN and
// infinite extents), for a box that w's zero line crosses or comes near, or for an empty cell.
#pragma once

#include <math.h>
#include <stdint.h>
#include "mcv_common.h"

namespace mcv {

static const int kHCellG = 4;      // 4-D grid over (x, y, x', y') for the points the candidate rejects
static const int kHCellGs = 12;    // 2-D grid over (x, y) for the candidate's inliers
static const int kHCellMaxG = 6, kHCellMaxGs = 24;   // the largest grid the screens use
static const int kHCellInts = 9;   // per cell: min / max of x, y, x', y' (ordered-integer encoding), size
static const double kHCellSlack = 0x1p-6;
static const double kHCellWFloor = 0x1p-10;   // |w| >= kHCellWFloor * Bw at every corner

MCV_HD int h_cell_count(int G, int Gs) { return G * G * G * G + Gs * Gs; }

// Monotone map float -> int (an involution on the bit patterns): integer min / max order the floats.
MCV_HD int h_cell_enc(float f) {
    union { float f; int32_t i; } c;
    c.f = f;
    return c.i >= 0 ? c.i : (int)(c.i ^ 0x7fffffff);
}
MCV_HD float h_cell_dec(int e) {
    union { float f; int32_t i; } c;
    c.i = e >= 0 ? e : (int)(e ^ 0x7fffffff);
    return c.f;
}

// Bin of coordinate c on a grid of G bins over [-E, E], E = the point set's max |c|. A zero, infinite
// or NaN extent gives bin 0 (one-cell-wide grid); any c gets a bin in range.
MCV_HD int h_cell_bin(float c, double E, int G) {
    if (!(E > 0.0) || !(E <= 0x1p40)) return 0;
    const double t = ((double)c + E) / (2.0 * E) * (double)G;
    if (!(t >= 0.0)) return 0;
    if (t >= (double)G) return G - 1;
    return (int)t;
}

// Cell of a correspondence: [0, G^4) for the points the candidate rejects, [G^4, G^4 + Gs^2) for its inliers.
// bb = {max|x|, max|y|, max|x'|, max|y'|}.
MCV_HD int h_cell_index(float x, float y, float mx, float my, bool inlier, const double* bb, int G, int Gs) {
    if (inlier) return G * G * G * G + h_cell_bin(y, bb[1], Gs) * Gs + h_cell_bin(x, bb[0], Gs);
    return ((h_cell_bin(my, bb[3], G) * G + h_cell_bin(mx, bb[2], G)) * G + h_cell_bin(y, bb[1], G)) * G +
           h_cell_bin(x, bb[0], G);
}

// kappa of a call: from the certified sweep's slopes a_in (<= 0) and d (>= 0). Host only (a launch constant).
inline double h_cell_kappa(float a_in, float d) { return sqrt((double)d - (double)a_in) * (1.0 + kHCellSlack); }

// Per-model constants of the test. ok = h_cert_offsets' domain test (VALU form).
struct HCellModel {
    double kappa, betaX, betaY, wFloor;
    bool ok;
};

// Restates h_cert_offsets (h_cert.h, the VALU form; certT = kCertT, certSlop = kCertSlop): b_x from
// above. The float round-ups there (b_in = RU(K1), b_x = RU((K2 + b_in)(1 + slop))) are bounded by a factor
// 1 + 2^-23 each (the values are >= 2^-120: normal floats).
MCV_HD HCellModel h_cell_model(const float* h, const double* bb, float thr2, double kappa, double certT,
                               double certSlop) {
    const double X = bb[0], Y = bb[1], MX = bb[2], MY = bb[3];
    const double u = 0x1p-24, t = certT;
    const double Bu = fabs((double)h[0]) * X + fabs((double)h[1]) * Y + fabs((double)h[2]);
    const double Bv = fabs((double)h[3]) * X + fabs((double)h[4]) * Y + fabs((double)h[5]);
    const double Bw = fabs((double)h[6]) * X + fabs((double)h[7]) * Y + 1.0;
    const double Gx = Bu + MX * Bw + 0x1p-40, Gy = Bv + MY * Bw + 0x1p-40;
    const double T = (double)thr2;
    HCellModel m;
    m.ok = X <= 0x1p40 && Y <= 0x1p40 && MX <= 0x1p40 && MY <= 0x1p40 && Bw <= 0x1p50 && Gx <= 0x1p50 &&
           Gy <= 0x1p50 && T >= 0x1p-100 && T <= 0x1p20;   // false for NaN
    const double cx = 7.5 * u * Gx, cy = 7.5 * u * Gy, cw = 5.1 * u * Bw;
    const double C = cx * cx + cy * cy, Cw = cw * cw;
    const double tiny = 0x1p-120 + 0x1p-140 * Bw * Bw;
    const double K1 = (1.0 + 2 * certSlop) * ((1.0 + 1.0 / t) * C + T * Cw / t) + tiny;
    const double K2 = (1.0 + 2 * certSlop) / (1.0 - t) * (C / t + T * (1.0 + 1.0 / t) * Cw) + tiny;
    const double up = 1.0 + 0x1p-23;
    const double bx = (K2 + K1 * up) * (1.0 + certSlop) * up;   // >= the sweep's float b_x
    const double r = sqrt(bx) * (1.0 + kHCellSlack);
    m.kappa = kappa;
    m.betaX = r + 8.0 * u * (Gx + kappa * Bw);
    m.betaY = r + 8.0 * u * (Gy + kappa * Bw);
    m.wFloor = kHCellWFloor * Bw;
    return m;
}

// min over the box [x0, x1] x [y0, y1] of sg ((c0 - mm h6) x + (c1 - mm h7) y + (c2 - mm)) > beta
MCV_HD bool h_cell_side(double c0, double c1, double c2, double h6, double h7, double mm, double sg, double x0,
                        double x1, double y0, double y1, double beta) {
    const double a = sg * (c0 - mm * h6), b = sg * (c1 - mm * h7), c = sg * (c2 - mm);
    const double ax0 = a * x0, ax1 = a * x1, by0 = b * y0, by1 = b * y1;
    return (ax0 < ax1 ? ax0 : ax1) + (by0 < by1 ? by0 : by1) + c > beta;
}

// True when every correspondence of the cell is an outlier of the model. box = {xmin, xmax, ymin, ymax,
// x'min, x'max, y'min, y'max} of a non-empty cell of finite points.
MCV_HD bool h_cell_certified(const float* h, const HCellModel& m, const float* box) {
    if (!m.ok) return false;
    const double x0 = box[0], x1 = box[1], y0 = box[2], y1 = box[3];
    const double h6 = h[6], h7 = h[7];
    const double wx0 = h6 * x0, wx1 = h6 * x1, wy0 = h7 * y0, wy1 = h7 * y1;
    const double wmin = (wx0 < wx1 ? wx0 : wx1) + (wy0 < wy1 ? wy0 : wy1) + 1.0;
    const double wmax = (wx0 < wx1 ? wx1 : wx0) + (wy0 < wy1 ? wy1 : wy0) + 1.0;
    double s;
    if (wmin >= m.wFloor) s = 1.0;
    else if (wmax <= -m.wFloor) s = -1.0;
    else return false;
    const double k = m.kappa;
    const double h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3], h4 = h[4], h5 = h[5];
    const bool right = h_cell_side(h0, h1, h2, h6, h7, (double)box[5] + k, s, x0, x1, y0, y1, m.betaX);
    const bool left = h_cell_side(h0, h1, h2, h6, h7, (double)box[4] - k, -s, x0, x1, y0, y1, m.betaX);
    const bool above = h_cell_side(h3, h4, h5, h6, h7, (double)box[7] + k, s, x0, x1, y0, y1, m.betaY);
    const bool below = h_cell_side(h3, h4, h5, h6, h7, (double)box[6] - k, -s, x0, x1, y0, y1, m.betaY);
    return right || left || above || below;
}

}  // namespace mcv
