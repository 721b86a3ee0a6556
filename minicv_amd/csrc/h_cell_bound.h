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
    double Bu, Bv, Bw;   // bounds of |u|, |v|, |w| over the point set's extents (the candidate-relative test's slack)
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
    m.Bu = Bu;
    m.Bv = Bv;
    m.Bw = Bw;
    return m;
}

// min over the box [x0, x1] x [y0, y1] of sg ((c0 - mm h6) x + (c1 - mm h7) y + (c2 - mm)) > beta
MCV_HD bool h_cell_side(double c0, double c1, double c2, double h6, double h7, double mm, double sg, double x0,
                        double x1, double y0, double y1, double beta) {
    const double a = sg * (c0 - mm * h6), b = sg * (c1 - mm * h7), c = sg * (c2 - mm);
    const double ax0 = a * x0, ax1 = a * x1, by0 = b * y0, by1 = b * y1;
    return (ax0 < ax1 ? ax0 : ax1) + (by0 < by1 ? by0 : by1) + c > beta;
}

// The sign of w = h6 x + h7 y + 1 over the box when |w| >= floor on all of it (+1 / -1), else 0 (the zero
// line crosses the box or comes near). wabs: the larger of |w|'s two extremes as computed.
MCV_HD double h_cell_wsign(double h6, double h7, double x0, double x1, double y0, double y1, double floor,
                           double* wabs) {
    const double wx0 = h6 * x0, wx1 = h6 * x1, wy0 = h7 * y0, wy1 = h7 * y1;
    const double wmin = (wx0 < wx1 ? wx0 : wx1) + (wy0 < wy1 ? wy0 : wy1) + 1.0;
    const double wmax = (wx0 < wx1 ? wx1 : wx0) + (wy0 < wy1 ? wy1 : wy0) + 1.0;
    if (wabs) *wabs = fabs(wmin) > fabs(wmax) ? fabs(wmin) : fabs(wmax);
    if (wmin >= floor) return 1.0;
    if (wmax <= -floor) return -1.0;
    return 0.0;
}

// True when every correspondence of the cell is an outlier of the model. box = {xmin, xmax, ymin, ymax,
// x'min, x'max, y'min, y'max} of a non-empty cell of finite points.
MCV_HD bool h_cell_certified(const float* h, const HCellModel& m, const float* box) {
    if (!m.ok) return false;
    const double x0 = box[0], x1 = box[1], y0 = box[2], y1 = box[3];
    const double h6 = h[6], h7 = h[7];
    const double s = h_cell_wsign(h6, h7, x0, x1, y0, y1, m.wFloor, nullptr);
    if (s == 0.0) return false;
    const double k = m.kappa;
    const double h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3], h4 = h[4], h5 = h[5];
    const bool right = h_cell_side(h0, h1, h2, h6, h7, (double)box[5] + k, s, x0, x1, y0, y1, m.betaX);
    const bool left = h_cell_side(h0, h1, h2, h6, h7, (double)box[4] - k, -s, x0, x1, y0, y1, m.betaX);
    const bool above = h_cell_side(h3, h4, h5, h6, h7, (double)box[7] + k, s, x0, x1, y0, y1, m.betaY);
    const bool below = h_cell_side(h3, h4, h5, h6, h7, (double)box[6] - k, -s, x0, x1, y0, y1, m.betaY);
    return right || left || above || below;
}

// ------------------------------------------------------------------------------------------
// The candidate-relative test, for the cells of the candidate's inliers (index >= G^4): every point of such a
// cell is an inlier of the candidate c under the op-by-op error. The certificate above, read for one
// correspondence (a one-point box) of c itself and turned round, says: where m_c.ok and s_c w_c >= wFloor_c,
// a candidate inlier has |x' - u_c / w_c| <= kappa + betaX_c / |w_c| (y' likewise). The right-side test of a
// model h, s (u - (x' + kappa) w) > betaX_h, falls as x' grows, so it holds for every candidate inlier of the
// cell when it holds at the largest x' the candidate allows; multiplied by s_c w_c > 0 that is, over the
// source box,
//     min [ s s_c (u w_c - u_c w) - 2 kappa (s w)(s_c w_c) ]  >  betaX_c max|w| + betaX_h max|w_c|
// (left side: the first term's sign flipped; above / below: v and betaY). Derivation: DESIGN.md §4, "The
// candidate-relative test". The bracket is a quadratic q in (x, y); about any centre (xc, yc) it is exactly
//     q(c) + q_x dx + q_y dy + Qxx dx^2 + Qxy dx dy + Qyy dy^2,
// so over |dx| <= rx, |dy| <= ry its minimum is at least
//     q(c) - |q_x| rx - |q_y| ry - (|Qxx| rx^2 + |Qxy| rx ry + |Qyy| ry^2).
// Roundings: the centre is whatever double 0.5 (x0 + x1) comes to, and the radii are taken from it and
// widened by 2^-40, so the box lies inside centre +- radius exactly. Every monomial of u w_c, u_c w and
// 2 kappa w w_c at a point of the extents is bounded by M = Bu Bw_c + Bu_c Bw + 2 kappa Bw Bw_c; the
// evaluation below sums terms whose absolute values total at most 6 M (value M, two gradient terms 2 M each,
// the second-order term M) in fewer than 40 roundings per path: an error below 40 x 6 x 2^-53 M < 2^-45 M.
// The slack is 2^-38 M. The right-hand side's own roundings, and those of the computed max|w| (absolute
// 2^-51 Bw against |w| >= 2^-10 Bw), are covered by the factor 1 + 2^-30. The slack stays below 2^-7 of the
// right-hand side (beta >= 2^-21 (G + kappa Bw), max|w| >= 2^-10 Bw), so it costs the test nothing visible.
// ------------------------------------------------------------------------------------------
struct HCellRel {
    double D[6], E[6], P[6];   // u w_c - u_c w, v w_c - v_c w, w w_c: coefficients of x^2, xy, y^2, x, y, 1
    double slackX, slackY;
    bool ok;                   // both models inside h_cert_offsets' domain
};

// q = (a0 x + a1 y + a2)(b0 x + b1 y + b2)
MCV_HD void h_cell_quad(const double* a, const double* b, double* q) {
    q[0] = a[0] * b[0];
    q[1] = a[0] * b[1] + a[1] * b[0];
    q[2] = a[1] * b[1];
    q[3] = a[0] * b[2] + a[2] * b[0];
    q[4] = a[1] * b[2] + a[2] * b[1];
    q[5] = a[2] * b[2];
}

// Per (model, candidate) constants of the relative test. m, mc: h_cell_model of the model and the candidate.
MCV_HD HCellRel h_cell_rel(const float* h, const HCellModel& m, const float* c, const HCellModel& mc) {
    const double U[3] = {h[0], h[1], h[2]}, V[3] = {h[3], h[4], h[5]}, W[3] = {h[6], h[7], 1.0};
    const double Uc[3] = {c[0], c[1], c[2]}, Vc[3] = {c[3], c[4], c[5]}, Wc[3] = {c[6], c[7], 1.0};
    HCellRel r;
    double a[6], b[6];
    h_cell_quad(U, Wc, a);
    h_cell_quad(Uc, W, b);
#pragma unroll
    for (int j = 0; j < 6; ++j) r.D[j] = a[j] - b[j];
    h_cell_quad(V, Wc, a);
    h_cell_quad(Vc, W, b);
#pragma unroll
    for (int j = 0; j < 6; ++j) r.E[j] = a[j] - b[j];
    h_cell_quad(W, Wc, r.P);
    const double k2 = 2.0 * m.kappa;
    r.slackX = 0x1p-38 * (m.Bu * mc.Bw + mc.Bu * m.Bw + k2 * m.Bw * mc.Bw);
    r.slackY = 0x1p-38 * (m.Bv * mc.Bw + mc.Bv * m.Bw + k2 * m.Bw * mc.Bw);
    r.ok = m.ok && mc.ok;
    return r;
}

// value, d/dx and d/dy of the quadratic q at (x, y)
MCV_HD void h_cell_quad_at(const double* q, double x, double y, double* val, double* gx, double* gy) {
    *val = q[0] * x * x + q[1] * x * y + q[2] * y * y + q[3] * x + q[4] * y + q[5];
    *gx = 2.0 * q[0] * x + q[1] * y + q[3];
    *gy = q[1] * x + 2.0 * q[2] * y + q[4];
}

// lower bound over the box of sg Q - k P > rhs (Q, P: quadratics with values and gradients at the centre)
MCV_HD bool h_cell_rel_side(double sg, const double* Q, double Qv, double Qx, double Qy, double k, const double* P,
                            double Pv, double Px, double Py, double rx, double ry, double rhs) {
    const double val = sg * Qv - k * Pv;
    const double gx = sg * Qx - k * Px, gy = sg * Qy - k * Py;
    const double xx = sg * Q[0] - k * P[0], xy = sg * Q[1] - k * P[1], yy = sg * Q[2] - k * P[2];
    const double low = val - fabs(gx) * rx - fabs(gy) * ry - (fabs(xx) * rx * rx + fabs(xy) * rx * ry + fabs(yy) * ry * ry);
    return low > rhs;
}

// True when every correspondence of the cell is an outlier of the model h, given that each of them is an
// inlier of the candidate c. box as in h_cell_certified (only the source box is used).
MCV_HD bool h_cell_rel_certified(const float* h, const HCellModel& m, const float* c, const HCellModel& mc,
                                 const HCellRel& r, const float* box) {
    if (!r.ok) return false;
    const double x0 = box[0], x1 = box[1], y0 = box[2], y1 = box[3];
    double wabs, wcabs;
    const double s = h_cell_wsign(h[6], h[7], x0, x1, y0, y1, m.wFloor, &wabs);
    const double sc = h_cell_wsign(c[6], c[7], x0, x1, y0, y1, mc.wFloor, &wcabs);
    if (s == 0.0 || sc == 0.0) return false;
    const double xc = 0.5 * (x0 + x1), yc = 0.5 * (y0 + y1);
    const double wide = 1.0 + 0x1p-40;
    const double rx = (x1 - xc > xc - x0 ? x1 - xc : xc - x0) * wide;
    const double ry = (y1 - yc > yc - y0 ? y1 - yc : yc - y0) * wide;
    if (!(rx <= 0x1p41) || !(ry <= 0x1p41)) return false;   // a box that is not finite
    double Dv, Dx, Dy, Ev, Ex, Ey, Pv, Px, Py;
    h_cell_quad_at(r.D, xc, yc, &Dv, &Dx, &Dy);
    h_cell_quad_at(r.E, xc, yc, &Ev, &Ex, &Ey);
    h_cell_quad_at(r.P, xc, yc, &Pv, &Px, &Py);
    const double t = s * sc, k = 2.0 * m.kappa * t;
    const double up = 1.0 + 0x1p-30;
    const double rhsX = (mc.betaX * wabs + m.betaX * wcabs) * up + r.slackX;
    const double rhsY = (mc.betaY * wabs + m.betaY * wcabs) * up + r.slackY;
    const bool right = h_cell_rel_side(t, r.D, Dv, Dx, Dy, k, r.P, Pv, Px, Py, rx, ry, rhsX);
    const bool left = h_cell_rel_side(-t, r.D, Dv, Dx, Dy, k, r.P, Pv, Px, Py, rx, ry, rhsX);
    const bool above = h_cell_rel_side(t, r.E, Ev, Ex, Ey, k, r.P, Pv, Px, Py, rx, ry, rhsY);
    const bool below = h_cell_rel_side(-t, r.E, Ev, Ex, Ey, k, r.P, Pv, Px, Py, rx, ry, rhsY);
    return right || left || above || below;
}

}  // namespace mcv
