// h_cell_pre.h — a certified fp32 prefilter for the box test of the per-cell bound (h_cell_bound.h). Compiled
// for gfx950 (mcv_h_cell_bound, mcv_h_cell_rel) and for the host twin. For one (model, cell) it answers
// certified, not certified or undecided; an undecided pair goes to the unchanged fp64 h_cell_certified.
// Contract: a decided verdict equals h_cell_certified's for the same model, extents and cell, always, so
// everything downstream (UB, bitmaps, lists, `left`) is bit-identical with the prefilter on or off.
//
// The fp64 test compares four affine forms, minimised over the cell's source box, with beta, after a sign test
// of w against wFloor. The prefilter evaluates the same minima in fp32 about the box's centre,
//     s (u(c) - m w(c)) - |a| rx - |b| ry,    a = h0 - m h6, b = h1 - m h7, m = x'max + kappa (right side),
// with explicit fmaf (one rounding each; -ffp-contract=off keeps the rest as written, so host and device agree
// bit for bit), and decides only outside a band around the thresholds that covers every difference to the value
// the fp64 code computes ("The box test's fp32 prefilter"):
//     sides:  | fp32 value - fp64 value | <= 32 u (G + kappa Bw),  u = 2^-24, G = Bu + MX Bw (Bv, MY for y')
//     w:      | fp32 value - fp64 value | <= 16 u Bw
// Accounted: 15.1 u and 12.1 u. The band is a per-model constant, so the thresholds are six floats per model
// (rounded to the safe side) and the loop compares against registers. The bounds need the cell's box inside the
// point set's extents (it is: the extents are the maxima over the same points) and the model inside
// h_cell_model's domain; outside it the verdict is `not certified`, as h_cell_certified's first line says. NaN
// anywhere (an empty cell's box decodes to NaN) fails every comparison: undecided.
#pragma once

#include <math.h>
#include <stdint.h>
#include "mcv_common.h"
#include "h_cell_bound.h"

namespace mcv {

static const int kHCellPreFloats = 8;   // per cell: xc, yc, rx, ry, x'max + kappa, x'min - kappa, y'max + kappa, y'min - kappa
// The record list the two bound passes loop over (mcv_h_cell_pre_build): kHCellRecHead ints (the first is the
// number of records), then one record of kHCellRecInts ints per non-empty cell, in cell order: the
// kHCellPreFloats floats, the cell's size, its index in the table. One pass reads a record with two scalar loads
// and never visits an empty cell.
static const int kHCellRecHead = 4, kHCellRecInts = 12;
MCV_HD size_t h_cell_rec_ints(int cells) { return kHCellRecHead + (size_t)cells * kHCellRecInts; }
enum { kHCellPreNot = 0, kHCellPreCert = 1, kHCellPreUndecided = 2 };
static const double kHCellPreSideBand = 32 * 0x1p-24;   // of G + kappa Bw
static const double kHCellPreWBand = 16 * 0x1p-24;      // of Bw

// The neighbouring float of f, towards +inf (up) or -inf.
MCV_HD float h_pre_next(float f, bool up) {
    union { float f; uint32_t i; } c;
    c.f = f;
    if (f == 0.f) c.i = up ? 1u : 0x80000001u;
    else c.i += ((f > 0.f) == up) ? 1u : 0xFFFFFFFFu;
    return c.f;
}
// A float >= d (up) / <= d (down): the nearest float, moved one step where it fell on the wrong side. NaN stays NaN.
MCV_HD float h_pre_up(double d) {
    const float f = (float)d;
    return (double)f < d ? h_pre_next(f, true) : f;
}
MCV_HD float h_pre_dn(double d) {
    const float f = (float)d;
    return (double)f > d ? h_pre_next(f, false) : f;
}

// Per cell, once per call: the centre (a float inside the box), radii rounded outward so that the box lies inside
// centre +- radius exactly, and the four destination-side offsets (nearest float: their rounding is in the band).
MCV_HD void h_cell_pre_box(const float* box, double kappa, float* out) {
    const double x0 = box[0], x1 = box[1], y0 = box[2], y1 = box[3];
    const float xc = (float)(0.5 * (x0 + x1)), yc = (float)(0.5 * (y0 + y1));
    const double wide = 1.0 + 0x1p-40;
    const double dx = x1 - (double)xc > (double)xc - x0 ? x1 - (double)xc : (double)xc - x0;
    const double dy = y1 - (double)yc > (double)yc - y0 ? y1 - (double)yc : (double)yc - y0;
    out[0] = xc;
    out[1] = yc;
    out[2] = h_pre_up(dx * wide);
    out[3] = h_pre_up(dy * wide);
    out[4] = (float)((double)box[5] + kappa);
    out[5] = (float)((double)box[4] - kappa);
    out[6] = (float)((double)box[7] + kappa);
    out[7] = (float)((double)box[6] - kappa);
}

// Per model: the thresholds moved out of the band, rounded away from it.
struct HCellPreModel {
    float bxHi, bxLo, byHi, byLo;   // beta +- 32 u (G + kappa Bw)
    float wHi, wLo;                 // wFloor +- 16 u Bw
    bool ok;
};

MCV_HD HCellPreModel h_cell_pre_model(const HCellModel& m, const double* bb) {
    const double Gx = m.Bu + bb[2] * m.Bw + 0x1p-40, Gy = m.Bv + bb[3] * m.Bw + 0x1p-40;
    const double ex = kHCellPreSideBand * (Gx + m.kappa * m.Bw), ey = kHCellPreSideBand * (Gy + m.kappa * m.Bw);
    const double ew = kHCellPreWBand * m.Bw;
    HCellPreModel p;
    p.bxHi = h_pre_up(m.betaX + ex);
    p.bxLo = h_pre_dn(m.betaX - ex);
    p.byHi = h_pre_up(m.betaY + ey);
    p.byLo = h_pre_dn(m.betaY - ey);
    p.wHi = h_pre_up(m.wFloor + ew);
    p.wLo = h_pre_dn(m.wFloor - ew);
    p.ok = m.ok;
    return p;
}

// fp32 lower bound of sg (u - mm w) over the box: value at the centre minus |a| rx + |b| ry
MCV_HD float h_cell_pre_side(float c0, float c1, float uc, float h6, float h7, float wc, float mm, float sg, float rx,
                             float ry) {
    const float a = fmaf(-mm, h6, c0), b = fmaf(-mm, h7, c1);
    const float val = fmaf(-mm, wc, uc);
    const float rad = fmaf(fabsf(b), ry, fabsf(a) * rx);
    return fmaf(sg, val, -rad);
}

// The three-way verdict for one (model, cell). h: the fp32 model; q: the cell's kHCellPreFloats.
MCV_HD int h_cell_pre(const float* h, const HCellPreModel& p, const float* q) {
    // straight-line on purpose (bitwise & and | on the flags): the lanes of a wave rarely agree on an early exit
    const float xc = q[0], yc = q[1], rx = q[2], ry = q[3];
    const float wc = fmaf(h[6], xc, fmaf(h[7], yc, 1.f));
    const float wr = fmaf(fabsf(h[7]), ry, fabsf(h[6]) * rx);
    const float wmin = wc - wr, wmax = wc + wr;
    const bool pos = wmin >= p.wHi, neg = wmax <= -p.wHi;
    const bool zero = (wmin < p.wLo) & (wmax > -p.wLo);   // the zero line crosses the box or comes near
    const bool sign = pos | neg;                          // else the sign test itself is in its band: undecided
    const float s = pos ? 1.f : -1.f;
    const float uc = fmaf(h[0], xc, fmaf(h[1], yc, h[2]));
    const float vc = fmaf(h[3], xc, fmaf(h[4], yc, h[5]));
    const float r = h_cell_pre_side(h[0], h[1], uc, h[6], h[7], wc, q[4], s, rx, ry);
    const float l = h_cell_pre_side(h[0], h[1], uc, h[6], h[7], wc, q[5], -s, rx, ry);
    const float a = h_cell_pre_side(h[3], h[4], vc, h[6], h[7], wc, q[6], s, rx, ry);
    const float b = h_cell_pre_side(h[3], h[4], vc, h[6], h[7], wc, q[7], -s, rx, ry);
    const bool cert = sign & ((r > p.bxHi) | (l > p.bxHi) | (a > p.byHi) | (b > p.byHi));
    const bool none = sign & (r < p.bxLo) & (l < p.bxLo) & (a < p.byLo) & (b < p.byLo);
    // out of the domain, no sign, or every side clearly below beta: not certified (never together with cert:
    // the Hi thresholds lie above the Lo ones)
    if (!p.ok | zero | none) return kHCellPreNot;
    return cert ? kHCellPreCert : kHCellPreUndecided;
}

}  // namespace mcv
