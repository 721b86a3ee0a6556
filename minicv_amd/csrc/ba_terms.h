// ba_terms.h — the arithmetic of bundle adjustment, compiled for gfx950
// (bundle_adjust.hip) and x86-64 (the twin, ba_ref.h). Everything is fp64 with + - * / and sqrt only,
// written in the one evaluation order both sides run (files are built -ffp-contract=off), so a value
// computed here has the same bits on the host and on the GPU.
//
// A camera is the 14 doubles of an mcvCamera: location c [0..2], forward [3..5], up [6..8],
// right [9..11], focal [12..13]; R has the rows (right, up, forward) and pc = R (X - c).
// A camera's six parameters are (omega, dc); R <- Q(omega) R with the Cayley map Q, c <- c + dc.
// An observation's linearisation is the 20 doubles {A (2x6, row-major), B (2x3), r (2)}, already
// scaled by sqrt(w).
#pragma once

#include "mcv_common.h"

namespace mcv {

static const int kBaEntry = 20;        // doubles per linearised observation
static const int kBaSeg = 1024;        // entries of a camera's list per segment (one workgroup)
static const int kBaSegLanes = 256;    // lanes of a segment: lane l chains entries l, l + 256, ...
static const int kBaShortMax = 64;     // tracks of at most this many observations: one chain
static const int kBaCgChunk = 8;       // PCG iterations enqueued between two reads of the solve's record
static const double kBaDampMin = 1e-6, kBaDampMax = 1e32;   // clamp of the damped diagonal
static const double kBaLambdaMin = 1e-12, kBaLambdaMax = 1e12;

// termination codes of the summary
static const int kBaTermFunction = 1, kBaTermIterations = 2, kBaTermZero = 3, kBaTermLambda = 4, kBaTermNothing = 5;

#if defined(__HIP_DEVICE_COMPILE__)
#define MCV_BA_UNROLL _Pragma("unroll")
#else
#define MCV_BA_UNROLL
#endif

MCV_HD bool ba_finite(double v) { return __builtin_fabs(v) <= 0x1.fffffffffffffp1023; }

// packed upper triangle of a symmetric 6x6 (21 values) and 3x3 (6 values), row-major, a <= b
MCV_HD int ba_u6(int a, int b) { return a * 6 - a * (a - 1) / 2 + (b - a); }
MCV_HD int ba_s6(int a, int b) { return a <= b ? ba_u6(a, b) : ba_u6(b, a); }
MCV_HD int ba_u3(int a, int b) { return a * 3 - a * (a - 1) / 2 + (b - a); }
MCV_HD int ba_s3(int a, int b) { return a <= b ? ba_u3(a, b) : ba_u3(b, a); }
// packed lower triangle of a Cholesky factor, row-major, j <= i
MCV_HD int ba_l6(int i, int j) { return i * (i + 1) / 2 + j; }

// pc = R (X - c) and the residual. True when the observation may be used: pc.z > 0, finite residual.
MCV_HD bool ba_project(const double* __restrict__ cam, const double* __restrict__ X, double ox, double oy,
                       double (&pc)[3], double (&r)[2]) {
    const double d0 = X[0] - cam[0], d1 = X[1] - cam[1], d2 = X[2] - cam[2];
    pc[0] = d0 * cam[9] + d1 * cam[10] + d2 * cam[11];
    pc[1] = d0 * cam[6] + d1 * cam[7] + d2 * cam[8];
    pc[2] = d0 * cam[3] + d1 * cam[4] + d2 * cam[5];
    r[0] = cam[12] * pc[0] / pc[2] - ox;
    r[1] = cam[13] * pc[1] / pc[2] - oy;
    return pc[2] > 0.0 && ba_finite(r[0]) && ba_finite(r[1]);
}

// The loss at a residual: the weight w and rho.
MCV_HD void ba_loss(const double (&r)[2], double delta, double& w, double& rho) {
    const double e2 = r[0] * r[0] + r[1] * r[1];
    const double e = sqrt(e2);
    if (delta <= 0.0 || e <= delta) {
        w = 1.0;
        rho = e2;
    } else {
        w = delta / e;
        rho = 2.0 * delta * e - delta * delta;
    }
}

// rho of one observation at given parameters; zpos = pc.z > 0 (the acceptance flag of a trial).
MCV_HD double ba_rho(const double* __restrict__ cam, const double* __restrict__ X, double ox, double oy,
                     double delta, bool& zpos) {
    double pc[3], r[2], w, rho;
    ba_project(cam, X, ox, oy, pc, r);
    zpos = pc[2] > 0.0;
    ba_loss(r, delta, w, rho);
    return rho;
}

// The linearisation of one used observation: e = {A, B, r} scaled by sqrt(w); A is zero for a camera
// that stays constant. Returns w.
MCV_HD double ba_linearize(const double* __restrict__ cam, const double* __restrict__ X, double ox, double oy,
                           double delta, bool active, double* __restrict__ e) {
    double pc[3], r[2], w, rho;
    ba_project(cam, X, ox, oy, pc, r);
    ba_loss(r, delta, w, rho);
    const double sw = sqrt(w);
    const double x = pc[0], y = pc[1], z = pc[2];
    const double jx = cam[12] / z, jy = cam[13] / z;
    const double kx = -(cam[12] * x / z / z), ky = -(cam[13] * y / z / z);
    double B[6];
    MCV_BA_UNROLL
    for (int c = 0; c < 3; ++c) {
        B[c] = jx * cam[9 + c] + kx * cam[3 + c];
        B[3 + c] = jy * cam[6 + c] + ky * cam[3 + c];
    }
    double A[12];
    A[0] = kx * y;
    A[1] = jx * z - kx * x;
    A[2] = -(jx * y);
    A[6] = ky * y - jy * z;
    A[7] = -(ky * x);
    A[8] = jy * x;
    MCV_BA_UNROLL
    for (int c = 0; c < 3; ++c) {
        A[3 + c] = -B[c];
        A[9 + c] = -B[3 + c];
    }
    MCV_BA_UNROLL
    for (int k = 0; k < 12; ++k) e[k] = active ? A[k] * sw : 0.0;
    MCV_BA_UNROLL
    for (int k = 0; k < 6; ++k) e[12 + k] = B[k] * sw;
    e[18] = r[0] * sw;
    e[19] = r[1] * sw;
    return w;
}

// ---- the terms an observation adds to a sum; acc[q] = acc[q] + term, one per call, in call order ----

// points, linearise: V += B^T B (6), hs += B^T r (3)
MCV_HD void ba_acc_point_lin(const double* __restrict__ e, double* __restrict__ acc) {
    const double* B = e + 12;
    MCV_BA_UNROLL
    for (int a = 0; a < 3; ++a)
        MCV_BA_UNROLL
        for (int b = a; b < 3; ++b) acc[ba_u3(a, b)] = acc[ba_u3(a, b)] + (B[a] * B[b] + B[3 + a] * B[3 + b]);
    MCV_BA_UNROLL
    for (int a = 0; a < 3; ++a) acc[6 + a] = acc[6 + a] + (B[a] * e[18] + B[3 + a] * e[19]);
}

// cameras, linearise: U += A^T A (21), gs += A^T r (6)
MCV_HD void ba_acc_cam_lin(const double* __restrict__ e, double* __restrict__ acc) {
    MCV_BA_UNROLL
    for (int a = 0; a < 6; ++a)
        MCV_BA_UNROLL
        for (int b = a; b < 6; ++b) acc[ba_u6(a, b)] = acc[ba_u6(a, b)] + (e[a] * e[b] + e[6 + a] * e[6 + b]);
    MCV_BA_UNROLL
    for (int a = 0; a < 6; ++a) acc[21 + a] = acc[21 + a] + (e[a] * e[18] + e[6 + a] * e[19]);
}

// cameras, reduced system: with C = B Vinv B^T (2x2), += A^T C A (21) and += A^T (B t) (6), t = Vinv h
MCV_HD void ba_acc_cam_schur(const double* __restrict__ e, const double* __restrict__ Vinv,
                             const double* __restrict__ t, double* __restrict__ acc) {
    const double* B = e + 12;
    double BV[6];   // B Vinv, 2x3
    MCV_BA_UNROLL
    for (int r = 0; r < 2; ++r)
        MCV_BA_UNROLL
        for (int c = 0; c < 3; ++c)
            BV[3 * r + c] = B[3 * r] * Vinv[ba_s3(0, c)] + B[3 * r + 1] * Vinv[ba_s3(1, c)] + B[3 * r + 2] * Vinv[ba_s3(2, c)];
    const double c00 = BV[0] * B[0] + BV[1] * B[1] + BV[2] * B[2];
    const double c01 = BV[0] * B[3] + BV[1] * B[4] + BV[2] * B[5];
    const double c11 = BV[3] * B[3] + BV[4] * B[4] + BV[5] * B[5];
    double CA0[6], CA1[6];   // C A, 2x6
    MCV_BA_UNROLL
    for (int a = 0; a < 6; ++a) {
        CA0[a] = c00 * e[a] + c01 * e[6 + a];
        CA1[a] = c01 * e[a] + c11 * e[6 + a];
    }
    MCV_BA_UNROLL
    for (int a = 0; a < 6; ++a)
        MCV_BA_UNROLL
        for (int b = a; b < 6; ++b) acc[ba_u6(a, b)] = acc[ba_u6(a, b)] + (e[a] * CA0[b] + e[6 + a] * CA1[b]);
    const double bt0 = B[0] * t[0] + B[1] * t[1] + B[2] * t[2];
    const double bt1 = B[3] * t[0] + B[4] * t[1] + B[5] * t[2];
    MCV_BA_UNROLL
    for (int a = 0; a < 6; ++a) acc[21 + a] = acc[21 + a] + (e[a] * bt0 + e[6 + a] * bt1);
}

// points, PCG: += W^T p = B^T (A p) (3)
MCV_HD void ba_acc_point_wtp(const double* __restrict__ e, const double* __restrict__ p, double* __restrict__ acc) {
    const double ap0 = e[0] * p[0] + e[1] * p[1] + e[2] * p[2] + e[3] * p[3] + e[4] * p[4] + e[5] * p[5];
    const double ap1 = e[6] * p[0] + e[7] * p[1] + e[8] * p[2] + e[9] * p[3] + e[10] * p[4] + e[11] * p[5];
    MCV_BA_UNROLL
    for (int a = 0; a < 3; ++a) acc[a] = acc[a] + (e[12 + a] * ap0 + e[15 + a] * ap1);
}

// cameras, PCG: += W y = A^T (B y) (6)
MCV_HD void ba_acc_cam_wy(const double* __restrict__ e, const double* __restrict__ y, double* __restrict__ acc) {
    const double by0 = e[12] * y[0] + e[13] * y[1] + e[14] * y[2];
    const double by1 = e[15] * y[0] + e[16] * y[1] + e[17] * y[2];
    MCV_BA_UNROLL
    for (int a = 0; a < 6; ++a) acc[a] = acc[a] + (e[a] * by0 + e[6 + a] * by1);
}

// ---- small dense algebra ----

MCV_HD double ba_damp(double d, double lambda) {
    const double c = d < kBaDampMin ? kBaDampMin : (d > kBaDampMax ? kBaDampMax : d);
    return d + lambda * c;
}

// y = S v for a packed symmetric 3x3 / 6x6
MCV_HD void ba_symv3(const double* __restrict__ S, const double* __restrict__ v, double* __restrict__ y) {
    MCV_BA_UNROLL
    for (int a = 0; a < 3; ++a) y[a] = S[ba_s3(a, 0)] * v[0] + S[ba_s3(a, 1)] * v[1] + S[ba_s3(a, 2)] * v[2];
}
MCV_HD void ba_symv6(const double* __restrict__ S, const double* __restrict__ v, double* __restrict__ y) {
    MCV_BA_UNROLL
    for (int a = 0; a < 6; ++a) {
        double s = S[ba_s6(a, 0)] * v[0];
        MCV_BA_UNROLL
        for (int b = 1; b < 6; ++b) s = s + S[ba_s6(a, b)] * v[b];
        y[a] = s;
    }
}

// Inverse of the damped V (packed 3x3) by Cholesky: V = L L^T, Vinv = L^-T L^-1. False when a pivot is
// not positive or a value is not finite.
MCV_HD bool ba_inv3(const double* __restrict__ V, double lambda, double* __restrict__ inv) {
    const double v00 = ba_damp(V[0], lambda), v11 = ba_damp(V[3], lambda), v22 = ba_damp(V[5], lambda);
    if (!(v00 > 0.0)) return false;
    const double l00 = sqrt(v00);
    const double l10 = V[1] / l00, l20 = V[2] / l00;
    const double d1 = v11 - l10 * l10;
    if (!(d1 > 0.0)) return false;
    const double l11 = sqrt(d1);
    const double l21 = (V[4] - l20 * l10) / l11;
    const double d2 = v22 - l20 * l20 - l21 * l21;
    if (!(d2 > 0.0)) return false;
    const double l22 = sqrt(d2);
    // M = L^-1 (lower)
    const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22;
    const double m10 = -(l10 * m00) / l11;
    const double m21 = -(l21 * m11) / l22;
    const double m20 = -(l20 * m00 + l21 * m10) / l22;
    inv[0] = m00 * m00 + m10 * m10 + m20 * m20;
    inv[1] = m10 * m11 + m20 * m21;
    inv[2] = m20 * m22;
    inv[3] = m11 * m11 + m21 * m21;
    inv[4] = m21 * m22;
    inv[5] = m22 * m22;
    bool ok = true;
    MCV_BA_UNROLL
    for (int k = 0; k < 6; ++k) ok = ok && ba_finite(inv[k]);
    return ok;
}

// Cholesky factor (packed lower, 21) of a packed symmetric 6x6. False when a pivot is not positive
// or not finite.
MCV_HD bool ba_chol6(const double* __restrict__ S, double* __restrict__ L) {
    bool ok = true;
    MCV_BA_UNROLL
    for (int j = 0; j < 6; ++j) {
        double d = S[ba_u6(j, j)];
        MCV_BA_UNROLL
        for (int k = 0; k < j; ++k) d = d - L[ba_l6(j, k)] * L[ba_l6(j, k)];
        ok = ok && d > 0.0 && ba_finite(d);
        const double l = sqrt(d);
        L[ba_l6(j, j)] = l;
        MCV_BA_UNROLL
        for (int i = j + 1; i < 6; ++i) {
            double s = S[ba_u6(j, i)];
            MCV_BA_UNROLL
            for (int k = 0; k < j; ++k) s = s - L[ba_l6(i, k)] * L[ba_l6(j, k)];
            L[ba_l6(i, j)] = s / l;
        }
    }
    return ok;
}

// z = (L L^T)^-1 r
MCV_HD void ba_chol6_solve(const double* __restrict__ L, const double* __restrict__ r, double* __restrict__ z) {
    double y[6];
    MCV_BA_UNROLL
    for (int i = 0; i < 6; ++i) {
        double s = r[i];
        MCV_BA_UNROLL
        for (int k = 0; k < i; ++k) s = s - L[ba_l6(i, k)] * y[k];
        y[i] = s / L[ba_l6(i, i)];
    }
    MCV_BA_UNROLL
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
        MCV_BA_UNROLL
        for (int k = i + 1; k < 6; ++k) s = s - L[ba_l6(k, i)] * z[k];
        z[i] = s / L[ba_l6(i, i)];
    }
}

MCV_HD double ba_dot6(const double* __restrict__ a, const double* __restrict__ b) {
    double s = a[0] * b[0];
    MCV_BA_UNROLL
    for (int k = 1; k < 6; ++k) s = s + a[k] * b[k];
    return s;
}

// The retraction of one camera by its six parameters (omega, dc): R <- Q R with the Cayley map
// Q = I + (2 / s)([a]x + [a]x^2), a = omega / 2, s = 1 + a.a; c <- c + dc. The focal lengths stay.
MCV_HD void ba_retract(const double* __restrict__ cam, const double* __restrict__ x, double* __restrict__ out) {
    const double a0 = 0.5 * x[0], a1 = 0.5 * x[1], a2 = 0.5 * x[2];
    const double aa = a0 * a0 + a1 * a1 + a2 * a2;
    const double f = 2.0 / (1.0 + aa);
    double Q[9];
    // [a]x = (0 -a2 a1; a2 0 -a0; -a1 a0 0), [a]x^2 = a a^T - (a.a) I
    Q[0] = 1.0 + f * (a0 * a0 - aa);
    Q[1] = f * (-a2 + a0 * a1);
    Q[2] = f * (a1 + a0 * a2);
    Q[3] = f * (a2 + a1 * a0);
    Q[4] = 1.0 + f * (a1 * a1 - aa);
    Q[5] = f * (-a0 + a1 * a2);
    Q[6] = f * (-a1 + a2 * a0);
    Q[7] = f * (a0 + a2 * a1);
    Q[8] = 1.0 + f * (a2 * a2 - aa);
    MCV_BA_UNROLL
    for (int c = 0; c < 3; ++c) {
        const double rt = cam[9 + c], up = cam[6 + c], fw = cam[3 + c];
        out[9 + c] = Q[0] * rt + Q[1] * up + Q[2] * fw;
        out[6 + c] = Q[3] * rt + Q[4] * up + Q[5] * fw;
        out[3 + c] = Q[6] * rt + Q[7] * up + Q[8] * fw;
        out[c] = cam[c] + x[3 + c];
    }
    out[12] = cam[12];
    out[13] = cam[13];
}

// ---- focal lengths ----
// fm = 1: one scale s per group, focal <- focal (1 + s), linearised at s = 0; fm = 2: (dfx, dfy),
// focal <- focal + (dfx, dfy). An observation's focal block is the two doubles u, scaled by sqrt(w):
// the column (u0, u1)^T for fm = 1, diag(u0, u1) for fm = 2; zero for a group that stays constant.
// A group's vectors are kept two doubles wide and its packed symmetric block three (fm = 1 uses the first).
// fm is a constant at every call, so the branches fold.

static const int kBaFocalPart = 5;   // sums of the widest focal pass: the reduced system's, fm = 2

MCV_HD void ba_linearize_focal(int fm, const double* __restrict__ cam, const double* __restrict__ X, double ox,
                               double oy, double delta, bool ffree, double* __restrict__ u) {
    double pc[3], r[2], w, rho;
    ba_project(cam, X, ox, oy, pc, r);
    ba_loss(r, delta, w, rho);
    const double sw = sqrt(w);
    const double a0 = fm == 1 ? cam[12] * pc[0] / pc[2] : pc[0] / pc[2];
    const double a1 = fm == 1 ? cam[13] * pc[1] / pc[2] : pc[1] / pc[2];
    u[0] = ffree ? a0 * sw : 0.0;
    u[1] = ffree ? a1 * sw : 0.0;
}

// linearise: the diagonal of F^T F, then F^T r (fm = 1: 1 + 1 sums, fm = 2: 2 + 2)
MCV_HD void ba_acc_focal_lin(int fm, const double* __restrict__ u, const double* __restrict__ e, double* __restrict__ acc) {
    if (fm == 1) {
        acc[0] = acc[0] + (u[0] * u[0] + u[1] * u[1]);
        acc[1] = acc[1] + (u[0] * e[18] + u[1] * e[19]);
    } else {
        acc[0] = acc[0] + u[0] * u[0];
        acc[1] = acc[1] + u[1] * u[1];
        acc[2] = acc[2] + u[0] * e[18];
        acc[3] = acc[3] + u[1] * e[19];
    }
}
MCV_HD int ba_focal_lin_sums(int fm) { return fm == 1 ? 2 : 4; }

// reduced system: with C = B Vinv B^T, F^T C F packed (1 or 3 sums), then F^T (B t) (1 or 2)
MCV_HD void ba_acc_focal_schur(int fm, const double* __restrict__ u, const double* __restrict__ e,
                               const double* __restrict__ Vinv, const double* __restrict__ t, double* __restrict__ acc) {
    const double* B = e + 12;
    double BV[6];
    MCV_BA_UNROLL
    for (int r = 0; r < 2; ++r)
        MCV_BA_UNROLL
        for (int c = 0; c < 3; ++c)
            BV[3 * r + c] = B[3 * r] * Vinv[ba_s3(0, c)] + B[3 * r + 1] * Vinv[ba_s3(1, c)] + B[3 * r + 2] * Vinv[ba_s3(2, c)];
    const double c00 = BV[0] * B[0] + BV[1] * B[1] + BV[2] * B[2];
    const double c01 = BV[0] * B[3] + BV[1] * B[4] + BV[2] * B[5];
    const double c11 = BV[3] * B[3] + BV[4] * B[4] + BV[5] * B[5];
    const double bt0 = B[0] * t[0] + B[1] * t[1] + B[2] * t[2];
    const double bt1 = B[3] * t[0] + B[4] * t[1] + B[5] * t[2];
    if (fm == 1) {
        acc[0] = acc[0] + (u[0] * (c00 * u[0] + c01 * u[1]) + u[1] * (c01 * u[0] + c11 * u[1]));
        acc[1] = acc[1] + (u[0] * bt0 + u[1] * bt1);
    } else {
        acc[0] = acc[0] + u[0] * c00 * u[0];
        acc[1] = acc[1] + u[0] * c01 * u[1];
        acc[2] = acc[2] + u[1] * c11 * u[1];
        acc[3] = acc[3] + u[0] * bt0;
        acc[4] = acc[4] + u[1] * bt1;
    }
}
MCV_HD int ba_focal_schur_sums(int fm) { return fm == 1 ? 2 : 5; }

// points, PCG: += B^T (A p + F pf) (3)
MCV_HD void ba_acc_point_wtp_focal(int fm, const double* __restrict__ e, const double* __restrict__ u,
                                   const double* __restrict__ p, const double* __restrict__ pf, double* __restrict__ acc) {
    const double ap0 = e[0] * p[0] + e[1] * p[1] + e[2] * p[2] + e[3] * p[3] + e[4] * p[4] + e[5] * p[5] + u[0] * pf[0];
    const double ap1 = e[6] * p[0] + e[7] * p[1] + e[8] * p[2] + e[9] * p[3] + e[10] * p[4] + e[11] * p[5] +
                       u[1] * pf[fm == 1 ? 0 : 1];
    MCV_BA_UNROLL
    for (int a = 0; a < 3; ++a) acc[a] = acc[a] + (e[12 + a] * ap0 + e[15 + a] * ap1);
}

// cameras and groups, PCG: += A^T (B y - F pf) (6), then += F^T (B y - A p) (1 or 2): W y together with
// the coupling of the camera's block and its group's, which no stored matrix holds
MCV_HD void ba_acc_cam_wy_focal(int fm, const double* __restrict__ e, const double* __restrict__ u,
                                const double* __restrict__ y, const double* __restrict__ p,
                                const double* __restrict__ pf, double* __restrict__ acc) {
    const double by0 = e[12] * y[0] + e[13] * y[1] + e[14] * y[2];
    const double by1 = e[15] * y[0] + e[16] * y[1] + e[17] * y[2];
    const double v0 = by0 - u[0] * pf[0], v1 = by1 - u[1] * pf[fm == 1 ? 0 : 1];
    MCV_BA_UNROLL
    for (int a = 0; a < 6; ++a) acc[a] = acc[a] + (e[a] * v0 + e[6 + a] * v1);
    const double ap0 = e[0] * p[0] + e[1] * p[1] + e[2] * p[2] + e[3] * p[3] + e[4] * p[4] + e[5] * p[5];
    const double ap1 = e[6] * p[0] + e[7] * p[1] + e[8] * p[2] + e[9] * p[3] + e[10] * p[4] + e[11] * p[5];
    const double w0 = by0 - ap0, w1 = by1 - ap1;
    if (fm == 1) {
        acc[6] = acc[6] + (u[0] * w0 + u[1] * w1);
    } else {
        acc[6] = acc[6] + u[0] * w0;
        acc[7] = acc[7] + u[1] * w1;
    }
}
MCV_HD int ba_focal_wy_sums(int fm) { return fm == 1 ? 1 : 2; }

// A group's block of the reduced system from its chained sums: S = damped diagonal - F^T C F, its
// Cholesky factor L (packed lower: l00, l10, l11) and b = gf - F^T B t. False when a pivot is not
// positive and finite.
MCV_HD bool ba_focal_block(int fm, const double* __restrict__ Gd, const double* __restrict__ gf,
                           const double* __restrict__ sums, double lambda, double* __restrict__ L,
                           double* __restrict__ b) {
    const double s00 = ba_damp(Gd[0], lambda) - sums[0];
    bool ok = s00 > 0.0 && ba_finite(s00);
    L[0] = sqrt(s00);
    if (fm == 1) {
        L[1] = 0.0;
        L[2] = 0.0;
        b[0] = gf[0] - sums[1];
        b[1] = 0.0;
        return ok;
    }
    const double s01 = -sums[1];
    const double s11 = ba_damp(Gd[1], lambda) - sums[2];
    L[1] = s01 / L[0];
    const double d = s11 - L[1] * L[1];
    ok = ok && d > 0.0 && ba_finite(d);
    L[2] = sqrt(d);
    b[0] = gf[0] - sums[3];
    b[1] = gf[1] - sums[4];
    return ok;
}

// z = (L L^T)^-1 r of a group
MCV_HD void ba_focal_solve(int fm, const double* __restrict__ L, const double* __restrict__ r, double* __restrict__ z) {
    const double y0 = r[0] / L[0];
    if (fm == 1) {
        z[0] = y0 / L[0];
        z[1] = 0.0;
        return;
    }
    const double y1 = (r[1] - L[1] * y0) / L[2];
    z[1] = y1 / L[2];
    z[0] = (y0 - L[1] * z[1]) / L[0];
}

MCV_HD double ba_focal_dot(int fm, const double* __restrict__ a, const double* __restrict__ b) {
    return fm == 1 ? a[0] * b[0] : a[0] * b[0] + a[1] * b[1];
}

// q = G_lambda pf - sums of a group, sums being the chained F^T (B y - A p)
MCV_HD void ba_focal_q(int fm, const double* __restrict__ Gd, double lambda, const double* __restrict__ pf,
                       const double* __restrict__ sums, double* __restrict__ q) {
    q[0] = ba_damp(Gd[0], lambda) * pf[0] - sums[0];
    q[1] = fm == 1 ? 0.0 : ba_damp(Gd[1], lambda) * pf[1] - sums[1];
}

// The trial focal length of a free group's camera. False when it is not finite and positive.
MCV_HD bool ba_focal_update(int fm, const double* __restrict__ focal, const double* __restrict__ xf,
                            double* __restrict__ out) {
    if (fm == 1) {
        const double s = 1.0 + xf[0];
        out[0] = focal[0] * s;
        out[1] = focal[1] * s;
    } else {
        out[0] = focal[0] + xf[0];
        out[1] = focal[1] + xf[1];
    }
    return ba_finite(out[0]) && ba_finite(out[1]) && out[0] > 0.0 && out[1] > 0.0;
}

}  // namespace mcv
