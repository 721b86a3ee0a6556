// pnp_refine.h — the host arithmetic of solvePnPRansac's final solve, once, for the single call
// (pnp_host.cpp) and the batched calls (ransac_batch_pnp_host.cpp): the Levenberg-Marquardt controller of
// pnp_lm and the iteration of pnp_vvs as steppers, and the O(1) algebra between the inlier EPnP's device
// passes. Both callers feed the same sums (the single call's reductions and the batch forms of the same kernels), so a problem of a batch
// runs the same body on the same values as its single call.
#pragma once

#include "epnp.h"
#include "kernels.h"
#include "linalg.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

namespace mcv {

void rodrigues(const double* r, double* R, double* dR);   // pnp_host.cpp
void rodrigues_inv(const double* R, double* r);

inline void skew(const double* v, double* S) {
    S[0] = 0; S[1] = -v[2]; S[2] = v[1];
    S[3] = v[2]; S[4] = 0; S[5] = -v[0];
    S[6] = -v[1]; S[7] = v[0]; S[8] = 0;
}
inline void mul33(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

// Levenberg-Marquardt on (rvec, t): damping A + lambda diag(A), lambda from 1e-3 (x10 on rejection, /10 on
// acceptance), at most maxIters accepted-or-rejected steps, stop when the step is below FLT_EPSILON relative
// to the parameters or the cost stalls. request() is the point whose 28 sums (OpPnpLM with the Jacobian:
// J^T J upper triangle, J^T r, |r|^2) the caller computes; feed() takes them. The normal equations at a trial
// point ride along with its cost, so every step is one evaluation: at most maxIters + 1 in all.
struct PnpLmStepper {
    double p[6], q[6], A[36], g[6];
    double S = 0, lambda = 1e-3, dn = 0, pn = 0;
    int it = 0, maxIters = 0;
    bool first = true, done = false;

    void begin(const double* rvec, const double* t, int iters) {
        for (int k = 0; k < 3; ++k) { p[k] = rvec[k]; p[3 + k] = t[k]; }
        std::memcpy(q, p, sizeof(q));
        S = 0; lambda = 1e-3; dn = 0; pn = 0;
        it = 0; maxIters = iters;
        first = true; done = false;
    }
    bool finished() const { return done; }
    const double* request() const { return first ? p : q; }
    void feed(const double* buf28) {
        double Aq[36], gq[6];
        int o = 0;
        for (int j = 0; j < 6; ++j)
            for (int k = j; k < 6; ++k) { Aq[6 * j + k] = buf28[o]; Aq[6 * k + j] = buf28[o]; ++o; }
        for (int j = 0; j < 6; ++j) gq[j] = buf28[21 + j];
        const double Sq = buf28[27];
        if (first) {
            first = false;
            S = Sq;
            std::memcpy(A, Aq, sizeof(Aq));
            std::memcpy(g, gq, sizeof(gq));
            propose();
            return;
        }
        if (Sq < S) {
            const bool stall = (S - Sq) <= FLT_EPSILON * S;
            for (int k = 0; k < 6; ++k) p[k] = q[k];
            lambda = std::max(lambda * 0.1, 1e-12);
            S = Sq;
            std::memcpy(A, Aq, sizeof(Aq));
            std::memcpy(g, gq, sizeof(gq));
            if (stall || dn <= FLT_EPSILON * (pn + FLT_EPSILON)) { done = true; return; }
        } else {
            lambda *= 10;
            if (dn <= FLT_EPSILON * (pn + FLT_EPSILON) || lambda > 1e16) { done = true; return; }
        }
        ++it;
        propose();
    }
    void result(double* rvec, double* t) const {
        for (int k = 0; k < 3; ++k) { rvec[k] = p[k]; t[k] = p[3 + k]; }
    }

private:
    void propose() {
        if (it >= maxIters) { done = true; return; }
        double M[36], rhs[6], d[6];
        for (int k = 0; k < 36; ++k) M[k] = A[k];
        for (int k = 0; k < 6; ++k) {
            M[7 * k] = A[7 * k] + lambda * std::max(A[7 * k], DBL_EPSILON);
            rhs[k] = -g[k];
        }
        eig_solve(M, 6, rhs, d);
        dn = 0; pn = 0;
        for (int k = 0; k < 6; ++k) {
            q[k] = p[k] + d[k];
            dn = std::max(dn, std::fabs(d[k]));
            pn = std::max(pn, std::fabs(p[k]));
        }
    }
};

// Virtual visual servoing (pnp_vvs's loop body): the pose is kept as (R, t); every step takes the 28 sums of
// OpPnpVVS at it (L^T L upper triangle, L^T e, |e|^2), solves v = -lambda (L^T L)^+ L^T e and applies
// cMo <- exp(v)^-1 cMo. At most maxIters steps; the |v| < FLT_EPSILON test comes after the update.
// R / t are the point whose sums the caller computes; result() converts R back once.
struct PnpVvsStepper {
    double R[9], t[3];
    double lambda = 1.0;
    int it = 0, maxIters = 0;
    bool done = false;

    void begin(const double* rvec, const double* t0, int iters, double lam) {
        rodrigues(rvec, R, nullptr);
        for (int k = 0; k < 3; ++k) t[k] = t0[k];
        lambda = lam;
        it = 0; maxIters = iters;
        done = it >= maxIters;
    }
    bool finished() const { return done; }
    void feed(const double* buf) {
        double A[36], g[6], v[6];
        int o = 0;
        for (int j = 0; j < 6; ++j)
            for (int k = j; k < 6; ++k) { A[6 * j + k] = buf[o]; A[6 * k + j] = buf[o]; ++o; }
        for (int j = 0; j < 6; ++j) g[j] = buf[21 + j];
        eig_solve(A, 6, g, v);
        double vn = 0;
        for (int k = 0; k < 6; ++k) { v[k] = -lambda * v[k]; vn += v[k] * v[k]; }
        // T = exp(v): rotation Rodrigues(w), translation V u
        const double* u = v;
        const double* w = v + 3;
        double Rw[9], S[9], S2[9], V[9];
        rodrigues(w, Rw, nullptr);
        skew(w, S);
        mul33(S, S, S2);
        const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = std::sqrt(th2);
        const double a = th < 1e-8 ? 0.5 : (1 - std::cos(th)) / th2;
        const double b = th < 1e-8 ? 1.0 / 6.0 : (th - std::sin(th)) / (th2 * th);
        for (int k = 0; k < 9; ++k) V[k] = (k % 4 == 0 ? 1.0 : 0.0) + a * S[k] + b * S2[k];
        double tt[3];
        for (int i = 0; i < 3; ++i) tt[i] = V[3 * i] * u[0] + V[3 * i + 1] * u[1] + V[3 * i + 2] * u[2];
        // cMo <- T^-1 cMo: R' = Rw^T R, t' = Rw^T (t - tt)
        double Rn[9], tn[3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) Rn[3 * i + j] = Rw[i] * R[j] + Rw[3 + i] * R[3 + j] + Rw[6 + i] * R[6 + j];
        for (int i = 0; i < 3; ++i)
            tn[i] = Rw[i] * (t[0] - tt[0]) + Rw[3 + i] * (t[1] - tt[1]) + Rw[6 + i] * (t[2] - tt[2]);
        std::memcpy(R, Rn, sizeof(R));
        std::memcpy(t, tn, sizeof(tn));
        ++it;
        if (std::sqrt(vn) < FLT_EPSILON || it >= maxIters) done = true;
    }
    void result(double* rvec, double* tout) const {
        rodrigues_inv(R, rvec);
        for (int k = 0; k < 3; ++k) tout[k] = t[k];
    }
};

// The host algebra of epnp_device between its four read-backs, in its order:
//   first(sum, p6, n)   after {SumPw, Pw0}: control points                 -> A.C, A.c0
//   mtm(sums, p0)       after MtM: betas, sign-fixed control points        -> A.ccs, A.pw0
//   abt(pcs, abt)       after {Pc, Abt}: the three poses                   -> A.pc0, A.R, A.t
//   pick(rep3, R9, t3)  after Reproj: compute_pose's pick
// A is the argument block the next device pass reads (kernels.h EpnpPassArgs; A.cam set by the caller).
struct EpnpHostSolve {
    int n = 0;
    double sum[3] = {0, 0, 0};

    void first(EpnpPassArgs& A, const double (&s3)[3], const double (&p6)[6], int count) {
        n = count;
        for (int j = 0; j < 3; ++j) sum[j] = s3[j];
        for (int j = 0; j < 3; ++j) A.c0[j] = sum[j] / n;
        const double P3[3][3] = {{p6[0], p6[1], p6[2]}, {p6[1], p6[3], p6[4]}, {p6[2], p6[4], p6[5]}};
        epnp_control(sum, P3, n, A.C);
    }
    void mtm(EpnpPassArgs& A, const double (&m)[kMtmSums], const double (&p0)[3]) {
        EpnpBetas B;
        epnp_betas(m, A.C, B);
        double al0[4];
        epnp_alphas(A.C, p0, al0);
        for (int N = 0; N < 3; ++N) {
            epnp_ccs(B, B.betas[N + 1], A.ccs[N]);
            double pc[3];
            epnp_pc(al0, A.ccs[N], pc);
            if (pc[2] < 0.0)   // solve_for_sign on the first point; -ccs gives exactly the negated pcs
                for (int j = 0; j < 4; ++j)
                    for (int k = 0; k < 3; ++k) A.ccs[N][j][k] = -A.ccs[N][j][k];
        }
        for (int j = 0; j < 3; ++j) A.pw0[j] = sum[j] / n;
    }
    void abt(EpnpPassArgs& A, const double (&pcs)[9], const double (&ab27)[27]) {
        for (int N = 0; N < 3; ++N)
            for (int j = 0; j < 3; ++j) A.pc0[N][j] = pcs[3 * N + j] / n;
        for (int N = 0; N < 3; ++N) {
            double ab[3][3];
            for (int j = 0; j < 3; ++j)
                for (int k = 0; k < 3; ++k) ab[j][k] = ab27[9 * N + 3 * j + k];
            epnp_rt(ab, A.pc0[N], A.pw0, A.R[N], A.t[N]);
        }
    }
    void pick(const EpnpPassArgs& A, const double (&rep3)[3], double* R9, double* t3) const {
        const double rep[4] = {0, rep3[0] / n, rep3[1] / n, rep3[2] / n};
        const int N = epnp_pick(rep) - 1;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) R9[3 * i + j] = A.R[N][i][j];
            t3[i] = A.t[N][i];
        }
    }
};

// Sums of a pass's block partials part[acc * nblk + blk], in block order from 0 (as the device's derived means).
inline void epnp_block_sums(const double* part, int nacc, int nblk, double* out) {
    for (int a = 0; a < nacc; ++a) {
        double t = 0;
        for (int b = 0; b < nblk; ++b) t += part[(size_t)a * nblk + b];
        out[a] = t;
    }
}

}  // namespace mcv
