// lm_solver_step.h — lm_solver_run (lm_solver.h) as a resumable step, for callers that evaluate many
// solvers' callbacks together (the batched refine, ransac_batch_host.cpp): the solver asks for one
// evaluation at a time (request()), the caller feeds back its sums (feed()), and between the two it is
// free to run the evaluations of every other solver in the same device pass. Every operation is the one
// lm_solver_run performs, in the same order, on the same values: the two return the same bits.
#pragma once

#include "lm_solver.h"

namespace mcv {

template <int LX>
struct LmStepper {
    double x[LX], xd[LX], d[LX], v[LX], A[LX * LX], D[LX];
    double S = 0, lambda = 1, lc = 0.75;
    int iter = 0, maxIters = 0;
    bool first = true, done = false;

    void begin(const double* x0, int iters) {
        for (int i = 0; i < LX; ++i) x[i] = x0[i];
        S = 0; lambda = 1; lc = 0.75; iter = 0; maxIters = iters;
        first = true; done = false;
    }
    // The parameters the next evaluation is wanted at (valid until feed()).
    const double* request() const { return first ? x : xd; }
    bool finished() const { return done; }

    // sums: {JtJ upper triangle, Jtr, |r|^2} at request(). Returns true while another evaluation is wanted.
    bool feed(const double* sums) {
        const int lx = LX;
        const double epsx = FLT_EPSILON, epsf = FLT_EPSILON;
        const double Rlo = 0.25, Rhi = 0.75;
        if (first) {
            S = lm_unpack_sums<LX>(sums, A, v);
            for (int i = 0; i < lx; ++i) D[i] = A[i * lx + i];
            first = false;
            step();
            return true;
        }
        double Ad[LX * LX], vd[LX], Ap[LX * LX], temp_d[LX];
        const double Sd = lm_unpack_sums<LX>(sums, Ad, vd);
        for (int i = 0; i < lx; ++i) {   // temp_d = -A d + 2 v
            double acc = 0;
            for (int k = 0; k < lx; ++k) acc += A[i * lx + k] * d[k];
            temp_d[i] = -acc + 2 * v[i];
        }
        double dS = 0;
        for (int i = 0; i < lx; ++i) dS += d[i] * temp_d[i];
        const double R = (S - Sd) / (std::fabs(dS) > DBL_EPSILON ? dS : 1);
        if (R > Rhi) {
            lambda *= 0.5;
            if (lambda < lc) lambda = 0;
        } else if (R < Rlo) {
            double t = 0;
            for (int i = 0; i < lx; ++i) t += d[i] * v[i];
            double nu = (Sd - S) / (std::fabs(t) > DBL_EPSILON ? t : 1) + 2;
            nu = std::min(std::max(nu, 2.), 10.);
            if (lambda == 0) {
                eig_invert(A, lx, Ap);
                double maxval = DBL_EPSILON;
                for (int i = 0; i < lx; ++i) maxval = std::max(maxval, std::fabs(Ap[i * lx + i]));
                lambda = lc = 1. / maxval;
                nu *= 0.5;
            }
            lambda *= nu;
        }
        if (Sd < S) {
            S = Sd;
            for (int i = 0; i < lx; ++i) x[i] = xd[i];
            std::memcpy(A, Ad, sizeof(Ad));
            std::memcpy(v, vd, sizeof(vd));
        }
        ++iter;
        double dn = 0;
        for (int i = 0; i < lx; ++i) dn = std::max(dn, std::fabs(d[i]));
        const bool proceed = iter < maxIters && dn >= epsx && S >= epsf * epsf;
        if (!proceed) {
            done = true;
            return false;
        }
        step();
        return true;
    }

private:
    void step() {   // the damped solve at the current x -> the trial point xd
        const int lx = LX;
        double Ap[LX * LX];
        for (int i = 0; i < lx * lx; ++i) Ap[i] = A[i];
        for (int i = 0; i < lx; ++i) Ap[i * lx + i] += lambda * D[i];
        eig_solve(Ap, lx, v, d);
        for (int i = 0; i < lx; ++i) xd[i] = x[i] - d[i];
    }
};

}  // namespace mcv
