// ba_ref.h — the host side of bundle adjustment that needs no HIP: the argument checks,
// the camera-side CSR and its segments, the Levenberg-Marquardt driver shared by the device export and
// the twin, and the twin itself: ba_terms.h arithmetic summed sequentially in the orders the kernels
// use. Plain C++ over plain arrays, so a stand-alone program can run it under a sanitizer
// (tests/asan/bundle_adjust_asan_main.cpp).
#pragma once

#include "ba_terms.h"
#include "triangulate_ref.h"
#include <cstdint>
#include <cstring>
#include <vector>

namespace mcv {

static const long long kBaMaxObs = 1ll << 26;

// Mirrors of mcvBaConfig / mcvBaSummary (minicv_native.h), so that this header needs no other.
struct BaConfig {
    int maxIterations, maxCgIterations;
    double cgTolerance, initialLambda, functionTolerance, huberDelta;
};
struct BaSummary {
    double initialCost, finalCost;
    int iterations, accepted, rejected, cgIterations, usedObservations, usedTracks, termination;
};
inline BaConfig ba_default_config() { return BaConfig{50, 64, 0.1, 1e-3, 1e-6, 0.0}; }

// nullptr, or what is wrong with the configuration.
inline const char* ba_check_config(const BaConfig& c) {
    if (c.maxIterations < 0) return "negative maxIterations";
    if (c.maxCgIterations < 0) return "negative maxCgIterations";
    if (!(c.cgTolerance > 0.0) || !ba_finite(c.cgTolerance)) return "cgTolerance is not positive and finite";
    if (!(c.initialLambda > 0.0) || !ba_finite(c.initialLambda)) return "initialLambda is not positive and finite";
    if (!(c.functionTolerance >= 0.0) || !ba_finite(c.functionTolerance)) return "functionTolerance is negative or not finite";
    if (c.huberDelta != c.huberDelta) return "huberDelta is NaN";
    return nullptr;
}

// First camera with a non-finite entry, or -1.
inline int ba_check_cameras_finite(const double* cameras, int nCameras) {
    for (int j = 0; j < nCameras; ++j)
        for (int k = 0; k < 14; ++k)
            if (!ba_finite(cameras[14 * (size_t)j + k])) return j;
    return -1;
}

// The camera-side CSR: camObs lists, camera after camera, the observations of that camera in
// ascending index (a stable counting sort of cameraIdx); a camera's list is cut into segments of
// kBaSeg entries, segment s covering camObs[segStart[s] .. segEnd[s]) of camera segCam[s].
struct BaCsr {
    std::vector<int> camPtr, camObs, obsTrack, segCam, segStart, segEnd, camSegPtr;
    void swap(BaCsr& o) {
        camPtr.swap(o.camPtr);
        camObs.swap(o.camObs);
        obsTrack.swap(o.obsTrack);
        segCam.swap(o.segCam);
        segStart.swap(o.segStart);
        segEnd.swap(o.segEnd);
        camSegPtr.swap(o.camSegPtr);
    }
};

// Builds the CSR; the pass over cameraIdx is also the index check: returns the first observation whose
// camera is outside [0, nCameras), or -1.
inline long long ba_build_csr(const int* cameraIdx, const int* offsets, int T, int nCameras, BaCsr& c) {
    const int n = T > 0 ? offsets[T] : 0;
    c.camPtr.assign((size_t)nCameras + 1, 0);
    for (int k = 0; k < n; ++k) {
        if (cameraIdx[k] < 0 || cameraIdx[k] >= nCameras) return k;
        c.camPtr[(size_t)cameraIdx[k] + 1] += 1;
    }
    for (int j = 0; j < nCameras; ++j) c.camPtr[(size_t)j + 1] += c.camPtr[j];
    std::vector<int> fill(c.camPtr.begin(), c.camPtr.end() - 1);
    c.camObs.assign((size_t)n, 0);
    for (int k = 0; k < n; ++k) c.camObs[(size_t)fill[cameraIdx[k]]++] = k;
    c.obsTrack.assign((size_t)n, 0);
    for (int t = 0; t < T; ++t)
        for (int k = offsets[t]; k < offsets[t + 1]; ++k) c.obsTrack[k] = t;
    c.segCam.clear();
    c.segStart.clear();
    c.segEnd.clear();
    c.camSegPtr.assign((size_t)nCameras + 1, 0);
    for (int j = 0; j < nCameras; ++j) {
        for (int s = c.camPtr[j]; s < c.camPtr[j + 1]; s += kBaSeg) {
            c.segCam.push_back(j);
            c.segStart.push_back(s);
            c.segEnd.push_back(s + kBaSeg < c.camPtr[j + 1] ? s + kBaSeg : c.camPtr[j + 1]);
        }
        c.camSegPtr[(size_t)j + 1] = (int)c.segCam.size();
    }
    return -1;
}

// ---- the summation orders, sequentially ----

// Per point: f(k, acc) adds observation k's terms (nothing for an unused one). Up to kBaShortMax
// observations one chain from +0.0 in track order; longer, lane l of 64 chains l, l + 64, ... and the
// lanes fold as p[l] += p[l + s], s = 32 .. 1.
template <int NQ, class F>
inline void ba_host_point_sum(int o0, int R, F f, double* out) {
    if (R <= kBaShortMax) {
        for (int q = 0; q < NQ; ++q) out[q] = 0.0;
        for (int i = 0; i < R; ++i) f(o0 + i, out);
        return;
    }
    std::vector<double> lanes((size_t)64 * NQ, 0.0);
    for (int i = 0; i < R; ++i) f(o0 + i, lanes.data() + (size_t)(i % 64) * NQ);
    for (int s = 32; s >= 1; s >>= 1)
        for (int l = 0; l < s; ++l)
            for (int q = 0; q < NQ; ++q) lanes[(size_t)l * NQ + q] = lanes[(size_t)l * NQ + q] + lanes[(size_t)(l + s) * NQ + q];
    for (int q = 0; q < NQ; ++q) out[q] = lanes[q];
}

// n values v(i) over kBaSegLanes strided lanes and the tree s = 128 .. 1: the order of a segment's
// entries, of the dot products over the cameras and of the total cost.
template <int NQ, class F>
inline void ba_host_lane_sum(int n, F f, double* out) {
    std::vector<double> lanes((size_t)kBaSegLanes * NQ, 0.0);
    for (int i = 0; i < n; ++i) f(i, lanes.data() + (size_t)(i % kBaSegLanes) * NQ);
    for (int s = kBaSegLanes / 2; s >= 1; s >>= 1)
        for (int l = 0; l < s; ++l)
            for (int q = 0; q < NQ; ++q) lanes[(size_t)l * NQ + q] = lanes[(size_t)l * NQ + q] + lanes[(size_t)(l + s) * NQ + q];
    for (int q = 0; q < NQ; ++q) out[q] = lanes[q];
}

// Per camera: every segment by ba_host_lane_sum, the segments chained in order from +0.0.
template <int NQ, class F>
inline void ba_host_cam_sum(const BaCsr& c, int j, F f, double* out) {
    for (int q = 0; q < NQ; ++q) out[q] = 0.0;
    for (int s = c.camSegPtr[j]; s < c.camSegPtr[j + 1]; ++s) {
        double part[NQ];
        const int* list = c.camObs.data() + c.segStart[s];
        ba_host_lane_sum<NQ>(c.segEnd[s] - c.segStart[s], [&](int i, double* acc) { f(list[i], acc); }, part);
        for (int q = 0; q < NQ; ++q) out[q] = out[q] + part[q];
    }
}

// ---- the Levenberg-Marquardt driver, shared by the device export and the twin ----
// Backend: setup(usedObs, usedTracks); cost(cost, zok) of the current parameters; linearize();
// solve(lambda, cgIters) -> false for a failed solve; trial(cost, zok) of the step just solved;
// accept() makes the trial parameters current.
template <class Backend>
inline int ba_run(Backend& be, const BaConfig& cfg, BaSummary& sm) {
    std::memset(&sm, 0, sizeof(sm));
    be.setup(sm.usedObservations, sm.usedTracks);
    if (sm.usedTracks == 0) {
        sm.termination = kBaTermNothing;
        return 0;
    }
    double cost = 0.0;
    bool zok = true;
    be.cost(cost, zok);
    sm.initialCost = sm.finalCost = cost;
    if (cost == 0.0) {
        sm.termination = kBaTermZero;
        return 0;
    }
    double lambda = cfg.initialLambda;
    for (;;) {
        if (sm.iterations >= cfg.maxIterations) {
            sm.termination = kBaTermIterations;
            break;
        }
        be.linearize();
        bool accepted = false;
        while (!accepted && sm.termination == 0) {
            if (sm.iterations >= cfg.maxIterations) {
                sm.termination = kBaTermIterations;
                break;
            }
            int cg = 0;
            double trial = 0.0;
            bool tz = false;
            const bool ok = be.solve(lambda, cg);
            sm.cgIterations += cg;
            if (ok) be.trial(trial, tz);
            sm.iterations += 1;
            if (ok && ba_finite(trial) && tz && trial < cost) {
                be.accept();
                accepted = true;
                sm.accepted += 1;
                const double before = cost;
                cost = trial;
                sm.finalCost = cost;
                lambda = lambda / 10.0 > kBaLambdaMin ? lambda / 10.0 : kBaLambdaMin;
                if (cost == 0.0) sm.termination = kBaTermZero;
                else if (before - cost <= cfg.functionTolerance * before) sm.termination = kBaTermFunction;
            } else {
                sm.rejected += 1;
                lambda = lambda * 10.0;
                if (lambda > kBaLambdaMax) sm.termination = kBaTermLambda;
            }
        }
        if (sm.termination != 0) break;
    }
    return sm.iterations;
}

// ---- the twin ----
struct BaHost {
    BaConfig cfg;
    int nCameras = 0, T = 0, n = 0;
    const uint8_t* fixed = nullptr;
    const int* cameraIdx = nullptr;
    const double* obs = nullptr;
    const int* offsets = nullptr;
    BaCsr csr;
    std::vector<double> cams, pts, cams2, pts2;     // current and trial parameters
    std::vector<uint8_t> used, trackUsed, active;
    std::vector<double> E, W;                       // kBaEntry doubles and the weight per observation
    std::vector<double> U, g, V, h, Vinv, t, L, b;  // per camera 21 / 6, per point 6 / 3 / 6 / 3, per camera 21 / 6
    std::vector<double> x, r, z, p, q, y;
    bool solveFailed = false;

    void init(const double* cameras, int nCameras_, const uint8_t* fixed_, const int* cameraIdx_, const double* obs_,
              const int* offsets_, int T_, const double* points, const BaConfig& cfg_) {
        cfg = cfg_;
        nCameras = nCameras_;
        T = T_;
        n = T > 0 ? offsets_[T] : 0;
        fixed = fixed_;
        cameraIdx = cameraIdx_;
        obs = obs_;
        offsets = offsets_;
        cams.assign(cameras, cameras + 14 * (size_t)nCameras);
        pts.assign(points, points + 3 * (size_t)T);
        cams2 = cams;
        pts2 = pts;
    }

    void setup(int& usedObs, int& usedTracks) {
        used.assign((size_t)n, 0);
        trackUsed.assign((size_t)T, 0);
        active.assign((size_t)nCameras, 0);
        usedObs = usedTracks = 0;
        for (int tr = 0; tr < T; ++tr) {
            const double* X = pts.data() + 3 * (size_t)tr;
            const bool fin = ba_finite(X[0]) && ba_finite(X[1]) && ba_finite(X[2]);
            int cnt = 0;
            for (int k = offsets[tr]; k < offsets[tr + 1]; ++k) {
                double pc[3], r2[2];
                used[k] = fin && ba_project(cams.data() + 14 * (size_t)cameraIdx[k], X, obs[2 * (size_t)k],
                                            obs[2 * (size_t)k + 1], pc, r2);
                cnt += used[k];
            }
            if (cnt < 2) {
                for (int k = offsets[tr]; k < offsets[tr + 1]; ++k) used[k] = 0;
                continue;
            }
            trackUsed[tr] = 1;
            usedTracks += 1;
            usedObs += cnt;
            for (int k = offsets[tr]; k < offsets[tr + 1]; ++k)
                if (used[k]) active[cameraIdx[k]] = 1;
        }
        for (int j = 0; j < nCameras; ++j) active[j] = active[j] && !(fixed && fixed[j]);
        E.assign((size_t)kBaEntry * n, 0.0);
        W.assign((size_t)n, 0.0);
        U.assign(21 * (size_t)nCameras, 0.0);
        L = U;
        g.assign(6 * (size_t)nCameras, 0.0);
        b = x = r = z = p = q = g;
        V.assign(6 * (size_t)T, 0.0);
        Vinv = V;
        h.assign(3 * (size_t)T, 0.0);
        t = y = h;
    }

    void cost_of(const std::vector<double>& C, const std::vector<double>& P, double& cost, bool& zok) {
        bool allz = true;
        std::vector<double> camCost((size_t)nCameras, 0.0);
        for (int j = 0; j < nCameras; ++j)
            ba_host_cam_sum<1>(csr, j, [&](int k, double* acc) {
                if (!used[k]) return;
                bool zp;
                const double rho = ba_rho(C.data() + 14 * (size_t)j, P.data() + 3 * (size_t)csr.obsTrack[k],
                                          obs[2 * (size_t)k], obs[2 * (size_t)k + 1], cfg.huberDelta, zp);
                allz = allz && zp;
                acc[0] = acc[0] + rho;
            }, &camCost[j]);
        ba_host_lane_sum<1>(nCameras, [&](int j, double* acc) { acc[0] = acc[0] + camCost[j]; }, &cost);
        zok = allz;
    }
    void cost(double& c, bool& zok) { cost_of(cams, pts, c, zok); }

    void linearize() {
        for (int t_ = 0; t_ < T; ++t_) {
            if (!trackUsed[t_]) continue;
            double acc[9];
            ba_host_point_sum<9>(offsets[t_], offsets[t_ + 1] - offsets[t_], [&](int k, double* a) {
                if (!used[k]) return;
                double* e = E.data() + (size_t)kBaEntry * k;
                W[k] = ba_linearize(cams.data() + 14 * (size_t)cameraIdx[k], pts.data() + 3 * (size_t)t_,
                                    obs[2 * (size_t)k], obs[2 * (size_t)k + 1], cfg.huberDelta,
                                    active[cameraIdx[k]] != 0, e);
                ba_acc_point_lin(e, a);
            }, acc);
            for (int q_ = 0; q_ < 6; ++q_) V[6 * (size_t)t_ + q_] = acc[q_];
            for (int q_ = 0; q_ < 3; ++q_) h[3 * (size_t)t_ + q_] = -acc[6 + q_];
        }
        for (int j = 0; j < nCameras; ++j) {
            double acc[27];
            ba_host_cam_sum<27>(csr, j, [&](int k, double* a) {
                if (used[k]) ba_acc_cam_lin(E.data() + (size_t)kBaEntry * k, a);
            }, acc);
            for (int q_ = 0; q_ < 21; ++q_) U[21 * (size_t)j + q_] = acc[q_];
            for (int q_ = 0; q_ < 6; ++q_) g[6 * (size_t)j + q_] = -acc[21 + q_];
        }
    }

    // y_i = Vinv_i sum W_k^T v_j over the used tracks
    void point_pass(const std::vector<double>& v) {
        for (int t_ = 0; t_ < T; ++t_) {
            if (!trackUsed[t_]) continue;
            double acc[3];
            ba_host_point_sum<3>(offsets[t_], offsets[t_ + 1] - offsets[t_], [&](int k, double* a) {
                if (used[k]) ba_acc_point_wtp(E.data() + (size_t)kBaEntry * k, v.data() + 6 * (size_t)cameraIdx[k], a);
            }, acc);
            ba_symv3(Vinv.data() + 6 * (size_t)t_, acc, y.data() + 3 * (size_t)t_);
        }
    }

    void damped_u(int j, double lambda, double* Ul) const {
        for (int q_ = 0; q_ < 21; ++q_) Ul[q_] = U[21 * (size_t)j + q_];
        for (int a = 0; a < 6; ++a) Ul[ba_u6(a, a)] = ba_damp(Ul[ba_u6(a, a)], lambda);
    }

    double cam_dot(const std::vector<double>& a, const std::vector<double>& c) {
        double s;
        ba_host_lane_sum<1>(nCameras, [&](int j, double* acc) {
            acc[0] = acc[0] + ba_dot6(a.data() + 6 * (size_t)j, c.data() + 6 * (size_t)j);
        }, &s);
        return s;
    }

    // The damped reduced system at lambda and its PCG solve into x. False for a failed solve.
    bool solve(double lambda, int& cgIters) {
        cgIters = 0;
        bool fail = false;
        for (int t_ = 0; t_ < T; ++t_) {
            if (!trackUsed[t_]) continue;
            if (!ba_inv3(V.data() + 6 * (size_t)t_, lambda, Vinv.data() + 6 * (size_t)t_)) fail = true;
            ba_symv3(Vinv.data() + 6 * (size_t)t_, h.data() + 3 * (size_t)t_, t.data() + 3 * (size_t)t_);
        }
        for (int j = 0; j < nCameras; ++j) {
            double acc[27], S[21];
            ba_host_cam_sum<27>(csr, j, [&](int k, double* a) {
                if (!used[k]) return;
                const int i = csr.obsTrack[k];
                ba_acc_cam_schur(E.data() + (size_t)kBaEntry * k, Vinv.data() + 6 * (size_t)i, t.data() + 3 * (size_t)i, a);
            }, acc);
            damped_u(j, lambda, S);
            for (int q_ = 0; q_ < 21; ++q_) S[q_] = S[q_] - acc[q_];
            for (int q_ = 0; q_ < 6; ++q_) b[6 * (size_t)j + q_] = g[6 * (size_t)j + q_] - acc[21 + q_];
            if (!ba_chol6(S, L.data() + 21 * (size_t)j)) fail = true;
        }
        if (fail) return false;
        // PCG
        for (int j = 0; j < nCameras; ++j) {
            for (int a = 0; a < 6; ++a) {
                x[6 * (size_t)j + a] = 0.0;
                r[6 * (size_t)j + a] = b[6 * (size_t)j + a];
            }
            ba_chol6_solve(L.data() + 21 * (size_t)j, r.data() + 6 * (size_t)j, z.data() + 6 * (size_t)j);
            for (int a = 0; a < 6; ++a) p[6 * (size_t)j + a] = z[6 * (size_t)j + a];
        }
        double rz = cam_dot(r, z);
        const double rz0 = rz, tol2 = cfg.cgTolerance * cfg.cgTolerance;
        if (!ba_finite(rz)) return false;
        bool done = rz <= tol2 * rz0;
        while (!done && cgIters < cfg.maxCgIterations) {
            point_pass(p);
            for (int j = 0; j < nCameras; ++j) {
                double acc[6], Ul[21], up[6];
                ba_host_cam_sum<6>(csr, j, [&](int k, double* a) {
                    if (used[k]) ba_acc_cam_wy(E.data() + (size_t)kBaEntry * k, y.data() + 3 * (size_t)csr.obsTrack[k], a);
                }, acc);
                damped_u(j, lambda, Ul);
                ba_symv6(Ul, p.data() + 6 * (size_t)j, up);
                for (int a = 0; a < 6; ++a) q[6 * (size_t)j + a] = up[a] - acc[a];
            }
            const double pq = cam_dot(p, q);
            const double alpha = rz / pq;
            if (!(pq > 0.0) || !ba_finite(alpha)) return false;
            for (int j = 0; j < nCameras; ++j) {
                for (int a = 0; a < 6; ++a) {
                    x[6 * (size_t)j + a] = x[6 * (size_t)j + a] + alpha * p[6 * (size_t)j + a];
                    r[6 * (size_t)j + a] = r[6 * (size_t)j + a] - alpha * q[6 * (size_t)j + a];
                }
                ba_chol6_solve(L.data() + 21 * (size_t)j, r.data() + 6 * (size_t)j, z.data() + 6 * (size_t)j);
            }
            const double rzn = cam_dot(r, z);
            if (!ba_finite(rzn)) return false;
            const double beta = rzn / rz;
            for (size_t a = 0; a < 6 * (size_t)nCameras; ++a) p[a] = z[a] + beta * p[a];
            rz = rzn;
            cgIters += 1;
            done = rz <= tol2 * rz0;
        }
        return true;
    }

    // The step of the last solve: x for the cameras, dX_i = t_i - y_i(x) for the points, applied
    // into the trial copy. dPts (nullable) receives the point steps.
    void apply_step(double* dPts) {
        point_pass(x);
        pts2 = pts;
        for (int t_ = 0; t_ < T; ++t_) {
            for (int a = 0; a < 3; ++a) {
                const double d = trackUsed[t_] ? t[3 * (size_t)t_ + a] - y[3 * (size_t)t_ + a] : 0.0;
                if (dPts) dPts[3 * (size_t)t_ + a] = d;
                if (trackUsed[t_]) pts2[3 * (size_t)t_ + a] = pts[3 * (size_t)t_ + a] + d;
            }
        }
        cams2 = cams;
        for (int j = 0; j < nCameras; ++j)
            if (active[j]) ba_retract(cams.data() + 14 * (size_t)j, x.data() + 6 * (size_t)j, cams2.data() + 14 * (size_t)j);
    }
    void trial(double& c, bool& zok) {
        apply_step(nullptr);
        cost_of(cams2, pts2, c, zok);
    }
    void accept() {
        cams.swap(cams2);
        pts.swap(pts2);
    }
};

// The twin of cvBundleAdjust over checked arguments and their CSR (taken over). Returns the LM iterations.
inline int ba_host_bundle_adjust(const double* cameras, int nCameras, const uint8_t* fixed, const int* cameraIdx,
                                 const double* obs, const int* offsets, int T, const double* points,
                                 const BaConfig& cfg, BaCsr& csr, double* outCameras, double* outPoints,
                                 BaSummary& sm) {
    BaHost H;
    H.init(cameras, nCameras, fixed, cameraIdx, obs, offsets, T, points, cfg);
    H.csr.swap(csr);   // the CSR the caller's checks built
    const int it = ba_run(H, cfg, sm);
    if (nCameras > 0) std::memcpy(outCameras, H.cams.data(), 14 * (size_t)nCameras * sizeof(double));
    if (T > 0) std::memcpy(outPoints, H.pts.data(), 3 * (size_t)T * sizeof(double));
    return it;
}

}  // namespace mcv
