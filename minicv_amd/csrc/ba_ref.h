// ba_ref.h — the host side of bundle adjustment that needs no HIP (focal groups §7p): the argument checks,
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

// ---- focal groups ----
struct BaFocalConfig {
    BaConfig base;
    int focalMode, pad;
};
struct BaFocalSummary {
    BaSummary base;
    int freeFocalGroups, pad;
};

// The groups of a call, numbered by their first camera: group g holds the cameras
// grpCam[grpPtr[g] .. grpPtr[g + 1]) in ascending index.
struct BaGroups {
    int nG = 0;
    std::vector<int> camGrp, grpPtr, grpCam;
    std::vector<uint8_t> grpFixed;
};

// Builds the groups and checks them: 0, or 1 unknown focalMode, 2 group value outside [0, nCameras),
// 3 unequal focal lengths within a group, 4 a free group's focal length is not finite and positive
// (fm != 0 only); *where is the camera at fault.
inline int ba_build_groups(int fm, const int* focalGroup, const uint8_t* fixedFocal, const double* cameras,
                           int nCameras, BaGroups& G, int* where) {
    *where = 0;
    if (fm < 0 || fm > 2) return 1;
    std::vector<int> idOf((size_t)nCameras, -1);
    G.camGrp.assign((size_t)nCameras, 0);
    G.nG = 0;
    for (int j = 0; j < nCameras; ++j) {
        const int v = focalGroup ? focalGroup[j] : j;
        *where = j;
        if (v < 0 || v >= nCameras) return 2;
        if (idOf[v] < 0) idOf[v] = G.nG++;
        G.camGrp[j] = idOf[v];
    }
    G.grpPtr.assign((size_t)G.nG + 1, 0);
    for (int j = 0; j < nCameras; ++j) G.grpPtr[(size_t)G.camGrp[j] + 1] += 1;
    for (int g = 0; g < G.nG; ++g) G.grpPtr[(size_t)g + 1] += G.grpPtr[g];
    std::vector<int> fill(G.grpPtr.begin(), G.grpPtr.end() - 1);
    G.grpCam.assign((size_t)nCameras, 0);
    for (int j = 0; j < nCameras; ++j) G.grpCam[(size_t)fill[G.camGrp[j]]++] = j;
    G.grpFixed.assign((size_t)G.nG, 0);
    for (int j = 0; j < nCameras; ++j)
        if (fixedFocal && fixedFocal[j]) G.grpFixed[G.camGrp[j]] = 1;
    for (int j = 0; j < nCameras; ++j) {
        const double* f = cameras + 14 * (size_t)j + 12;
        const double* f0 = cameras + 14 * (size_t)G.grpCam[G.grpPtr[G.camGrp[j]]] + 12;
        *where = j;
        if (std::memcmp(f, f0, 2 * sizeof(double)) != 0) return 3;
        if (fm != 0 && !G.grpFixed[G.camGrp[j]] && !(ba_finite(f[0]) && ba_finite(f[1]) && f[0] > 0.0 && f[1] > 0.0))
            return 4;
    }
    return 0;
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
    // focal lengths (§7p); fm == 0 leaves every line below idle
    int fm = 0, freeGroups = 0;
    BaGroups grp;
    std::vector<uint8_t> camHas, grpFree;
    std::vector<double> Ef;                                   // 2 per observation: the focal block
    std::vector<double> Gd, gf, Lf, bf, xf, rf, zf, pf, qf;   // per group 2, 2, 3, 2 ...
    bool focalBad = false;                                    // the last trial's focal lengths

    // The chain over a group's cameras, in ascending index from +0.0, of their per-camera sums.
    template <int NQ, class F>
    void group_sum(int g, F f, double* out) {
        for (int q_ = 0; q_ < NQ; ++q_) out[q_] = 0.0;
        for (int i = grp.grpPtr[g]; i < grp.grpPtr[g + 1]; ++i) {
            double part[NQ];
            ba_host_cam_sum<NQ>(csr, grp.grpCam[i], [&](int k, double* a) { f(k, a); }, part);
            for (int q_ = 0; q_ < NQ; ++q_) out[q_] = out[q_] + part[q_];
        }
    }

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
        if (fm) {
            camHas = active;
            grpFree.assign((size_t)grp.nG, 0);
            freeGroups = 0;
            for (int g = 0; g < grp.nG; ++g) {
                bool has = false;
                for (int i = grp.grpPtr[g]; i < grp.grpPtr[g + 1]; ++i) has = has || camHas[grp.grpCam[i]];
                grpFree[g] = has && !grp.grpFixed[g];
                freeGroups += grpFree[g];
            }
            Ef.assign(2 * (size_t)n, 0.0);
            Gd.assign(2 * (size_t)grp.nG, 0.0);
            gf = bf = xf = rf = zf = pf = qf = Gd;
            Lf.assign(3 * (size_t)grp.nG, 0.0);
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
                if (fm)
                    ba_linearize_focal(fm, cams.data() + 14 * (size_t)cameraIdx[k], pts.data() + 3 * (size_t)t_,
                                       obs[2 * (size_t)k], obs[2 * (size_t)k + 1], cfg.huberDelta,
                                       grpFree[grp.camGrp[cameraIdx[k]]] != 0, Ef.data() + 2 * (size_t)k);
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
        for (int g_ = 0; fm && g_ < grp.nG; ++g_) {
            double acc[4];
            group_sum<4>(g_, [&](int k, double* a) {
                if (used[k]) ba_acc_focal_lin(fm, Ef.data() + 2 * (size_t)k, E.data() + (size_t)kBaEntry * k, a);
            }, acc);
            const int nd = fm == 1 ? 1 : 2;
            for (int a = 0; a < 2; ++a) {
                Gd[2 * (size_t)g_ + a] = a < nd ? acc[a] : 0.0;
                gf[2 * (size_t)g_ + a] = a < nd ? -acc[nd + a] : 0.0;
            }
        }
    }

    // y_i = Vinv_i sum W_k^T v_j over the used tracks
    void point_pass(const std::vector<double>& v, const std::vector<double>& vf) {
        for (int t_ = 0; t_ < T; ++t_) {
            if (!trackUsed[t_]) continue;
            double acc[3];
            ba_host_point_sum<3>(offsets[t_], offsets[t_ + 1] - offsets[t_], [&](int k, double* a) {
                if (!used[k]) return;
                if (fm)
                    ba_acc_point_wtp_focal(fm, E.data() + (size_t)kBaEntry * k, Ef.data() + 2 * (size_t)k,
                                           v.data() + 6 * (size_t)cameraIdx[k],
                                           vf.data() + 2 * (size_t)grp.camGrp[cameraIdx[k]], a);
                else ba_acc_point_wtp(E.data() + (size_t)kBaEntry * k, v.data() + 6 * (size_t)cameraIdx[k], a);
            }, acc);
            ba_symv3(Vinv.data() + 6 * (size_t)t_, acc, y.data() + 3 * (size_t)t_);
        }
    }

    void damped_u(int j, double lambda, double* Ul) const {
        for (int q_ = 0; q_ < 21; ++q_) Ul[q_] = U[21 * (size_t)j + q_];
        for (int a = 0; a < 6; ++a) Ul[ba_u6(a, a)] = ba_damp(Ul[ba_u6(a, a)], lambda);
    }

    // over the cameras and, after them, the groups (af . cf)
    double cam_dot(const std::vector<double>& a, const std::vector<double>& c, const std::vector<double>& af,
                   const std::vector<double>& cf) {
        double s;
        ba_host_lane_sum<1>(nCameras + (fm ? grp.nG : 0), [&](int j, double* acc) {
            if (j < nCameras) acc[0] = acc[0] + ba_dot6(a.data() + 6 * (size_t)j, c.data() + 6 * (size_t)j);
            else acc[0] = acc[0] + ba_focal_dot(fm, af.data() + 2 * (size_t)(j - nCameras), cf.data() + 2 * (size_t)(j - nCameras));
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
        for (int g_ = 0; fm && g_ < grp.nG; ++g_) {
            double acc[kBaFocalPart];
            group_sum<kBaFocalPart>(g_, [&](int k, double* a) {
                if (!used[k]) return;
                const int i = csr.obsTrack[k];
                ba_acc_focal_schur(fm, Ef.data() + 2 * (size_t)k, E.data() + (size_t)kBaEntry * k,
                                   Vinv.data() + 6 * (size_t)i, t.data() + 3 * (size_t)i, a);
            }, acc);
            if (!ba_focal_block(fm, Gd.data() + 2 * (size_t)g_, gf.data() + 2 * (size_t)g_, acc, lambda,
                                Lf.data() + 3 * (size_t)g_, bf.data() + 2 * (size_t)g_))
                fail = true;
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
        for (int g_ = 0; fm && g_ < grp.nG; ++g_) {
            for (int a = 0; a < 2; ++a) {
                xf[2 * (size_t)g_ + a] = 0.0;
                rf[2 * (size_t)g_ + a] = bf[2 * (size_t)g_ + a];
            }
            ba_focal_solve(fm, Lf.data() + 3 * (size_t)g_, rf.data() + 2 * (size_t)g_, zf.data() + 2 * (size_t)g_);
            for (int a = 0; a < 2; ++a) pf[2 * (size_t)g_ + a] = zf[2 * (size_t)g_ + a];
        }
        double rz = cam_dot(r, z, rf, zf);
        const double rz0 = rz, tol2 = cfg.cgTolerance * cfg.cgTolerance;
        if (!ba_finite(rz)) return false;
        bool done = rz <= tol2 * rz0;
        while (!done && cgIters < cfg.maxCgIterations) {
            point_pass(p, pf);
            for (int j = 0; j < nCameras; ++j) {
                double acc[8], Ul[21], up[6];
                if (fm)
                    ba_host_cam_sum<8>(csr, j, [&](int k, double* a) {
                        if (used[k])
                            ba_acc_cam_wy_focal(fm, E.data() + (size_t)kBaEntry * k, Ef.data() + 2 * (size_t)k,
                                                y.data() + 3 * (size_t)csr.obsTrack[k], p.data() + 6 * (size_t)j,
                                                pf.data() + 2 * (size_t)grp.camGrp[j], a);
                    }, acc);
                else
                ba_host_cam_sum<6>(csr, j, [&](int k, double* a) {
                    if (used[k]) ba_acc_cam_wy(E.data() + (size_t)kBaEntry * k, y.data() + 3 * (size_t)csr.obsTrack[k], a);
                }, acc);
                damped_u(j, lambda, Ul);
                ba_symv6(Ul, p.data() + 6 * (size_t)j, up);
                for (int a = 0; a < 6; ++a) q[6 * (size_t)j + a] = up[a] - acc[a];
            }
            for (int g_ = 0; fm && g_ < grp.nG; ++g_) {
                double acc[8];
                group_sum<8>(g_, [&](int k, double* a) {
                    if (used[k])
                        ba_acc_cam_wy_focal(fm, E.data() + (size_t)kBaEntry * k, Ef.data() + 2 * (size_t)k,
                                            y.data() + 3 * (size_t)csr.obsTrack[k], p.data() + 6 * (size_t)cameraIdx[k],
                                            pf.data() + 2 * (size_t)g_, a);
                }, acc);
                ba_focal_q(fm, Gd.data() + 2 * (size_t)g_, lambda, pf.data() + 2 * (size_t)g_, acc + 6,
                           qf.data() + 2 * (size_t)g_);
            }
            const double pq = cam_dot(p, q, pf, qf);
            const double alpha = rz / pq;
            if (!(pq > 0.0) || !ba_finite(alpha)) return false;
            for (int j = 0; j < nCameras; ++j) {
                for (int a = 0; a < 6; ++a) {
                    x[6 * (size_t)j + a] = x[6 * (size_t)j + a] + alpha * p[6 * (size_t)j + a];
                    r[6 * (size_t)j + a] = r[6 * (size_t)j + a] - alpha * q[6 * (size_t)j + a];
                }
                ba_chol6_solve(L.data() + 21 * (size_t)j, r.data() + 6 * (size_t)j, z.data() + 6 * (size_t)j);
            }
            for (int g_ = 0; fm && g_ < grp.nG; ++g_) {
                for (int a = 0; a < 2; ++a) {
                    xf[2 * (size_t)g_ + a] = xf[2 * (size_t)g_ + a] + alpha * pf[2 * (size_t)g_ + a];
                    rf[2 * (size_t)g_ + a] = rf[2 * (size_t)g_ + a] - alpha * qf[2 * (size_t)g_ + a];
                }
                ba_focal_solve(fm, Lf.data() + 3 * (size_t)g_, rf.data() + 2 * (size_t)g_, zf.data() + 2 * (size_t)g_);
            }
            const double rzn = cam_dot(r, z, rf, zf);
            if (!ba_finite(rzn)) return false;
            const double beta = rzn / rz;
            for (size_t a = 0; a < 6 * (size_t)nCameras; ++a) p[a] = z[a] + beta * p[a];
            for (size_t a = 0; fm && a < 2 * (size_t)grp.nG; ++a) pf[a] = zf[a] + beta * pf[a];
            rz = rzn;
            cgIters += 1;
            done = rz <= tol2 * rz0;
        }
        return true;
    }

    // The step of the last solve: x for the cameras, dX_i = t_i - y_i(x) for the points, applied
    // into the trial copy. dPts (nullable) receives the point steps.
    void apply_step(double* dPts) {
        point_pass(x, xf);
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
        focalBad = false;
        for (int j = 0; fm && j < nCameras; ++j)
            if (grpFree[grp.camGrp[j]] &&
                !ba_focal_update(fm, cams.data() + 14 * (size_t)j + 12, xf.data() + 2 * (size_t)grp.camGrp[j],
                                 cams2.data() + 14 * (size_t)j + 12))
                focalBad = true;
    }
    void trial(double& c, bool& zok) {
        apply_step(nullptr);
        cost_of(cams2, pts2, c, zok);
        zok = zok && !focalBad;
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

// The twin of cvBundleAdjustFocal over checked arguments, their CSR and their groups (both taken over).
inline int ba_host_bundle_adjust_focal(const double* cameras, int nCameras, const uint8_t* fixed, const int* cameraIdx,
                                       const double* obs, const int* offsets, int T, const double* points,
                                       const BaFocalConfig& cfg, BaCsr& csr, BaGroups& grp, double* outCameras,
                                       double* outPoints, BaFocalSummary& sm) {
    BaHost H;
    H.init(cameras, nCameras, fixed, cameraIdx, obs, offsets, T, points, cfg.base);
    H.csr.swap(csr);
    H.fm = cfg.focalMode;
    std::swap(H.grp, grp);
    const int it = ba_run(H, cfg.base, sm.base);
    sm.freeFocalGroups = H.fm ? H.freeGroups : 0;
    sm.pad = 0;
    if (nCameras > 0) std::memcpy(outCameras, H.cams.data(), 14 * (size_t)nCameras * sizeof(double));
    if (T > 0) std::memcpy(outPoints, H.pts.data(), 3 * (size_t)T * sizeof(double));
    return it;
}

}  // namespace mcv
