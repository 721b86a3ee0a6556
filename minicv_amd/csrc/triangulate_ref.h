// triangulate_ref.h — the host side of track triangulation that needs no HIP: the CSR checks shared
// by every export and the sequential twin of the kernels (Ray.intersection per track, hyp_rays.h
// arithmetic). Plain C++ over plain arrays, so a stand-alone program can run it under a sanitizer
// (tests/asan/triangulate_asan_main.cpp).
#pragma once

#include "hyp_rays.h"
#include <limits>
#include <vector>

#ifndef MCV_MAX_TRACK_LEN
#define MCV_MAX_TRACK_LEN 4096
#endif

namespace mcv {

// CSR offsets of T tracks: offsets[0] == 0, non-decreasing, no track over the cap.
// Returns 0, or 1 (offsets[0] != 0), 2 (decrease), 3 (over the cap) with *where = the track.
inline int tri_check_offsets(const int* offsets, int T, int* where) {
    *where = 0;
    if (offsets[0] != 0) return 1;
    for (int t = 0; t < T; ++t) {
        *where = t;
        if (offsets[t + 1] < offsets[t]) return 2;
        if (offsets[t + 1] - offsets[t] > MCV_MAX_TRACK_LEN) return 3;
    }
    return 0;
}

// First observation whose camera index is outside [0, nCameras), or -1.
inline long long tri_check_cameras(const int* cameraIdx, long long n, int nCameras) {
    for (long long i = 0; i < n; ++i)
        if (cameraIdx[i] < 0 || cameraIdx[i] >= nCameras) return i;
    return -1;
}

// Ray.intersection of one track (Utilities.fs:159-165) over rays[6 R] in input order. Writes the
// point (three quiet NaNs when no pair survives) and returns the number of midpoints folded.
// rejected (nullable) counts, per kRayPair* verdict, the pairs dropped, and in [0] the duplicates.
inline int tri_intersect_track(const double* rays, int R, double (&point)[3], long long* rejected = nullptr) {
    std::vector<int> kept;   // HashSet.ofList: the first of equal rays stays, in input order
    kept.reserve((size_t)R);
    for (int j = 0; j < R; ++j) {
        const double(&rj)[6] = *reinterpret_cast<const double(*)[6]>(rays + 6 * (size_t)j);
        bool dup = false;
        for (int i = 0; i < j && !dup; ++i)
            dup = ray_equal(*reinterpret_cast<const double(*)[6]>(rays + 6 * (size_t)i), rj);
        if (!dup) kept.push_back(j);
        else if (rejected) rejected[0] += 1;
    }
    int c = 0;
    double s[3] = {0.0, 0.0, 0.0};
    for (size_t a = 0; a < kept.size(); ++a)
        for (size_t b = a + 1; b < kept.size(); ++b) {
            double pt[3];
            const int v = ray_pair(*reinterpret_cast<const double(*)[6]>(rays + 6 * (size_t)kept[a]),
                                   *reinterpret_cast<const double(*)[6]>(rays + 6 * (size_t)kept[b]), pt);
            if (v != kRayPairOk) {
                if (rejected) rejected[v] += 1;
                continue;
            }
            c += 1;
            for (int k = 0; k < 3; ++k) s[k] = s[k] + pt[k];
        }
    for (int k = 0; k < 3; ++k) point[k] = c == 0 ? std::numeric_limits<double>::quiet_NaN() : s[k] / (double)c;
    return c;
}

// avgReprojectionError's form over one track's observations (duplicates included, input order).
inline void tri_track_stats(const double* cameras, const int* cameraIdx, const double* obs, int R,
                            const double (&point)[3], double* cost, int* visible) {
    double sum = 0.0;
    int cnt = 0;
    for (int i = 0; i < R; ++i) {
        double e;
        if (ray_project_term(cameras + 14 * (size_t)cameraIdx[i], point, obs[2 * (size_t)i], obs[2 * (size_t)i + 1], e)) {
            sum = sum + e;
            cnt += 1;
        }
    }
    if (cost) *cost = cnt == 0 ? std::numeric_limits<double>::infinity() : sum / (double)cnt;
    if (visible) *visible = cnt;
}

// All tracks of a call, rays given. Returns the number of tracks with a point.
inline int tri_host_intersect(const double* rays, const int* offsets, int T, double* points, int* pairCounts,
                              long long* rejected = nullptr) {
    int withPoint = 0;
    for (int t = 0; t < T; ++t) {
        double p[3];
        const int c = tri_intersect_track(rays + 6 * (size_t)offsets[t], offsets[t + 1] - offsets[t], p, rejected);
        for (int k = 0; k < 3; ++k) points[3 * (size_t)t + k] = p[k];
        pairCounts[t] = c;
        withPoint += c > 0;
    }
    return withPoint;
}

// All tracks of a call, observations given: unproject1 per observation, then as above.
inline int tri_host_triangulate(const double* cameras, const int* cameraIdx, const double* obs, const int* offsets,
                                int T, double* points, int* pairCounts, double* cost, int* visible) {
    int withPoint = 0;
    std::vector<double> rays;
    for (int t = 0; t < T; ++t) {
        const int o0 = offsets[t], R = offsets[t + 1] - o0;
        rays.resize(6 * (size_t)R);
        for (int i = 0; i < R; ++i)
            ray_unproject(cameras + 14 * (size_t)cameraIdx[o0 + i], obs[2 * (size_t)(o0 + i)],
                          obs[2 * (size_t)(o0 + i) + 1], *reinterpret_cast<double(*)[6]>(rays.data() + 6 * (size_t)i));
        double p[3];
        const int c = tri_intersect_track(rays.data(), R, p);
        for (int k = 0; k < 3; ++k) points[3 * (size_t)t + k] = p[k];
        pairCounts[t] = c;
        withPoint += c > 0;
        if (cost || visible)
            tri_track_stats(cameras, cameraIdx + o0, obs + 2 * (size_t)o0, R, p, cost ? cost + t : nullptr,
                            visible ? visible + t : nullptr);
    }
    return withPoint;
}

}  // namespace mcv
