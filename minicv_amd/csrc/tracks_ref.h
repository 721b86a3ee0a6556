// tracks_ref.h — the host side of track building that needs no HIP: the argument checks shared by
// cvBuildTracks and mcvHostBuildTracks, the match CSR -> node-edge list conversion, and the
// sequential twin of the kernels (union-find with union-by-smaller-id, then the classification and
// ordering of DESIGN §7l). Plain C++17 over plain arrays, so a stand-alone program can run it under
// a sanitizer (tests/asan/tracks_asan_main.cpp).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#ifndef MCV_MAX_TRACK_LEN
#define MCV_MAX_TRACK_LEN 4096
#endif

namespace mcv {

static const long long kTrkMaxTotal = 1ll << 30;   // nodes of a call, and matches of a call

inline std::string trk_msg(const char* fmt, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
    char buf[256];
    std::snprintf(buf, sizeof(buf), fmt, a, b, c, d);
    return buf;
}

// Every argument check of the exports, in one O(nImages + B + E) pass that touches no output.
// base: nImages + 1 node offsets (the exclusive prefix sum of featureCounts). edges (nullable):
// grown to 2 * offsets[B] ints once the offsets are known to be good; receives the kept matches as
// node pairs (u, v), in input order. *nKept = their number. Returns false with the message in err.
inline bool trk_prepare(const char* name, const int* featureCounts, int nImages, const int* imagePairs, int B,
                        const int* pairs, const int* offsets, const uint8_t* mask, int minLength,
                        const int* trackOffsets, int maxTracks, const int* cameraIdx, const int* featureIdx,
                        int maxObs, std::vector<int>& base, std::vector<int>* edgeBuf, long long* nKept,
                        std::string& err) {
    const std::string who = std::string(name) + ": ";
    if (!featureCounts || !imagePairs || !pairs || !offsets || !trackOffsets || !cameraIdx || !featureIdx) {
        err = who + "null featureCounts, imagePairs, pairs, offsets, trackOffsets, cameraIdx or featureIdx";
        return false;
    }
    if (nImages < 0 || B < 0) return err = who + "negative nImages or B", false;
    if (maxTracks < 0 || maxObs < 0) return err = who + "negative maxTracks or maxObs", false;
    if (minLength < 2) return err = who + trk_msg("minLength = %lld, below 2", minLength), false;
    base.assign((size_t)nImages + 1, 0);
    long long total = 0;
    for (int i = 0; i < nImages; ++i) {
        if (featureCounts[i] < 0)
            return err = who + trk_msg("featureCounts[%lld] = %lld is negative", i, featureCounts[i]), false;
        total += featureCounts[i];
        if (total > kTrkMaxTotal) return err = who + "more than 2^30 features in all", false;
        base[(size_t)i + 1] = (int)total;
    }
    if (offsets[0] != 0) return err = who + trk_msg("offsets[0] = %lld, not 0", offsets[0]), false;
    for (int p = 0; p < B; ++p) {
        if (offsets[p + 1] < offsets[p])
            return err = who + trk_msg("offsets decrease at problem %lld (%lld after %lld)", p, offsets[p + 1],
                                       offsets[p]), false;
        if (offsets[p + 1] > kTrkMaxTotal) return err = who + "more than 2^30 matches in all", false;
    }
    if (edgeBuf && edgeBuf->size() < 2 * (size_t)offsets[B]) edgeBuf->resize(2 * (size_t)offsets[B]);
    int* edges = edgeBuf ? edgeBuf->data() : nullptr;
    long long n = 0;
    for (int p = 0; p < B; ++p) {
        const int i = imagePairs[2 * (size_t)p], j = imagePairs[2 * (size_t)p + 1];
        if (i < 0 || i >= nImages || j < 0 || j >= nImages)
            return err = who + trk_msg("imagePairs of problem %lld = (%lld, %lld) outside [0, %lld)", p, i, j, nImages),
                   false;
        const int ni = featureCounts[i], nj = featureCounts[j], bi = base[(size_t)i], bj = base[(size_t)j];
        for (long long k = offsets[p]; k < offsets[p + 1]; ++k) {
            const int a = pairs[2 * k], b = pairs[2 * k + 1];
            if (a < 0 || a >= ni || b < 0 || b >= nj)   // masked-out matches are checked too
                return err = who + trk_msg("match %lld = (%lld, %lld) of problem %lld is outside its images", k, a, b, p),
                       false;
            if (mask && !mask[k]) continue;
            if (edges) {
                edges[2 * n] = bi + a;
                edges[2 * n + 1] = bj + b;
            }
            n += 1;
        }
    }
    *nKept = n;
    return true;
}

// The image of node g: the i with base[i] <= g < base[i + 1] (images without features own no node).
inline int trk_image_of(const int* base, int nImages, int g) {
    return (int)(std::upper_bound(base + 1, base + nImages + 1, g) - (base + 1));
}

struct TrkResult {
    std::vector<int> trackOffsets, cameraIdx, featureIdx, trackOfFeature;
    long long dropped[3] = {0, 0, 0};   // oversize, conflicts, short
};

// The twin: sequential union-find over the node edges (the smaller root stays the root, so a
// component's root is its smallest node), then per component, in root order: oversize, conflict
// (two nodes of one image: neighbours once the nodes are in id order), short, or a track.
inline void trk_host_build(const int* base, int nImages, const int* edges, long long nEdges, int minLength,
                           TrkResult& R) {
    const int N = base[nImages];
    std::vector<int> parent((size_t)N), size((size_t)N, 0), start;
    std::vector<uint8_t> touched((size_t)N, 0);
    for (int g = 0; g < N; ++g) parent[(size_t)g] = g;
    auto find = [&](int x) {
        while (parent[(size_t)x] != x) {
            parent[(size_t)x] = parent[(size_t)parent[(size_t)x]];
            x = parent[(size_t)x];
        }
        return x;
    };
    for (long long k = 0; k < nEdges; ++k) {
        const int u = edges[2 * k], v = edges[2 * k + 1];
        touched[(size_t)u] = touched[(size_t)v] = 1;
        const int a = find(u), b = find(v);
        if (a != b) parent[(size_t)std::max(a, b)] = std::min(a, b);
    }
    // members of every component in id order: a counting sort by root over the ascending nodes
    for (int g = 0; g < N; ++g)
        if (touched[(size_t)g]) size[(size_t)find(g)] += 1;
    start.assign((size_t)N + 1, 0);
    for (int g = 0; g < N; ++g) start[(size_t)g + 1] = start[(size_t)g] + size[(size_t)g];
    std::vector<int> members((size_t)start[(size_t)N]), fill(start.begin(), start.end() - 1);
    for (int g = 0; g < N; ++g)
        if (touched[(size_t)g]) members[(size_t)fill[(size_t)find(g)]++] = g;
    R.trackOffsets.assign(1, 0);
    R.cameraIdx.clear();
    R.featureIdx.clear();
    R.trackOfFeature.assign((size_t)N, -1);
    R.dropped[0] = R.dropped[1] = R.dropped[2] = 0;
    std::vector<int> img;
    for (int r = 0; r < N; ++r) {
        const int s = size[(size_t)r];
        if (s == 0) continue;
        if (s > MCV_MAX_TRACK_LEN) {
            R.dropped[0] += 1;
            continue;
        }
        const int* m = members.data() + start[(size_t)r];
        img.resize((size_t)s);
        bool conflict = false;
        for (int k = 0; k < s; ++k) {
            img[(size_t)k] = trk_image_of(base, nImages, m[k]);
            conflict = conflict || (k > 0 && img[(size_t)k] == img[(size_t)k - 1]);
        }
        if (conflict) {
            R.dropped[1] += 1;
            continue;
        }
        if (s < minLength) {
            R.dropped[2] += 1;
            continue;
        }
        const int t = (int)R.trackOffsets.size() - 1;
        for (int k = 0; k < s; ++k) {
            R.cameraIdx.push_back(img[(size_t)k]);
            R.featureIdx.push_back(m[k] - base[img[(size_t)k]]);
            R.trackOfFeature[(size_t)m[k]] = t;
        }
        R.trackOffsets.push_back((int)R.cameraIdx.size());
    }
}

}  // namespace mcv
