// sift_ref.h — SIFT detection on the host: the argument checks and the plan (sizes, blur
// taps) that cvDetectFeatures and its twin share, and the twin itself, a sequential walk through the
// specification that shares only the per-sample arithmetic of sift_math.h with the kernels. No HIP.
#pragma once

#include "sift_math.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

namespace mcv {

// SiftConfig as the caller passes it (include/minicv_native.h declares the same 40 bytes).
struct SiftConfigIn {
    int FeatureCount, OctaveLayers;
    double ContrastThreshold, EdgeThreshold, Sigma;
    int DescriptorType;
};

struct SiftPlan {
    SiftParams P;
    int featureCount = 0, descType = 0;
    int w = 0, h = 0, channels = 1;         // input
    int nOctaves = 0;
    std::vector<int> ow, oh;                // octave sizes
    std::vector<size_t> obase;              // float offset of an octave's first Gaussian image
    size_t pyramidFloats = 0;
    // blur b = 0: the base blur; b = i: Gaussian image i from i - 1 (i = 1 .. nl + 2)
    std::vector<float> taps;
    std::vector<int> tapOff, tapRadius;
};

inline bool sift_fail(std::string& err, const char* name, const char* what) {
    err = std::string(name) + ": " + what;
    return false;
}

inline bool sift_plan(const char* name, const void* data, int width, int height, int channels, int mode,
                      const void* config, SiftPlan& S, std::string& err) {
    char buf[160];
    if (mode != 4) {
        snprintf(buf, sizeof buf, "mode %d is outside the MI355X hot path: only SIFT (mode 4) is built (DESIGN 7n)",
                 mode);
        return sift_fail(err, name, buf);
    }
    if (!data) return sift_fail(err, name, "null image");
    if (width <= 0 || height <= 0) return sift_fail(err, name, "width and height must be positive");
    if (width > kSiftMaxSide || height > kSiftMaxSide) {
        snprintf(buf, sizeof buf, "width and height are capped at %d", kSiftMaxSide);
        return sift_fail(err, name, buf);
    }
    if (channels != 1 && channels != 3 && channels != 4) return sift_fail(err, name, "channels must be 1, 3 or 4");
    SiftConfigIn c = {0, 3, 0.04, 10.0, 1.6, 0};
    if (config) c = *(const SiftConfigIn*)config;
    if (c.OctaveLayers < kSiftMinLayers || c.OctaveLayers > kSiftMaxLayers) {
        snprintf(buf, sizeof buf, "OctaveLayers must lie in %d..%d", kSiftMinLayers, kSiftMaxLayers);
        return sift_fail(err, name, buf);
    }
    if (!(c.Sigma > 0.0) || !(c.Sigma <= kSiftMaxSigma)) return sift_fail(err, name, "Sigma must lie in (0, 4]");
    if (!(c.ContrastThreshold >= 0.0) || !(c.ContrastThreshold <= 1e6))
        return sift_fail(err, name, "ContrastThreshold must be >= 0 (and finite)");
    if (!(c.EdgeThreshold > 0.0) || !(c.EdgeThreshold <= 1e6))
        return sift_fail(err, name, "EdgeThreshold must be > 0 (and finite)");
    if (c.DescriptorType != 0 && c.DescriptorType != 5)
        return sift_fail(err, name, "DescriptorType must be 0 (uint8) or 5 (float32)");
    const int nl = c.OctaveLayers;
    S.P.nl = nl;
    S.P.thr = (float)(int)std::floor(0.5 * c.ContrastThreshold / (double)nl * 255.0);
    S.P.edge = (float)c.EdgeThreshold;
    S.P.contrast = c.ContrastThreshold;
    S.P.sigma = c.Sigma;
    S.featureCount = c.FeatureCount;
    S.descType = c.DescriptorType;
    S.w = width;
    S.h = height;
    S.channels = channels;
    const int m = 2 * (width < height ? width : height);
    const int nOct = (int)std::nearbyint(std::log2((double)m) - 2.0);
    S.nOctaves = nOct > 0 ? nOct : 0;
    S.ow.clear();
    S.oh.clear();
    S.obase.clear();
    size_t at = 0;
    int ow = 2 * width, oh = 2 * height;
    for (int o = 0; o < S.nOctaves; ++o) {
        S.ow.push_back(ow);
        S.oh.push_back(oh);
        S.obase.push_back(at);
        at += (size_t)(nl + 3) * (size_t)ow * (size_t)oh;
        ow /= 2;
        oh /= 2;
    }
    S.pyramidFloats = at;
    // taps: double throughout, rounded to float once
    std::vector<double> sig((size_t)nl + 3);
    const double s0 = c.Sigma * c.Sigma - 1.0;
    sig[0] = std::sqrt(s0 > 0.01 ? s0 : 0.01);
    const double k = std::pow(2.0, 1.0 / (double)nl);
    for (int i = 1; i < nl + 3; ++i) {
        const double prev = std::pow(k, (double)(i - 1)) * c.Sigma, total = prev * k;
        sig[(size_t)i] = std::sqrt(total * total - prev * prev);
    }
    S.taps.clear();
    S.tapOff.clear();
    S.tapRadius.clear();
    for (int b = 0; b < nl + 3; ++b) {
        const double s = sig[(size_t)b];
        const int ks = (int)std::nearbyint(8.0 * s + 1.0) | 1, R = (ks - 1) / 2;
        if (R > kSiftMaxRadius) return sift_fail(err, name, "blur radius above the column tile's LDS budget");
        std::vector<double> t((size_t)ks);
        double sum = 0.0;
        for (int i = 0; i < ks; ++i) {
            const double x = (double)(i - R);
            t[(size_t)i] = std::exp(-(x * x) / (2.0 * s * s));
            sum += t[(size_t)i];
        }
        S.tapOff.push_back((int)S.taps.size());
        S.tapRadius.push_back(R);
        for (int i = 0; i < ks; ++i) S.taps.push_back((float)(t[(size_t)i] / sum));
    }
    return true;
}

// rows first (along x), then columns; every value is exact in float
inline void sift_host_double(const uint8_t* data, const SiftPlan& S, std::vector<float>& up) {
    const int w = S.w, h = S.h, W = 2 * w, H = 2 * h;
    std::vector<float> rows((size_t)W * (size_t)h);
    for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c) {
            const int c1 = c + 1 < w ? c + 1 : w - 1;
            const float a = sift_grey(data + ((size_t)r * w + c) * S.channels, S.channels);
            const float b = sift_grey(data + ((size_t)r * w + c1) * S.channels, S.channels);
            rows[(size_t)r * W + 2 * c] = a;
            rows[(size_t)r * W + 2 * c + 1] = 0.5f * a + 0.5f * b;
        }
    up.assign((size_t)W * (size_t)H, 0.0f);
    for (int r = 0; r < h; ++r) {
        const int r1 = r + 1 < h ? r + 1 : h - 1;
        for (int c = 0; c < W; ++c) {
            const float a = rows[(size_t)r * W + c], b = rows[(size_t)r1 * W + c];
            up[(size_t)(2 * r) * W + c] = a;
            up[(size_t)(2 * r + 1) * W + c] = 0.5f * a + 0.5f * b;
        }
    }
}

// separable blur: rows (along x), then columns, taps in ascending index from a zero accumulator
inline void sift_host_blur(const float* in, float* out, int w, int h, const float* taps, int R,
                           std::vector<float>& tmp) {
    tmp.assign((size_t)w * (size_t)h, 0.0f);
    std::vector<int> idx;
    for (int pass = 0; pass < 2; ++pass) {
        const int n = pass == 0 ? w : h;
        idx.assign((size_t)(n + 2 * R), 0);
        for (int i = 0; i < n + 2 * R; ++i) idx[(size_t)i] = sift_reflect(i - R, n);
        for (int r = 0; r < h; ++r)
            for (int c = 0; c < w; ++c) {
                float acc = 0.0f;
                if (pass == 0)
                    for (int t = 0; t <= 2 * R; ++t) acc = acc + taps[t] * in[(size_t)r * w + idx[(size_t)(c + t)]];
                else
                    for (int t = 0; t <= 2 * R; ++t) acc = acc + taps[t] * tmp[(size_t)idx[(size_t)(r + t)] * w + c];
                (pass == 0 ? tmp.data() : out)[(size_t)r * w + c] = acc;
            }
    }
}

inline void sift_host_pyramid(const uint8_t* data, const SiftPlan& S, std::vector<float>& pyr) {
    pyr.assign(S.pyramidFloats, 0.0f);
    if (S.nOctaves == 0) return;
    std::vector<float> up, tmp;
    sift_host_double(data, S, up);
    const int nl = S.P.nl;
    for (int o = 0; o < S.nOctaves; ++o) {
        const int w = S.ow[(size_t)o], h = S.oh[(size_t)o];
        const size_t plane = (size_t)w * (size_t)h;
        float* g = pyr.data() + S.obase[(size_t)o];
        if (o == 0)
            sift_host_blur(up.data(), g, w, h, S.taps.data() + S.tapOff[0], S.tapRadius[0], tmp);
        else {
            const int pw = S.ow[(size_t)o - 1];
            const float* src = pyr.data() + S.obase[(size_t)o - 1] +
                               (size_t)nl * (size_t)pw * (size_t)S.oh[(size_t)o - 1];
            for (int r = 0; r < h; ++r)
                for (int c = 0; c < w; ++c) g[(size_t)r * w + c] = src[(size_t)(2 * r) * pw + 2 * c];
        }
        for (int i = 1; i < nl + 3; ++i)
            sift_host_blur(g + (size_t)(i - 1) * plane, g + (size_t)i * plane, w, h,
                           S.taps.data() + S.tapOff[(size_t)i], S.tapRadius[(size_t)i], tmp);
    }
}

// is DoG (layer, r, c) a candidate: |v| above the threshold and an extremum of its 26 neighbours
inline bool sift_is_candidate(const float* g, size_t plane, int w, int layer, int r, int c, float thr) {
    const float v = sift_dog(g, plane, w, layer, r, c);
    if (!(fabsf(v) > thr)) return false;
    for (int dl = -1; dl <= 1; ++dl)
        for (int dr = -1; dr <= 1; ++dr)
            for (int dc = -1; dc <= 1; ++dc) {
                const float n = sift_dog(g, plane, w, layer + dl, r + dr, c + dc);
                if (v > 0.0f ? !(v >= n) : !(v <= n)) return false;
            }
    return true;
}

struct SiftHostResult {
    std::vector<SiftRec> recs;
    std::vector<float> desc;   // [n][128], scaled to 512, unrounded
    long long candidates = 0, refined = 0, oriented = 0;
};

struct SiftSortItem {
    unsigned long long key, start;
    SiftRec rec;
};

inline void sift_host_detect(const uint8_t* data, const SiftPlan& S, SiftHostResult& R) {
    R = SiftHostResult();
    std::vector<float> pyr;
    sift_host_pyramid(data, S, pyr);
    const int nl = S.P.nl;
    std::vector<SiftSortItem> items;
    for (int o = 0; o < S.nOctaves; ++o) {
        const int w = S.ow[(size_t)o], h = S.oh[(size_t)o];
        const size_t plane = (size_t)w * (size_t)h;
        const float* g = pyr.data() + S.obase[(size_t)o];
        for (int layer = 1; layer <= nl; ++layer)
            for (int r = kSiftBorder; r < h - kSiftBorder; ++r)
                for (int c = kSiftBorder; c < w - kSiftBorder; ++c) {
                    if (!sift_is_candidate(g, plane, w, layer, r, c, S.P.thr)) continue;
                    ++R.candidates;
                    SiftKp kp;
                    if (!sift_refine(g, w, h, o, layer, r, c, S.P, kp)) continue;
                    ++R.refined;
                    const float* img = g + (size_t)kp.layer * plane;
                    long long hist[kSiftOriBins] = {0};
                    const int rad = sift_ori_radius(kp.scl);
                    const float es = sift_ori_escale(kp.scl);
                    for (int i = -rad; i <= rad; ++i)
                        for (int j = -rad; j <= rad; ++j) {
                            int bin;
                            long long q;
                            if (sift_ori_sample(img, w, h, kp.r, kp.c, i, j, es, bin, q)) hist[bin] += q;
                        }
                    int bins[kSiftMaxPeaks];
                    float angles[kSiftMaxPeaks];
                    const int np = sift_ori_peaks(hist, bins, angles);
                    const float sc = (float)(1 << o) * 0.5f;
                    for (int k = 0; k < np; ++k) {
                        SiftSortItem it;
                        it.key = sift_key(kp.o, kp.layer, kp.r, kp.c, bins[k]);
                        it.start = sift_key(o, layer, r, c, bins[k]);
                        it.rec = SiftRec{((float)kp.c + kp.xc) * sc, ((float)kp.r + kp.xr) * sc, kp.size, angles[k],
                                         kp.response, kp.octave, kp.o, kp.layer, kp.r, kp.c, kp.scl, 0};
                        items.push_back(it);
                        ++R.oriented;
                    }
                }
    }
    // order, exact duplicates out (the smallest start survives; the copies are identical anyway)
    std::sort(items.begin(), items.end(), [](const SiftSortItem& a, const SiftSortItem& b) {
        return a.key != b.key ? a.key < b.key : a.start < b.start;
    });
    std::vector<SiftSortItem> uniq;
    for (const auto& it : items)
        if (uniq.empty() || uniq.back().key != it.key) uniq.push_back(it);
    if (S.featureCount > 0 && uniq.size() > (size_t)S.featureCount) {
        std::vector<size_t> ord(uniq.size());
        for (size_t i = 0; i < ord.size(); ++i) ord[i] = i;
        std::stable_sort(ord.begin(), ord.end(),
                         [&](size_t a, size_t b) { return uniq[a].rec.response > uniq[b].rec.response; });
        ord.resize((size_t)S.featureCount);
        std::sort(ord.begin(), ord.end());
        std::vector<SiftSortItem> kept;
        for (size_t i : ord) kept.push_back(uniq[i]);
        uniq.swap(kept);
    }
    R.recs.reserve(uniq.size());
    for (const auto& it : uniq) R.recs.push_back(it.rec);
    R.desc.assign(R.recs.size() * (size_t)kSiftDescLen, 0.0f);
    for (size_t n = 0; n < R.recs.size(); ++n) {
        const SiftRec& q = R.recs[n];
        const int w = S.ow[(size_t)q.o], h = S.oh[(size_t)q.o];
        const float* img = pyr.data() + S.obase[(size_t)q.o] + (size_t)q.layer * (size_t)w * (size_t)h;
        const SiftDescFrame F = sift_desc_frame(q.angle, q.scl, w, h);
        long long sum[kSiftDescLen] = {0};
        for (int i = -F.radius; i <= F.radius; ++i)
            for (int j = -F.radius; j <= F.radius; ++j)
                sift_desc_sample(img, w, h, q.r, q.c, i, j, F, [&](int k, long long v) { sum[k] += v; });
        sift_desc_finish(sum, R.desc.data() + n * (size_t)kSiftDescLen);
    }
}

}  // namespace mcv
