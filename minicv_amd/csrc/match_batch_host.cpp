// match_batch_host.cpp — cvMatchFeaturesBatch / cvMatchAndFindModelBatch: the matches of B image pairs
// over nImages images in one call whose kernel launches, stream synchronisations and copies do not grow
// with B or nImages (kernels: match_batch.hip).
//
//   images   the descriptor rows of every image that some pair names are staged once into one pinned buffer
//            and go to the device in one copy, however many pairs an image is in (an image in no pair is
//            not sent); one prep launch pads / shifts / norms every
//            row once (skipped for Hamming rows of exactly 32 or 64 bytes, which are matched in place)
//   tables   directed problems (with crossCheck the reverse problems follow the B forward ones), the
//            workgroup table and the forward problems' query starts: one pinned buffer, one copy
//   knn      one launch over every (problem, query tile)
//   compact  filter + counts, scan, scatter, offsets: four launches over the concatenated forward queries
//   back     offsets (one copy, one synchronisation: the total sizes the rest), then pairs and dist
// cvMatchAndFindModelBatch gathers the matched keypoints on the host from the pair list (float widened to
// double, which is exact) and hands them to cvFindModelBatch: the keypoints never go to the device twice.
#include "minicv_native.h"
#include "mcv_runtime.h"
#include "kernels.h"
#include "plan.h"

#include <algorithm>
#include <climits>
#include <cstring>
#include <numeric>
#include <vector>

namespace mcv {

namespace {
const int kElemU8 = 0, kElemF32 = 5;
const int kHammingMaxRows = 1 << 22;   // the key's index field (match_hamming.hip)

struct MbStats : CallStats {   // no memset is issued
    long long problems = 0, workgroups = 0;
};
thread_local MbStats t_mb_stats;

// The index arithmetic of a call. Directed problem d < B is pair d, query image first; with cross,
// d >= B is pair d - B reversed. Outputs are concatenated in d order, so the forward problems' queries
// are the first totalQ entries. Workgroups: the problems in descending train length (ties: ascending d),
// each problem's query tiles in ascending order; a problem without queries has none.
struct MbLayout {
    std::vector<MatchBatchProblem> prob;
    std::vector<int> qImage, tImage;   // per directed problem
    std::vector<int> rowOff;           // per image, nImages + 1 (an image in no pair has no rows)
    std::vector<int> wg;               // 2 per workgroup
    std::vector<int> qStart;           // B + 1
    int rowsPerWg = 0, totalQ = 0;
    long long totalOut = 0;
};

void mb_layout(const int* counts, int nImages, const int* imagePairs, int B, bool cross, int rowsPerWg, MbLayout& L) {
    L.rowsPerWg = rowsPerWg;
    L.rowOff.assign((size_t)nImages + 1, 0);
    // only the images some pair names take rows of the device buffer
    std::vector<char> used((size_t)nImages, 0);
    for (int k = 0; k < 2 * B; ++k) used[(size_t)imagePairs[k]] = 1;
    long long rows = 0;
    for (int i = 0; i < nImages; ++i) {
        if (used[(size_t)i]) rows += counts[i];
        if (rows > INT_MAX) fail("match batch: more than 2^31 - 1 descriptor rows");
        L.rowOff[(size_t)i + 1] = (int)rows;
    }
    const int D = cross ? 2 * B : B;
    L.prob.resize((size_t)D);
    L.qImage.resize((size_t)D);
    L.tImage.resize((size_t)D);
    L.qStart.assign((size_t)B + 1, 0);
    long long out = 0, nwg = 0;
    for (int d = 0; d < D; ++d) {
        const int p = d < B ? d : d - B;
        const int qi = imagePairs[2 * p + (d < B ? 0 : 1)], ti = imagePairs[2 * p + (d < B ? 1 : 0)];
        L.qImage[(size_t)d] = qi;
        L.tImage[(size_t)d] = ti;
        if (out > INT_MAX) fail("match batch: more than 2^31 - 1 queries over the problems");
        L.prob[(size_t)d] = MatchBatchProblem{L.rowOff[(size_t)qi], counts[qi], L.rowOff[(size_t)ti], counts[ti], (int)out};
        if (d < B) L.qStart[(size_t)d] = (int)out;
        out += counts[qi];
        if (d == B - 1) L.qStart[(size_t)B] = (int)std::min<long long>(out, INT_MAX);
        nwg += (counts[qi] + rowsPerWg - 1) / rowsPerWg;
    }
    if (out > INT_MAX) fail("match batch: more than 2^31 - 1 queries over the problems");
    if (nwg > INT_MAX / 2) fail("match batch: too many workgroups");
    L.totalOut = out;
    L.totalQ = L.qStart[(size_t)B];
    std::vector<int> order((size_t)D);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(),
                     [&](int a, int b) { return L.prob[(size_t)a].nt > L.prob[(size_t)b].nt; });
    L.wg.clear();
    L.wg.reserve((size_t)nwg * 2);
    for (int d : order) {
        const int tiles = (L.prob[(size_t)d].nq + rowsPerWg - 1) / rowsPerWg;
        for (int t = 0; t < tiles; ++t) {
            L.wg.push_back(d);
            L.wg.push_back(t);
        }
    }
}

struct MbWs : DeviceWs {
    DevBuf<uint8_t> raw, rows, keep;
    DevBuf<int> norms, tables, idx, idx2, di1, di2, cnt, off, pairs, offsets;
    DevBuf<float> df1, df2, dist;
    PinnedBuf<uint8_t> h_raw;
    PinnedBuf<int> h_tables, h_offsets;
};

void mb_sync(hipStream_t s) { counted_sync(t_mb_stats, s); }

int padded_width(bool ham, int dim) {
    if (ham) return dim <= 32 ? 32 : 64;
    return dim <= 32 ? 32 : dim <= 64 ? 64 : dim <= 128 ? 128 : dim <= 256 ? 256 : 512;
}

// Device tables of a layout: [problems (5 ints each)] [workgroups (2 ints each)] [qStart (B + 1)], each
// part starting at a multiple of 4 ints.
struct MbTables {
    const MatchBatchProblem* prob;
    const int* wg;
    const int* qStart;
};
MbTables upload_tables(MbWs& W, const MbLayout& L, hipStream_t s) {
    auto up4 = [](size_t n) { return (n + 3) / 4 * 4; };
    const size_t nProb = up4(L.prob.size() * 5), nWg = up4(L.wg.size()), nQ = up4(L.qStart.size());
    const size_t n = nProb + nWg + nQ;
    W.h_tables.ensure(n);
    W.tables.ensure(n);
    static_assert(sizeof(MatchBatchProblem) == 5 * sizeof(int), "MatchBatchProblem is 5 ints");
    if (!L.prob.empty()) std::memcpy(W.h_tables.p, L.prob.data(), L.prob.size() * sizeof(MatchBatchProblem));
    if (!L.wg.empty()) std::memcpy(W.h_tables.p + nProb, L.wg.data(), L.wg.size() * sizeof(int));
    std::memcpy(W.h_tables.p + nProb + nWg, L.qStart.data(), L.qStart.size() * sizeof(int));
    counted_copy(t_mb_stats, W.tables.p, W.h_tables.p, n * sizeof(int), hipMemcpyHostToDevice, s);
    return MbTables{(const MatchBatchProblem*)W.tables.p, W.tables.p + nProb, W.tables.p + nProb + nWg};
}

// Rows to the device once, the prep launch, the knn launch. rowsOf(i) = image i's rows (counts[i] x dim
// bytes). Leaves idx / idx2 and di1 / di2 (Hamming) or df1 / df2 (L2) filled for every directed problem.
template <class RowsOf>
MbTables mb_knn(MbWs& W, const MbLayout& L, int nImages, const int* counts, RowsOf rowsOf, int dim, bool ham,
                hipStream_t s) {
    const int R = L.rowOff[(size_t)nImages];
    const int KP = padded_width(ham, dim);
    const size_t rawBytes = (size_t)R * dim;
    W.h_raw.ensure(rawBytes);
    W.raw.ensure(rawBytes);
    for (int i = 0; i < nImages; ++i)
        if (L.rowOff[(size_t)i + 1] > L.rowOff[(size_t)i])
            std::memcpy(W.h_raw.p + (size_t)L.rowOff[(size_t)i] * dim, rowsOf(i), (size_t)counts[i] * dim);
    if (rawBytes) counted_copy(t_mb_stats, W.raw.p, W.h_raw.p, rawBytes, hipMemcpyHostToDevice, s);
    const uint8_t* d_rows = W.raw.p;
    if (!ham || dim != KP) {
        W.rows.ensure((size_t)R * KP);
        if (!ham) W.norms.ensure((size_t)R);
        launch_match_batch_prep(W.raw.p, R, dim, KP, !ham, W.rows.p, W.norms.p, s);
        if (R > 0) ++t_mb_stats.launches;
        d_rows = W.rows.p;
    }
    const MbTables T = upload_tables(W, L, s);
    const size_t nOut = (size_t)L.totalOut;
    W.idx.ensure(nOut);
    W.idx2.ensure(nOut);
    const int nwg = (int)(L.wg.size() / 2);
    if (ham) {
        W.di1.ensure(nOut);
        W.di2.ensure(nOut);
        launch_match_batch_hamming(d_rows, KP / 4, T.prob, T.wg, nwg, W.idx.p, W.di1.p, W.idx2.p, W.di2.p, s);
    } else {
        W.df1.ensure(nOut);
        W.df2.ensure(nOut);
        launch_match_batch_l2u8(d_rows, W.norms.p, KP, T.prob, T.wg, nwg, W.idx.p, W.df1.p, W.idx2.p, W.df2.p, s);
    }
    if (nwg > 0) ++t_mb_stats.launches;
    t_mb_stats.problems = (long long)L.prob.size();
    t_mb_stats.workgroups = nwg;
    return T;
}

// Everything cvMatchFeaturesBatch refuses without touching the device. Returns the descriptor width
// (0: every image is empty) and whether the norm is Hamming.
int mb_check(const char* who, const DetectorResult* images, int nImages, const int* imagePairs, int B, int norm,
             const int* pairs, int maxPairs, const int* offsets, bool& ham) {
    if (nImages < 0) fail("%s: negative nImages (%d)", who, nImages);
    if (B < 0) fail("%s: negative B (%d)", who, B);
    if (maxPairs < 0) fail("%s: negative maxPairs (%d)", who, maxPairs);
    if (!offsets) fail("%s: null argument (offsets)", who);
    if (!pairs) fail("%s: null argument (pairs)", who);
    if (nImages > 0 && !images) fail("%s: null argument (images)", who);
    if (B > 0 && !imagePairs) fail("%s: null argument (imagePairs)", who);
    if (norm != MCV_NORM_AUTO && norm != MCV_NORM_L2 && norm != MCV_NORM_HAMMING)
        fail("%s: norm %d is none of MCV_NORM_AUTO (0), MCV_NORM_L2 (4), MCV_NORM_HAMMING (6)", who, norm);
    ham = norm != MCV_NORM_L2;
    int dim = 0;
    for (int i = 0; i < nImages; ++i) {
        const DetectorResult& r = images[i];
        if (r.PointCount < 0 || r.DescriptorEntries < 0) fail("%s: image %d has negative sizes", who, i);
        if (r.PointCount > 0 && (!r.Points || !r.Descriptors)) fail("%s: image %d has NULL arrays", who, i);
        if (r.PointCount > 0 && r.DescriptorEntries % r.PointCount != 0)
            fail("%s: image %d DescriptorEntries %d not a multiple of PointCount %d", who, i, r.DescriptorEntries,
                 r.PointCount);
        if (r.DescriptorElementType != images[0].DescriptorElementType)
            fail("%s: mixed descriptor element types (image 0: %d, image %d: %d)", who, images[0].DescriptorElementType,
                 i, r.DescriptorElementType);
        if (r.PointCount == 0) continue;
        const int w = r.DescriptorEntries / r.PointCount;
        if (dim == 0) dim = w;
        if (w != dim) fail("%s: mixed descriptor widths (%d, image %d: %d)", who, dim, i, w);
        if (ham && r.PointCount >= kHammingMaxRows)
            fail("%s: image %d has %d features, Hamming needs fewer than 2^22", who, i, r.PointCount);
    }
    if (nImages > 0) {
        const int et = images[0].DescriptorElementType;
        if (et == kElemF32)
            fail("%s: float32 descriptors are not batched (their exact re-rank is per pair): call "
                 "cvMatchFeaturesNorm / cvMatchAndFindModelNorm per pair",
                 who);
        if (et != kElemU8) fail("%s: descriptor element type %d unsupported (0 = uint8)", who, et);
    }
    if (dim > 0) {
        if (ham) {
            if (dim < 1 || dim > 64) fail("%s: Hamming descriptors of %d bytes outside [1, 64]", who, dim);
        } else {
            int mx = 0;
            for (int i = 0; i < nImages; ++i) mx = std::max(mx, images[i].PointCount);
            check_match_l2u8(who, mx, mx, dim);
        }
    }
    for (int p = 0; p < 2 * B; ++p)
        if (imagePairs[p] < 0 || imagePairs[p] >= nImages)
            fail("%s: problem %d names image %d outside [0, %d)", who, p / 2, imagePairs[p], nImages);
    return dim;
}

// The body of cvMatchFeaturesBatch after the argument checks. Returns offsets[B].
int match_features_batch(const char* who, const DetectorResult* images, int nImages, const int* imagePairs, int B,
                         const MatchConfig& cfg, bool ham, int dim, int* pairs, float* dist, int maxPairs,
                         int* offsets) {
    t_mb_stats = MbStats();
    for (int p = 0; p <= B; ++p) offsets[p] = 0;
    if (B == 0 || dim == 0) return 0;
    std::vector<int> counts((size_t)nImages);
    for (int i = 0; i < nImages; ++i) counts[(size_t)i] = images[i].PointCount;
    MbLayout L;
    mb_layout(counts.data(), nImages, imagePairs, B, cfg.crossCheck != 0, ham ? kMatchBatchRowsHamming : kMatchBatchRowsL2,
              L);
    if (L.totalQ == 0) return 0;
    require_device();
    MbWs& W = thread_device_ws<MbWs>();
    hipStream_t s = W.stream();
    const MbTables T = mb_knn(W, L, nImages, counts.data(), [&](int i) { return images[i].Descriptors; }, dim, ham, s);
    const int totalQ = L.totalQ, nb = (totalQ + 255) / 256;
    W.keep.ensure((size_t)totalQ);
    W.cnt.ensure((size_t)nb);
    W.off.ensure((size_t)nb + 1);
    W.pairs.ensure((size_t)2 * totalQ);
    W.dist.ensure((size_t)totalQ);
    W.offsets.ensure((size_t)B + 1);
    W.h_offsets.ensure((size_t)B + 1);
    launch_match_batch_compact(W.idx.p, ham ? W.di1.p : nullptr, ham ? W.di2.p : nullptr, ham ? nullptr : W.df1.p,
                               ham ? nullptr : W.df2.p, T.prob, T.qStart, B, cfg.crossCheck != 0, totalQ, cfg.ratio,
                               cfg.maxDistance, W.keep.p, W.cnt.p, W.off.p, W.pairs.p, W.dist.p, W.offsets.p, s);
    t_mb_stats.launches += 4;
    counted_copy(t_mb_stats, W.h_offsets.p, W.offsets.p, ((size_t)B + 1) * sizeof(int), hipMemcpyDeviceToHost, s);
    mb_sync(s);
    const int total = W.h_offsets.p[B];
    if (total > maxPairs) fail("%s: %d matches exceed maxPairs %d", who, total, maxPairs);
    std::memcpy(offsets, W.h_offsets.p, ((size_t)B + 1) * sizeof(int));
    if (total > 0) {
        counted_copy(t_mb_stats, pairs, W.pairs.p, (size_t)2 * total * sizeof(int), hipMemcpyDeviceToHost, s);
        if (dist) counted_copy(t_mb_stats, dist, W.dist.p, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, s);
        mb_sync(s);
    }
    return total;
}

const MatchConfig kDefaultMatchConfig{0.8f, 0, 0.f, MCV_MODEL_HOMOGRAPHY};
}  // namespace

}  // namespace mcv

using namespace mcv;

extern "C" MCV_API int cvMatchFeaturesBatch(const DetectorResult* images, int nImages, const int* imagePairs, int B,
                                            const MatchConfig* cfgp, int norm, int* pairs, float* dist, int maxPairs,
                                            int* offsets) {
    MCV_GUARD(-1, {
        bool ham = true;
        const int dim = mb_check("cvMatchFeaturesBatch", images, nImages, imagePairs, B, norm, pairs, maxPairs, offsets,
                                 ham);
        const MatchConfig cfg = cfgp ? *cfgp : kDefaultMatchConfig;
        return match_features_batch("cvMatchFeaturesBatch", images, nImages, imagePairs, B, cfg, ham, dim, pairs, dist,
                                    maxPairs, offsets);
    })
}

extern "C" MCV_API int cvMatchAndFindModelBatch(const DetectorResult* images, int nImages, const int* imagePairs, int B,
                                                const MatchConfig* mcfgp, int norm, const RansacConfig* rcfg,
                                                int* pairs, int maxPairs, int* offsets, mcvM33d* models, uint8_t* mask,
                                                int* counts) {
    MCV_GUARD(-1, {
        const char* who = "cvMatchAndFindModelBatch";
        if (!models || !mask || !counts) fail("%s: null argument (models, mask and counts are required)", who);
        bool ham = true;
        const int dim = mb_check(who, images, nImages, imagePairs, B, norm, pairs, maxPairs, offsets, ham);
        const MatchConfig mcfg = mcfgp ? *mcfgp : kDefaultMatchConfig;
        try {
            batch_check_config(mcfg.model, rcfg);   // what cvFindModelBatch refuses, before the device is touched
        } catch (const Error& e) {
            fail("%s: %s", who, e.what());
        }
        const int total = match_features_batch(who, images, nImages, imagePairs, B, mcfg, ham, dim, pairs, nullptr,
                                               maxPairs, offsets);
        // the matched keypoints, float widened to double
        std::vector<mcvV2d> a((size_t)std::max(total, 1)), b((size_t)std::max(total, 1));
        for (int p = 0; p < B; ++p) {
            const KeyPoint2d* ka = images[imagePairs[2 * p]].Points;
            const KeyPoint2d* kb = images[imagePairs[2 * p + 1]].Points;
            for (int k = offsets[p]; k < offsets[p + 1]; ++k) {
                const KeyPoint2d& x = ka[pairs[2 * k]];
                const KeyPoint2d& y = kb[pairs[2 * k + 1]];
                a[(size_t)k] = mcvV2d{(double)x.pt.X, (double)x.pt.Y};
                b[(size_t)k] = mcvV2d{(double)y.pt.X, (double)y.pt.Y};
            }
        }
        const int ok = cvFindModelBatch(mcfg.model, a.data(), b.data(), offsets, B, rcfg, models, mask, counts);
        if (ok < 0) {
            const std::string inner = mcvGetLastError();
            fail("%s: %s", who, inner.c_str());
        }
        return ok;   // the last error, if any, names the first pair without a model (cvFindModelBatch's rule)
    })
}

extern "C" MCV_API int mcvHostMatchBatchLayout(const int* featureCounts, int nImages, const int* imagePairs, int B,
                                               int crossCheck, int norm, int* problems5, int* info4, int* wgTable,
                                               int maxWorkgroups) {
    MCV_GUARD(-1, {
        const char* who = "mcvHostMatchBatchLayout";
        if (nImages < 0 || B < 0 || !info4 || (nImages > 0 && !featureCounts) || (B > 0 && !imagePairs))
            fail("%s: bad argument", who);
        if (norm != MCV_NORM_AUTO && norm != MCV_NORM_L2 && norm != MCV_NORM_HAMMING) fail("%s: norm %d", who, norm);
        for (int i = 0; i < nImages; ++i)
            if (featureCounts[i] < 0) fail("%s: negative feature count of image %d", who, i);
        for (int p = 0; p < 2 * B; ++p)
            if (imagePairs[p] < 0 || imagePairs[p] >= nImages) fail("%s: problem %d names image %d", who, p / 2, imagePairs[p]);
        MbLayout L;
        mb_layout(featureCounts, nImages, imagePairs, B, crossCheck != 0,
                  norm == MCV_NORM_L2 ? kMatchBatchRowsL2 : kMatchBatchRowsHamming, L);
        const int D = (int)L.prob.size(), G = (int)(L.wg.size() / 2);
        info4[0] = D;
        info4[1] = L.rowsPerWg;
        info4[2] = G;
        info4[3] = L.totalQ;
        if (problems5)
            for (int d = 0; d < D; ++d) {
                problems5[5 * d + 0] = L.qImage[(size_t)d];
                problems5[5 * d + 1] = L.tImage[(size_t)d];
                problems5[5 * d + 2] = L.prob[(size_t)d].nq;
                problems5[5 * d + 3] = L.prob[(size_t)d].nt;
                problems5[5 * d + 4] = L.prob[(size_t)d].outOff;
            }
        if (wgTable) {
            if (maxWorkgroups < G) fail("%s: %d workgroups exceed maxWorkgroups %d", who, G, maxWorkgroups);
            if (G > 0) std::memcpy(wgTable, L.wg.data(), (size_t)G * 2 * sizeof(int));
        }
        return G;
    })
}

extern "C" MCV_API int mcvTestMatchBatchStats(long long* stats8) {
    if (!stats8) return 0;
    for (int i = 0; i < 8; ++i) stats8[i] = 0;
    stats8[0] = t_mb_stats.launches;
    stats8[1] = t_mb_stats.syncs;
    stats8[2] = t_mb_stats.problems;
    stats8[3] = t_mb_stats.workgroups;
    stats8[4] = t_mb_stats.copies;
    return 1;
}

extern "C" MCV_API int mcvTestMatchBatchKnn(const uint8_t* rows, const int* featureCounts, int nImages, int dim,
                                            const int* directedPairs, int D, int norm, int* idx, void* dist, int* idx2,
                                            void* dist2) {
    MCV_GUARD(-1, {
        const char* who = "mcvTestMatchBatchKnn";
        if (nImages < 0 || D < 0 || (nImages > 0 && !featureCounts) || (D > 0 && !directedPairs) || !idx || !dist ||
            !idx2 || !dist2)
            fail("%s: bad argument", who);
        if (norm != MCV_NORM_L2 && norm != MCV_NORM_HAMMING) fail("%s: norm %d is neither L2 (4) nor Hamming (6)", who, norm);
        const bool ham = norm == MCV_NORM_HAMMING;
        long long R = 0;
        int mx = 0;
        std::vector<size_t> first((size_t)nImages + 1, 0);   // image i's first row in `rows`
        for (int i = 0; i < nImages; ++i) {
            if (featureCounts[i] < 0) fail("%s: negative feature count of image %d", who, i);
            R += featureCounts[i];
            first[(size_t)i + 1] = (size_t)R;
            mx = std::max(mx, featureCounts[i]);
        }
        if (R > 0 && !rows) fail("%s: rows is NULL", who);
        if (ham) {
            if (dim < 1 || dim > 64) fail("%s: Hamming descriptors of %d bytes outside [1, 64]", who, dim);
            if (mx >= kHammingMaxRows) fail("%s: Hamming needs fewer than 2^22 features per image", who);
        } else {
            check_match_l2u8(who, mx, mx, dim);
        }
        for (int p = 0; p < 2 * D; ++p)
            if (directedPairs[p] < 0 || directedPairs[p] >= nImages)
                fail("%s: problem %d names image %d", who, p / 2, directedPairs[p]);
        t_mb_stats = MbStats();
        MbLayout L;
        mb_layout(featureCounts, nImages, directedPairs, D, false, ham ? kMatchBatchRowsHamming : kMatchBatchRowsL2, L);
        if (L.totalOut == 0) return 0;
        require_device();
        MbWs& W = thread_device_ws<MbWs>();
        hipStream_t s = W.stream();
        mb_knn(W, L, nImages, featureCounts, [&](int i) { return rows + first[(size_t)i] * dim; }, dim, ham, s);
        const size_t n = (size_t)L.totalOut;
        MCV_HIP(hipMemcpyAsync(idx, W.idx.p, n * 4, hipMemcpyDeviceToHost, s));
        MCV_HIP(hipMemcpyAsync(idx2, W.idx2.p, n * 4, hipMemcpyDeviceToHost, s));
        MCV_HIP(hipMemcpyAsync(dist, ham ? (const void*)W.di1.p : (const void*)W.df1.p, n * 4, hipMemcpyDeviceToHost, s));
        MCV_HIP(hipMemcpyAsync(dist2, ham ? (const void*)W.di2.p : (const void*)W.df2.p, n * 4, hipMemcpyDeviceToHost, s));
        mb_sync(s);
        return (int)n;
    })
}
