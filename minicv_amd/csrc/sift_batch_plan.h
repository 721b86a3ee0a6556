// sift_batch_plan.h — the plan of a cvDetectFeaturesBatch call on the host: every argument
// check, sift_plan per image, the per-image table the kernels read, the bucket bases, the sizes of the
// buffers that do not depend on the content (in size_t, an overflow refused, never wrapped) and the
// call's launches, synchronisations, copies and memsets. No HIP: cvDetectFeaturesBatch,
// mcvTestSiftBatchPlan and the stand-alone sanitizer program (tests/native) all run this code.
#pragma once

#include "sift_ref.h"

#include <climits>
#include <cstring>

namespace mcv {

// The caller's image (include/minicv_native.h declares the same 24 bytes).
struct SiftImageIn {
    const uint8_t* data;
    int width, height, channels, reserved;
};

static const int kSiftBatchOctaves = 16;   // kSiftMaxOctaves (kernels.h)
// One image of a batch as the kernels read it (sift_batch.hip): SiftPyramid's fields with offsets into
// the batch's buffers. An image without an octave has nOctaves 0 and an empty bucket range.
struct SiftBatchImage {
    size_t imgOff;                         // bytes into the staged images
    size_t scratchOff;                     // floats into the doubled bases, and into the row blur's scratch
    size_t obase[kSiftBatchOctaves];       // float offset of an octave's first image in the batch's pyramid
    int ow[kSiftBatchOctaves], oh[kSiftBatchOctaves];
    int rowBase[kSiftBatchOctaves];        // first bucket of an octave: a bucket is one (image, octave, layer, row)
    int w, h, ch, nOctaves;
    int bucketBegin, bucketEnd;            // the image's buckets; the next image's begin here
};
static const int kSiftBatchImageBytes = 360;
static_assert(sizeof(SiftBatchImage) == kSiftBatchImageBytes, "SiftBatchImage is 360 bytes");

// Kernel launches of a cvDetectFeaturesBatch call with M = the largest nOctaves of its images > 0:
// kSiftBatchLaunchesFixed (grey + doubling, the base blur's two, refine, orientation, the bucket scan's
// three, scatter, rank, the compaction scan's three, the compaction, the per-image offsets, descriptors)
// + M x (2 x (OctaveLayers + 2) + 1) + (M - 1) + 1 if FeatureCount > 0: the single call's formula with
// another constant. None of the four counts depends on nImages, the sizes or the content.
static const int kSiftBatchLaunchesFixed = 16;
static const int kSiftBatchSyncs = 4, kSiftBatchCopies = 8, kSiftBatchMemsets = 1;
static const int kSiftBatchScanBlocks = 1024;   // blocks (and partial sums) of each pass of the two grid-wide scans

inline bool sift_size_add(size_t a, size_t b, size_t& out) { return !__builtin_add_overflow(a, b, &out); }
inline bool sift_size_mul(size_t a, size_t b, size_t& out) { return !__builtin_mul_overflow(a, b, &out); }

struct SiftBatchPlan {
    SiftPlan cfg;                          // P, featureCount, descType and the taps: the shared configuration's
    int nImages = 0, maxOctaves = 0, noOctave = 0;
    std::vector<SiftBatchImage> table;
    std::vector<int> lw, lh;               // per octave level, the largest width and height among the images that have it
    size_t imgBytes = 0, scratchFloats = 0, pyramidFloats = 0;
    int nBuckets = 0;
    unsigned capC = 1;                     // places of the candidate list
    size_t counterWords = 0, zeroWords = 0;
    size_t workspaceBytes = 0;
    long long launches = 0, syncs = 0, copies = 0, memsets = 0;
    // counter words: ctr[kSiftCtrs = 4], icnt[nImages], bcnt[nBuckets] (these are zeroed), boff[nBuckets + 1],
    // koff[nImages + 1], part[kSiftBatchScanBlocks + 1]
    size_t icntAt() const { return 4; }
    size_t bcntAt() const { return 4 + (size_t)nImages; }
    size_t boffAt() const { return bcntAt() + (size_t)nBuckets; }
    size_t koffAt() const { return boffAt() + (size_t)nBuckets + 1; }
    size_t partAt() const { return koffAt() + (size_t)nImages + 1; }
};

inline long long sift_batch_launches(int maxOctaves, int nl, int featureCount) {
    if (maxOctaves <= 0) return 0;
    return kSiftBatchLaunchesFixed + (long long)maxOctaves * (2 * (nl + 2) + 1) + (maxOctaves - 1) +
           (featureCount > 0 ? 1 : 0);
}

inline bool sift_batch_plan(const char* name, const SiftImageIn* images, int nImages, int mode, const void* config,
                            SiftBatchPlan& B, std::string& err) {
    char buf[200];
    B = SiftBatchPlan();
    if (nImages < 0) return sift_fail(err, name, "nImages must not be negative");
    if (nImages > kSiftBatchMaxImages) {
        snprintf(buf, sizeof buf, "nImages %d exceeds the cap of %d images (split the batch)", nImages,
                 kSiftBatchMaxImages);
        return sift_fail(err, name, buf);
    }
    if (nImages > 0 && !images) return sift_fail(err, name, "null images");
    // the mode and the shared configuration, on an image of one pixel
    const uint8_t one = 0;
    if (!sift_plan(name, &one, 1, 1, 1, mode, config, B.cfg, err)) return false;
    B.nImages = nImages;
    B.table.assign((size_t)nImages, SiftBatchImage());
    const int nl = B.cfg.P.nl;
    size_t interior = 0;
    long long buckets = 0;
    bool fits = true;
    SiftPlan S;
    for (int i = 0; i < nImages; ++i) {
        const SiftImageIn& im = images[i];
        snprintf(buf, sizeof buf, "%s: image %d", name, i);
        if (im.reserved != 0) return sift_fail(err, buf, "reserved must be 0");
        if (!sift_plan(buf, im.data, im.width, im.height, im.channels, mode, config, S, err)) return false;
        SiftBatchImage& T = B.table[(size_t)i];
        std::memset(&T, 0, sizeof T);
        T.w = im.width;
        T.h = im.height;
        T.ch = im.channels;
        T.nOctaves = S.nOctaves;
        T.imgOff = B.imgBytes;
        T.scratchOff = B.scratchFloats;
        T.bucketBegin = (int)buckets;
        size_t bytes = 0;
        fits = fits && sift_size_mul((size_t)im.width * (size_t)im.height, (size_t)im.channels, bytes) &&
               sift_size_add(B.imgBytes, bytes, B.imgBytes);
        if (S.nOctaves == 0) ++B.noOctave;
        if (S.nOctaves > 0)
            fits = fits && sift_size_add(B.scratchFloats, (size_t)S.ow[0] * (size_t)S.oh[0], B.scratchFloats);
        if (S.nOctaves > B.maxOctaves) {
            B.maxOctaves = S.nOctaves;
            B.lw.resize((size_t)S.nOctaves, 0);
            B.lh.resize((size_t)S.nOctaves, 0);
        }
        for (int o = 0; o < S.nOctaves; ++o) {
            const int ow = S.ow[(size_t)o], oh = S.oh[(size_t)o];
            fits = fits && sift_size_add(B.pyramidFloats, S.obase[(size_t)o], T.obase[o]);
            T.ow[o] = ow;
            T.oh[o] = oh;
            T.rowBase[o] = (int)buckets;
            buckets += (long long)nl * oh;
            if (buckets > INT_MAX) fits = false, buckets = 0;
            B.lw[(size_t)o] = std::max(B.lw[(size_t)o], ow);
            B.lh[(size_t)o] = std::max(B.lh[(size_t)o], oh);
            interior += (size_t)std::max(ow - 2 * kSiftBorder, 0) * (size_t)std::max(oh - 2 * kSiftBorder, 0) * (size_t)nl;
        }
        fits = fits && sift_size_add(B.pyramidFloats, S.pyramidFloats, B.pyramidFloats);
        T.bucketEnd = (int)buckets;
    }
    B.nBuckets = (int)buckets;
    B.capC = (unsigned)std::min<size_t>(std::max<size_t>(interior, 1), (size_t)kSiftBatchMaxCandidates);
    B.zeroWords = B.boffAt();
    B.counterWords = B.partAt() + (size_t)kSiftBatchScanBlocks + 1;
    // the buffers whose sizes the plan knows: images, the doubled bases, the row blur's scratch, the pyramids,
    // the taps, the table, the counters and the candidate list
    size_t total = B.imgBytes, part = 0;
    fits = fits && sift_size_mul(B.scratchFloats, 2 * sizeof(float), part) && sift_size_add(total, part, total);
    fits = fits && sift_size_mul(B.pyramidFloats, sizeof(float), part) && sift_size_add(total, part, total);
    fits = fits && sift_size_add(total, B.cfg.taps.size() * sizeof(float), total);
    fits = fits && sift_size_add(total, (size_t)nImages * sizeof(SiftBatchImage), total);
    fits = fits && sift_size_mul(B.counterWords, sizeof(unsigned), part) && sift_size_add(total, part, total);
    fits = fits && sift_size_add(total, (size_t)B.capC * 16, total);
    if (!fits || total > kSiftBatchMaxWorkspaceBytes) {
        if (fits)
            snprintf(buf, sizeof buf, "the workspace of %zu bytes exceeds the cap of %llu bytes (split the batch)", total,
                     kSiftBatchMaxWorkspaceBytes);
        else
            snprintf(buf, sizeof buf, "the workspace overflows its size type (split the batch)");
        return sift_fail(err, name, buf);
    }
    B.workspaceBytes = total;
    B.launches = sift_batch_launches(B.maxOctaves, nl, B.cfg.featureCount);
    if (B.maxOctaves > 0) {
        B.syncs = kSiftBatchSyncs;
        B.copies = kSiftBatchCopies;
        B.memsets = kSiftBatchMemsets;
    }
    return true;
}

inline void sift_batch_plan_out8(const SiftBatchPlan& B, long long* out8) {
    const long long v[8] = {B.maxOctaves, B.launches, B.syncs, B.copies, B.memsets, B.nBuckets,
                            (long long)B.workspaceBytes, B.noOctave};
    std::copy(v, v + 8, out8);
}

}  // namespace mcv
