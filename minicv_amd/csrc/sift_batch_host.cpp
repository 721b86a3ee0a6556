// sift_batch_host.cpp — cvDetectFeaturesBatch: nImages cvDetectFeatures(mode 4) calls under
// one SiftConfig in one call. The plan (sift_batch_plan.h) checks every argument and sizes the layout on
// the host before the device is touched; the images go up through one pinned buffer in one copy, the
// stages of sift_batch.hip run over all images at once, and the keypoints and descriptors come down in
// one copy each and are split into the caller's DetectorResult array. Launches, copies, memsets and the
// four synchronisations depend on the largest nOctaves, OctaveLayers and FeatureCount > 0 alone.
#include "minicv_native.h"
#include "mcv_runtime.h"
#include "sift_batch_plan.h"
#include "kernels.h"
#include "plan.h"

#include <cstddef>
#include <cstring>

using namespace mcv;

static_assert(sizeof(mcvImage) == 24 && sizeof(SiftImageIn) == 24, "mcvImage is 24 bytes");
static_assert(offsetof(mcvImage, width) == offsetof(SiftImageIn, width) &&
                  offsetof(mcvImage, reserved) == offsetof(SiftImageIn, reserved),
              "mcvImage and SiftImageIn are one layout");
static_assert(kSiftCtrs == 4, "SiftBatchPlan lays four counters before the per-image ones");

namespace {

struct SiftBatchStats : CallStats {
    long long candidates = 0, refined = 0, oriented = 0, kept = 0;
};
thread_local SiftBatchStats t_st;

struct SiftBatchWork : DeviceWs {
    PinnedBuf<uint8_t> h_img, h_desc;
    PinnedBuf<SiftBatchImage> h_table;
    PinnedBuf<unsigned> h_ctr;
    PinnedBuf<SiftKeyPointOut> h_kp;
    DevBuf<uint8_t> img, flagA, flagB, descU8;
    DevBuf<SiftBatchImage> table;
    DevBuf<float> up, tmp, pyr, taps, descF32;
    DevBuf<int> cand, perm, sortedIdx;
    DevBuf<SiftKp> kps;
    DevBuf<SiftRec> recs, sorted;
    DevBuf<unsigned long long> keys, starts, rkeys, skeys, srkeys;
    DevBuf<unsigned> ctr, pos;
    DevBuf<SiftKeyPointOut> kp;
};

void fill_result(DetectorResult& res, size_t n, int descType) {
    res.PointCount = (int)n;
    res.DescriptorEntries = (int)(n * (size_t)kSiftDescLen);
    res.DescriptorElementType = descType;
    res.Points = new KeyPoint2d[n ? n : 1];
    res.Descriptors = new uint8_t[(n ? n : 1) * (size_t)kSiftDescLen * (descType == 0 ? 1 : sizeof(float))];
}

void free_results(DetectorResult* results, int nImages) {
    for (int i = 0; i < nImages; ++i) {
        delete[] results[i].Descriptors;
        delete[] results[i].Points;
    }
    std::memset((void*)results, 0, (size_t)nImages * sizeof(DetectorResult));
}

}  // namespace

extern "C" MCV_API void cvFreeFeaturesBatch(DetectorResult* results, int nImages) {
    if (results && nImages > 0) free_results(results, nImages);
}

extern "C" MCV_API long long cvDetectFeaturesBatch(const mcvImage* images, int nImages, int mode, void* config,
                                                   DetectorResult* results) {
    if (results && nImages > 0) std::memset((void*)results, 0, (size_t)nImages * sizeof(DetectorResult));
    MCV_GUARD(-1, {
        const char* name = "cvDetectFeaturesBatch";
        SiftBatchPlan B;
        std::string err;
        if (!sift_batch_plan(name, (const SiftImageIn*)images, nImages, mode, config, B, err)) fail("%s", err.c_str());
        if (nImages == 0) return 0;
        if (!results) fail("%s: null results", name);
        require_device();
        SiftBatchStats& st = t_st;
        st = SiftBatchStats();
        const int descType = B.cfg.descType, nl = B.cfg.P.nl;
        const size_t elt = descType == 0 ? 1 : sizeof(float);
        try {
            if (B.maxOctaves == 0) {
                for (int i = 0; i < nImages; ++i) fill_result(results[i], 0, descType);
                return 0;
            }
            int dev = -1;
            MCV_HIP(hipGetDevice(&dev));
            SiftBatchWork& w = thread_device_ws_on<SiftBatchWork>(dev);
            hipStream_t s = w.stream();
            w.h_img.ensure(B.imgBytes);
            w.h_table.ensure((size_t)nImages);
            w.h_ctr.ensure(kSiftCtrs + 2 * (size_t)nImages + 1);
            w.img.ensure(B.imgBytes);
            w.table.ensure((size_t)nImages);
            w.up.ensure(B.scratchFloats);
            w.tmp.ensure(B.scratchFloats);
            w.pyr.ensure(B.pyramidFloats);
            w.taps.ensure(B.cfg.taps.size());
            w.ctr.ensure(B.counterWords);
            w.cand.ensure(4 * (size_t)B.capC);
            for (int i = 0; i < nImages; ++i) {
                const SiftBatchImage& T = B.table[(size_t)i];
                std::memcpy(w.h_img.p + T.imgOff, images[i].data, (size_t)T.w * (size_t)T.h * (size_t)T.ch);
                w.h_table.p[i] = T;
            }
            SiftBatchDevice D;
            std::memset(&D, 0, sizeof D);
            D.table = w.table.p;
            D.nImages = nImages;
            D.img = w.img.p;
            D.up = w.up.p;
            D.tmp = w.tmp.p;
            D.pyr = w.pyr.p;
            D.taps = w.taps.p;
            D.ctr = w.ctr.p;
            D.icnt = w.ctr.p + B.icntAt();
            D.bcnt = w.ctr.p + B.bcntAt();
            D.boff = w.ctr.p + B.boffAt();
            D.koff = w.ctr.p + B.koffAt();
            D.part = w.ctr.p + B.partAt();
            D.nBuckets = B.nBuckets;
            D.cand = (int4*)w.cand.p;
            D.capC = B.capC;
            counted_copy(st, w.img.p, w.h_img.p, B.imgBytes, hipMemcpyHostToDevice, s);
            counted_copy(st, w.table.p, w.h_table.p, (size_t)nImages * sizeof(SiftBatchImage), hipMemcpyHostToDevice, s);
            counted_copy(st, w.taps.p, B.cfg.taps.data(), B.cfg.taps.size() * sizeof(float), hipMemcpyHostToDevice, s);
            counted_zero(st, w.ctr.p, B.zeroWords * sizeof(unsigned), s);
            {
                ProfScope ps("sift_batch_pyramid", s);
                launch_sift_batch_grey_double(D, B.lw[0], B.lh[0], s);
                launch_sift_batch_blur(D, 0, 0, B.cfg.tapOff[0], B.cfg.tapRadius[0], B.lw[0], B.lh[0], s);
                st.launches += 1 + kSiftLaunchesPerBlur;
            }
            for (int o = 0; o < B.maxOctaves; ++o) {
                const int mw = B.lw[(size_t)o], mh = B.lh[(size_t)o];
                {
                    ProfScope ps("sift_batch_pyramid", s);
                    if (o > 0) {
                        launch_sift_batch_downsample(D, o, nl, mw, mh, s);
                        st.launches += kSiftLaunchesDownsample;
                    }
                    for (int i = 1; i < nl + 3; ++i) {
                        launch_sift_batch_blur(D, o, i, B.cfg.tapOff[(size_t)i], B.cfg.tapRadius[(size_t)i], mw, mh, s);
                        st.launches += kSiftLaunchesPerBlur;
                    }
                }
                ProfScope ps("sift_batch_extrema", s);
                launch_sift_batch_extrema(D, o, nl, B.cfg.P.thr, mw, mh, s);
                st.launches += kSiftLaunchesExtrema;
            }
            MCV_HIP(hipGetLastError());
            unsigned* ctr = w.h_ctr.p;
            counted_copy(st, ctr, w.ctr.p, (kSiftCtrs + (size_t)nImages) * sizeof(unsigned), hipMemcpyDeviceToHost, s);
            counted_wait(st, s);
            st.candidates = ctr[0];
            for (int i = 0; i < nImages; ++i)
                if ((long long)ctr[kSiftCtrs + i] > kSiftMaxCandidates)
                    fail("%s: image %d: %lld extremum candidates exceed the cap of %d (raise ContrastThreshold)", name, i,
                         (long long)ctr[kSiftCtrs + i], kSiftMaxCandidates);
            if (st.candidates > kSiftBatchMaxCandidates)
                fail("%s: %lld extremum candidates of all images together exceed the cap of %d (split the batch)", name,
                     st.candidates, kSiftBatchMaxCandidates);
            const int nC = (int)ctr[0];
            const size_t capK = (size_t)kSiftMaxPeaks * (size_t)std::max(nC, 1);
            w.kps.ensure((size_t)std::max(nC, 1));
            w.recs.ensure(capK);
            w.keys.ensure(capK);
            w.starts.ensure(capK);
            w.rkeys.ensure(capK);
            {
                ProfScope ps("sift_batch_refine", s);
                launch_sift_batch_refine(D, B.cfg.P, nC, w.kps.p, s);
            }
            {
                ProfScope ps("sift_batch_orient", s);
                launch_sift_batch_orient(D, w.kps.p, nC, w.recs.p, w.keys.p, w.starts.p, w.rkeys.p, s);
            }
            st.launches += 2;
            MCV_HIP(hipGetLastError());
            counted_copy(st, ctr, w.ctr.p, kSiftCtrs * sizeof(unsigned), hipMemcpyDeviceToHost, s);
            counted_wait(st, s);
            st.refined = ctr[1];
            st.oriented = ctr[2];
            const int nK = (int)ctr[2];
            const size_t nk1 = (size_t)std::max(nK, 1);
            w.flagA.ensure(nk1);
            w.flagB.ensure(nk1);
            w.sorted.ensure(nk1);
            w.perm.ensure(nk1);
            w.sortedIdx.ensure(nk1);
            w.skeys.ensure(nk1);
            w.srkeys.ensure(nk1);
            w.pos.ensure(nk1 + 1);
            {
                ProfScope ps("sift_batch_order", s);
                SiftOrder O;
                O.nBuckets = B.nBuckets;
                O.bcnt = D.bcnt;
                O.boff = D.boff;
                O.keys = w.keys.p;
                O.starts = w.starts.p;
                O.rkeys = w.rkeys.p;
                O.recs = w.recs.p;
                O.perm = w.perm.p;
                O.sortedIdx = w.sortedIdx.p;
                O.skeys = w.skeys.p;
                O.srkeys = w.srkeys.p;
                O.keepA = w.flagA.p;
                O.keepB = w.flagB.p;
                O.out = w.sorted.p;
                O.count = nullptr;
                launch_sift_batch_order(D, O, w.pos.p, nK, B.cfg.featureCount, s);
                st.launches += 10 + (B.cfg.featureCount > 0 ? kSiftLaunchesSelect : 0);
            }
            MCV_HIP(hipGetLastError());
            unsigned* koff = w.h_ctr.p + kSiftCtrs;
            counted_copy(st, koff, D.koff, ((size_t)nImages + 1) * sizeof(unsigned), hipMemcpyDeviceToHost, s);
            counted_wait(st, s);
            const size_t nF = koff[nImages], nf1 = nF ? nF : 1;
            st.kept = (long long)nF;
            w.kp.ensure(nf1);
            w.h_kp.ensure(nf1);
            w.h_desc.ensure(nf1 * (size_t)kSiftDescLen * elt);
            if (descType == 0)
                w.descU8.ensure(nf1 * (size_t)kSiftDescLen);
            else
                w.descF32.ensure(nf1 * (size_t)kSiftDescLen);
            {
                ProfScope ps("sift_batch_describe", s);
                launch_sift_batch_describe(D, w.sorted.p, (int)nF, descType, w.kp.p, w.descU8.p, w.descF32.p, s);
                st.launches += 1;
            }
            MCV_HIP(hipGetLastError());
            counted_copy(st, w.h_kp.p, w.kp.p, nF * sizeof(KeyPoint2d), hipMemcpyDeviceToHost, s);
            counted_copy(st, w.h_desc.p, descType == 0 ? (const void*)w.descU8.p : (const void*)w.descF32.p,
                         nF * (size_t)kSiftDescLen * elt, hipMemcpyDeviceToHost, s);
            counted_wait(st, s);
            for (int i = 0; i < nImages; ++i) {
                const size_t at = koff[i], n = (size_t)koff[i + 1] - at;
                fill_result(results[i], n, descType);
                std::memcpy((void*)results[i].Points, w.h_kp.p + at, n * sizeof(KeyPoint2d));
                std::memcpy(results[i].Descriptors, w.h_desc.p + at * (size_t)kSiftDescLen * elt,
                            n * (size_t)kSiftDescLen * elt);
            }
            return (long long)nF;
        } catch (...) {
            free_results(results, nImages);
            throw;
        }
    })
}

extern "C" MCV_API int mcvTestSiftBatchStats(long long* stats8) {
    MCV_GUARD(-1, {
        const SiftBatchStats& st = t_st;
        return stats8_out("mcvTestSiftBatchStats", stats8, st, {st.candidates, st.refined, st.oriented, st.kept});
    })
}

extern "C" MCV_API int mcvTestSiftBatchPlan(const mcvImage* images, int nImages, int mode, const void* config,
                                            long long* out8) {
    MCV_GUARD(-1, {
        const char* name = "mcvTestSiftBatchPlan";
        if (!out8) fail("%s: null argument", name);
        SiftBatchPlan B;
        std::string err;
        if (!sift_batch_plan(name, (const SiftImageIn*)images, nImages, mode, config, B, err)) fail("%s", err.c_str());
        sift_batch_plan_out8(B, out8);
        return 0;
    })
}
