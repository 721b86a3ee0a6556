// sift_host.cpp — cvDetectFeatures (mode 4, SIFT) and its host twin: the argument checks
// and the plan (sift_ref.h, on the host before the device is touched), the launches of sift.hip and
// the three counter reads that size what follows them. The launches, copies, memsets and the four
// synchronisations of a call depend on nOctaves, OctaveLayers and FeatureCount > 0, never on the image
// content or the keypoint count: a stage with nothing to do is still launched, over one block.
#include "minicv_native.h"
#include "mcv_runtime.h"
#include "sift_ref.h"
#include "kernels.h"
#include "plan.h"

#include <cstring>

using namespace mcv;

static_assert(sizeof(SiftConfig) == 40 && sizeof(SiftConfigIn) == 40, "SiftConfig is 40 bytes");
static_assert(sizeof(KeyPoint2d) == 28 && sizeof(SiftKeyPointOut) == 28, "KeyPoint2d is 28 bytes");

namespace {

struct SiftStats : CallStats {
    long long candidates = 0, refined = 0, oriented = 0, kept = 0;
};
thread_local SiftStats t_st;

// What mcvTestSiftStage reads of the calling thread's last finished call: the device whose workspace
// holds the stages, and their sizes. Like the statistics it is reset once the arguments have passed
// their checks, so a call that fails on the device leaves none.
struct SiftStage {
    bool done = false;
    int dev = -1;
    size_t pyramidFloats = 0;
    long long candidates = 0;
};
thread_local SiftStage t_stage;

struct SiftWork : DeviceWs {
    DevBuf<uint8_t> img, flagA, flagB, descU8;
    DevBuf<float> up, tmp, pyr, taps, descF32;
    DevBuf<int> cand, perm, sortedIdx;
    DevBuf<SiftKp> kps;
    DevBuf<SiftRec> recs, sorted;
    DevBuf<unsigned long long> keys, starts, rkeys, skeys, srkeys;
    DevBuf<unsigned> ctr;
    DevBuf<SiftKeyPointOut> kp;
};

DetectorResult* make_result(size_t n, int descType) {
    DetectorResult* res = new DetectorResult();
    res->PointCount = (int)n;
    res->DescriptorEntries = (int)(n * (size_t)kSiftDescLen);
    res->DescriptorElementType = descType;
    res->Points = new KeyPoint2d[n ? n : 1];
    res->Descriptors = new uint8_t[(n ? n : 1) * (size_t)kSiftDescLen * (descType == 0 ? 1 : sizeof(float))];
    return res;
}

void check_candidates(const char* name, long long n) {
    if (n > kSiftMaxCandidates)
        fail("%s: %lld extremum candidates exceed the cap of %d (raise ContrastThreshold)", name, n,
             kSiftMaxCandidates);
}

}  // namespace

extern "C" MCV_API DetectorResult* cvDetectFeatures(char* data, int width, int height, int channels, int mode,
                                                    void* config) {
    MCV_GUARD(nullptr, {
        const char* name = "cvDetectFeatures";
        SiftPlan S;
        std::string err;
        if (!sift_plan(name, data, width, height, channels, mode, config, S, err)) fail("%s", err.c_str());
        require_device();
        SiftStats& st = t_st;
        st = SiftStats();
        SiftStage& stage = t_stage;
        stage = SiftStage();
        MCV_HIP(hipGetDevice(&stage.dev));
        if (S.nOctaves == 0) {
            stage.done = true;
            return make_result(0, S.descType);
        }
        SiftWork& w = thread_device_ws_on<SiftWork>(stage.dev);
        hipStream_t s = w.stream();
        const int nl = S.P.nl, W0 = S.ow[0], H0 = S.oh[0];
        const size_t imgBytes = (size_t)width * (size_t)height * (size_t)channels;
        w.img.ensure(imgBytes);
        w.up.ensure((size_t)W0 * (size_t)H0);
        w.tmp.ensure((size_t)W0 * (size_t)H0);
        w.pyr.ensure(S.pyramidFloats);
        w.taps.ensure(S.taps.size());
        int nBuckets = 0;   // one per (octave, layer, row): the order stage's counters follow the call's four
        for (int o = 0; o < S.nOctaves; ++o) nBuckets += nl * S.oh[(size_t)o];
        w.ctr.ensure((size_t)kSiftCtrs + 2 * (size_t)nBuckets + 1);
        unsigned* bcnt = w.ctr.p + kSiftCtrs;
        long long interior = 0;
        for (int o = 0; o < S.nOctaves; ++o)
            interior += (long long)std::max(S.ow[(size_t)o] - 2 * kSiftBorder, 0) *
                        (long long)std::max(S.oh[(size_t)o] - 2 * kSiftBorder, 0) * nl;
        const unsigned capC = (unsigned)std::min<long long>(std::max<long long>(interior, 1), kSiftMaxCandidates);
        w.cand.ensure(4 * (size_t)capC);
        SiftPyramid Y;
        std::memset(&Y, 0, sizeof Y);
        Y.base = w.pyr.p;
        for (int o = 0, rows = 0; o < S.nOctaves; ++o) {
            Y.obase[o] = S.obase[(size_t)o];
            Y.ow[o] = S.ow[(size_t)o];
            Y.oh[o] = S.oh[(size_t)o];
            Y.rowBase[o] = rows;
            rows += nl * S.oh[(size_t)o];
        }
        counted_copy(st, w.img.p, data, imgBytes, hipMemcpyHostToDevice, s);
        counted_copy(st, w.taps.p, S.taps.data(), S.taps.size() * sizeof(float), hipMemcpyHostToDevice, s);
        counted_zero(st, w.ctr.p, ((size_t)kSiftCtrs + (size_t)nBuckets) * sizeof(unsigned), s);
        {
            ProfScope ps("sift_pyramid", s);
            launch_sift_grey_double(w.img.p, width, height, channels, w.up.p, s);
            launch_sift_blur(w.up.p, w.pyr.p, w.tmp.p, W0, H0, w.taps.p + S.tapOff[0], S.tapRadius[0], s);
            st.launches += 1 + kSiftLaunchesPerBlur;
        }
        for (int o = 0; o < S.nOctaves; ++o) {
            const int ow = S.ow[(size_t)o], oh = S.oh[(size_t)o];
            const size_t plane = (size_t)ow * (size_t)oh;
            float* g = w.pyr.p + S.obase[(size_t)o];
            {
                ProfScope ps("sift_pyramid", s);
                if (o > 0) {
                    const int pw = S.ow[(size_t)o - 1];
                    launch_sift_downsample(w.pyr.p + S.obase[(size_t)o - 1] +
                                               (size_t)nl * (size_t)pw * (size_t)S.oh[(size_t)o - 1],
                                           pw, g, ow, oh, s);
                    st.launches += kSiftLaunchesDownsample;
                }
                for (int i = 1; i < nl + 3; ++i) {
                    launch_sift_blur(g + (size_t)(i - 1) * plane, g + (size_t)i * plane, w.tmp.p, ow, oh,
                                     w.taps.p + S.tapOff[(size_t)i], S.tapRadius[(size_t)i], s);
                    st.launches += kSiftLaunchesPerBlur;
                }
            }
            ProfScope ps("sift_extrema", s);
            launch_sift_extrema(g, ow, oh, o, nl, S.P.thr, w.cand.p, capC, w.ctr.p, s);
            st.launches += kSiftLaunchesExtrema;
        }
        MCV_HIP(hipGetLastError());
        unsigned ctr[kSiftCtrs];
        counted_copy(st, ctr, w.ctr.p, sizeof ctr, hipMemcpyDeviceToHost, s);
        counted_wait(st, s);
        st.candidates = ctr[0];
        check_candidates(name, st.candidates);
        const int nC = (int)ctr[0];
        const size_t capK = (size_t)kSiftMaxPeaks * (size_t)std::max(nC, 1);
        w.kps.ensure((size_t)std::max(nC, 1));
        w.recs.ensure(capK);
        w.keys.ensure(capK);
        w.starts.ensure(capK);
        w.rkeys.ensure(capK);
        {
            ProfScope ps("sift_refine", s);
            launch_sift_refine(Y, S.P, w.cand.p, nC, w.kps.p, w.ctr.p, s);
        }
        {
            ProfScope ps("sift_orient", s);
            launch_sift_orient(Y, w.cand.p, w.kps.p, nC, w.recs.p, w.keys.p, w.starts.p, w.rkeys.p, w.ctr.p, bcnt,
                               s);
        }
        st.launches += 2;
        MCV_HIP(hipGetLastError());
        counted_copy(st, ctr, w.ctr.p, sizeof ctr, hipMemcpyDeviceToHost, s);
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
        {
            ProfScope ps("sift_order", s);
            SiftOrder O;
            O.nBuckets = nBuckets;
            O.bcnt = bcnt;
            O.boff = bcnt + nBuckets;
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
            O.count = w.ctr.p + 3;
            launch_sift_order(Y, O, nK, S.featureCount, s);
            st.launches += 4 + (S.featureCount > 0 ? kSiftLaunchesSelect : 0);
        }
        MCV_HIP(hipGetLastError());
        counted_copy(st, ctr, w.ctr.p, sizeof ctr, hipMemcpyDeviceToHost, s);
        counted_wait(st, s);
        st.kept = ctr[3];
        const size_t nF = (size_t)ctr[3], nf1 = nF ? nF : 1;
        const size_t descBytes = nF * (size_t)kSiftDescLen * (S.descType == 0 ? 1 : sizeof(float));
        w.kp.ensure(nf1);
        if (S.descType == 0)
            w.descU8.ensure(nf1 * (size_t)kSiftDescLen);
        else
            w.descF32.ensure(nf1 * (size_t)kSiftDescLen);
        {
            ProfScope ps("sift_describe", s);
            launch_sift_describe(Y, w.sorted.p, (int)nF, S.descType, w.kp.p, w.descU8.p, w.descF32.p, s);
            st.launches += 1;
        }
        MCV_HIP(hipGetLastError());
        DetectorResult* res = make_result(nF, S.descType);
        try {
            counted_copy(st, res->Points, w.kp.p, nF * sizeof(KeyPoint2d), hipMemcpyDeviceToHost, s);
            counted_copy(st, res->Descriptors, S.descType == 0 ? (const void*)w.descU8.p : (const void*)w.descF32.p,
                         descBytes, hipMemcpyDeviceToHost, s);
            counted_wait(st, s);
        } catch (...) {
            cvFreeFeatures(res);
            throw;
        }
        stage.pyramidFloats = S.pyramidFloats;
        stage.candidates = st.candidates;
        stage.done = true;
        return res;
    })
}

extern "C" MCV_API DetectorResult* mcvHostDetectFeatures(char* data, int width, int height, int channels, int mode,
                                                        void* config) {
    MCV_GUARD(nullptr, {
        const char* name = "mcvHostDetectFeatures";
        SiftPlan S;
        std::string err;
        if (!sift_plan(name, data, width, height, channels, mode, config, S, err)) fail("%s", err.c_str());
        SiftHostResult R;
        sift_host_detect((const uint8_t*)data, S, R);
        check_candidates(name, R.candidates);
        const size_t n = R.recs.size();
        DetectorResult* res = make_result(n, S.descType);
        for (size_t i = 0; i < n; ++i) {
            const SiftRec& q = R.recs[i];
            KeyPoint2d& k = res->Points[i];
            k.pt.X = q.x;
            k.pt.Y = q.y;
            k.size = q.size;
            k.angle = q.angle;
            k.response = q.response;
            k.octave = q.octave;
            k.class_id = -1;
            for (int e = 0; e < kSiftDescLen; ++e) {
                const float v = R.desc[i * (size_t)kSiftDescLen + (size_t)e];
                if (S.descType == 0)
                    res->Descriptors[i * (size_t)kSiftDescLen + (size_t)e] = sift_desc_byte(v);
                else
                    ((float*)res->Descriptors)[i * (size_t)kSiftDescLen + (size_t)e] = v;
            }
        }
        return res;
    })
}

// A stage of the calling thread's last finished cvDetectFeatures call on the current device, read from
// the workspace: one copy, no launch, and the call's statistics stay as they are.
extern "C" MCV_API int mcvTestSiftStage(int what, void* out, long long capBytes, long long* count) {
    MCV_GUARD(-1, {
        const char* name = "mcvTestSiftStage";
        if (what != 0 && what != 1) fail("%s: unknown stage %d (0: Gaussian pyramid, 1: candidates)", name, what);
        if (!out || !count) fail("%s: null argument", name);
        if (capBytes < 0) fail("%s: capBytes %lld is too small", name, capBytes);
        const SiftStage& stage = t_stage;
        if (!stage.done) fail("%s: the calling thread has no finished cvDetectFeatures call", name);
        int dev = -1;
        MCV_HIP(hipGetDevice(&dev));
        if (dev != stage.dev)
            fail("%s: the calling thread's last cvDetectFeatures call ran on device %d, not on the current device %d",
                 name, stage.dev, dev);
        const long long n = what == 0 ? (long long)stage.pyramidFloats : stage.candidates;
        const long long bytes = n * (what == 0 ? (long long)sizeof(float) : (long long)(4 * sizeof(int)));
        if (capBytes < bytes) fail("%s: capBytes %lld is too small: stage %d holds %lld bytes", name, capBytes, what, bytes);
        if (bytes) {
            SiftWork& w = thread_device_ws_on<SiftWork>(dev);
            const void* src = what == 0 ? (const void*)w.pyr.p : (const void*)w.cand.p;
            MCV_HIP(hipMemcpyAsync(out, src, (size_t)bytes, hipMemcpyDeviceToHost, w.stream()));
            MCV_HIP(hipStreamSynchronize(w.stream()));
        }
        *count = n;
        return 0;
    })
}

extern "C" MCV_API int mcvTestSiftStats(long long* stats8) {
    MCV_GUARD(-1, {
        const SiftStats& st = t_st;
        return stats8_out("mcvTestSiftStats", stats8, st, {st.candidates, st.refined, st.oriented, st.kept});
    })
}
