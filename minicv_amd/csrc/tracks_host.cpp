// tracks_host.cpp — exports of track building (pairwise matches -> track CSR): the argument checks
// (tracks_ref.h, all on the host before the device is touched), staging and the launches of
// tracks.hip, and the host twin. The launches, copies, memsets and the two synchronisations of a call
// depend on whether trackOfFeature is asked for, never on B, the nodes, the edges or T.
#include "minicv_native.h"
#include "mcv_runtime.h"
#include "tracks_ref.h"
#include "kernels.h"
#include "plan.h"

#include <cstring>

using namespace mcv;

namespace {

struct TrkStats : CallStats {
    long long candidates = 0, longCandidates = 0, keptEdges = 0;
};
// The host side of the calling thread's last call: its statistics (mcvTestTracksStats) and the staging
// trk_prepare fills before the device is touched. No device resource, so not part of the workspace.
struct TrkHost {
    TrkStats st;
    std::vector<int> base, edges;
};
thread_local TrkHost t_host;

struct TrkWork : DeviceWs {
    DevBuf<int> edges, base, parent, size, cursor, trk, slots, candList, longList, trackOffsets, cameraIdx,
        featureIdx, trackOfFeature;
    DevBuf<uint8_t> touched;
    DevBuf<unsigned long long> blockSums, ctr;
};

void copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    counted_copy(t_host.st, dst, src, bytes, kind, s);   // by the call's form: an empty array changes no count
}

void check_fit(const char* name, long long T, long long nObs, int maxTracks, int maxObs) {
    if (T > maxTracks) fail("%s: %lld tracks do not fit maxTracks = %d", name, T, maxTracks);
    if (nObs > maxObs) fail("%s: %lld observations do not fit maxObs = %d", name, nObs, maxObs);
}

}  // namespace

extern "C" MCV_API int cvBuildTracks(const int* featureCounts, int nImages, const int* imagePairs, int B,
                                     const int* pairs, const int* offsets, const uint8_t* mask, int minLength,
                                     int* trackOffsets, int maxTracks, int* cameraIdx, int* featureIdx, int maxObs,
                                     int* trackOfFeature, long long* dropped) {
    MCV_GUARD(-1, {
        const char* name = "cvBuildTracks";
        TrkHost& h = t_host;
        std::string err;
        long long nEdges = 0;
        if (!trk_prepare(name, featureCounts, nImages, imagePairs, B, pairs, offsets, mask, minLength, trackOffsets,
                         maxTracks, cameraIdx, featureIdx, maxObs, h.base, &h.edges, &nEdges, err))
            fail("%s", err.c_str());
        require_device();
        h.st = TrkStats();
        h.st.keptEdges = nEdges;
        const int N = h.base[(size_t)nImages];
        if (nEdges == 0) {   // nothing is touched: no component, no track
            trackOffsets[0] = 0;
            if (trackOfFeature)
                for (int g = 0; g < N; ++g) trackOfFeature[g] = -1;
            if (dropped) dropped[0] = dropped[1] = dropped[2] = 0;
            return 0;
        }
        TrkWork& w = thread_device_ws<TrkWork>();
        hipStream_t s = w.stream();
        const size_t n = (size_t)N;
        const size_t slotCap = (size_t)(2 * nEdges < (long long)N ? 2 * nEdges : (long long)N);
        const size_t nb = (n + kTrkScanItems - 1) / kTrkScanItems;
        w.edges.ensure(2 * (size_t)nEdges);
        w.base.ensure((size_t)nImages + 1);
        w.parent.ensure(n);
        w.size.ensure(n);
        w.cursor.ensure(n);
        w.trk.ensure(n);
        w.touched.ensure(n);
        w.blockSums.ensure(nb + 1);
        w.slots.ensure(slotCap);
        w.candList.ensure(slotCap / 2 + 1);
        w.longList.ensure(slotCap / kTrkShortMax + 1);
        w.trackOffsets.ensure(slotCap / 2 + 1);
        w.cameraIdx.ensure(slotCap);
        w.featureIdx.ensure(slotCap);
        if (trackOfFeature) w.trackOfFeature.ensure(n);
        w.ctr.ensure(kTrkCtrs);
        {
            ProfScope ps("trk_upload", s);
            copy(w.base.p, h.base.data(), ((size_t)nImages + 1) * sizeof(int), hipMemcpyHostToDevice, s);
            copy(w.edges.p, h.edges.data(), 2 * (size_t)nEdges * sizeof(int), hipMemcpyHostToDevice, s);
        }
        counted_zero(h.st, w.ctr.p, kTrkCtrs * sizeof(unsigned long long), s);
        TrkDevice D;
        D.edges = w.edges.p;
        D.nEdges = nEdges;
        D.base = w.base.p;
        D.nImages = nImages;
        D.nNodes = N;
        D.minLength = minLength;
        D.parent = w.parent.p;
        D.size = w.size.p;
        D.cursor = w.cursor.p;
        D.trk = w.trk.p;
        D.touched = w.touched.p;
        D.blockSums = w.blockSums.p;
        D.slotCap = (int)slotCap;
        D.slots = w.slots.p;
        D.candList = w.candList.p;
        D.longList = w.longList.p;
        D.trackOffsets = w.trackOffsets.p;
        D.cameraIdx = w.cameraIdx.p;
        D.featureIdx = w.featureIdx.p;
        D.trackOfFeature = trackOfFeature ? w.trackOfFeature.p : nullptr;
        D.ctr = w.ctr.p;
        launch_build_tracks(D, s);
        h.st.launches += kTrkLaunches;
        MCV_HIP(hipGetLastError());
        // the one read-back: T, nObs, the drop counters and the fail word; the outputs follow it
        unsigned long long ctr[kTrkCtrs];
        copy(ctr, w.ctr.p, sizeof(ctr), hipMemcpyDeviceToHost, s);
        counted_wait(h.st, s);
        if (ctr[3]) fail("%s: a bounded loop of the union gave up (fail word %llu)", name, ctr[3]);
        const long long T = (long long)(ctr[5] >> 32), nObs = (long long)(ctr[5] & 0xffffffffull);
        h.st.candidates = (long long)(ctr[4] >> 32);
        h.st.longCandidates = (long long)ctr[6];
        check_fit(name, T, nObs, maxTracks, maxObs);
        {
            ProfScope ps("trk_download", s);
            copy(trackOffsets, w.trackOffsets.p, ((size_t)T + 1) * sizeof(int), hipMemcpyDeviceToHost, s);
            copy(cameraIdx, w.cameraIdx.p, (size_t)nObs * sizeof(int), hipMemcpyDeviceToHost, s);
            copy(featureIdx, w.featureIdx.p, (size_t)nObs * sizeof(int), hipMemcpyDeviceToHost, s);
            if (trackOfFeature)
                copy(trackOfFeature, w.trackOfFeature.p, n * sizeof(int), hipMemcpyDeviceToHost, s);
        }
        counted_wait(h.st, s);
        if (dropped)
            for (int k = 0; k < 3; ++k) dropped[k] = (long long)ctr[k];
        return (int)T;
    })
}

extern "C" MCV_API int mcvHostBuildTracks(const int* featureCounts, int nImages, const int* imagePairs, int B,
                                          const int* pairs, const int* offsets, const uint8_t* mask, int minLength,
                                          int* trackOffsets, int maxTracks, int* cameraIdx, int* featureIdx,
                                          int maxObs, int* trackOfFeature, long long* dropped) {
    MCV_GUARD(-1, {
        const char* name = "mcvHostBuildTracks";
        std::vector<int> base, edges;
        std::string err;
        long long nEdges = 0;
        if (!trk_prepare(name, featureCounts, nImages, imagePairs, B, pairs, offsets, mask, minLength, trackOffsets,
                         maxTracks, cameraIdx, featureIdx, maxObs, base, &edges, &nEdges, err))
            fail("%s", err.c_str());
        TrkResult R;
        trk_host_build(base.data(), nImages, edges.data(), nEdges, minLength, R);
        const size_t T = R.trackOffsets.size() - 1, nObs = R.cameraIdx.size();
        check_fit(name, (long long)T, (long long)nObs, maxTracks, maxObs);
        std::memcpy(trackOffsets, R.trackOffsets.data(), (T + 1) * sizeof(int));
        if (nObs) {
            std::memcpy(cameraIdx, R.cameraIdx.data(), nObs * sizeof(int));
            std::memcpy(featureIdx, R.featureIdx.data(), nObs * sizeof(int));
        }
        if (trackOfFeature && !R.trackOfFeature.empty())
            std::memcpy(trackOfFeature, R.trackOfFeature.data(), R.trackOfFeature.size() * sizeof(int));
        if (dropped)
            for (int k = 0; k < 3; ++k) dropped[k] = R.dropped[k];
        return (int)T;
    })
}

extern "C" MCV_API int mcvTestTracksStats(long long* stats8) {
    MCV_GUARD(-1, {
        const TrkStats& st = t_host.st;
        return stats8_out("mcvTestTracksStats", stats8, st, {st.candidates, st.longCandidates, st.keptEdges});
    })
}
