// triangulate_host.cpp — exports of track triangulation (Ray.intersection, Utilities.fs:100-165, for
// many tracks in one call): argument checks, staging and the launches of triangulate.hip, and the
// host twins (triangulate_ref.h). The number of launches, copies and synchronisations of a call
// depends on which export it is and on whether statistics are asked for, never on T.
#include "minicv_native.h"
#include "mcv_runtime.h"
#include "triangulate_ref.h"
#include "kernels.h"

using namespace mcv;

namespace {

static_assert(sizeof(mcvRay3d) == 48 && sizeof(mcvCamera) == 112, "rays and cameras are read as plain doubles");

struct TriStats : CallStats {
    long long shortTracks = 0, longTracks = 0;
};
thread_local TriStats t_stats;   // the calling thread's last call (mcvTestTriangulateStats)

struct TriWork : DeviceWs {
    DevBuf<double> rays, obs, cameras, points, cost;
    DevBuf<int> offsets, camIdx, counts, visible, longList;
    DevBuf<unsigned int> ctr;
};

void copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    counted_copy(t_stats, dst, src, bytes, kind, s);   // by the call's form: an empty array changes no count
}

void check_host_offsets(const char* name, const int* offsets, int T) {
    int t = 0;
    switch (tri_check_offsets(offsets, T, &t)) {
        case 1: fail("%s: offsets[0] = %d, not 0", name, offsets[0]);
        case 2: fail("%s: offsets decrease at track %d (%d after %d)", name, t, offsets[t + 1], offsets[t]);
        case 3:
            fail("%s: track %d has %d rays, over MCV_MAX_TRACK_LEN = %d", name, t, offsets[t + 1] - offsets[t],
                 MCV_MAX_TRACK_LEN);
        default: break;
    }
}

void check_host_cameras(const char* name, const int* cameraIdx, long long n, int nCameras) {
    if (nCameras < 0) fail("%s: negative nCameras", name);
    const long long bad = tri_check_cameras(cameraIdx, n, nCameras);
    if (bad >= 0) fail("%s: cameraIdx[%lld] = %d outside [0, %d)", name, bad, cameraIdx[bad], nCameras);
}

// The launches over device arrays: d_rays given (d_cameras == nullptr) or built from the observations.
// w.ctr is zero on entry. Leaves the counters on the device; the caller reads them back.
void run_device(TriWork& w, const double* d_rays, const double* d_cameras, const int* d_camIdx, const double* d_obs,
                const int* d_offsets, int T, long long nObs, double* d_points, int* d_counts, double* d_cost,
                int* d_visible, hipStream_t s) {
    if (d_cameras) {
        w.rays.ensure(6 * (size_t)nObs);
        launch_tri_unproject(d_cameras, d_camIdx, d_obs, d_offsets, T, w.rays.p, s);
        t_stats.launches += 1;
        d_rays = w.rays.p;
    }
    w.longList.ensure((size_t)T);
    launch_tri_intersect(d_rays, d_offsets, T, d_points, d_counts, w.longList.p, w.ctr.p, s);
    t_stats.launches += 2;
    if (d_cameras && (d_cost || d_visible)) {
        launch_tri_stats(d_cameras, d_camIdx, d_obs, d_offsets, T, d_points, d_cost, d_visible, s);
        t_stats.launches += 1;
    }
    MCV_HIP(hipGetLastError());
}

void zero_counters(TriWork& w, hipStream_t s) {
    w.ctr.ensure(kTriCtrs);
    counted_zero(t_stats, w.ctr.p, kTriCtrs * sizeof(unsigned int), s);
}

// Host-pointer calls: rays != nullptr (cvIntersectRays) or the camera form (cvTriangulateTracks).
int run_host_pointers(const char* name, const mcvRay3d* rays, const mcvCamera* cameras, int nCameras,
                      const int* cameraIdx, const mcvV2d* observations, const int* offsets, int T, mcvV3d* points,
                      int* pairCounts, double* cost, int* visible) {
    if (T < 0) fail("%s: negative T", name);
    if (T == 0) return 0;
    if (!offsets || !points || !pairCounts) fail("%s: null offsets, points or pairCounts", name);
    if (!cameras && !rays) fail("%s: null rays", name);
    if (cameras && (!cameraIdx || !observations)) fail("%s: null cameraIdx or observations", name);
    check_host_offsets(name, offsets, T);
    const long long n = offsets[T];
    if (cameras) check_host_cameras(name, cameraIdx, n, nCameras);
    require_device();
    TriWork& w = thread_device_ws<TriWork>();
    t_stats = TriStats();
    hipStream_t s = w.stream();
    w.offsets.ensure((size_t)T + 1);
    w.points.ensure(3 * (size_t)T);
    w.counts.ensure((size_t)T);
    copy(w.offsets.p, offsets, ((size_t)T + 1) * sizeof(int), hipMemcpyHostToDevice, s);
    if (cameras) {
        w.cameras.ensure(14 * (size_t)(nCameras ? nCameras : 1));
        w.camIdx.ensure((size_t)n);
        w.obs.ensure(2 * (size_t)n);
        copy(w.cameras.p, cameras, (size_t)nCameras * sizeof(mcvCamera), hipMemcpyHostToDevice, s);
        copy(w.camIdx.p, cameraIdx, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s);
        copy(w.obs.p, observations, (size_t)n * sizeof(mcvV2d), hipMemcpyHostToDevice, s);
        if (cost) w.cost.ensure((size_t)T);
        if (visible) w.visible.ensure((size_t)T);
    } else {
        w.rays.ensure(6 * (size_t)n);
        copy(w.rays.p, rays, (size_t)n * sizeof(mcvRay3d), hipMemcpyHostToDevice, s);
    }
    zero_counters(w, s);
    run_device(w, cameras ? nullptr : w.rays.p, cameras ? w.cameras.p : nullptr, w.camIdx.p, w.obs.p, w.offsets.p, T,
               n, w.points.p, w.counts.p, cameras && cost ? w.cost.p : nullptr,
               cameras && visible ? w.visible.p : nullptr, s);
    unsigned int ctr[kTriCtrs];
    copy(points, w.points.p, (size_t)T * sizeof(mcvV3d), hipMemcpyDeviceToHost, s);
    copy(pairCounts, w.counts.p, (size_t)T * sizeof(int), hipMemcpyDeviceToHost, s);
    if (cameras && cost) copy(cost, w.cost.p, (size_t)T * sizeof(double), hipMemcpyDeviceToHost, s);
    if (cameras && visible) copy(visible, w.visible.p, (size_t)T * sizeof(int), hipMemcpyDeviceToHost, s);
    copy(ctr, w.ctr.p, sizeof(ctr), hipMemcpyDeviceToHost, s);
    counted_wait(t_stats, s);
    t_stats.longTracks = ctr[0];
    t_stats.shortTracks = (long long)T - ctr[0];
    return (int)ctr[1];
}

}  // namespace

extern "C" MCV_API int cvIntersectRays(const mcvRay3d* rays, const int* offsets, int T, mcvV3d* points,
                                       int* pairCounts) {
    MCV_GUARD(-1, {
        return run_host_pointers("cvIntersectRays", rays, nullptr, 0, nullptr, nullptr, offsets, T, points,
                                 pairCounts, nullptr, nullptr);
    })
}

extern "C" MCV_API int cvTriangulateTracks(const mcvCamera* cameras, int nCameras, const int* cameraIdx,
                                           const mcvV2d* observations, const int* offsets, int T, mcvV3d* points,
                                           int* pairCounts, double* cost, int* visible) {
    MCV_GUARD(-1, {
        if (T > 0 && !cameras) fail("cvTriangulateTracks: null cameras");
        return run_host_pointers("cvTriangulateTracks", nullptr, cameras, nCameras, cameraIdx, observations, offsets,
                                 T, points, pairCounts, cost, visible);
    })
}

extern "C" MCV_API int mcvTriangulateTracksDevice(const mcvCamera* d_cameras, int nCameras, const int* d_cameraIdx,
                                                  const mcvV2d* d_observations, const int* d_offsets, int T,
                                                  mcvV3d* d_points, int* d_pairCounts, double* d_cost,
                                                  int* d_visible) {
    MCV_GUARD(-1, {
        const char* name = "mcvTriangulateTracksDevice";
        if (T < 0) fail("%s: negative T", name);
        if (T == 0) return 0;
        if (!d_cameras || !d_cameraIdx || !d_observations || !d_offsets || !d_points || !d_pairCounts)
            fail("%s: null argument", name);
        if (nCameras < 0) fail("%s: negative nCameras", name);
        require_device();
        TriWork& w = thread_device_ws<TriWork>();
        t_stats = TriStats();
        hipStream_t s = nullptr;
        zero_counters(w, s);
        launch_tri_validate(d_offsets, T, d_cameraIdx, nCameras, w.ctr.p, s);
        t_stats.launches += 2;
        MCV_HIP(hipGetLastError());
        unsigned int ctr[kTriCtrs];
        int nObs = 0;
        copy(ctr, w.ctr.p, sizeof(ctr), hipMemcpyDeviceToHost, s);
        copy(&nObs, d_offsets + T, sizeof(int), hipMemcpyDeviceToHost, s);
        counted_wait(t_stats, s);
        if (ctr[2]) {   // the first bad track: read its offsets back for the message
            const int t = T - (int)ctr[2];
            int off[3];
            MCV_HIP(hipMemcpy(off, d_offsets, sizeof(int), hipMemcpyDeviceToHost));
            MCV_HIP(hipMemcpy(off + 1, d_offsets + t, 2 * sizeof(int), hipMemcpyDeviceToHost));
            if (off[0] != 0) fail("%s: offsets[0] = %d, not 0", name, off[0]);
            if (off[2] < off[1]) fail("%s: offsets decrease at track %d (%d after %d)", name, t, off[2], off[1]);
            fail("%s: track %d has %d rays, over MCV_MAX_TRACK_LEN = %d", name, t, off[2] - off[1],
                 MCV_MAX_TRACK_LEN);
        }
        if (ctr[4]) fail("%s: cameraIdx[%d] outside [0, %d)", name, nObs - (int)ctr[4], nCameras);
        run_device(w, nullptr, (const double*)d_cameras, d_cameraIdx, (const double*)d_observations, d_offsets, T,
                   nObs, (double*)d_points, d_pairCounts, d_cost, d_visible, s);
        copy(ctr, w.ctr.p, sizeof(ctr), hipMemcpyDeviceToHost, s);
        counted_wait(t_stats, s);
        t_stats.longTracks = ctr[0];
        t_stats.shortTracks = (long long)T - ctr[0];
        return (int)ctr[1];
    })
}

extern "C" MCV_API int mcvTestTriangulateStats(long long* stats8) {
    MCV_GUARD(-1, {
        return stats8_out("mcvTestTriangulateStats", stats8, t_stats, {t_stats.shortTracks, t_stats.longTracks});
    })
}

extern "C" MCV_API int mcvHostIntersectRays(const mcvRay3d* rays, const int* offsets, int T, mcvV3d* points,
                                            int* pairCounts) {
    MCV_GUARD(-1, {
        const char* name = "mcvHostIntersectRays";
        if (T < 0) fail("%s: negative T", name);
        if (T == 0) return 0;
        if (!rays || !offsets || !points || !pairCounts) fail("%s: null argument", name);
        check_host_offsets(name, offsets, T);
        return tri_host_intersect((const double*)rays, offsets, T, (double*)points, pairCounts);
    })
}

extern "C" MCV_API int mcvHostTriangulateTracks(const mcvCamera* cameras, int nCameras, const int* cameraIdx,
                                                const mcvV2d* observations, const int* offsets, int T,
                                                mcvV3d* points, int* pairCounts, double* cost, int* visible) {
    MCV_GUARD(-1, {
        const char* name = "mcvHostTriangulateTracks";
        if (T < 0) fail("%s: negative T", name);
        if (T == 0) return 0;
        if (!cameras || !cameraIdx || !observations || !offsets || !points || !pairCounts)
            fail("%s: null argument", name);
        check_host_offsets(name, offsets, T);
        check_host_cameras(name, cameraIdx, offsets[T], nCameras);
        return tri_host_triangulate((const double*)cameras, cameraIdx, (const double*)observations, offsets, T,
                                    (double*)points, pairCounts, cost, visible);
    })
}
