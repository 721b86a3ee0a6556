// scaled_pose_host.cpp — exports of CameraPose.findScaled (CameraPose.fs:39-134):
// the per-call setup (scaled_setup.h, shared with the batch) on the host in fp64,
// the O(N^2) candidate verify on the GPU (scaled_pose.hip), and the host twin for the CPU tests.
#include "minicv_native.h"
#include "mcv_runtime.h"
#include "scaled_setup.h"
#include "kernels.h"

using namespace mcv;

namespace {

struct ScaledWork : DeviceWs {
    DevBuf<double> w, o, soa, scales, costs;
    DevBuf<uint8_t> used;
    DevBuf<long long> out;
};

// Device part shared by the host-pointer and device-pointer exports. Synchronises s.
int scaled_device(ScaledWork& w, const ScaledSetup& S, const double* d_w3, const double* d_o2, int N,
                  double* outCost, double* outScale, hipStream_t s, double* h_scales = nullptr,
                  double* h_costs = nullptr) {
    w.soa.ensure((size_t)N * 5);
    w.scales.ensure((size_t)N * 2);
    w.costs.ensure((size_t)N * 2);
    w.used.ensure((size_t)N);
    w.out.ensure(2);
    launch_scaled(S, d_w3, d_o2, N, w.soa.p, w.scales.p, w.used.p, w.costs.p, w.out.p, s);
    MCV_HIP(hipGetLastError());
    long long out[2];
    MCV_HIP(hipMemcpyAsync(out, w.out.p, sizeof(out), hipMemcpyDeviceToHost, s));
    if (h_scales) MCV_HIP(hipMemcpyAsync(h_scales, w.scales.p, (size_t)N * 2 * 8, hipMemcpyDeviceToHost, s));
    if (h_costs) MCV_HIP(hipMemcpyAsync(h_costs, w.costs.p, (size_t)N * 2 * 8, hipMemcpyDeviceToHost, s));
    MCV_HIP(hipStreamSynchronize(s));
    double cost = std::numeric_limits<double>::infinity(), scale = 0.0;
    if (out[0] >= 0) {
        MCV_HIP(hipMemcpyAsync(&cost, w.costs.p + out[0], 8, hipMemcpyDeviceToHost, s));
        MCV_HIP(hipMemcpyAsync(&scale, w.scales.p + out[0], 8, hipMemcpyDeviceToHost, s));
        MCV_HIP(hipStreamSynchronize(s));
    }
    if (outCost) *outCost = cost;
    if (outScale) *outScale = scale;
    return (int)out[1];
}

void check_args(const mcvCamera* c, const void* w, const void* o, int N, const mcvM33d* R, const mcvV3d* T) {
    if (!c || !R || !T || N < 0 || (N > 0 && (!w || !o))) fail("cvFindScaledPose: bad argument");
    if (N > (1 << 28)) fail("cvFindScaledPose: N = %d too large", N);
}

}  // namespace

extern "C" MCV_API int cvFindScaledPose(double inlierThreshold, const mcvCamera* srcCam, const mcvV3d* worldPoints,
                                        const mcvV2d* observations, int N, const mcvM33d* rotation,
                                        const mcvV3d* translation, double* outCost, double* outScale) {
    (void)inlierThreshold;   // unused by the reference too (CameraPose.fs:39; only countInliers reads it)
    MCV_GUARD(-1, {
        check_args(srcCam, worldPoints, observations, N, rotation, translation);
        if (N == 0) {   // CameraPose.fs:42: [] -> +inf, CameraPose()
            if (outCost) *outCost = std::numeric_limits<double>::infinity();
            if (outScale) *outScale = 0.0;
            return 0;
        }
        require_device();
        const ScaledSetup S = make_setup(*srcCam, *rotation, *translation);
        ScaledWork& w = thread_device_ws<ScaledWork>();
        hipStream_t s = w.stream();
        w.w.ensure((size_t)N * 3);
        w.o.ensure((size_t)N * 2);
        MCV_HIP(hipMemcpyAsync(w.w.p, worldPoints, (size_t)N * 24, hipMemcpyHostToDevice, s));
        MCV_HIP(hipMemcpyAsync(w.o.p, observations, (size_t)N * 16, hipMemcpyHostToDevice, s));
        return scaled_device(w, S, w.w.p, w.o.p, N, outCost, outScale, s);
    })
}

extern "C" MCV_API int cvFindScaledPoseCosts(const mcvCamera* srcCam, const mcvV3d* worldPoints,
                                             const mcvV2d* observations, int N, const mcvM33d* rotation,
                                             const mcvV3d* translation, double* scales, double* costs) {
    MCV_GUARD(-1, {
        check_args(srcCam, worldPoints, observations, N, rotation, translation);
        if (N == 0) return 0;
        if (!scales || !costs) fail("cvFindScaledPoseCosts: bad argument");
        require_device();
        const ScaledSetup S = make_setup(*srcCam, *rotation, *translation);
        ScaledWork& w = thread_device_ws<ScaledWork>();
        hipStream_t s = w.stream();
        w.w.ensure((size_t)N * 3);
        w.o.ensure((size_t)N * 2);
        MCV_HIP(hipMemcpyAsync(w.w.p, worldPoints, (size_t)N * 24, hipMemcpyHostToDevice, s));
        MCV_HIP(hipMemcpyAsync(w.o.p, observations, (size_t)N * 16, hipMemcpyHostToDevice, s));
        scaled_device(w, S, w.w.p, w.o.p, N, nullptr, nullptr, s, scales, costs);
        return N;
    })
}

extern "C" MCV_API int mcvFindScaledPoseDevice(const mcvCamera* srcCam, const mcvV3d* d_world, const mcvV2d* d_obs,
                                               int N, const mcvM33d* rotation, const mcvV3d* translation,
                                               double* outCost, double* outScale, void* stream) {
    MCV_GUARD(-1, {
        check_args(srcCam, d_world, d_obs, N, rotation, translation);
        if (N == 0) {
            if (outCost) *outCost = std::numeric_limits<double>::infinity();
            if (outScale) *outScale = 0.0;
            return 0;
        }
        require_device();
        const ScaledSetup S = make_setup(*srcCam, *rotation, *translation);
        return scaled_device(thread_device_ws<ScaledWork>(), S, (const double*)d_world, (const double*)d_obs, N,
                             outCost, outScale, (hipStream_t)stream);
    })
}

extern "C" MCV_API int mcvHostScaledCosts(const mcvCamera* srcCam, const mcvV3d* worldPoints,
                                          const mcvV2d* observations, int N, const mcvM33d* rotation,
                                          const mcvV3d* translation, double* scales, double* costs) {
    MCV_GUARD(-1, {
        check_args(srcCam, worldPoints, observations, N, rotation, translation);
        const ScaledSetup S = make_setup(*srcCam, *rotation, *translation);
        scaled_host_costs(S, worldPoints, observations, N, scales, costs);
        return N;
    })
}
