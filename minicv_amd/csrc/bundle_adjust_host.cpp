// bundle_adjust_host.cpp — cvBundleAdjust: the argument checks, the camera-side CSR, the
// staging and the launches of bundle_adjust.hip under the Levenberg-Marquardt driver of ba_ref.h, and
// the host hooks (the twin mcvHostBundleAdjust, mcvHostBaLinearize, mcvHostBaStep). Launches, copies
// and synchronisations per LM iteration and per chunk of PCG iterations never depend on the sizes.
#include "minicv_native.h"
#include "mcv_runtime.h"
#include "ba_ref.h"
#include "kernels.h"
#include "plan.h"

using namespace mcv;

namespace {

static_assert(sizeof(mcvBaConfig) == sizeof(BaConfig) && sizeof(mcvBaSummary) == sizeof(BaSummary),
              "the public records are read as ba_ref.h's");
static_assert(sizeof(mcvCamera) == 112 && sizeof(mcvV3d) == 24 && sizeof(mcvV2d) == 16, "read as plain doubles");

struct BaStats : CallStats {
    long long linearizations = 0, trials = 0, cgChunks = 0, segments = 0;
};
thread_local BaStats t_stats;   // the calling thread's last call (mcvTestBundleAdjustStats)

struct BaWork : DeviceWs {
    DevBuf<int> ints;          // offsets, cameraIdx, obsTrack, camObs, segCam, segStart, segEnd, camSegPtr, longList
    DevBuf<double> doubles;    // everything fp64
    DevBuf<uint8_t> bytes;     // fixed, used, trackUsed, active
    DevBuf<unsigned int> ctr;
    DevBuf<BaCgState> cg;
    DevBuf<BaCostRecord> rec;
};

// The checks every form shares; everything here runs before the device is touched. Fills the CSR.
void check_arguments(const char* name, const mcvCamera* cameras, int nCameras, const int* cameraIdx,
                     const mcvV2d* observations, const int* offsets, int T, const mcvV3d* points, const BaConfig& cfg,
                     BaCsr& csr) {
    if (T < 0 || nCameras < 0) fail("%s: negative T or nCameras", name);
    if (!offsets || (T > 0 && !points)) fail("%s: null offsets or points", name);
    if (nCameras > 0 && !cameras) fail("%s: null cameras", name);
    if (const char* why = ba_check_config(cfg)) fail("%s: %s", name, why);
    int t = 0;
    switch (tri_check_offsets(offsets, T, &t)) {
        case 1: fail("%s: offsets[0] = %d, not 0", name, offsets[0]);
        case 2: fail("%s: offsets decrease at track %d (%d after %d)", name, t, offsets[t + 1], offsets[t]);
        case 3:
            fail("%s: track %d has %d observations, over MCV_MAX_TRACK_LEN = %d", name, t, offsets[t + 1] - offsets[t],
                 MCV_MAX_TRACK_LEN);
        default: break;
    }
    const long long n = offsets[T];
    if (n > kBaMaxObs) fail("%s: %lld observations, over 2^26", name, n);
    if (n > 0 && (!cameraIdx || !observations)) fail("%s: null cameraIdx or observations", name);
    const long long bad = ba_build_csr(cameraIdx, offsets, T, nCameras, csr);
    if (bad >= 0) fail("%s: cameraIdx[%lld] = %d outside [0, %d)", name, bad, cameraIdx[bad], nCameras);
    const int badCam = ba_check_cameras_finite((const double*)cameras, nCameras);
    if (badCam >= 0) fail("%s: camera %d has a non-finite entry", name, badCam);
}

BaConfig config_of(const mcvBaConfig* cfg) {
    if (!cfg) return ba_default_config();
    return BaConfig{cfg->maxIterations, cfg->maxCgIterations, cfg->cgTolerance,
                    cfg->initialLambda, cfg->functionTolerance, cfg->huberDelta};
}

void copy_out(const void* src, void* dst, size_t bytes) {
    if (bytes) std::memcpy(dst, src, bytes);
}

void write_summary(mcvBaSummary* out, const BaSummary& sm) {
    if (out) std::memcpy(out, &sm, sizeof(sm));
}

// The device backend of ba_run.
struct BaGpu {
    BaDevice D;
    hipStream_t s;

    void launched(int k) {
        MCV_HIP(hipGetLastError());
        t_stats.launches += k;
    }
    void copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
        counted_copy(t_stats, dst, src, bytes, kind, s);
    }
    void sync() { counted_wait(t_stats, s); }
    void read_cost(double& cost, bool& zok) {
        BaCostRecord rec;
        copy(&rec, D.rec, sizeof(rec), hipMemcpyDeviceToHost);
        sync();
        cost = rec.cost;
        zok = rec.badz == 0;
    }

    void setup(int& usedObs, int& usedTracks) {
        launch_ba_setup(D, s);
        launched(kBaLaunchesSetup);
        unsigned int ctr[kBaCtrs];
        copy(ctr, D.ctr, sizeof(ctr), hipMemcpyDeviceToHost);
        sync();
        usedObs = (int)ctr[1];
        usedTracks = (int)ctr[2];
    }
    void cost(double& c, bool& zok) {
        launch_ba_cost(D, D.cams, D.pts, s);
        launched(kBaLaunchesCost);
        read_cost(c, zok);
    }
    void linearize() {
        launch_ba_linearize(D, s);
        launched(kBaLaunchesLinearize);
        t_stats.linearizations += 1;
    }
    bool solve(double lambda, int& cgIters) {
        D.lambda = lambda;
        counted_zero(t_stats, D.ctr + 3, sizeof(unsigned int), s);
        launch_ba_system(D, s);
        launched(kBaLaunchesSystem);
        BaCgState st;
        do {   // a chunk of iterations, then one small record; the kernels of a finished solve leave at once
            for (int i = 0; i < kBaCgChunk; ++i) launch_ba_cg_iteration(D, s);
            launched(kBaCgChunk * kBaLaunchesCgIter);
            copy(&st, D.cg, sizeof(st), hipMemcpyDeviceToHost);
            sync();
            t_stats.cgChunks += 1;
        } while (!st.done);
        cgIters = st.iter;
        return !st.failed;
    }
    void trial(double& c, bool& zok) {
        launch_ba_trial(D, s);
        launched(kBaLaunchesTrial);
        t_stats.trials += 1;
        read_cost(c, zok);
    }
    void accept() {
        std::swap(D.cams, D.cams2);
        std::swap(D.pts, D.pts2);
    }
};

template <class T>
T* carve(T*& cursor, size_t count) {
    T* p = cursor;
    cursor += count;
    return p;
}

int run_device(const mcvCamera* cameras, int nCameras, const uint8_t* fixedCameras, const int* cameraIdx,
               const mcvV2d* observations, const int* offsets, int T, const mcvV3d* points, const BaConfig& cfg,
               const BaCsr& csr, mcvCamera* outCameras, mcvV3d* outPoints, BaSummary& sm) {
    require_device();
    BaWork& w = thread_device_ws<BaWork>();
    t_stats = BaStats();
    hipStream_t s = w.stream();
    const size_t n = (size_t)offsets[T], nC = (size_t)nCameras, nT = (size_t)T, nSeg = csr.segCam.size();
    t_stats.segments = (long long)nSeg;
    const size_t nCp = nC ? nC : 1;

    w.ints.ensure((nT + 1) + 3 * n + 3 * nSeg + (nC + 1) + nT);
    w.doubles.ensure(2 * n + 2 * 14 * nC + 2 * 3 * nT + (size_t)kBaEntry * n + (21 + 6 + 21 + 6 + 6 * 5) * nC + nCp +
                     (6 + 3 + 6 + 3 + 3) * nT + 27 * (nSeg ? nSeg : 1));
    w.bytes.ensure(nC + n + nT + nC);
    w.ctr.ensure(kBaCtrs);
    w.cg.ensure(1);
    w.rec.ensure(1);

    BaDevice D{};
    D.nCameras = nCameras;
    D.T = T;
    D.n = (int)n;
    D.nSeg = (int)nSeg;
    int* ip = w.ints.p;
    int* d_offsets = carve(ip, nT + 1);
    int* d_cameraIdx = carve(ip, n);
    int* d_obsTrack = carve(ip, n);
    int* d_camObs = carve(ip, n);
    int* d_segCam = carve(ip, nSeg);
    int* d_segStart = carve(ip, nSeg);
    int* d_segEnd = carve(ip, nSeg);
    int* d_camSegPtr = carve(ip, nC + 1);
    D.longList = carve(ip, nT);
    D.offsets = d_offsets;
    D.cameraIdx = d_cameraIdx;
    D.obsTrack = d_obsTrack;
    D.camObs = d_camObs;
    D.segCam = d_segCam;
    D.segStart = d_segStart;
    D.segEnd = d_segEnd;
    D.camSegPtr = d_camSegPtr;
    double* dp = w.doubles.p;
    double* d_obs = carve(dp, 2 * n);
    D.obs = d_obs;
    D.cams = carve(dp, 14 * nC);
    D.cams2 = carve(dp, 14 * nC);
    D.pts = carve(dp, 3 * nT);
    D.pts2 = carve(dp, 3 * nT);
    D.E = carve(dp, (size_t)kBaEntry * n);
    D.U = carve(dp, 21 * nC);
    D.g = carve(dp, 6 * nC);
    D.L = carve(dp, 21 * nC);
    D.b = carve(dp, 6 * nC);
    D.x = carve(dp, 6 * nC);
    D.r = carve(dp, 6 * nC);
    D.z = carve(dp, 6 * nC);
    D.p = carve(dp, 6 * nC);
    D.q = carve(dp, 6 * nC);
    D.pq = carve(dp, nCp);
    D.V = carve(dp, 6 * nT);
    D.h = carve(dp, 3 * nT);
    D.Vinv = carve(dp, 6 * nT);
    D.t = carve(dp, 3 * nT);
    D.y = carve(dp, 3 * nT);
    D.part = carve(dp, 27 * (nSeg ? nSeg : 1));
    uint8_t* bp = w.bytes.p;
    uint8_t* d_fixed = carve(bp, nC);
    D.fixed = d_fixed;
    D.used = carve(bp, n);
    D.trackUsed = carve(bp, nT);
    D.active = carve(bp, nC);
    D.ctr = w.ctr.p;
    D.cg = w.cg.p;
    D.rec = w.rec.p;
    D.lambda = cfg.initialLambda;
    D.delta = cfg.huberDelta;
    D.tol2 = cfg.cgTolerance * cfg.cgTolerance;
    D.maxCg = cfg.maxCgIterations;

    BaGpu be{D, s};
    const hipMemcpyKind up = hipMemcpyHostToDevice;
    {
        ProfScope ps("ba_upload", s);
        be.copy(d_offsets, offsets, (nT + 1) * sizeof(int), up);
        be.copy(d_cameraIdx, cameraIdx, n * sizeof(int), up);
        be.copy(d_obsTrack, csr.obsTrack.data(), n * sizeof(int), up);
        be.copy(d_camObs, csr.camObs.data(), n * sizeof(int), up);
        be.copy(d_segCam, csr.segCam.data(), nSeg * sizeof(int), up);
        be.copy(d_segStart, csr.segStart.data(), nSeg * sizeof(int), up);
        be.copy(d_segEnd, csr.segEnd.data(), nSeg * sizeof(int), up);
        be.copy(d_camSegPtr, csr.camSegPtr.data(), (nC + 1) * sizeof(int), up);
        be.copy(d_obs, observations, n * sizeof(mcvV2d), up);
        be.copy(be.D.cams, cameras, nC * sizeof(mcvCamera), up);
        be.copy(be.D.pts, points, nT * sizeof(mcvV3d), up);
        if (fixedCameras) be.copy(d_fixed, fixedCameras, nC, up);
        else counted_zero(t_stats, d_fixed, nC, s);
        counted_zero(t_stats, D.ctr, kBaCtrs * sizeof(unsigned int), s);
        counted_zero(t_stats, D.pq, nCp * sizeof(double), s);   // the setup's per-camera marks
    }

    const int it = ba_run(be, cfg, sm);
    std::vector<double> hc(14 * nC), hp(3 * nT);   // the outputs are written only once the whole result is here
    {
        ProfScope ps("ba_download", s);
        be.copy(hc.data(), be.D.cams, nC * sizeof(mcvCamera), hipMemcpyDeviceToHost);
        be.copy(hp.data(), be.D.pts, nT * sizeof(mcvV3d), hipMemcpyDeviceToHost);
    }
    be.sync();
    copy_out(hc.data(), outCameras, nC * sizeof(mcvCamera));
    copy_out(hp.data(), outPoints, nT * sizeof(mcvV3d));
    return it;
}

}  // namespace

extern "C" MCV_API int cvBundleAdjust(const mcvCamera* cameras, int nCameras, const uint8_t* fixedCameras,
                                      const int* cameraIdx, const mcvV2d* observations, const int* offsets, int T,
                                      const mcvV3d* points, const mcvBaConfig* cfg, mcvCamera* outCameras,
                                      mcvV3d* outPoints, mcvBaSummary* summary) {
    MCV_GUARD(-1, {
        const char* name = "cvBundleAdjust";
        const BaConfig c = config_of(cfg);
        BaCsr csr;
        check_arguments(name, cameras, nCameras, cameraIdx, observations, offsets, T, points, c, csr);
        if ((nCameras > 0 && !outCameras) || (T > 0 && !outPoints)) fail("%s: null outCameras or outPoints", name);
        BaSummary sm;
        std::memset(&sm, 0, sizeof(sm));
        int it = 0;
        if (T == 0 || offsets[T] == 0) {   // nothing to adjust: the inputs, without touching the device
            sm.termination = kBaTermNothing;
            copy_out(cameras, outCameras, (size_t)nCameras * sizeof(mcvCamera));
            copy_out(points, outPoints, (size_t)T * sizeof(mcvV3d));
        } else {
            it = run_device(cameras, nCameras, fixedCameras, cameraIdx, observations, offsets, T, points, c, csr,
                            outCameras, outPoints, sm);
        }
        write_summary(summary, sm);
        return it;
    })
}

extern "C" MCV_API int mcvHostBundleAdjust(const mcvCamera* cameras, int nCameras, const uint8_t* fixedCameras,
                                           const int* cameraIdx, const mcvV2d* observations, const int* offsets,
                                           int T, const mcvV3d* points, const mcvBaConfig* cfg,
                                           mcvCamera* outCameras, mcvV3d* outPoints, mcvBaSummary* summary) {
    MCV_GUARD(-1, {
        const char* name = "mcvHostBundleAdjust";
        const BaConfig c = config_of(cfg);
        BaCsr csr;
        check_arguments(name, cameras, nCameras, cameraIdx, observations, offsets, T, points, c, csr);
        if ((nCameras > 0 && !outCameras) || (T > 0 && !outPoints)) fail("%s: null outCameras or outPoints", name);
        BaSummary sm;
        std::vector<double> hc(14 * (size_t)nCameras), hp(3 * (size_t)T);
        const int it = ba_host_bundle_adjust((const double*)cameras, nCameras, fixedCameras, cameraIdx,
                                             (const double*)observations, offsets, T, (const double*)points, c,
                                             csr, hc.data(), hp.data(), sm);
        copy_out(hc.data(), outCameras, hc.size() * sizeof(double));
        copy_out(hp.data(), outPoints, hp.size() * sizeof(double));
        write_summary(summary, sm);
        return it;
    })
}

extern "C" MCV_API int mcvHostBaLinearize(const mcvCamera* cameras, int nCameras, const uint8_t* fixedCameras,
                                          const int* cameraIdx, const mcvV2d* observations, const int* offsets,
                                          int T, const mcvV3d* points, const mcvBaConfig* cfg, uint8_t* used,
                                          double* A, double* B, double* r, double* w) {
    MCV_GUARD(-1, {
        const char* name = "mcvHostBaLinearize";
        const BaConfig c = config_of(cfg);
        BaHost H;
        check_arguments(name, cameras, nCameras, cameraIdx, observations, offsets, T, points, c, H.csr);
        const int n = offsets[T];
        if (n > 0 && (!used || !A || !B || !r || !w)) fail("%s: null output", name);
        H.init((const double*)cameras, nCameras, fixedCameras, cameraIdx, (const double*)observations, offsets, T,
               (const double*)points, c);
        int usedObs = 0, usedTracks = 0;
        H.setup(usedObs, usedTracks);
        H.linearize();
        for (int k = 0; k < n; ++k) {
            used[k] = H.used[k];
            const double* e = H.E.data() + (size_t)kBaEntry * k;
            for (int q = 0; q < 12; ++q) A[12 * (size_t)k + q] = e[q];
            for (int q = 0; q < 6; ++q) B[6 * (size_t)k + q] = e[12 + q];
            r[2 * (size_t)k] = e[18];
            r[2 * (size_t)k + 1] = e[19];
            w[k] = H.W[k];
        }
        return usedObs;
    })
}

extern "C" MCV_API int mcvHostBaStep(const mcvCamera* cameras, int nCameras, const uint8_t* fixedCameras,
                                     const int* cameraIdx, const mcvV2d* observations, const int* offsets, int T,
                                     const mcvV3d* points, const mcvBaConfig* cfg, double lambda, double* dCameras,
                                     double* dPoints) {
    MCV_GUARD(-1, {
        const char* name = "mcvHostBaStep";
        const BaConfig c = config_of(cfg);
        BaHost H;
        check_arguments(name, cameras, nCameras, cameraIdx, observations, offsets, T, points, c, H.csr);
        if (!(lambda > 0.0) || !ba_finite(lambda)) fail("%s: lambda is not positive and finite", name);
        if ((nCameras > 0 && !dCameras) || (T > 0 && !dPoints)) fail("%s: null output", name);
        H.init((const double*)cameras, nCameras, fixedCameras, cameraIdx, (const double*)observations, offsets, T,
               (const double*)points, c);
        int usedObs = 0, usedTracks = 0, cg = 0;
        H.setup(usedObs, usedTracks);
        H.linearize();
        if (!H.solve(lambda, cg)) fail("%s: the solve failed", name);
        H.apply_step(dPoints);
        copy_out(H.x.data(), dCameras, 6 * (size_t)nCameras * sizeof(double));
        return cg;
    })
}

extern "C" MCV_API int mcvTestBundleAdjustStats(long long* stats8) {
    MCV_GUARD(-1, {
        const BaStats& st = t_stats;
        return stats8_out("mcvTestBundleAdjustStats", stats8, st,
                          {st.linearizations, st.trials, st.cgChunks, st.segments});
    })
}
