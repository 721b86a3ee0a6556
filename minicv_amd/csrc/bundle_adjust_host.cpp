// bundle_adjust_host.cpp — cvBundleAdjust: the argument checks, the camera-side CSR, the
// staging and the launches of bundle_adjust.hip under the Levenberg-Marquardt driver of ba_ref.h, and
// the host hooks (the twin mcvHostBundleAdjust, mcvHostBaLinearize, mcvHostBaStep). Launches, copies
// and synchronisations per LM iteration and per chunk of PCG iterations never depend on the sizes.
// cvBundleAdjustFocal and its hooks follow at the end: the same driver with the focal kernels.
#include "minicv_native.h"
#include "mcv_runtime.h"
#include "ba_ref.h"
#include "kernels.h"
#include "plan.h"

using namespace mcv;

namespace {

static_assert(sizeof(mcvBaConfig) == sizeof(BaConfig) && sizeof(mcvBaSummary) == sizeof(BaSummary),
              "the public records are read as ba_ref.h's");
static_assert(sizeof(mcvBaFocalConfig) == sizeof(BaFocalConfig) && sizeof(mcvBaFocalSummary) == sizeof(BaFocalSummary),
              "the public records are read as ba_ref.h's");
static_assert(sizeof(mcvCamera) == 112 && sizeof(mcvV3d) == 24 && sizeof(mcvV2d) == 16, "read as plain doubles");

struct BaStats : CallStats {
    long long linearizations = 0, trials = 0, cgChunks = 0, segments = 0;
};
thread_local BaStats t_stats;   // the calling thread's last call (mcvTestBundleAdjustStats)
thread_local BaStats t_focal_stats;   // the same of cvBundleAdjustFocal (mcvTestBundleAdjustFocalStats)

struct BaWork : DeviceWs {
    DevBuf<int> ints;          // offsets, cameraIdx, obsTrack, camObs, segCam, segStart, segEnd, camSegPtr, longList
    DevBuf<double> doubles;    // everything fp64
    DevBuf<uint8_t> bytes;     // fixed, used, trackUsed, active
    DevBuf<unsigned int> ctr;
    DevBuf<BaCgState> cg;
    DevBuf<BaCostRecord> rec;
    DevBuf<int> focalInts;        // camGrp, grpPtr, grpCam
    DevBuf<double> focalDoubles;  // Ef, partF and the groups' vectors
    DevBuf<uint8_t> focalBytes;   // grpFixed, grpFree
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
// fm != 0: the focal kernels (§7p) stand in for their stages; fm == 0 is cvBundleAdjust's sequence.
struct BaGpu {
    BaDevice D;
    hipStream_t s;
    BaStats& t_stats;   // the calling export's counters
    int fm = 0;
    BaFocal F{};
    int freeGroups = 0;

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
        if (fm) launch_baf_setup(D, F, s);
        else launch_ba_setup(D, s);
        launched(fm ? kBafLaunchesSetup : kBaLaunchesSetup);
        unsigned int ctr[kBaCtrs];
        copy(ctr, D.ctr, sizeof(ctr), hipMemcpyDeviceToHost);
        sync();
        usedObs = (int)ctr[1];
        usedTracks = (int)ctr[2];
        freeGroups = (int)ctr[5];
    }
    void cost(double& c, bool& zok) {
        launch_ba_cost(D, D.cams, D.pts, s);
        launched(kBaLaunchesCost);
        read_cost(c, zok);
    }
    void linearize() {
        if (fm) launch_baf_linearize(D, F, s);
        else launch_ba_linearize(D, s);
        launched(fm ? kBafLaunchesLinearize : kBaLaunchesLinearize);
        t_stats.linearizations += 1;
    }
    bool solve(double lambda, int& cgIters) {
        D.lambda = lambda;
        counted_zero(t_stats, D.ctr + 3, sizeof(unsigned int), s);
        if (fm) launch_baf_system(D, F, s);
        else launch_ba_system(D, s);
        launched(fm ? kBafLaunchesSystem : kBaLaunchesSystem);
        BaCgState st;
        do {   // a chunk of iterations, then one small record; the kernels of a finished solve leave at once
            for (int i = 0; i < kBaCgChunk; ++i) {
                if (fm) launch_baf_cg_iteration(D, F, s);
                else launch_ba_cg_iteration(D, s);
            }
            launched(kBaCgChunk * (fm ? kBafLaunchesCgIter : kBaLaunchesCgIter));
            copy(&st, D.cg, sizeof(st), hipMemcpyDeviceToHost);
            sync();
            t_stats.cgChunks += 1;
        } while (!st.done);
        cgIters = st.iter;
        return !st.failed;
    }
    void trial(double& c, bool& zok) {
        if (fm) launch_baf_trial(D, F, s);
        else launch_ba_trial(D, s);
        launched(fm ? kBafLaunchesTrial : kBaLaunchesTrial);
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
               const BaCsr& csr, mcvCamera* outCameras, mcvV3d* outPoints, BaSummary& sm, BaStats& t_stats = ::t_stats,
               int fm = 0, const BaGroups* grp = nullptr, int* freeGroups = nullptr) {
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

    BaGpu be{D, s, t_stats};
    const size_t nG = fm ? (size_t)grp->nG : 0, nGp = nG ? nG : 1;
    int *d_camGrp = nullptr, *d_grpPtr = nullptr, *d_grpCam = nullptr;
    uint8_t* d_grpFixed = nullptr;
    if (fm) {
        w.focalInts.ensure(2 * nC + nG + 1);
        w.focalDoubles.ensure(2 * n + (size_t)kBaFocalPart * (nSeg ? nSeg : 1) + (2 + 2 + 3 + 2 + 2 * 5 + 1) * nGp);
        w.focalBytes.ensure(2 * nGp);
        BaFocal& F = be.F;
        be.fm = F.fm = fm;
        F.nG = (int)nG;
        int* fi = w.focalInts.p;
        F.camGrp = d_camGrp = carve(fi, nC);
        F.grpPtr = d_grpPtr = carve(fi, nG + 1);
        F.grpCam = d_grpCam = carve(fi, nC);
        double* fd = w.focalDoubles.p;
        F.Ef = carve(fd, 2 * n);
        F.partF = carve(fd, (size_t)kBaFocalPart * (nSeg ? nSeg : 1));
        F.Gd = carve(fd, 2 * nGp);
        F.gf = carve(fd, 2 * nGp);
        F.Lf = carve(fd, 3 * nGp);
        F.bf = carve(fd, 2 * nGp);
        F.xf = carve(fd, 2 * nGp);
        F.rf = carve(fd, 2 * nGp);
        F.zf = carve(fd, 2 * nGp);
        F.pf = carve(fd, 2 * nGp);
        F.qf = carve(fd, 2 * nGp);
        F.pqf = carve(fd, nGp);
        uint8_t* fb = w.focalBytes.p;
        F.grpFixed = d_grpFixed = carve(fb, nGp);
        F.grpFree = carve(fb, nGp);
    }
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
        if (fm) {
            be.copy(d_camGrp, grp->camGrp.data(), nC * sizeof(int), up);
            be.copy(d_grpPtr, grp->grpPtr.data(), (nG + 1) * sizeof(int), up);
            be.copy(d_grpCam, grp->grpCam.data(), nC * sizeof(int), up);
            be.copy(d_grpFixed, grp->grpFixed.data(), nG, up);
        }
    }

    const int it = ba_run(be, cfg, sm);
    std::vector<double> hc(14 * nC), hp(3 * nT);   // the outputs are written only once the whole result is here
    {
        ProfScope ps("ba_download", s);
        be.copy(hc.data(), be.D.cams, nC * sizeof(mcvCamera), hipMemcpyDeviceToHost);
        be.copy(hp.data(), be.D.pts, nT * sizeof(mcvV3d), hipMemcpyDeviceToHost);
    }
    be.sync();
    if (freeGroups) *freeGroups = fm ? be.freeGroups : 0;
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

// ---- focal groups ----
namespace {

BaFocalConfig focal_config_of(const mcvBaFocalConfig* cfg) {
    if (!cfg) return BaFocalConfig{ba_default_config(), 1, 0};
    return BaFocalConfig{config_of(&cfg->base), cfg->focalMode, 0};
}

// cvBundleAdjust's checks, then the groups'. Everything here runs before the device is touched.
void check_focal_arguments(const char* name, const mcvCamera* cameras, int nCameras, const int* focalGroup,
                           const uint8_t* fixedFocal, const int* cameraIdx, const mcvV2d* observations,
                           const int* offsets, int T, const mcvV3d* points, const BaFocalConfig& cfg, BaCsr& csr,
                           BaGroups& grp) {
    if (cfg.focalMode < 0 || cfg.focalMode > 2) fail("%s: unknown focalMode %d", name, cfg.focalMode);
    check_arguments(name, cameras, nCameras, cameraIdx, observations, offsets, T, points, cfg.base, csr);
    int j = 0;
    switch (ba_build_groups(cfg.focalMode, focalGroup, fixedFocal, (const double*)cameras, nCameras, grp, &j)) {
        case 1: fail("%s: unknown focalMode %d", name, cfg.focalMode);
        case 2: fail("%s: focalGroup[%d] = %d outside [0, %d)", name, j, focalGroup[j], nCameras);
        case 3: fail("%s: camera %d's focal length differs from its group's", name, j);
        case 4: fail("%s: camera %d's focal length is free and not finite and positive", name, j);
        default: break;
    }
}

void write_focal_summary(mcvBaFocalSummary* out, const BaFocalSummary& sm) {
    if (out) std::memcpy(out, &sm, sizeof(sm));
}

}  // namespace

extern "C" MCV_API int cvBundleAdjustFocal(const mcvCamera* cameras, int nCameras, const uint8_t* fixedCameras,
                                           const int* focalGroup, const uint8_t* fixedFocal, const int* cameraIdx,
                                           const mcvV2d* observations, const int* offsets, int T,
                                           const mcvV3d* points, const mcvBaFocalConfig* cfg, mcvCamera* outCameras,
                                           mcvV3d* outPoints, mcvBaFocalSummary* summary) {
    MCV_GUARD(-1, {
        const char* name = "cvBundleAdjustFocal";
        const BaFocalConfig c = focal_config_of(cfg);
        BaCsr csr;
        BaGroups grp;
        check_focal_arguments(name, cameras, nCameras, focalGroup, fixedFocal, cameraIdx, observations, offsets, T,
                              points, c, csr, grp);
        if ((nCameras > 0 && !outCameras) || (T > 0 && !outPoints)) fail("%s: null outCameras or outPoints", name);
        BaFocalSummary sm;
        std::memset(&sm, 0, sizeof(sm));
        int it = 0;
        if (T == 0 || offsets[T] == 0) {   // nothing to adjust: the inputs, without touching the device
            sm.base.termination = kBaTermNothing;
            copy_out(cameras, outCameras, (size_t)nCameras * sizeof(mcvCamera));
            copy_out(points, outPoints, (size_t)T * sizeof(mcvV3d));
        } else {
            it = run_device(cameras, nCameras, fixedCameras, cameraIdx, observations, offsets, T, points, c.base, csr,
                            outCameras, outPoints, sm.base, t_focal_stats, c.focalMode, &grp, &sm.freeFocalGroups);
        }
        write_focal_summary(summary, sm);
        return it;
    })
}

extern "C" MCV_API int mcvHostBundleAdjustFocal(const mcvCamera* cameras, int nCameras, const uint8_t* fixedCameras,
                                                const int* focalGroup, const uint8_t* fixedFocal,
                                                const int* cameraIdx, const mcvV2d* observations, const int* offsets,
                                                int T, const mcvV3d* points, const mcvBaFocalConfig* cfg,
                                                mcvCamera* outCameras, mcvV3d* outPoints, mcvBaFocalSummary* summary) {
    MCV_GUARD(-1, {
        const char* name = "mcvHostBundleAdjustFocal";
        const BaFocalConfig c = focal_config_of(cfg);
        BaCsr csr;
        BaGroups grp;
        check_focal_arguments(name, cameras, nCameras, focalGroup, fixedFocal, cameraIdx, observations, offsets, T,
                              points, c, csr, grp);
        if ((nCameras > 0 && !outCameras) || (T > 0 && !outPoints)) fail("%s: null outCameras or outPoints", name);
        BaFocalSummary sm;
        std::memset(&sm, 0, sizeof(sm));
        std::vector<double> hc(14 * (size_t)nCameras), hp(3 * (size_t)T);
        const int it = ba_host_bundle_adjust_focal((const double*)cameras, nCameras, fixedCameras, cameraIdx,
                                                   (const double*)observations, offsets, T, (const double*)points, c,
                                                   csr, grp, hc.data(), hp.data(), sm);
        copy_out(hc.data(), outCameras, hc.size() * sizeof(double));
        copy_out(hp.data(), outPoints, hp.size() * sizeof(double));
        write_focal_summary(summary, sm);
        return it;
    })
}

extern "C" MCV_API int mcvHostBaFocalStep(const mcvCamera* cameras, int nCameras, const uint8_t* fixedCameras,
                                          const int* focalGroup, const uint8_t* fixedFocal, const int* cameraIdx,
                                          const mcvV2d* observations, const int* offsets, int T, const mcvV3d* points,
                                          const mcvBaFocalConfig* cfg, double lambda, double* focalBlocks,
                                          double* dCameras, double* dFocal, double* dPoints) {
    MCV_GUARD(-1, {
        const char* name = "mcvHostBaFocalStep";
        const BaFocalConfig c = focal_config_of(cfg);
        BaHost H;
        check_focal_arguments(name, cameras, nCameras, focalGroup, fixedFocal, cameraIdx, observations, offsets, T,
                              points, c, H.csr, H.grp);
        if (c.focalMode == 0) fail("%s: focalMode 0 has no focal step", name);
        if (!(lambda > 0.0) || !ba_finite(lambda)) fail("%s: lambda is not positive and finite", name);
        const int n = offsets[T];
        if ((nCameras > 0 && (!dCameras || !dFocal)) || (T > 0 && !dPoints) || (n > 0 && !focalBlocks))
            fail("%s: null output", name);
        H.init((const double*)cameras, nCameras, fixedCameras, cameraIdx, (const double*)observations, offsets, T,
               (const double*)points, c.base);
        H.fm = c.focalMode;
        int usedObs = 0, usedTracks = 0, cg = 0;
        H.setup(usedObs, usedTracks);
        H.linearize();
        if (!H.solve(lambda, cg)) fail("%s: the solve failed", name);
        H.apply_step(dPoints);
        copy_out(H.Ef.data(), focalBlocks, 2 * (size_t)n * sizeof(double));
        copy_out(H.x.data(), dCameras, 6 * (size_t)nCameras * sizeof(double));
        for (int j = 0; j < nCameras; ++j) {
            dFocal[2 * (size_t)j] = H.xf[2 * (size_t)H.grp.camGrp[j]];
            dFocal[2 * (size_t)j + 1] = H.xf[2 * (size_t)H.grp.camGrp[j] + 1];
        }
        return cg;
    })
}

extern "C" MCV_API int mcvTestBundleAdjustFocalStats(long long* stats8) {
    MCV_GUARD(-1, {
        const BaStats& st = t_focal_stats;
        return stats8_out("mcvTestBundleAdjustFocalStats", stats8, st,
                          {st.linearizations, st.trials, st.cgChunks, st.segments});
    })
}
