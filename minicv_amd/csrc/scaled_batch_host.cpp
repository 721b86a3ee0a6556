// scaled_batch_host.cpp — exports of the batched CameraPose.findScaled: P problems (a source
// camera and a pose each) over S observation sets given as a CSR, in one call. Argument checks and the
// index spaces (scaled_batch_index.h) on the host, the per-problem setup by the single call's make_setup
// (scaled_setup.h), the launches of scaled_batch.hip, and the sequential host twin. The launches,
// copies and synchronisations of a call depend on which export it is, never on P or S.
#include "minicv_native.h"
#include "mcv_runtime.h"
#include "scaled_setup.h"
#include "scaled_batch_index.h"
#include "kernels.h"
#include <cstring>
#include <vector>

using namespace mcv;

namespace {

static_assert(sizeof(ScaledSetup) == 59 * sizeof(double) && sizeof(ScaledBatchProb) == 16,
              "the setups, the problem table and the work list go up as one array of doubles");

struct SbStats : CallStats {
    long long problems = 0, tiles = 0;
};
thread_local SbStats t_stats;   // the calling thread's last call (mcvTestScaledBatchStats)

struct SbWork : DeviceWs {
    DevBuf<double> w, o, soa, scales, costs, res, meta;
    DevBuf<uint8_t> used;
    std::vector<double> hmeta, hres;
    std::vector<int> hlist;
};

void copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    counted_copy(t_stats, dst, src, bytes, kind, s);
}

struct SbLayout {
    std::vector<ScaledBatchProb> probs;
    long long cands = 0, blocks = 0;
    int live = 0, rows = 0;
};

// Every refusal of the batch exports, before anything is written or the device is touched. Returns false
// when P == 0 (nothing to do).
bool check_batch(const char* name, const mcvCamera* srcCams, const mcvM33d* rotations, const mcvV3d* translations,
                 const int* setIdx, int P, const mcvV3d* worldPoints, const mcvV2d* observations, const int* offsets,
                 int S, const void* out0, const void* out1, SbLayout& L) {
    if (P < 0) fail("%s: negative P", name);
    if (S < 0) fail("%s: negative S", name);
    if (P == 0) return false;
    if (!srcCams || !rotations || !translations || !offsets || !out0 || !out1)
        fail("%s: null srcCams, rotations, translations, offsets or output", name);
    if (!setIdx && S != P) fail("%s: a null setIdx needs S == P (S = %d, P = %d)", name, S, P);
    int where = 0;
    switch (scaled_batch_check_offsets(offsets, S, &where)) {
        case 1: fail("%s: offsets[0] = %d, not 0", name, offsets[0]);
        case 2: fail("%s: offsets decrease at set %d (%d after %d)", name, where, offsets[where + 1], offsets[where]);
        default: break;
    }
    if (offsets[S] > kScaledBatchMax) fail("%s: offsets[S] = %d rows, over 2^28", name, offsets[S]);
    if (offsets[S] > 0 && (!worldPoints || !observations)) fail("%s: null worldPoints or observations", name);
    const int bad = scaled_batch_check_sets(setIdx, P, S);
    if (bad >= 0) fail("%s: setIdx[%d] = %d outside [0, %d)", name, bad, setIdx[bad], S);
    L.probs.resize((size_t)P);
    L.rows = offsets[S];
    if (!scaled_batch_layout(offsets, setIdx, P, L.probs.data(), &L.cands, &L.blocks, &L.live))
        fail("%s: over 2^28 candidates (2 x the observations of every problem's set)", name);
    return true;
}

// Uploads, pack, candidates and the sweep; with `best` the per-problem reduce and its results in w.hres
// (cost[P], scale[P], evaluated[P]); h_scales / h_costs, when given, get the per-candidate arrays.
// Ends with the call's one synchronisation.
void run_device(SbWork& w, const SbLayout& L, const mcvCamera* srcCams, const mcvM33d* rotations,
                const mcvV3d* translations, int P, const mcvV3d* worldPoints, const mcvV2d* observations, bool best,
                double* h_scales, double* h_costs) {
    t_stats = SbStats();
    hipStream_t s = w.stream();
    const size_t R = (size_t)L.rows, nb = (size_t)L.blocks, nc = (size_t)L.cands;
    // one array: setups[P], problem table[P], work list[blocks]
    const size_t setupDoubles = 59 * (size_t)P, probDoubles = 2 * (size_t)P, listDoubles = (nb + 1) / 2;
    w.hmeta.assign(setupDoubles + probDoubles + listDoubles, 0.0);
    for (int p = 0; p < P; ++p) {
        if (L.probs[p].N == 0) continue;   // an empty problem's setup is never read
        const ScaledSetup S = make_setup(srcCams[p], rotations[p], translations[p]);
        std::memcpy(w.hmeta.data() + 59 * (size_t)p, &S, sizeof(S));
    }
    std::memcpy(w.hmeta.data() + setupDoubles, L.probs.data(), (size_t)P * sizeof(ScaledBatchProb));
    w.hlist.resize(nb);
    scaled_batch_work_list(L.probs.data(), P, w.hlist.data());
    std::memcpy(w.hmeta.data() + setupDoubles + probDoubles, w.hlist.data(), nb * sizeof(int));
    w.meta.ensure(w.hmeta.size());
    w.w.ensure(3 * R);
    w.o.ensure(2 * R);
    w.soa.ensure(5 * R);
    w.scales.ensure(nc);
    w.costs.ensure(nc);
    w.used.ensure(nc / 2);
    copy(w.meta.p, w.hmeta.data(), w.hmeta.size() * sizeof(double), hipMemcpyHostToDevice, s);
    copy(w.w.p, worldPoints, R * sizeof(mcvV3d), hipMemcpyHostToDevice, s);
    copy(w.o.p, observations, R * sizeof(mcvV2d), hipMemcpyHostToDevice, s);
    const ScaledSetup* d_setups = reinterpret_cast<const ScaledSetup*>(w.meta.p);
    const ScaledBatchProb* d_probs = reinterpret_cast<const ScaledBatchProb*>(w.meta.p + setupDoubles);
    const int* d_list = reinterpret_cast<const int*>(w.meta.p + setupDoubles + probDoubles);
    launch_scaled_batch_pack(w.w.p, w.o.p, L.rows, w.soa.p, s);
    launch_scaled_batch_candidates(d_setups, d_probs, d_list, (int)nb, w.soa.p, L.rows, w.scales.p, w.used.p, s);
    launch_scaled_batch_costs(d_setups, d_probs, d_list, (int)nb, w.soa.p, L.rows, w.scales.p, w.used.p, w.costs.p, s);
    t_stats.launches += 3;
    if (best) {
        w.res.ensure(3 * (size_t)P);
        w.hres.resize(3 * (size_t)P);
        launch_scaled_batch_best(d_probs, P, w.costs.p, w.scales.p, w.used.p, w.res.p, s);
        t_stats.launches += 1;
    }
    MCV_HIP(hipGetLastError());
    if (best) copy(w.hres.data(), w.res.p, 3 * (size_t)P * sizeof(double), hipMemcpyDeviceToHost, s);
    if (h_scales) copy(h_scales, w.scales.p, nc * sizeof(double), hipMemcpyDeviceToHost, s);
    if (h_costs) copy(h_costs, w.costs.p, nc * sizeof(double), hipMemcpyDeviceToHost, s);
    counted_wait(t_stats, s);
    t_stats.problems = L.live;
    t_stats.tiles = L.blocks;
}

}  // namespace

extern "C" MCV_API int cvFindScaledPoseBatch(const mcvCamera* srcCams, const mcvM33d* rotations,
                                             const mcvV3d* translations, const int* setIdx, int P,
                                             const mcvV3d* worldPoints, const mcvV2d* observations,
                                             const int* offsets, int S, double* costs, double* scales,
                                             int* evaluated) {
    MCV_GUARD(-1, {
        SbLayout L;
        if (!check_batch("cvFindScaledPoseBatch", srcCams, rotations, translations, setIdx, P, worldPoints,
                         observations, offsets, S, costs, scales, L))
            return 0;
        if (L.cands == 0) {   // every problem on an empty set (CameraPose.fs:42): nothing for the device
            for (int p = 0; p < P; ++p) {
                costs[p] = std::numeric_limits<double>::infinity();
                scales[p] = 0.0;
                if (evaluated) evaluated[p] = 0;
            }
            return 0;
        }
        require_device();
        SbWork& w = thread_device_ws<SbWork>();
        run_device(w, L, srcCams, rotations, translations, P, worldPoints, observations, true, nullptr, nullptr);
        int finite = 0;
        for (int p = 0; p < P; ++p) {
            costs[p] = w.hres[p];
            scales[p] = w.hres[(size_t)P + p];
            long long ev;   // the third part of res holds 64-bit integers
            std::memcpy(&ev, &w.hres[2 * (size_t)P + p], sizeof(ev));
            if (evaluated) evaluated[p] = (int)ev;
            finite += std::isfinite(costs[p]) ? 1 : 0;
        }
        return finite;
    })
}

extern "C" MCV_API int cvFindScaledPoseBatchCosts(const mcvCamera* srcCams, const mcvM33d* rotations,
                                                  const mcvV3d* translations, const int* setIdx, int P,
                                                  const mcvV3d* worldPoints, const mcvV2d* observations,
                                                  const int* offsets, int S, double* scales, double* costs) {
    MCV_GUARD(-1, {
        SbLayout L;
        if (!check_batch("cvFindScaledPoseBatchCosts", srcCams, rotations, translations, setIdx, P, worldPoints,
                         observations, offsets, S, scales, costs, L))
            return 0;
        if (L.cands == 0) return 0;
        require_device();
        run_device(thread_device_ws<SbWork>(), L, srcCams, rotations, translations, P, worldPoints, observations, false, scales, costs);
        return (int)(L.cands / 2);
    })
}

extern "C" MCV_API int mcvHostFindScaledPoseBatch(const mcvCamera* srcCams, const mcvM33d* rotations,
                                                  const mcvV3d* translations, const int* setIdx, int P,
                                                  const mcvV3d* worldPoints, const mcvV2d* observations,
                                                  const int* offsets, int S, double* costs, double* scales,
                                                  int* evaluated) {
    MCV_GUARD(-1, {
        SbLayout L;
        if (!check_batch("mcvHostFindScaledPoseBatch", srcCams, rotations, translations, setIdx, P, worldPoints,
                         observations, offsets, S, costs, scales, L))
            return 0;
        std::vector<double> sc, co;
        int finite = 0;
        for (int p = 0; p < P; ++p) {
            const ScaledBatchProb& pd = L.probs[p];
            double cost = std::numeric_limits<double>::infinity(), scale = 0.0;
            int n = 0;
            if (pd.N > 0) {
                const ScaledSetup S_ = make_setup(srcCams[p], rotations[p], translations[p]);
                sc.resize(2 * (size_t)pd.N);
                co.resize(2 * (size_t)pd.N);
                scaled_host_costs(S_, worldPoints + pd.rowOff, observations + pd.rowOff, pd.N, sc.data(), co.data());
                for (int i = 0; i < pd.N; ++i) {   // first strictly smaller cost (CameraPose.fs:119-125)
                    const mcvV3d& wp = worldPoints[pd.rowOff + i];
                    const mcvV2d& ob = observations[pd.rowOff + i];
                    double sx, sy;
                    if (!scaled_candidate(S_, wp.X, wp.Y, wp.Z, ob.X, ob.Y, sx, sy)) continue;   // skipped
                    for (int c = 2 * i; c < 2 * i + 2; ++c) {
                        n += 1;
                        if (co[c] < cost) {
                            cost = co[c];
                            scale = sc[c];
                        }
                    }
                }
            }
            costs[p] = cost;
            scales[p] = scale;
            if (evaluated) evaluated[p] = n;
            finite += std::isfinite(cost) ? 1 : 0;
        }
        return finite;
    })
}

extern "C" MCV_API int mcvTestScaledBatchStats(long long* stats8) {
    MCV_GUARD(-1, {
        return stats8_out("mcvTestScaledBatchStats", stats8, t_stats, {t_stats.problems, t_stats.tiles});
    })
}
