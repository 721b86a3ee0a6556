// ransac_batch_pnp_host.cpp — cvSolvePnPRansacBatch: B independent cvSolvePnPRansacCfg problems in one call
// whose kernel launches, stream synchronisations and copies do not grow with B, and the
// batched refinement behind it (cvRefinePnPBatch, cvSolvePnPRansacRefineBatch: §7k).
//
//   pack:     the raw image and world points in one copy, mcv_pnp_pack over all of them in one launch, one
//             table of cameras (8 doubles per problem)
//   rounds:   the single call's generate in its batch form (AP3P: one kernel; EPnP: the five split stages) +
//             the batched sweep over every problem still searching, one copy of the counts back, the single
//             call's sequential replay per problem on the host (mcvReplayChunk); the problems whose best
//             changed get that pose copied out of the round's buffer before the next round reuses it
//   finalize: every winner masked and counted in one launch, one copy back
//   refine:   kind 0: the winners' Levenberg-Marquardt solvers in lockstep (PnpLmStepper, the controller
//             pnp_lm loops over), one batched reduction and one read-back per step, at most 21 steps;
//             other kinds: EPnP on the inliers for all winners at once, the four read-backs of the single
//             call once each, EpnpHostSolve's algebra per job between them
// Every device step is the batch form of the single call's kernel (same body) and every host step the single
// call's own function, so each problem returns the single call's bits. Problems with exactly the sample
// size take the single export's direct solve, one by one.
//
// cvRefinePnPBatch / cvSolvePnPRansacRefineBatch: the refinement step of solvePnPInternal for
// B cameras. The rows are packed as above, every problem's selected rows are gathered into one compact array
// (mcv_mask_compact's job form + mcv_pnp_batch_gather: 2 launches, none without a mask), and the steppers of
// pnp_lm / pnp_vvs run in lockstep over the gathered rows, unmasked: the single call's sums on gathered arrays.
// The fused call runs it behind the rounds on the packed rows and the mask they left on the device.
//
// One round (B problems, every one on the device and with a winner), counted by BatchStats:
//   AP3P, NO_REFINE   launches 4 (pack, generate, sweep, mask) + 1 fetch = 5, synchronisations 2
//   EPnP kinds        generate is 5 kernels: 9 launches before the refine; + compact, prep and 6 passes = 17
//                     with 4 more synchronisations (6 in all)
//   kind 0            9 + 2 per LM step, one synchronisation per step (at most 21)
// each further round adds the generate, the sweep, a fetch and one synchronisation.
#include "minicv_native.h"
#include "mcv_runtime.h"
#include "kernels.h"
#include "hyp_pnp.h"
#include "pnp_refine.h"
#include "pnp_refine_batch_index.h"
#include "plan.h"

#include <array>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include <memory>
#include <algorithm>
#include <chrono>

namespace mcv {

namespace {

struct BatchPnpWs {
    int device = 0;
    hipStream_t stream = nullptr;
    DevBuf<double> raw, cams, scratch, lmPart, lmOut, pw, us, part;
    DevBuf<float> pts, comp;
    DevBuf<uint8_t> models, best, mask;
    DevBuf<int> table, counts, cnt, idx, ecount, tab;
    DevBuf<BatchPnpDesc> desc;
    DevBuf<BatchPnpFetch> fetch;
    DevBuf<BatchPnpFin> fin;
    DevBuf<BatchPnpLmJob> lmJobs;
    DevBuf<BatchPnpEpnpJob> eJobs;
    PinnedBuf<double> h_raw, h_cams, h_lmOut, h_part;
    PinnedBuf<uint8_t> h_best, h_mask;
    PinnedBuf<int> h_table, h_counts, h_cnt, h_ecount, h_tab;
    PinnedBuf<BatchPnpDesc> h_desc;
    PinnedBuf<BatchPnpFetch> h_fetch;
    PinnedBuf<BatchPnpFin> h_fin;
    PinnedBuf<BatchPnpLmJob> h_lmJobs;
    PinnedBuf<BatchPnpEpnpJob> h_eJobs;
    ~BatchPnpWs() {
        if (stream) (void)hipStreamDestroy(stream);
    }
};

BatchPnpWs& thread_batch_pnp_ws() {
    int dev = 0;
    MCV_HIP(hipGetDevice(&dev));
    thread_local std::vector<std::unique_ptr<BatchPnpWs>> all;
    for (auto& w : all)
        if (w->device == dev) return *w;
    all.emplace_back(new BatchPnpWs());
    all.back()->device = dev;
    MCV_HIP(hipStreamCreateWithFlags(&all.back()->stream, hipStreamNonBlocking));
    return *all.back();
}

long long us_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
}

void pnp_sync(hipStream_t s) {
    MCV_HIP(hipGetLastError());
    MCV_HIP(hipStreamSynchronize(s));
    ++batch_stats().syncs;
}
void pnp_copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    MCV_HIP(hipMemcpyAsync(dst, src, bytes, kind, s));
    ++batch_stats().copies;
}

bool camera_ok(const mcvM33d& K) {
    const double fx = K.M[0], fy = K.M[4];
    return fx != 0 && fy != 0 && std::isfinite(fx) && std::isfinite(fy);
}

struct Winner {     // a device problem with a pose
    size_t d;       // device index
    int p;          // problem
    int ptOff, N, count;
    double r[3], t[3];
    bool ok;
};

// The two refinements as the lockstep driver sees them: begin at a pose, fill a job's pose constants.
void stepper_begin(PnpLmStepper& st, const double* r, const double* t) { st.begin(r, t, 20); }
void stepper_begin(PnpVvsStepper& st, const double* r, const double* t) { st.begin(r, t, 20, 1.0); }
void stepper_job(const PnpLmStepper& st, BatchPnpLmJob& J) {
    const double* q = st.request();
    rodrigues(q, J.R, J.dR);
    for (int k = 0; k < 3; ++k) J.t[k] = q[3 + k];
}
void stepper_job(const PnpVvsStepper& st, BatchPnpLmJob& J) {
    std::memcpy(J.R, st.R, sizeof(J.R));
    std::memcpy(J.t, st.t, sizeof(J.t));
    std::memset(J.dR, 0, sizeof(J.dR));   // OpPnpVVS reads none
}

// pnp_lm(.., 20) / pnp_vvs(.., 20, 1) of every job in lockstep: job j reduces over the rows
// [ptOff, ptOff + N) of d_pts under d_mask (nullptr: all of them) with the camera h_cams + 8 d. A step is one
// copy of the table of the jobs still running up, one batched reduction (2 launches), one copy of their 28
// sums down and one synchronisation.
template <class Stepper>
void batch_pnp_lockstep(BatchPnpWs& W, std::vector<Winner*>& jobs, const double* h_cams, const void* d_pts,
                        const uint8_t* d_mask, bool vvs, hipStream_t s) {
    if (jobs.empty()) return;
    BatchStats& stats = batch_stats();
    std::vector<Stepper> st(jobs.size());
    int maxN = 0;
    for (size_t j = 0; j < jobs.size(); ++j) {
        stepper_begin(st[j], jobs[j]->r, jobs[j]->t);
        maxN = std::max(maxN, jobs[j]->N);
    }
    const size_t per = (size_t)batch_reduce_blocks(maxN);
    W.lmJobs.ensure(jobs.size());
    W.h_lmJobs.ensure(jobs.size());
    W.lmOut.ensure(jobs.size() * 28);
    W.h_lmOut.ensure(jobs.size() * 28);
    W.lmPart.ensure(jobs.size() * per * 28);
    for (;;) {
        std::vector<size_t> who;
        int actMaxN = 0;
        for (size_t j = 0; j < jobs.size(); ++j)
            if (!st[j].finished()) {
                BatchPnpLmJob& J = W.h_lmJobs.p[who.size()];
                J.ptOff = jobs[j]->ptOff;
                J.N = jobs[j]->N;
                std::memcpy(J.cam, h_cams + 8 * jobs[j]->d, sizeof(J.cam));
                stepper_job(st[j], J);
                actMaxN = std::max(actMaxN, J.N);
                who.push_back(j);
            }
        if (who.empty()) break;
        const size_t n = who.size();
        pnp_copy(W.lmJobs.p, W.h_lmJobs.p, n * sizeof(BatchPnpLmJob), hipMemcpyHostToDevice, s);
        stats.launches += launch_pnp_batch_reduce(vvs, d_pts, d_mask, W.lmJobs.p, (int)n, actMaxN, W.lmPart.p,
                                                  W.lmOut.p, s);
        pnp_copy(W.h_lmOut.p, W.lmOut.p, n * 28 * sizeof(double), hipMemcpyDeviceToHost, s);
        pnp_sync(s);
        ++stats.lmRounds;
        for (size_t k = 0; k < n; ++k) st[who[k]].feed(W.h_lmOut.p + 28 * k);
    }
    for (size_t j = 0; j < jobs.size(); ++j) st[j].result(jobs[j]->r, jobs[j]->t);
}

// The RANSAC batch's ITERATIVE tail: LM masked in place over every winner's rows.
void batch_pnp_lm(BatchPnpWs& W, std::vector<Winner*>& jobs, const double* h_cams, hipStream_t s) {
    batch_pnp_lockstep<PnpLmStepper>(W, jobs, h_cams, W.pts.p, W.mask.p, false, s);
}

// ---- the batched refinement (cvRefinePnPBatch, cvSolvePnPRansacRefineBatch) ----------
const char* const kRefineSingle = "cvRefinePnP";   // the single exports' prefix of their messages

// One copy of the raw points up and one launch of the pack over all of them: W.pts = every problem's rows.
void refine_pack(BatchPnpWs& W, const mcvV2d* img, const mcvV3d* world, int total, hipStream_t s) {
    BatchStats& stats = batch_stats();
    auto t0 = std::chrono::steady_clock::now();
    W.h_raw.ensure((size_t)total * 5);
    W.raw.ensure((size_t)total * 5);
    W.pts.ensure((size_t)total * 8);
    std::memcpy(W.h_raw.p, img, (size_t)total * sizeof(mcvV2d));
    std::memcpy(W.h_raw.p + 2 * (size_t)total, world, (size_t)total * sizeof(mcvV3d));
    stats.packUs += us_since(t0);
    pnp_copy(W.raw.p, W.h_raw.p, (size_t)total * 5 * sizeof(double), hipMemcpyHostToDevice, s);
    launch_pnp_pack(W.raw.p, W.raw.p + 2 * (size_t)total, total, W.pts.p, s);
    ++stats.launches;
}

// The host half of a refine: every problem's selected rows and place in the compact array, why a problem does
// not run, and the table of those that do (pnp_refine_batch_index.h). run (may be null): the problems asked
// for; a problem asked for that cannot run is reported through failed(p, the single call's message).
struct RefinePlan {
    std::vector<int> counts, compOff, reason;
    std::vector<RefineBatchJob> jobs;
    int largest = 0;
    bool gathered = false;
};
template <class Failed>
void refine_plan(const int* offsets, int B, const mcvM33d* K, const uint8_t* h_mask, const uint8_t* run, Failed failed,
                 RefinePlan& R) {
    R.gathered = h_mask != nullptr;
    R.counts.assign((size_t)B, 0);
    R.compOff.assign((size_t)B + 1, 0);
    R.reason.assign((size_t)B, kRefineTooFew);
    refine_batch_layout(offsets, B, h_mask, R.counts.data(), R.compOff.data());
    for (int p = 0; p < B; ++p) {
        if (run && !run[p]) continue;   // not asked for: no job, no message
        R.reason[p] = refine_batch_reason(R.counts[p], camera_ok(K[p]));
        char buf[160];
        if (R.reason[p] == kRefineTooFew) {
            snprintf(buf, sizeof(buf), "%s: need at least %d correspondences (N=%d)", kRefineSingle, kRefineMinRows,
                     R.counts[p]);
            failed(p, buf);
        } else if (R.reason[p] == kRefineBadCamera) {
            failed(p, "camera matrix needs finite non-zero fx, fy");
        }
    }
    R.jobs.resize((size_t)B);
    const int n = refine_batch_jobs(offsets, B, R.counts.data(), R.compOff.data(), R.reason.data(), R.gathered,
                                    R.jobs.data(), &R.largest);
    R.jobs.resize((size_t)n);
}

// The device half, for a call whose packed rows sit in W.pts and, with a mask, whose mask sits in W.mask with
// the bytes the plan counted: every job refines (rVecs[p], tVecs[p]) in place over its selected rows, gathered
// in index order (compact + gather, one launch each; without a mask it reduces over its own rows), as
// cvRefinePnPLM / cvRefinePnPVVS on those rows. Returns the problems refined.
int refine_on_device(BatchPnpWs& W, const RefinePlan& R, const int* offsets, int B, const mcvM33d* K,
                     const double* dist, int refineKind, mcvV3d* tVecs, mcvV3d* rVecs, uint8_t* refined,
                     hipStream_t s) {
    BatchStats& stats = batch_stats();
    const std::vector<RefineBatchJob>& tab = R.jobs;
    const std::vector<int>& compOff = R.compOff;
    const bool gathered = R.gathered;
    const int nJobs = (int)tab.size();
    if (nJobs == 0) return 0;
    const int total = offsets[B], selected = compOff[B];
    const void* d_pts = W.pts.p;
    if (gathered) {
        // every problem's selected rows into one compact array: mcv_mask_compact's job form, then one lane per
        // output row. The host counted the rows itself, so nothing is read back.
        W.eJobs.ensure((size_t)B);
        W.h_eJobs.ensure((size_t)B);
        W.ecount.ensure((size_t)B);
        W.idx.ensure((size_t)total);
        W.comp.ensure((size_t)selected * 8);
        W.tab.ensure(2 * ((size_t)B + 1));
        W.h_tab.ensure(2 * ((size_t)B + 1));
        std::memset(W.h_eJobs.p, 0, (size_t)B * sizeof(BatchPnpEpnpJob));
        for (int p = 0; p < B; ++p) {
            W.h_eJobs.p[p].ptOff = offsets[p];
            W.h_eJobs.p[p].N = offsets[p + 1] - offsets[p];
        }
        std::memcpy(W.h_tab.p, offsets, ((size_t)B + 1) * sizeof(int));
        std::memcpy(W.h_tab.p + B + 1, compOff.data(), ((size_t)B + 1) * sizeof(int));
        pnp_copy(W.eJobs.p, W.h_eJobs.p, (size_t)B * sizeof(BatchPnpEpnpJob), hipMemcpyHostToDevice, s);
        pnp_copy(W.tab.p, W.h_tab.p, 2 * ((size_t)B + 1) * sizeof(int), hipMemcpyHostToDevice, s);
        stats.launches += launch_pnp_batch_gather(W.pts.p, W.mask.p, W.eJobs.p, B, W.tab.p, W.tab.p + B + 1, selected,
                                                  W.idx.p, W.ecount.p, W.comp.p, s);
        d_pts = W.comp.p;
    }
    std::vector<double> cams((size_t)nJobs * 8);
    std::vector<Winner> win((size_t)nJobs);
    std::vector<Winner*> jobs((size_t)nJobs);
    for (int j = 0; j < nJobs; ++j) {
        const int p = tab[(size_t)j].prob;
        double* c = cams.data() + 8 * (size_t)j;
        c[0] = K[p].M[0]; c[1] = K[p].M[4]; c[2] = K[p].M[2]; c[3] = K[p].M[5];
        for (int k = 0; k < 4; ++k) c[4 + k] = dist ? dist[4 * (size_t)p + k] : 0.0;
        Winner& w = win[(size_t)j];
        w = Winner{};
        w.d = (size_t)j;
        w.p = p;
        w.ptOff = tab[(size_t)j].ptOff;
        w.N = tab[(size_t)j].N;
        w.r[0] = rVecs[p].X; w.r[1] = rVecs[p].Y; w.r[2] = rVecs[p].Z;
        w.t[0] = tVecs[p].X; w.t[1] = tVecs[p].Y; w.t[2] = tVecs[p].Z;
        w.ok = true;
        jobs[(size_t)j] = &w;
    }
    if (refineKind == 1) batch_pnp_lockstep<PnpVvsStepper>(W, jobs, cams.data(), d_pts, nullptr, true, s);
    else batch_pnp_lockstep<PnpLmStepper>(W, jobs, cams.data(), d_pts, nullptr, false, s);
    for (const Winner& w : win) {
        rVecs[w.p].X = w.r[0]; rVecs[w.p].Y = w.r[1]; rVecs[w.p].Z = w.r[2];
        tVecs[w.p].X = w.t[0]; tVecs[w.p].Y = w.t[1]; tVecs[w.p].Z = w.t[2];
        if (refined) refined[w.p] = 1;
    }
    return nJobs;
}

// epnp_inliers of every winner at once: compact + prep + the passes with grid y = the job, the single call's
// four read-backs once each. world: the caller's points (a job's first inlier as pw holds it: the double of
// its float coordinates). A job whose inlier count is below 4 fails, as epnp_inliers does.
template <class Failed>
void batch_pnp_epnp(BatchPnpWs& W, std::vector<Winner*>& jobs, const double* h_cams, const mcvV3d* world, int total,
                    Failed failed, hipStream_t s) {
    if (jobs.empty()) return;
    BatchStats& stats = batch_stats();
    const size_t n = jobs.size();
    W.eJobs.ensure(n);
    W.h_eJobs.ensure(n);
    W.ecount.ensure(n);
    W.h_ecount.ensure(n);
    W.idx.ensure((size_t)total);
    W.pw.ensure((size_t)3 * total);
    W.us.ensure((size_t)2 * total);
    int maxN = 0, maxNblk = 0;
    int64_t partTotal = 0;
    std::vector<std::array<double, 3>> p0(n);
    for (size_t j = 0; j < n; ++j) {
        BatchPnpEpnpJob& J = W.h_eJobs.p[j];
        std::memset(&J, 0, sizeof(J));
        J.ptOff = jobs[j]->ptOff;
        J.N = jobs[j]->N;
        J.n = -1;
        J.nblk = (J.N + kEpnpBlock - 1) / kEpnpBlock;
        J.partOff = partTotal;
        partTotal += (int64_t)kMtmSums * J.nblk;
        std::memcpy(J.cam, h_cams + 8 * jobs[j]->d, sizeof(J.cam));
        J.A.cam = EpnpCam{J.cam[0], J.cam[1], J.cam[2], J.cam[3]};
        maxN = std::max(maxN, J.N);
        maxNblk = std::max(maxNblk, J.nblk);
        p0[j] = {0, 0, 0};
        for (int i = 0; i < J.N; ++i)
            if (W.h_mask.p[J.ptOff + i]) {
                const mcvV3d& w = world[J.ptOff + i];
                p0[j] = {(double)(float)w.X, (double)(float)w.Y, (double)(float)w.Z};
                break;
            }
    }
    W.part.ensure((size_t)partTotal);
    W.h_part.ensure((size_t)partTotal);
    auto upload = [&]() { pnp_copy(W.eJobs.p, W.h_eJobs.p, n * sizeof(BatchPnpEpnpJob), hipMemcpyHostToDevice, s); };
    auto pass = [&](int mode, int nacc, int region, int prev) {
        stats.launches += launch_pnp_batch_epnp_pass(mode, W.eJobs.p, (int)n, maxNblk, W.ecount.p, W.pw.p, W.us.p, nacc,
                                                     region, prev, W.part.p, s);
    };
    auto fetch = [&]() {
        pnp_copy(W.h_part.p, W.part.p, (size_t)partTotal * sizeof(double), hipMemcpyDeviceToHost, s);
        pnp_sync(s);
    };
    // ---- {count, SumPw, Pw0}
    upload();
    stats.launches += launch_pnp_batch_epnp_prep(W.pts.p, W.mask.p, W.eJobs.p, (int)n, maxN, W.idx.p, W.ecount.p,
                                                 W.pw.p, W.us.p, s);
    pass(kEpnpPassSumPw, 3, 0, -1);
    pass(kEpnpPassPw0, 6, 1, 0);
    pnp_copy(W.h_ecount.p, W.ecount.p, n * sizeof(int), hipMemcpyDeviceToHost, s);
    fetch();
    std::vector<EpnpHostSolve> H(n);
    std::vector<int> nblk(n, 0);
    std::vector<char> live(n, 1);
    for (size_t j = 0; j < n; ++j) {
        BatchPnpEpnpJob& J = W.h_eJobs.p[j];
        const int c = W.h_ecount.p[j];
        J.n = std::max(c, 0);
        if (c < 4) {
            char buf[120];
            snprintf(buf, sizeof(buf), "EPnP needs at least 4 points (n=%d)", c);
            failed(jobs[j]->p, buf);
            jobs[j]->ok = false;
            live[j] = 0;
            J.n = 0;
            continue;
        }
        nblk[j] = (c + kEpnpBlock - 1) / kEpnpBlock;
        double sum[3], p6[6];
        epnp_block_sums(W.h_part.p + J.partOff, 3, nblk[j], sum);
        epnp_block_sums(W.h_part.p + J.partOff + (size_t)3 * J.nblk, 6, nblk[j], p6);
        H[j].first(J.A, sum, p6, c);
    }
    // ---- MtM
    upload();
    pass(kEpnpPassMtm, kMtmSums, 0, -1);
    fetch();
    for (size_t j = 0; j < n; ++j) {
        if (!live[j]) continue;
        BatchPnpEpnpJob& J = W.h_eJobs.p[j];
        double mtm[kMtmSums];
        epnp_block_sums(W.h_part.p + J.partOff, kMtmSums, nblk[j], mtm);
        const double q0[3] = {p0[j][0], p0[j][1], p0[j][2]};
        H[j].mtm(J.A, mtm, q0);
    }
    // ---- {Pc, Abt}
    upload();
    pass(kEpnpPassPc, 9, 0, -1);
    pass(kEpnpPassAbt, 27, 2, 0);
    fetch();
    for (size_t j = 0; j < n; ++j) {
        if (!live[j]) continue;
        BatchPnpEpnpJob& J = W.h_eJobs.p[j];
        double pcs[9], abt[27];
        epnp_block_sums(W.h_part.p + J.partOff, 9, nblk[j], pcs);
        epnp_block_sums(W.h_part.p + J.partOff + (size_t)9 * nblk[j], 27, nblk[j], abt);
        H[j].abt(J.A, pcs, abt);
    }
    // ---- Reproj
    upload();
    pass(kEpnpPassReproj, 3, 0, -1);
    fetch();
    for (size_t j = 0; j < n; ++j) {
        if (!live[j]) continue;
        BatchPnpEpnpJob& J = W.h_eJobs.p[j];
        double rep3[3], R2[9];
        epnp_block_sums(W.h_part.p + J.partOff, 3, nblk[j], rep3);
        H[j].pick(J.A, rep3, R2, jobs[j]->t);
        rodrigues_inv(R2, jobs[j]->r);
    }
}

int pnp_batch(const char* who, const mcvV2d* img, const mcvV3d* world, const int* offsets, int B, const mcvM33d* K,
              const double* dist, const RansacConfig& cfg, const RansacConfig* cfgp, mcvV3d* tVecs, mcvV3d* rVecs,
              uint8_t* mask, int* counts, int refineKind = -1) {
    BatchStats& stats = batch_stats();
    stats = BatchStats();
    stats.problems = B;
    if (B == 0) return 0;
    const int total = offsets[B];
    std::memset(tVecs, 0, (size_t)B * sizeof(mcvV3d));
    std::memset(rVecs, 0, (size_t)B * sizeof(mcvV3d));
    std::memset(counts, 0, (size_t)B * sizeof(int));
    std::memset(mask, 0, (size_t)total);
    require_device();

    const bool epnp = pnp_cfg_epnp(cfg);
    const int m = epnp ? 5 : 4;
    const bool fixed = (cfg.flags & MCV_FLAG_FIXED_ITERS) != 0;
    const bool refine = !(cfg.flags & MCV_FLAG_NO_REFINE);
    const float thr2 = (float)(cfg.threshold * cfg.threshold);
    int firstFail = -1;
    std::string firstMsg;
    auto failed = [&](int p, const std::string& msg) {
        if (firstFail < 0 || p < firstFail) { firstFail = p; firstMsg = msg; }
    };
    int ok = 0;
    int directPoses = 0;         // poses of the single export's direct solve: their masks never reach the device
    bool maskOnDevice = false;   // W.mask holds the returned mask of every device problem

    BatchLayout L;
    batch_layout(offsets, B, m, cfg.maxIters, batch_cap_pnp(), L);
    std::vector<int> dev;   // device problems, in order
    std::vector<int> idxBuf;
    for (int p = 0; p < B; ++p) {
        const int N = offsets[p + 1] - offsets[p];
        char buf[200];
        if (N < 4) {
            snprintf(buf, sizeof(buf), "need at least 4 correspondences (N=%d)", N);
            failed(p, buf);
        } else if (!camera_ok(K[p])) {
            failed(p, "camera matrix needs finite non-zero fx, fy");
        } else if (N <= m) {
            // npoints == model_points (and N == 4 with a 5-point kind): the single export's direct solve
            ++stats.single;
            const int o = offsets[p];
            idxBuf.assign((size_t)N, 0);
            int c = 0;
            mcvV3d tv{0, 0, 0}, rv{0, 0, 0};
            if (cvSolvePnPRansacCfg(img + o, world + o, N, K[p], dist ? dist + 4 * (size_t)p : nullptr, cfgp, &tv, &rv,
                                    &c, idxBuf.data()) &&
                c > 0) {
                tVecs[p] = tv;
                rVecs[p] = rv;
                counts[p] = c;
                for (int k = 0; k < c; ++k) mask[o + idxBuf[(size_t)k]] = 1;
                ++ok;
                ++directPoses;
            } else {
                const char* e = mcvGetLastError();
                failed(p, e && *e ? e : "the direct solve found no pose");
            }
        } else {
            dev.push_back(p);
        }
    }
    const size_t D = dev.size();
    if (D) {
        BatchPnpWs& W = thread_batch_pnp_ws();
        hipStream_t s = W.stream;
        // ---- points: the raw image and world points in one copy, packed to PnpPoint rows by one launch
        auto t0 = std::chrono::steady_clock::now();
        W.h_raw.ensure((size_t)total * 5);
        W.raw.ensure((size_t)total * 5);
        W.pts.ensure((size_t)total * 8);
        std::memcpy(W.h_raw.p, img, (size_t)total * sizeof(mcvV2d));
        std::memcpy(W.h_raw.p + 2 * (size_t)total, world, (size_t)total * sizeof(mcvV3d));
        W.h_cams.ensure(D * 8);
        W.cams.ensure(D * 8);
        for (size_t d = 0; d < D; ++d) {
            const int p = dev[d];
            double* c = W.h_cams.p + 8 * d;
            c[0] = K[p].M[0]; c[1] = K[p].M[4]; c[2] = K[p].M[2]; c[3] = K[p].M[5];
            for (int k = 0; k < 4; ++k) c[4 + k] = dist ? dist[4 * (size_t)p + k] : 0.0;
        }
        stats.packUs = us_since(t0);
        pnp_copy(W.raw.p, W.h_raw.p, (size_t)total * 5 * sizeof(double), hipMemcpyHostToDevice, s);
        pnp_copy(W.cams.p, W.h_cams.p, D * 8 * sizeof(double), hipMemcpyHostToDevice, s);
        launch_pnp_pack(W.raw.p, W.raw.p + 2 * (size_t)total, total, W.pts.p, s);
        ++stats.launches;
        // ---- OpenCV's sample stream: one cv::RNG((uint64)-1) stream per problem, as each single call draws.
        // PnPRansacCallback has no checkSubset, so the rows depend on N and the sample size alone: one table
        // per distinct N of the call.
        const int* d_table = nullptr;
        std::vector<int64_t> rowOff(D, 0);
        if (cv_sampler(cfg)) {
            t0 = std::chrono::steady_clock::now();
            const size_t rowInts = (size_t)L.iters * m;
            std::map<int, int64_t> byN;
            std::vector<int> rows, all;
            for (size_t d = 0; d < D; ++d) {
                const int N = offsets[dev[d] + 1] - offsets[dev[d]];
                auto it = byN.find(N);
                if (it == byN.end()) {
                    cv_table_build(MCV_MODEL_PNP, cfg, nullptr, N, L.iters, rows);
                    it = byN.emplace(N, (int64_t)byN.size() * L.iters).first;
                    all.insert(all.end(), rows.begin(), rows.begin() + (ptrdiff_t)rowInts);
                }
                rowOff[d] = it->second;
            }
            W.h_table.ensure(all.size());
            W.table.ensure(all.size());
            std::memcpy(W.h_table.p, all.data(), all.size() * sizeof(int));
            stats.tableUs = us_since(t0);
            pnp_copy(W.table.p, W.h_table.p, all.size() * sizeof(int), hipMemcpyHostToDevice, s);
            d_table = W.table.p;
        }
        // ---- hypothesis rounds
        std::vector<mcvReplayState> st(D);
        for (auto& x : st) mcvReplayInit(&x, cfg.maxIters);
        std::vector<size_t> active(D);
        for (size_t d = 0; d < D; ++d) active[d] = d;
        W.desc.ensure(D);
        W.h_desc.ensure(D);
        W.fetch.ensure(D);
        W.h_fetch.ensure(D);
        W.best.ensure(D * sizeof(PnpPose));
        W.h_best.ensure(D * sizeof(PnpPose));
        MCV_HIP(hipMemsetAsync(W.best.p, 0, D * sizeof(PnpPose), s));
        for (int64_t begin = 0; !active.empty(); begin += L.per) {
            // a round holds the hypotheses [begin, begin + per) of every problem still searching; the problems
            // are compacted, so problem j of the round owns the slots [j stride, j stride + count)
            std::vector<size_t> run;
            int stride = 0, maxN = 0;
            for (size_t d : active) {
                const int64_t left = (int64_t)st[d].niters - begin;
                if (st[d].stopped || left <= 0) continue;
                const int p = dev[d];
                BatchPnpDesc& X = W.h_desc.p[run.size()];
                X.d.ptOff = offsets[p];
                X.d.N = offsets[p + 1] - offsets[p];
                X.d.hypBegin = (int)begin;
                X.d.hypCount = (int)std::min<int64_t>(left, L.per);
                X.d.rowOff = rowOff[d];
                X.cam = (int)d;
                X.pad = 0;
                stride = std::max(stride, X.d.hypCount);
                maxN = std::max(maxN, X.d.N);
                run.push_back(d);
            }
            active.swap(run);
            if (active.empty()) break;
            const size_t n = active.size();
            const size_t cols = n * (size_t)stride;
            for (size_t j = 0; j < n; ++j) W.h_desc.p[j].d.slotOff = (int64_t)j * stride;
            W.models.ensure(cols * sizeof(PnpPose));
            W.counts.ensure(cols);
            W.h_counts.ensure(cols);
            if (epnp) W.scratch.ensure(cols * (size_t)kEpnpSplitDoubles);
            pnp_copy(W.desc.p, W.h_desc.p, n * sizeof(BatchPnpDesc), hipMemcpyHostToDevice, s);
            {
                ProfScope pg("batch_pnp_generate", s);
                stats.launches += launch_pnp_batch_generate(W.pts.p, W.desc.p, (int)n, stride, W.cams.p, cfg.seed,
                                                            d_table, epnp, W.models.p, W.counts.p, W.scratch.p, s);
            }
            {
                ProfScope ps("batch_pnp_sweep", s);
                launch_batch_pnp_sweep(W.pts.p, W.desc.p, (int)n, stride, maxN, W.cams.p, W.models.p, W.counts.p, thr2,
                                       s);
            }
            ++stats.launches;
            pnp_copy(W.h_counts.p, W.counts.p, cols * sizeof(int), hipMemcpyDeviceToHost, s);
            pnp_sync(s);
            ++stats.rounds;
            stats.problemRounds += (long long)n;
            size_t nFetch = 0;
            for (size_t j = 0; j < n; ++j) {
                const size_t d = active[j];
                const BatchDesc& X = W.h_desc.p[j].d;
                const int64_t before = st[d].bestIndex;
                mcvReplayChunk(&st[d], W.h_counts.p + X.slotOff, begin, X.hypCount, X.N, m, cfg.confidence,
                               fixed ? 1 : 0);
                if (begin + X.hypCount >= st[d].niters) st[d].stopped = 1;
                if (st[d].bestIndex != before)
                    W.h_fetch.p[nFetch++] = BatchPnpFetch{X.slotOff + (st[d].bestIndex - begin), (int)d, 0};
            }
            if (nFetch) {   // in stream order before the next round's generate reuses the pose buffer
                pnp_copy(W.fetch.p, W.h_fetch.p, nFetch * sizeof(BatchPnpFetch), hipMemcpyHostToDevice, s);
                launch_batch_pnp_fetch(W.fetch.p, (int)nFetch, W.models.p, W.best.p, s);
                ++stats.launches;
                // the next round rewrites h_fetch only after its own synchronisation
            }
        }
        // ---- winners: mask and count, all in one launch
        std::vector<Winner> win;
        int winMaxN = 0;
        W.fin.ensure(D);
        W.h_fin.ensure(D);
        for (size_t d = 0; d < D; ++d) {
            const int p = dev[d];
            if (st[d].bestIndex < 0) {
                failed(p, "RANSAC found no pose with >= 4 inliers");
                continue;
            }
            Winner w{};
            w.d = d;
            w.p = p;
            w.ptOff = offsets[p];
            w.N = offsets[p + 1] - offsets[p];
            w.ok = true;
            W.h_fin.p[win.size()] = BatchPnpFin{w.ptOff, w.N, (int)d, (int)d};
            winMaxN = std::max(winMaxN, w.N);
            win.push_back(w);
        }
        if (!win.empty()) {
            const size_t n = win.size();
            W.cnt.ensure(n);
            W.h_cnt.ensure(n);
            W.mask.ensure((size_t)total);
            W.h_mask.ensure((size_t)total);
            pnp_copy(W.fin.p, W.h_fin.p, n * sizeof(BatchPnpFin), hipMemcpyHostToDevice, s);
            MCV_HIP(hipMemsetAsync(W.cnt.p, 0, n * sizeof(int), s));
            MCV_HIP(hipMemsetAsync(W.mask.p, 0, (size_t)total, s));
            launch_batch_pnp_mask(W.pts.p, W.fin.p, (int)n, winMaxN, W.cams.p, W.best.p, thr2, W.mask.p, W.cnt.p, s);
            ++stats.launches;
            pnp_copy(W.h_best.p, W.best.p, D * sizeof(PnpPose), hipMemcpyDeviceToHost, s);
            pnp_copy(W.h_cnt.p, W.cnt.p, n * sizeof(int), hipMemcpyDeviceToHost, s);
            pnp_copy(W.h_mask.p, W.mask.p, (size_t)total, hipMemcpyDeviceToHost, s);
            pnp_sync(s);
            std::vector<Winner*> jobs;
            for (size_t k = 0; k < n; ++k) {
                Winner& w = win[k];
                w.count = W.h_cnt.p[k];
                if (w.count <= 0) {   // cannot happen for a replay winner (its sweep count was >= m): fail closed
                    failed(w.p, "the winning pose has no inliers");
                    w.ok = false;
                    continue;
                }
                PnpPose pose;
                std::memcpy(&pose, W.h_best.p + w.d * sizeof(PnpPose), sizeof(PnpPose));
                rodrigues_inv(pose.R, w.r);
                for (int k3 = 0; k3 < 3; ++k3) w.t[k3] = pose.t[k3];
                if (refine) jobs.push_back(&w);
            }
            // solvePnPRansac's tail (p_finalize): ITERATIVE refines the RANSAC pose with LM, every other kind
            // runs EPnP on the inliers
            if (pnp_kind(cfg.pnpKind) == 0) batch_pnp_lm(W, jobs, W.h_cams.p, s);
            else batch_pnp_epnp(W, jobs, W.h_cams.p, world, total, failed, s);
            maskOnDevice = true;
            for (const Winner& w : win) {
                if (!w.ok) {   // its device mask slice is not the (zero) one the call returns
                    maskOnDevice = false;
                    continue;
                }
                rVecs[w.p].X = w.r[0]; rVecs[w.p].Y = w.r[1]; rVecs[w.p].Z = w.r[2];
                tVecs[w.p].X = w.t[0]; tVecs[w.p].Y = w.t[1]; tVecs[w.p].Z = w.t[2];
                counts[w.p] = w.count;
                std::memcpy(mask + w.ptOff, W.h_mask.p + w.ptOff, (size_t)w.N);
                ++ok;
            }
        }
    }
    if (refineKind >= 0 && ok > 0) {
        // cvRefinePnPBatch on the returned mask, for every problem with a pose: the packed rows and the mask are
        // read where the rounds left them on the device. Only what never got there is sent now: the points
        // when no problem ran on the device, the mask when a direct solve or a failed inlier solve made the
        // returned one differ from the device's.
        BatchPnpWs& W = thread_batch_pnp_ws();
        hipStream_t s = W.stream;
        if (!D) refine_pack(W, img, world, total, s);
        if (!maskOnDevice || directPoses > 0) {
            W.mask.ensure((size_t)total);
            W.h_mask.ensure((size_t)total);
            std::memcpy(W.h_mask.p, mask, (size_t)total);
            pnp_copy(W.mask.p, W.h_mask.p, (size_t)total, hipMemcpyHostToDevice, s);
        }
        std::vector<uint8_t> run((size_t)B);
        for (int p = 0; p < B; ++p) run[(size_t)p] = counts[p] > 0 ? 1 : 0;
        RefinePlan R;
        refine_plan(offsets, B, K, mask, run.data(), failed, R);
        refine_on_device(W, R, offsets, B, K, dist, refineKind, tVecs, rVecs, nullptr, s);
    }
    if (firstFail >= 0) {
        // a problem that failed returns a zero pose, count and mask slice; the first one is named
        char buf[400];
        snprintf(buf, sizeof(buf), "%s: problem %d: %s", who, firstFail, firstMsg.c_str());
        set_last_error(buf);
    } else {
        clear_last_error();
    }
    return ok;
}

}  // namespace

}  // namespace mcv

using namespace mcv;

// The argument checks cvSolvePnPRansacBatch and cvSolvePnPRansacRefineBatch share; returns the configuration.
static RansacConfig pnp_batch_check(const char* who, const mcvV2d* imgPoints, const mcvV3d* worldPoints,
                                    const int* offsets, int B, const mcvM33d* K, const RansacConfig* cfgp,
                                    mcvV3d* tVecs, mcvV3d* rVecs, uint8_t* mask, int* counts) {
    if (!imgPoints || !worldPoints || !offsets || !K || !tVecs || !rVecs || !mask || !counts)
        fail("%s: null argument (imgPoints, worldPoints, offsets, K, tVecs, rVecs, mask and counts are required)", who);
    if (B < 0) fail("%s: negative B (%d)", who, B);
    if (offsets[0] != 0) fail("%s: offsets[0] must be 0 (is %d)", who, offsets[0]);
    for (int p = 0; p < B; ++p)
        if (offsets[p + 1] < offsets[p])
            fail("%s: offsets decrease at problem %d (%d -> %d)", who, p, offsets[p], offsets[p + 1]);
    const RansacConfig cfg = cfgp ? *cfgp : pnp_config(100, 8.0f, 0.99, 0);
    check_flags(cfg, who);
    if (cfg.method != MCV_METHOD_RANSAC) fail("%s: unsupported method %d (only MCV_METHOD_RANSAC)", who, cfg.method);
    if (cfg.flags & MCV_FLAG_FUSED_ERROR) fail("%s: unsupported flag MCV_FLAG_FUSED_ERROR", who);
    if (cfg.flags & MCV_FLAG_FAST_MINIMAL) fail("%s: unsupported flag MCV_FLAG_FAST_MINIMAL", who);
    if (cfg.deviceCount > 1) fail("%s: unsupported deviceCount %d (one GPU per call)", who, cfg.deviceCount);
    if (!(cfg.confidence > 0 && cfg.confidence < 1)) fail("%s: confidence must be in (0,1)", who);
    for (int p = 0; p < B; ++p)
        if (offsets[p + 1] - offsets[p] > 65535 * kBatchPnpTile)
            fail("%s: problem %d has more than %d correspondences", who, p, 65535 * kBatchPnpTile);
    return cfg;
}

extern "C" MCV_API int cvSolvePnPRansacBatch(const mcvV2d* imgPoints, const mcvV3d* worldPoints, const int* offsets,
                                             int B, const mcvM33d* K, const double* distortionCoeffs,
                                             const RansacConfig* cfgp, mcvV3d* tVecs, mcvV3d* rVecs, uint8_t* mask,
                                             int* counts) {
    MCV_GUARD(-1, {
        const char* who = "cvSolvePnPRansacBatch";
        const RansacConfig cfg = pnp_batch_check(who, imgPoints, worldPoints, offsets, B, K, cfgp, tVecs, rVecs, mask,
                                                 counts);
        return pnp_batch(who, imgPoints, worldPoints, offsets, B, K, distortionCoeffs, cfg, cfgp, tVecs, rVecs, mask,
                         counts);
    })
}

extern "C" MCV_API int cvSolvePnPRansacRefineBatch(const mcvV2d* imgPoints, const mcvV3d* worldPoints,
                                                   const int* offsets, int B, const mcvM33d* K,
                                                   const double* distortionCoeffs, const RansacConfig* cfgp,
                                                   int refineKind, mcvV3d* tVecs, mcvV3d* rVecs, uint8_t* mask,
                                                   int* counts) {
    MCV_GUARD(-1, {
        const char* who = "cvSolvePnPRansacRefineBatch";
        const RansacConfig cfg = pnp_batch_check(who, imgPoints, worldPoints, offsets, B, K, cfgp, tVecs, rVecs, mask,
                                                 counts);
        if (refineKind != 0 && refineKind != 1)
            fail("%s: unsupported refineKind %d (0 = LM, 1 = VVS)", who, refineKind);
        return pnp_batch(who, imgPoints, worldPoints, offsets, B, K, distortionCoeffs, cfg, cfgp, tVecs, rVecs, mask,
                         counts, refineKind);
    })
}

extern "C" MCV_API int cvRefinePnPBatch(const mcvV2d* imgPoints, const mcvV3d* worldPoints, const int* offsets, int B,
                                        const mcvM33d* K, const double* distortionCoeffs, const uint8_t* mask,
                                        int refineKind, mcvV3d* tVecs, mcvV3d* rVecs, uint8_t* refined) {
    MCV_GUARD(-1, {
        const char* who = "cvRefinePnPBatch";
        if (!imgPoints || !worldPoints || !offsets || !K || !tVecs || !rVecs)
            fail("%s: null argument (imgPoints, worldPoints, offsets, K, tVecs and rVecs are required)", who);
        if (B < 0) fail("%s: negative B (%d)", who, B);
        int where = 0;
        const int bad = refine_batch_check_offsets(offsets, B, &where);
        if (bad == 1) fail("%s: offsets[0] must be 0 (is %d)", who, offsets[0]);
        if (bad == 2)
            fail("%s: offsets decrease at problem %d (%d -> %d)", who, where, offsets[where], offsets[where + 1]);
        where = refine_batch_check_sizes(offsets, B, 65535 * kBatchPnpTile);
        if (where >= 0) fail("%s: problem %d has more than %d correspondences", who, where, 65535 * kBatchPnpTile);
        if (refineKind != 0 && refineKind != 1)
            fail("%s: unsupported refineKind %d (0 = LM, 1 = VVS)", who, refineKind);
        BatchStats& stats = batch_stats();
        stats = BatchStats();
        stats.problems = B;
        if (B == 0) return 0;
        int firstFail = -1;
        std::string firstMsg;
        auto failed = [&](int p, const std::string& msg) {
            if (firstFail < 0 || p < firstFail) { firstFail = p; firstMsg = msg; }
        };
        RefinePlan R;
        refine_plan(offsets, B, K, mask, nullptr, failed, R);
        // a call in which no problem can run needs no device, as the single call that refuses its N
        if (!R.jobs.empty()) require_device();
        if (refined) std::memset(refined, 0, (size_t)B);
        int ok = 0;
        if (!R.jobs.empty()) {
            BatchPnpWs& W = thread_batch_pnp_ws();
            hipStream_t s = W.stream;
            const int total = offsets[B];
            refine_pack(W, imgPoints, worldPoints, total, s);
            if (mask) {
                W.mask.ensure((size_t)total);
                W.h_mask.ensure((size_t)total);
                std::memcpy(W.h_mask.p, mask, (size_t)total);
                pnp_copy(W.mask.p, W.h_mask.p, (size_t)total, hipMemcpyHostToDevice, s);
            }
            ok = refine_on_device(W, R, offsets, B, K, distortionCoeffs, refineKind, tVecs, rVecs, refined, s);
        }
        if (firstFail >= 0) {
            // a problem that was not refined keeps its pose; the first one is named
            char buf[400];
            snprintf(buf, sizeof(buf), "%s: problem %d: %s", who, firstFail, firstMsg.c_str());
            set_last_error(buf);
        } else {
            clear_last_error();
        }
        return ok;
    })
}

// The index arithmetic of cvRefinePnPBatch as the export computes it (no device): counts[B] the selected rows
// of every problem, compOff[B + 1] their place in the compact array. Returns the largest count, -1 on a bad
// argument.
extern "C" MCV_API int mcvHostRefinePnPBatchLayout(const int* offsets, int B, const uint8_t* mask, int* counts,
                                                   int* compOff) {
    MCV_GUARD(-1, {
        const char* who = "mcvHostRefinePnPBatchLayout";
        if (!offsets || !counts || !compOff) fail("%s: null argument", who);
        if (B < 0) fail("%s: negative B (%d)", who, B);
        int where = 0;
        const int bad = refine_batch_check_offsets(offsets, B, &where);
        if (bad == 1) fail("%s: offsets[0] must be 0 (is %d)", who, offsets[0]);
        if (bad == 2)
            fail("%s: offsets decrease at problem %d (%d -> %d)", who, where, offsets[where], offsets[where + 1]);
        return refine_batch_layout(offsets, B, mask, counts, compOff);
    })
}

extern "C" MCV_API int mcvTestBatchSweepPnp(const float* pts8, const int* offsets, int B, const double* cam8,
                                            const double* poses12, const int* poseOffsets, float thr2, int* counts) {
    MCV_GUARD(0, {
        if (!pts8 || !offsets || !cam8 || !poses12 || !poseOffsets || !counts || B <= 0)
            fail("mcvTestBatchSweepPnp: null argument or B <= 0");
        if (offsets[0] != 0 || poseOffsets[0] != 0) fail("mcvTestBatchSweepPnp: offsets must start at 0");
        int maxHyp = 0, maxN = 0;
        for (int p = 0; p < B; ++p) {
            if (offsets[p + 1] < offsets[p] || poseOffsets[p + 1] < poseOffsets[p])
                fail("mcvTestBatchSweepPnp: decreasing offsets at problem %d", p);
            maxHyp = std::max(maxHyp, poseOffsets[p + 1] - poseOffsets[p]);
            maxN = std::max(maxN, offsets[p + 1] - offsets[p]);
        }
        const int total = offsets[B], nPoses = poseOffsets[B];
        if (nPoses <= 0 || total <= 0) fail("mcvTestBatchSweepPnp: nothing to sweep");
        if (maxN > 65535 * kBatchPnpTile) fail("mcvTestBatchSweepPnp: too many points in one problem");
        require_device();
        DevBuf<float> p;
        DevBuf<double> mdl, cams;
        DevBuf<int> c;
        DevBuf<BatchPnpDesc> d;
        std::vector<BatchPnpDesc> h((size_t)B);
        for (int k = 0; k < B; ++k) {
            BatchPnpDesc& X = h[(size_t)k];
            X.d.ptOff = offsets[k];
            X.d.N = offsets[k + 1] - offsets[k];
            X.d.hypBegin = 0;
            X.d.hypCount = poseOffsets[k + 1] - poseOffsets[k];
            X.d.slotOff = poseOffsets[k];
            X.d.rowOff = 0;
            X.cam = k;
            X.pad = 0;
        }
        p.ensure((size_t)total * 8);
        mdl.ensure((size_t)nPoses * 12);
        cams.ensure((size_t)B * 8);
        c.ensure((size_t)nPoses);
        d.ensure((size_t)B);
        MCV_HIP(hipMemcpy(p.p, pts8, (size_t)total * 32, hipMemcpyHostToDevice));
        MCV_HIP(hipMemcpy(mdl.p, poses12, (size_t)nPoses * 96, hipMemcpyHostToDevice));
        MCV_HIP(hipMemcpy(cams.p, cam8, (size_t)B * 64, hipMemcpyHostToDevice));
        MCV_HIP(hipMemcpy(d.p, h.data(), (size_t)B * sizeof(BatchPnpDesc), hipMemcpyHostToDevice));
        MCV_HIP(hipMemset(c.p, 0, (size_t)nPoses * 4));
        launch_batch_pnp_sweep(p.p, d.p, B, maxHyp, maxN, cams.p, mdl.p, c.p, thr2, 0);
        MCV_HIP(hipGetLastError());
        MCV_HIP(hipMemcpy(counts, c.p, (size_t)nPoses * 4, hipMemcpyDeviceToHost));
        return 1;
    })
}
