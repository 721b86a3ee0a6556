// ransac_batch_pnp_host.cpp — cvSolvePnPRansacBatch: B independent cvSolvePnPRansacCfg problems in one call
// whose kernel launches, stream synchronisations and copies do not grow with B, and the
// batched refinement behind it (cvRefinePnPBatch, cvSolvePnPRansacRefineBatch: §7k).
//
//   pack:     the raw image and world points in one copy, mcv_pnp_pack over all of them in one launch, one
//             table of cameras (8 doubles per problem)
//   rounds:   batch_host.h's driver over the single call's generate in its batch form (AP3P: one kernel; EPnP:
//             the five split stages) + the batched sweep; a changed best pose is copied out of the round's buffer
//   finalize: every winner masked and counted in one launch, one copy back
//   refine:   kind 0: the winners' LM solvers in lockstep (PnpLmStepper), one batched reduction and one read-back
//             per step, at most 21 steps; other kinds: EPnP on the inliers for all winners at once, the four
//             read-backs of the single call once each, EpnpHostSolve's algebra per job between them
// Every device step is the batch form of the single call's kernel and every host step the single call's own
// function, so each problem returns the single call's bits. Problems with exactly the sample size take the
// single export's direct solve, one by one.
//
// cvRefinePnPBatch / cvSolvePnPRansacRefineBatch: the rows are packed as above, every problem's selected rows
// are gathered into one compact array (2 launches, none without a mask), and the steppers of pnp_lm / pnp_vvs
// run in lockstep over the gathered rows, unmasked. The fused call runs it behind the rounds on the packed rows
// and the mask they left on the device.
//
// One round (B problems, every one on the device and with a winner), counted by BatchStats:
//   AP3P, NO_REFINE   launches 4 (pack, generate, sweep, mask) + 1 fetch = 5, synchronisations 2
//   EPnP kinds        generate is 5 kernels: 9 launches before the refine; + compact, prep and 6 passes = 17
//                     with 4 more synchronisations (6 in all)
//   kind 0            9 + 2 per LM step, one synchronisation per step (at most 21)
// each further round adds the generate, the sweep, a fetch and one synchronisation.
#include "kernels.h"
#include "hyp_pnp.h"
#include "pnp_refine.h"
#include "pnp_refine_batch_index.h"
#include "batch_host.h"

#include <array>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>

namespace mcv {

namespace {

struct BatchPnpWs : DeviceWs {
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
};

bool camera_ok(const mcvM33d& K) {
    const double fx = K.M[0], fy = K.M[4];
    return fx != 0 && fy != 0 && std::isfinite(fx) && std::isfinite(fy);
}

// A problem's row of the camera table: fx, fy, cx, cy, then its four distortion coefficients (dist: 4 per
// problem, or null).
void camera_fill(const mcvM33d* K, const double* dist, int p, double* c) {
    c[0] = K[p].M[0]; c[1] = K[p].M[4]; c[2] = K[p].M[2]; c[3] = K[p].M[5];
    for (int k = 0; k < 4; ++k) c[4 + k] = dist ? dist[4 * (size_t)p + k] : 0.0;
}

struct Winner {     // a device problem with a pose
    size_t d;       // device index
    int p;          // problem
    int ptOff, N;
    int count = 0;
    double r[3] = {0, 0, 0}, t[3] = {0, 0, 0};
    bool ok = true;
};
// The host mask of a call to the device (one copy).
void mask_upload(BatchPnpWs& W, const uint8_t* mask, int total, hipStream_t s) {
    W.mask.ensure((size_t)total);
    W.h_mask.ensure((size_t)total);
    std::memcpy(W.h_mask.p, mask, (size_t)total);
    batch_copy(W.mask.p, W.h_mask.p, (size_t)total, hipMemcpyHostToDevice, s);
}

void winner_store(const Winner& w, mcvV3d* rVecs, mcvV3d* tVecs) {
    rVecs[w.p] = mcvV3d{w.r[0], w.r[1], w.r[2]};
    tVecs[w.p] = mcvV3d{w.t[0], w.t[1], w.t[2]};
}

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
        batch_copy(W.lmJobs.p, W.h_lmJobs.p, n * sizeof(BatchPnpLmJob), hipMemcpyHostToDevice, s);
        stats.launches += launch_pnp_batch_reduce(vvs, d_pts, d_mask, W.lmJobs.p, (int)n, actMaxN, W.lmPart.p,
                                                  W.lmOut.p, s);
        batch_copy(W.h_lmOut.p, W.lmOut.p, n * 28 * sizeof(double), hipMemcpyDeviceToHost, s);
        batch_sync(s);
        ++stats.lmRounds;
        for (size_t k = 0; k < n; ++k) st[who[k]].feed(W.h_lmOut.p + 28 * k);
    }
    for (size_t j = 0; j < jobs.size(); ++j) st[j].result(jobs[j]->r, jobs[j]->t);
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
    batch_copy(W.raw.p, W.h_raw.p, (size_t)total * 5 * sizeof(double), hipMemcpyHostToDevice, s);
    launch_pnp_pack(W.raw.p, W.raw.p + 2 * (size_t)total, total, W.pts.p, s);
    ++stats.launches;
}

// The host half of a refine: every problem's selected rows and place in the compact array, why a problem does
// not run, and the table of those that do (pnp_refine_batch_index.h). run (may be null): the problems asked
// for; a problem asked for that cannot run is noted in fails with the single call's message.
struct RefinePlan {
    std::vector<int> counts, compOff, reason;
    std::vector<RefineBatchJob> jobs;
    int largest = 0;
    bool gathered = false;
};
void refine_plan(const int* offsets, int B, const mcvM33d* K, const uint8_t* h_mask, const uint8_t* run,
                 BatchFailures& fails, RefinePlan& R) {
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
            fails.note(p, buf);
        } else if (R.reason[p] == kRefineBadCamera) {
            fails.note(p, "camera matrix needs finite non-zero fx, fy");
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
        batch_copy(W.eJobs.p, W.h_eJobs.p, (size_t)B * sizeof(BatchPnpEpnpJob), hipMemcpyHostToDevice, s);
        batch_copy(W.tab.p, W.h_tab.p, 2 * ((size_t)B + 1) * sizeof(int), hipMemcpyHostToDevice, s);
        stats.launches += launch_pnp_batch_gather(W.pts.p, W.mask.p, W.eJobs.p, B, W.tab.p, W.tab.p + B + 1, selected,
                                                  W.idx.p, W.ecount.p, W.comp.p, s);
        d_pts = W.comp.p;
    }
    std::vector<double> cams((size_t)nJobs * 8);
    std::vector<Winner> win((size_t)nJobs);
    std::vector<Winner*> jobs((size_t)nJobs);
    for (int j = 0; j < nJobs; ++j) {
        const int p = tab[(size_t)j].prob;
        camera_fill(K, dist, p, cams.data() + 8 * (size_t)j);
        Winner& w = win[(size_t)j];
        w = Winner{(size_t)j, p, tab[(size_t)j].ptOff, tab[(size_t)j].N};
        std::memcpy(w.r, &rVecs[p], sizeof(w.r));   // mcvV3d: three doubles
        std::memcpy(w.t, &tVecs[p], sizeof(w.t));
        jobs[(size_t)j] = &w;
    }
    if (refineKind == 1) batch_pnp_lockstep<PnpVvsStepper>(W, jobs, cams.data(), d_pts, nullptr, true, s);
    else batch_pnp_lockstep<PnpLmStepper>(W, jobs, cams.data(), d_pts, nullptr, false, s);
    for (const Winner& w : win) {
        winner_store(w, rVecs, tVecs);
        if (refined) refined[w.p] = 1;
    }
    return nJobs;
}

// epnp_inliers of every winner at once: compact + prep + the passes with grid y = the job, the single call's
// four read-backs once each. world: the caller's points (a job's first inlier as pw holds it: the double of
// its float coordinates). A job whose inlier count is below 4 fails, as epnp_inliers does.
void batch_pnp_epnp(BatchPnpWs& W, std::vector<Winner*>& jobs, const double* h_cams, const mcvV3d* world, int total,
                    BatchFailures& fails, hipStream_t s) {
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
    auto upload = [&]() { batch_copy(W.eJobs.p, W.h_eJobs.p, n * sizeof(BatchPnpEpnpJob), hipMemcpyHostToDevice, s); };
    auto pass = [&](int mode, int nacc, int region, int prev) {
        stats.launches += launch_pnp_batch_epnp_pass(mode, W.eJobs.p, (int)n, maxNblk, W.ecount.p, W.pw.p, W.us.p, nacc,
                                                     region, prev, W.part.p, s);
    };
    auto fetch = [&]() {
        batch_copy(W.h_part.p, W.part.p, (size_t)partTotal * sizeof(double), hipMemcpyDeviceToHost, s);
        batch_sync(s);
    };
    // ---- {count, SumPw, Pw0}
    upload();
    stats.launches += launch_pnp_batch_epnp_prep(W.pts.p, W.mask.p, W.eJobs.p, (int)n, maxN, W.idx.p, W.ecount.p,
                                                 W.pw.p, W.us.p, s);
    pass(kEpnpPassSumPw, 3, 0, -1);
    pass(kEpnpPassPw0, 6, 1, 0);
    batch_copy(W.h_ecount.p, W.ecount.p, n * sizeof(int), hipMemcpyDeviceToHost, s);
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
            fails.note(jobs[j]->p, buf);
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

// The PnP batch's part of a hypothesis round (batch_host.h's batch_rounds): one pose per hypothesis, one
// confidence for all problems, each descriptor with its camera.
struct RoundsPnp {
    BatchPnpWs& W;
    bool epnp;
    uint64_t seed;
    const int* d_table;
    float thr2;
    double conf;
    static constexpr int slots = 1;
    BatchDesc& desc(size_t j, int d) {   // entry j with its camera: cams + 8 d
        W.h_desc.p[j].cam = d;
        W.h_desc.p[j].pad = 0;
        return W.h_desc.p[j].d;
    }
    void launch(const std::vector<int>&, BatchRound R, hipStream_t s) {
        BatchStats& stats = batch_stats();
        const size_t n = (size_t)R.n, cols = n * (size_t)R.stride;
        int maxN = 0;
        for (size_t j = 0; j < n; ++j) maxN = std::max(maxN, W.h_desc.p[j].d.N);
        W.models.ensure(cols * sizeof(PnpPose));
        W.counts.ensure(cols);
        W.h_counts.ensure(cols);
        if (epnp) W.scratch.ensure(cols * (size_t)kEpnpSplitDoubles);
        {
            ProfScope pg("batch_pnp_generate", s);
            stats.launches += launch_pnp_batch_generate(W.pts.p, W.desc.p, R.n, R.stride, W.cams.p, seed, d_table, epnp,
                                                        W.models.p, W.counts.p, W.scratch.p, s);
        }
        {
            ProfScope ps("batch_pnp_sweep", s);
            launch_batch_pnp_sweep(W.pts.p, W.desc.p, R.n, R.stride, maxN, W.cams.p, W.models.p, W.counts.p, thr2, s);
        }
        ++stats.launches;
    }
    double confidence(int) const { return conf; }
    void best_changed(const std::vector<BestChange>& ch, hipStream_t s) {
        for (size_t k = 0; k < ch.size(); ++k)
            W.h_fetch.p[k] = BatchPnpFetch{W.h_desc.p[ch[k].j].d.slotOff + ch[k].slot, ch[k].d, 0};
        // in stream order before the next round's generate reuses the pose buffer; the next round rewrites
        // h_fetch only after its own synchronisation
        batch_copy(W.fetch.p, W.h_fetch.p, ch.size() * sizeof(BatchPnpFetch), hipMemcpyHostToDevice, s);
        launch_batch_pnp_fetch(W.fetch.p, (int)ch.size(), W.models.p, W.best.p, s);
        ++batch_stats().launches;
    }
};

int pnp_batch(const char* who, const mcvV2d* img, const mcvV3d* world, const int* offsets, int B, const mcvM33d* K,
              const double* dist, const RansacConfig& cfg, const RansacConfig* cfgp, mcvV3d* tVecs, mcvV3d* rVecs,
              uint8_t* mask, int* counts, int refineKind = -1) {
    BatchStats& stats = batch_stats_begin(B);
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
    BatchFailures fails;
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
            fails.note(p, buf);
        } else if (!camera_ok(K[p])) {
            fails.note(p, "camera matrix needs finite non-zero fx, fy");
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
                fails.note(p, e && *e ? e : "the direct solve found no pose");
            }
        } else {
            dev.push_back(p);
        }
    }
    const size_t D = dev.size();
    if (D) {
        BatchPnpWs& W = thread_device_ws<BatchPnpWs>();
        hipStream_t s = W.stream();
        // ---- points: refine_pack; the table of cameras in one more copy
        refine_pack(W, img, world, total, s);
        const auto t0 = std::chrono::steady_clock::now();
        W.h_cams.ensure(D * 8);
        W.cams.ensure(D * 8);
        std::vector<BatchProblem> prob(D);
        for (size_t d = 0; d < D; ++d) {
            const int p = dev[d];
            camera_fill(K, dist, p, W.h_cams.p + 8 * d);
            prob[d] = BatchProblem{offsets[p], offsets[p + 1] - offsets[p], 0};
        }
        stats.packUs += us_since(t0);
        batch_copy(W.cams.p, W.h_cams.p, D * 8 * sizeof(double), hipMemcpyHostToDevice, s);
        // ---- OpenCV's sample stream (PnPRansacCallback has no checkSubset: one table per distinct N)
        const int* d_table = cv_tables_by_n(MCV_MODEL_PNP, cfg, prob, L.iters, m, W.h_table, W.table, s);
        // ---- hypothesis rounds
        W.fetch.ensure(D);
        W.h_fetch.ensure(D);
        W.best.ensure(D * sizeof(PnpPose));
        W.h_best.ensure(D * sizeof(PnpPose));
        MCV_HIP(hipMemsetAsync(W.best.p, 0, D * sizeof(PnpPose), s));
        RoundsPnp F{W, epnp, cfg.seed, d_table, thr2, cfg.confidence};
        std::vector<mcvReplayState> st;
        batch_rounds(F, prob, st, cfg.maxIters, L.per, L.per, m, fixed, s);
        // ---- winners: mask and count, all in one launch
        std::vector<Winner> win;
        int winMaxN = 0;
        W.fin.ensure(D);
        W.h_fin.ensure(D);
        for (size_t d = 0; d < D; ++d) {
            const int p = dev[d];
            if (st[d].bestIndex < 0) {
                fails.note(p, "RANSAC found no pose with >= 4 inliers");
                continue;
            }
            const Winner w{d, p, offsets[p], offsets[p + 1] - offsets[p]};
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
            batch_copy(W.fin.p, W.h_fin.p, n * sizeof(BatchPnpFin), hipMemcpyHostToDevice, s);
            MCV_HIP(hipMemsetAsync(W.cnt.p, 0, n * sizeof(int), s));
            MCV_HIP(hipMemsetAsync(W.mask.p, 0, (size_t)total, s));
            launch_batch_pnp_mask(W.pts.p, W.fin.p, (int)n, winMaxN, W.cams.p, W.best.p, thr2, W.mask.p, W.cnt.p, s);
            ++stats.launches;
            batch_copy(W.h_best.p, W.best.p, D * sizeof(PnpPose), hipMemcpyDeviceToHost, s);
            batch_copy(W.h_cnt.p, W.cnt.p, n * sizeof(int), hipMemcpyDeviceToHost, s);
            batch_copy(W.h_mask.p, W.mask.p, (size_t)total, hipMemcpyDeviceToHost, s);
            batch_sync(s);
            std::vector<Winner*> jobs;
            for (size_t k = 0; k < n; ++k) {
                Winner& w = win[k];
                w.count = W.h_cnt.p[k];
                if (w.count <= 0) {   // cannot happen for a replay winner (its sweep count was >= m): fail closed
                    fails.note(w.p, "the winning pose has no inliers");
                    w.ok = false;
                    continue;
                }
                PnpPose pose;
                std::memcpy(&pose, W.h_best.p + w.d * sizeof(PnpPose), sizeof(PnpPose));
                rodrigues_inv(pose.R, w.r);
                for (int k3 = 0; k3 < 3; ++k3) w.t[k3] = pose.t[k3];
                if (refine) jobs.push_back(&w);
            }
            // solvePnPRansac's tail (p_finalize): ITERATIVE refines the RANSAC pose with LM, masked in place over
            // every winner's rows; every other kind runs EPnP on the inliers
            if (pnp_kind(cfg.pnpKind) == 0)
                batch_pnp_lockstep<PnpLmStepper>(W, jobs, W.h_cams.p, W.pts.p, W.mask.p, false, s);
            else batch_pnp_epnp(W, jobs, W.h_cams.p, world, total, fails, s);
            maskOnDevice = true;
            for (const Winner& w : win) {
                if (!w.ok) {   // its device mask slice is not the (zero) one the call returns
                    maskOnDevice = false;
                    continue;
                }
                winner_store(w, rVecs, tVecs);
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
        BatchPnpWs& W = thread_device_ws<BatchPnpWs>();
        hipStream_t s = W.stream();
        if (!D) refine_pack(W, img, world, total, s);
        if (!maskOnDevice || directPoses > 0) mask_upload(W, mask, total, s);
        std::vector<uint8_t> run((size_t)B);
        for (int p = 0; p < B; ++p) run[(size_t)p] = counts[p] > 0 ? 1 : 0;
        RefinePlan R;
        refine_plan(offsets, B, K, mask, run.data(), fails, R);
        refine_on_device(W, R, offsets, B, K, dist, refineKind, tVecs, rVecs, nullptr, s);
    }
    fails.report(who);   // a problem that failed returns a zero pose, count and mask slice; the first one is named
    return ok;
}

}  // namespace

}  // namespace mcv

using namespace mcv;

// The kernels' grids take at most 65535 tiles of a problem's rows.
static void pnp_check_sizes(const char* who, const int* offsets, int B) {
    const int where = refine_batch_check_sizes(offsets, B, 65535 * kBatchPnpTile);
    if (where >= 0) fail("%s: problem %d has more than %d correspondences", who, where, 65535 * kBatchPnpTile);
}

// The argument checks cvSolvePnPRansacBatch and cvSolvePnPRansacRefineBatch share; returns the configuration.
static RansacConfig pnp_batch_check(const char* who, const mcvV2d* imgPoints, const mcvV3d* worldPoints,
                                    const int* offsets, int B, const mcvM33d* K, const RansacConfig* cfgp,
                                    mcvV3d* tVecs, mcvV3d* rVecs, uint8_t* mask, int* counts) {
    if (!imgPoints || !worldPoints || !offsets || !K || !tVecs || !rVecs || !mask || !counts)
        fail("%s: null argument (imgPoints, worldPoints, offsets, K, tVecs, rVecs, mask and counts are required)", who);
    check_batch_offsets(who, offsets, B);
    const RansacConfig cfg = cfgp ? *cfgp : pnp_config(100, 8.0f, 0.99, 0);
    check_batch_config(who, cfg);
    pnp_check_sizes(who, offsets, B);
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
        check_batch_offsets(who, offsets, B);
        pnp_check_sizes(who, offsets, B);
        if (refineKind != 0 && refineKind != 1)
            fail("%s: unsupported refineKind %d (0 = LM, 1 = VVS)", who, refineKind);
        batch_stats_begin(B);
        if (B == 0) return 0;
        BatchFailures fails;
        RefinePlan R;
        refine_plan(offsets, B, K, mask, nullptr, fails, R);
        // a call in which no problem can run needs no device, as the single call that refuses its N
        if (!R.jobs.empty()) require_device();
        if (refined) std::memset(refined, 0, (size_t)B);
        int ok = 0;
        if (!R.jobs.empty()) {
            BatchPnpWs& W = thread_device_ws<BatchPnpWs>();
            hipStream_t s = W.stream();
            const int total = offsets[B];
            refine_pack(W, imgPoints, worldPoints, total, s);
            if (mask) mask_upload(W, mask, total, s);
            ok = refine_on_device(W, R, offsets, B, K, distortionCoeffs, refineKind, tVecs, rVecs, refined, s);
        }
        fails.report(who);   // a problem that was not refined keeps its pose; the first one is named
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
        check_batch_offsets(who, offsets, B);
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
