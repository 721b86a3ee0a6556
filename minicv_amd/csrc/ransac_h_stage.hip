// ransac_h_stage.hip — the staged homography sweep on gfx950: the certified sweep run in stages that
// prune themselves (launch_h_verify_staged), for callers that consume only the best key. Here: the
// control block's init, the candidate's exact count and the cell table (mcv_h_stage_count), the stage
// planner, the survivor compaction, the per-cell bound (h_cell_bound.h: mcv_h_cell_bound, the box pass over
// every slot; mcv_h_cell_rel, the second pass with the candidate-relative test and the per-slot `left`;
// mcv_h_cell_prefix, its prefix table; mcv_h_cell_pre_build, the record list of the non-empty cells with the floats
// of the box test's fp32 prefilter, h_cell_pre.h) and the host twins. The stages themselves are the sweeps of
// ransac_h_sweep.hip / ransac_h_mfma.hip.
#include <algorithm>
#include <vector>
#include "mcv_common.h"
#include "hyp_homography.h"
#include "h_cert.h"
#include "h_cell_bound.h"
#include "h_cell_pre.h"

namespace mcv {

// ------------------------------------------------------------------------------------------
// Staged sweep: the small kernels between the stages (launch_h_verify_staged).
// ------------------------------------------------------------------------------------------
// cells: the cell slots of the per-cell bound (0: the bound is off and stage 1 takes every slot; else the
// bound kernel counts the slots it keeps into ctl[kCtlAlive + 1], from 0).
// swept0: the slots stage 0 sweeps (hypCount, or the leading subset).
__global__ void mcv_h_stage_init(int* __restrict__ ctl, int pa, int hypCount, int cells, int swept0) {
    const int i = threadIdx.x;
    if (i >= kHStageCtlInts) return;
    int v = 0;
    if (i == kCtlBound + 1) v = pa;
    if (i == kCtlAlive) v = swept0;
    if (i == kCtlAlive + 1 && cells == 0) v = hypCount;
    if (i == kCtlCells) v = cells;
    ctl[i] = v;
}

// Empty cell table: min slots at INT_MAX, max slots at INT_MIN (ordered-integer encoding), size 0.
__global__ void mcv_h_cell_init(int* __restrict__ cells, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int f = i % kHCellInts;
    cells[i] = f == kHCellInts - 1 ? 0 : ((f & 1) ? INT32_MIN : INT32_MAX);
}

// The cell table of the per-cell bound (h_cell_bound.h), filled by mcv_h_stage_count.
struct HCellArgs {
    int* cells;          // kHCellInts ints per cell, set up by mcv_h_cell_init (nullptr: no table)
    const double* bb;    // the point set's extents (launch_abs_bound4)
    int G, Gs;
    int lds;             // 1: each block gathers a private table in LDS (dynamic shared memory) and flushes it
    int* cellOut;        // test hook: every point's cell (nullptr in the sweep)
};

__device__ __forceinline__ void h_cell_add(int* t, const float4& q) {
    const int ex = h_cell_enc(q.x), ey = h_cell_enc(q.y), emx = h_cell_enc(q.z), emy = h_cell_enc(q.w);
    atomicMin(t + 0, ex);
    atomicMax(t + 1, ex);
    atomicMin(t + 2, ey);
    atomicMax(t + 3, ey);
    atomicMin(t + 4, emx);
    atomicMax(t + 5, emx);
    atomicMin(t + 6, emy);
    atomicMax(t + 7, emy);
    atomicAdd(t + 8, 1);
}

// The candidate (best partial count of stage 0) counted over all N correspondences with the exact
// op-by-op error: ctl[kCtlB] (zeroed by mcv_h_stage_init). No candidate (key 0): B stays 0.
// With a cell table: every correspondence also goes to its cell (the candidate's inliers to the 2-D
// grid, the rest to the 4-D grid): the cell's min / max of x, y, x', y' and its size, all
// order-independent, so the table is deterministic.
__global__ __launch_bounds__(1024) void mcv_h_stage_count(const float4* __restrict__ pts, int N,
                                                          const HModelF* __restrict__ models, int64_t hypBegin,
                                                          float thr2, int* __restrict__ ctl, HCellArgs ca) {
    extern __shared__ int tab[];
    const uint64_t key = *(const uint64_t*)(ctl + kCtlKey);
    if (key == 0) return;
    const int64_t hyp = (int64_t)(0xFFFFFFFFull - (key & 0xFFFFFFFFull));
    const HModelF m = models[hyp - hypBegin];
    const int nt = ca.cells ? h_cell_count(ca.G, ca.Gs) * kHCellInts : 0;
    double b4[4] = {0, 0, 0, 0};
    if (ca.cells) {
#pragma unroll
        for (int j = 0; j < 4; ++j) b4[j] = ca.bb[j];
    }
    if (ca.lds) {
        for (int i = threadIdx.x; i < nt; i += blockDim.x) {
            const int f = i % kHCellInts;
            tab[i] = f == kHCellInts - 1 ? 0 : ((f & 1) ? INT32_MIN : INT32_MAX);
        }
        __syncthreads();
    }
    const int stride = gridDim.x * blockDim.x;
    for (int base = blockIdx.x * blockDim.x; base < N; base += stride) {   // block-uniform trip count
        const int i = base + threadIdx.x;
        bool in = false;
        if (i < N) {
            const float4 q = pts[i];
            in = h_error(m.h, q.x, q.y, q.z, q.w) <= thr2;
            if (ca.cells) {
                const int c = h_cell_index(q.x, q.y, q.z, q.w, in, b4, ca.G, ca.Gs);   // always in [0, cells)
                if (ca.cellOut) ca.cellOut[i] = c;
                h_cell_add((ca.lds ? tab : ca.cells) + c * kHCellInts, q);
            }
        }
        const uint64_t b = __ballot(in);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(ctl + kCtlB, (int)__popcll(b));
    }
    if (ca.lds) {
        __syncthreads();
        for (int i = threadIdx.x; i < nt; i += blockDim.x) {
            const int f = i % kHCellInts;
            if (tab[i - f + kHCellInts - 1] == 0) continue;   // the block saw no point of this cell
            if (f == kHCellInts - 1) atomicAdd(ca.cells + i, tab[i]);
            else if (f & 1) atomicMax(ca.cells + i, tab[i]);
            else atomicMin(ca.cells + i, tab[i]);
        }
    }
}

// What the planner gets beside B, for the kernel and its host twin alike: the trip, the stages behind the first
// pruning boundary, the slack, the late-boundary rule and stage 0's range in pairs: ~N / kHStagePrefixDiv points
// (N / kHCellPrefixDiv with the per-cell bound: stage 0 is then the one full-width stage left), a whole number of
// trips (at least one where N has one).
struct HStagePlanArgs {
    int trip, later, slackPts, latest256, pa;
};
static HStagePlanArgs h_stage_plan_args(int N, bool cellBound) {
    const int trip = 64 * kCertNP, nFull = N / 2 / trip * trip;
    int pa = (N / (cellBound ? kHCellPrefixDiv : kHStagePrefixDiv) / 2 + trip / 2) / trip * trip;
    if (pa < trip) pa = trip;
    if (pa > nFull) pa = nFull;
    return HStagePlanArgs{trip, kHStageLater, N / kHStageSlackDiv, kHStageLatest256, pa};
}

HStagePlan h_stage_plan_host(int N, bool candidate, bool failure, int B, bool cellBound, bool half, bool subset,
                             int* pa) {
    const HStagePlanArgs a = h_stage_plan_args(N, cellBound);
    if (pa) *pa = a.pa;
    return h_stage_plan(N, a.trip, a.later, a.slackPts, a.latest256, cellBound && subset, cellBound && half,
                        candidate, failure, B, a.pa);
}

// One thread: the stage boundaries from B. The first boundary is the first point count at which a
// slot can fall below the bound (N - B) plus the slack, rounded up to a trip; the later stages split
// the rest evenly. Pruning switches itself off (stage 1 runs every slot to the end) without a
// candidate, with a sampler failure in the chunk (the host then reads every count) and when the first
// boundary lies beyond latest/256 of the pairs.
// subset: stage 0 swept only a leading subset of the slots, into a scratch buffer. The candidate's key is the
// subset's; the chunk's first sampler failure is the earlier of the subset's and the one a pass over every slot's
// status left in ctl[kCtlFailAll]; and stage 1 starts at point 0 (boundary 1 is reset), since the counts buffer
// holds no stage-0 partials.
// half: the half boundary in the middle of stage 1's range (with the per-cell bound's second pass). The
// arithmetic is h_stage_plan (kernels.h), shared with the host twin above.
__global__ void mcv_h_stage_plan(int* __restrict__ ctl, int N, int trip, int later, int slackPts, int latest256,
                                 int subset, int half) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint64_t key = *(const uint64_t*)(ctl + kCtlKey);
    int64_t fail = *(const int64_t*)(ctl + kCtlKey + 2);
    if (subset) {
        const int64_t all = *(const int64_t*)(ctl + kCtlFailAll);
        fail = all < fail ? all : fail;
        *(int64_t*)(ctl + kCtlKey + 2) = fail;
    }
    const HStagePlan pl = h_stage_plan(N, trip, later, slackPts, latest256, subset != 0, half != 0, key != 0,
                                       fail != INT64_MAX, ctl[kCtlB], ctl[kCtlBound + 1]);
    ctl[kCtlReason] = pl.reason;
    ctl[kCtlStages] = pl.stages;
#pragma unroll
    for (int i = 1; i <= kHStageMax; ++i)
        if (i <= pl.stages) ctl[kCtlBound + i] = pl.bound[i];
}

// Who goes on past a boundary: a slot with a count (a status, count < 0, never enters a list) that can still
// reach B. Inclusive, so ties survive.
__device__ __forceinline__ bool h_stage_keeps(int count, int left, int B) { return count >= 0 && count + left >= B; }

// `left` of a slot at a boundary: its own figure where the per-cell bound's second pass wrote one (row: the
// boundary's row of slotLeft), else the points not yet processed at the boundary (given in pairs).
__device__ __forceinline__ int h_stage_left(const int* __restrict__ row, int slot, int N, int boundPairs) {
    if (row) return row[slot];
    const int done2 = 2 * boundPairs;
    return N - (done2 < N ? done2 : N);
}

// Appends the threads with `keep` to a survivor list, any order: a ballot per wave and one atomic per block.
// The waves' ballot counts go to LDS (sh: WAVES + 1 ints of the caller's, one set per push of a kernel), one
// returning atomic per block goes to the list's counter, and a lane writes at the block's base + its wave's
// offset + its rank in the ballot. The counter serialises the pushes (a returning atomic on one address
// costs about 12.5 ns when the waves arrive together), so a block of WAVES waves takes 1 / WAVES of
// the time. Every thread of the block must call it (two barriers); a block that keeps nothing takes no atomic.
template <int WAVES>
__device__ __forceinline__ void h_list_push_block(bool keep, int slot, int* total, int* __restrict__ dst, int* sh) {
    const uint64_t b = __ballot(keep);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sh[wave] = (int)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const int c = sh[w];
            sh[w] = sum;
            sum += c;
        }
        sh[WAVES] = sum ? atomicAdd(total, sum) : 0;
    }
    __syncthreads();
    if (keep) dst[sh[WAVES] + sh[wave] + (int)__popcll(b & ((1ull << lane) - 1))] = slot;
}

// Survivors entering `stage` (>= 2): the slots of the previous stage (src; nullptr: all of them)
// whose count can still reach B, count + left >= B. Inclusive, so ties survive; a status
// (count < 0: no model, no sample, the exact-recount mark) never enters a list. Any order: ballot
// and one atomic per block of 16 waves. left: without the per-cell bound (slotLeft == nullptr) the points not yet
// processed, N - processed; with it the slot's own figure, the unprocessed points of the cells the bound
// did not certify for the slot's model (slotLeft[(stage - 2) * hypCount + slot], written by mcv_h_cell_rel,
// or by mcv_h_cell_bound for the slots it keeps out of the second pass).
static constexpr int kHCompactThreads = 1024;
__global__ __launch_bounds__(kHCompactThreads) void mcv_h_stage_compact(const int* __restrict__ counts, int hypCount,
                                                                        int N, int* __restrict__ ctl, int stage,
                                                                        const int* __restrict__ src,
                                                                        int* __restrict__ dst,
                                                                        const int* __restrict__ slotLeft) {
    __shared__ int push[kHCompactThreads / 64 + 1];
    if (ctl[kCtlReason] != 0) return;
    const int n = src ? ctl[kCtlAlive + stage - 1] : hypCount;
    if ((int)(blockIdx.x * kHCompactThreads) >= n) return;   // block-uniform, as the return above
    const int i = blockIdx.x * kHCompactThreads + threadIdx.x;
    const int* row = slotLeft ? slotLeft + (size_t)(stage - 2) * hypCount : nullptr;
    bool keep = false;
    int slot = 0;
    if (i < n) {
        slot = src ? src[i] : i;
        keep = h_stage_keeps(counts[slot], h_stage_left(row, slot, N, ctl[kCtlBound + stage]), ctl[kCtlB]);
    }
    h_list_push_block<kHCompactThreads / 64>(keep, slot, ctl + kCtlAlive + stage, dst, push);
}

// d_src: the previous stage's list (its length in ctl[kCtlAlive + stage - 1]; nullptr: every slot below hypCount);
// d_left: the per-slot `left` rows (nullptr: the points not yet processed). The grid covers every slot.
void launch_h_stage_compact(const int* d_counts, int hypCount, int N, int* d_ctl, int stage, const int* d_src,
                            int* d_dst, const int* d_left, hipStream_t s) {
    hipLaunchKernelGGL(mcv_h_stage_compact, dim3((hypCount + kHCompactThreads - 1) / kHCompactThreads),
                       dim3(kHCompactThreads), 0, s, d_counts, hypCount, N, d_ctl, stage, d_src, d_dst, d_left);
}

// The second pass's buffers as the box pass sees them (pre == nullptr: no second pass, the test hook).
struct HCellPre {
    int* pre;        // the list of the slots the second pass can still drop; its length goes to ctl[kCtlPre]
    int* slotLeft;   // nLater x hypCount ints
    int relBase;     // first cell of the candidate's inliers (G^4)
    int nLater, N;
};

// The record list of the non-empty cells (h_cell_pre.h: kHCellRec*), once per call: one block, the cells in
// table order (ballot + a scan over the block's waves), so the list is deterministic.
__global__ __launch_bounds__(1024) void mcv_h_cell_pre_build(const int* __restrict__ cells, int nCells, double kappa,
                                                             int* __restrict__ rec) {
    __shared__ int wsum[16];
    __shared__ int base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int c0 = 0; c0 < nCells; c0 += 1024) {   // block-uniform trip count
        const int c = c0 + threadIdx.x;
        const int size = c < nCells ? cells[c * kHCellInts + kHCellInts - 1] : 0;
        const uint64_t b = __ballot(size > 0);
        if (lane == 0) wsum[wave] = (int)__popcll(b);
        __syncthreads();
        if (size > 0) {
            int at = base + (int)__popcll(b & ((1ull << lane) - 1));
            for (int w = 0; w < wave; ++w) at += wsum[w];
            int* r = rec + kHCellRecHead + at * kHCellRecInts;   // at <= c < nCells
            float box[8], q[kHCellPreFloats];
#pragma unroll
            for (int j = 0; j < 8; ++j) box[j] = h_cell_dec(cells[c * kHCellInts + j]);
            h_cell_pre_box(box, kappa, q);
#pragma unroll
            for (int j = 0; j < kHCellPreFloats; ++j) r[j] = __float_as_int(q[j]);
            r[kHCellPreFloats] = size;
            r[kHCellPreFloats + 1] = c;
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int w = 0; w < 16; ++w) base += wsum[w];
        __syncthreads();
    }
    if (threadIdx.x == 0) rec[0] = base;
}

// The box test of one non-empty cell (e: its table entry; r: its record; on: the prefilter's switch; all
// wave-uniform) for the lanes with a model (active; the verdict of the others is not used): the fp32 prefilter, and
// the fp64 test for the lanes it leaves undecided, skipped when the wave has none. undecided: the wave's count of
// such lanes (wave-uniform).
__device__ __forceinline__ bool h_cell_box_test(const float* h, const HCellModel& cm, const HCellPreModel& pm,
                                                const int* e, const int* r, int on, bool active,
                                                int& undecided) {
    int v = kHCellPreUndecided;
    if (on) {
        float qq[kHCellPreFloats];
#pragma unroll
        for (int j = 0; j < kHCellPreFloats; ++j) qq[j] = __int_as_float(r[j]);
        v = h_cell_pre(h, pm, qq);
    }
    bool cert = v == kHCellPreCert;
    // a lane without a model (a status, the tail of the grid) holds whatever its slot's model bytes are: it never
    // sends the wave into the fp64 body and is not counted
    const bool und = active && v == kHCellPreUndecided;
    const uint64_t open = __ballot(und);
    if (open) {
        undecided += (int)__popcll(open);
        if (und) {
            float box[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) box[j] = h_cell_dec(e[j]);
            cert = h_cell_certified(h, cm, box);
        }
    }
    return cert;
}

// One wave's figures into the counters (stats == nullptr, the sweep unless mcvTestHCellPre asked: nothing): tested
// cells x its lanes with a model, and the undecided of them.
__device__ __forceinline__ void h_cell_pre_stats(unsigned long long* stats, int tested, bool active, int undecided) {
    if (!stats) return;
    const uint64_t lanes = __ballot(active);
    if ((threadIdx.x & 63) != 0) return;
    atomicAdd(stats, (unsigned long long)tested * (unsigned long long)__popcll(lanes));
    if (undecided) atomicAdd(stats + 1, (unsigned long long)undecided);
}

// The per-cell bound (h_cell_bound.h), lane = slot: UB = the sizes of the cells the model does not certify
// as all-outlier, an upper bound of the slot's full count. Slots with a model and UB >= B (inclusive: ties
// survive) enter the survivor list of stage 1 as mcv_h_stage_compact writes its lists (ballot, one
// atomic per block, any order); their number goes to ctl[kCtlAlive + 1]. A status (count < 0: no model, no
// sample, stage 0's exact-recount mark) never enters the list. Where pruning is off on the device
// (ctl[kCtlReason] != 0) every slot with a model is kept. The cells are wave-uniform (scalar loads); all
// stores are per lane. ubOut / bitsOut (test hook): every slot's UB and its certified-cell bitmap
// (bitWords zeroed words per slot).
// With the second pass behind it (mcv_h_cell_rel, hp.pre != nullptr) a kept slot goes one of two ways. The
// relative test certifies cells of the candidate's inliers only, so it can take a slot below B only when the
// uncertified cells of the other points alone hold fewer than B: those slots go to hp.pre for the second
// pass. The others stay whatever the relative test finds; they go straight to dst, and their `left` is the
// compaction's old figure, the points not yet processed (an upper bound of any slot's `left`). Where
// pruning is off on the device the second pass does nothing and every slot with a model goes to dst.
__global__ __launch_bounds__(256) void mcv_h_cell_bound(const HModelF* __restrict__ models,
                                                        const int* __restrict__ counts, int hypCount, float thr2,
                                                        double kappa, const double* __restrict__ bb,
                                                        const int* __restrict__ cells, int nCells, int* ctl,
                                                        int* __restrict__ dst, HCellPre hp,
                                                        int* __restrict__ ubOut, uint32_t* __restrict__ bitsOut,
                                                        int bitWords, HCellPreBufs pa) {
    __shared__ int push[2][256 / 64 + 1];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool have = i < hypCount && counts[i] >= 0;
    bool keep = have, second = false;
    if (ctl[kCtlReason] == 0 && __ballot(have) != 0) {   // per wave: the block-level pushes stay outside
        const HModelF m = models[i < hypCount ? i : hypCount - 1];
        double b4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) b4[j] = bb[j];
        const HCellModel cm = h_cell_model(m.h, b4, thr2, kappa, kCertT, kCertSlop);
        const HCellPreModel pm = h_cell_pre_model(cm, b4);
        int ub = 0, ubRel = 0;   // ubRel: the part of ub in the cells of the candidate's inliers
        const int tested = pa.rec[0];   // the non-empty cells
        int undecided = 0;              // wave-uniform
        for (int k = 0; k < tested; ++k) {
            const int* r = pa.rec + kHCellRecHead + k * kHCellRecInts;
            const int size = r[kHCellPreFloats], c = r[kHCellPreFloats + 1];
            const bool cert = h_cell_box_test(m.h, cm, pm, cells + c * kHCellInts, r, pa.on, have, undecided);
            ub += cert ? 0 : size;
            if (hp.pre && c >= hp.relBase) ubRel += cert ? 0 : size;
            if (bitsOut && cert && i < hypCount) bitsOut[(size_t)i * bitWords + (c >> 5)] |= 1u << (c & 31);
        }
        if (ubOut && i < hypCount) ubOut[i] = ub;
        h_cell_pre_stats(pa.stats, tested, have, undecided);
        const int B = ctl[kCtlB];
        keep = have && ub >= B;
        if (hp.pre) {
            second = keep && ub - ubRel < B;
            keep = keep && !second;
            if (keep) {
#pragma unroll
                for (int j = 0; j < kHCellLater; ++j) {
                    if (j >= hp.nLater) continue;
                    const int d2 = 2 * ctl[kCtlBound + 2 + j];
                    hp.slotLeft[(size_t)j * hypCount + i] = hp.N - (d2 < hp.N ? d2 : hp.N);
                }
            }
        }
    }
    // `second` is false in a wave that skipped the bound (pruning off, or no lane with a model)
    if (hp.pre) h_list_push_block<256 / 64>(second, i, ctl + kCtlPre, hp.pre, push[0]);
    h_list_push_block<256 / 64>(keep, i, ctl + kCtlAlive + 1, dst, push[1]);
}

// The prefix table of the per-slot `left` figures: pref[j * nCells + c] = the points of cell c with index
// below min(2 * boundary, N) for the boundary that ends stage 1 + j (j < nLater), the convention of
// mcv_h_stage_compact. Zeroed before the launch; each block gathers a histogram in LDS (nLater * nCells ints)
// and adds its non-zero entries. Integer adds: any order gives the same table. Does nothing where pruning is
// off on the device (without a candidate the cell ids were never written).
__global__ __launch_bounds__(1024) void mcv_h_cell_prefix(const int* __restrict__ cellId, int N,
                                                          const int* __restrict__ ctl, int nLater, int nCells,
                                                          int* __restrict__ pref) {
    extern __shared__ int hist[];
    if (ctl[kCtlReason] != 0) return;
    const int nt = nLater * nCells;
    for (int i = threadIdx.x; i < nt; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    int lim[kHCellLater];
#pragma unroll
    for (int j = 0; j < kHCellLater; ++j) {
        const int d2 = j < nLater ? 2 * ctl[kCtlBound + 2 + j] : 0;
        lim[j] = d2 < N ? d2 : N;
    }
    const int stride = gridDim.x * blockDim.x;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride) {
        const int c = cellId[i];
        if ((unsigned)c >= (unsigned)nCells) continue;   // never: mcv_h_stage_count wrote every id in range
#pragma unroll
        for (int j = 0; j < kHCellLater; ++j)
            if (j < nLater && i < lim[j]) atomicAdd(hist + j * nCells + c, 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nt; i += blockDim.x)
        if (hist[i]) atomicAdd(pref + i, hist[i]);
}

// The second pass of the per-cell bound, lane = entry of the list the first pass wrote (src; nullptr: every
// slot below hypCount, the test hook): the box test again per cell, the candidate-relative test
// (h_cell_bound.h) on the cells of the candidate's inliers (index >= relBase), UB over the cells neither
// certifies, and per later boundary j the slot's `left`: the points of those cells that the sweep has not
// processed at that boundary, size - pref. Slots with UB >= B (inclusive) are appended to dst behind the
// slots the first pass put there (ctl[kCtlAlive + 1] counts both), their `left` figures go to
// slotLeft[j * hypCount + slot]. The candidate is the slot the
// control block's key names, read from candModels (the chunk's models; the hook's own buffer). Nothing to do
// where pruning is off on the device: the first pass then wrote the final list. Cells, prefix table and
// candidate are wave-uniform; all stores are per lane.
__global__ __launch_bounds__(256) void mcv_h_cell_rel(const HModelF* __restrict__ models,
                                                      const HModelF* __restrict__ candModels, int64_t hypBegin,
                                                      int hypCount, float thr2, double kappa,
                                                      const double* __restrict__ bb, const int* __restrict__ cells,
                                                      int nCells, int relBase, const int* __restrict__ pref,
                                                      int nLater, int* ctl, const int* __restrict__ src,
                                                      int* __restrict__ dst, int* __restrict__ slotLeft,
                                                      int* __restrict__ ubOut, uint32_t* __restrict__ bitsOut,
                                                      int bitWords, HCellPreBufs pa) {
    __shared__ int push[256 / 64 + 1];
    if (ctl[kCtlReason] != 0) return;
    const uint64_t key = *(const uint64_t*)(ctl + kCtlKey);
    if (key == 0) return;   // never with pruning on
    const int n = src ? ctl[kCtlPre] : hypCount;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x * 256 >= n) return;
    const bool have = i < n;
    const int slot = have ? (src ? src[i] : i) : 0;
    const HModelF m = models[slot];
    const HModelF cand = candModels[(int64_t)(0xFFFFFFFFull - (key & 0xFFFFFFFFull)) - hypBegin];
    double b4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) b4[j] = bb[j];
    const HCellModel cm = h_cell_model(m.h, b4, thr2, kappa, kCertT, kCertSlop);
    const HCellModel cc = h_cell_model(cand.h, b4, thr2, kappa, kCertT, kCertSlop);
    const HCellRel rel = h_cell_rel(m.h, cm, cand.h, cc);
    const HCellPreModel pm = h_cell_pre_model(cm, b4);
    int ub = 0;
    int left[kHCellLater];
#pragma unroll
    for (int j = 0; j < kHCellLater; ++j) left[j] = 0;
    const int tested = pa.rec[0];   // the non-empty cells
    int undecided = 0;              // wave-uniform
    for (int k = 0; k < tested; ++k) {
        const int* r = pa.rec + kHCellRecHead + k * kHCellRecInts;
        const int size = r[kHCellPreFloats], c = r[kHCellPreFloats + 1];
        const int* e = cells + c * kHCellInts;
        bool cert = h_cell_box_test(m.h, cm, pm, e, r, pa.on, have, undecided);
        if (c >= relBase && !cert) {
            float box[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) box[j] = h_cell_dec(e[j]);
            cert = h_cell_rel_certified(m.h, cm, cand.h, cc, rel, box);
        }
        if (!cert) {
            ub += size;
#pragma unroll
            for (int j = 0; j < kHCellLater; ++j)
                if (j < nLater) left[j] += size - pref[j * nCells + c];
        }
        if (bitsOut && cert && have) bitsOut[(size_t)slot * bitWords + (c >> 5)] |= 1u << (c & 31);
    }
    if (ubOut && have) ubOut[slot] = ub;
    h_cell_pre_stats(pa.stats, tested, have, undecided);
    const bool keep = have && ub >= ctl[kCtlB];
    if (have) {
#pragma unroll
        for (int j = 0; j < kHCellLater; ++j)
            if (j < nLater) slotLeft[(size_t)j * hypCount + slot] = left[j];
    }
    h_list_push_block<256 / 64>(keep, slot, ctl + kCtlAlive + 1, dst, push);   // the returns above are block-uniform
}

// The certified sweep in stages that prune themselves (the caller consumes only the best key): stage 0
// sweeps a prefix, its best partial count names a candidate, the candidate's full count B bounds the
// winning count from below, and from the first boundary on only the slots that can still reach B go on
// (kernels above; the exactness argument is at the caller's staging decision). Everything is enqueued
// on s: the boundaries and the live counts stay on the device, the grids are sized for every slot and
// the waves beyond the live count exit at once.
// Cell table + candidate count. With d_cells: blocks of 1024 threads, at most 64 of them, each gathering a
// private table in LDS where it fits (up to kHCellLdsCells cells), so the global atomics are one flush of the
// non-empty cells per block; larger grids add straight to the global table.
static constexpr int kHCellLdsCells = 1024;   // 36 KB of LDS
void launch_h_stage_count(const float* d_pts4, int N, const void* d_models, int64_t hypBegin, float thr2, int* d_ctl,
                          const double* d_bb, int* d_cells, int G, int Gs, int* d_cellOut, hipStream_t s) {
    if (!d_cells) {
        hipLaunchKernelGGL(mcv_h_stage_count, dim3((N + 255) / 256), dim3(256), 0, s, (const float4*)d_pts4, N,
                           (const HModelF*)d_models, hypBegin, thr2, d_ctl, HCellArgs{nullptr, nullptr, 0, 0, 0, nullptr});
        return;
    }
    const int nCells = h_cell_count(G, Gs), nt = nCells * kHCellInts;
    hipLaunchKernelGGL(mcv_h_cell_init, dim3((nt + 255) / 256), dim3(256), 0, s, d_cells, nt);
    const int lds = nCells <= kHCellLdsCells;
    const int blocks = std::min(lds ? 64 : 256, (N + 1023) / 1024);
    hipLaunchKernelGGL(mcv_h_stage_count, dim3(blocks), dim3(1024), lds ? nt * sizeof(int) : 0, s,
                       (const float4*)d_pts4, N, (const HModelF*)d_models, hypBegin, thr2, d_ctl,
                       HCellArgs{d_cells, d_bb, G, Gs, lds, d_cellOut});
}

void launch_h_cell_bound(const void* d_models, const int* d_counts, int hypCount, float thr2, const double* d_bb,
                         const int* d_cells, int G, int Gs, int* d_ctl, int* d_list, int* d_ub, uint32_t* d_bits,
                         hipStream_t s, int* d_listPre, int* d_left, int nLater, int N, HCellPreBufs pre) {
    const HCertSlopes slopes = h_cert_slopes_host(thr2);
    const int nCells = h_cell_count(G, Gs);
    hipLaunchKernelGGL(mcv_h_cell_bound, dim3((hypCount + 255) / 256), dim3(256), 0, s, (const HModelF*)d_models,
                       d_counts, hypCount, thr2, h_cell_kappa(slopes.a.x, slopes.a.y), d_bb, d_cells, nCells, d_ctl,
                       d_list, HCellPre{d_listPre, d_left, G * G * G * G, nLater, N}, d_ub, d_bits, (nCells + 31) / 32,
                       pre);
}

// The record list of the non-empty cells (h_cell_rec_ints(cells) ints) from the cell table, for the two bound
// passes: they loop over it whether the prefilter is on or off.
void launch_h_cell_pre(const int* d_cells, int G, int Gs, float thr2, int* d_rec, hipStream_t s) {
    const HCertSlopes slopes = h_cert_slopes_host(thr2);
    hipLaunchKernelGGL(mcv_h_cell_pre_build, dim3(1), dim3(1024), 0, s, d_cells, h_cell_count(G, Gs),
                       h_cell_kappa(slopes.a.x, slopes.a.y), d_rec);
}

// mcvTestHCellPreVerdicts: lane = model, the prefilter's verdict for every cell of the table (empty ones too).
__global__ __launch_bounds__(256) void mcv_h_cell_pre_verdicts(const HModelF* __restrict__ models, int nModels,
                                                               float thr2, double kappa, const double* __restrict__ bb,
                                                               const int* __restrict__ cells, int nCells,
                                                               const int* __restrict__ rec,
                                                               uint8_t* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nModels) return;
    const HModelF m = models[i];
    double b4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) b4[j] = bb[j];
    const HCellModel cm = h_cell_model(m.h, b4, thr2, kappa, kCertT, kCertSlop);
    const HCellPreModel pm = h_cell_pre_model(cm, b4);
    for (int c = 0; c < nCells; ++c) {
        if (cells[c * kHCellInts + kHCellInts - 1] != 0) continue;   // non-empty: from its record, below
        float box[8], q[kHCellPreFloats];
#pragma unroll
        for (int j = 0; j < 8; ++j) box[j] = h_cell_dec(cells[c * kHCellInts + j]);
        h_cell_pre_box(box, kappa, q);
        out[(size_t)i * nCells + c] = (uint8_t)h_cell_pre(m.h, pm, q);
    }
    // the floats mcv_h_cell_pre_build wrote, as the two bound passes read them
    const int nRec = rec[0];
    for (int k = 0; k < nRec; ++k) {
        const int* r = rec + kHCellRecHead + k * kHCellRecInts;
        float q[kHCellPreFloats];
#pragma unroll
        for (int j = 0; j < kHCellPreFloats; ++j) q[j] = __int_as_float(r[j]);
        const int c = r[kHCellPreFloats + 1];
        if ((unsigned)c < (unsigned)nCells) out[(size_t)i * nCells + c] = (uint8_t)h_cell_pre(m.h, pm, q);
    }
}

void launch_h_cell_pre_verdicts(const void* d_models, int nModels, float thr2, const double* d_bb, const int* d_cells,
                                const int* d_rec, int G, int Gs, uint8_t* d_out, hipStream_t s) {
    const HCertSlopes slopes = h_cert_slopes_host(thr2);
    hipLaunchKernelGGL(mcv_h_cell_pre_verdicts, dim3((nModels + 255) / 256), dim3(256), 0, s,
                       (const HModelF*)d_models, nModels, thr2, h_cell_kappa(slopes.a.x, slopes.a.y), d_bb, d_cells,
                       h_cell_count(G, Gs), d_rec, d_out);
}

// d_pref: nLater x cells ints, from the cell ids mcv_h_stage_count kept and the control block's boundaries
void launch_h_cell_prefix(const int* d_cellId, int N, const int* d_ctl, int nLater, int G, int Gs, int* d_pref,
                          hipStream_t s) {
    const int nCells = h_cell_count(G, Gs);
    const size_t bytes = (size_t)nLater * nCells * sizeof(int);   // at most 4 x 1872 ints of LDS
    (void)hipMemsetAsync(d_pref, 0, bytes, s);
    const int blocks = std::min(64, (N + 1023) / 1024);
    hipLaunchKernelGGL(mcv_h_cell_prefix, dim3(blocks), dim3(1024), bytes, s, d_cellId, N, d_ctl, nLater, nCells,
                       d_pref);
}

// The second pass over d_src (the first pass's list, its length in ctl[kCtlPre]; nullptr: every slot).
// d_left: nLater x hypCount ints.
void launch_h_cell_rel(const void* d_models, const void* d_candModels, int64_t hypBegin, int hypCount, float thr2,
                       const double* d_bb, const int* d_cells, int G, int Gs, const int* d_pref, int nLater,
                       int* d_ctl, const int* d_src, int* d_list, int* d_left, int* d_ub, uint32_t* d_bits,
                       hipStream_t s, HCellPreBufs pre) {
    const HCertSlopes slopes = h_cert_slopes_host(thr2);
    const int nCells = h_cell_count(G, Gs);
    hipLaunchKernelGGL(mcv_h_cell_rel, dim3((hypCount + 255) / 256), dim3(256), 0, s, (const HModelF*)d_models,
                       (const HModelF*)d_candModels, hypBegin, hypCount, thr2, h_cell_kappa(slopes.a.x, slopes.a.y),
                       d_bb, d_cells, nCells, G * G * G * G, d_pref, nLater, d_ctl, d_src, d_list, d_left, d_ub,
                       d_bits, (nCells + 31) / 32, pre);
}

// The device's h_cell_box_test on the host: the prefilter (pre) and fp64 for what it leaves undecided.
// stats (may be nullptr): [0] tests, [1] undecided of them.
static bool h_cell_box_host(const float* h, const HCellModel& cm, const HCellPreModel& pm, const float* box, bool pre,
                            double kappa, long long* stats, uint8_t* verdict) {
    int v = kHCellPreUndecided;
    if (pre || verdict) {
        float q[kHCellPreFloats];
        h_cell_pre_box(box, kappa, q);
        const int pv = h_cell_pre(h, pm, q);
        if (verdict) *verdict = (uint8_t)pv;
        if (pre) v = pv;
    }
    if (stats) {
        ++stats[0];
        stats[1] += v == kHCellPreUndecided;
    }
    return v == kHCellPreUndecided ? h_cell_certified(h, cm, box) : v == kHCellPreCert;
}

// Host twin of the cell build and the bound (mcvTestHCellBound): the same headers, the same arithmetic.
// pre: with the fp32 prefilter in front (as the device kernels run it); stats: its counters; verdicts (nModels x
// cells bytes): its three-way verdict for every cell, empty ones included (mcvTestHCellPreVerdicts).
void h_cell_host(const float* pts4, int N, const float* cand8, const float* models8, int nModels, float thr2, int B,
                 int G, int Gs, int* cellId, float* boxes, int* sizes, int* ub, uint32_t* bits, int* alive, bool pre,
                 long long* stats, uint8_t* verdicts) {
    const int nCells = h_cell_count(G, Gs), words = (nCells + 31) / 32;
    double bb[4] = {0, 0, 0, 0};
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < 4; ++j) {
            const double v = pts4[4 * i + j];
            bb[j] = v == v ? fmax(bb[j], fabs(v)) : __builtin_inf();
        }
    std::vector<int> tab((size_t)nCells * kHCellInts);
    for (size_t i = 0; i < tab.size(); ++i) {
        const int f = (int)(i % kHCellInts);
        tab[i] = f == kHCellInts - 1 ? 0 : ((f & 1) ? INT32_MIN : INT32_MAX);
    }
    for (int i = 0; i < N; ++i) {
        const float* q = pts4 + 4 * i;
        const bool in = h_error(cand8, q[0], q[1], q[2], q[3]) <= thr2;
        const int c = h_cell_index(q[0], q[1], q[2], q[3], in, bb, G, Gs);
        if (cellId) cellId[i] = c;
        int* t = tab.data() + (size_t)c * kHCellInts;
        for (int j = 0; j < 4; ++j) {
            const int e = h_cell_enc(q[j]);
            t[2 * j] = std::min(t[2 * j], e);
            t[2 * j + 1] = std::max(t[2 * j + 1], e);
        }
        ++t[8];
    }
    for (int c = 0; c < nCells; ++c) {
        for (int j = 0; j < 8; ++j) boxes[8 * c + j] = h_cell_dec(tab[(size_t)c * kHCellInts + j]);
        sizes[c] = tab[(size_t)c * kHCellInts + 8];
    }
    const HCertSlopes slopes = h_cert_slopes_host(thr2);
    const double kappa = h_cell_kappa(slopes.a.x, slopes.a.y);
    int kept = 0;
    for (int k = 0; k < nModels; ++k) {
        const float* h = models8 + 8 * k;
        const HCellModel cm = h_cell_model(h, bb, thr2, kappa, kCertT, kCertSlop);
        const HCellPreModel pm = h_cell_pre_model(cm, bb);
        int u = 0;
        for (int w = 0; w < words; ++w) bits[(size_t)k * words + w] = 0;
        for (int c = 0; c < nCells; ++c) {
            uint8_t* vd = verdicts ? verdicts + (size_t)k * nCells + c : nullptr;
            if (sizes[c] == 0) {
                if (vd) {
                    float q[kHCellPreFloats];
                    h_cell_pre_box(boxes + 8 * c, kappa, q);
                    *vd = (uint8_t)h_cell_pre(h, pm, q);
                }
                continue;
            }
            const bool cert = h_cell_box_host(h, cm, pm, boxes + 8 * c, pre, kappa, stats, vd);
            u += cert ? 0 : sizes[c];
            if (cert) bits[(size_t)k * words + (c >> 5)] |= 1u << (c & 31);
        }
        ub[k] = u;
        kept += u >= B;
    }
    if (alive) *alive = kept;
}

// Host twin of the second pass (mcvTestHCellRel): the union of the box test and the candidate-relative test,
// UB and the `left` figures at the given boundaries (in pairs of points, the control block's unit).
void h_cell_rel_host(const float* pts4, int N, const float* cand8, const float* models8, int nModels, float thr2,
                     int B, int G, int Gs, const int* bounds, int nBounds, int* cellId, int* ub, uint32_t* bits,
                     int* left, int* alive, bool pre, long long* stats) {
    const int nCells = h_cell_count(G, Gs), words = (nCells + 31) / 32, relBase = G * G * G * G;
    std::vector<float> boxes((size_t)nCells * 8);
    std::vector<int> sizes(nCells), u0(nModels);
    std::vector<uint32_t> b0((size_t)nModels * words);
    h_cell_host(pts4, N, cand8, models8, nModels, thr2, B, G, Gs, cellId, boxes.data(), sizes.data(), u0.data(),
                b0.data(), nullptr, false, nullptr, nullptr);
    double bb[4] = {0, 0, 0, 0};
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < 4; ++j) {
            const double v = pts4[4 * i + j];
            bb[j] = v == v ? fmax(bb[j], fabs(v)) : __builtin_inf();
        }
    std::vector<int> pref((size_t)nBounds * nCells, 0);
    for (int j = 0; j < nBounds; ++j) {
        const int64_t d2 = 2 * (int64_t)bounds[j];
        const int lim = d2 < N ? (int)d2 : N;
        for (int i = 0; i < lim; ++i) ++pref[(size_t)j * nCells + cellId[i]];
    }
    const HCertSlopes slopes = h_cert_slopes_host(thr2);
    const double kappa = h_cell_kappa(slopes.a.x, slopes.a.y);
    const HCellModel cc = h_cell_model(cand8, bb, thr2, kappa, kCertT, kCertSlop);
    int kept = 0;
    for (int k = 0; k < nModels; ++k) {
        const float* h = models8 + 8 * k;
        const HCellModel cm = h_cell_model(h, bb, thr2, kappa, kCertT, kCertSlop);
        const HCellRel rel = h_cell_rel(h, cm, cand8, cc);
        const HCellPreModel pm = h_cell_pre_model(cm, bb);
        int u = 0;
        for (int w = 0; w < words; ++w) bits[(size_t)k * words + w] = 0;
        for (int j = 0; j < nBounds; ++j) left[(size_t)j * nModels + k] = 0;
        for (int c = 0; c < nCells; ++c) {
            if (sizes[c] == 0) continue;
            const float* box = boxes.data() + 8 * c;
            bool cert = h_cell_box_host(h, cm, pm, box, pre, kappa, stats, nullptr);
            if (c >= relBase && !cert) cert = h_cell_rel_certified(h, cm, cand8, cc, rel, box);
            if (cert) {
                bits[(size_t)k * words + (c >> 5)] |= 1u << (c & 31);
                continue;
            }
            u += sizes[c];
            for (int j = 0; j < nBounds; ++j) left[(size_t)j * nModels + k] += sizes[c] - pref[(size_t)j * nCells + c];
        }
        ub[k] = u;
        kept += u >= B;
    }
    if (alive) *alive = kept;
}

// With the per-cell bound and d_s0 (s0Slots ints, fewer than hypCount) stage 0 sweeps the prefix for the first
// s0Slots slots only, into d_s0: it exists to name the candidate. d_counts then keeps the generate's 0 / status
// until stage 1, which runs the bound's list from point 0 (the plan resets boundary 1).
// d_ctl: kHStageCtlInts ints; d_list: 2 x hypCount ints (the survivor lists, ping-pong).
// d_cells (h_cell_count(G, Gs) x kHCellInts ints; nullptr: no per-cell bound): the cell table is built beside
// the candidate's count, mcv_h_cell_bound drops the slots whose upper bound is below B before stage 1, and
// stage 1 runs through its list. d_cell (with d_cells; id == nullptr: the box pass alone, the compactions
// on N - processed): every point's cell id (N ints), the prefix table
// (kHStageCellLater x cells ints) and the per-slot `left` figures (kHStageCellLater x hypCount ints) that the
// later boundaries' tests use in place of N - processed (why that is exact: the caller's staging decision).
// With the second pass (d_cell.id) the plan has the half boundary: 5 stages (0, 1a, 1b, 2, 3), else 4.
void launch_h_verify_staged(const float* d_pts4, const void* d_pairs, int N, const void* d_models, int* d_counts,
                            int hypCount, int64_t hypBegin, float thr2, const double* d_bb, int* d_ctl, int* d_list,
                            uint64_t* d_pkey, int64_t* d_pfail, hipStream_t s, const void* d_rec,
                            unsigned long long* d_stats, int form, int* d_cells, int G, int Gs, HCellBufs d_cell,
                            HCellPreBufs d_pre, int* d_s0, int s0Slots) {
    // stage 0 on the first s0 slots only, into d_s0 (0: on every slot, into d_counts); only with the bound, whose
    // list stage 1 then runs from point 0
    const int s0 = d_cells && d_s0 && s0Slots > 0 && s0Slots < hypCount ? s0Slots : 0;
    if (d_stats) (void)hipMemsetAsync(d_stats, 0, kHMfmaStats * sizeof(unsigned long long), s);
    const bool mfma = d_rec && d_stats && h_mfma_engages(N, hypCount, form, true);
    // the form's engage rule goes by the launch's width
    const bool mfma0 = s0 ? d_rec && d_stats && h_mfma_engages(N, s0, form, true) : mfma;
    // stages that run a list keep the VALU kernel; kHFormMfma is the A/B partner
    const bool mfmaList = mfma && form == kHFormMfma;
    const HStagePlanArgs pa = h_stage_plan_args(N, d_cells != nullptr);
    const HCertSlopes slopes = h_cert_slopes_host(thr2);
    const bool rel = d_cells && d_cell.id;   // the bound's second pass and the per-slot `left`
    // with the second pass the half boundary splits stage 1 (kernels.h): one stage and one `left` row more
    const int rows = rel ? kHStageCellLater : kHStageLater;   // the boundaries behind a list stage
    const int nStages = 2 + rows;
    int* lists[2] = {d_list, d_list + hypCount};
    auto stage = [&](int st, const int* list) {   // the list of stage st is lists[st & 1]
        const HStageArgs sa{d_ctl, list, st};
        int* cnt = st == 0 && s0 ? d_s0 : d_counts;
        const int width = st == 0 && s0 ? s0 : hypCount;
        if (list ? mfmaList : (st == 0 ? mfma0 : mfma))
            launch_h_mfma_sweep(d_pts4, d_rec, N, d_models, cnt, width, thr2, slopes, d_bb, sa, d_stats, s);
        else
            launch_h_cert_sweep(d_pairs, N, d_models, cnt, width, thr2, slopes, d_bb, sa, s);
    };
    hipLaunchKernelGGL(mcv_h_stage_init, dim3(1), dim3(64), 0, s, d_ctl, pa.pa, hypCount,
                       d_cells ? h_cell_count(G, Gs) : 0, s0 ? s0 : hypCount);
    if (s0) {
        // the subset's statuses as the generate wrote them, and the chunk's first sampler failure from one pass
        // over every slot's status (d_counts holds 0 or a status until stage 1): the key that pass packs is not read
        (void)hipMemcpyAsync(d_s0, d_counts, (size_t)s0 * sizeof(int), hipMemcpyDeviceToDevice, s);
        launch_best(d_counts, hypCount, hypBegin, 0, d_pkey, d_pfail, (uint64_t*)(d_ctl + kCtlFailAll - 2), s);
    }
    stage(0, nullptr);
    // candidate: the best partial count before any sampler failure (minimum count 0: any model will do)
    launch_best(s0 ? d_s0 : d_counts, s0 ? s0 : hypCount, hypBegin, 0, d_pkey, d_pfail, (uint64_t*)(d_ctl + kCtlKey), s);
    launch_h_stage_count(d_pts4, N, d_models, hypBegin, thr2, d_ctl, d_bb, d_cells, G, Gs, rel ? d_cell.id : nullptr, s);
    hipLaunchKernelGGL(mcv_h_stage_plan, dim3(1), dim3(64), 0, s, d_ctl, N, pa.trip, pa.later, pa.slackPts,
                       pa.latest256, s0 ? 1 : 0, rel ? 1 : 0);
    // the list of stage 1 is lists[1 & 1], the source of the first count-based test: the box pass writes
    // lists[1] (the slots the relative test cannot drop) and lists[0] (the others), the second pass (box +
    // candidate-relative test, the per-slot `left`) appends what it keeps of lists[0] to lists[1]
    if (d_cells && d_pre.stats) (void)hipMemsetAsync(d_pre.stats, 0, 2 * sizeof(unsigned long long), s);
    if (d_cells) launch_h_cell_pre(d_cells, G, Gs, thr2, d_pre.rec, s);
    if (d_cells && !rel)
        launch_h_cell_bound(d_models, d_counts, hypCount, thr2, d_bb, d_cells, G, Gs, d_ctl, lists[1], nullptr, nullptr,
                            s, nullptr, nullptr, 0, 0, d_pre);
    if (rel) {
        launch_h_cell_prefix(d_cell.id, N, d_ctl, rows, G, Gs, d_cell.pref, s);
        launch_h_cell_bound(d_models, d_counts, hypCount, thr2, d_bb, d_cells, G, Gs, d_ctl, lists[1], nullptr, nullptr,
                            s, lists[0], d_cell.left, rows, N, d_pre);
        launch_h_cell_rel(d_models, d_models, hypBegin, hypCount, thr2, d_bb, d_cells, G, Gs, d_cell.pref, rows,
                          d_ctl, lists[0], lists[1], d_cell.left, nullptr, nullptr, s, d_pre);
    }
    // With the bound's second pass: stage 1a, compaction, stage 1b, compaction, stage 2, compaction, stage 3;
    // without it the plan has no half boundary (and without the bound stage 1 runs full width). Behind an empty stage (boundaries that coincide) the
    // compaction hands the list on, with the same test on the unchanged counts.
    stage(1, d_cells ? lists[1] : nullptr);
    for (int st = 2; st < nStages; ++st) {
        launch_h_stage_compact(d_counts, hypCount, N, d_ctl, st, st == 2 && !d_cells ? nullptr : lists[(st - 1) & 1],
                               lists[st & 1], rel ? d_cell.left : nullptr, s);
        stage(st, lists[st & 1]);
    }
    // One recount, behind the last stage. A wave that leaves the fast path (a model outside the certificate's
    // domain; event overflow in the tail of the last stage) marks its slots kStatusRedo. A marked slot enters no
    // later list: every compaction reads the mark (count < 0), which only this recount overwrites. So no stage
    // adds to a marked slot, and the recount over all N gives it its full count whenever it runs. The recount that
    // used to sit behind the first compaction changed nothing that a stage or a compaction reads, and cost a
    // launch over every slot (0.04 ms at 2^20 hypotheses): it pays for the half boundary's two launches where
    // pruning is off on the device and they do nothing.
    launch_h_recount(d_pts4, N, d_models, d_counts, hypCount, thr2, false, nullptr, s);
}

}  // namespace mcv
