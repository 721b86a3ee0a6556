// ransac_h_gen.hip — homography hypothesis generation on gfx950: Philox sample -> subset check -> 4-point
// DLT in fp64 (runKernel's normalisation, LtL and 9x9 Jacobi eigen-solve) -> fp32 model (32 B) + fp64 model
// + status, one lane per hypothesis.                                      [SURVEY §2 K1, first half]
//
//   mcv_h_generate          the one-pass solve (and the MCV_FLAG_FAST_MINIMAL elimination)
//   mcv_h_gen_aw / _v / _ovf  the default: the eigen-solve split in two passes over a rotation log
//   mcv_h_gen_r             the certified one-row pass 2 (key-only evaluates): the reverse replay of one row
//                           nominates the fp32 model, mcv_h_gen_v_list solves the lanes it cannot certify
//   mcv_h_one               one hypothesis in full (the finalize path's winner re-solve)
//
// Built with -ffp-contract=off (see hyp_homography.h): every model is the host twin's, bit for bit.
#include <algorithm>
#include "mcv_common.h"
#include "hyp_homography.h"
#include "kernels.h"
#include "minicv_native.h"

namespace mcv {

// ------------------------------------------------------------------------------------------
// Hypothesis generation
// ------------------------------------------------------------------------------------------
// One lane per hypothesis; the runKernel eigen-solve's working set (127 doubles) in LDS, one slice
// per lane (jacobi_eig.h): 40.6 KB per 40-lane block, 4 blocks per CU. FAST = MCV_FLAG_FAST_MINIMAL
// (no workspace).
template <bool FAST, int L = kEigLanes>
__global__ __launch_bounds__(FAST ? 256 : L) void mcv_h_generate(const float* __restrict__ pts4, int N, Sampler smp,
                                                     int64_t hypBegin, int hypCount, HModelF* __restrict__ models,
                                                     double* __restrict__ h64, int* __restrict__ counts) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hypCount) return;
    double H[9];
    HModelF mf;
    int st;
    if constexpr (FAST) {
        EigWsLocal unused;   // the elimination never touches it (folded away)
        st = h_hypothesis(pts4, N, smp, (uint64_t)(hypBegin + i), H, &mf, nullptr, unused, true);
    } else {
        __shared__ double lds[kEigWs * L];
        EigWsLane ws{lds + threadIdx.x * kEigWs};
        st = h_hypothesis(pts4, N, smp, (uint64_t)(hypBegin + i), H, &mf, nullptr, ws);
    }
    if (st == 1) {
        models[i] = mf;
        for (int j = 0; j < 9; ++j) h64[9 * (int64_t)i + j] = H[j];
        counts[i] = 0;
    } else {
        // the zero model (w = 1 everywhere) keeps the packed sweep's slot well-defined
        for (int j = 0; j < 8; ++j) mf.h[j] = 0.f;
        models[i] = mf;
        counts[i] = st;
    }
}

// The default generate as two passes over the split eigen-solve (round 6; jacobi_eig.h):
//   mcv_h_gen_aw  lane per hypothesis: sample, subset check, runKernel's normalisation and LtL, then
//                 JacobiImpl_ on the upper triangle and W only (a 45-double LDS slice per lane, 360 B
//                 against the one-pass solve's 1016 B: 2.8x the lanes per CU) with every rotation's
//                 (c, s, k, l) logged to HBM (16 B; SoA by hypothesis, so a wave's log writes and reads
//                 are contiguous); the sort of W names the eigenvector's row r;
//   mcv_h_gen_v   lane per hypothesis: V rebuilt from the log (an 81-double slice), row r -> H0, the
//                 de-normalisation and the fp32 model (the normalisation recomputed from the stored
//                 sample's four points);
//   mcv_h_gen_ovf the one-pass solve for the lanes whose rotation count exceeded the log's capacity
//                 (kEigLogCap; a cfg3 LtL takes 110-157 rotations) — normally none.
// Every value is computed by the same operations in the same order as the one-pass solve, so the
// models are the same bits (tests: the whole-range cfg3 counts, the eigen stress test).
static constexpr int kEigLogCap = 192;
// the log rows pass 1 may use (mcvTestEigLogCap lowers it so the tests drive the overflow path)
static int g_eig_log_cap = kEigLogCap;
// 64 x 360 B = 22.5 KB: 7 blocks of one full wave per CU (7 x 23040 B of the 160 KB). Screen on the
// trimmed rotation loop ("Fewer instructions per rotation in pass 1"; kernel ms per 2^20
// hypotheses): 56 lanes (8 blocks of 20480 B, the former choice) 2.909, 60 lanes 3.014, 64 lanes 2.847.
// Round 6 had screened 64 lanes only with 376-byte slices, where six blocks fit (40 / 64 / 32-lane
// blocks, 10 / 6 / 13 per CU: 6.6 / 5.7 / 6.7 ms against 5.2 ms of generate per 2^20 at 54).
static constexpr int kHGenAwLanes = 64;
// pass 2: one column of V per lane (9 lanes per hypothesis, 7 hypotheses per 63-lane block), 4 log
// loads in flight. Round-6 screen at cfg3 (generate ms per 2^20 hypotheses, pass 1 ~3.7 of it): one
// lane per hypothesis with one load ahead 5.78, with 8 ahead 5.78; 3 lanes x 3 columns 5.16-5.17 (V
// transposed 5.06); 9 lanes 4.76-4.81 (8 loads ahead, V transposed, 14 hypotheses per block: the same).
// Every 9-lane form moves the same 288 LDS bytes per rotation and hypothesis: LDS-bandwidth-bound.
static constexpr int kHGenVG = 9, kHGenVQ = 7, kHGenVD = 4;
static constexpr int kHGenOvfBlocks = 64;
// meta: >= 0 -> rotation count | r << 16 (pass 2 builds the model); kMetaDone: pass 1 wrote the
// status; kMetaOverflow: mcv_h_gen_ovf solves it
static constexpr int kMetaDone = -1, kMetaOverflow = -2;

__device__ __forceinline__ void h_store_none(HModelF* models, int* counts, int i, int st) {
    HModelF mf;
    for (int j = 0; j < 8; ++j) mf.h[j] = 0.f;   // the zero model (w = 1) keeps the sweep's slot defined
    models[i] = mf;
    counts[i] = st;
}

template <int L>
__global__ __launch_bounds__(L) void mcv_h_gen_aw(const float* __restrict__ pts4, int N, Sampler smp,
                                                  int64_t hypBegin, int count, HModelF* __restrict__ models,
                                                  int* __restrict__ counts, int4* __restrict__ sidx,
                                                  int* __restrict__ meta, EigRot* __restrict__ log, int logStride,
                                                  int* __restrict__ ovf, int ovfBase, int logCap) {
    const int j = blockIdx.x * L + threadIdx.x;   // lane within the piece
    if (j >= count) return;
    const int i = ovfBase + j;                    // hypothesis within the chunk
    __shared__ double lds[kEigAwWs * L];
    EigWsLane ws{lds + threadIdx.x * kEigAwWs};
    float sx[4], sy[4], dx[4], dy[4];
    int idx[4];
    double nm[8];
    int st = 0;
    if (!h_sample(pts4, N, smp, (uint64_t)(hypBegin + i), sx, sy, dx, dy, idx)) st = kStatusNoSample;
    else if (!h_norm4(sx, sy, dx, dy, nm) || !h_ltl4(sx, sy, dx, dy, nm, ws)) st = kStatusNoModel;
    if (st != 0) {
        h_store_none(models, counts, i, st);
        meta[j] = kMetaDone;
        return;
    }
    double w[9];
    int nrot = 0;
    const int r = eig9_jacobi<EigWsLane, true>(ws, w, 8, &nrot, log + j, logStride, logCap);
    sidx[j] = make_int4(idx[0], idx[1], idx[2], idx[3]);
    if (nrot < 0) {
        meta[j] = kMetaOverflow;
        ovf[1 + atomicAdd(ovf, 1)] = i;
        return;
    }
    meta[j] = nrot | (r << 16);
}

// Pass 2 for piece lane j with meta word m, run by the G lanes of its group (every lane of the block calls it:
// it holds a barrier): V from the log, row r -> the models of hypothesis base + j. CNT = false: no status written
// (finalize's winner: the counts buffer holds the sweep's counts by then).
template <int G, int D, bool TR, bool CNT>
__device__ __forceinline__ void h_gen_v_lane(const float* __restrict__ pts4, int j, int m, int g, EigWsLane v, int base,
                                             const int4* __restrict__ sidx, const EigRot* __restrict__ log,
                                             int logStride, HModelF* __restrict__ models, double* __restrict__ h64,
                                             int* __restrict__ counts) {
    constexpr int C = 9 / G;
    if (m >= 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i)
#pragma unroll
            for (int c = 0; c < C; ++c) v[TR ? 9 * (g * C + c) + i : 9 * i + g * C + c] = (i == g * C + c) ? 1.0 : 0.0;
        eig9_replay_cols<C, D, TR>(v, g * C, log + j, logStride, m & 0xffff);
    }
    if constexpr (G > 1) __syncthreads();   // the row's other columns come from the group's other lanes
    if (m < 0 || g != 0) return;
    const int i = base + j;
    const int r = m >> 16;
    double H0[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) H0[k] = v[TR ? 9 * k + r : 9 * r + k];
    const int4 id = sidx[j];
    const int ix[4] = {id.x, id.y, id.z, id.w};
    float sx[4], sy[4], dx[4], dy[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float4 q = reinterpret_cast<const float4*>(pts4)[ix[k]];
        sx[k] = q.x; sy[k] = q.y; dx[k] = q.z; dy[k] = q.w;
    }
    double nm[8], H[9];
    HModelF mf;
    (void)h_norm4(sx, sy, dx, dy, nm);   // pass 1 accepted this sample: the same values again
    if (h_from_eig(H0, nm, H) && h_model_f(H, &mf)) {
        models[i] = mf;
        for (int k = 0; k < 9; ++k) h64[9 * (int64_t)i + k] = H[k];
        if constexpr (CNT) counts[i] = 0;
    } else {
        if constexpr (CNT) h_store_none(models, counts, i, kStatusNoModel);
    }
}

// Pass 2: G lanes per hypothesis (9 / G columns of V each; G = 1 or 3), Q hypotheses per block.
template <int G, int Q, int D, bool TR = false>
__global__ __launch_bounds__(G * Q) void mcv_h_gen_v(const float* __restrict__ pts4, int count, int base,
                                                     const int4* __restrict__ sidx, const int* __restrict__ meta,
                                                     const EigRot* __restrict__ log, int logStride,
                                                     HModelF* __restrict__ models, double* __restrict__ h64,
                                                     int* __restrict__ counts) {
    const int h = threadIdx.x / G, g = threadIdx.x - h * G;   // hypothesis of the block, column group
    const int j = blockIdx.x * Q + h;
    __shared__ double lds[kEigVWs * Q];
    EigWsLane v{lds + h * kEigVWs};
    const int m = j < count ? meta[j] : kMetaDone;
    h_gen_v_lane<G, D, TR, true>(pts4, j, m, g, v, base, sidx, log, logStride, models, h64, counts);
}

// Pass 2 for the one-row pass's undecided lanes: a fixed grid strides over list[1 .. list[0]], the piece-local
// lanes to solve (list == nullptr: the one lane `single`, finalize's winner, with CNT = false).
template <int G, int Q, int D, bool CNT, bool TR = false>
__global__ __launch_bounds__(G * Q) void mcv_h_gen_v_list(const float* __restrict__ pts4, int count, int base,
                                                          const int4* __restrict__ sidx, const int* __restrict__ meta,
                                                          const EigRot* __restrict__ log, int logStride,
                                                          HModelF* __restrict__ models, double* __restrict__ h64,
                                                          int* __restrict__ counts, const int* __restrict__ list,
                                                          int single) {
    const int h = threadIdx.x / G, g = threadIdx.x - h * G;
    __shared__ double lds[kEigVWs * Q];
    EigWsLane v{lds + h * kEigVWs};
    const int n = list ? min(list[0], count) : 1;
    for (int e0 = blockIdx.x * Q; e0 < n; e0 += gridDim.x * Q) {   // the same trips for every lane of the block
        const int e = e0 + h;
        const int j = e < n ? (list ? list[1 + e] : single) : -1;
        const int m = (j >= 0 && j < count) ? meta[j] : kMetaDone;
        h_gen_v_lane<G, D, TR, CNT>(pts4, j, m, g, v, base, sidx, log, logStride, models, h64, counts);
        if constexpr (G > 1) __syncthreads();   // the slices are rewritten by the next trip
    }
}

// The certified one-row pass 2 (jacobi_eig.h eig9_replay_row_rev, hyp_homography.h h_model_f_cert): lane per
// hypothesis, one wave per block, y in a 9-double LDS slice (odd stride). The wave walks the log rows from
// its largest rotation count down, so every step reads one contiguous row. A decided lane writes its fp32
// model and status 0 (no h64: finalize replays the winner); an undecided one appends its piece-local index
// to und[1 ..] (und[0] = the length; one atomic per wave) for mcv_h_gen_v_list. Lanes pass 1 finished
// (meta < 0: status written, or handed to mcv_h_gen_ovf) are skipped. stats[0 / 1] += decided / undecided
// lanes, the overflow lanes among the latter. errScale multiplies err (mcvTestHGenRow: 2^40 leaves no lane
// decided).
static constexpr int kHGenRD = 8;
__global__ __launch_bounds__(64) void mcv_h_gen_r(const float* __restrict__ pts4, int count, int base,
                                                  const int4* __restrict__ sidx, const int* __restrict__ meta,
                                                  const EigRot* __restrict__ log, int logStride,
                                                  HModelF* __restrict__ models, int* __restrict__ counts,
                                                  int* __restrict__ und, int* __restrict__ stats, double errScale) {
    __shared__ double lds[9 * 64];
    const int lane = threadIdx.x;
    const int j = blockIdx.x * 64 + lane;
    const int m = j < count ? meta[j] : kMetaDone;
    const int nrot = m >= 0 ? (m & 0xffff) : 0;
    int ntop = nrot;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ntop = max(ntop, __shfl_xor(ntop, o));
    EigWsLane ys{lds + lane * 9};
    double err = 0;
    eig9_replay_row_rev<kHGenRD>(log + j, logStride, nrot, ntop, m >= 0 ? (m >> 16) : 0, ys, &err);
    bool dec = false;
    if (m >= 0) {
        double y[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) y[k] = ys[k];
        const int4 id = sidx[j];
        const int ix[4] = {id.x, id.y, id.z, id.w};
        float sx[4], sy[4], dx[4], dy[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 q = reinterpret_cast<const float4*>(pts4)[ix[k]];
            sx[k] = q.x; sy[k] = q.y; dx[k] = q.z; dy[k] = q.w;
        }
        double nm[8];
        HModelF mf;
        (void)h_norm4(sx, sy, dx, dy, nm);   // pass 1 accepted this sample: the same values again
        dec = h_model_f_cert(y, err * errScale, nm, &mf);
        if (dec) {
            models[base + j] = mf;
            counts[base + j] = 0;
        }
    }
    const bool un = m >= 0 && !dec;
    const uint64_t bu = __ballot(un), bd = __ballot(dec), bo = __ballot(m == kMetaOverflow);
    int at = 0;
    if (lane == 0) {
        if (bu) at = atomicAdd(und, (int)__popcll(bu));
        if (bd) atomicAdd(stats, (int)__popcll(bd));
        if (bu | bo) atomicAdd(stats + 1, (int)__popcll(bu) + (int)__popcll(bo));
    }
    at = __shfl(at, 0);
    if (un) und[1 + at + (int)__popcll(bu & ((1ull << lane) - 1ull))] = j;
}

template <int L>
__global__ __launch_bounds__(L) void mcv_h_gen_ovf(const float* __restrict__ pts4, int N, Sampler smp,
                                                   int64_t hypBegin, const int* __restrict__ ovf,
                                                   HModelF* __restrict__ models, double* __restrict__ h64,
                                                   int* __restrict__ counts) {
    __shared__ double lds[kEigWs * L];
    EigWsLane ws{lds + threadIdx.x * kEigWs};
    const int n = ovf[0];
    for (int j = blockIdx.x * L + threadIdx.x; j < n; j += gridDim.x * L) {
        const int i = ovf[1 + j];
        double H[9];
        HModelF mf;
        const int st = h_hypothesis(pts4, N, smp, (uint64_t)(hypBegin + i), H, &mf, nullptr, ws);
        if (st == 1) {
            models[i] = mf;
            for (int k = 0; k < 9; ++k) h64[9 * (int64_t)i + k] = H[k];
            counts[i] = 0;
        } else {
            h_store_none(models, counts, i, st);
        }
    }
}

// One hypothesis in full (finalize path): fp64 model, fp32 model, status, sample.
__global__ void mcv_h_one(const float* __restrict__ pts4, int N, Sampler smp, int64_t hyp, HOneOut* __restrict__ out,
                          bool fast) {
    __shared__ double lds[kEigWs];
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    EigWsLane ws{lds};
    HOneOut o;
    HModelF mf;
    for (int j = 0; j < 9; ++j) o.H[j] = 0;
    for (int j = 0; j < 8; ++j) mf.h[j] = 0;
    o.status = h_hypothesis(pts4, N, smp, (uint64_t)hyp, o.H, &mf, o.idx, ws, fast);
    for (int j = 0; j < 8; ++j) o.hf[j] = mf.h[j];
    *out = o;
}

// Rows of the split generate's scratch per piece: the whole call up to 2^20 hypotheses (3.2 GB of
// rotation log at 192 entries of 16 B). Round 6, same box: one piece 4.40 ms per 2^20 against 4.85 ms
// for pieces of two rounds of mcv_h_gen_aw's resident lanes (5 pieces: each launch drains its slowest
// waves, whose rotation counts vary per lane), 4.69 / 4.67 for pieces of four rounds / two halves.
static constexpr int kHGenMaxPiece = 1 << 20;
static int h_gen_piece(int hypCount) { return std::min(hypCount, kHGenMaxPiece); }

// The scratch of the split generate: one piece's rotation log, samples and meta words, the overflow list of
// the whole call, and the one-row pass's undecided list (one piece) with its two counters.
struct HGenScratch {
    EigRot* log;
    int4* sidx;
    int *meta, *ovf, *und, *stats;
    size_t bytes;
};
static HGenScratch h_gen_layout(void* d_scratch, int hypCount) {
    const size_t piece = (size_t)h_gen_piece(hypCount);
    const size_t oSidx = piece * kEigLogCap * sizeof(EigRot), oMeta = oSidx + piece * sizeof(int4);
    const size_t oOvf = oMeta + piece * sizeof(int), oUnd = oOvf + ((size_t)hypCount + 1) * sizeof(int);
    const size_t oStats = oUnd + (piece + 1) * sizeof(int);
    HGenScratch L{};
    L.bytes = oStats + 2 * sizeof(int);
    if (!d_scratch) return L;   // the size alone
    char* b = (char*)d_scratch;
    L.log = (EigRot*)b;
    L.sidx = (int4*)(b + oSidx);
    L.meta = (int*)(b + oMeta);
    L.ovf = (int*)(b + oOvf);
    L.und = (int*)(b + oUnd);
    L.stats = (int*)(b + oStats);
    return L;
}

size_t h_gen_scratch_bytes(int hypCount) { return h_gen_layout(nullptr, hypCount).bytes; }

// mcvTestHGenRow's second switch: err times 2^40, so that no lane is decided (tests drive the fallback)
static double g_hrow_err_scale = 1.0;
void h_gen_row_err_scale(bool huge) { g_hrow_err_scale = huge ? 0x1p40 : 1.0; }
static constexpr int kHGenVListBlocks = 1024;

void launch_h_generate(const float* d_pts4, int N, Sampler smp, int64_t hypBegin, int hypCount, void* d_models,
                       double* d_h64, int* d_counts, hipStream_t s, bool fast, void* d_scratch, bool certifiedRow) {
    if (fast) {
        hipLaunchKernelGGL(mcv_h_generate<true>, dim3((hypCount + 255) / 256), dim3(256), 0, s, d_pts4, N, smp, hypBegin,
                           hypCount, (HModelF*)d_models, d_h64, d_counts);
        return;
    }
    if (!d_scratch) {   // the one-pass solve: kEigLanes per block, one wave per SIMD (jacobi_eig.h)
        hipLaunchKernelGGL((mcv_h_generate<false, kEigLanes>), dim3((hypCount + kEigLanes - 1) / kEigLanes),
                           dim3(kEigLanes), 0, s, d_pts4, N, smp, hypBegin, hypCount, (HModelF*)d_models, d_h64,
                           d_counts);
        return;
    }
    const int piece = h_gen_piece(hypCount);
    const HGenScratch L = h_gen_layout(d_scratch, hypCount);
    (void)hipMemsetAsync(L.ovf, 0, sizeof(int), s);   // errors surface at the caller's hipGetLastError
    if (certifiedRow) (void)hipMemsetAsync(L.stats, 0, 2 * sizeof(int), s);
    for (int base = 0; base < hypCount; base += piece) {
        const int cnt = std::min(piece, hypCount - base);
        hipLaunchKernelGGL(mcv_h_gen_aw<kHGenAwLanes>, dim3((cnt + kHGenAwLanes - 1) / kHGenAwLanes),
                           dim3(kHGenAwLanes), 0, s, d_pts4, N, smp, hypBegin, cnt, (HModelF*)d_models, d_counts,
                           L.sidx, L.meta, L.log, piece, L.ovf, base, g_eig_log_cap);
        if (certifiedRow) {
            (void)hipMemsetAsync(L.und, 0, sizeof(int), s);
            hipLaunchKernelGGL(mcv_h_gen_r, dim3((cnt + 63) / 64), dim3(64), 0, s, d_pts4, cnt, base, L.sidx, L.meta,
                               L.log, piece, (HModelF*)d_models, d_counts, L.und, L.stats, g_hrow_err_scale);
            hipLaunchKernelGGL((mcv_h_gen_v_list<kHGenVG, kHGenVQ, kHGenVD, true>), dim3(kHGenVListBlocks),
                               dim3(kHGenVG * kHGenVQ), 0, s, d_pts4, cnt, base, L.sidx, L.meta, L.log, piece,
                               (HModelF*)d_models, d_h64, d_counts, L.und, -1);
        } else {
            hipLaunchKernelGGL((mcv_h_gen_v<kHGenVG, kHGenVQ, kHGenVD>), dim3((cnt + kHGenVQ - 1) / kHGenVQ),
                               dim3(kHGenVG * kHGenVQ), 0, s, d_pts4, cnt, base, L.sidx, L.meta, L.log, piece,
                               (HModelF*)d_models, d_h64, d_counts);
        }
    }
    hipLaunchKernelGGL(mcv_h_gen_ovf<kEigLanes>, dim3(kHGenOvfBlocks), dim3(kEigLanes), 0, s, d_pts4, N, smp, hypBegin,
                       L.ovf, (HModelF*)d_models, d_h64, d_counts);
}

bool h_gen_row_log_kept(int hypCount) { return hypCount <= h_gen_piece(hypCount); }

void launch_h_gen_v_one(const float* d_pts4, int hypCount, int local, void* d_scratch, void* d_models, double* d_h64,
                        hipStream_t s) {
    const HGenScratch L = h_gen_layout(d_scratch, hypCount);
    hipLaunchKernelGGL((mcv_h_gen_v_list<kHGenVG, kHGenVQ, kHGenVD, false>), dim3(1), dim3(kHGenVG * kHGenVQ), 0, s,
                       d_pts4, hypCount, 0, L.sidx, L.meta, L.log, h_gen_piece(hypCount), (HModelF*)d_models, d_h64,
                       nullptr, nullptr, local);
}

const int* h_gen_row_stats(const void* d_scratch, int hypCount) {
    return h_gen_layout(const_cast<void*>(d_scratch), hypCount).stats;
}

void launch_h_one(const float* d_pts4, int N, Sampler smp, int64_t hyp, HOneOut* d_out, hipStream_t s, bool fast) {
    hipLaunchKernelGGL(mcv_h_one, dim3(1), dim3(64), 0, s, d_pts4, N, smp, hyp, d_out, fast);
}

}  // namespace mcv

// Test hook: the split generate's usable log rows in [0, 192] (lanes needing more go to the one-pass
// overflow kernel); returns the previous value. Not thread-safe: tests only.
extern "C" MCV_API int mcvTestEigLogCap(int cap) {
    const int prev = mcv::g_eig_log_cap;
    mcv::g_eig_log_cap = cap < 0 ? 0 : cap > mcv::kEigLogCap ? mcv::kEigLogCap : cap;
    return prev;
}
