// scaled_batch.hip — gfx950 kernels of the batched CameraPose.findScaled (cvFindScaledPoseBatch,
// DESIGN §7j): P independent problems (a source camera and a pose each) over S observation sets in
// a fixed number of launches. The arithmetic is hyp_scaled.h's, as in scaled_pose.hip; what is new
// is the addressing: a problem's rows, candidates and blocks are slices (scaled_batch_index.h) of
// arrays that hold every problem's, and its ScaledSetup is element p of an array.
//
//   mcv_scaled_batch_pack        every set's AoS rows -> SoA fp64 (5 streams of R rows), once per set
//   mcv_scaled_batch_candidates  lane per candidate of a (problem, block): the observation's scales
//   mcv_scaled_batch_costs       the sweep: a workgroup owns one block of 64 candidates of one problem;
//                                8 waves project LDS-staged tiles of 32 observations of the problem's
//                                set while a ninth adds the previous tile's terms to each candidate's
//                                running sum in list order (mcv_scaled_costs' structure and fold)
//   mcv_scaled_batch_best        per problem: min (cost bits, index) over the finite costs, the
//                                evaluated count, and the winner's cost and scale gathered
//
// Every clamp stays inside the problem: a block's idle lanes take the problem's own last candidate,
// a tile's tail the set's own last row.
#include "hyp_scaled.h"
#include "kernels.h"
#include "plan.h"
#include "scaled_batch_index.h"

namespace mcv {

__global__ __launch_bounds__(256) void mcv_scaled_batch_pack(const double* __restrict__ w3,
                                                             const double* __restrict__ o2, int R,
                                                             double* __restrict__ soa) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R) return;
    soa[i] = w3[3 * (size_t)i];
    soa[(size_t)R + i] = w3[3 * (size_t)i + 1];
    soa[2 * (size_t)R + i] = w3[3 * (size_t)i + 2];
    soa[3 * (size_t)R + i] = o2[2 * (size_t)i];
    soa[4 * (size_t)R + i] = o2[2 * (size_t)i + 1];
}

// A wave per block of the work list, lane l = the block's candidate l (observation l / 2, s.X for even
// l, s.Y for odd l): both lanes of an observation compute the pair and keep their half.
__global__ __launch_bounds__(256) void mcv_scaled_batch_candidates(const ScaledSetup* __restrict__ setups,
                                                                   const ScaledBatchProb* __restrict__ probs,
                                                                   const int* __restrict__ blockProb, int nBlocks,
                                                                   const double* __restrict__ soa, int R,
                                                                   double* __restrict__ scales,
                                                                   uint8_t* __restrict__ used) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (b >= nBlocks) return;
    const int p = blockProb[b];
    const ScaledBatchProb pd = probs[p];
    const int c = (b - pd.blockOff) * kScaledBatchCands + lane;
    if (c >= 2 * pd.N) return;
    const int i = c >> 1;
    const size_t row = (size_t)pd.rowOff + i;
    double sx = __builtin_nan(""), sy = __builtin_nan("");
    const bool ok = scaled_candidate(setups[p], soa[row], soa[(size_t)R + row], soa[2 * (size_t)R + row],
                                     soa[3 * (size_t)R + row], soa[4 * (size_t)R + row], sx, sy);
    scales[(size_t)pd.candOff + c] = ok ? ((c & 1) ? sy : sx) : __builtin_nan("");
    if (!(c & 1)) used[(size_t)(pd.candOff >> 1) + i] = ok ? 1 : 0;
}

// mcv_scaled_costs (scaled_pose.hip) per (problem, block): the same tiles, waves, -0.0 parking and
// list-order fold. The setup is read from setups[p], uniform across the workgroup; the rows are the
// problem's set (soa + rowOff, N of them), the candidates its own 2 N.
static const int kSbTile = 32;
static const int kSbComputeWaves = 8;
static const int kSbThreads = (kSbComputeWaves + 1) * 64;

__global__ __launch_bounds__(kSbThreads) void mcv_scaled_batch_costs(const ScaledSetup* __restrict__ setups,
                                                                     const ScaledBatchProb* __restrict__ probs,
                                                                     const int* __restrict__ blockProb,
                                                                     const double* __restrict__ soa, int R,
                                                                     const double* __restrict__ scales,
                                                                     const uint8_t* __restrict__ used,
                                                                     double* __restrict__ costs) {
    __shared__ double terms[2][kSbTile][kScaledBatchCands];
    __shared__ double obs[2][5][kSbTile];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int p = blockProb[blockIdx.x];
    const ScaledBatchProb pd = probs[p];
    const ScaledSetup S = setups[p];
    const int N = pd.N, nCand = 2 * N;
    const int c = ((int)blockIdx.x - pd.blockOff) * kScaledBatchCands + lane;
    const int cc = c < nCand ? c : nCand - 1;   // idle lanes: the problem's own last candidate
    double loc[3];
    scaled_location(S, scales[(size_t)pd.candOff + cc], loc);
    const int per = kSbTile / kSbComputeWaves;   // observations per compute wave and tile
    const int sw = kSbComputeWaves;               // the staging / summing wave
    const int ntiles = (N + kSbTile - 1) / kSbTile;
    const double* __restrict__ rows = soa + pd.rowOff;
    // the summing wave stages tile t's observations (5 SoA streams) into obs[t % 2]; past N: the set's last one
    auto stage = [&](int t) {
        if (lane < kSbTile) {
            const int j0 = t * kSbTile + lane;
            const int j = j0 < N ? j0 : N - 1;
#pragma unroll
            for (int q = 0; q < 5; ++q) obs[t & 1][q][lane] = rows[(size_t)q * R + j];
        }
    };
    if (wv == sw) stage(0);
    __syncthreads();
    double sum = 0.0;
    int cnt = 0;
    for (int t = 0; t <= ntiles; ++t) {
        if (wv < sw && t < ntiles) {
            double (*buf)[kScaledBatchCands] = terms[t & 1];
            const double (*o)[kSbTile] = obs[t & 1];
            const int r0 = wv * per;
            const int j0 = t * kSbTile + r0;
#pragma unroll 4
            for (int k = 0; k < per; ++k) {
                double e;
                const bool vis = scaled_term(S, loc, o[0][r0 + k], o[1][r0 + k], o[2][r0 + k], o[3][r0 + k],
                                             o[4][r0 + k], e);
                buf[r0 + k][lane] = (vis && j0 + k < N) ? e : -0.0;
            }
        }
        if (wv == sw) {
            if (t + 1 < ntiles) stage(t + 1);
            if (t > 0) {
                const double (*buf)[kScaledBatchCands] = terms[(t - 1) & 1];
#pragma unroll 8
                for (int k = 0; k < kSbTile; ++k) {
                    const double d = buf[k][lane];
                    sum = sum + d;
                    cnt += __double_as_longlong(d) != (long long)0x8000000000000000ull ? 1 : 0;
                }
            }
        }
        __syncthreads();
    }
    if (wv == sw && c < nCand)
        costs[(size_t)pd.candOff + c] =
            (!used[(size_t)(pd.candOff >> 1) + (c >> 1)] || cnt == 0) ? __builtin_inf() : sum / (double)cnt;
}

// A workgroup per problem (grid-stride over the problems): mcv_scaled_best's choice, the first strictly
// smaller cost in candidate order, as the minimum of (cost bits, index) over the finite costs of used
// observations. res: cost[P], scale[P], then evaluated[P] as 64-bit integers; an empty problem and
// one without a finite cost get +inf, 0.0.
static const int kSbBestThreads = 256;

__global__ __launch_bounds__(kSbBestThreads) void mcv_scaled_batch_best(const ScaledBatchProb* __restrict__ probs,
                                                                        int P, const double* __restrict__ costs,
                                                                        const double* __restrict__ scales,
                                                                        const uint8_t* __restrict__ used,
                                                                        double* __restrict__ res) {
    __shared__ unsigned long long sb[kSbBestThreads / 64];
    __shared__ int si[kSbBestThreads / 64], sn[kSbBestThreads / 64];
    const unsigned long long kInfBits = 0x7FF0000000000000ull;
    long long* __restrict__ evaluated = reinterpret_cast<long long*>(res + 2 * (size_t)P);
    for (int p = blockIdx.x; p < P; p += gridDim.x) {
        const ScaledBatchProb pd = probs[p];
        const int nCand = 2 * pd.N;
        const double* __restrict__ pc = costs + pd.candOff;
        const uint8_t* __restrict__ pu = used + (pd.candOff >> 1);
        unsigned long long best = ~0ull;
        int bi = -1, n = 0;
        for (int c = threadIdx.x; c < nCand; c += kSbBestThreads) {
            const bool u = pu[c >> 1] != 0;
            if (u) ++n;
            const unsigned long long b = (unsigned long long)__double_as_longlong(pc[c]);
            // finite, non-negative costs only (+inf never wins: strict <; NaN never compares smaller)
            if (u && b < kInfBits && (b < best || (b == best && c < bi))) {
                best = b;
                bi = c;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned long long ob = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            n += __shfl_xor(n, off, 64);
            if (oi >= 0 && (ob < best || (ob == best && (bi < 0 || oi < bi)))) {
                best = ob;
                bi = oi;
            }
        }
        const int w = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) {
            sb[w] = best;
            si[w] = bi;
            sn[w] = n;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int k = 1; k < kSbBestThreads / 64; ++k) {
                n += sn[k];
                if (si[k] >= 0 && (sb[k] < best || (sb[k] == best && (bi < 0 || si[k] < bi)))) {
                    best = sb[k];
                    bi = si[k];
                }
            }
            res[p] = bi >= 0 ? pc[bi] : __builtin_inf();
            res[(size_t)P + p] = bi >= 0 ? scales[(size_t)pd.candOff + bi] : 0.0;
            evaluated[p] = n;
        }
        __syncthreads();   // the partials are reused by the next problem
    }
}

void launch_scaled_batch_pack(const double* d_w3, const double* d_o2, int R, double* d_soa, hipStream_t s) {
    hipLaunchKernelGGL(mcv_scaled_batch_pack, dim3((R + 255) / 256), dim3(256), 0, s, d_w3, d_o2, R, d_soa);
}

void launch_scaled_batch_candidates(const ScaledSetup* d_setups, const ScaledBatchProb* d_probs,
                                    const int* d_blockProb, int nBlocks, const double* d_soa, int R,
                                    double* d_scales, uint8_t* d_used, hipStream_t s) {
    hipLaunchKernelGGL(mcv_scaled_batch_candidates, dim3((nBlocks + 3) / 4), dim3(256), 0, s, d_setups, d_probs,
                       d_blockProb, nBlocks, d_soa, R, d_scales, d_used);
}

void launch_scaled_batch_costs(const ScaledSetup* d_setups, const ScaledBatchProb* d_probs, const int* d_blockProb,
                               int nBlocks, const double* d_soa, int R, const double* d_scales,
                               const uint8_t* d_used, double* d_costs, hipStream_t s) {
    ProfScope ps("scaled_batch_costs", s);
    hipLaunchKernelGGL(mcv_scaled_batch_costs, dim3(nBlocks), dim3(kSbThreads), 0, s, d_setups, d_probs,
                       d_blockProb, d_soa, R, d_scales, d_used, d_costs);
}

void launch_scaled_batch_best(const ScaledBatchProb* d_probs, int P, const double* d_costs, const double* d_scales,
                              const uint8_t* d_used, double* d_res, hipStream_t s) {
    const int grid = P < 65536 ? P : 65536;
    hipLaunchKernelGGL(mcv_scaled_batch_best, dim3(grid), dim3(kSbBestThreads), 0, s, d_probs, P, d_costs,
                       d_scales, d_used, d_res);
}

}  // namespace mcv
