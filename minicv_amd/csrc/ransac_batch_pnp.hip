// ransac_batch_pnp.hip — gfx950 kernels of cvSolvePnPRansacBatch that have no single-call form: the inlier
// sweep over many problems' poses, the copy of a round's winning poses, the winners' masks.
// The generate, the LM sums and the inlier EPnP passes are the batch forms of the single call's kernels and
// live beside them (ransac_pnp.hip). All problems' PnpPoint rows sit in one segmented buffer.
//
//   mcv_batch_pnp_sweep  the hot kernel. A workgroup of kBatchPnpWidth = 64 lanes (one wave) belongs to one
//                        problem; each LANE holds one pose (12 doubles) and its problem's camera in registers;
//                        one tile of kBatchPnpTile = 512 PnpPoint rows (16 KiB) is staged in LDS and every lane
//                        walks it on the same address (an LDS broadcast). Grid: x = (64-pose group, problem),
//                        y = the tile of the problem's points. The default budget is 100 hypotheses a problem,
//                        so a 256-lane workgroup would idle 156 lanes; 64 lanes idle 28 of 128, and the split of
//                        the points over y gives a problem of N points 2 ceil(N / 512) waves instead of 2. The
//                        partial counts of the tiles are added with integer atomics: exact in any order.
//                        A count is the number of points with pnp_error(cam, R, t, ..., false) <= thr2, the
//                        defining function (NaN: never); no prefilter, no certificate.
//   mcv_batch_pnp_fetch  best[out] = models[slot] for the problems whose best changed in a round.
//   mcv_batch_pnp_mask   mcv_pnp_mask's test for every winner in one launch.
#include "mcv_common.h"
#include "hyp_pnp.h"
#include "kernels.h"

namespace mcv {

static __device__ __forceinline__ PnpCamera batch_pnp_cam(const double* __restrict__ cam8) {
    PnpCamera c;
    c.fx = cam8[0]; c.fy = cam8[1]; c.cx = cam8[2]; c.cy = cam8[3];
    c.k1 = cam8[4]; c.k2 = cam8[5]; c.p1 = cam8[6]; c.p2 = cam8[7];
    return c;
}

__global__ __launch_bounds__(kBatchPnpWidth) void mcv_batch_pnp_sweep(const PnpPoint* __restrict__ pts,
                                                                      const BatchPnpDesc* __restrict__ desc,
                                                                      int blocksPer, const double* __restrict__ cams,
                                                                      const PnpPose* __restrict__ models,
                                                                      int* __restrict__ counts, float thr2) {
    __shared__ float4 tile[2 * kBatchPnpTile];
    const BatchPnpDesc D = desc[blockIdx.x / blocksPer];
    const int i0 = (blockIdx.x % blocksPer) * kBatchPnpWidth;
    const int base = blockIdx.y * kBatchPnpTile;
    if (i0 >= D.d.hypCount || base >= D.d.N) return;   // uniform over the workgroup
    const int i = i0 + threadIdx.x;
    const bool mine = i < D.d.hypCount;
    // lanes past the problem's hypotheses re-read its last slot and write nothing
    const int64_t slot = D.d.slotOff + (mine ? i : D.d.hypCount - 1);
    const bool valid = mine && counts[slot] >= 0;   // other tiles only add to a non-negative count
    const PnpCamera cam = batch_pnp_cam(cams + 8 * (size_t)D.cam);
    double R[9], t[3];
    if (valid) {
        const PnpPose m = models[slot];
#pragma unroll
        for (int j = 0; j < 9; ++j) R[j] = m.R[j];
#pragma unroll
        for (int j = 0; j < 3; ++j) t[j] = m.t[j];
    } else {   // a slot without a model holds no pose (its buffer entry was never written)
#pragma unroll
        for (int j = 0; j < 9; ++j) R[j] = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) t[j] = 0.0;
    }
    const int n = min(kBatchPnpTile, D.d.N - base);
    const float4* p = reinterpret_cast<const float4*>(pts + D.d.ptOff + base);
    for (int j = threadIdx.x; j < 2 * n; j += kBatchPnpWidth) tile[j] = p[j];
    __syncthreads();
    int cnt = 0;
    for (int j = 0; j < n; ++j) {
        const float4 a = tile[2 * j], b = tile[2 * j + 1];   // {X, Y, Z, u}, {v, pad, pad, pad}
        cnt += pnp_error(cam, R, t, a.x, a.y, a.z, a.w, b.x, false) <= thr2 ? 1 : 0;
    }
    if (valid && cnt) atomicAdd(counts + slot, cnt);
}

__global__ __launch_bounds__(64) void mcv_batch_pnp_fetch(const BatchPnpFetch* __restrict__ fetch, int nFetch,
                                                          const PnpPose* __restrict__ models,
                                                          PnpPose* __restrict__ best) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= nFetch) return;
    const BatchPnpFetch F = fetch[f];
    best[F.out] = models[F.slot];
}

// Grid: blocksPer x nFin blocks of 256; block b of winner f masks its points [256 b, 256 b + 256).
__global__ __launch_bounds__(256) void mcv_batch_pnp_mask(const PnpPoint* __restrict__ pts,
                                                          const BatchPnpFin* __restrict__ fin, int blocksPer,
                                                          const double* __restrict__ cams,
                                                          const PnpPose* __restrict__ best, float thr2,
                                                          uint8_t* __restrict__ mask, int* __restrict__ count) {
    const int f = blockIdx.x / blocksPer;
    const BatchPnpFin D = fin[f];
    const int i = (blockIdx.x % blocksPer) * 256 + threadIdx.x;
    if ((blockIdx.x % blocksPer) * 256 >= D.N) return;   // uniform over the workgroup
    const PnpCamera cam = batch_pnp_cam(cams + 8 * (size_t)D.cam);
    const PnpPose m = best[D.pose];
    bool in = false;
    if (i < D.N) {
        const PnpPoint q = pts[D.ptOff + i];
        in = pnp_error(cam, m.R, m.t, q.X, q.Y, q.Z, q.u, q.v, false) <= thr2;
        mask[D.ptOff + i] = in ? 1 : 0;
    }
    const uint64_t b = __ballot(in);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(count + f, (int)__popcll(b));
}

void launch_batch_pnp_sweep(const void* d_pts, const BatchPnpDesc* d_desc, int nDesc, int maxHyp, int maxN,
                            const double* d_cams, const void* d_models, int* d_counts, float thr2, hipStream_t s) {
    const int per = (maxHyp + kBatchPnpWidth - 1) / kBatchPnpWidth;
    const int tiles = (maxN + kBatchPnpTile - 1) / kBatchPnpTile;
    if (per <= 0 || tiles <= 0 || nDesc <= 0) return;
    // grid y is limited to 65535 tiles = 33.5 M points a problem; the host refuses more (an int offset buffer
    // cannot hold 64 such problems anyway)
    hipLaunchKernelGGL(mcv_batch_pnp_sweep, dim3((unsigned)per * nDesc, (unsigned)tiles), dim3(kBatchPnpWidth), 0, s,
                       (const PnpPoint*)d_pts, d_desc, per, d_cams, (const PnpPose*)d_models, d_counts, thr2);
}

void launch_batch_pnp_fetch(const BatchPnpFetch* d_fetch, int nFetch, const void* d_models, void* d_best,
                            hipStream_t s) {
    if (nFetch <= 0) return;
    hipLaunchKernelGGL(mcv_batch_pnp_fetch, dim3((nFetch + 63) / 64), dim3(64), 0, s, d_fetch, nFetch,
                       (const PnpPose*)d_models, (PnpPose*)d_best);
}

void launch_batch_pnp_mask(const void* d_pts, const BatchPnpFin* d_fin, int nFin, int maxN, const double* d_cams,
                           const void* d_best, float thr2, uint8_t* d_mask, int* d_count, hipStream_t s) {
    const int per = (maxN + 255) / 256;
    if (per <= 0 || nFin <= 0) return;
    hipLaunchKernelGGL(mcv_batch_pnp_mask, dim3((unsigned)per * nFin), dim3(256), 0, s, (const PnpPoint*)d_pts, d_fin,
                       per, d_cams, (const PnpPose*)d_best, thr2, d_mask, d_count);
}

}  // namespace mcv
