// ransac_batch_e.hip — gfx950 kernels of cvFindEssentialMatBatch / cvRecoverPoseBatch: B independent
// essential-matrix RANSAC problems in launches whose number does not depend on B. All
// problems' double4 normalised correspondences sit in one segmented buffer; every kernel indexes the grid
// as (block within problem, problem). The generate is the single call's own three kernels in their batch
// form (ransac_e5.hip: mcv_e5_coeffs<true>, mcv_e5_lu, mcv_e5_roots<true>); this file holds the rest.
//
//   mcv_batch_e_pack        (x - pp) / focal in fp64 with each problem's focal and principal point:
//                           mcv_e_pack's operations.
//   mcv_batch_e_sweep<KIND> the inlier sweep, transposed against mcv_e_verify in the manner of
//                           mcv_batch_sweep: a workgroup of 256 lanes belongs to one problem, each lane holds
//                           one model of the problem's dense region in registers (9 doubles), the problem's
//                           points are staged through LDS in tiles of kBatchETile double4 (16 KiB) and every
//                           lane walks the tile reading the same address (an LDS broadcast) and counts in a
//                           register: no ballot, no atomics. The error is f_error itself, so a count is by
//                           construction the number of points with error <= thr2 (NaN: never), which is what
//                           the single call's certified sweep produces.
//   mcv_batch_e_fetch       the round's new best models out of the dense regions (slot -> model), as
//                           mcv_e_fetch does for the single call.
//   mcv_batch_e_mask        every winner's inlier mask and count (mcv_e_mask's test) in one launch.
//   mcv_batch_e_cheirality  recoverPose's cheirality counts of every winner's four candidates in one launch:
//                           one lane per (correspondence, candidate), masked points only (mcv_e_cheirality).
#include "mcv_common.h"
#include "hyp_essential.h"
#include "hyp_fundamental.h"
#include "kernels.h"

namespace mcv {

// Grid: blocksPer x nPack blocks of 256; block b of problem f packs points [256 b, 256 b + 256).
__global__ __launch_bounds__(256) void mcv_batch_e_pack(const double2* __restrict__ a, const double2* __restrict__ b,
                                                        const BatchEPack* __restrict__ desc, int blocksPer,
                                                        double4* __restrict__ out) {
    const BatchEPack D = desc[blockIdx.x / blocksPer];
    const int i = (blockIdx.x % blocksPer) * 256 + threadIdx.x;
    if (i >= D.N) return;
    const double2 p = a[D.ptOff + i], q = b[D.ptOff + i];
    double4 o;
    o.x = (p.x - D.cx) / D.focal;
    o.y = (p.y - D.cy) / D.focal;
    o.z = (q.x - D.cx) / D.focal;
    o.w = (q.y - D.cy) / D.focal;
    out[D.ptOff + i] = o;
}

// Grid: blocksPer x nDesc blocks of 256. kBatchETile double4 points = 16 KiB of LDS per workgroup, the
// budget of mcv_batch_sweep's float4 tile: eight workgroups per CU take 128 of the 160 KiB.
template <int KIND>
__global__ __launch_bounds__(256) void mcv_batch_e_sweep(const double4* __restrict__ pts,
                                                         const BatchESweep* __restrict__ desc, int blocksPer,
                                                         const EModel* __restrict__ dense,
                                                         const int* __restrict__ denseSlot,
                                                         const int* __restrict__ nDense, int* __restrict__ counts) {
    __shared__ double4 tile[kBatchETile];
    const int prob = blockIdx.x / blocksPer;
    const BatchESweep D = desc[prob];
    const int total = nDense[prob];
    const int i0 = (blockIdx.x % blocksPer) * 256;
    if (i0 >= total) return;   // uniform over the workgroup
    const int i = i0 + threadIdx.x;
    const bool mine = i < total;
    // lanes past the problem's dense count re-read its last model and write nothing
    const int64_t at = D.denseOff + (mine ? i : total - 1);
    const EModel m = dense[at];
    const double4* p = pts + D.ptOff;
    const float thr2 = D.thr2;
    int cnt = 0;
    for (int base = 0; base < D.N; base += kBatchETile) {
        const int n = min(kBatchETile, D.N - base);
        if (base) __syncthreads();   // the previous tile has been read by every lane
        for (int j = threadIdx.x; j < n; j += 256) tile[j] = p[base + j];
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const double4 q = tile[j];
            cnt += f_error(KIND, m.e, q.x, q.y, q.z, q.w) <= thr2 ? 1 : 0;
        }
    }
    if (mine) counts[D.countOff + (denseSlot ? denseSlot[at] : i)] = cnt;
}

// One workgroup per entry: the model of slot `slot` of its problem's dense region -> out[outIdx].
__global__ __launch_bounds__(256) void mcv_batch_e_fetch(const BatchEFetch* __restrict__ fetch,
                                                         const EModel* __restrict__ dense,
                                                         const int* __restrict__ denseSlot,
                                                         const int* __restrict__ nDense, EModel* __restrict__ out,
                                                         int* __restrict__ found) {
    const BatchEFetch D = fetch[blockIdx.x];
    const int total = nDense[D.prob];
    for (int i = threadIdx.x; i < total; i += 256) {
        if (denseSlot[D.denseOff + i] == D.slot) {
            out[D.outIdx] = dense[D.denseOff + i];
            found[D.outIdx] = D.stamp;
        }
    }
}

// Grid: blocksPer x nFin blocks of 256; block b of winner f masks points [256 b, 256 b + 256).
__global__ __launch_bounds__(256) void mcv_batch_e_mask(const double4* __restrict__ pts,
                                                        const BatchEFin* __restrict__ fin, int blocksPer,
                                                        const EModel* __restrict__ models, int kind,
                                                        uint8_t* __restrict__ mask, int* __restrict__ count) {
    const int f = blockIdx.x / blocksPer;
    const BatchEFin D = fin[f];
    const int i = (blockIdx.x % blocksPer) * 256 + threadIdx.x;
    if ((blockIdx.x % blocksPer) * 256 >= D.N) return;   // uniform over the workgroup
    const EModel m = models[D.modelIdx];
    bool in = false;
    if (i < D.N) {
        const double4 q = pts[D.ptOff + i];
        in = f_error(kind, m.e, q.x, q.y, q.z, q.w) <= D.thr2;
        mask[D.ptOff + i] = in ? 1 : 0;
    }
    const uint64_t b = __ballot(in);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(count + f, (int)__popcll(b));
}

// Grid: blocksPer x nPose blocks of 256; lane t of problem f tests correspondence t / 4 with candidate t % 4.
__global__ __launch_bounds__(256) void mcv_batch_e_cheirality(const double4* __restrict__ pts,
                                                              const uint8_t* __restrict__ mask,
                                                              const BatchEPose* __restrict__ pose, int blocksPer,
                                                              double dist, int* __restrict__ good4) {
    const int f = blockIdx.x / blocksPer;
    const int ptOff = pose[f].ptOff, N = pose[f].N;
    const int t = (blockIdx.x % blocksPer) * 256 + threadIdx.x;
    if ((blockIdx.x % blocksPer) * 64 >= N) return;   // uniform over the workgroup
    const int i = t >> 2, k = t & 3;
    const bool act = i < N && mask[ptOff + i];
    double4 q = {0, 0, 0, 0};
    if (act) q = pts[ptOff + i];
    double P[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) P[j] = pose[f].P[k][j];
    const bool g = e_cheirality(P, q.x, q.y, q.z, q.w, dist) && act;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const uint64_t b = __ballot(g && k == kk);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(good4 + 4 * f + kk, (int)__popcll(b));
    }
}

// ---- launchers ---------------------------------------------------------------------------------
void launch_batch_e_pack(const double* d_a, const double* d_b, const BatchEPack* d_desc, int nDesc, int maxN,
                         double* d_pts4, hipStream_t s) {
    if (nDesc <= 0 || maxN <= 0) return;
    const int per = (maxN + 255) / 256;
    hipLaunchKernelGGL(mcv_batch_e_pack, dim3((unsigned)per * nDesc), dim3(256), 0, s, (const double2*)d_a,
                       (const double2*)d_b, d_desc, per, (double4*)d_pts4);
}

void launch_batch_e_sweep(int kind, const double* d_pts4, const BatchESweep* d_desc, int nDesc, int maxModels,
                          const void* d_dense, const int* d_denseSlot, const int* d_nDense, int* d_counts,
                          hipStream_t s) {
    if (nDesc <= 0 || maxModels <= 0) return;
    const int per = (maxModels + 255) / 256;
    const dim3 g((unsigned)per * nDesc);
    if (kind == 0)
        hipLaunchKernelGGL(mcv_batch_e_sweep<0>, g, dim3(256), 0, s, (const double4*)d_pts4, d_desc, per,
                           (const EModel*)d_dense, d_denseSlot, d_nDense, d_counts);
    else
        hipLaunchKernelGGL(mcv_batch_e_sweep<1>, g, dim3(256), 0, s, (const double4*)d_pts4, d_desc, per,
                           (const EModel*)d_dense, d_denseSlot, d_nDense, d_counts);
}

void launch_batch_e_fetch(const BatchEFetch* d_fetch, int nFetch, const void* d_dense, const int* d_denseSlot,
                          const int* d_nDense, double* d_out9, int* d_found, hipStream_t s) {
    if (nFetch <= 0) return;
    hipLaunchKernelGGL(mcv_batch_e_fetch, dim3(nFetch), dim3(256), 0, s, d_fetch, (const EModel*)d_dense, d_denseSlot,
                       d_nDense, (EModel*)d_out9, d_found);
}

void launch_batch_e_mask(int kind, const double* d_pts4, const BatchEFin* d_fin, int nFin, int maxN,
                         const double* d_models9, uint8_t* d_mask, int* d_count, hipStream_t s) {
    if (nFin <= 0 || maxN <= 0) return;
    const int per = (maxN + 255) / 256;
    hipLaunchKernelGGL(mcv_batch_e_mask, dim3((unsigned)per * nFin), dim3(256), 0, s, (const double4*)d_pts4, d_fin,
                       per, (const EModel*)d_models9, kind, d_mask, d_count);
}

void launch_batch_e_cheirality(const double* d_pts4, const uint8_t* d_mask, const BatchEPose* d_pose, int nPose,
                               int maxN, double dist, int* d_good4, hipStream_t s) {
    if (nPose <= 0 || maxN <= 0) return;
    const int per = (int)((4 * (int64_t)maxN + 255) / 256);
    hipLaunchKernelGGL(mcv_batch_e_cheirality, dim3((unsigned)per * nPose), dim3(256), 0, s, (const double4*)d_pts4,
                       d_mask, d_pose, per, dist, d_good4);
}

}  // namespace mcv
