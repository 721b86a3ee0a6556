// triangulate.hip — gfx950 kernels of track triangulation: Ray.intersection (Utilities.fs:100-165)
// for many tracks in one call, over a CSR of rays (hyp_rays.h arithmetic, fp64, bit for bit).
//
//   mcv_tri_check_offsets / mcv_tri_check_cameras   the device export's argument checks
//   mcv_tri_unproject   lane per observation: Camera.unproject1 into the ray buffer (48 B each)
//   mcv_tri_short       lane per track of at most kTriShortMax rays: dedupe mask in a register, the
//                       i < j pair loop re-reading rays from L1/L2 (no per-lane ray array), the
//                       ordered fold in registers; longer tracks are queued for mcv_tri_long
//   mcv_tri_long        workgroup per queued track: dedupe flags across the threads, compaction by
//                       one wave, the first kTriLdsRays kept rays in LDS (the rest stream from L2),
//                       pair tiles in flattened lexicographic order computed by two waves and parked
//                       in LDS while a third wave adds the previous tile to the single ordered chain
//   mcv_tri_stats       lane per track: cost / visible over the track's observations in input order
//
// The fold order is the contract (one sequential chain per track, Utilities.fs:164), so there is no
// tree reduction anywhere: a rejected pair parks -0.0, which leaves any running sum unchanged (the
// chain starts at +0.0 and can never become -0.0), and the pair count is summed apart, as integers.
#include "minicv_native.h"
#include "hyp_rays.h"
#include "kernels.h"
#include "plan.h"

namespace mcv {

static const int kTriLdsRays = 256;     // kept rays of a long track held in LDS (12 KiB)
static const int kTriTile = 128;        // pairs per tile: one per thread of the two compute waves
static const int kTriLongThreads = 192; // two compute waves + the adding wave
static_assert(kTriShortMax <= 32, "the short kernel keeps its dedupe flags in one 32-bit mask");
static_assert(MCV_MAX_TRACK_LEN <= 65536, "kept indices are stored as 16-bit");

__global__ __launch_bounds__(256) void mcv_tri_check_offsets(const int* __restrict__ offsets, int T,
                                                             unsigned int* __restrict__ ctr) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    int kind = 0;
    if (t == 0 && offsets[0] != 0) kind = 1;
    else if (offsets[t + 1] < offsets[t]) kind = 2;
    else if (offsets[t + 1] - offsets[t] > MCV_MAX_TRACK_LEN) kind = 3;
    // first bad track: max of (T - t), so the smallest t wins; its kind is read back from the offsets
    if (kind) atomicMax(&ctr[2], (unsigned int)(T - t));
}

// Runs after mcv_tri_check_offsets on the same stream: with bad offsets offsets[T] means nothing.
__global__ __launch_bounds__(256) void mcv_tri_check_cameras(const int* __restrict__ offsets, int T,
                                                             const int* __restrict__ cameraIdx, int nCameras,
                                                             unsigned int* __restrict__ ctr) {
    if (ctr[2] != 0) return;
    const int n = offsets[T];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
        if (cameraIdx[i] < 0 || cameraIdx[i] >= nCameras) atomicMax(&ctr[4], (unsigned int)(n - i));
}

__global__ __launch_bounds__(256) void mcv_tri_unproject(const double* __restrict__ cameras,
                                                         const int* __restrict__ cameraIdx,
                                                         const double* __restrict__ obs,
                                                         const int* __restrict__ offsets, int T,
                                                         double* __restrict__ rays) {
    const int n = offsets[T];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        double r[6];
        ray_unproject(cameras + 14 * (size_t)cameraIdx[i], obs[2 * (size_t)i], obs[2 * (size_t)i + 1], r);
#pragma unroll
        for (int k = 0; k < 6; ++k) rays[6 * (size_t)i + k] = r[k];
    }
}

__device__ __forceinline__ void tri_load(const double* __restrict__ p, double (&r)[6]) {
#pragma unroll
    for (int k = 0; k < 6; ++k) r[k] = p[k];
}

__global__ __launch_bounds__(256) void mcv_tri_short(const double* __restrict__ rays, const int* __restrict__ offsets,
                                                     int T, double* __restrict__ points,
                                                     int* __restrict__ pairCounts, int* __restrict__ longList,
                                                     unsigned int* __restrict__ ctr) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    bool has = false;
    if (t < T) {
        const int o0 = offsets[t], R = offsets[t + 1] - o0;
        if (R > kTriShortMax) {
            longList[atomicAdd(&ctr[0], 1u)] = t;
        } else {
            const double* tr = rays + 6 * (size_t)o0;
            double a[6], b[6];
            unsigned int keep = 0;   // bit j: ray j is the first of its value
            for (int j = 0; j < R; ++j) {
                tri_load(tr + 6 * j, b);
                bool dup = false;
                for (int i = 0; i < j; ++i) {
                    if (tr[6 * i + 3] != b[3]) continue;   // one load settles nearly every comparison
                    tri_load(tr + 6 * i, a);
                    dup = dup || ray_equal(a, b);
                }
                keep |= dup ? 0u : 1u << j;
            }
            int c = 0;
            double s0 = 0.0, s1 = 0.0, s2 = 0.0;
            for (int i = 0; i < R; ++i) {
                if (!(keep >> i & 1u)) continue;
                tri_load(tr + 6 * i, a);
                for (int j = i + 1; j < R; ++j) {
                    if (!(keep >> j & 1u)) continue;
                    tri_load(tr + 6 * j, b);
                    double pt[3];
                    if (ray_pair(a, b, pt) == kRayPairOk) {
                        c += 1;
                        s0 = s0 + pt[0];
                        s1 = s1 + pt[1];
                        s2 = s2 + pt[2];
                    }
                }
            }
            const double nan = __builtin_nan("");
            points[3 * (size_t)t] = c == 0 ? nan : s0 / (double)c;
            points[3 * (size_t)t + 1] = c == 0 ? nan : s1 / (double)c;
            points[3 * (size_t)t + 2] = c == 0 ? nan : s2 / (double)c;
            pairCounts[t] = c;
            has = c > 0;
        }
    }
    const unsigned long long m = __ballot(has);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&ctr[1], (unsigned int)__popcll(m));
}

// First pair index of row i among K kept rays: pairs (i, i+1) .. (i, K-1) follow those of rows < i.
__device__ __forceinline__ int tri_row_start(int i, int K) { return i * (2 * K - i - 1) / 2; }

__global__ __launch_bounds__(kTriLongThreads) void mcv_tri_long(const double* __restrict__ rays,
                                                                const int* __restrict__ offsets,
                                                                const int* __restrict__ longList,
                                                                double* __restrict__ points,
                                                                int* __restrict__ pairCounts,
                                                                unsigned int* __restrict__ ctr) {
    __shared__ double lr[6][kTriLdsRays];
    __shared__ double terms[2][3][kTriTile];
    __shared__ unsigned short kidx[MCV_MAX_TRACK_LEN];
    __shared__ unsigned char keep[MCV_MAX_TRACK_LEN];
    __shared__ int sK, sCnt;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nLong = (int)ctr[0];
    for (int q = blockIdx.x; q < nLong; q += gridDim.x) {
        const int t = longList[q];
        const int o0 = offsets[t], R = offsets[t + 1] - o0;   // kTriShortMax < R <= MCV_MAX_TRACK_LEN
        const double* tr = rays + 6 * (size_t)o0;
        // 1. dedupe flags: thread per ray, against every earlier ray (L1/L2 broadcast reads)
        for (int j = tid; j < R; j += kTriLongThreads) {
            double a[6], b[6];
            tri_load(tr + 6 * j, b);
            bool dup = false;
            for (int i = 0; i < j && !dup; ++i) {
                if (tr[6 * i + 3] != b[3]) continue;   // one load settles nearly every comparison
                tri_load(tr + 6 * i, a);
                dup = ray_equal(a, b);
            }
            keep[j] = dup ? 0 : 1;
        }
        if (tid == 0) sCnt = 0;
        __syncthreads();
        // 2. compaction, input order kept: one wave, ballot + prefix count per 64 rays
        if (wv == 0) {
            int base = 0;
            for (int c0 = 0; c0 < R; c0 += 64) {
                const int j = c0 + lane;
                const bool k = j < R && keep[j];
                const unsigned long long m = __ballot(k);
                if (k) kidx[base + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)j;
                base += __popcll(m);
            }
            if (lane == 0) sK = base;
        }
        __syncthreads();
        const int K = sK;
        // 3. the first kTriLdsRays kept rays into LDS, component-major
        for (int k = tid; k < K && k < kTriLdsRays; k += kTriLongThreads) {
            const double* p = tr + 6 * (int)kidx[k];
#pragma unroll
            for (int c = 0; c < 6; ++c) lr[c][k] = p[c];
        }
        __syncthreads();
        auto fetch = [&](int k, double (&r)[6]) {
            if (k < kTriLdsRays) {
#pragma unroll
                for (int c = 0; c < 6; ++c) r[c] = lr[c][k];
            } else {
                tri_load(tr + 6 * (int)kidx[k], r);
            }
        };
        // 4. pair tiles in the order of the fold; the adding wave runs one tile behind
        const int nPairs = K * (K - 1) / 2;   // K <= 4096: below 2^23
        const int ntiles = (nPairs + kTriTile - 1) / kTriTile;
        int myc = 0;
        double s = 0.0;   // lanes 0..2 of the adding wave: the running sum of X, Y, Z
        for (int tile = 0; tile <= ntiles; ++tile) {
            if (wv < 2 && tile < ntiles) {
                const int p = tile * kTriTile + tid;
                double pt[3] = {-0.0, -0.0, -0.0};
                if (p < nPairs) {
                    const double w = (double)(2 * K - 1);
                    int i = (int)((w - sqrt(w * w - 8.0 * (double)p)) * 0.5);
                    i = i < 0 ? 0 : (i > K - 2 ? K - 2 : i);
                    while (i < K - 2 && tri_row_start(i + 1, K) <= p) ++i;
                    while (i > 0 && tri_row_start(i, K) > p) --i;
                    const int j = i + 1 + (p - tri_row_start(i, K));
                    double a[6], b[6], m[3];
                    fetch(i, a);
                    fetch(j, b);
                    if (ray_pair(a, b, m) == kRayPairOk) {
                        myc += 1;
                        pt[0] = m[0];
                        pt[1] = m[1];
                        pt[2] = m[2];
                    }
                }
                terms[tile & 1][0][tid] = pt[0];
                terms[tile & 1][1][tid] = pt[1];
                terms[tile & 1][2][tid] = pt[2];
            }
            if (wv == 2 && tile > 0 && lane < 3) {
                const double* d = terms[(tile - 1) & 1][lane];
#pragma unroll 8
                for (int k = 0; k < kTriTile; ++k) s = s + d[k];
            }
            __syncthreads();
        }
        // 5. the count (integers: any order), the point, the outputs
        if (wv < 2 && myc) atomicAdd(&sCnt, myc);
        __syncthreads();
        const int c = sCnt;
        if (wv == 2 && lane < 3) points[3 * (size_t)t + lane] = c == 0 ? __builtin_nan("") : s / (double)c;
        if (tid == 0) {
            pairCounts[t] = c;
            if (c > 0) atomicAdd(&ctr[1], 1u);
        }
        __syncthreads();   // sCnt, keep, kidx, lr are rewritten by the next track
    }
}

__global__ __launch_bounds__(256) void mcv_tri_stats(const double* __restrict__ cameras,
                                                     const int* __restrict__ cameraIdx,
                                                     const double* __restrict__ obs,
                                                     const int* __restrict__ offsets, int T,
                                                     const double* __restrict__ points, double* __restrict__ cost,
                                                     int* __restrict__ visible) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int o0 = offsets[t], o1 = offsets[t + 1];
    const double pt[3] = {points[3 * (size_t)t], points[3 * (size_t)t + 1], points[3 * (size_t)t + 2]};
    double sum = 0.0;
    int cnt = 0;
    for (int i = o0; i < o1; ++i) {
        double e;
        if (ray_project_term(cameras + 14 * (size_t)cameraIdx[i], pt, obs[2 * (size_t)i], obs[2 * (size_t)i + 1], e)) {
            sum = sum + e;
            cnt += 1;
        }
    }
    if (cost) cost[t] = cnt == 0 ? __builtin_inf() : sum / (double)cnt;
    if (visible) visible[t] = cnt;
}

void launch_tri_validate(const int* d_offsets, int T, const int* d_cameraIdx, int nCameras, unsigned int* d_ctr,
                         hipStream_t s) {
    hipLaunchKernelGGL(mcv_tri_check_offsets, dim3((unsigned)(((long long)T + 255) / 256)), dim3(256), 0, s, d_offsets, T, d_ctr);
    if (d_cameraIdx)
        hipLaunchKernelGGL(mcv_tri_check_cameras, dim3(kTriGrid), dim3(256), 0, s, d_offsets, T, d_cameraIdx,
                           nCameras, d_ctr);
}

void launch_tri_unproject(const double* d_cameras, const int* d_cameraIdx, const double* d_obs,
                          const int* d_offsets, int T, double* d_rays, hipStream_t s) {
    ProfScope ps("tri_unproject", s);
    hipLaunchKernelGGL(mcv_tri_unproject, dim3(kTriGrid), dim3(256), 0, s, d_cameras, d_cameraIdx, d_obs, d_offsets,
                       T, d_rays);
}

void launch_tri_intersect(const double* d_rays, const int* d_offsets, int T, double* d_points, int* d_pairCounts,
                          int* d_longList, unsigned int* d_ctr, hipStream_t s) {
    {
        ProfScope ps("tri_short", s);
        hipLaunchKernelGGL(mcv_tri_short, dim3((unsigned)(((long long)T + 255) / 256)), dim3(256), 0, s, d_rays, d_offsets, T, d_points,
                           d_pairCounts, d_longList, d_ctr);
    }
    // the queue's length stays on the device: a fixed grid strides over it (no workgroup: no work)
    const int grid = T < 8 * kTriGrid ? T : 8 * kTriGrid;
    ProfScope ps("tri_long", s);
    hipLaunchKernelGGL(mcv_tri_long, dim3(grid), dim3(kTriLongThreads), 0, s, d_rays, d_offsets, d_longList,
                       d_points, d_pairCounts, d_ctr);
}

void launch_tri_stats(const double* d_cameras, const int* d_cameraIdx, const double* d_obs, const int* d_offsets,
                      int T, const double* d_points, double* d_cost, int* d_visible, hipStream_t s) {
    ProfScope ps("tri_stats", s);
    hipLaunchKernelGGL(mcv_tri_stats, dim3((unsigned)(((long long)T + 255) / 256)), dim3(256), 0, s, d_cameras, d_cameraIdx, d_obs,
                       d_offsets, T, d_points, d_cost, d_visible);
}

}  // namespace mcv
