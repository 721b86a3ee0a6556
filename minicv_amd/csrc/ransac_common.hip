// ransac_common.hip — the two small kernels every RANSAC model family uses.
//
//   mcv_best_*   packed-key argmax (count << 32 | ~idx) over a chunk's counts with OpenCV's "first
//                strictly greater wins" order and the sampler-failure `break`.   [SURVEY §2 K3]
//   mcv_fill_u8  a byte fill (the essential and PnP paths' all-inlier masks).
#include "mcv_common.h"
#include "kernels.h"

namespace mcv {

// ------------------------------------------------------------------------------------------
// Best packed key + first sampler failure.
// ------------------------------------------------------------------------------------------
static const int kBestThreads = 256;
static const int kBestMaxBlocks = 512;

__device__ __forceinline__ uint64_t pack_key(int count, int64_t hyp, int minCount) {
    return count >= minCount ? (((uint64_t)(uint32_t)count << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)hyp)) : 0ull;
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint64_t o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ int64_t wave_min_i64(int64_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int64_t o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ void block_maxmin(uint64_t& key, int64_t& fail) {
    __shared__ uint64_t sk[kBestThreads / 64];
    __shared__ int64_t sf[kBestThreads / 64];
    key = wave_max_u64(key);
    fail = wave_min_i64(fail);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { sk[wave] = key; sf[wave] = fail; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBestThreads / 64; ++w) {
            key = sk[w] > key ? sk[w] : key;
            fail = sf[w] < fail ? sf[w] : fail;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(kBestThreads) void mcv_best_partial(const int* __restrict__ counts, int n,
                                                                 int64_t hypBegin, int minCount,
                                                                 uint64_t* __restrict__ pkey,
                                                                 int64_t* __restrict__ pfail) {
    uint64_t key = 0;
    int64_t fail = INT64_MAX;
    for (int i = blockIdx.x * kBestThreads + threadIdx.x; i < n; i += gridDim.x * kBestThreads) {
        const int c = counts[i];
        const uint64_t k = pack_key(c, hypBegin + i, minCount);
        key = k > key ? k : key;
        if (c == kStatusNoSample && hypBegin + i < fail) fail = hypBegin + i;
    }
    block_maxmin(key, fail);
    if (threadIdx.x == 0) { pkey[blockIdx.x] = key; pfail[blockIdx.x] = fail; }
}

// out[0] = best key among hypotheses before the first sampler failure; out[1] = that failure.
__global__ __launch_bounds__(kBestThreads) void mcv_best_final(const uint64_t* __restrict__ pkey,
                                                               const int64_t* __restrict__ pfail, int nblocks,
                                                               const int* __restrict__ counts, int n,
                                                               int64_t hypBegin, int minCount,
                                                               uint64_t* __restrict__ out) {
    __shared__ int64_t s_fail;
    uint64_t key = 0;
    int64_t fail = INT64_MAX;
    for (int b = threadIdx.x; b < nblocks; b += kBestThreads) {
        key = pkey[b] > key ? pkey[b] : key;
        fail = pfail[b] < fail ? pfail[b] : fail;
    }
    block_maxmin(key, fail);
    if (threadIdx.x == 0) s_fail = fail;
    __syncthreads();
    fail = s_fail;
    if (fail != INT64_MAX) {
        // Rare (degenerate input): only hypotheses before the failure count.
        key = 0;
        const int lim = (int)(fail - hypBegin);
        for (int i = threadIdx.x; i < lim; i += kBestThreads) {
            const uint64_t k = pack_key(counts[i], hypBegin + i, minCount);
            key = k > key ? k : key;
        }
        int64_t dummy = INT64_MAX;
        block_maxmin(key, dummy);
    }
    if (threadIdx.x == 0) {
        out[0] = key;
        out[1] = (uint64_t)fail;
    }
}

__global__ void mcv_fill_u8(uint8_t* __restrict__ p, int n, uint8_t v) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

void launch_best(const int* d_counts, int n, int64_t hypBegin, int minCount, uint64_t* d_pkey, int64_t* d_pfail,
                 uint64_t* d_out, hipStream_t s) {
    int nb = (n + kBestThreads * 8 - 1) / (kBestThreads * 8);
    if (nb < 1) nb = 1;
    if (nb > kBestMaxBlocks) nb = kBestMaxBlocks;
    hipLaunchKernelGGL(mcv_best_partial, dim3(nb), dim3(kBestThreads), 0, s, d_counts, n, hypBegin, minCount, d_pkey,
                       d_pfail);
    hipLaunchKernelGGL(mcv_best_final, dim3(1), dim3(kBestThreads), 0, s, d_pkey, d_pfail, nb, d_counts, n, hypBegin,
                       minCount, d_out);
}

void launch_fill_u8(uint8_t* d, int n, uint8_t v, hipStream_t s) {
    hipLaunchKernelGGL(mcv_fill_u8, dim3((n + 255) / 256), dim3(256), 0, s, d, n, v);
}

}  // namespace mcv
