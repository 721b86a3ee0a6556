// sift.hip — SIFT detection kernels for gfx950, wave64: grey conversion and doubling,
// the separable blur on LDS tiles, the fused DoG / 26-neighbour pass, refinement (one lane per
// candidate), orientation and descriptor (one wave per keypoint, integer histograms in LDS), and the
// bucket passes that order, de-duplicate and select the keypoints. The arithmetic of every sample is
// sift_math.h's, which the host twin compiles too; the loops over tiles, patches and windows are
// sift_device.h's, which the batch's kernels (sift_batch.hip) call too; no kernel adds floats in an
// order that depends on the hardware's scheduling.
#include "kernels.h"
#include "sift_math.h"
#include "sift_device.h"

namespace mcv {
namespace {

typedef unsigned long long u64;

__global__ __launch_bounds__(256) void sift_grey_double_kernel(const uint8_t* __restrict__ img, int w, int h, int ch,
                                                               float* __restrict__ up) {
    sift_dev_grey_double(img, w, h, ch, up, blockIdx.x * 256 + threadIdx.x, blockIdx.y);
}

__global__ __launch_bounds__(kSiftRowTile) void sift_blur_rows_kernel(const float* __restrict__ in,
                                                                      float* __restrict__ out, int w, int h,
                                                                      const float* __restrict__ taps, int R) {
    extern __shared__ float tile[];
    sift_dev_blur_rows(in, out, w, taps, R, blockIdx.y, blockIdx.x * kSiftRowTile, tile);
}

__global__ __launch_bounds__(256) void sift_blur_cols_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                             int w, int h, const float* __restrict__ taps, int R) {
    extern __shared__ float tile[];
    sift_dev_blur_cols(in, out, w, h, taps, R, blockIdx.x, blockIdx.y, tile);
}

__global__ __launch_bounds__(256) void sift_downsample_kernel(const float* __restrict__ src, int pw, float* __restrict__ dst,
                                                              int w, int h) {
    const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (c < w) dst[(size_t)r * (size_t)w + c] = src[(size_t)(2 * r) * (size_t)pw + 2 * c];
}

// DoG and the 26-neighbour test of one octave in one pass (sift_device.h); a wave covers 64 columns of
// one row. Candidates are appended wave by wave.
__global__ __launch_bounds__(256) void sift_extrema_kernel(const float* __restrict__ g, int w, int h, int o, int nl,
                                                           float thr, int4* __restrict__ cand, unsigned cap,
                                                           unsigned* __restrict__ ctr) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
    sift_dev_extrema(g, w, h, nl, thr, r, c, [=](bool is, int layer) {
        sift_dev_append(is, make_int4(o, layer, r, c), cand, cap, &ctr[0], nullptr);
    });
}

__global__ __launch_bounds__(256) void sift_refine_kernel(SiftPyramid Y, SiftParams P, const int4* __restrict__ cand,
                                                          int nC, SiftKp* __restrict__ kps, unsigned* __restrict__ ctr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nC) return;
    const int4 q = cand[i];
    SiftKp kp;
    const bool ok = sift_refine(Y.base + Y.obase[q.x], Y.ow[q.x], Y.oh[q.x], q.x, q.y, q.z, q.w, P, kp);
    if (!ok) kp.o = -1;
    kps[i] = kp;
    if (ok) atomicAdd(&ctr[1], 1u);
}

// One wave per refined candidate: the histogram and its peaks (sift_device.h), then lane 0 appends one
// record per peak.
__global__ __launch_bounds__(256) void sift_orient_kernel(SiftPyramid Y, const int4* __restrict__ cand,
                                                          const SiftKp* __restrict__ kps, int nC,
                                                          SiftRec* __restrict__ recs, u64* __restrict__ keys,
                                                          u64* __restrict__ starts, u64* __restrict__ rkeys,
                                                          unsigned* __restrict__ ctr, unsigned* __restrict__ bcnt) {
    __shared__ u64 hist[4][kSiftOriBins];
    const int wv = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wv;
    bool valid = i < nC;
    SiftKp kp;
    kp.o = -1;
    if (valid) kp = kps[i];
    valid = valid && kp.o >= 0;
    const int o = valid ? kp.o : 0;
    int bins[kSiftMaxPeaks];
    float angles[kSiftMaxPeaks];
    const int np = sift_dev_orient(Y.base + Y.obase[o], Y.ow[o], Y.oh[o], kp, valid, hist[wv], bins, angles);
    if (np) {   // lane 0 of a valid wave
        const unsigned base = atomicAdd(&ctr[2], (unsigned)np);
        atomicAdd(&bcnt[sift_bucket(Y, kp.o, kp.layer, kp.r)], (unsigned)np);   // the row's count, for the order
        // base + np <= 18 nC, the buffers' size
        sift_dev_orient_records(kp, cand[i], np, bins, angles, (size_t)base, 0, recs, keys, starts, rkeys);
    }
}

// ---- order. The records were appended in arrival order, which no output may depend on. The rows of the
// pyramid (octave, layer, row) are buckets whose counts the orientation kernel took: a scan gives every
// row its segment, a scatter fills the segments in any order, and every record finds its place inside
// its row's segment by counting the records of that row before it in (key, start) order. What comes out
// is the total order by (key, start), the later copies of an exact duplicate flagged.

// One block: boff = exclusive scan of bcnt[0 .. nB) (boff[nB] = the total), and bcnt back to 0 for the scatter.
__global__ __launch_bounds__(1024) void sift_bucket_scan_kernel(unsigned* __restrict__ bcnt, unsigned* __restrict__ boff,
                                                                 int nB) {
    __shared__ unsigned part[1024];
    const int per = (nB + 1023) / 1024, lo = threadIdx.x * per, hi = lo + per < nB ? lo + per : nB;
    unsigned sum = 0;
    for (int b = lo; b < hi; ++b) sum += bcnt[b];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned run = 0;
        for (int t = 0; t < 1024; ++t) {
            const unsigned v = part[t];
            part[t] = run;
            run += v;
        }
        boff[nB] = run;
    }
    __syncthreads();
    unsigned run = part[threadIdx.x];
    for (int b = lo; b < hi; ++b) {
        boff[b] = run;
        run += bcnt[b];
        bcnt[b] = 0;
    }
}

__device__ __forceinline__ int sift_key_bucket(const SiftPyramid& Y, u64 key) {
    return sift_bucket(Y, (int)(key >> 40), (int)(key >> 36) & 15, (int)(key >> 21) & 0x7fff);
}

__global__ __launch_bounds__(256) void sift_bucket_scatter_kernel(SiftPyramid Y, const u64* __restrict__ keys, int n,
                                                                  const unsigned* __restrict__ boff,
                                                                  unsigned* __restrict__ bcur, int* __restrict__ perm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int b = sift_key_bucket(Y, keys[i]);
    perm[boff[b] + atomicAdd(&bcur[b], 1u)] = i;   // boff[b] + (a place below the row's count) < boff[b + 1] <= n
}

// sortedIdx[q], skeys[q], srkeys[q], keep[q] for the place q of every record in (key, start) order
__global__ __launch_bounds__(256) void sift_bucket_rank_kernel(SiftPyramid Y, const u64* __restrict__ keys,
                                                               const u64* __restrict__ starts,
                                                               const u64* __restrict__ rkeys, int n,
                                                               const unsigned* __restrict__ boff,
                                                               const int* __restrict__ perm, int* __restrict__ sortedIdx,
                                                               u64* __restrict__ skeys, u64* __restrict__ srkeys,
                                                               uint8_t* __restrict__ keep) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int i = perm[p];
    const u64 ki = keys[i], si = starts[i];
    const int b = sift_key_bucket(Y, ki);
    unsigned E;
    const unsigned q = sift_dev_rank(keys, starts, perm, boff[b], boff[b + 1], ki, si, E);   // < n
    sortedIdx[q] = i;
    skeys[q] = ki;
    srkeys[q] = rkeys[i];
    keep[q] = E == 0;
}

// FeatureCount: of the kept records, those with fewer than `limit` before them in (k1, k2) order, counted
// over LDS tiles of all n records (quadratic; it runs only when FeatureCount > 0).
__global__ __launch_bounds__(256) void sift_select_kernel(const u64* __restrict__ k1, const u64* __restrict__ k2,
                                                          const uint8_t* __restrict__ flagIn, int n, int limit,
                                                          uint8_t* __restrict__ flagOut) {
    __shared__ u64 a1[256], a2[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool mine = i < n && flagIn[i];
    const u64 my1 = mine ? k1[i] : 0, my2 = mine ? k2[i] : 0;
    int before = 0;
    for (int base = 0; base < n; base += 256) {
        const int m = base + threadIdx.x;
        const bool ok = m < n && flagIn[m];
        a1[threadIdx.x] = ok ? k1[m] : ~0ull;
        a2[threadIdx.x] = ok ? k2[m] : ~0ull;
        __syncthreads();
#pragma unroll 8
        for (int t = 0; t < 256; ++t) before += (a1[t] < my1 || (a1[t] == my1 && a2[t] < my2)) ? 1 : 0;
        __syncthreads();
    }
    if (i < n) flagOut[i] = mine && before < limit;
}

// One block: out = the kept records in order, *count = how many.
__global__ __launch_bounds__(1024) void sift_compact_kernel(const uint8_t* __restrict__ keep,
                                                            const int* __restrict__ sortedIdx,
                                                            const SiftRec* __restrict__ recs, int n,
                                                            SiftRec* __restrict__ out, unsigned* __restrict__ count) {
    __shared__ unsigned wsum[16];
    __shared__ unsigned base;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int start = 0; start < n; start += 1024) {
        const int q = start + (int)threadIdx.x;
        const bool k = q < n && keep[q];
        const u64 m = __ballot(k);
        if (lane == 0) wsum[wv] = (unsigned)__popcll(m);
        __syncthreads();
        unsigned off = base;
        for (int v = 0; v < wv; ++v) off += wsum[v];
        if (k) out[off + (unsigned)__popcll(m & ((1ull << lane) - 1ull))] = recs[sortedIdx[q]];
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned tot = 0;
            for (int v = 0; v < 16; ++v) tot += wsum[v];
            base += tot;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = base;
}

// One wave per output keypoint (sift_device.h).
__global__ __launch_bounds__(256) void sift_describe_kernel(SiftPyramid Y, const SiftRec* __restrict__ recs, int n,
                                                            int descType, SiftKeyPointOut* __restrict__ kpOut,
                                                            uint8_t* __restrict__ descU8, float* __restrict__ descF32) {
    __shared__ u64 sum[4][kSiftDescLen];
    __shared__ float fo[4][kSiftDescLen];
    const int wv = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wv;
    const bool valid = i < n;
    SiftRec q;
    q.o = 0;
    if (valid) q = recs[i];
    sift_dev_describe(Y.base + Y.obase[q.o], Y.ow[q.o], Y.oh[q.o], q, valid, (size_t)(valid ? i : 0), descType, kpOut,
                      descU8, descF32, sum[wv], fo[wv]);
}

inline unsigned blocks(long long n, int per) { return (unsigned)(n > 0 ? (n + per - 1) / per : 1); }

}  // namespace

void launch_sift_grey_double(const uint8_t* d_img, int w, int h, int ch, float* d_up, hipStream_t s) {
    sift_grey_double_kernel<<<dim3(blocks(2 * w, 256), (unsigned)(2 * h)), 256, 0, s>>>(d_img, w, h, ch, d_up);
}

void launch_sift_blur(const float* d_in, float* d_out, float* d_tmp, int w, int h, const float* d_taps, int R,
                      hipStream_t s) {
    sift_blur_rows_kernel<<<dim3(blocks(w, kSiftRowTile), (unsigned)h), kSiftRowTile,
                            (size_t)(kSiftRowTile + 2 * R) * sizeof(float), s>>>(d_in, d_tmp, w, h, d_taps, R);
    sift_blur_cols_kernel<<<dim3(blocks(w, kSiftColTileW), blocks(h, kSiftColTileH)), 256,
                            (size_t)(kSiftColTileH + 2 * R) * kSiftColTileW * sizeof(float), s>>>(d_tmp, d_out, w, h,
                                                                                                 d_taps, R);
}

void launch_sift_downsample(const float* d_src, int pw, float* d_dst, int w, int h, hipStream_t s) {
    sift_downsample_kernel<<<dim3(blocks(w, 256), (unsigned)h), 256, 0, s>>>(d_src, pw, d_dst, w, h);
}

void launch_sift_extrema(const float* d_g, int w, int h, int o, int nl, float thr, void* d_cand, unsigned cap,
                         unsigned* d_ctr, hipStream_t s) {
    sift_extrema_kernel<<<dim3(blocks(w, 64), blocks(h, 4)), 256, 0, s>>>(d_g, w, h, o, nl, thr, (int4*)d_cand, cap,
                                                                         d_ctr);
}

void launch_sift_refine(const SiftPyramid& Y, const SiftParams& P, const void* d_cand, int nC, SiftKp* d_kps,
                        unsigned* d_ctr, hipStream_t s) {
    sift_refine_kernel<<<blocks(nC, 256), 256, 0, s>>>(Y, P, (const int4*)d_cand, nC, d_kps, d_ctr);
}

void launch_sift_orient(const SiftPyramid& Y, const void* d_cand, const SiftKp* d_kps, int nC, SiftRec* d_recs,
                        unsigned long long* d_keys, unsigned long long* d_starts, unsigned long long* d_rkeys,
                        unsigned* d_ctr, unsigned* d_bcnt, hipStream_t s) {
    sift_orient_kernel<<<blocks(nC, 4), 256, 0, s>>>(Y, (const int4*)d_cand, d_kps, nC, d_recs, d_keys, d_starts,
                                                     d_rkeys, d_ctr, d_bcnt);
}

void launch_sift_order(const SiftPyramid& Y, const SiftOrder& O, int n, int featureCount, hipStream_t s) {
    sift_bucket_scan_kernel<<<1, 1024, 0, s>>>(O.bcnt, O.boff, O.nBuckets);
    sift_bucket_scatter_kernel<<<blocks(n, 256), 256, 0, s>>>(Y, O.keys, n, O.boff, O.bcnt, O.perm);
    sift_bucket_rank_kernel<<<blocks(n, 256), 256, 0, s>>>(Y, O.keys, O.starts, O.rkeys, n, O.boff, O.perm,
                                                           O.sortedIdx, O.skeys, O.srkeys, O.keepA);
    const uint8_t* keep = O.keepA;
    if (featureCount > 0) {
        sift_select_kernel<<<blocks(n, 256), 256, 0, s>>>(O.srkeys, O.skeys, O.keepA, n, featureCount, O.keepB);
        keep = O.keepB;
    }
    sift_compact_kernel<<<1, 1024, 0, s>>>(keep, O.sortedIdx, O.recs, n, O.out, O.count);
}

void launch_sift_describe(const SiftPyramid& Y, const SiftRec* d_recs, int n, int descType, SiftKeyPointOut* d_kp,
                          uint8_t* d_u8, float* d_f32, hipStream_t s) {
    sift_describe_kernel<<<blocks(n, 4), 256, 0, s>>>(Y, d_recs, n, descType, d_kp, d_u8, d_f32);
}

}  // namespace mcv
