// sift.hip — SIFT detection kernels for gfx950, wave64: grey conversion and doubling,
// the separable blur on LDS tiles, the fused DoG / 26-neighbour pass, refinement (one lane per
// candidate), orientation and descriptor (one wave per keypoint, integer histograms in LDS), and the
// bucket passes that order, de-duplicate and select the keypoints. The arithmetic of every sample is
// sift_math.h's, which the host twin compiles too; no kernel adds floats in an order that depends on
// the hardware's scheduling.
#include "kernels.h"
#include "sift_math.h"

namespace mcv {
namespace {

typedef unsigned long long u64;

__global__ __launch_bounds__(256) void sift_grey_double_kernel(const uint8_t* __restrict__ img, int w, int h, int ch,
                                                               float* __restrict__ up) {
    const int C = blockIdx.x * 256 + threadIdx.x, R = blockIdx.y;
    if (C >= 2 * w) return;
    const int c0 = C >> 1, r0 = R >> 1;
    const int c1 = (C & 1) ? (c0 + 1 < w ? c0 + 1 : w - 1) : c0;
    const int r1 = (R & 1) ? (r0 + 1 < h ? r0 + 1 : h - 1) : r0;
    // rows (along x) first, then columns; every value is exact in float
    float a = sift_grey(img + ((size_t)r0 * w + c0) * ch, ch);
    float b = sift_grey(img + ((size_t)r1 * w + c0) * ch, ch);
    if (C & 1) {
        a = 0.5f * a + 0.5f * sift_grey(img + ((size_t)r0 * w + c1) * ch, ch);
        b = 0.5f * b + 0.5f * sift_grey(img + ((size_t)r1 * w + c1) * ch, ch);
    }
    up[(size_t)R * (size_t)(2 * w) + C] = (R & 1) ? 0.5f * a + 0.5f * b : a;
}

// One row segment of kSiftRowTile outputs per block, the segment and its halo in LDS.
__global__ __launch_bounds__(kSiftRowTile) void sift_blur_rows_kernel(const float* __restrict__ in,
                                                                      float* __restrict__ out, int w, int h,
                                                                      const float* __restrict__ taps, int R) {
    extern __shared__ float tile[];
    const int r = blockIdx.y, x0 = blockIdx.x * kSiftRowTile;
    const float* row = in + (size_t)r * (size_t)w;
    for (int k = threadIdx.x; k < kSiftRowTile + 2 * R; k += kSiftRowTile) tile[k] = row[sift_reflect(x0 + k - R, w)];
    __syncthreads();
    const int c = x0 + threadIdx.x;
    if (c >= w) return;
    float acc = 0.0f;
    for (int t = 0; t <= 2 * R; ++t) acc = acc + taps[t] * tile[threadIdx.x + t];
    out[(size_t)r * (size_t)w + c] = acc;
}

// A tile of kSiftColTileW columns x kSiftColTileH rows per block, with a halo of R rows above and below.
__global__ __launch_bounds__(256) void sift_blur_cols_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                             int w, int h, const float* __restrict__ taps, int R) {
    extern __shared__ float tile[];
    const int cx = threadIdx.x & (kSiftColTileW - 1), ty = threadIdx.x / kSiftColTileW;
    const int c = blockIdx.x * kSiftColTileW + cx, y0 = blockIdx.y * kSiftColTileH;
    const int cc = c < w ? c : w - 1;
    for (int k = ty; k < kSiftColTileH + 2 * R; k += 256 / kSiftColTileW)
        tile[k * kSiftColTileW + cx] = in[(size_t)sift_reflect(y0 + k - R, h) * (size_t)w + cc];
    __syncthreads();
    if (c >= w) return;
    const int per = kSiftColTileH / (256 / kSiftColTileW);
    for (int q = 0; q < per; ++q) {
        const int rr = ty * per + q, r = y0 + rr;
        if (r >= h) break;
        float acc = 0.0f;
        for (int t = 0; t <= 2 * R; ++t) acc = acc + taps[t] * tile[(rr + t) * kSiftColTileW + cx];
        out[(size_t)r * (size_t)w + c] = acc;
    }
}

__global__ __launch_bounds__(256) void sift_downsample_kernel(const float* __restrict__ src, int pw, float* __restrict__ dst,
                                                              int w, int h) {
    const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (c < w) dst[(size_t)r * (size_t)w + c] = src[(size_t)(2 * r) * (size_t)pw + 2 * c];
}

// DoG and the 26-neighbour test of one octave in one pass: a lane walks its pixel's 3 x 3 patch up the
// Gaussian stack, keeps three DoG patches in registers, and tests the middle one. Candidates are
// appended wave by wave: one counter add per wave, the lanes' places by their rank in the ballot.
__global__ __launch_bounds__(256) void sift_extrema_kernel(const float* __restrict__ g, int w, int h, int o, int nl,
                                                           float thr, int4* __restrict__ cand, unsigned cap,
                                                           unsigned* __restrict__ ctr) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 64 + lane, r = blockIdx.y * 4 + (threadIdx.x >> 6);
    const bool active = r >= kSiftBorder && r < h - kSiftBorder && c >= kSiftBorder && c < w - kSiftBorder;
    const size_t plane = (size_t)w * (size_t)h;
    float gp[9], d0[9], d1[9], d2[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        gp[k] = active ? g[(size_t)(r + k / 3 - 1) * (size_t)w + (size_t)(c + k % 3 - 1)] : 0.0f;
        d0[k] = d1[k] = d2[k] = 0.0f;
    }
    for (int L = 0; L < nl + 2; ++L) {
        const float* gn = g + (size_t)(L + 1) * plane;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float v = active ? gn[(size_t)(r + k / 3 - 1) * (size_t)w + (size_t)(c + k % 3 - 1)] : 0.0f;
            d0[k] = d1[k];
            d1[k] = d2[k];
            d2[k] = v - gp[k];
            gp[k] = v;
        }
        if (L < 2) continue;
        const float v = d1[4];
        bool is = active && fabsf(v) > thr;
        if (is) {
            bool mx = true, mn = true;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                mx = mx && v >= d0[k] && v >= d1[k] && v >= d2[k];
                mn = mn && v <= d0[k] && v <= d1[k] && v <= d2[k];
            }
            is = v > 0.0f ? mx : mn;
        }
        const u64 m = __ballot(is);
        if (m) {
            const int leader = __ffsll((long long)m) - 1;
            unsigned base = 0;
            if (lane == leader) base = atomicAdd(&ctr[0], (unsigned)__popcll(m));
            base = __shfl(base, leader);
            if (is) {
                const unsigned at = base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
                if (at < cap) cand[at] = make_int4(o, L - 1, r, c);
            }
        }
    }
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

// One wave per refined candidate: the 36-bin histogram as 64-bit integer LDS atomics (the sum does not
// depend on the order), then lane 0 smooths it and appends one record per peak.
__global__ __launch_bounds__(256) void sift_orient_kernel(SiftPyramid Y, const int4* __restrict__ cand,
                                                          const SiftKp* __restrict__ kps, int nC,
                                                          SiftRec* __restrict__ recs, u64* __restrict__ keys,
                                                          u64* __restrict__ starts, u64* __restrict__ rkeys,
                                                          unsigned* __restrict__ ctr, unsigned* __restrict__ bcnt) {
    __shared__ u64 hist[4][kSiftOriBins];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + wv;
    bool valid = i < nC;
    SiftKp kp;
    kp.o = -1;
    if (valid) kp = kps[i];
    valid = valid && kp.o >= 0;
    if (lane < kSiftOriBins) hist[wv][lane] = 0;
    __syncthreads();
    if (valid) {
        const int w = Y.ow[kp.o], h = Y.oh[kp.o];
        const float* img = Y.base + Y.obase[kp.o] + (size_t)kp.layer * (size_t)w * (size_t)h;
        const int rad = sift_ori_radius(kp.scl), side = 2 * rad + 1, n = side * side;
        const float es = sift_ori_escale(kp.scl);
        for (int s = lane; s < n; s += 64) {
            int bin;
            long long q;
            if (sift_ori_sample(img, w, h, kp.r, kp.c, s / side - rad, s % side - rad, es, bin, q))
                atomicAdd(&hist[wv][bin], (u64)q);
        }
    }
    __syncthreads();
    if (valid && lane == 0) {
        int bins[kSiftMaxPeaks];
        float angles[kSiftMaxPeaks];
        const int np = sift_ori_peaks((const long long*)hist[wv], bins, angles);
        const unsigned base = np ? atomicAdd(&ctr[2], (unsigned)np) : 0u;
        if (np) atomicAdd(&bcnt[sift_bucket(Y, kp.o, kp.layer, kp.r)], (unsigned)np);   // the row's count, for the order
        const int4 q = cand[i];
        const float sc = (float)(1 << kp.o) * 0.5f;
        for (int k = 0; k < np; ++k) {
            const size_t at = (size_t)base + (size_t)k;   // at < 18 nC, the buffers' size
            recs[at] = SiftRec{((float)kp.c + kp.xc) * sc, ((float)kp.r + kp.xr) * sc, kp.size, angles[k],
                               kp.response, kp.octave, kp.o, kp.layer, kp.r, kp.c, kp.scl, 0};
            keys[at] = sift_key(kp.o, kp.layer, kp.r, kp.c, bins[k]);
            starts[at] = sift_key(q.x, q.y, q.z, q.w, bins[k]);
            rkeys[at] = (u64)(0xffffffffu - __float_as_uint(kp.response));
        }
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
    const unsigned lo = boff[b], hi = boff[b + 1];
    unsigned L = 0, E = 0;
    for (unsigned m = lo; m < hi; ++m) {
        const int j = perm[m];
        const u64 kj = keys[j];
        L += kj < ki ? 1u : 0u;
        E += (kj == ki && starts[j] < si) ? 1u : 0u;
    }
    const unsigned q = lo + L + E;   // < hi <= n: the other records of the row are hi - lo - 1
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

// One wave per output keypoint: the 4 x 4 x 8 histogram as 64-bit integer LDS atomics, lane 0
// normalises, the wave writes the row and the KeyPoint2d.
__global__ __launch_bounds__(256) void sift_describe_kernel(SiftPyramid Y, const SiftRec* __restrict__ recs, int n,
                                                            int descType, SiftKeyPointOut* __restrict__ kpOut,
                                                            uint8_t* __restrict__ descU8, float* __restrict__ descF32) {
    __shared__ u64 sum[4][kSiftDescLen];
    __shared__ float fo[4][kSiftDescLen];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + wv;
    const bool valid = i < n;
    for (int k = lane; k < kSiftDescLen; k += 64) sum[wv][k] = 0;
    __syncthreads();
    SiftRec q;
    if (valid) {
        q = recs[i];
        const int w = Y.ow[q.o], h = Y.oh[q.o];
        const float* img = Y.base + Y.obase[q.o] + (size_t)q.layer * (size_t)w * (size_t)h;
        const SiftDescFrame F = sift_desc_frame(q.angle, q.scl, w, h);
        const int side = 2 * F.radius + 1;
        const long long ns = (long long)side * side;
        u64* mySum = sum[wv];
        for (long long s = lane; s < ns; s += 64)
            sift_desc_sample(img, w, h, q.r, q.c, (int)(s / side) - F.radius, (int)(s % side) - F.radius, F,
                             [mySum](int k, long long v) { atomicAdd(&mySum[k], (u64)v); });
    }
    __syncthreads();
    if (valid && lane == 0) sift_desc_finish((const long long*)sum[wv], fo[wv]);
    __syncthreads();
    if (!valid) return;
    for (int k = lane; k < kSiftDescLen; k += 64) {
        if (descType == 0)
            descU8[(size_t)i * kSiftDescLen + k] = sift_desc_byte(fo[wv][k]);
        else
            descF32[(size_t)i * kSiftDescLen + k] = fo[wv][k];
    }
    if (lane == 0) kpOut[i] = SiftKeyPointOut{q.x, q.y, q.size, q.angle, q.response, q.octave, -1};
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
