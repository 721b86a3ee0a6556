// sift_batch.hip — SIFT detection of many images in one call, for gfx950, wave64. The stages
// of sift.hip over (image, tile), (image, candidate) and (image, keypoint) grids: blockIdx.z is the image
// where a stage walks pixels, and a record carries its image where a stage walks records. Sizes and
// offsets come from the table of SiftBatchImage. The loops and every sample's arithmetic are
// sift_device.h's and sift_math.h's, shared with the single call. The order stage's bucket scan and its
// compaction are grid-wide three-pass integer scans; nothing adds floats in an order that depends on the
// hardware's scheduling, and no output depends on the order in which records arrive.
#include "kernels.h"
#include "sift_math.h"
#include "sift_batch_plan.h"
#include "sift_device.h"

namespace mcv {
namespace {

typedef unsigned long long u64;
static_assert(kSiftBatchOctaves == kSiftMaxOctaves, "one octave cap");
static_assert(kSiftBatchMaxImages <= 65535, "the image index is a grid's z");
static_assert((long long)kSiftMaxPeaks * kSiftBatchMaxCandidates < (1ll << 31), "record places are ints");

__global__ __launch_bounds__(256) void sift_batch_grey_double_kernel(SiftBatchDevice D) {
    const SiftBatchImage& T = D.table[blockIdx.z];
    const int R = blockIdx.y;
    if (T.nOctaves == 0 || R >= 2 * T.h) return;
    sift_dev_grey_double(D.img + T.imgOff, T.w, T.h, T.ch, D.up + T.scratchOff, blockIdx.x * 256 + threadIdx.x, R);
}

// the source of blur `blur` of octave o: the doubled base, or the octave's image blur - 1
__device__ __forceinline__ const float* blur_source(const SiftBatchDevice& D, const SiftBatchImage& T, int o, int blur) {
    if (blur == 0) return D.up + T.scratchOff;
    return D.pyr + T.obase[o] + (size_t)(blur - 1) * (size_t)T.ow[o] * (size_t)T.oh[o];
}

__global__ __launch_bounds__(kSiftRowTile) void sift_batch_blur_rows_kernel(SiftBatchDevice D, int o, int blur,
                                                                            const float* __restrict__ taps, int R) {
    extern __shared__ float tile[];
    const SiftBatchImage& T = D.table[blockIdx.z];
    if (o >= T.nOctaves) return;
    const int w = T.ow[o], h = T.oh[o], r = blockIdx.y, x0 = blockIdx.x * kSiftRowTile;
    if (r >= h || x0 >= w) return;   // the whole block
    sift_dev_blur_rows(blur_source(D, T, o, blur), D.tmp + T.scratchOff, w, taps, R, r, x0, tile);
}

__global__ __launch_bounds__(256) void sift_batch_blur_cols_kernel(SiftBatchDevice D, int o, int blur,
                                                                   const float* __restrict__ taps, int R) {
    extern __shared__ float tile[];
    const SiftBatchImage& T = D.table[blockIdx.z];
    if (o >= T.nOctaves) return;
    const int w = T.ow[o], h = T.oh[o];
    if ((int)blockIdx.x * kSiftColTileW >= w || (int)blockIdx.y * kSiftColTileH >= h) return;   // the whole block
    float* out = D.pyr + T.obase[o] + (size_t)blur * (size_t)w * (size_t)h;
    sift_dev_blur_cols(D.tmp + T.scratchOff, out, w, h, taps, R, blockIdx.x, blockIdx.y, tile);
}

__global__ __launch_bounds__(256) void sift_batch_downsample_kernel(SiftBatchDevice D, int o, int nl) {
    const SiftBatchImage& T = D.table[blockIdx.z];
    if (o >= T.nOctaves) return;
    const int w = T.ow[o], h = T.oh[o], pw = T.ow[o - 1];
    const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (r >= h || c >= w) return;
    const float* src = D.pyr + T.obase[o - 1] + (size_t)nl * (size_t)pw * (size_t)T.oh[o - 1];
    (D.pyr + T.obase[o])[(size_t)r * (size_t)w + c] = src[(size_t)(2 * r) * (size_t)pw + 2 * c];
}

__global__ __launch_bounds__(256) void sift_batch_extrema_kernel(SiftBatchDevice D, int o, int nl, float thr) {
    const int b = blockIdx.z;
    const SiftBatchImage& T = D.table[b];
    if (o >= T.nOctaves) return;
    const int w = T.ow[o], h = T.oh[o];
    if ((int)blockIdx.x * 64 >= w || (int)blockIdx.y * 4 >= h) return;   // the whole block
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
    int4* cand = D.cand;
    const unsigned cap = D.capC;
    unsigned *ctr = D.ctr, *icnt = D.icnt + b;
    sift_dev_extrema(D.pyr + T.obase[o], w, h, nl, thr, r, c, [=](bool is, int layer) {
        sift_dev_append(is, make_int4((b << 4) | o, layer, r, c), cand, cap, ctr, icnt);
    });
}

__global__ __launch_bounds__(256) void sift_batch_refine_kernel(SiftBatchDevice D, SiftParams P, int nC,
                                                                SiftKp* __restrict__ kps) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nC) return;
    const int4 q = D.cand[i];
    const int o = q.x & 15;
    const SiftBatchImage& T = D.table[q.x >> 4];
    SiftKp kp;
    const bool ok = sift_refine(D.pyr + T.obase[o], T.ow[o], T.oh[o], o, q.y, q.z, q.w, P, kp);
    if (!ok) kp.o = -1;
    kps[i] = kp;
    if (ok) atomicAdd(&D.ctr[1], 1u);
}

__global__ __launch_bounds__(256) void sift_batch_orient_kernel(SiftBatchDevice D, const SiftKp* __restrict__ kps, int nC,
                                                                SiftRec* __restrict__ recs, u64* __restrict__ keys,
                                                                u64* __restrict__ starts, u64* __restrict__ rkeys) {
    __shared__ u64 hist[4][kSiftOriBins];
    const int wv = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wv;
    bool valid = i < nC;
    SiftKp kp;
    kp.o = -1;
    int4 q = make_int4(0, 0, 0, 0);
    if (valid) {
        kp = kps[i];
        q = D.cand[i];
    }
    valid = valid && kp.o >= 0;
    const int b = q.x >> 4, o = valid ? kp.o : 0;
    const SiftBatchImage& T = D.table[b];
    int bins[kSiftMaxPeaks];
    float angles[kSiftMaxPeaks];
    const int np = sift_dev_orient(D.pyr + T.obase[o], T.ow[o], T.oh[o], kp, valid, hist[wv], bins, angles);
    if (np) {   // lane 0 of a valid wave
        const unsigned base = atomicAdd(&D.ctr[2], (unsigned)np);
        atomicAdd(&D.bcnt[T.rowBase[kp.o] + (kp.layer - 1) * T.oh[kp.o] + kp.r], (unsigned)np);
        q.x &= 15;   // the start key holds the octave alone
        // base + np <= 18 nC, the buffers' size
        sift_dev_orient_records(kp, q, np, bins, angles, (size_t)base, b, recs, keys, starts, rkeys);
    }
}

// ---- grid-wide exclusive scan of n words or flags in three passes over kSiftBatchScanBlocks contiguous
// ranges: the ranges' sums, their scan in one block, and every range again from its base. Integers only.

// The exclusive prefix of v over the block's threads and the block's total. wsum: 16 words. Has barriers.
__device__ __forceinline__ unsigned block_exscan(unsigned v, unsigned* wsum, unsigned& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    unsigned off = 0, tot = 0;
    for (int k = 0; k < nw; ++k) {
        const unsigned sv = wsum[k];
        off += k < wv ? sv : 0u;
        tot += sv;
    }
    __syncthreads();
    total = tot;
    return off + inc - v;
}

__device__ __forceinline__ void scan_range(long long n, long long& lo, long long& hi) {
    const long long per = (n + kSiftBatchScanBlocks - 1) / kSiftBatchScanBlocks;
    lo = (long long)blockIdx.x * per;
    hi = lo + per < n ? lo + per : n;
}

template <class T>
__global__ __launch_bounds__(256) void sift_batch_scan_sums_kernel(const T* __restrict__ in, long long n,
                                                                   unsigned* __restrict__ part) {
    __shared__ unsigned wsum[16];
    long long lo, hi;
    scan_range(n, lo, hi);
    unsigned sum = 0;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) sum += (unsigned)in[i];
    unsigned total;
    block_exscan(sum, wsum, total);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// One block of kSiftBatchScanBlocks threads: part -> its exclusive scan, part[kSiftBatchScanBlocks] and
// *totalOut = the total.
__global__ __launch_bounds__(kSiftBatchScanBlocks) void sift_batch_scan_parts_kernel(unsigned* __restrict__ part,
                                                                                    unsigned* __restrict__ totalOut) {
    __shared__ unsigned wsum[16];
    unsigned total;
    const unsigned ex = block_exscan(part[threadIdx.x], wsum, total);
    part[threadIdx.x] = ex;
    if (threadIdx.x == 0) {
        part[kSiftBatchScanBlocks] = total;
        *totalOut = total;
    }
}

// out[i] = the exclusive scan at i; `in` back to 0 where zeroIn (the bucket counts, for the scatter)
template <class T>
__global__ __launch_bounds__(256) void sift_batch_scan_apply_kernel(T* __restrict__ in, long long n,
                                                                    const unsigned* __restrict__ part,
                                                                    unsigned* __restrict__ out, bool zeroIn) {
    __shared__ unsigned wsum[16];
    long long lo, hi;
    scan_range(n, lo, hi);
    unsigned run = part[blockIdx.x];
    for (long long base = lo; base < hi; base += 256) {   // the same trips for the whole block
        const long long i = base + threadIdx.x;
        const unsigned v = i < hi ? (unsigned)in[i] : 0u;
        unsigned total;
        const unsigned ex = block_exscan(v, wsum, total);
        if (i < hi) {
            out[i] = run + ex;
            if (zeroIn) in[i] = 0;
        }
        run += total;
    }
}

template <class T>
void scan(T* d_in, long long n, unsigned* d_part, unsigned* d_out, bool zeroIn, hipStream_t s) {
    sift_batch_scan_sums_kernel<T><<<kSiftBatchScanBlocks, 256, 0, s>>>(d_in, n, d_part);
    sift_batch_scan_parts_kernel<<<1, kSiftBatchScanBlocks, 0, s>>>(d_part, d_out + n);
    sift_batch_scan_apply_kernel<T><<<kSiftBatchScanBlocks, 256, 0, s>>>(d_in, n, d_part, d_out, zeroIn);
}

// ---- order: sift.hip's scheme with (image, octave, layer, row) buckets. The key holds the image above
// sift_key's bits, so the total order is image-major and an image's records are those of its buckets.
__device__ __forceinline__ int key_bucket(const SiftBatchDevice& D, u64 key) {
    const SiftBatchImage& T = D.table[(int)(key >> kSiftKeyBits)];
    const int o = (int)(key >> 40) & 31;
    return T.rowBase[o] + (((int)(key >> 36) & 15) - 1) * T.oh[o] + ((int)(key >> 21) & 0x7fff);
}

__global__ __launch_bounds__(256) void sift_batch_scatter_kernel(SiftBatchDevice D, const u64* __restrict__ keys, int n,
                                                                 int* __restrict__ perm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int b = key_bucket(D, keys[i]);
    perm[D.boff[b] + atomicAdd(&D.bcnt[b], 1u)] = i;   // boff[b] + (a place below the bucket's count) < boff[b + 1] <= n
}

__global__ __launch_bounds__(256) void sift_batch_rank_kernel(SiftBatchDevice D, const u64* __restrict__ keys,
                                                              const u64* __restrict__ starts,
                                                              const u64* __restrict__ rkeys, int n,
                                                              const int* __restrict__ perm, int* __restrict__ sortedIdx,
                                                              u64* __restrict__ skeys, u64* __restrict__ srkeys,
                                                              uint8_t* __restrict__ keep) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int i = perm[p];
    const u64 ki = keys[i], si = starts[i];
    const int b = key_bucket(D, ki);
    unsigned E;
    const unsigned q = sift_dev_rank(keys, starts, perm, D.boff[b], D.boff[b + 1], ki, si, E);   // < n
    sortedIdx[q] = i;
    skeys[q] = ki;
    srkeys[q] = rkeys[i];
    keep[q] = E == 0;
}

// FeatureCount per image: of an image's kept records, those with fewer than `limit` of the same image
// before them in (k1, k2) order. A block's 256 places may lie in several images; it walks the records
// of all of them (one contiguous range of the order) in LDS tiles and every lane counts its own image's.
__global__ __launch_bounds__(256) void sift_batch_select_kernel(SiftBatchDevice D, const u64* __restrict__ k1,
                                                                const u64* __restrict__ k2,
                                                                const uint8_t* __restrict__ flagIn, int n, int limit,
                                                                uint8_t* __restrict__ flagOut) {
    __shared__ u64 a1[256], a2[256];
    const int p0 = blockIdx.x * 256;
    if (p0 >= n) return;   // the whole block
    const int i = p0 + threadIdx.x, pl = p0 + 255 < n ? p0 + 255 : n - 1;
    const unsigned lo = D.boff[D.table[(int)(k2[p0] >> kSiftKeyBits)].bucketBegin];
    const unsigned hi = D.boff[D.table[(int)(k2[pl] >> kSiftKeyBits)].bucketEnd];   // <= n
    const bool mine = i < n && flagIn[i];
    const u64 my1 = mine ? k1[i] : 0, my2 = mine ? k2[i] : 0, myImage = my2 >> kSiftKeyBits;
    int before = 0;
    for (unsigned base = lo; base < hi; base += 256) {
        const unsigned m = base + threadIdx.x;
        const bool ok = m < hi && flagIn[m];
        a1[threadIdx.x] = ok ? k1[m] : ~0ull;
        a2[threadIdx.x] = ok ? k2[m] : ~0ull;
        __syncthreads();
#pragma unroll 8
        for (int t = 0; t < 256; ++t)
            before += ((a2[t] >> kSiftKeyBits) == myImage && (a1[t] < my1 || (a1[t] == my1 && a2[t] < my2))) ? 1 : 0;
        __syncthreads();
    }
    if (i < n) flagOut[i] = mine && before < limit;
}

__global__ __launch_bounds__(256) void sift_batch_compact_kernel(const uint8_t* __restrict__ keep,
                                                                 const unsigned* __restrict__ pos,
                                                                 const int* __restrict__ sortedIdx,
                                                                 const SiftRec* __restrict__ recs, int n,
                                                                 SiftRec* __restrict__ out) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q < n && keep[q]) out[pos[q]] = recs[sortedIdx[q]];   // pos[q] < pos[n] <= n
}

// koff[b] = the kept records before image b's first record in the order; koff[nImages] = all of them
__global__ __launch_bounds__(256) void sift_batch_offsets_kernel(SiftBatchDevice D, const unsigned* __restrict__ pos) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b > D.nImages) return;
    D.koff[b] = pos[D.boff[b < D.nImages ? D.table[b].bucketBegin : D.nBuckets]];   // boff[..] <= n
}

__global__ __launch_bounds__(256) void sift_batch_describe_kernel(SiftBatchDevice D, const SiftRec* __restrict__ recs,
                                                                  int n, int descType, SiftKeyPointOut* __restrict__ kpOut,
                                                                  uint8_t* __restrict__ descU8,
                                                                  float* __restrict__ descF32) {
    __shared__ u64 sum[4][kSiftDescLen];
    __shared__ float fo[4][kSiftDescLen];
    const int wv = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wv;
    const bool valid = i < n;
    SiftRec q;
    q.o = 0;
    q.pad = 0;
    if (valid) q = recs[i];
    const SiftBatchImage& T = D.table[q.pad];
    sift_dev_describe(D.pyr + T.obase[q.o], T.ow[q.o], T.oh[q.o], q, valid, (size_t)(valid ? i : 0), descType, kpOut,
                      descU8, descF32, sum[wv], fo[wv]);
}

inline unsigned blocks(long long n, int per) { return (unsigned)(n > 0 ? (n + per - 1) / per : 1); }

}  // namespace

void launch_sift_batch_grey_double(const SiftBatchDevice& D, int maxW, int maxH, hipStream_t s) {
    sift_batch_grey_double_kernel<<<dim3(blocks(maxW, 256), (unsigned)maxH, (unsigned)D.nImages), 256, 0, s>>>(D);
}

void launch_sift_batch_blur(const SiftBatchDevice& D, int o, int blur, int tapOff, int R, int maxW, int maxH,
                            hipStream_t s) {
    // the single call's tiles and LDS: at most 65 024 bytes at the largest radius, no opt-in
    sift_batch_blur_rows_kernel<<<dim3(blocks(maxW, kSiftRowTile), (unsigned)maxH, (unsigned)D.nImages), kSiftRowTile,
                                  (size_t)(kSiftRowTile + 2 * R) * sizeof(float), s>>>(D, o, blur, D.taps + tapOff, R);
    sift_batch_blur_cols_kernel<<<dim3(blocks(maxW, kSiftColTileW), blocks(maxH, kSiftColTileH), (unsigned)D.nImages),
                                  256, (size_t)(kSiftColTileH + 2 * R) * kSiftColTileW * sizeof(float), s>>>(
        D, o, blur, D.taps + tapOff, R);
}

void launch_sift_batch_downsample(const SiftBatchDevice& D, int o, int nl, int maxW, int maxH, hipStream_t s) {
    sift_batch_downsample_kernel<<<dim3(blocks(maxW, 256), (unsigned)maxH, (unsigned)D.nImages), 256, 0, s>>>(D, o, nl);
}

void launch_sift_batch_extrema(const SiftBatchDevice& D, int o, int nl, float thr, int maxW, int maxH, hipStream_t s) {
    sift_batch_extrema_kernel<<<dim3(blocks(maxW, 64), blocks(maxH, 4), (unsigned)D.nImages), 256, 0, s>>>(D, o, nl,
                                                                                                          thr);
}

void launch_sift_batch_refine(const SiftBatchDevice& D, const SiftParams& P, int nC, SiftKp* d_kps, hipStream_t s) {
    sift_batch_refine_kernel<<<blocks(nC, 256), 256, 0, s>>>(D, P, nC, d_kps);
}

void launch_sift_batch_orient(const SiftBatchDevice& D, const SiftKp* d_kps, int nC, SiftRec* d_recs,
                              unsigned long long* d_keys, unsigned long long* d_starts, unsigned long long* d_rkeys,
                              hipStream_t s) {
    sift_batch_orient_kernel<<<blocks(nC, 4), 256, 0, s>>>(D, d_kps, nC, d_recs, d_keys, d_starts, d_rkeys);
}

void launch_sift_batch_order(const SiftBatchDevice& D, const SiftOrder& O, unsigned* d_pos, int n, int featureCount,
                             hipStream_t s) {
    scan<unsigned>(D.bcnt, D.nBuckets, D.part, D.boff, true, s);
    sift_batch_scatter_kernel<<<blocks(n, 256), 256, 0, s>>>(D, O.keys, n, O.perm);
    sift_batch_rank_kernel<<<blocks(n, 256), 256, 0, s>>>(D, O.keys, O.starts, O.rkeys, n, O.perm, O.sortedIdx, O.skeys,
                                                          O.srkeys, O.keepA);
    uint8_t* keep = O.keepA;
    if (featureCount > 0) {
        sift_batch_select_kernel<<<blocks(n, 256), 256, 0, s>>>(D, O.srkeys, O.skeys, O.keepA, n, featureCount, O.keepB);
        keep = O.keepB;
    }
    scan<uint8_t>(keep, n, D.part, d_pos, false, s);
    sift_batch_compact_kernel<<<blocks(n, 256), 256, 0, s>>>(keep, d_pos, O.sortedIdx, O.recs, n, O.out);
    sift_batch_offsets_kernel<<<blocks(D.nImages + 1, 256), 256, 0, s>>>(D, d_pos);
}

void launch_sift_batch_describe(const SiftBatchDevice& D, const SiftRec* d_recs, int n, int descType,
                                SiftKeyPointOut* d_kp, uint8_t* d_u8, float* d_f32, hipStream_t s) {
    sift_batch_describe_kernel<<<blocks(n, 4), 256, 0, s>>>(D, d_recs, n, descType, d_kp, d_u8, d_f32);
}

}  // namespace mcv
