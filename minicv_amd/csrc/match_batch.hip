// match_batch.hip — knn-2 matching, filtering and compaction for many image pairs in launches that do
// not grow with the number of pairs (host side: match_batch_host.cpp).
//
// All images' descriptor rows sit in one buffer, image after image. A directed problem is
// (query image, train image) as two row ranges of that buffer; with crossCheck the reverse problems are
// more entries of the same table. A host-built table maps workgroup -> (problem, query tile), the
// problems with the longest train sets first. A workgroup owns one query tile and walks all of its
// problem's train rows itself: no partials, no traffic between workgroups, no second launch, and the
// final idx, dist, idx2, dist2 of its queries are written directly. Both score forms are exact integers
// under the order (score, lowest train index), so the answer does not depend on the tile shape.
//
//   mcv_mb_prep        rows -> padded rows of KP bytes, once per image row: Hamming widths other than
//                      32 / 64 bytes are zero-padded, byte-SIFT rows are shifted (x ^ 0x80, read as int8)
//                      and get their i32 norm (the row layout and norms of mcv_l2u8_prep)
//   mcv_mb_hamming<W>  XOR / popcount: a wave = 64 queries, a query on each lane; the train rows are
//                      wave-uniform, so the compiler reads them through scalar loads. Keys are
//                      (distance << 22 | train index), as in match_hamming.hip. The loop ends at nt:
//                      the rows of the next image, right behind the last train row, are never read.
//   mcv_mb_l2u8<KP>    v_mfma_i32_32x32x32_i8 on the shifted bytes: 4 waves x 32 queries, the query
//                      fragments resident in VGPRs, a tile = 32 train rows read by the fragment rule of
//                      match_l2u8.hip (lane half h takes bytes 32 ks + 16 h .. + 15 of its row). The last
//                      tile is partial: its lanes past nt re-read row nt - 1 and their scores are masked
//                      to INT_MAX, which never enters the top-2 (strict <).
//   mcv_mb_filter      mcv_match_filter's rule over the concatenation of all problems' queries, plus the
//                      per-256 counts; mcv_mb_scan: one exclusive scan; mcv_mb_scatter: order-preserving
//                      compaction of (query, train) and dist; mcv_mb_offsets: the scan value at each
//                      problem's first query.
#include "kernels.h"
#include "mcv_runtime.h"
#include <climits>
#include <cmath>

namespace mcv {

typedef int intx4 __attribute__((ext_vector_type(4)));
typedef int intx16 __attribute__((ext_vector_type(16)));

static constexpr int kMbIdxBits = 22;
static constexpr uint32_t kMbIdxMask = (1u << kMbIdxBits) - 1;

// One lane owns 16 bytes of a padded row (G = KP / 16 lanes a row, G a power of two <= 32, so a row's
// lanes share a wave); the row's norm is the G lanes' xor tree.
__global__ __launch_bounds__(256) void mcv_mb_prep(const uint8_t* __restrict__ src, int rows, int dim, int KP,
                                                   unsigned flip, uint8_t* __restrict__ dst,
                                                   int* __restrict__ norms) {
    const int G = KP / 16;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long r = t / G;
    const int c = (int)(t % G);
    const bool live = r < rows;
    unsigned w[4] = {0u, 0u, 0u, 0u};
    if (live && dim % 16 == 0) {   // rows start at multiples of 16 bytes (the buffer itself is aligned)
        if (16 * c < dim) {
            const uint4 v = *reinterpret_cast<const uint4*>(src + (size_t)r * dim + 16 * c);
            const unsigned f4 = flip * 0x01010101u;
            w[0] = v.x ^ f4; w[1] = v.y ^ f4; w[2] = v.z ^ f4; w[3] = v.w ^ f4;
        }
    } else if (live) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int k = 16 * c + e;
            if (k < dim) w[e >> 2] |= (unsigned)(src[(size_t)r * dim + k] ^ flip) << (8 * (e & 3));
        }
    }
    int acc = 0;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int x = (int)(int8_t)(w[e >> 2] >> (8 * (e & 3)));
        acc += x * x;
    }
    for (int off = G / 2; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (!live) return;
    *reinterpret_cast<uint4*>(dst + (size_t)r * KP + 16 * c) = make_uint4(w[0], w[1], w[2], w[3]);
    if (norms && c == 0) norms[r] = acc;
}

// W = words per padded row (8: up to 32 bytes, 16: up to 64). One wave per workgroup.
template <int W>
__global__ __launch_bounds__(64) void mcv_mb_hamming(const uint32_t* __restrict__ rows,
                                                     const MatchBatchProblem* __restrict__ prob,
                                                     const int2* __restrict__ wg, int* __restrict__ idx,
                                                     int* __restrict__ dist, int* __restrict__ idx2,
                                                     int* __restrict__ dist2) {
    const int2 e = wg[blockIdx.x];
    const MatchBatchProblem P = prob[e.x];
    const int qi = e.y * kMatchBatchRowsHamming + (int)threadIdx.x;
    const int qs = min(qi, P.nq - 1);   // a workgroup exists only for nq > 0
    uint32_t qv[W];
    {
        const uint4* qrow = reinterpret_cast<const uint4*>(rows + (size_t)(P.qRow + qs) * W);
#pragma unroll
        for (int k = 0; k < W / 4; ++k) {
            const uint4 v = qrow[k];
            qv[4 * k] = v.x; qv[4 * k + 1] = v.y; qv[4 * k + 2] = v.z; qv[4 * k + 3] = v.w;
        }
    }
    const uint32_t* __restrict__ t = rows + (size_t)P.tRow * W;
    uint32_t m1 = 0xFFFFFFFFu, m2 = 0xFFFFFFFFu;
    auto row = [&](int j) __attribute__((always_inline)) {
        const uint32_t* td = t + (size_t)j * W;
        uint32_t d = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) d += (uint32_t)__popc(qv[w] ^ td[w]);
        const uint32_t key = (d << kMbIdxBits) | (uint32_t)j;
        m2 = min(m2, max(m1, key));
        m1 = min(m1, key);
    };
    int j = 0;
    for (; j + 4 <= P.nt; j += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) row(j + u);
    }
    for (; j < P.nt; ++j) row(j);
    if (qi >= P.nq) return;
    const size_t o = (size_t)P.outOff + qi;
    idx[o] = m1 == 0xFFFFFFFFu ? -1 : (int)(m1 & kMbIdxMask);
    dist[o] = m1 == 0xFFFFFFFFu ? INT_MAX : (int)(m1 >> kMbIdxBits);
    idx2[o] = m2 == 0xFFFFFFFFu ? -1 : (int)(m2 & kMbIdxMask);
    dist2[o] = m2 == 0xFFFFFFFFu ? INT_MAX : (int)(m2 >> kMbIdxBits);
}

// (score, index) order of match_l2u8.hip; index -1 (an empty slot) sorts last.
__device__ __forceinline__ bool mb_less(int a, int ia, int b, int ib) {
    return (a < b) | ((a == b) & ((unsigned)ia < (unsigned)ib));
}
__device__ __forceinline__ void mb_push(int& b1, int& i1, int& b2, int& i2, int s, int i) {
    const bool c1 = mb_less(s, i, b1, i1);
    const bool c2 = mb_less(s, i, b2, i2);
    const int nb2 = c1 ? b1 : (c2 ? s : b2);
    const int ni2 = c1 ? i1 : (c2 ? i : i2);
    b1 = c1 ? s : b1;
    i1 = c1 ? i : i1;
    b2 = nb2;
    i2 = ni2;
}
// Scores arriving in ascending index order: a later index never wins a tie.
__device__ __forceinline__ void mb_push_asc(int& b1, int& i1, int& b2, int& i2, int s, int i) {
    const bool c1 = s < b1, c2 = s < b2;
    const int nb2 = c1 ? b1 : (c2 ? s : b2);
    const int ni2 = c1 ? i1 : (c2 ? i : i2);
    b1 = c1 ? s : b1;
    i1 = c1 ? i : i1;
    b2 = nb2;
    i2 = ni2;
}

// rows: the shifted padded rows [R][KP]; norms[R]. A workgroup = 4 waves x 32 queries; there is no LDS
// and no barrier, so a wave without queries leaves at once.
template <int KP>
__global__ __launch_bounds__(256) void mcv_mb_l2u8(const uint8_t* __restrict__ rows, const int* __restrict__ norms,
                                                   const MatchBatchProblem* __restrict__ prob,
                                                   const int2* __restrict__ wg, int* __restrict__ idx,
                                                   float* __restrict__ dist, int* __restrict__ idx2,
                                                   float* __restrict__ dist2) {
    constexpr int KS = KP / 32;
    const int2 e = wg[blockIdx.x];
    const MatchBatchProblem P = prob[e.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, col = lane & 31;
    const int q0 = e.y * kMatchBatchRowsL2 + wave * 32;
    if (q0 >= P.nq) return;
    const int qi = q0 + col;
    const int qs = min(qi, P.nq - 1);

    // B fragments: query qs, bytes 32 ks + 16 h .. + 15
    intx4 b[KS];
    {
        const intx4* qrow = reinterpret_cast<const intx4*>(rows + (size_t)(P.qRow + qs) * KP + 16 * h);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) b[ks] = qrow[2 * ks];
    }
    int b1 = INT_MAX, b2 = INT_MAX, i1 = -1, i2 = -1;
    const int nt = P.nt, ntTiles = (nt + 31) / 32;
    const int* __restrict__ tn = norms + P.tRow;

    // A fragments of a tile: train row min(32 tile + col, nt - 1), the same bytes
    intx4 nxt[KS];
    auto aload = [&](int tile) __attribute__((always_inline)) {
        const int tr = min(tile * 32 + col, nt - 1);
        const intx4* arow = reinterpret_cast<const intx4*>(rows + (size_t)(P.tRow + tr) * KP + 16 * h);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) nxt[ks] = arow[2 * ks];
    };
    if (ntTiles > 0) aload(0);
    for (int tile = 0; tile < ntTiles; ++tile) {
        intx4 a[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) a[ks] = nxt[ks];
        // the next tile's loads in flight under this tile's MFMAs (the last trip reloads its own tile)
        aload(tile + 1 < ntTiles ? tile + 1 : tile);
        intx16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[ks], b[ks], acc, 0, 0, 0);
        // lane = query col, register r = train row 32 tile + (r & 3) + 8 (r >> 2) + 4 h, ascending per lane
        int sv[16];
        int mn = INT_MAX;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            const int n = tn[min(j, nt - 1)];
            sv[r] = j < nt ? n - 2 * acc[r] : INT_MAX;
            mn = min(mn, sv[r]);
        }
        if (mn < b2) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                mb_push_asc(b1, i1, b2, i2, sv[r], tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * h);
        }
    }
    // merge the two lane halves that hold the same query
    const int ob1 = __shfl_xor(b1, 32, 64), ob2 = __shfl_xor(b2, 32, 64);
    const int oi1 = __shfl_xor(i1, 32, 64), oi2 = __shfl_xor(i2, 32, 64);
    if (h != 0 || qi >= P.nq) return;
    mb_push(b1, i1, b2, i2, ob1, oi1);
    mb_push(b1, i1, b2, i2, ob2, oi2);
    const int qn = norms[P.qRow + qi];
    const size_t o = (size_t)P.outOff + qi;
    idx[o] = i1;
    dist[o] = i1 >= 0 ? (float)sqrt((double)(qn + b1)) : INFINITY;
    idx2[o] = i2;
    dist2[o] = i2 >= 0 ? (float)sqrt((double)(qn + b2)) : INFINITY;
}

// The forward problem that owns position g of the concatenated queries: the last p with qStart[p] <= g
// (empty problems share their start with the next one and are never the last).
__device__ __forceinline__ int mb_problem_of(const int* __restrict__ qStart, int B, int g) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (qStart[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// mcv_match_filter's rule, expression for expression, and the block's count of survivors. With cross,
// prob[B + p] is the reverse of problem p and its answers sit at its outOff in the same arrays.
__global__ __launch_bounds__(256) void mcv_mb_filter(const int* __restrict__ idx, const int* __restrict__ di1,
                                                     const int* __restrict__ di2, const float* __restrict__ df1,
                                                     const float* __restrict__ df2,
                                                     const MatchBatchProblem* __restrict__ prob,
                                                     const int* __restrict__ qStart, int B, int cross, int totalQ,
                                                     float ratio, float maxDist, uint8_t* __restrict__ keep,
                                                     int* __restrict__ cnt) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    bool k = false;
    if (g < totalQ) {
        const int j = idx[g];
        k = j >= 0;
        float d1, d2;
        if (di1) {
            d1 = (float)di1[g];
            d2 = di2[g] == INT_MAX ? INFINITY : (float)di2[g];
        } else {
            d1 = df1[g];
            d2 = df2[g];
        }
        if (ratio > 0) k = k && d1 < ratio * d2;
        if (maxDist > 0) k = k && d1 <= maxDist;
        if (cross && j >= 0) {
            const int p = mb_problem_of(qStart, B, g);
            k = k && idx[(size_t)prob[B + p].outOff + j] == g - qStart[p];
        }
        keep[g] = k ? 1 : 0;
    }
    const uint64_t bal = __ballot(k);
    __shared__ int w[4];
    if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = (int)__popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = w[0] + w[1] + w[2] + w[3];
}

// Exclusive scan of nb block counts in one block (sequential chunks of 1024, fixed order); off[nb] = total.
__global__ __launch_bounds__(1024) void mcv_mb_scan(const int* __restrict__ cnt, int nb, int* __restrict__ off) {
    __shared__ int sh[1024];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nb; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < nb ? cnt[i] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const int t = threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
            __syncthreads();
            sh[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < nb) off[i] = carry + sh[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += sh[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) off[nb] = carry;
}

__global__ __launch_bounds__(256) void mcv_mb_scatter(const uint8_t* __restrict__ keep, const int* __restrict__ idx,
                                                      const int* __restrict__ di1, const float* __restrict__ df1,
                                                      const int* __restrict__ off, const int* __restrict__ qStart,
                                                      int B, int totalQ, int* __restrict__ pairs,
                                                      float* __restrict__ dist) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    const bool k = g < totalQ && keep[g];
    const uint64_t bal = __ballot(k);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __shared__ int w[4];
    if (lane == 0) w[wv] = (int)__popcll(bal);
    __syncthreads();
    int base = off[blockIdx.x];
    for (int q = 0; q < wv; ++q) base += w[q];
    if (!k) return;
    const int pos = base + (int)__popcll(bal & ((1ull << lane) - 1));
    const int p = mb_problem_of(qStart, B, g);
    pairs[2 * (size_t)pos] = g - qStart[p];
    pairs[2 * (size_t)pos + 1] = idx[g];
    dist[pos] = di1 ? (float)di1[g] : df1[g];
}

// offsets[p] = the scan value at problem p's first query (p = B: the total).
__global__ __launch_bounds__(256) void mcv_mb_offsets(const uint8_t* __restrict__ keep, const int* __restrict__ off,
                                                      const int* __restrict__ qStart, int B, int totalQ,
                                                      int* __restrict__ offsets) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p > B) return;
    const int g = p < B ? qStart[p] : totalQ;
    const int blk = g >> 8;
    int v = off[blk];   // g == totalQ a multiple of 256: off[nb], the total
    for (int i = blk << 8; i < g; ++i) v += keep[i];
    offsets[p] = v;
}

void launch_match_batch_prep(const uint8_t* d_src, int rows, int dim, int KP, bool shift, uint8_t* d_dst,
                             int* d_norms, hipStream_t s) {
    if (rows <= 0) return;
    const long long threads = (long long)rows * (KP / 16);
    hipLaunchKernelGGL(mcv_mb_prep, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, d_src, rows, dim, KP,
                       shift ? 0x80u : 0u, d_dst, shift ? d_norms : nullptr);
}

void launch_match_batch_hamming(const uint8_t* d_rows, int W, const MatchBatchProblem* d_prob, const int* d_wg,
                                int nwg, int* d_idx, int* d_dist, int* d_idx2, int* d_dist2, hipStream_t s) {
    if (nwg <= 0) return;
    if (W == 8)
        hipLaunchKernelGGL(mcv_mb_hamming<8>, dim3(nwg), dim3(64), 0, s, (const uint32_t*)d_rows, d_prob,
                           (const int2*)d_wg, d_idx, d_dist, d_idx2, d_dist2);
    else
        hipLaunchKernelGGL(mcv_mb_hamming<16>, dim3(nwg), dim3(64), 0, s, (const uint32_t*)d_rows, d_prob,
                           (const int2*)d_wg, d_idx, d_dist, d_idx2, d_dist2);
}

template <int KP>
static void mb_l2u8_launch(const uint8_t* d_rows, const int* d_norms, const MatchBatchProblem* d_prob, const int* d_wg,
                           int nwg, int* d_idx, float* d_dist, int* d_idx2, float* d_dist2, hipStream_t s) {
    hipLaunchKernelGGL(mcv_mb_l2u8<KP>, dim3(nwg), dim3(256), 0, s, d_rows, d_norms, d_prob, (const int2*)d_wg, d_idx,
                       d_dist, d_idx2, d_dist2);
}

void launch_match_batch_l2u8(const uint8_t* d_rows, const int* d_norms, int KP, const MatchBatchProblem* d_prob,
                             const int* d_wg, int nwg, int* d_idx, float* d_dist, int* d_idx2, float* d_dist2,
                             hipStream_t s) {
    if (nwg <= 0) return;
    switch (KP) {
        case 32: mb_l2u8_launch<32>(d_rows, d_norms, d_prob, d_wg, nwg, d_idx, d_dist, d_idx2, d_dist2, s); break;
        case 64: mb_l2u8_launch<64>(d_rows, d_norms, d_prob, d_wg, nwg, d_idx, d_dist, d_idx2, d_dist2, s); break;
        case 128: mb_l2u8_launch<128>(d_rows, d_norms, d_prob, d_wg, nwg, d_idx, d_dist, d_idx2, d_dist2, s); break;
        case 256: mb_l2u8_launch<256>(d_rows, d_norms, d_prob, d_wg, nwg, d_idx, d_dist, d_idx2, d_dist2, s); break;
        case 512: mb_l2u8_launch<512>(d_rows, d_norms, d_prob, d_wg, nwg, d_idx, d_dist, d_idx2, d_dist2, s); break;
        default: fail("launch_match_batch_l2u8: KP %d", KP);
    }
}

// Four launches over the totalQ > 0 concatenated forward queries; d_off[nb] and d_offsets[B] = the total.
void launch_match_batch_compact(const int* d_idx, const int* d_di1, const int* d_di2, const float* d_df1,
                                const float* d_df2, const MatchBatchProblem* d_prob, const int* d_qStart, int B,
                                bool cross, int totalQ, float ratio, float maxDist, uint8_t* d_keep, int* d_cnt,
                                int* d_off, int* d_pairs, float* d_dist, int* d_offsets, hipStream_t s) {
    const int nb = (totalQ + 255) / 256;
    hipLaunchKernelGGL(mcv_mb_filter, dim3(nb), dim3(256), 0, s, d_idx, d_di1, d_di2, d_df1, d_df2, d_prob, d_qStart, B,
                       cross ? 1 : 0, totalQ, ratio, maxDist, d_keep, d_cnt);
    hipLaunchKernelGGL(mcv_mb_scan, dim3(1), dim3(1024), 0, s, d_cnt, nb, d_off);
    hipLaunchKernelGGL(mcv_mb_scatter, dim3(nb), dim3(256), 0, s, d_keep, d_idx, d_di1, d_df1, d_off, d_qStart, B,
                       totalQ, d_pairs, d_dist);
    hipLaunchKernelGGL(mcv_mb_offsets, dim3((B + 256) / 256), dim3(256), 0, s, d_keep, d_off, d_qStart, B, totalQ,
                       d_offsets);
}

}  // namespace mcv
