// match_l2u8.hip — exact brute-force L2 matcher for uint8 descriptors on the int8 matrix cores
// (cv::BFMatcher(NORM_L2).knnMatch(k = 2) on CV_8U rows: byte SIFT, the reference's default
// descriptor type; layout = DetectorResult row-major [n][dim] uint8).
//
//   x' = x - 128 (the byte XOR 0x80, read as int8):  q - t = q' - t', so
//   |q - t|^2 = |q'|^2 + |t'|^2 - 2 q'.t', every term an exact integer in i32 for dim <= 512:
//   |q'.t'| <= 512 * 128^2 = 2^23, |x'|^2 <= 2^23, d^2 <= 512 * 255^2 < 2^25.
//   argmin over t needs only s(t) = |t'|^2 - 2 q'.t' (in [-2^23, 2^25), exact).
//
// Because the GEMM-form score is the exact squared distance minus a per-query constant, its top-2
// under the key (s, train index) is the answer: there is no fp64 re-rank, no tolerance and no exact
// scan (match_l2.hip needs all three only because fp32 products round). Integer keys also make the
// result independent of how the train set is cut into chunks and of the order the partials are folded.
//
// mcv_l2u8_prep: shifted copies [nPad][KP] (KP = dim rounded up to the template's K; the padding
//   bytes are 0 in the shifted domain, so they add nothing to q'.t' or to the norms; padding rows are
//   all zero) and the i32 norms sum x'^2; padding train rows get the norm INT_MAX, hence the score
//   INT_MAX, which never beats anything (strict <) and leaves index -1 in an empty slot.
// mcv_l2u8_gemm<KP, NC>: v_mfma_i32_32x32x32_i8. A = 32 train rows of a tile (LDS), B = the wave's 32
//   queries, VGPR-resident for the whole kernel (4 VGPRs per 32 k). The 32x32 accumulator puts a query
//   on each lane (col = lane & 31) and 16 train rows in its registers (row = (r & 3) + 8 (r >> 2) +
//   4 (lane >> 5)), so the top-2 is lane-local: rows arrive in ascending index order per lane, the two
//   lane halves that share a query are merged once at the end. A and B fragments are loaded by one and
//   the same rule (lane half h takes bytes 32 ks + 16 h .. + 15 of its row), so the product does not
//   depend on the order of k inside an instruction, only on both operands using the same one.
//   A block = 4 waves = 128 queries; a tile = TR = 32 NC train rows (NC independent accumulator
//   chains sharing the query operands); tiles are double-buffered in LDS (row stride KP + 16 bytes:
//   the b128 fragment reads of consecutive rows fall in distinct bank groups), register-staged, one
//   barrier per tile. Grid = query blocks x train chunks; each (query, chunk) leaves (s1, s2, i1, i2).
// mcv_l2u8_merge: folds the chunks' partials by (s, index), adds |q'|^2 and writes
//   dist = (float)sqrt((double)d^2): mcv_l2_refine's final expression on the same integer.
#include "kernels.h"
#include "mcv_runtime.h"
#include <algorithm>
#include <climits>
#include <cmath>

namespace mcv {

typedef int intx4 __attribute__((ext_vector_type(4)));
typedef int intx16 __attribute__((ext_vector_type(16)));

static constexpr int kL2U8MaxDim = 512;
static constexpr int kL2U8MaxRows = 1 << 24;   // nq and nt: a padded copy is at most 2^33 bytes
static constexpr int kL2U8PrepBlocks = 4096;

// (score, index) order; index -1 (an empty slot) sorts last.
__device__ __forceinline__ bool l2u8_less(int a, int ia, int b, int ib) {
    return (a < b) | ((a == b) & ((unsigned)ia < (unsigned)ib));
}

// Branchless top-2 insertion under the (score, index) order, any arrival order.
__device__ __forceinline__ void l2u8_push(int& b1, int& i1, int& b2, int& i2, int s, int i) {
    const bool c1 = l2u8_less(s, i, b1, i1);
    const bool c2 = l2u8_less(s, i, b2, i2);
    const int nb2 = c1 ? b1 : (c2 ? s : b2);
    const int ni2 = c1 ? i1 : (c2 ? i : i2);
    b1 = c1 ? s : b1;
    i1 = c1 ? i : i1;
    b2 = nb2;
    i2 = ni2;
}

// The same for scores arriving in ascending index order: a later index never wins a tie, so the
// strict < on the score decides (2 v_cmp + 6 v_cndmask, no divergent branch).
__device__ __forceinline__ void l2u8_push_asc(int& b1, int& i1, int& b2, int& i2, int s, int i) {
    const bool c1 = s < b1, c2 = s < b2;
    const int nb2 = c1 ? b1 : (c2 ? s : b2);
    const int ni2 = c1 ? i1 : (c2 ? i : i2);
    b1 = c1 ? s : b1;
    i1 = c1 ? i : i1;
    b2 = nb2;
    i2 = ni2;
}

struct L2U8Prep {
    const uint8_t* src;
    int n, nPad;
    uint8_t* dst;
    int* norms;
    int padNorm;
};

// One launch covers both sets (rows of q, then rows of t; grid-stride). A lane owns 16 bytes of a
// padded row (G = KP / 16 lanes a row, 64 / G rows per wave-trip); vec (dim % 16 == 0, 16-byte
// aligned sets): one 16-byte load, else byte loads. The row's norm is the G lanes' xor tree.
__global__ __launch_bounds__(256) void mcv_l2u8_prep(L2U8Prep q, L2U8Prep t, int dim, int KP, int vec) {
    const int lane = threadIdx.x & 63;
    const int G = KP / 16, RW = 64 / G;
    const int sub = lane / G, c = lane % G;
    const int nrows = q.nPad + t.nPad;   // both multiples of RW
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), nw = gridDim.x * 4;
    for (int r0 = wave * RW; r0 < nrows; r0 += nw * RW) {
        const int rr = r0 + sub;
        const bool isq = rr < q.nPad;
        const int r = isq ? rr : rr - q.nPad, n = isq ? q.n : t.n;
        const uint8_t* src = isq ? q.src : t.src;
        unsigned w[4] = {0u, 0u, 0u, 0u};
        if (r < n) {
            if (vec) {
                if (16 * c < dim) {
                    const uint4 v = *reinterpret_cast<const uint4*>(src + (size_t)r * dim + 16 * c);
                    w[0] = v.x ^ 0x80808080u; w[1] = v.y ^ 0x80808080u;
                    w[2] = v.z ^ 0x80808080u; w[3] = v.w ^ 0x80808080u;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int k = 16 * c + e;
                    if (k < dim) w[e >> 2] |= (unsigned)(src[(size_t)r * dim + k] ^ 0x80u) << (8 * (e & 3));
                }
            }
        }
        int acc = 0;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int x = (int)(int8_t)(w[e >> 2] >> (8 * (e & 3)));
            acc += x * x;
        }
        for (int off = G / 2; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
        uint8_t* dst = isq ? q.dst : t.dst;
        *reinterpret_cast<uint4*>(dst + (size_t)r * KP + 16 * c) = make_uint4(w[0], w[1], w[2], w[3]);
        if (c == 0) (isq ? q.norms : t.norms)[r] = r < n ? acc : (isq ? q.padNorm : t.padNorm);
    }
}

// Grid (query blocks of 128, train chunks of tilesPerChunk tiles). qp / tp: the shifted padded
// copies, tnorm: the train norms (INT_MAX on padding rows), part[chunk][nqPad].
template <int KP, int NC>
__global__ __launch_bounds__(256) void mcv_l2u8_gemm(const uint8_t* __restrict__ qp, const uint8_t* __restrict__ tp,
                                                     const int* __restrict__ tnorm, int ntTiles, int tilesPerChunk,
                                                     int nqPad, int4* __restrict__ part) {
    constexpr int TR = 32 * NC;                    // train rows per tile
    constexpr int KS = KP / 32;                    // MFMA k-steps
    constexpr int ROWB = KP + 16;                  // padded LDS row, bytes
    constexpr int TILEB = TR * KP;                 // tile bytes in the padded copy (contiguous)
    constexpr int PER = (TILEB + 4095) / 4096;     // 16-byte staging registers per thread
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * TR * ROWB];
    __shared__ __attribute__((aligned(16))) int lnorm[2 * TR];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, col = lane & 31;
    const int q0 = (blockIdx.x * 4 + wave) * 32;
    const int tBegin = blockIdx.y * tilesPerChunk, tEnd = min(tBegin + tilesPerChunk, ntTiles);

    // B fragments: query q0 + col, bytes 32 ks + 16 h .. + 15
    intx4 b[KS];
    {
        const intx4* qrow = reinterpret_cast<const intx4*>(qp + (size_t)(q0 + col) * KP + 16 * h);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) b[ks] = qrow[2 * ks];
    }

    int b1 = INT_MAX, b2 = INT_MAX, i1 = -1, i2 = -1;

    intx4 stg[PER];
    int nstg = 0;
    auto gload = [&](int tile) __attribute__((always_inline)) {
        const uint8_t* src = tp + (size_t)tile * TILEB;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int o = (threadIdx.x + 256 * j) * 16;
            if (TILEB % 4096 == 0 || o < TILEB) stg[j] = *reinterpret_cast<const intx4*>(src + o);
        }
        if (threadIdx.x < TR) nstg = tnorm[(size_t)tile * TR + threadIdx.x];
    };
    auto lstore = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int o = (threadIdx.x + 256 * j) * 16;
            if (TILEB % 4096 == 0 || o < TILEB)
                *reinterpret_cast<intx4*>(&lds[buf * TR * ROWB + (o / KP) * ROWB + (o % KP)]) = stg[j];
        }
        if (threadIdx.x < TR) lnorm[buf * TR + threadIdx.x] = nstg;
    };

    if (tBegin < tEnd) {
        gload(tBegin);
        lstore(0);
    }
    __syncthreads();
    for (int t = tBegin; t < tEnd; ++t) {
        const int buf = (t - tBegin) & 1;
        // the next tile's loads in flight under this tile's MFMAs (the last trip reloads its own tile
        // into the idle buffer: no branch around the staging registers)
        gload(t + 1 < tEnd ? t + 1 : t);
        // this lane's rows' norms: rows 8 j + 4 h .. + 3 of each chain
        intx4 nv[NC][4];
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                nv[c][j] = *reinterpret_cast<const intx4*>(&lnorm[buf * TR + 32 * c + 8 * j + 4 * h]);
        intx16 acc[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][r] = 0;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            intx4 a[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c)
                a[c] = *reinterpret_cast<const intx4*>(&lds[buf * TR * ROWB + (32 * c + col) * ROWB + 32 * ks + 16 * h]);
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[c] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[c], b[ks], acc[c], 0, 0, 0);
        }
        // epilogue: lane = query col, register r of chain c = train row 32 c + (r & 3) + 8 (r >> 2) + 4 h,
        // ascending per lane. One test per chain first: past the first tiles almost no chain holds a
        // score below the lane's second best, and the insertions are skipped.
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            int sv[16];
            int mn = INT_MAX;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sv[r] = nv[c][r >> 2][r & 3] - 2 * acc[c][r];
                mn = min(mn, sv[r]);
            }
            if (mn < b2) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    l2u8_push_asc(b1, i1, b2, i2, sv[r], t * TR + 32 * c + (r & 3) + 8 * (r >> 2) + 4 * h);
            }
        }
        lstore(buf ^ 1);
        __syncthreads();
    }
    // merge the two lane halves that hold the same query
    const int ob1 = __shfl_xor(b1, 32, 64), ob2 = __shfl_xor(b2, 32, 64);
    const int oi1 = __shfl_xor(i1, 32, 64), oi2 = __shfl_xor(i2, 32, 64);
    if (h == 0) {
        l2u8_push(b1, i1, b2, i2, ob1, oi1);
        l2u8_push(b1, i1, b2, i2, ob2, oi2);
        part[(size_t)blockIdx.y * nqPad + q0 + col] = make_int4(b1, b2, i1, i2);
    }
}

// One thread per query: fold the chunks' partials, add |q'|^2, write the four outputs.
__global__ __launch_bounds__(256) void mcv_l2u8_merge(const int4* __restrict__ part, int nq, int nqPad, int nchunks,
                                                      const int* __restrict__ qnorm, int* __restrict__ idx,
                                                      float* __restrict__ dist, int* __restrict__ idx2,
                                                      float* __restrict__ dist2) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    int b1 = INT_MAX, b2 = INT_MAX, i1 = -1, i2 = -1;
    for (int c = 0; c < nchunks; ++c) {
        const int4 p = part[(size_t)c * nqPad + q];
        l2u8_push(b1, i1, b2, i2, p.x, p.z);
        l2u8_push(b1, i1, b2, i2, p.y, p.w);
    }
    const int qn = qnorm[q];
    idx[q] = i1;
    dist[q] = i1 >= 0 ? (float)sqrt((double)(qn + b1)) : INFINITY;
    if (idx2) idx2[q] = i2;
    if (dist2) dist2[q] = i2 >= 0 ? (float)sqrt((double)(qn + b2)) : INFINITY;
}

struct L2U8Work {
    DevBuf<uint8_t> qp, tp;   // shifted padded copies
    DevBuf<int> qn, tn;       // i32 norms
    DevBuf<int4> part;        // [chunk][nqPad] partial top-2s
    StreamFence fence;        // calls on different streams take turns on these buffers
};

// The calling thread's workspace on the current device; it runs on the caller's stream and owns none.
static L2U8Work& l2u8_work() { return thread_device_ws<L2U8Work>(); }

void check_match_l2u8(const char* who, int nq, int nt, int dim) {
    if (dim < 1 || dim > kL2U8MaxDim) fail("%s: dim %d outside [1, %d]", who, dim, kL2U8MaxDim);
    if (nq > kL2U8MaxRows) fail("%s: nq %d above %d", who, nq, kL2U8MaxRows);
    if (nt > kL2U8MaxRows) fail("%s: nt %d above %d", who, nt, kL2U8MaxRows);
}

template <int KP, int NC>
static void l2u8_gemm_launch(const L2U8Work& wk, int qblocks, int nchunks, int ntTiles, int tilesPerChunk, int nqPad,
                             hipStream_t s) {
    hipLaunchKernelGGL((mcv_l2u8_gemm<KP, NC>), dim3(qblocks, nchunks), dim3(256), 0, s, wk.qp.p, wk.tp.p, wk.tn.p,
                       ntTiles, tilesPerChunk, nqPad, wk.part.p);
}

// Three launches, all on the caller's stream, no host round trip: prep -> gemm -> merge.
int launch_match_l2u8(const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int dim, int* d_idx, float* d_dist,
                      int* d_idx2, float* d_dist2, hipStream_t s) {
    check_match_l2u8("cvMatchL2U8", nq, nt, dim);
    if (nq <= 0) return 0;
    L2U8Work& wk = l2u8_work();
    wk.fence.enter(s);
    const int KP = dim <= 32 ? 32 : dim <= 64 ? 64 : dim <= 128 ? 128 : dim <= 256 ? 256 : 512;
    const int NC = KP <= 256 ? 2 : 1;   // 512: one chain keeps two blocks' LDS and registers per CU
    const int TR = 32 * NC;
    const int nqPad = (nq + 127) / 128 * 128;   // whole 128-query blocks
    const int ntPad = nt > 0 ? (nt + TR - 1) / TR * TR : TR;
    const int ntTiles = ntPad / TR;
    wk.qp.ensure((size_t)nqPad * KP);
    wk.tp.ensure((size_t)ntPad * KP);
    wk.qn.ensure(nqPad);
    wk.tn.ensure(ntPad);
    {
        const L2U8Prep pq{d_q, nq, nqPad, wk.qp.p, wk.qn.p, 0};
        const L2U8Prep pt{d_t, nt, ntPad, wk.tp.p, wk.tn.p, INT_MAX};
        const int vec = dim % 16 == 0 && (((uintptr_t)d_q | (uintptr_t)d_t) & 15) == 0;
        const int rowsPerBlock = 4 * (64 / (KP / 16));
        const int64_t rows = (int64_t)nqPad + ntPad;
        const int blocks = (int)std::min<int64_t>(kL2U8PrepBlocks, (rows + rowsPerBlock - 1) / rowsPerBlock);
        hipLaunchKernelGGL(mcv_l2u8_prep, dim3(blocks), dim3(256), 0, s, pq, pt, dim, KP, vec);
    }
    // train chunks: enough (query block, chunk) items to fill the device several times over, at
    // least 4 tiles each so small calls keep few partials per query
    const int qblocks = nqPad / 128;
    int nchunks = (2048 + qblocks - 1) / qblocks;
    nchunks = std::max(1, std::min(nchunks, (ntTiles + 3) / 4));
    const int tilesPerChunk = (ntTiles + nchunks - 1) / nchunks;
    nchunks = (ntTiles + tilesPerChunk - 1) / tilesPerChunk;
    wk.part.ensure((size_t)nchunks * nqPad);
    switch (KP) {
        case 32: l2u8_gemm_launch<32, 2>(wk, qblocks, nchunks, ntTiles, tilesPerChunk, nqPad, s); break;
        case 64: l2u8_gemm_launch<64, 2>(wk, qblocks, nchunks, ntTiles, tilesPerChunk, nqPad, s); break;
        case 128: l2u8_gemm_launch<128, 2>(wk, qblocks, nchunks, ntTiles, tilesPerChunk, nqPad, s); break;
        case 256: l2u8_gemm_launch<256, 2>(wk, qblocks, nchunks, ntTiles, tilesPerChunk, nqPad, s); break;
        default: l2u8_gemm_launch<512, 1>(wk, qblocks, nchunks, ntTiles, tilesPerChunk, nqPad, s); break;
    }
    hipLaunchKernelGGL(mcv_l2u8_merge, dim3((nq + 255) / 256), dim3(256), 0, s, wk.part.p, nq, nqPad, nchunks, wk.qn.p,
                       d_idx, d_dist, d_idx2, d_dist2);
    MCV_HIP(hipGetLastError());
    wk.fence.leave(s);
    return nq;
}

}  // namespace mcv
