// ransac_h_mfma.hip — the certified homography sweep with W, U, V on the bf16 matrix cores of gfx950:
// the exact three-piece bf16 split, the point records (mcv_h_rec), the fragment builders, the sweep
// (mcv_h_verify_mfma, whole or as one stage of the staged sweep), its test kernel (mcv_h_mfma_wuv) and
// the size rule that engages it. The certificate itself is h_cert.h's, shared with the VALU sweep.
#include "mcv_common.h"
#include "hyp_homography.h"
#include "h_cert.h"

namespace mcv {

// ------------------------------------------------------------------------------------------
// The certified sweep with W, U, V on the bf16 matrix cores (mcv_h_verify_mfma). A wave takes 32
// hypotheses x 32 correspondences per tile: one v_mfma_f32_32x32x16_bf16 per affine form, then the
// certificate of mcv_h_verify_cert (DX .. X, the two compares) on the accumulators, lane =
// correspondence, register = hypothesis, packed over register pairs (two hypotheses).
// Operands: every f32 v is split exactly into three bf16 pieces, each rounded to nearest,
// v = v1 + v2 + v3 (bf16 keeps the f32 exponent range); a product h x keeps the six piece products
// (1,1) (1,2) (2,1) (1,3) (3,1) (2,2). The 16 k-slots, lane half 0 / 1 = slots 0..7 / 8..15:
//   half 0: the six products of the x term, then c1 . 1, c2 . 1   (c = the constant h2 / h5 / 1)
//   half 1: the six products of the y term, then c3 . 1, 0 . 1
// so a lane's B fragment is {p1 p2 | p1 p3 | p1 p2 | 1 1} of its half's coordinate: two stored words.
// Rows with an undecided lane add nothing in the sweep; they are logged (tile << 5 | row) and
// recounted after it with the exact h_error over the tile's 32 correspondences.
// ------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t bf16_rn_bits(float v) {   // round to nearest even (finite v)
    const uint32_t b = __float_as_uint(v);
    return (b + 0x7FFFu + ((b >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ float bf16_value(uint32_t p) { return __uint_as_float(p << 16); }
// v - v1 and (v - v1) - v2 are exact in f32, and the last remainder has at most 8 significant bits
__device__ __forceinline__ void bf16_split3(float v, uint32_t& p1, uint32_t& p2, uint32_t& p3) {
    p1 = bf16_rn_bits(v);
    const float r1 = v - bf16_value(p1);
    p2 = bf16_rn_bits(r1);
    const float r2 = r1 - bf16_value(p2);
    p3 = bf16_rn_bits(r2);
}

static int h_rec_pad(int N) { return (N + 31) / 32 * 32; }
size_t h_rec_bytes(int N) { return (size_t)h_rec_pad(N) * 24; }

// Point records: pieces[2 i + half] = {p1 | p2 << 16, p1 | p3 << 16} of x (half 0) / y (half 1),
// mxy[i] = {x', y'}; the pad up to a multiple of 32 has zero pieces and NaN x', y' (a NaN error:
// never an inlier, never undecided).
__global__ __launch_bounds__(256) void mcv_h_rec(const float4* __restrict__ pts, int N, int nPad,
                                                 uint2* __restrict__ pieces, f2* __restrict__ mxy) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nPad) return;
    const float nan = __builtin_nanf("");
    uint2 wx = make_uint2(0u, 0u), wy = make_uint2(0u, 0u);
    f2 m = f2{nan, nan};
    if (i < N) {
        const float4 q = pts[i];
        uint32_t p1, p2, p3;
        bf16_split3(q.x, p1, p2, p3);
        wx = make_uint2(p1 | (p2 << 16), p1 | (p3 << 16));
        bf16_split3(q.y, p1, p2, p3);
        wy = make_uint2(p1 | (p2 << 16), p1 | (p3 << 16));
        m = f2{q.z, q.w};
    }
    pieces[2 * i] = wx;
    pieces[2 * i + 1] = wy;
    mxy[i] = m;
}

// A fragment of one affine form for the lane's hypothesis: coef = the coefficient of the lane half's
// coordinate, cst = the form's constant term.
__device__ __forceinline__ bf16x8 h_mfma_a_frag(float coef, float cst, int half) {
    uint32_t a1, a2, a3, c1, c2, c3;
    bf16_split3(coef, a1, a2, a3);
    bf16_split3(cst, c1, c2, c3);
    const u32x4 w = {a1 | (a1 << 16), a2 | (a1 << 16), a3 | (a2 << 16), half ? c3 : (c1 | (c2 << 16))};
    return __builtin_bit_cast(bf16x8, w);
}
__device__ __forceinline__ bf16x8 h_mfma_b_frag(uint2 rec) {
    const u32x4 w = {rec.x, rec.y, rec.x, 0x3F803F80u};
    return __builtin_bit_cast(bf16x8, w);
}
// accumulator register i of lane half `half` holds hypothesis row:
__device__ __forceinline__ constexpr int h_mfma_row(int i, int half) { return (i & 3) + 8 * (i >> 2) + 4 * half; }

struct HMfmaFrags {
    bf16x8 w, u, v;
};
__device__ __forceinline__ HMfmaFrags h_mfma_frags(const HModelF& m, int half) {
    HMfmaFrags a;
    a.w = h_mfma_a_frag(half ? m.h[7] : m.h[6], 1.0f, half);
    a.u = h_mfma_a_frag(half ? m.h[1] : m.h[0], m.h[2], half);
    a.v = h_mfma_a_frag(half ? m.h[4] : m.h[3], m.h[5], half);
    return a;
}
__device__ __forceinline__ f32x16 h_mfma_dot(bf16x8 a, bf16x8 b) {
    const f32x16 z = {0};
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, z, 0, 0, 0);
}

static constexpr int kMfmaEvents = 1024;   // per wave

// __launch_bounds__(256, 2): a register budget of 256 makes the compiler keep the accumulators in
// VGPRs (with 512 it places them in AGPRs and copies all 48 out with v_accvgpr_read every tile).

template <bool STAGED>
__global__ __launch_bounds__(256, 2) void mcv_h_verify_mfma(const uint2* __restrict__ pieces, const f2* __restrict__ mxy,
                                                         const float4* __restrict__ pts, int N,
                                                         const HModelF* __restrict__ models, int* __restrict__ counts,
                                                         int hypCount, float thr2, HCertSlopes slopes,
                                                         const double* __restrict__ bb, HStageArgs sa,
                                                         unsigned long long* __restrict__ stats) {
    __shared__ uint32_t events[4][kMfmaEvents];
    const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * 256u + threadIdx.x) >> 6));
    const int wib = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int row = lane & 31, half = lane >> 5;
    const int h0 = wave * 32;
    const int nTiles = (N + 31) / 32;
    int tBeg = 0, tEnd = nTiles;
    if constexpr (STAGED) {
        // stage boundaries are multiples of 64 pairs = 4 tiles, except the last one (the pair count)
        const int pBeg = sa.ctl[kCtlBound + sa.stage], pEnd = sa.ctl[kCtlBound + sa.stage + 1];
        if (pBeg >= pEnd) return;
        if (sa.list) hypCount = sa.ctl[kCtlAlive + sa.stage];
        tBeg = pBeg / 16;
        tEnd = pEnd >= (N + 1) / 2 ? nTiles : pEnd / 16;
    }
    if (h0 >= hypCount) return;

    // lane = hypothesis row (both halves): its slot, model, offsets and A fragments
    const int hk = h0 + row;
    const int ent = hk < hypCount ? hk : hypCount - 1;
    int slot = ent;
    if constexpr (STAGED) slot = sa.list ? sa.list[ent] : ent;
    const bool valid = hk < hypCount && counts[slot] >= 0;
    const HModelF m = models[slot];
    double b4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) b4[j] = bb[j];
    f2 cb;
    const bool ok = h_cert_offsets<true>(m.h, b4, thr2, slopes.t, cb);
    bool fast = __builtin_amdgcn_ballot_w64(valid && !ok) == 0;
    const bool inDomain = fast;
    // bit r: row r is written (a slot below hypCount that holds a model); only those rows log events
    const uint32_t vrows = (uint32_t)__builtin_amdgcn_ballot_w64(valid);
    const HMfmaFrags A = h_mfma_frags(m, half);
    // {b_in, b_x} of the rows this lane's accumulator registers hold, as pairs of registers
    f2 bin2[8], bx2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int r0 = h_mfma_row(2 * j, 0) + 4 * half, r1 = h_mfma_row(2 * j + 1, 0) + 4 * half;
        bin2[j] = f2{__shfl(cb.x, r0, 64), __shfl(cb.x, r1, 64)};
        bx2[j] = f2{__shfl(cb.y, r0, 64), __shfl(cb.y, r1, 64)};
    }

    uint32_t cnt[32];
#pragma unroll
    for (int r = 0; r < 32; ++r) cnt[r] = 0;
    int nev = 0;
    uint32_t extra = 0;   // lane r: the recounted rows of hypothesis row r
    if (fast) {
        uint2 rec = pieces[(size_t)tBeg * 64 + row * 2 + half];   // [2 (32 t + row) + half]
        f2 q = mxy[(size_t)tBeg * 32 + row];
        for (int t = tBeg; t < tEnd; ++t) {
            const bf16x8 B = h_mfma_b_frag(make_uint2(rec.x, rec.y));
            const f2 qc = q;
            const int tn = t + 1 < tEnd ? t + 1 : t;
            rec = pieces[(size_t)tn * 64 + row * 2 + half];
            q = mxy[(size_t)tn * 32 + row];
            const f32x16 W = h_mfma_dot(A.w, B), U = h_mfma_dot(A.u, B), V = h_mfma_dot(A.v, B);
#pragma unroll
            for (int jj = 0; jj < 8; jj += 2) {
                // masks of the accumulator registers 2 jj .. 2 jj + 3; mask halves = the rows r and r + 4 of
                // a register. Every row counts its certified inliers at once; the rare branch (one per four
                // registers) takes back a row with an undecided lane and logs it.
                uint64_t in[4], un[4];
#pragma unroll
                for (int d = 0; d < 2; ++d) {
                    const int j = jj + d;
                    const f2 W2 = f2{W[2 * j], W[2 * j + 1]}, U2 = f2{U[2 * j], U[2 * j + 1]},
                             V2 = f2{V[2 * j], V[2 * j + 1]};
                    const f2 DX = pk_fma(-lo(qc), W2, U2);
                    const f2 DY = pk_fma(-hi(qc), W2, V2);
                    const f2 L = pk_fma(DX, DX, pk_fma(DY, DY, bin2[j]));
                    const f2 WW = W2 * W2;
                    const f2 I = pk_fma(WW, lo(slopes.a), L);
                    const f2 X = pk_fma(WW, hi(slopes.a), bx2[j]);
                    in[2 * d] = __builtin_amdgcn_ballot_w64(I.x < 0.0f);
                    in[2 * d + 1] = __builtin_amdgcn_ballot_w64(I.y < 0.0f);
                    un[2 * d] = __builtin_amdgcn_ballot_w64(__float_as_uint(I.x) <= __float_as_uint(X.x));
                    un[2 * d + 1] = __builtin_amdgcn_ballot_w64(__float_as_uint(I.y) <= __float_as_uint(X.y));
                    const int ra = h_mfma_row(2 * j, 0), rb = h_mfma_row(2 * j + 1, 0);
                    cnt[ra] += (uint32_t)__builtin_popcount((uint32_t)in[2 * d]);
                    cnt[ra + 4] += (uint32_t)__builtin_popcount((uint32_t)(in[2 * d] >> 32));
                    cnt[rb] += (uint32_t)__builtin_popcount((uint32_t)in[2 * d + 1]);
                    cnt[rb + 4] += (uint32_t)__builtin_popcount((uint32_t)(in[2 * d + 1] >> 32));
                }
                if (__builtin_expect((un[0] | un[1] | un[2] | un[3]) != 0, 0)) {
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        const int r = h_mfma_row(2 * jj + (c >> 1), 0) + 4 * (c & 1);
                        const uint32_t um = (uint32_t)(c & 1 ? un[c >> 1] >> 32 : un[c >> 1]);
                        const uint32_t im = (uint32_t)(c & 1 ? in[c >> 1] >> 32 : in[c >> 1]);
                        if (um != 0 && (vrows & (1u << r)) != 0) {
                            if (lane == r) extra -= (uint32_t)__builtin_popcount(im);   // lane r: row r's corrections
                            if (nev < kMfmaEvents) {
                                if (lane == 0) events[wib][nev] = ((uint32_t)t << 5) | (uint32_t)r;
                            }
                            ++nev;
                        }
                    }
                }
            }
        }
        if (nev > kMfmaEvents) fast = false;   // too many to recount here: exact recount of the wave's slots
        else if (nev > 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // two logged rows per pass: lane half 0 recounts event e, half 1 event e + 1 (lane & 31 = the
            // tile's correspondence)
            for (int e = 0; e < nev; e += 2) {
                const bool have = e + half < nev;
                const uint32_t ev = events[wib][have ? e + half : e];
                const int r = (int)(ev & 31u);
                const int sl = __shfl(slot, r, 64);
                const HModelF mm = models[sl];
                const int p = (int)(ev >> 5) * 32 + row;
                bool in = false;
                if (have && p < N) {
                    const float4 c = pts[p];
                    in = h_error(mm.h, c.x, c.y, c.z, c.w) <= thr2;
                }
                const uint64_t b = __builtin_amdgcn_ballot_w64(in);
                const int r0 = __builtin_amdgcn_readlane(r, 0), r1 = __builtin_amdgcn_readlane(r, 32);
                if (lane == r0) extra += (uint32_t)__builtin_popcount((uint32_t)b);
                if (lane == r1) extra += (uint32_t)__builtin_popcount((uint32_t)(b >> 32));
            }
        }
    }
    uint32_t tot = extra;
#pragma unroll
    for (int r = 0; r < 32; ++r) tot += lane == r ? cnt[r] : 0u;
    if (lane < 32 && valid) {
        if constexpr (STAGED)
            counts[slot] = fast ? counts[slot] + (int)tot : kStatusRedo;
        else
            counts[slot] = fast ? (int)tot : kStatusRedo;
    }
    // stats: [0] undecided rows logged, [1] waves whose event list overflowed, [2] waves outside the domain
    if (lane == 0 && nev > 0) {
        atomicAdd(stats, (unsigned long long)nev);
        if (nev > kMfmaEvents) atomicAdd(stats + 1, 1ull);
    }
    if (lane == 0 && !inDomain) atomicAdd(stats + 2, 1ull);
}

// W, U, V of the matrix-core form (mcvTestHMfmaWuv): the same fragments and the same instruction.
__global__ __launch_bounds__(256, 2) void mcv_h_mfma_wuv(const uint2* __restrict__ pieces, int N,
                                                      const HModelF* __restrict__ models, int nModels,
                                                      float* __restrict__ out) {
    const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * 256u + threadIdx.x) >> 6));
    const int lane = threadIdx.x & 63;
    const int row = lane & 31, half = lane >> 5;
    const int h0 = wave * 32;
    if (h0 >= nModels) return;
    const HModelF m = models[h0 + row < nModels ? h0 + row : nModels - 1];
    const HMfmaFrags A = h_mfma_frags(m, half);
    const int nTiles = (N + 31) / 32;
    for (int t = 0; t < nTiles; ++t) {
        const bf16x8 B = h_mfma_b_frag(pieces[(size_t)t * 64 + row * 2 + half]);
        const f32x16 W = h_mfma_dot(A.w, B), U = h_mfma_dot(A.u, B), V = h_mfma_dot(A.v, B);
        const int p = t * 32 + row;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int hk = h0 + h_mfma_row(i, 0) + 4 * half;
            if (p < N && hk < nModels) {
                float* o = out + ((size_t)hk * N + p) * 3;
                o[0] = W[i];
                o[1] = U[i];
                o[2] = V[i];
            }
        }
    }
}

void launch_h_rec(const float* d_pts4, int N, void* d_rec, hipStream_t s) {
    const int nPad = h_rec_pad(N);
    hipLaunchKernelGGL(mcv_h_rec, dim3((nPad + 255) / 256), dim3(256), 0, s, (const float4*)d_pts4, N, nPad,
                       (uint2*)d_rec, (f2*)((char*)d_rec + (size_t)nPad * 16));
}

// The size rule of the matrix-core form (form = kHFormAuto): the staged sweep of large calls. A wave holds
// 32 hypotheses, so small calls leave most of the chip idle, and an unstaged sweep of 100k points
// overflows event lists and does not win. Staged, screened at N = 5000 / 20000 / 100000: it wins from
// 2^19 hypotheses at every N and loses at 2^18 x 100000 (the engage-rule screens).
static constexpr int kHMfmaMinHyp = 1 << 19;
static constexpr int kHMfmaMinN = kHStageMinN;
bool h_mfma_engages(int N, int hypCount, int form, bool staged) {
    if (form == kHFormValu) return false;
    if (form == kHFormMfma || form == kHFormMixed) return true;
    return staged && hypCount >= kHMfmaMinHyp && N >= kHMfmaMinN;
}

void launch_h_mfma_sweep(const float* d_pts4, const void* d_rec, int N, const void* d_models, int* d_counts,
                         int hypCount, float thr2, const HCertSlopes& slopes, const double* d_bb, HStageArgs sa,
                         unsigned long long* d_stats, hipStream_t s) {
    const int waves = (hypCount + 31) / 32;
    const int blocks = (waves + 3) / 4;
    const int nPad = h_rec_pad(N);
    auto* kernel = sa.ctl ? mcv_h_verify_mfma<true> : mcv_h_verify_mfma<false>;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, s, (const uint2*)d_rec,
                       (const f2*)((const char*)d_rec + (size_t)nPad * 16), (const float4*)d_pts4, N,
                       (const HModelF*)d_models, d_counts, hypCount, thr2, slopes, d_bb, sa, d_stats);
}

void launch_h_mfma_wuv(const void* d_rec, int N, const void* d_models, int nModels, float* d_wuv, hipStream_t s) {
    const int waves = (nModels + 31) / 32;
    hipLaunchKernelGGL(mcv_h_mfma_wuv, dim3((waves + 3) / 4), dim3(256), 0, s, (const uint2*)d_rec, N,
                       (const HModelF*)d_models, nModels, d_wuv);
}

}  // namespace mcv
