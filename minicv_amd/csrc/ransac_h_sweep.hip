// ransac_h_sweep.hip — the homography inlier sweeps on gfx950: every hypothesis of a chunk against all N
// correspondences, one count per hypothesis.                              [SURVEY §2 K1, the hot loop]
//
//   mcv_h_verify<K, P>    the scalar sweep (either error), also the exact recount of kStatusRedo slots
//   mcv_h_verify_pk       the packed-f32 sweep of the fused error
//   mcv_h_verify_cert     the certified division-free sweep of the op-by-op error (the default), whole
//                         or as one stage of the staged sweep (ransac_h_stage.hip)
//   mcv_h_pair, mcv_bbox  the paired point layout and the source points' bounding box
// Built with -ffp-contract=off (see hyp_homography.h): the fp32 error rounds exactly like the host
// oracle, which is what makes the counts and the inlier masks bit-exact.
#include "mcv_common.h"
#include "hyp_homography.h"
#include "h_cert.h"

namespace mcv {

// ------------------------------------------------------------------------------------------
// Inlier sweep. Wave w evaluates hypotheses [w*K, w*K+K). The hypothesis index is made provably
// wave-uniform (readfirstlane), so the models come in through scalar loads and every VALU op
// reads its model coefficient straight from an SGPR; the counts accumulate in SGPRs too.
// ------------------------------------------------------------------------------------------
// Class mask of v_cmp_class_f32 for "not a normal number" (sNaN, qNaN, +-inf, +-denormal, +-0).
static constexpr int kClassNotNormal = 0x001 | 0x002 | 0x004 | 0x010 | 0x020 | 0x040 | 0x080 | 0x200;

// Wave mask of lanes whose w falls in the classes `cls`: one v_cmp_class_f32 writing an SGPR pair
// (the builtin + ballot pair lowers to cmp + cndmask + cmp on ROCm 7.2).
__device__ __forceinline__ uint64_t class_mask(float w, int cls) {
    uint64_t m;
    asm("v_cmp_class_f32_e64 %0, %1, %2" : "=s"(m) : "v"(w), "s"(cls));
    return m;
}

// One trip of the sweep: P correspondences per lane against the wave's K hypotheses.
// PRED: lane predicates (ragged tail only). FUSED fast path: rcp_newton, with the trip redone by
// IEEE division when any denominator is zero / denormal / non-finite.
template <int K, int P, bool FUSED, bool PRED>
__device__ __forceinline__ void h_sweep_trip(const float (&hm)[K][8], const float4 (&q)[P], const bool (&v)[P],
                                             float thr2, bool fast, uint32_t (&cnt)[K]) {
    auto vote = [&](int j, bool pred) -> uint32_t {
        if constexpr (PRED)
            return (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(v[j] && pred));
        else
            return (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(pred));
    };
    if constexpr (FUSED) {
        if (fast) {
            uint64_t bad = 0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
#pragma unroll
                for (int j = 0; j < P; ++j) {
                    const float w = h_denominator_fused(hm[k], q[j].x, q[j].y);
                    bad |= class_mask(w, kClassNotNormal);
                    const float e = h_error_fused_ww(hm[k], q[j].x, q[j].y, q[j].z, q[j].w, rcp_newton(w));
                    cnt[k] += vote(j, e <= thr2);
                }
            }
            if (__builtin_expect(bad == 0, 1)) return;
#pragma unroll
            for (int k = 0; k < K; ++k) {   // replace this trip's fast counts by the exact ones
#pragma unroll
                for (int j = 0; j < P; ++j) {
                    const float w = h_denominator_fused(hm[k], q[j].x, q[j].y);
                    const float f = h_error_fused_ww(hm[k], q[j].x, q[j].y, q[j].z, q[j].w, rcp_newton(w));
                    const float e = h_error_fused_ww(hm[k], q[j].x, q[j].y, q[j].z, q[j].w, 1.f / w);
                    cnt[k] = cnt[k] - vote(j, f <= thr2) + vote(j, e <= thr2);
                }
            }
            return;
        }
#pragma unroll
        for (int k = 0; k < K; ++k)   // exact for the whole wave
#pragma unroll
            for (int j = 0; j < P; ++j)
                cnt[k] += vote(j, h_error_fused(hm[k], q[j].x, q[j].y, q[j].z, q[j].w) <= thr2);
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int j = 0; j < P; ++j) cnt[k] += vote(j, h_error(hm[k], q[j].x, q[j].y, q[j].z, q[j].w) <= thr2);
    }
}

// redo: count only the slots the packed sweep marked kStatusRedo (a wave with none exits).
template <int K, int P, bool FUSED>
__global__ __launch_bounds__(256) void mcv_h_verify(const float4* __restrict__ pts, int N,
                                                    const HModelF* __restrict__ models, int* __restrict__ counts,
                                                    int hypCount, float thr2, const float* __restrict__ bbox,
                                                    int redo) {
    const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * 256u + threadIdx.x) >> 6));
    const int lane = threadIdx.x & 63;
    const int h0 = wave * K;
    if (h0 >= hypCount) return;

    float hm[K][8];
    bool valid[K];
    bool any = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int hk = h0 + k;
        valid[k] = (hk < hypCount) && (redo ? counts[hk] == kStatusRedo : counts[hk] >= 0);
        any = any || valid[k];
        const HModelF m = models[valid[k] ? hk : h0];
#pragma unroll
        for (int j = 0; j < 8; ++j) hm[k][j] = valid[k] ? m.h[j] : __builtin_nanf("");
        // h2 and h5 meet another uniform operand in fma(h1, y, h2) / fma(h4, y, h5); a VALU op
        // reads at most one SGPR (gfx9 constant-bus limit), so keep those two in VGPRs and the
        // other six in SGPRs (no per-use v_mov, and SGPR pressure stays below the spill point).
        asm volatile("" : "+v"(hm[k][2]));
        asm volatile("" : "+v"(hm[k][5]));
    }

    if (!any) return;
    uint32_t cnt[K];
#pragma unroll
    for (int k = 0; k < K; ++k) cnt[k] = 0;

    // Fused fast path precondition, per hypothesis: max |w| over the points' bounding box stays
    // below 2^125, so every denominator is below 2^126 (the exhaustively verified range of
    // rcp_newton). The lower end (0, denormal, inf, NaN) is checked per point.
    bool fast = FUSED;
    if constexpr (FUSED) {
        const float X = bbox[0], Y = bbox[1];
        bool anyValidBig = false;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float wmax = fabsf(hm[k][6]) * X + fabsf(hm[k][7]) * Y + 1.f;
            anyValidBig = anyValidBig || (valid[k] && !(wmax < 0x1p125f));
        }
        fast = !anyValidBig;
    }

    // Wave-uniform trip count (the counts are per-wave SGPR sums of ballots: every lane must take
    // part in every ballot). P correspondences per lane per trip (P loads in flight); full trips
    // run unpredicated, the ragged tail once with lane predicates.
    constexpr int TRIP = 64 * P;
    const int nFull = N / TRIP * TRIP;
    bool vt[P];
#pragma unroll
    for (int j = 0; j < P; ++j) vt[j] = true;
    for (int base = 0; base < nFull; base += TRIP) {
        float4 q[P];
#pragma unroll
        for (int j = 0; j < P; ++j) q[j] = pts[base + 64 * j + lane];
        h_sweep_trip<K, P, FUSED, false>(hm, q, vt, thr2, fast, cnt);
    }
    if (nFull < N) {
        float4 q[P];
        bool v[P];
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int p = nFull + 64 * j + lane;
            v[j] = p < N;
            q[j] = pts[v[j] ? p : 0];
        }
        h_sweep_trip<K, P, FUSED, true>(hm, q, v, thr2, fast, cnt);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (valid[k]) counts[h0 + k] = (int)cnt[k];
    }
}

// ------------------------------------------------------------------------------------------
// Packed-f32 inlier sweep (fused error). Two correspondences share a 64-bit VGPR pair per
// coordinate, so every FMA of the error runs as one v_pk_fma_f32 over both (a VOP3 v_fma_f32
// issues at the same cost as a v_pk_fma_f32 on gfx950: the packed form halves the FMA issue).
// Layout: HPair p = correspondences (2p, 2p+1) as {x, y, x', y'} pairs, 32 B; an odd N is padded
// with {0, 0, NaN, NaN}, whose error is NaN (never an inlier) and whose w is 1 (never "bad").
// Model coefficients stay in SGPRs and are broadcast to both halves with op_sel / op_sel_hi.
// Every operation rounds exactly like h_denominator_fused / rcp_newton / h_error_fused_ww.
// (f2, HPair and the packed helpers pk_fma / lo / hi: pk_pair.h, shared with ransac_a.hip.)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mcv_h_pair(const float4* __restrict__ pts, int N, HPair* __restrict__ out) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= (N + 1) / 2) return;
    const float4 a = pts[2 * p];
    const float nan = __builtin_nanf("");
    const float4 b = 2 * p + 1 < N ? pts[2 * p + 1] : make_float4(0.f, 0.f, nan, nan);
    HPair o;
    o.x = f2{a.x, b.x};
    o.y = f2{a.y, b.y};
    o.mx = f2{a.z, b.z};
    o.my = f2{a.w, b.w};
    out[p] = o;
}

// One trip: NP pairs per lane against the wave's K hypotheses.
template <int K, int NP, bool PRED>
__device__ __forceinline__ void h_pk_trip(const f2 (&hp)[K][4], const f2 (&hc)[K], const HPair (&q)[NP],
                                          const bool (&v)[NP], float thr2, f2 one, uint32_t (&cnt)[K],
                                          float (&wmin)[NP]) {
    auto vote = [&](int j, bool pred) -> uint32_t {
        if constexpr (PRED)
            return (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(v[j] && pred));
        else
            return (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(pred));
    };
#pragma unroll
    for (int k = 0; k < K; ++k) {
        // Re-define the pairs in the trip (no instruction): a broadcast is then built per use and
        // folds into op_sel / op_sel_hi, instead of being hoisted out of the loop as a splat pair
        // (which doubles the SGPRs the models take and spills them).
        f2 p0 = hp[k][0], p1 = hp[k][1], p2 = hp[k][2], p3 = hp[k][3];   // (h0,h1) .. (h6,h7)
        f2 c = hc[k];                                                       // (h2, h5)
        asm volatile("" : "+s"(p0), "+s"(p1), "+s"(p2), "+s"(p3), "+v"(c));
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            f2 W = pk_fma(lo(p3), q[j].x, pk_fma(hi(p3), q[j].y, one));
            const f2 U = pk_fma(lo(p0), q[j].x, pk_fma(hi(p0), q[j].y, lo(c)));
            const f2 V = pk_fma(hi(p1), q[j].x, pk_fma(lo(p2), q[j].y, hi(c)));
            // smallest |w| per lane and pair slot (one v_min3_f32 with |.| modifiers; an fma result
            // is canonical, so no quieting op): |w| < 2^-126 (0, denormal) is a "bad" denominator.
            // One accumulator per slot j keeps the min chains short (a single running min was
            // 4% slower than the two v_cmp_class per pair it replaces; two chains are 4% faster).
            // A NaN w (NaN point) is not tracked: the fast and the exact error are both NaN there
            // (outlier); the bounding-box precondition rules out an infinite w.
            wmin[j] = __builtin_fminf(__builtin_fminf(wmin[j], __builtin_fabsf(W.x)), __builtin_fabsf(W.y));
            f2 R = f2{__builtin_amdgcn_rcpf(W.x), __builtin_amdgcn_rcpf(W.y)};
            const f2 E = pk_fma(-W, R, one);              // fma(-w, r, 1)
            R = pk_fma(E, R, R);                          // fma(e, r, r)
            const f2 DX = pk_fma(U, R, -q[j].mx);         // fma(u, r, -x')
            const f2 DY = pk_fma(V, R, -q[j].my);         // fma(v, r, -y')
            const f2 ERR = pk_fma(DX, DX, DY * DY);       // fma(ex, ex, ey * ey)
            cnt[k] += vote(j, ERR.x <= thr2) + vote(j, ERR.y <= thr2);
        }
    }
}

// A wave whose hypotheses fail the bounding-box precondition, or which meets a "bad" denominator
// (0, denormal, inf, NaN) in any trip, marks its valid slots kStatusRedo instead of writing
// counts; mcv_h_verify<.., redo = true> then recounts exactly those slots with the scalar sweep
// (IEEE division fallback). Keeping the exact path out of this kernel keeps its registers free.
template <int K, int NP>
__global__ __launch_bounds__(256) void mcv_h_verify_pk(const HPair* __restrict__ pairs, int nPairs,
                                                       const HModelF* __restrict__ models, int* __restrict__ counts,
                                                       int hypCount, float thr2, const float* __restrict__ bbox) {
    const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * 256u + threadIdx.x) >> 6));
    const int lane = threadIdx.x & 63;
    const int h0 = wave * K;
    if (h0 >= hypCount) return;

    // Every slot below hypCount holds a model (mcv_h_generate writes the zero model, w = 1, for a
    // failed hypothesis); slots past hypCount re-read the last one. Reading the models unselected
    // keeps the (h0,h1) .. (h6,h7) SGPR pairs intact: coefficients broadcast by op_sel.
    f2 hp[K][4], hc[K];
    bool valid[K];
    const float X = bbox[0], Y = bbox[1];
    bool fast = true;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int hk = h0 + k;
        valid[k] = (hk < hypCount) && (counts[hk] >= 0);
        const f2* mp = (const f2*)&models[hk < hypCount ? hk : hypCount - 1];
#pragma unroll
        for (int j = 0; j < 4; ++j) hp[k][j] = mp[j];
        // h2, h5 are the addends of fma(h1, y, h2) / fma(h4, y, h5), beside an SGPR multiplier:
        // one VGPR pair per hypothesis (constant-bus limit), broadcast by op_sel as well.
        hc[k] = f2{hp[k][1].x, hp[k][2].y};
        asm volatile("" : "+v"(hc[k]));
        // precondition (as mcv_h_verify): max |w| over the bounding box below 2^125
        const float wmax = fabsf(hp[k][3].x) * X + fabsf(hp[k][3].y) * Y + 1.f;
        fast = fast && !(valid[k] && !(wmax < 0x1p125f));
    }
    const f2 one = f2{1.f, 1.f};

    uint32_t cnt[K];
#pragma unroll
    for (int k = 0; k < K; ++k) cnt[k] = 0;
    float wmin[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) wmin[j] = 1.0f;
    if (fast) {
        constexpr int TRIP = 64 * NP;
        const int nFull = nPairs / TRIP * TRIP;
        bool vt[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) vt[j] = true;
        for (int base = 0; base < nFull; base += TRIP) {
            HPair q[NP];
#pragma unroll
            for (int j = 0; j < NP; ++j) q[j] = pairs[base + 64 * j + lane];
            h_pk_trip<K, NP, false>(hp, hc, q, vt, thr2, one, cnt, wmin);
        }
        if (nFull < nPairs) {
            HPair q[NP];
            bool v[NP];
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const int p = nFull + 64 * j + lane;
                v[j] = p < nPairs;
                q[j] = pairs[v[j] ? p : 0];
            }
            h_pk_trip<K, NP, true>(hp, hc, q, v, thr2, one, cnt, wmin);
        }
    }
    float wm = wmin[0];
#pragma unroll
    for (int j = 1; j < NP; ++j) wm = __builtin_fminf(wm, wmin[j]);
    const bool redo = !fast || __builtin_amdgcn_ballot_w64(!(wm >= 0x1p-126f)) != 0;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (valid[k]) counts[h0 + k] = redo ? kStatusRedo : (int)cnt[k];
    }
}

// ------------------------------------------------------------------------------------------
// Certified division-free sweep of the op-by-op error (the default: OpenCV's computeError as an
// x86-64 SSE build evaluates it, h_error). Per pair of correspondences in packed f32:
//   W = fma(h6,x,fma(h7,y,1)), U = fma(h0,x,fma(h1,y,h2)), V likewise,
//   DX = fma(-x',W,U), DY = fma(-y',W,V), L = fma(DX,DX,fma(DY,DY,b_in)), W2 = W*W,
//   I = fma(W2, a_in, L), X = fma(W2, d, b_x);
//   I < 0                     -> certified inlier
//   bits(I) <= bits(X)        -> undecided (0 <= I <= X as floats); otherwise certified outlier.
// The reference error times w^2 lies within relative (t + O(u)) and absolute O(u^2 G^2 / t) of
// DX^2 + DY^2, and w^2 within the same of W2 (derivation in DESIGN.md §4); a_in, d (launch) and
// b_in, b_x (per model) put the two cuts outside those intervals, so a decided lane has the answer
// of the op-by-op fp32 error bit for bit. 13 packed ops + 4 VOPC e32 compares per pair, no
// reciprocal (the fused sweep: 12 packed + 2 v_rcp_f32 + v_min3 + 2 compares). Undecided lanes
// (where points crowd the threshold, ~1e-4 of evaluations on the cfg3 data) are recorded per trip
// and resolved after the sweep with the exact error and IEEE division.
// (The band parameter, the slopes a_in, d and the per-model offsets b_in, b_x: h_cert.h.)
// ------------------------------------------------------------------------------------------

// Unpacked model k (for the exact path): h[0..7] from the coefficient pairs.
template <int K>
__device__ __forceinline__ void h_cert_model(const f2 (&hp)[K][4], int k, float (&h)[8]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        h[2 * j] = hp[k][j].x;
        h[2 * j + 1] = hp[k][j].y;
    }
}

// The certified values of one pair of correspondences against one model: I and X (see above).
// a = {a_in, d} (shared), b = the model's {b_in, b_x}, c = {h2, h5}.
__device__ __forceinline__ void h_cert_values(f2 p0, f2 p1, f2 p2, f2 p3, f2 c, f2 a, f2 b, const HPair& q, f2 one,
                                              f2& I, f2& X) {
    const f2 W = pk_fma(lo(p3), q.x, pk_fma(hi(p3), q.y, one));      // fma(h6,x,fma(h7,y,1))
    const f2 U = pk_fma(lo(p0), q.x, pk_fma(hi(p0), q.y, lo(c)));    // fma(h0,x,fma(h1,y,h2))
    const f2 V = pk_fma(hi(p1), q.x, pk_fma(lo(p2), q.y, hi(c)));    // fma(h3,x,fma(h4,y,h5))
    const f2 DX = pk_fma(-q.mx, W, U);
    const f2 DY = pk_fma(-q.my, W, V);
    const f2 L = pk_fma(DX, DX, pk_fma(DY, DY, lo(b)));
    const f2 W2 = W * W;
    I = pk_fma(W2, lo(a), L);
    X = pk_fma(W2, hi(a), hi(b));
}

// Lane masks from the certified values: inliers and
// undecided lanes per half.
__device__ __forceinline__ void h_cert_masks(f2 I, f2 X, uint64_t& inx, uint64_t& iny, uint64_t& ux,
                                             uint64_t& uy) {
    inx = __builtin_amdgcn_ballot_w64(I.x < 0.0f);
    iny = __builtin_amdgcn_ballot_w64(I.y < 0.0f);
    ux = __builtin_amdgcn_ballot_w64(__float_as_uint(I.x) <= __float_as_uint(X.x));
    uy = __builtin_amdgcn_ballot_w64(__float_as_uint(I.y) <= __float_as_uint(X.y));
}

// h_error of both correspondences of a pair, packed, operation for operation (every product and sum
// rounded as written) with the reciprocal by rcp_exact_bounded, which equals the IEEE 1.f / w for
// every |w| < 2^126 (exhaustive GPU check, mcvTestRcpExhaustive mode 5): bit-identical to h_error in
// the certified sweep's domain (|w| <= Bw (1 + 2^-20), Bw <= 2^50).
__device__ __forceinline__ f2 h_error_pk(f2 p0, f2 p1, f2 p2, f2 p3, const HPair& q) {
    const f2 w = (lo(p3) * q.x + hi(p3) * q.y) + f2{1.f, 1.f};
    const f2 ww = f2{rcp_exact_bounded(w.x), rcp_exact_bounded(w.y)};   // |w| <= 2^51 in the certified domain
    const f2 ex = ((lo(p0) * q.x + hi(p0) * q.y) + lo(p1)) * ww - q.mx;
    const f2 ey = ((hi(p1) * q.x + lo(p2) * q.y) + hi(p2)) * ww - q.my;
    return ex * ex + ey * ey;
}

// One trip: NP pairs per lane against the wave's K models. vx / vy: lanes whose first / second
// correspondence of pair slot j exists (tail trip only). Returns the mask of models with an
// undecided lane in this trip (bit k); their certified counts are already in cnt.
template <int K, int NP, bool PRED>
__device__ __forceinline__ uint32_t h_cert_trip(f2 (&hp)[K][4], const f2 (&hc)[K], f2 a, const f2 (&cb)[K],
                                                const HPair (&q)[NP], const uint64_t (&vx)[NP],
                                                const uint64_t (&vy)[NP], f2 one, uint32_t (&cnt)[K]) {
    uint32_t undecided = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        // re-defined in place every trip (no copy): the loop cannot hoist the broadcasts, so each use
        // reads the SGPR pair through op_sel
        asm volatile("" : "+s"(hp[k][0]), "+s"(hp[k][1]), "+s"(hp[k][2]), "+s"(hp[k][3]));
        uint64_t und = 0;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            f2 I, X;
            h_cert_values(hp[k][0], hp[k][1], hp[k][2], hp[k][3], hc[k], a, cb[k], q[j], one, I, X);
            uint64_t inx, iny, ux, uy;
            if constexpr (PRED) {
                h_cert_masks(I, X, inx, iny, ux, uy);
                inx &= vx[j];
                iny &= vy[j];
                und |= (ux & vx[j]) | (uy & vy[j]);
            } else {
                h_cert_masks(I, X, inx, iny, ux, uy);
                und |= ux | uy;
            }
            cnt[k] += (uint32_t)__popcll(inx) + (uint32_t)__popcll(iny);
        }
        undecided |= (und != 0) ? (1u << k) : 0u;
    }
    return undecided;
}

// The exact op-by-op error for the undecided lanes of the models in `und`, with the models still in
// registers (compile-time model index; the branch per model is
// wave-uniform and rarely taken).
template <int K, int NP, bool PRED>
__device__ __forceinline__ void h_cert_fix_regs(uint32_t und, const f2 (&hp)[K][4], const f2 (&hc)[K], f2 a,
                                                const f2 (&cb)[K], const HPair (&q)[NP], const uint64_t (&vx)[NP],
                                                const uint64_t (&vy)[NP], float thr2, f2 one, uint32_t (&cnt)[K]) {
    const uint64_t me = 1ull << (__lane_id() & 63);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (!(und & (1u << k))) continue;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            f2 I, X;
            h_cert_values(hp[k][0], hp[k][1], hp[k][2], hp[k][3], hc[k], a, cb[k], q[j], one, I, X);
            uint64_t inx, iny, ux, uy;
            h_cert_masks(I, X, inx, iny, ux, uy);
            if constexpr (PRED) {
                ux &= vx[j];
                uy &= vy[j];
            }
            if ((ux | uy) == 0) continue;
            const f2 e = h_error_pk(hp[k][0], hp[k][1], hp[k][2], hp[k][3], q[j]);
            cnt[k] += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64((ux & me) != 0 && e.x <= thr2)) +
                      (uint32_t)__popcll(__builtin_amdgcn_ballot_w64((uy & me) != 0 && e.y <= thr2));
        }
    }
}

// The exact op-by-op error (IEEE division) for the undecided lanes of model hk at the trip starting
// at pair `base` (re-read from memory; validity from the pair counts). Returns their inlier count.
template <int NP>
__device__ __noinline__ uint32_t h_cert_resolve(const HPair* __restrict__ pairs, int nPairs, int nComplete, int base,
                                                const HModelF* __restrict__ models, int hk, f2 a, f2 b, float thr2) {
    const int lane = threadIdx.x & 63;
    const uint64_t me = 1ull << lane;
    const f2* mp = (const f2*)&models[hk];
    const f2 m0 = mp[0], m1 = mp[1], m2 = mp[2], m3 = mp[3];
    const float h[8] = {m0.x, m0.y, m1.x, m1.y, m2.x, m2.y, m3.x, m3.y};
    const f2 one = f2{1.f, 1.f};
    uint32_t add = 0;
    for (int j = 0; j < NP; ++j) {
        const int p = base + 64 * j + lane;
        const uint64_t vx = __builtin_amdgcn_ballot_w64(p < nPairs), vy = __builtin_amdgcn_ballot_w64(p < nComplete);
        const HPair q = pairs[p < nPairs ? p : 0];
        f2 I, X;
        h_cert_values(m0, m1, m2, m3, f2{m1.x, m2.y}, a, b, q, one, I, X);
        uint64_t inx, iny, ux, uy;
        h_cert_masks(I, X, inx, iny, ux, uy);
        ux &= vx;
        uy &= vy;
        bool ex = false, ey = false;
        if (ux & me) ex = h_error(h, q.x.x, q.y.x, q.mx.x, q.my.x) <= thr2;
        if (uy & me) ey = h_error(h, q.x.y, q.y.y, q.mx.y, q.my.y) <= thr2;
        add += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(ex)) + (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(ey));
    }
    return add;
}

// A wave whose models or point set leave the bound's domain marks its valid slots kStatusRedo
// (recounted by the exact scalar sweep mcv_h_verify<.., false> with redo = 1), as does a wave
// whose undecided trips overflow its event list. Trips with undecided lanes are only recorded in
// the sweep (LDS event list: trip base << 8 | model mask) and resolved after it, so the exact
// division stays out of the sweep's registers.
// nComplete = N / 2 pairs hold two correspondences; pair nComplete (odd N) holds one.
static constexpr int kCertEvents = 256;   // per wave

// STAGED: the wave sweeps only the pair range of its stage (read from the control block), takes its
// models through the survivor list and adds to the slots' counts; everything else (the certified
// arithmetic, the per-model offsets, the LDS offsets and events, the overflow fallback) is the one
// body. Stage ranges start trip-aligned, so only the stage that ends at nPairs meets the tail trip.
template <int K, int NP, bool STAGED>
__global__ __launch_bounds__(256) void mcv_h_verify_cert(const HPair* __restrict__ pairs, int nPairs, int nComplete,
                                                         const HModelF* __restrict__ models, int* __restrict__ counts,
                                                         int hypCount, float thr2, HCertSlopes slopes,
                                                         const double* __restrict__ bb, HStageArgs sa) {
    static_assert(K <= 8, "model mask in 8 bits");
    __shared__ uint32_t events[4][kCertEvents];
    __shared__ f2 offsets[4][K];
    const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * 256u + threadIdx.x) >> 6));
    const int wib = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int h0 = wave * K;
    int pBeg = 0, pEnd = nPairs;
    if constexpr (STAGED) {
        pBeg = sa.ctl[kCtlBound + sa.stage];
        pEnd = sa.ctl[kCtlBound + sa.stage + 1];
        if (pBeg >= pEnd) return;
        if (sa.list) hypCount = sa.ctl[kCtlAlive + sa.stage];
    }
    if (h0 >= hypCount) return;

    f2 hp[K][4], hc[K], cb[K];
    bool valid[K];
    int slot[STAGED ? K : 1];   // STAGED: the slots of the wave's entries (wave-uniform, kept for the write-back)
    auto slot_of = [&](int k) -> int {
        if constexpr (STAGED) return slot[k];
        else return h0 + k < hypCount ? h0 + k : hypCount - 1;
    };
    bool fast = true;
    double b4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) b4[j] = bb[j];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int hk = h0 + k;
        if constexpr (STAGED) {
            const int e = hk < hypCount ? hk : hypCount - 1;
            slot[k] = sa.list ? sa.list[e] : e;
        }
        valid[k] = (hk < hypCount) && (counts[STAGED ? slot_of(k) : hk] >= 0);
        const f2* mp = (const f2*)&models[slot_of(k)];
#pragma unroll
        for (int j = 0; j < 4; ++j) hp[k][j] = mp[j];
        hc[k] = f2{hp[k][1].x, hp[k][2].y};
        float h[8];
        h_cert_model<K>(hp, k, h);
        const bool ok = h_cert_offsets(h, b4, thr2, slopes.t, cb[k]);
        fast = fast && (ok || !valid[k]);
        if (lane == 0) offsets[wib][k] = cb[k];
        __builtin_amdgcn_wave_barrier();
        // VGPR-resident: hc and cb meet an SGPR coefficient or another model operand in the same
        // packed op (constant-bus limit)
        asm volatile("" : "+v"(hc[k]), "+v"(cb[k]));
    }
    const f2 one = f2{1.f, 1.f};
    uint32_t cnt[K];
#pragma unroll
    for (int k = 0; k < K; ++k) cnt[k] = 0;
    int nev = 0;
    // an event records the trip index (base / TRIP: < 2^24 for any N < 2^31, pairs = N / 2) and the
    // undecided-model mask in its low 8 bits
    constexpr int TRIP = 64 * NP;
    if (fast) {
        const int nFull = nComplete / TRIP * TRIP;
        const int fullEnd = STAGED ? (pEnd < nFull ? pEnd : nFull) : nFull;
        uint64_t all[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) all[j] = ~0ull;
        for (int base = pBeg; base < fullEnd; base += TRIP) {
            HPair q[NP];
#pragma unroll
            for (int j = 0; j < NP; ++j) q[j] = pairs[base + 64 * j + lane];
            const uint32_t und = h_cert_trip<K, NP, false>(hp, hc, slopes.a, cb, q, all, all, one, cnt);
            if (__builtin_expect(und != 0, 0))
                h_cert_fix_regs<K, NP, false>(und, hp, hc, slopes.a, cb, q, all, all, thr2, one, cnt);
        }
        // the tail: pairs [nFull, nPairs), part of the stage that ends at nPairs (pBeg <= nFull there)
        for (int base = STAGED ? (pBeg > nFull ? pBeg : nFull) : nFull; base < pEnd; base += TRIP) {
            HPair q[NP];
            uint64_t vx[NP], vy[NP];
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const int p = base + 64 * j + lane;
                vx[j] = __builtin_amdgcn_ballot_w64(p < nPairs);
                vy[j] = __builtin_amdgcn_ballot_w64(p < nComplete);
                q[j] = pairs[p < nPairs ? p : 0];
            }
            const uint32_t und = h_cert_trip<K, NP, true>(hp, hc, slopes.a, cb, q, vx, vy, one, cnt);
            if (und != 0) {
                if (nev < kCertEvents && lane == 0) events[wib][nev] = ((uint32_t)(base / TRIP) << 8) | und;
                ++nev;
            }
        }
        if (nev > kCertEvents) fast = false;   // too many to resolve here: exact recount of the wave
        else if (nev > 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int e = 0; e < nev; ++e) {
                const uint32_t ev = __builtin_amdgcn_readfirstlane(events[wib][e]);
                const int base = (int)(ev >> 8) * TRIP;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    if (!(ev & (1u << k))) continue;
                    cnt[k] += h_cert_resolve<NP>(pairs, nPairs, nComplete, base, models, slot_of(k), slopes.a,
                                                 offsets[wib][k], thr2);
                }
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (!valid[k]) continue;
            if constexpr (STAGED)
                counts[slot[k]] = fast ? counts[slot[k]] + (int)cnt[k] : kStatusRedo;
            else
                counts[h0 + k] = fast ? (int)cnt[k] : kStatusRedo;
        }
    }
}

// Bounding box of the source points: bbox[0] = max |x|, bbox[1] = max |y| (one block; the
// ordering of float maxima is exact, so the result does not depend on the reduction order).
__global__ __launch_bounds__(1024) void mcv_bbox(const float4* __restrict__ pts, int N, float* __restrict__ bbox) {
    __shared__ float sx[16], sy[16];
    float mx = 0, my = 0;
    for (int i = threadIdx.x; i < N; i += 1024) {
        const float4 q = pts[i];
        mx = fmaxf(mx, fabsf(q.x));
        my = fmaxf(my, fabsf(q.y));
        if (q.x != q.x || q.y != q.y) mx = __builtin_inff();   // NaN coordinate: force exact path
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        my = fmaxf(my, __shfl_xor(my, off, 64));
    }
    if ((threadIdx.x & 63) == 0) { sx[threadIdx.x >> 6] = mx; sy[threadIdx.x >> 6] = my; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) { mx = fmaxf(mx, sx[w]); my = fmaxf(my, sy[w]); }
        bbox[0] = mx;
        bbox[1] = my;
    }
}

void launch_bbox(const float* d_pts4, int N, float* d_bbox, hipStream_t s) {
    hipLaunchKernelGGL(mcv_bbox, dim3(1), dim3(1024), 0, s, (const float4*)d_pts4, N, d_bbox);
}

static void launch_h_scalar(const float* d_pts4, int N, const void* d_models, int* d_counts, int hypCount, float thr2,
                            bool fused, const float* d_bbox, int redo, hipStream_t s) {
    constexpr int K = kVerifyHypPerWave, P = kVerifyPtsPerLane;
    const int waves = (hypCount + K - 1) / K;
    const int blocks = (waves + 3) / 4;
    auto* kernel = fused ? mcv_h_verify<K, P, true> : mcv_h_verify<K, P, false>;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, s, (const float4*)d_pts4, N, (const HModelF*)d_models,
                       d_counts, hypCount, thr2, d_bbox, redo);
}

void launch_h_verify(const float* d_pts4, int N, const void* d_models, int* d_counts, int hypCount, float thr2,
                     bool fused, const float* d_bbox, hipStream_t s) {
    launch_h_scalar(d_pts4, N, d_models, d_counts, hypCount, thr2, fused, d_bbox, 0, s);
}

void launch_h_recount(const float* d_pts4, int N, const void* d_models, int* d_counts, int hypCount, float thr2,
                      bool fused, const float* d_bbox, hipStream_t s) {
    launch_h_scalar(d_pts4, N, d_models, d_counts, hypCount, thr2, fused, d_bbox, 1, s);
}

void launch_h_pair(const float* d_pts4, int N, void* d_pairs, hipStream_t s) {
    const int np = (N + 1) / 2;
    hipLaunchKernelGGL(mcv_h_pair, dim3((np + 255) / 256), dim3(256), 0, s, (const float4*)d_pts4, N,
                       (HPair*)d_pairs);
}

// Packed sweep (fused error, <8, 2>: DESIGN.md §7's screen) + the exact recount of the slots it
// marked kStatusRedo.
void launch_h_verify_packed(const float* d_pts4, const void* d_pairs, int N, const void* d_models, int* d_counts,
                            int hypCount, float thr2, const float* d_bbox, hipStream_t s) {
    constexpr int K = 8, NP = 2;
    const int waves = (hypCount + K - 1) / K;
    const int blocks = (waves + 3) / 4;
    hipLaunchKernelGGL((mcv_h_verify_pk<K, NP>), dim3(blocks), dim3(256), 0, s, (const HPair*)d_pairs, (N + 1) / 2,
                       (const HModelF*)d_models, d_counts, hypCount, thr2, d_bbox);
    launch_h_recount(d_pts4, N, d_models, d_counts, hypCount, thr2, true, d_bbox, s);
}

void launch_h_cert_sweep(const void* d_pairs, int N, const void* d_models, int* d_counts, int hypCount, float thr2,
                         const HCertSlopes& slopes, const double* d_bb, HStageArgs sa, hipStream_t s) {
    const int waves = (hypCount + kCertK - 1) / kCertK;
    const int blocks = (waves + 3) / 4;
    auto* kernel = sa.ctl ? mcv_h_verify_cert<kCertK, kCertNP, true> : mcv_h_verify_cert<kCertK, kCertNP, false>;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, s, (const HPair*)d_pairs, (N + 1) / 2, N / 2,
                       (const HModelF*)d_models, d_counts, hypCount, thr2, slopes, d_bb, sa);
}

// Certified sweep of the op-by-op error + the exact recount of the slots it marks kStatusRedo.
void launch_h_verify_certified(const float* d_pts4, const void* d_pairs, int N, const void* d_models, int* d_counts,
                               int hypCount, float thr2, const double* d_bb, hipStream_t s, const void* d_rec,
                               unsigned long long* d_stats, int form) {
    const HStageArgs whole{nullptr, nullptr, 0};
    if (d_stats) (void)hipMemsetAsync(d_stats, 0, kHMfmaStats * sizeof(unsigned long long), s);
    if (d_rec && d_stats && h_mfma_engages(N, hypCount, form, false))
        launch_h_mfma_sweep(d_pts4, d_rec, N, d_models, d_counts, hypCount, thr2, h_cert_slopes_host(thr2), d_bb, whole,
                            d_stats, s);
    else
        launch_h_cert_sweep(d_pairs, N, d_models, d_counts, hypCount, thr2, h_cert_slopes_host(thr2), d_bb, whole, s);
    launch_h_recount(d_pts4, N, d_models, d_counts, hypCount, thr2, false, nullptr, s);
}

}  // namespace mcv
