// h_cert.h — the certificate of the division-free homography sweep, shared by its VALU form
// (ransac_h_sweep.hip), its matrix-core form (ransac_h_mfma.hip) and the per-cell bound
// (ransac_h_stage.hip): the band constants, the launch slopes, the per-model offsets, and the stage
// arguments both sweep kernels take. The certificate is described at mcv_h_verify_cert. Device code only.
#pragma once

#include <cmath>
#include "pk_pair.h"
#include "kernels.h"

namespace mcv {

// Band parameter: relative half-width ~ t + O(u) around thr2 w^2, absolute part ~ (7.5 u G)^2 / t.
// One t for every model keeps the slopes launch constants.
static constexpr double kCertT = 0x1p-11;   // band parameter (screened 2^-12 / 2^-11 / 2^-10: DESIGN.md §7)
static constexpr double kCertSlop = 0x1p-18;   // covers the O(u) factors (< 16 u = 2^-20 in total)

struct HCertSlopes {
    f2 a;       // {a_in (<= 0), d (>= 0)}
    double t;   // band parameter the per-model offsets use
};

inline HCertSlopes h_cert_slopes_host(float thr2) {
    const double T = (double)thr2, t = kCertT, u = 0x1p-24;
    // inlier cut: |a_in| <= T (1-t)/(1+t) (1 - slop), rounded towards zero
    const double ain = -T * (1.0 - t) / (1.0 + t) * (1.0 - kCertSlop);
    float fi = (float)ain;
    if ((double)fi < ain) fi = std::nextafter(fi, 0.0f);
    // outlier cut: |a_in| + d (1 - 2u) >= T (1+t)/(1-t) (1 + slop), d rounded up
    const double need = T * (1.0 + t) / (1.0 - t) * (1.0 + kCertSlop);
    const double d = (need + (double)fi) / (1.0 - 2 * u);
    float fd = (float)d;
    if ((double)fd < d) fd = std::nextafter(fd, __builtin_inff());
    HCertSlopes c;
    c.a = f2{fi, fd};
    c.t = t;
    return c;
}

// Per-model offsets b = {b_in, b_x} (both > 0); false when the model or the point set leaves the
// domain of the error bound (the wave then hands its slots to the exact scalar sweep).
// bb = {max|x|, max|y|, max|x'|, max|y'|} of the correspondences (inf when any is NaN / inf).
// MFMA = true: W, U, V come from the bf16 matrix-core dot (mcv_h_verify_mfma) instead of the fma chains.
// The chains' 2 u B of each form (two roundings) is replaced by the dot's kMfmaDotC u B (the split's
// dropped products + the accumulation: DESIGN.md §4) and by an absolute term for bf16 pieces and sums
// below 2^-126, which the matrix core may flush; coefficients above 2^100 leave the domain (a bf16
// piece must not round to infinity).
static constexpr double kMfmaDotC = 8.5;
template <bool MFMA = false>
__device__ __forceinline__ bool h_cert_offsets(const float* h, const double* bb, float thr2, double t, f2& b) {
    const double X = bb[0], Y = bb[1], MX = bb[2], MY = bb[3];
    const double u = 0x1p-24;
    const double Bu = fabs((double)h[0]) * X + fabs((double)h[1]) * Y + fabs((double)h[2]);
    const double Bv = fabs((double)h[3]) * X + fabs((double)h[4]) * Y + fabs((double)h[5]);
    const double Bw = fabs((double)h[6]) * X + fabs((double)h[7]) * Y + 1.0;
    const double Gx = Bu + MX * Bw + 0x1p-40, Gy = Bv + MY * Bw + 0x1p-40;
    const double T = (double)thr2;
    bool ok = X <= 0x1p40 && Y <= 0x1p40 && MX <= 0x1p40 && MY <= 0x1p40 && Bw <= 0x1p50 &&
              Gx <= 0x1p50 && Gy <= 0x1p50 && T >= 0x1p-100 && T <= 0x1p20;   // false for NaN
    double cx = 7.5 * u * Gx, cy = 7.5 * u * Gy, cw = 5.1 * u * Bw;
    if constexpr (MFMA) {
        double hmax = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) hmax = fmax(hmax, fabs((double)h[j]));
        ok = ok && hmax <= 0x1p100;
        const double fl = 0x1p-122 * (X + Y + 1.0);
        const double eu = 0x1p-122 * (fabs((double)h[0]) + fabs((double)h[1])) + fl;
        const double ev = 0x1p-122 * (fabs((double)h[3]) + fabs((double)h[4])) + fl;
        const double ew = 0x1p-122 * (fabs((double)h[6]) + fabs((double)h[7])) + fl;
        cx = (5.5 + kMfmaDotC) * u * Gx + eu + MX * ew;
        cy = (5.5 + kMfmaDotC) * u * Gy + ev + MY * ew;
        cw = (3.1 + kMfmaDotC) * u * Bw + ew;
    }
    const double C = cx * cx + cy * cy, Cw = cw * cw;
    const double tiny = 0x1p-120 + 0x1p-140 * Bw * Bw;
    const double K1 = (1.0 + 2 * kCertSlop) * ((1.0 + 1.0 / t) * C + T * Cw / t) + tiny;
    const double K2 = (1.0 + 2 * kCertSlop) / (1.0 - t) * (C / t + T * (1.0 + 1.0 / t) * Cw) + tiny;
    const float bin = __double2float_ru(K1);
    const double bx = (K2 + (double)bin) * (1.0 + kCertSlop);
    b = f2{bin, __double2float_ru(bx)};
    return ok;
}

// Control block of the staged sweep (ints; device memory, kHStageCtlInts of them). Stage s sweeps the
// pairs [bound[s], bound[s + 1]): stage 0 is the prefix that finds the candidate, stage 1 runs every
// slot up to the first boundary, stages 2.. run the survivor lists.
// Indices: kCtl* in kernels.h.

struct HStageArgs {
    const int* ctl;    // control block
    const int* list;   // survivor slots of this stage (nullptr: every slot, in order)
    int stage;
};

// mcv_h_verify_cert's hypotheses per wave and pairs per lane per trip.
// <6, 1>: screened against <4, 2>, <4, 1>, <5, 1>, <3, 2>, <8, 2> and t = 2^-12 / 2^-11 / 2^-10
// (28.8 ms vs 29.6-33 ms at cfg3; scripts/gpu_r02_cert.sh); re-screened in round 5 (same box: 29.9-30.0 ms
// against 30.7-30.9 / 30.4-30.5 / 31.0-31.1 ms for <4, 1> / <5, 1> / <4, 2>; scripts/gpu_r05_am.sh).
static constexpr int kCertK = 6, kCertNP = 1;

// One launch of a certified sweep kernel, VALU (ransac_h_sweep.hip) or matrix-core form (ransac_h_mfma.hip):
// a stage of the staged sweep (sa.ctl given) or, with HStageArgs{nullptr, nullptr, 0}, the whole range.
void launch_h_cert_sweep(const void* d_pairs, int N, const void* d_models, int* d_counts, int hypCount, float thr2,
                         const HCertSlopes& slopes, const double* d_bb, HStageArgs sa, hipStream_t s);
void launch_h_mfma_sweep(const float* d_pts4, const void* d_rec, int N, const void* d_models, int* d_counts,
                         int hypCount, float thr2, const HCertSlopes& slopes, const double* d_bb, HStageArgs sa,
                         unsigned long long* d_stats, hipStream_t s);
// The exact recount, over all N, of the slots a sweep marked kStatusRedo (the scalar sweep mcv_h_verify).
void launch_h_recount(const float* d_pts4, int N, const void* d_models, int* d_counts, int hypCount, float thr2,
                      bool fused, const float* d_bbox, hipStream_t s);

}  // namespace mcv
