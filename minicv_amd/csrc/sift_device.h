// sift_device.h — the loops of the SIFT kernels, one copy for the single call's
// kernels (sift.hip) and the batch's (sift_batch.hip). A kernel of either file finds its image, octave
// and tile, then calls the body here with plain pointers and sizes, so a sample is computed by the same
// instructions in the same order whichever call it belongs to. Device code only.
#pragma once

#include "kernels.h"
#include "sift_math.h"

namespace mcv {

typedef unsigned long long sift_u64;

// one pixel (row R, column C) of the doubled grey image; the caller has checked R < 2 h
__device__ __forceinline__ void sift_dev_grey_double(const uint8_t* __restrict__ img, int w, int h, int ch,
                                                     float* __restrict__ up, int C, int R) {
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

// One row segment of kSiftRowTile outputs per block (row r < h, first column x0 < w), the segment and
// its halo in LDS (tile: kSiftRowTile + 2 R floats). Has a barrier: the whole block calls it.
__device__ __forceinline__ void sift_dev_blur_rows(const float* __restrict__ in, float* __restrict__ out, int w,
                                                   const float* __restrict__ taps, int R, int r, int x0,
                                                   float* tile) {
    const float* row = in + (size_t)r * (size_t)w;
    for (int k = threadIdx.x; k < kSiftRowTile + 2 * R; k += kSiftRowTile) tile[k] = row[sift_reflect(x0 + k - R, w)];
    __syncthreads();
    const int c = x0 + threadIdx.x;
    if (c >= w) return;
    float acc = 0.0f;
    for (int t = 0; t <= 2 * R; ++t) acc = acc + taps[t] * tile[threadIdx.x + t];
    out[(size_t)r * (size_t)w + c] = acc;
}

// A tile of kSiftColTileW columns x kSiftColTileH rows per block of 256 (tile column bx, tile row by,
// both inside the image), with a halo of R rows above and below (tile: (kSiftColTileH + 2 R) x
// kSiftColTileW floats). Has a barrier: the whole block calls it.
__device__ __forceinline__ void sift_dev_blur_cols(const float* __restrict__ in, float* __restrict__ out, int w, int h,
                                                   const float* __restrict__ taps, int R, int bx, int by,
                                                   float* tile) {
    const int cx = threadIdx.x & (kSiftColTileW - 1), ty = threadIdx.x / kSiftColTileW;
    const int c = bx * kSiftColTileW + cx, y0 = by * kSiftColTileH;
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

// DoG and the 26-neighbour test of one octave for the pixel (r, c) of every lane: a lane walks its
// pixel's 3 x 3 patch up the Gaussian stack, keeps three DoG patches in registers, and tests the middle
// one. emit(is, layer) is called by the whole wave for every layer 1 .. nl (it ballots).
template <class Emit>
__device__ __forceinline__ void sift_dev_extrema(const float* __restrict__ g, int w, int h, int nl, float thr, int r,
                                                 int c, Emit emit) {
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
        emit(is, L - 1);
    }
}

// Appends the record of every lane with `is` to cand, wave by wave: one add to *ctr per wave (and one
// to *ctr2 when it is given), the lanes' places by their rank in the ballot. Places >= cap are counted,
// not written. Called by the whole wave.
__device__ __forceinline__ void sift_dev_append(bool is, int4 rec, int4* __restrict__ cand, unsigned cap,
                                                unsigned* __restrict__ ctr, unsigned* __restrict__ ctr2) {
    const int lane = threadIdx.x & 63;
    const sift_u64 m = __ballot(is);
    if (!m) return;
    const int leader = __ffsll((long long)m) - 1;
    unsigned base = 0;
    if (lane == leader) {
        base = atomicAdd(ctr, (unsigned)__popcll(m));
        if (ctr2) atomicAdd(ctr2, (unsigned)__popcll(m));
    }
    base = __shfl(base, leader);
    if (is) {
        const unsigned at = base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        if (at < cap) cand[at] = rec;
    }
}

// The orientation histogram of one refined candidate per wave (g: its octave's first image, w x h),
// as 64-bit integer LDS atomics (the sum does not depend on the order); lane 0 smooths it and finds the
// peaks. Returns their number on lane 0 of a valid wave, 0 elsewhere. hist: the wave's kSiftOriBins
// words. Has barriers: the whole block calls it.
__device__ __forceinline__ int sift_dev_orient(const float* __restrict__ g, int w, int h, const SiftKp& kp, bool valid,
                                               sift_u64* hist, int* bins, float* angles) {
    const int lane = threadIdx.x & 63;
    if (lane < kSiftOriBins) hist[lane] = 0;
    __syncthreads();
    if (valid) {
        const float* img = g + (size_t)kp.layer * (size_t)w * (size_t)h;
        const int rad = sift_ori_radius(kp.scl), side = 2 * rad + 1, n = side * side;
        const float es = sift_ori_escale(kp.scl);
        for (int s = lane; s < n; s += 64) {
            int bin;
            long long q;
            if (sift_ori_sample(img, w, h, kp.r, kp.c, s / side - rad, s % side - rad, es, bin, q))
                atomicAdd(&hist[bin], (sift_u64)q);
        }
    }
    __syncthreads();
    return valid && lane == 0 ? sift_ori_peaks((const long long*)hist, bins, angles) : 0;
}

// The np records of one candidate (q: its start, kp: its refined position) at recs[at ..), with their
// keys; `image` goes into the record's pad and above the key's 45 bits (0 for the single call).
__device__ __forceinline__ void sift_dev_orient_records(const SiftKp& kp, int4 q, int np, const int* bins,
                                                        const float* angles, size_t at0, int image,
                                                        SiftRec* __restrict__ recs, sift_u64* __restrict__ keys,
                                                        sift_u64* __restrict__ starts, sift_u64* __restrict__ rkeys) {
    const float sc = (float)(1 << kp.o) * 0.5f;
    const sift_u64 hi = (sift_u64)image << kSiftKeyBits;
    for (int k = 0; k < np; ++k) {
        const size_t at = at0 + (size_t)k;
        recs[at] = SiftRec{((float)kp.c + kp.xc) * sc, ((float)kp.r + kp.xr) * sc, kp.size, angles[k],
                           kp.response, kp.octave, kp.o, kp.layer, kp.r, kp.c, kp.scl, image};
        keys[at] = hi | sift_key(kp.o, kp.layer, kp.r, kp.c, bins[k]);
        starts[at] = sift_key(q.x, q.y, q.z, q.w, bins[k]);
        rkeys[at] = (sift_u64)(0xffffffffu - __float_as_uint(kp.response));
    }
}

// One wave per output keypoint i (q, in the octave whose first image is g, w x h): the 4 x 4 x 8
// histogram as 64-bit integer LDS atomics, lane 0 normalises, the wave writes the row and the
// KeyPoint2d. sum, fo: the wave's kSiftDescLen words each. Has barriers: the whole block calls it.
__device__ __forceinline__ void sift_dev_describe(const float* __restrict__ g, int w, int h, const SiftRec& q,
                                                  bool valid, size_t i, int descType,
                                                  SiftKeyPointOut* __restrict__ kpOut, uint8_t* __restrict__ descU8,
                                                  float* __restrict__ descF32, sift_u64* sum, float* fo) {
    const int lane = threadIdx.x & 63;
    for (int k = lane; k < kSiftDescLen; k += 64) sum[k] = 0;
    __syncthreads();
    if (valid) {
        const float* img = g + (size_t)q.layer * (size_t)w * (size_t)h;
        const SiftDescFrame F = sift_desc_frame(q.angle, q.scl, w, h);
        const int side = 2 * F.radius + 1;
        const long long ns = (long long)side * side;
        for (long long s = lane; s < ns; s += 64)
            sift_desc_sample(img, w, h, q.r, q.c, (int)(s / side) - F.radius, (int)(s % side) - F.radius, F,
                             [sum](int k, long long v) { atomicAdd(&sum[k], (sift_u64)v); });
    }
    __syncthreads();
    if (valid && lane == 0) sift_desc_finish((const long long*)sum, fo);
    __syncthreads();
    if (!valid) return;
    for (int k = lane; k < kSiftDescLen; k += 64) {
        if (descType == 0)
            descU8[i * kSiftDescLen + k] = sift_desc_byte(fo[k]);
        else
            descF32[i * kSiftDescLen + k] = fo[k];
    }
    if (lane == 0) kpOut[i] = SiftKeyPointOut{q.x, q.y, q.size, q.angle, q.response, q.octave, -1};
}

// the order stage's place of a record among those of its bucket [lo, hi) in (key, start) order; E != 0
// for the later copies of an exact duplicate
__device__ __forceinline__ unsigned sift_dev_rank(const sift_u64* __restrict__ keys,
                                                  const sift_u64* __restrict__ starts, const int* __restrict__ perm,
                                                  unsigned lo, unsigned hi, sift_u64 ki, sift_u64 si, unsigned& E) {
    unsigned L = 0;
    E = 0;
    for (unsigned m = lo; m < hi; ++m) {
        const int j = perm[m];
        const sift_u64 kj = keys[j];
        L += kj < ki ? 1u : 0u;
        E += (kj == ki && starts[j] < si) ? 1u : 0u;
    }
    return lo + L + E;   // < hi: the other records of the bucket are hi - lo - 1
}

}  // namespace mcv
