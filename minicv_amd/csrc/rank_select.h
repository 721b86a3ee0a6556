// rank_select.h — the order key and the radix-select steps of the LMedS rank kernel (lmeds.hip),
// shared by the kernel and its host twin (mcvHostErrorRank): both run the same three passes
// (11 + 11 + 10 bits of the key, most significant first) over a 2048-bin histogram.
//
// Order: fp32 bit patterns read as unsigned, which for the non-negative errors of h_error /
// f_error is OpenCV's nth_element over the reinterpreted ints; every NaN is one class that sorts
// after +inf (key 0xFFFFFFFF).
#pragma once

#include "mcv_common.h"
#include <string.h>

namespace mcv {

static const int kRankBins = 2048;
static const int kRankPasses = 3;
static const uint32_t kRankKeyNaN = 0xFFFFFFFFu;

MCV_HD uint32_t rank_key(float e) {
    if (e != e) return kRankKeyNaN;
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(e);
#else
    uint32_t u;
    memcpy(&u, &e, sizeof(u));
    return u;
#endif
}

// The value a key stands for (the NaN class -> a quiet NaN).
MCV_HD float rank_value(uint32_t key) {
    const uint32_t u = key == kRankKeyNaN ? 0x7FC00000u : key;
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f;
    memcpy(&f, &u, sizeof(f));
    return f;
#endif
}

// Pass p looks at bits [shift, shift + width) of the keys whose higher bits equal the prefix found so far.
MCV_HD int rank_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }
MCV_HD int rank_width(int pass) { return pass == 2 ? 10 : 11; }
MCV_HD uint32_t rank_digit(uint32_t key, int pass) { return (key >> rank_shift(pass)) & ((1u << rank_width(pass)) - 1u); }
// prefix = the key's bits above this pass's digit, already shifted down (pass 0: none).
MCV_HD bool rank_in_prefix(uint32_t key, uint32_t prefix, int pass) {
    return pass == 0 || (key >> (rank_shift(pass) + rank_width(pass))) == prefix;
}

// Walk bins [begin, end): the bin holding the element of rank `rank` among them; `rank` becomes the
// rank inside that bin. With fewer than rank + 1 elements: the last bin (callers keep rank < count).
MCV_HD int rank_pick(const uint32_t* hist, int begin, int end, uint32_t& rank) {
    for (int b = begin; b < end; ++b) {
        const uint32_t c = hist[b];
        if (rank < c) return b;
        rank -= c;
    }
    return end - 1;
}

// Host twin of one slot's selection: err(i) = the fp32 error of correspondence i.
template <class Err>
inline uint32_t rank_select_host(const Err& err, int N, uint32_t rank) {
    uint32_t hist[kRankBins];
    uint32_t prefix = 0;
    for (int pass = 0; pass < kRankPasses; ++pass) {
        for (int b = 0; b < kRankBins; ++b) hist[b] = 0;
        for (int i = 0; i < N; ++i) {
            const uint32_t key = rank_key(err(i));
            if (rank_in_prefix(key, prefix, pass)) ++hist[rank_digit(key, pass)];
        }
        const int d = rank_pick(hist, 0, 1 << rank_width(pass), rank);
        prefix = (prefix << rank_width(pass)) | (uint32_t)d;
    }
    return prefix;
}

}  // namespace mcv
