// pk_pair.h — the paired point layout and the packed-f32 helpers shared by the packed inlier sweeps
// (ransac_h_sweep.hip: mcv_h_verify_pk, mcv_h_verify_cert; ransac_h_mfma.hip; ransac_a.hip: mcv_a_verify_pk). Device code only.
#pragma once

#include <hip/hip_runtime.h>

namespace mcv {

typedef float f2 __attribute__((ext_vector_type(2)));

// HPair p = correspondences (2p, 2p+1) as {x, y, x', y'} pairs, 32 B (written by mcv_h_pair; an odd N is
// padded with {0, 0, NaN, NaN}, whose error is NaN: never an inlier).
struct HPair {
    f2 x, y, mx, my;
};

// Packed FMA through the compiler (llvm.fma.v2f32 -> v_pk_fma_f32): it folds a splat of an SGPR
// coefficient into op_sel / op_sel_hi and inserts the wait states between dependent packed ops
// (hand-written asm would not get them: the hazard recognizer does not see into inline asm).
__device__ __forceinline__ f2 pk_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
// Broadcast one half of a coefficient pair: a shuffle the backend folds into op_sel / op_sel_hi.
__device__ __forceinline__ f2 lo(f2 v) { return __builtin_shufflevector(v, v, 0, 0); }
__device__ __forceinline__ f2 hi(f2 v) { return __builtin_shufflevector(v, v, 1, 1); }

}  // namespace mcv
