// linear_split.hpp — the pieces the split-bf16 MFMA products share (linear.hip:
// the node projections; linear_rhs.hip: the projected aggregation's output GEMM
// with the RHS / Runge-Kutta epilogue): tile constants, the row loads and the
// exact three-piece bf16 split of an f32 operand.
#pragma once
#include "common.hpp"

namespace gnpde {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kLinRowsPerWave = 32;
constexpr int kLinCols = 64;

// x elements as fp32: fp32 storage, or bf16 storage widened exactly (a bf16 state's
// projection reads it directly: the same values, so the same products and bits as
// the projection of its fp32 copy)
template <class XT>
__device__ __forceinline__ float4 lin_load4(const XT* __restrict__ p) {
  if constexpr (sizeof(XT) == 4) {
    return *reinterpret_cast<const float4*>(p);
  } else {
    const u32x2 w = *reinterpret_cast<const u32x2*>(p);
    return make_float4(__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u), __uint_as_float(w.y << 16),
                       __uint_as_float(w.y & 0xffff0000u));
  }
}
template <class XT>
__device__ __forceinline__ float lin_load1(const XT* __restrict__ p) {
  if constexpr (sizeof(XT) == 4)
    return *p;
  else
    return __uint_as_float((uint32_t)(*reinterpret_cast<const uint16_t*>(p)) << 16);
}

// ------------------------------------------------------------------ split-bf16 operands
// Every f32 operand is split EXACTLY into three bf16 pieces, v = v0 + v1 + v2
// (v0 = RNE(v), v1 = RNE(v - v0), v2 = v - v0 - v1: each residual keeps at most
// 16, then 8 significant bits); linear.hip says which products are kept.
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// one v_cvt_pk_bf16_f32 (RNE) per pair; the pair's f32 values of the pieces
// are the dword's halves moved to the high bits (shift / mask), the residuals
// one packed subtraction
__device__ __forceinline__ void split_pair(f32x2_t v, uint32_t& p0, uint32_t& p1, uint32_t& p2) {
  auto widen = [](uint32_t p) {
    const f32x2_t w = {__uint_as_float(p << 16), __uint_as_float(p & 0xffff0000u)};
    return w;
  };
  p0 = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
  const f32x2_t r1 = v - widen(p0);
  p1 = __builtin_bit_cast(uint32_t, __builtin_convertvector(r1, bf16x2_t));
  const f32x2_t r2 = r1 - widen(p1);
  p2 = __builtin_bit_cast(uint32_t, __builtin_convertvector(r2, bf16x2_t));
}

__device__ __forceinline__ void split3(const float4& lo, const float4& hi, bf16x8_t& p0, bf16x8_t& p1,
                                       bf16x8_t& p2) {
  uint32_t a0, a1, a2, a3, b0, b1, b2, b3, c0, c1, c2, c3;
  const f32x2_t v0 = {lo.x, lo.y}, v1 = {lo.z, lo.w}, v2 = {hi.x, hi.y}, v3 = {hi.z, hi.w};
  split_pair(v0, a0, b0, c0);
  split_pair(v1, a1, b1, c1);
  split_pair(v2, a2, b2, c2);
  split_pair(v3, a3, b3, c3);
  const u32x4_t a = {a0, a1, a2, a3}, b = {b0, b1, b2, b3}, c = {c0, c1, c2, c3};
  p0 = __builtin_bit_cast(bf16x8_t, a);
  p1 = __builtin_bit_cast(bf16x8_t, b);
  p2 = __builtin_bit_cast(bf16x8_t, c);
}

}  // namespace gnpde
