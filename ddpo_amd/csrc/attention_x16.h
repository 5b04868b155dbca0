// What the attention kernels of the 16-bit MFMA datapaths share (attention_bf16.hip: forward, attention_bwd_bf16.hip: backward): vector types,
// the two 32x32x16 MFMAs, the packed conversions and hi / lo splits, and the fragment helpers of the operand-chaining trick (the 32x32
// accumulator fragment of one product becomes, in registers, the B operand of the next).
#pragma once
#include "common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)
#define MFMA32H(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16((a), (b), (c), 0, 0, 0)

// Two floats -> packed bf16 / f16 pair, round to nearest even (v_cvt_pk_bf16_f32, v_cvt_pk_f16_f32).  Deliberately NOT inline assembly: the
// operands are the results of v_exp_f32, a transcendental-unit instruction, and gfx950 needs a wait state between a TRANS result and a VALU
// consumer — the compiler's hazard recognizer inserts it for instructions it selects itself and does not look inside an asm statement (round 4:
// the asm form read stale registers whenever the scheduler put the last exponential of a pair directly in front of it: ~10 % errors on long key
// sequences, NaNs at d = 64).  Nothing in the attention files may convert through an asm statement, whatever its operands are today.
__device__ __forceinline__ uint32_t cvt_pk_bf16_a(float lo, float hi) {
  const bf16x2 v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(uint32_t, v);
}
__device__ __forceinline__ uint32_t cvt_pk_f16_a(float lo, float hi) {
  const f16x2 v = {(_Float16)lo, (_Float16)hi};
  return __builtin_bit_cast(uint32_t, v);
}
// two floats -> packed bf16 hi pair and packed bf16 lo pair
__device__ __forceinline__ void split2(float a, float b, uint32_t& hi, uint32_t& lo) {
  hi = cvt_pk_bf16_a(a, b);
  lo = cvt_pk_bf16_a(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xFFFF0000u));
}
// two floats -> packed f16 hi pair and packed f16 lo pair; magnitudes beyond `lim` saturate (the forward clamps its V operand to the f16
// maximum 65504, the backward everything to 60000)
__device__ __forceinline__ void split2h(float a, float b, uint32_t& hi, uint32_t& lo, float lim) {
  a = fminf(fmaxf(a, -lim), lim);
  b = fminf(fmaxf(b, -lim), lim);
  hi = cvt_pk_f16_a(a, b);
  const f16x2 h = __builtin_bit_cast(f16x2, hi);
  lo = cvt_pk_f16_a(a - (float)h[0], b - (float)h[1]);
}

// 8 floats (held as 8 accumulator registers) -> bf16 B-operand fragments hi / lo
__device__ __forceinline__ void frag8(const float* v, bf16x8& hi, bf16x8& lo) {
  uint32_t h[4], l[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) split2(v[2 * e], v[2 * e + 1], h[e], l[e]);
  hi = __builtin_bit_cast(bf16x8, make_uint4(h[0], h[1], h[2], h[3]));
  lo = __builtin_bit_cast(bf16x8, make_uint4(l[0], l[1], l[2], l[3]));
}
// 8 floats -> ONE f16 B-operand fragment
__device__ __forceinline__ f16x8 frag8h(const float* v) {
  return __builtin_bit_cast(f16x8, make_uint4(cvt_pk_f16_a(v[0], v[1]), cvt_pk_f16_a(v[2], v[3]), cvt_pk_f16_a(v[4], v[5]), cvt_pk_f16_a(v[6], v[7])));
}
// 8 floats -> f16 hi / lo fragments
__device__ __forceinline__ void frag8h2(const float* v, f16x8& hi, f16x8& lo, float lim) {
  uint32_t h[4], l[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) split2h(v[2 * e], v[2 * e + 1], h[e], l[e], lim);
  hi = __builtin_bit_cast(f16x8, make_uint4(h[0], h[1], h[2], h[3]));
  lo = __builtin_bit_cast(f16x8, make_uint4(l[0], l[1], l[2], l[3]));
}
// row-major fragment: 8 consecutive 16-bit values at (row, col0) of an image with `ld` elements per row
template <typename V8>
__device__ __forceinline__ V8 ld_rm(const char* base, int ld, int row, int col0) {
  return *reinterpret_cast<const V8*>(base + (row * ld + col0) * 2);
}
// transposed fragment: image [row][slot]; slots {s0..s0+3, s0+8..s0+11} — the rows of a 32x32 accumulator that one lane half holds
template <typename V8>
__device__ __forceinline__ V8 ld_tr(const char* base, int ld, int row, int s0) {
  const uint2 a = *reinterpret_cast<const uint2*>(base + (row * ld + s0) * 2);
  const uint2 b = *reinterpret_cast<const uint2*>(base + (row * ld + s0 + 8) * 2);
  return __builtin_bit_cast(V8, make_uint4(a.x, a.y, b.x, b.y));
}
// transposed scatter: the packed hi / lo pairs of features f0 .. f0 + 3 of token `tok` into the images [feature][token] tr_hi / tr_lo
__device__ __forceinline__ void scatter_tr(char* tr_hi, char* tr_lo, int ldtr, int tok, int f0, uint32_t h0, uint32_t h1, uint32_t l0, uint32_t l1) {
  uint16_t* th = reinterpret_cast<uint16_t*>(tr_hi);
  uint16_t* tl = reinterpret_cast<uint16_t*>(tr_lo);
  th[(f0 + 0) * ldtr + tok] = (uint16_t)(h0 & 0xFFFFu); th[(f0 + 1) * ldtr + tok] = (uint16_t)(h0 >> 16);
  th[(f0 + 2) * ldtr + tok] = (uint16_t)(h1 & 0xFFFFu); th[(f0 + 3) * ldtr + tok] = (uint16_t)(h1 >> 16);
  tl[(f0 + 0) * ldtr + tok] = (uint16_t)(l0 & 0xFFFFu); tl[(f0 + 1) * ldtr + tok] = (uint16_t)(l0 >> 16);
  tl[(f0 + 2) * ldtr + tok] = (uint16_t)(l1 & 0xFFFFu); tl[(f0 + 3) * ldtr + tok] = (uint16_t)(l1 >> 16);
}
