// CLIP image preprocessing: the per-pixel integer arithmetic of an 8-bit two-pass bicubic resize (what Pillow's Image.resize does to an RGB
// image) as host + device inline functions.  csrc/clip_preprocess.hip runs them from its kernel and from the serial host entry
// (ddpo_clip_preprocess_host), so whether the bytes equal Pillow's is decided by the host entry against Pillow itself
// (tests/test_clip_preprocess_cpu.py) and the kernel only has to agree with the host entry.  Plain C++17: no HIP header is needed.
//
// Everything here is integer once the pixel is a byte: the coefficient tables arrive as 22-bit fixed-point int32 (built by the caller in double
// precision, lib.clip_preprocess_tables), a pass is acc = 2^21 + sum(pixel * coeff), result = clamp(acc >> 22, 0, 255), and the horizontal
// pass is rounded to a byte before the vertical pass reads it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CP_HD __host__ __device__ inline
#else
#define CP_HD inline
#endif

#define CP_PRECISION_BITS 22            // 32 - 8 - 2: a byte times a coefficient, summed over a kernel with negative lobes, stays inside int32

// (uint8)(x * 255.0f) for x in [0, 1]: the product in fp32, truncated; outside that range clamped to 0..255, NaN -> 0
CP_HD int cp_float_to_u8(float x) {
  const float v = x * 255.0f;
  if (!(v >= 0.0f)) return 0;           // negative or NaN
  return v >= 255.0f ? 255 : (int)v;
}

CP_HD int cp_round_clamp(int acc) {
  const int v = acc >> CP_PRECISION_BITS;          // arithmetic shift: the accumulator may be negative
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// One output byte of one pass: `count` taps over bytes `stride` apart
CP_HD int cp_taps(const uint8_t* px, int stride, const int32_t* coef, int count) {
  int acc = 1 << (CP_PRECISION_BITS - 1);
  for (int k = 0; k < count; ++k) acc += (int)px[(size_t)k * stride] * coef[k];
  return cp_round_clamp(acc);
}

// Bytes of LDS one workgroup of the kernel uses: `rows` horizontally resampled rows of size x 3 bytes + CP_STAGE_ROWS input rows of W x 3 bytes
// (each rounded up to 16) + the 256 x 3 normalisation table.  The supported domain is "this fits CP_LDS_LIMIT" for the device and the host entry alike.
#define CP_STAGE_ROWS 8
#define CP_LDS_LIMIT (160 * 1024)
CP_HD size_t cp_row_bytes(int pixels) { return ((size_t)pixels * 3 + 15) & ~(size_t)15; }
CP_HD size_t cp_lds_bytes(int rows, int size, int W) {
  return (size_t)rows * cp_row_bytes(size) + (size_t)CP_STAGE_ROWS * cp_row_bytes(W) + 256 * 3 * sizeof(float);
}
