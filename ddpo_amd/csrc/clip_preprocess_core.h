// CLIP image preprocessing: the per-pixel integer arithmetic of an 8-bit two-pass bicubic resize (what Pillow's Image.resize does to an RGB
// image) as host + device inline functions.  csrc/clip_preprocess.hip runs them from its kernel and from the serial host entry
// (ddpo_clip_preprocess_host), so whether the bytes equal Pillow's is decided by the host entry against Pillow itself
// (tests/test_clip_preprocess_cpu.py) and the kernel only has to agree with the host entry.  csrc/resize_u8.hip runs the same functions to
// output the resized bytes themselves.  Plain C++17 but for the kernels' row staging at the bottom (under __HIPCC__): no HIP header is needed.
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

#if defined(__HIPCC__)
// Kernel side: `nr` rows of w3 = W x 3 elements, starting at element `row0` of `images`, into s_in[r * srow + e] as bytes — float32 truncated by
// cp_float_to_u8 — by the TB threads of a workgroup (thread t).  VEC: W % 4 == 0 and an aligned base, so rows start on 16 B (float) / 4 B (uint8)
// and four elements move at a time.  The caller synchronises.
template <bool F32, bool VEC, int TB>
__device__ inline void cp_stage_rows(const void* images, size_t row0, int nr, int w3, uint8_t* s_in, int srow, int t) {
  if (VEC) {
    const int q = w3 >> 2;
    for (int i = t; i < nr * q; i += TB) {
      const int r = i / q, e = (i - r * q) * 4;
      const size_t src = row0 + (size_t)r * w3 + e;
      uint32_t pk;
      if (F32) {
        const float4 v = *reinterpret_cast<const float4*>(static_cast<const float*>(images) + src);
        pk = (uint32_t)cp_float_to_u8(v.x) | ((uint32_t)cp_float_to_u8(v.y) << 8) | ((uint32_t)cp_float_to_u8(v.z) << 16) |
             ((uint32_t)cp_float_to_u8(v.w) << 24);
      } else {
        pk = *reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(images) + src);
      }
      *reinterpret_cast<uint32_t*>(s_in + r * srow + e) = pk;
    }
  } else {
    for (int i = t; i < nr * w3; i += TB) {
      const int r = i / w3, e = i - r * w3;
      const size_t src = row0 + (size_t)r * w3 + e;
      s_in[r * srow + e] = F32 ? (uint8_t)cp_float_to_u8(static_cast<const float*>(images)[src]) : static_cast<const uint8_t*>(images)[src];
    }
  }
}
#endif
