// The byte-image front end of the device rewards (csrc/jpeg_size.hip, clip_preprocess.hip, resize_u8.hip, symmetry.hip): how an N x H x W x 3
// batch, uint8 or float32 in [0, 1], becomes bytes, on the host and on the device alike, and what the entries that take such a batch decide from
// its pointer before they launch.  Host + device inline functions; plain C++17 but for the part under __HIPCC__ (row staging into LDS, the
// large-LDS attribute), so the stand-alone host checks of tools/native include it without a HIP compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <type_traits>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define IU_HD __host__ __device__ inline
#else
#define IU_HD inline
#endif

// (uint8)(x * 255.0f) for x in [0, 1]: the product in fp32, truncated; outside that range clamped to 0..255, NaN -> 0.  The clamp comes before
// the conversion: no float that does not fit an int is ever cast.
IU_HD int iu_float_to_u8(float x) {
  const float v = x * 255.0f;
  if (!(v >= 0.0f)) return 0;           // negative or NaN
  return v >= 255.0f ? 255 : (int)v;
}

IU_HD int iu_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Bytes of a row of `pixels` RGB pixels kept in LDS: rounded up to 16
IU_HD size_t iu_row_bytes(int pixels) { return ((size_t)pixels * 3 + 15) & ~(size_t)15; }

// Element i of a batch as a byte: what the serial host entries read
inline int iu_byte(const void* images, int is_float32, size_t i) {
  return is_float32 ? iu_float_to_u8(static_cast<const float*>(images)[i]) : (int)static_cast<const uint8_t*>(images)[i];
}

// float32 input that is not aligned to its element: every entry refuses it
inline bool iu_misaligned(const void* images, int is_float32) { return is_float32 && (reinterpret_cast<uintptr_t>(images) & 3); }

// Four elements may move at a time: rows of W pixels start on a multiple of 4 elements and the base is aligned to the load (16 B float, 4 B uint8)
inline bool iu_vec_ok(const void* images, int is_float32, int W) {
  return (W & 3) == 0 && (reinterpret_cast<uintptr_t>(images) & (is_float32 ? 15 : 3)) == 0;
}

// Run-time bools as std::bool_constant arguments of a generic lambda: iu_dispatch(is_float32, vec, [&](auto F32, auto VEC) { launch
// kernel<F32(), VEC()> }) instantiates and reaches all four kernels from one line.
template <class Fn>
inline auto iu_dispatch(bool a, Fn&& fn) {
  return a ? fn(std::true_type{}) : fn(std::false_type{});
}
template <class Fn>
inline auto iu_dispatch(bool a, bool b, Fn&& fn) {
  return iu_dispatch(a, [&](auto A) { return iu_dispatch(b, [&](auto B) { return fn(A, B); }); });
}

#if defined(__HIPCC__)
// Kernel side: `rows` rows of `count` elements, `src_stride` elements apart from element `src0` of `images` on, into bytes `dst_stride` apart —
// float32 truncated by iu_float_to_u8 — by the TB threads of a workgroup (thread t).  VEC: count, src0 and src_stride are multiples of 4, dst
// and dst_stride too, and iu_vec_ok holds.  The caller synchronises.
template <bool F32, bool VEC, int TB>
__device__ __forceinline__ void iu_stage(uint8_t* dst, int dst_stride, const void* images, size_t src0, size_t src_stride, int rows, int count,
                                         int t) {
  if (VEC) {
    const int q = count >> 2;
    for (int i = t; i < rows * q; i += TB) {
      const int r = i / q, e = (i - r * q) * 4;
      const size_t src = src0 + (size_t)r * src_stride + e;
      uint32_t pk;
      if (F32) {
        const float4 v = *reinterpret_cast<const float4*>(static_cast<const float*>(images) + src);
        pk = (uint32_t)iu_float_to_u8(v.x) | ((uint32_t)iu_float_to_u8(v.y) << 8) | ((uint32_t)iu_float_to_u8(v.z) << 16) |
             ((uint32_t)iu_float_to_u8(v.w) << 24);
      } else {
        pk = *reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(images) + src);
      }
      *reinterpret_cast<uint32_t*>(dst + r * dst_stride + e) = pk;
    }
  } else {
    for (int i = t; i < rows * count; i += TB) {
      const int r = i / count, e = i - r * count;
      const size_t src = src0 + (size_t)r * src_stride + e;
      dst[r * dst_stride + e] = F32 ? (uint8_t)iu_float_to_u8(static_cast<const float*>(images)[src]) : static_cast<const uint8_t*>(images)[src];
    }
  }
}

// A kernel that asks for more dynamic LDS than the 64 KB default is told so once, before its first launch
template <auto Kernel>
inline void iu_large_lds(int bytes) {
  static const hipError_t once = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  (void)once;
}
#endif
