// What the translation units of the bf16 MFMA GEMM family share: gemm_bf16.hip (forward kernels, dispatch and entry points) and
// gemm_bf16_wgrad.hip (weight gradient).  gemm_bf16_pack.hip (weight / activation packers) needs common.h only.
#pragma once
#include "common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

#define BF_BK 32          // k-tile of the forward kernels
#define BF_THREADS 256    // workgroup of the four-wave tiles

// raw buffer addressing: a masked element carries this offset and the buffer unit returns zeros for it
#define BUF_OOB 0x80000000u
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7FFFFFFF, 0x00020000);
}
