// The pre-pass of the attention backward (attention_bwd_bf16.hip, both datapaths; attention_bwd.hip still carries a private copy of the
// AMAX == false form):
//   D[b,h,q] = sum_j dO[q][h*d+j] * O[q][h*d+j]
// AMAX (the f16mx datapath): also amax[b*heads+h] = max |dO| over the (batch, head) slab, as float bits — non-negative floats order like unsigned
// integers; the caller zeroes the buffer before the launch.  AMAX == false never touches `amax`.
#pragma once
#include "common.h"

template <bool AMAX>
static __global__ void __launch_bounds__(256) attn_dvec_kernel(const float* __restrict__ o, const float* __restrict__ d_o, float* __restrict__ dvec,
                                                        uint32_t* __restrict__ amax, int B, int heads, int Nq, int d) {
  const int64_t total = (int64_t)B * Nq * heads;
  const int C = heads * d;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int h = (int)(i % heads);
    const int64_t row = i / heads;
    const int b = (int)(row / Nq), q = (int)(row - (int64_t)b * Nq);
    const float4* po = reinterpret_cast<const float4*>(o + row * C + h * d);
    const float4* pd = reinterpret_cast<const float4*>(d_o + row * C + h * d);
    float s = 0.f, m = 0.f;
    for (int j = 0; j < d / 4; ++j) {
      const float4 a = po[j], c = pd[j];
      s += (a.x * c.x + a.y * c.y) + (a.z * c.z + a.w * c.w);
      if (AMAX) m = fmaxf(fmaxf(m, fmaxf(fabsf(c.x), fabsf(c.y))), fmaxf(fabsf(c.z), fabsf(c.w)));
    }
    dvec[((int64_t)b * heads + h) * Nq + q] = s;
    if (AMAX && m < INFINITY) {                           // (NaN / inf gradients propagate through the products anyway)
      uint32_t* slot = amax + (b * heads + h);
      const uint32_t bits = __float_as_uint(m);
      if (bits > *reinterpret_cast<volatile uint32_t*>(slot)) atomicMax(slot, bits);
    }
  }
}

// one thread per (batch, query, head), grid-stride beyond 8192 blocks
template <bool AMAX>
static void launch_attn_dvec(const float* o, const float* d_o, float* dvec, uint32_t* amax, int B, int heads, int Nq, int d, hipStream_t st) {
  int64_t blocks = ((int64_t)B * Nq * heads + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(attn_dvec_kernel<AMAX>, dim3((int)blocks), dim3(256), 0, st, o, d_o, dvec, amax, B, heads, Nq, d);
}
