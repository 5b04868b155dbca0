// Rescaled classifier-free guidance (`--guidance_rescale`; include/ddpo_cfg_rescale.h): the guided prediction of a v-prediction
// model is scaled per row so that its standard deviation moves towards the conditional prediction's.  The forward stands between the U-Net
// and the DDIM step / loss kernels, the backward between the loss kernels and the U-Net backward.  One workgroup per row reads the row
// several times (a 64 KB row stays in L2): means, then squared deviations, then the write.  The fixed-order block_sum of the other per-sample
// kernels, nothing shared between workgroups: bit-identical from run to run and independent of B.
#include <cmath>
#include "common.h"
#include "../../include/ddpo_cfg_rescale.h"

extern "C" int ddpo_cfg_rescale_abi_version(void) { return 1; }

namespace {

__global__ void __launch_bounds__(1024) cfg_rescale_fwd_kernel(const float* __restrict__ eps_c, const float* __restrict__ eps_u, float g,
                                                              float phi, float* __restrict__ out, float* __restrict__ stats, int chw) {
  __shared__ float red[16];
  const int b = blockIdx.x;
  const int64_t base = (int64_t)b * chw;
  float acc_t = 0.f, acc_c = 0.f;
  for (int i = threadIdx.x * 4; i < chw; i += blockDim.x * 4) {
    const float4 t4 = *reinterpret_cast<const float4*>(eps_c + base + i);
    const float4 u4 = *reinterpret_cast<const float4*>(eps_u + base + i);
    const float* pt = &t4.x; const float* pu = &u4.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc_t += pt[j];
      acc_c += pu[j] + g * (pt[j] - pu[j]);
    }
  }
  const float mt = block_sum(acc_t, red) / (float)chw;
  const float mc = block_sum(acc_c, red) / (float)chw;
  float dev_t = 0.f, dev_c = 0.f;
  for (int i = threadIdx.x * 4; i < chw; i += blockDim.x * 4) {
    const float4 t4 = *reinterpret_cast<const float4*>(eps_c + base + i);
    const float4 u4 = *reinterpret_cast<const float4*>(eps_u + base + i);
    const float* pt = &t4.x; const float* pu = &u4.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float dt = pt[j] - mt;
      const float dc = (pu[j] + g * (pt[j] - pu[j])) - mc;
      dev_t += dt * dt;
      dev_c += dc * dc;
    }
  }
  const float st = sqrtf(block_sum(dev_t, red) / (float)(chw - 1));
  const float sc = sqrtf(block_sum(dev_c, red) / (float)(chw - 1));
  const float k = (1.0f - phi) + phi * (st / sc);             // sc == 0: inf / NaN, as the formula gives it
  if (threadIdx.x == 0) {
    stats[b * 4 + 0] = mt;
    stats[b * 4 + 1] = st;
    stats[b * 4 + 2] = mc;
    stats[b * 4 + 3] = sc;
  }
  for (int i = threadIdx.x * 4; i < chw; i += blockDim.x * 4) {
    const float4 t4 = *reinterpret_cast<const float4*>(eps_c + base + i);
    const float4 u4 = *reinterpret_cast<const float4*>(eps_u + base + i);
    const float* pt = &t4.x; const float* pu = &u4.x;
    float4 o4;
    float* po = &o4.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) po[j] = k * (pu[j] + g * (pt[j] - pu[j]));
    *reinterpret_cast<float4*>(out + base + i) = o4;
  }
}

__global__ void __launch_bounds__(1024) cfg_rescale_bwd_kernel(const float* __restrict__ eps_c, const float* __restrict__ eps_u,
                                                              const float* __restrict__ d_out, const float* __restrict__ stats, float g,
                                                              float phi, float* __restrict__ d_eps_c, float* __restrict__ d_eps_u, int chw) {
  __shared__ float red[16];
  const int b = blockIdx.x;
  const int64_t base = (int64_t)b * chw;
  const float mt = stats[b * 4 + 0], st = stats[b * 4 + 1], mc = stats[b * 4 + 2], sc = stats[b * 4 + 3];
  float acc = 0.f;
  for (int i = threadIdx.x * 4; i < chw; i += blockDim.x * 4) {
    const float4 t4 = *reinterpret_cast<const float4*>(eps_c + base + i);
    const float4 u4 = *reinterpret_cast<const float4*>(eps_u + base + i);
    const float4 g4 = *reinterpret_cast<const float4*>(d_out + base + i);
    const float* pt = &t4.x; const float* pu = &u4.x; const float* pg = &g4.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc += pg[j] * (pu[j] + g * (pt[j] - pu[j]));
  }
  const float S = block_sum(acc, red);
  const float r = st / sc;
  const float k = (1.0f - phi) + phi * r;
  const float nm1 = (float)(chw - 1);
  const float ca = (S * phi) * r / (nm1 * (sc * sc));          // the weight of (c_i - mean c) in dL/dc
  const float cb = (S * phi) / (nm1 * (st * sc));              // the weight of (t_i - mean t) in dL/dt
  for (int i = threadIdx.x * 4; i < chw; i += blockDim.x * 4) {
    const float4 t4 = *reinterpret_cast<const float4*>(eps_c + base + i);
    const float4 u4 = *reinterpret_cast<const float4*>(eps_u + base + i);
    const float4 g4 = *reinterpret_cast<const float4*>(d_out + base + i);
    const float* pt = &t4.x; const float* pu = &u4.x; const float* pg = &g4.x;
    float4 dt4, du4;
    float* pdt = &dt4.x; float* pdu = &du4.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float c = pu[j] + g * (pt[j] - pu[j]);
      const float dc = k * pg[j] - ca * (c - mc);
      pdt[j] = g * dc + cb * (pt[j] - mt);
      pdu[j] = (1.0f - g) * dc;
    }
    *reinterpret_cast<float4*>(d_eps_c + base + i) = dt4;
    *reinterpret_cast<float4*>(d_eps_u + base + i) = du4;
  }
}

inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
inline bool bad_geometry(int B, int chw) { return B <= 0 || chw <= 0 || (chw & 3) || chw < 8; }
inline bool bad_rescale(float phi) { return !(phi >= 0.0f && phi <= 1.0f); }          // NaN, infinite or outside [0, 1]

}  // namespace

extern "C" int ddpo_cfg_rescale_fwd(const float* eps_c, const float* eps_u, float guidance_scale, float guidance_rescale, float* out,
                                    float* stats, int B, int chw, void* stream) {
  if (!eps_c || !eps_u || !out || !stats) return DDPO_EINVAL;
  if (bad_geometry(B, chw) || bad_rescale(guidance_rescale)) return DDPO_EINVAL;
  if (misaligned(eps_c) || misaligned(eps_u) || misaligned(out)) return DDPO_EINVAL;
  hipLaunchKernelGGL(cfg_rescale_fwd_kernel, dim3(B), dim3(1024), 0, as_stream(stream), eps_c, eps_u, guidance_scale, guidance_rescale, out,
                     stats, chw);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

extern "C" int ddpo_cfg_rescale_bwd(const float* eps_c, const float* eps_u, const float* d_out, const float* stats, float guidance_scale,
                                    float guidance_rescale, float* d_eps_c, float* d_eps_u, int B, int chw, void* stream) {
  if (!eps_c || !eps_u || !d_out || !stats || !d_eps_c || !d_eps_u) return DDPO_EINVAL;
  if (bad_geometry(B, chw) || bad_rescale(guidance_rescale)) return DDPO_EINVAL;
  if (misaligned(eps_c) || misaligned(eps_u) || misaligned(d_out) || misaligned(d_eps_c) || misaligned(d_eps_u)) return DDPO_EINVAL;
  hipLaunchKernelGGL(cfg_rescale_bwd_kernel, dim3(B), dim3(1024), 0, as_stream(stream), eps_c, eps_u, d_out, stats, guidance_scale,
                     guidance_rescale, d_eps_c, d_eps_u, chw);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}
