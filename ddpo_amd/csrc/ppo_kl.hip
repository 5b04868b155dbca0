// KL penalty to the frozen pretrained policy (`--kl_coef`; include/ddpo_ppo_kl.h): an additive pass behind the PPO launch.
// Both policies are Gaussians of the same sigma_c around means that are affine in the model output, so the KL and its gradient are closed
// forms in eps - ref: one read of the four U-Net outputs, one read-modify-write of the two gradient buffers.  One workgroup per row, the
// fixed-order block_sum of the other per-sample kernels, nothing shared between workgroups: bit-identical from run to run.
#include "ddim_coef.h"
#include "../../include/ddpo_ppo_kl.h"

extern "C" int ddpo_ppo_kl_abi_version(void) { return 1; }

namespace {

// old + inc, except that a zero increment leaves the word alone (-0.0f + 0.0f would flip its sign bit: a reference equal to the policy
// must leave the PPO gradient bit for bit as it was)
__device__ __forceinline__ float add_inc(float old, float inc) { return inc == 0.0f ? old : old + inc; }

__global__ void __launch_bounds__(1024) kl_ref_fwd_bwd_kernel(const float* __restrict__ eps_c, const float* __restrict__ eps_u,
                                                             const float* __restrict__ ref_c, const float* __restrict__ ref_u,
                                                             const int32_t* __restrict__ ts, float g, float kl_coef, int train_cfg,
                                                             ddpo_ddim_consts c, float* __restrict__ d_eps_c, float* __restrict__ d_eps_u,
                                                             float* __restrict__ kl_per_sample, int group, int chw) {
  __shared__ float red[16];
  const int b = blockIdx.x;
  const DdimCoef k = ddim_coef(c, ts[b]);
  const int64_t base = (int64_t)b * chw;
  // c_t = d mu / d e: the expressions of ppo_fwd_bwd_kernel (elementwise.hip)
  float dmu_de;
  if (c.pred_type == DDPO_PRED_EPSILON) dmu_de = k.dirc - k.sqrt_ap * k.sqrt_bt / k.sqrt_at;
  else dmu_de = k.dirc * k.sqrt_at - k.sqrt_ap * k.sqrt_bt;
  const float w = (dmu_de * dmu_de) / (k.std_c * k.std_c);                 // c_t^2 / sigma_c^2
  const float gcoef = (kl_coef / (float)group) * (w / (float)chw);
  float acc = 0.f;
  for (int i = threadIdx.x * 4; i < chw; i += blockDim.x * 4) {
    const float4 ec = *reinterpret_cast<const float4*>(eps_c + base + i);
    const float4 rc = *reinterpret_cast<const float4*>(ref_c + base + i);
    float4 eu = ec, ru = rc;
    if (train_cfg) {
      eu = *reinterpret_cast<const float4*>(eps_u + base + i);
      ru = *reinterpret_cast<const float4*>(ref_u + base + i);
    }
    float4 dc = *reinterpret_cast<const float4*>(d_eps_c + base + i);
    float4 du = dc;
    if (train_cfg) du = *reinterpret_cast<const float4*>(d_eps_u + base + i);
    const float* pec = &ec.x; const float* prc = &rc.x; const float* peu = &eu.x; const float* pru = &ru.x;
    float* pdc = &dc.x; float* pdu = &du.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float dlc = pec[j] - prc[j];
      const float dlu = peu[j] - pru[j];
      const float dl = train_cfg ? (dlu + g * (dlc - dlu)) : dlc;
      acc += dl * dl;
      const float de = gcoef * dl;
      pdc[j] = add_inc(pdc[j], train_cfg ? g * de : de);
      pdu[j] = add_inc(pdu[j], (1.0f - g) * de);
    }
    *reinterpret_cast<float4*>(d_eps_c + base + i) = dc;
    if (train_cfg) *reinterpret_cast<float4*>(d_eps_u + base + i) = du;
  }
  const float tot = block_sum(acc, red);
  if (threadIdx.x == 0) kl_per_sample[b] = (0.5f * w) * (tot / (float)chw);
}

// one wave per micro-batch (`group` consecutive rows), shaped like ppo_info_kernel: kl_info[j] = mean of its rows; loss column += kl_coef * that
__global__ void __launch_bounds__(64) kl_info_kernel(const float* __restrict__ kl_per_sample, float kl_coef, float* __restrict__ kl_info,
                                                    float* __restrict__ loss_info, int group) {
  const int b0 = blockIdx.x * group;
  float s = 0.f;
  for (int b = b0 + threadIdx.x; b < b0 + group; b += 64) s += kl_per_sample[b];
  s = wave_sum(s);
  if (threadIdx.x == 0) {
    const float m = s / (float)group;
    kl_info[blockIdx.x] = m;
    if (loss_info) loss_info[blockIdx.x * 3 + 2] = add_inc(loss_info[blockIdx.x * 3 + 2], kl_coef * m);
  }
}

inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace

extern "C" int ddpo_ddim_kl_ref_fwd_bwd(const float* eps_c, const float* eps_u, const float* ref_c, const float* ref_u, const int32_t* ts,
                                        float guidance_scale, float kl_coef, int train_cfg, const ddpo_ddim_consts* c, float* d_eps_c,
                                        float* d_eps_u, float* kl_per_sample, float* kl_info, float* loss_info, int B, int group, int chw,
                                        void* stream) {
  if (!eps_c || !ref_c || !ts || !c || !d_eps_c || !kl_per_sample || !kl_info) return DDPO_EINVAL;
  if (train_cfg && (!eps_u || !ref_u || !d_eps_u)) return DDPO_EINVAL;
  if (B <= 0 || group <= 0 || B % group || chw <= 0 || (chw & 3)) return DDPO_EINVAL;
  if (!(kl_coef >= 0.0f) || isinf(kl_coef)) return DDPO_EINVAL;          // negative, NaN or infinite
  if (c->pred_type != DDPO_PRED_EPSILON && c->pred_type != DDPO_PRED_V) return DDPO_EINVAL;
  if (misaligned(eps_c) || misaligned(ref_c) || misaligned(d_eps_c)) return DDPO_EINVAL;
  if (train_cfg && (misaligned(eps_u) || misaligned(ref_u) || misaligned(d_eps_u))) return DDPO_EINVAL;
  hipLaunchKernelGGL(kl_ref_fwd_bwd_kernel, dim3(B), dim3(1024), 0, as_stream(stream), eps_c, eps_u, ref_c, ref_u, ts, guidance_scale, kl_coef,
                     train_cfg, *c, d_eps_c, d_eps_u, kl_per_sample, group, chw);
  DDPO_LAUNCH_CHECK();
  hipLaunchKernelGGL(kl_info_kernel, dim3(B / group), dim3(64), 0, as_stream(stream), kl_per_sample, kl_coef, kl_info, loss_info, group);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}
