// Preference-pair loss against the frozen pretrained policy (`--pg_loss d3po`; include/ddpo_pref.h): the pass that stands in
// the place of the PPO launch.  The policy-to-pretrained log-ratio of a stored transition is a closed form in eps - ref (no difference of two
// log-probs), so one workgroup per pair reads the four U-Net outputs and the transition of its two rows twice: once for the two sums per row,
// once to write the gradient.  The fixed-order block_sum of the other per-sample kernels, nothing shared between workgroups: bit-identical
// from run to run.
#include "ddim_coef.h"
#include "../../include/ddpo_pref.h"

extern "C" int ddpo_pref_abi_version(void) { return 1; }

namespace {

// mean of the DDIM posterior given the (guided) model output e and the current sample x: ddim_mean of elementwise.hip, restated here
// operation for operation for the two prediction types the entry accepts (that unit is left as it is), so r = x' - mu is the float the
// PPO kernel forms
__device__ __forceinline__ float ddim_mean(const DdimCoef& k, int pred_type, float e, float x) {
  float x0;
  if (pred_type == DDPO_PRED_EPSILON) {
    x0 = (x - k.sqrt_bt * e) / k.sqrt_at;
  } else {
    x0 = k.sqrt_at * x - k.sqrt_bt * e;
    e = k.sqrt_at * e + k.sqrt_bt * x;
  }
  return k.sqrt_ap * x0 + k.dirc * e;
}

// c_t = d mu / d e: the expressions of ppo_fwd_bwd_kernel (elementwise.hip)
__device__ __forceinline__ float dmu_de_of(const DdimCoef& k, int pred_type) {
  if (pred_type == DDPO_PRED_EPSILON) return k.dirc - k.sqrt_ap * k.sqrt_bt / k.sqrt_at;
  return k.dirc * k.sqrt_at - k.sqrt_ap * k.sqrt_bt;
}

__global__ void __launch_bounds__(1024) pref_fwd_bwd_kernel(const float* __restrict__ eps_c, const float* __restrict__ eps_u,
                                                           const float* __restrict__ ref_c, const float* __restrict__ ref_u,
                                                           const float* __restrict__ x, const float* __restrict__ x_next,
                                                           const int32_t* __restrict__ ts, const float* __restrict__ pref, float g, float beta,
                                                           int train_cfg, ddpo_ddim_consts c, float* __restrict__ d_eps_c,
                                                           float* __restrict__ d_eps_u, float* __restrict__ per_pair, int group, int chw) {
  __shared__ float red[16];
  const int p = blockIdx.x;
  float h[2], dh_de[2];                            // per row: the log-ratio, and c_t / (sigma^2 chw) of d h / d e = that * r
#pragma unroll
  for (int row = 0; row < 2; ++row) {
    const int b = 2 * p + row;
    const DdimCoef k = ddim_coef(c, ts[b]);         // each row its own timestep
    const int64_t base = (int64_t)b * chw;
    const float ct = dmu_de_of(k, c.pred_type);
    const float var = k.std_c * k.std_c;
    float acc_rd = 0.f, acc_dd = 0.f;
    for (int i = threadIdx.x * 4; i < chw; i += blockDim.x * 4) {
      const float4 ec = *reinterpret_cast<const float4*>(eps_c + base + i);
      const float4 rc = *reinterpret_cast<const float4*>(ref_c + base + i);
      float4 eu = ec, ru = rc;
      if (train_cfg) {
        eu = *reinterpret_cast<const float4*>(eps_u + base + i);
        ru = *reinterpret_cast<const float4*>(ref_u + base + i);
      }
      const float4 xv = *reinterpret_cast<const float4*>(x + base + i);
      const float4 xn = *reinterpret_cast<const float4*>(x_next + base + i);
      const float* pec = &ec.x; const float* prc = &rc.x; const float* peu = &eu.x; const float* pru = &ru.x;
      const float* px = &xv.x; const float* pn = &xn.x;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float dlc = pec[j] - prc[j];
        const float dlu = peu[j] - pru[j];
        const float dl = train_cfg ? (dlu + g * (dlc - dlu)) : dlc;
        const float e = train_cfg ? (peu[j] + g * (pec[j] - peu[j])) : pec[j];
        const float r = pn[j] - ddim_mean(k, c.pred_type, e, px[j]);
        acc_rd += r * dl;
        acc_dd += dl * dl;
      }
    }
    const float s_rd = block_sum(acc_rd, red);
    const float s_dd = block_sum(acc_dd, red);
    h[row] = (2.0f * ct * s_rd + (ct * ct) * s_dd) / (2.0f * var * (float)chw);
    dh_de[row] = ct / (var * (float)chw);
  }
  // every thread holds both h: the pair's scalars are formed redundantly, from the same floats in the same order
  const float y = (pref[2 * p] - pref[2 * p + 1]) * 0.5f;
  const float s = (y == 0.0f) ? 0.0f : beta * y * (h[0] - h[1]);  // a tie: +0.0, whichever row comes first
  const float loss = fabsf(y) * (fmaxf(-s, 0.0f) + log1pf(expf(-fabsf(s))));
  float q;
  if (s >= 0.0f) { const float t = expf(-s); q = t / (1.0f + t); }
  else q = 1.0f / (1.0f + expf(s));
  if (threadIdx.x == 0) {
    per_pair[p * 4 + 0] = h[0];
    per_pair[p * 4 + 1] = h[1];
    per_pair[p * 4 + 2] = s;
    per_pair[p * 4 + 3] = (y == 0.0f) ? 0.0f : loss;
  }
  const float dl_even = -(beta * y * q) / (float)(group / 2);     // d loss_j / d h_2p; the odd row's is its negative
#pragma unroll
  for (int row = 0; row < 2; ++row) {
    const int b = 2 * p + row;
    const int64_t base = (int64_t)b * chw;
    if (y == 0.0f) {                                // a tie: +0.0, whatever the signs of the factors
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int i = threadIdx.x * 4; i < chw; i += blockDim.x * 4) {
        *reinterpret_cast<float4*>(d_eps_c + base + i) = z;
        if (train_cfg) *reinterpret_cast<float4*>(d_eps_u + base + i) = z;
      }
      continue;
    }
    const DdimCoef k = ddim_coef(c, ts[b]);
    const float coef = (row == 0 ? dl_even : -dl_even) * dh_de[row];
    for (int i = threadIdx.x * 4; i < chw; i += blockDim.x * 4) {
      const float4 ec = *reinterpret_cast<const float4*>(eps_c + base + i);
      float4 eu = ec;
      if (train_cfg) eu = *reinterpret_cast<const float4*>(eps_u + base + i);
      const float4 xv = *reinterpret_cast<const float4*>(x + base + i);
      const float4 xn = *reinterpret_cast<const float4*>(x_next + base + i);
      const float* pec = &ec.x; const float* peu = &eu.x; const float* px = &xv.x; const float* pn = &xn.x;
      float4 dc, du;
      float* pdc = &dc.x; float* pdu = &du.x;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float e = train_cfg ? (peu[j] + g * (pec[j] - peu[j])) : pec[j];
        const float r = pn[j] - ddim_mean(k, c.pred_type, e, px[j]);
        const float de = coef * r;
        pdc[j] = train_cfg ? g * de : de;
        pdu[j] = (1.0f - g) * de;
      }
      *reinterpret_cast<float4*>(d_eps_c + base + i) = dc;
      if (train_cfg) *reinterpret_cast<float4*>(d_eps_u + base + i) = du;
    }
  }
}

// one wave per micro-batch (`group` consecutive rows = group / 2 pairs), shaped like kl_info_kernel: info[j] = {pref_acc, pref_margin, loss}
__global__ void __launch_bounds__(64) pref_info_kernel(const float* __restrict__ per_pair, const float* __restrict__ pref,
                                                      float* __restrict__ info, int group) {
  const int n = group / 2;
  const int p0 = blockIdx.x * n;
  float acc = 0.f, mg = 0.f, ls = 0.f;
  for (int p = p0 + threadIdx.x; p < p0 + n; p += 64) {
    const float y = (pref[2 * p] - pref[2 * p + 1]) * 0.5f;
    const float m = y * (per_pair[p * 4 + 0] - per_pair[p * 4 + 1]);
    acc += (y != 0.0f && m > 0.0f) ? 1.0f : 0.0f;
    mg += m;
    ls += per_pair[p * 4 + 3];
  }
  acc = wave_sum(acc); mg = wave_sum(mg); ls = wave_sum(ls);
  if (threadIdx.x == 0) {
    info[blockIdx.x * 3 + 0] = acc / (float)n;
    info[blockIdx.x * 3 + 1] = mg / (float)n;
    info[blockIdx.x * 3 + 2] = ls / (float)n;
  }
}

inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace

extern "C" int ddpo_ddim_pref_fwd_bwd(const float* eps_c, const float* eps_u, const float* ref_c, const float* ref_u, const float* x,
                                      const float* x_next, const int32_t* ts, const float* pref, float guidance_scale, float beta,
                                      int train_cfg, const ddpo_ddim_consts* c, float* d_eps_c, float* d_eps_u, float* per_pair, float* info,
                                      int B, int group, int chw, void* stream) {
  if (!eps_c || !ref_c || !x || !x_next || !ts || !pref || !c || !d_eps_c || !per_pair || !info) return DDPO_EINVAL;
  if (train_cfg && (!eps_u || !ref_u || !d_eps_u)) return DDPO_EINVAL;
  if (B <= 0 || (B & 1) || group <= 0 || (group & 1) || B % group || chw <= 0 || (chw & 3)) return DDPO_EINVAL;
  if (!(beta > 0.0f) || isinf(beta)) return DDPO_EINVAL;                 // zero, negative, NaN or infinite
  if (c->pred_type != DDPO_PRED_EPSILON && c->pred_type != DDPO_PRED_V) return DDPO_EINVAL;
  if (misaligned(eps_c) || misaligned(ref_c) || misaligned(x) || misaligned(x_next) || misaligned(d_eps_c)) return DDPO_EINVAL;
  if (train_cfg && (misaligned(eps_u) || misaligned(ref_u) || misaligned(d_eps_u))) return DDPO_EINVAL;
  hipLaunchKernelGGL(pref_fwd_bwd_kernel, dim3(B / 2), dim3(1024), 0, as_stream(stream), eps_c, eps_u, ref_c, ref_u, x, x_next, ts, pref,
                     guidance_scale, beta, train_cfg, *c, d_eps_c, d_eps_u, per_pair, group, chw);
  DDPO_LAUNCH_CHECK();
  hipLaunchKernelGGL(pref_info_kernel, dim3(B / group), dim3(64), 0, as_stream(stream), per_pair, pref, info, group);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}
