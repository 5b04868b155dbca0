// Diffusion-DPO loss on ranked pairs of stored samples (`pipeline/dpo.py`; include/ddpo_dpo.h): the pass that stands in the
// place of the RWR loss launch.  The policy's denoising error minus the frozen reference's is a closed form in delta = eps - ref (no
// difference of two mean squared errors), so one workgroup per pair reads the U-Net outputs, the reference's and the target of its two rows
// twice: once for the three sums per row, once to write the gradient.  The fixed-order block_sum of the other per-sample kernels, nothing
// shared between workgroups: bit-identical from run to run.
#include <cmath>
#include "common.h"
#include "../../include/ddpo_dpo.h"

extern "C" int ddpo_dpo_abi_version(void) { return 1; }

namespace {

__global__ void __launch_bounds__(1024) dpo_pair_fwd_bwd_kernel(const float* __restrict__ eps_c, const float* __restrict__ eps_u,
                                                               const float* __restrict__ ref_c, const float* __restrict__ ref_u,
                                                               const float* __restrict__ target, const float* __restrict__ pref, float g,
                                                               float beta, int train_cfg, float* __restrict__ d_eps_c,
                                                               float* __restrict__ d_eps_u, float* __restrict__ per_row,
                                                               float* __restrict__ per_pair, int B, int chw) {
  __shared__ float red[16];
  const int p = blockIdx.x;
  float m[2], D[2];                                // per row: the policy's error, and that minus the reference's
#pragma unroll
  for (int row = 0; row < 2; ++row) {
    const int64_t base = (int64_t)(2 * p + row) * chw;
    float acc_aa = 0.f, acc_ad = 0.f, acc_dd = 0.f;
    for (int i = threadIdx.x * 4; i < chw; i += blockDim.x * 4) {
      const float4 ec = *reinterpret_cast<const float4*>(eps_c + base + i);
      const float4 rc = *reinterpret_cast<const float4*>(ref_c + base + i);
      float4 eu = ec, ru = rc;
      if (train_cfg) {
        eu = *reinterpret_cast<const float4*>(eps_u + base + i);
        ru = *reinterpret_cast<const float4*>(ref_u + base + i);
      }
      const float4 tg = *reinterpret_cast<const float4*>(target + base + i);
      const float* pec = &ec.x; const float* prc = &rc.x; const float* peu = &eu.x; const float* pru = &ru.x; const float* pt = &tg.x;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float dlc = pec[j] - prc[j];
        const float dlu = peu[j] - pru[j];
        const float dl = train_cfg ? (dlu + g * (dlc - dlu)) : dlc;
        const float e = train_cfg ? (peu[j] + g * (pec[j] - peu[j])) : pec[j];
        const float a = pt[j] - e;
        acc_aa += a * a;
        acc_ad += a * dl;
        acc_dd += dl * dl;
      }
    }
    const float s_aa = block_sum(acc_aa, red);
    const float s_ad = block_sum(acc_ad, red);
    const float s_dd = block_sum(acc_dd, red);
    m[row] = s_aa / (float)chw;
    D[row] = -(2.0f * s_ad + s_dd) / (float)chw;
  }
  // every thread holds both D: the pair's scalars are formed redundantly, from the same floats in the same order
  const float y = (pref[2 * p] - pref[2 * p + 1]) * 0.5f;
  const float s = (y == 0.0f) ? 0.0f : (-0.5f * beta) * y * (D[0] - D[1]);   // a tie: +0.0, whichever row comes first
  const float loss = fabsf(y) * (fmaxf(-s, 0.0f) + log1pf(expf(-fabsf(s))));
  float q;
  if (s >= 0.0f) { const float t = expf(-s); q = t / (1.0f + t); }
  else q = 1.0f / (1.0f + expf(s));
  if (threadIdx.x == 0) {
    per_row[(2 * p) * 2 + 0] = m[0];
    per_row[(2 * p) * 2 + 1] = D[0];
    per_row[(2 * p + 1) * 2 + 0] = m[1];
    per_row[(2 * p + 1) * 2 + 1] = D[1];
    per_pair[p * 3 + 0] = s;
    per_pair[p * 3 + 1] = (y == 0.0f) ? 0.0f : loss;
    per_pair[p * 3 + 2] = q;
  }
  const float c_even = ((0.5f * beta) * y * q / (float)(B / 2)) * (-2.0f / (float)chw);   // d loss / d e_2p = c_even a; the odd row's is its negative
#pragma unroll
  for (int row = 0; row < 2; ++row) {
    const int64_t base = (int64_t)(2 * p + row) * chw;
    if (y == 0.0f) {                                // a tie: +0.0, whatever the signs of the factors
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int i = threadIdx.x * 4; i < chw; i += blockDim.x * 4) {
        *reinterpret_cast<float4*>(d_eps_c + base + i) = z;
        if (train_cfg) *reinterpret_cast<float4*>(d_eps_u + base + i) = z;
      }
      continue;
    }
    const float coef = row == 0 ? c_even : -c_even;
    for (int i = threadIdx.x * 4; i < chw; i += blockDim.x * 4) {
      const float4 ec = *reinterpret_cast<const float4*>(eps_c + base + i);
      float4 eu = ec;
      if (train_cfg) eu = *reinterpret_cast<const float4*>(eps_u + base + i);
      const float4 tg = *reinterpret_cast<const float4*>(target + base + i);
      const float* pec = &ec.x; const float* peu = &eu.x; const float* pt = &tg.x;
      float4 dc, du;
      float* pdc = &dc.x; float* pdu = &du.x;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float e = train_cfg ? (peu[j] + g * (pec[j] - peu[j])) : pec[j];
        const float de = coef * (pt[j] - e);
        pdc[j] = train_cfg ? g * de : de;
        pdu[j] = (1.0f - g) * de;
      }
      *reinterpret_cast<float4*>(d_eps_c + base + i) = dc;
      if (train_cfg) *reinterpret_cast<float4*>(d_eps_u + base + i) = du;
    }
  }
}

// one wave, shaped like pref_info_kernel: info = {loss, implicit_acc, margin, mse, ref_mse} over the n = B / 2 pairs of the call
__global__ void __launch_bounds__(64) dpo_info_kernel(const float* __restrict__ per_row, const float* __restrict__ per_pair,
                                                     const float* __restrict__ pref, float* __restrict__ info, int B) {
  const int n = B / 2;
  float ls = 0.f, acc = 0.f, mg = 0.f, ms = 0.f, rs = 0.f;
  for (int p = threadIdx.x; p < n; p += 64) {
    const float y = (pref[2 * p] - pref[2 * p + 1]) * 0.5f;
    const float m0 = per_row[4 * p + 0], D0 = per_row[4 * p + 1], m1 = per_row[4 * p + 2], D1 = per_row[4 * p + 3];
    const float mrg = -y * (D0 - D1);
    ls += per_pair[p * 3 + 1];
    acc += (y != 0.0f && mrg > 0.0f) ? 1.0f : 0.0f;
    mg += mrg;
    ms += m0 + m1;
    rs += (m0 - D0) + (m1 - D1);
  }
  ls = wave_sum(ls); acc = wave_sum(acc); mg = wave_sum(mg); ms = wave_sum(ms); rs = wave_sum(rs);
  if (threadIdx.x == 0) {
    info[0] = ls / (float)n;
    info[1] = acc / (float)n;
    info[2] = mg / (float)n;
    info[3] = ms / (float)B;
    info[4] = rs / (float)B;
  }
}

inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace

extern "C" int ddpo_dpo_pair_fwd_bwd(const float* eps_c, const float* eps_u, const float* ref_c, const float* ref_u, const float* target,
                                     const float* pref, float guidance_scale, float beta, int train_cfg, float* d_eps_c, float* d_eps_u,
                                     float* per_row, float* per_pair, float* info, int B, int chw, void* stream) {
  if (!eps_c || !ref_c || !target || !pref || !d_eps_c || !per_row || !per_pair || !info) return DDPO_EINVAL;
  if (train_cfg && (!eps_u || !ref_u || !d_eps_u)) return DDPO_EINVAL;
  if (B <= 0 || (B & 1) || chw <= 0 || (chw & 3)) return DDPO_EINVAL;
  if (!(beta > 0.0f) || std::isinf(beta)) return DDPO_EINVAL;                 // zero, negative, NaN or infinite
  if (misaligned(eps_c) || misaligned(ref_c) || misaligned(target) || misaligned(d_eps_c)) return DDPO_EINVAL;
  if (train_cfg && (misaligned(eps_u) || misaligned(ref_u) || misaligned(d_eps_u))) return DDPO_EINVAL;
  hipLaunchKernelGGL(dpo_pair_fwd_bwd_kernel, dim3(B / 2), dim3(1024), 0, as_stream(stream), eps_c, eps_u, ref_c, ref_u, target, pref,
                     guidance_scale, beta, train_cfg, d_eps_c, d_eps_u, per_row, per_pair, B, chw);
  DDPO_LAUNCH_CHECK();
  hipLaunchKernelGGL(dpo_info_kernel, dim3(1), dim3(64), 0, as_stream(stream), per_row, per_pair, pref, info, B);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}
