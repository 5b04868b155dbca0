// Per-timestep scalars of the DDIM step (scheduling_ddim_flax.py:279-359), shared by the kernels that score a transition: elementwise.hip
// (sampling step, log-prob + PPO) and ppo_kl.hip (KL penalty to the frozen reference).  One definition, so sigma_c is the same float everywhere.
#pragma once
#include "common.h"
#include <math.h>

struct DdimCoef {
  float sqrt_at, sqrt_bt, sqrt_ap, dirc, std, std_c;
};

__device__ __forceinline__ DdimCoef ddim_coef(const ddpo_ddim_consts c, int t) {
  const int p = t - c.step_ratio;
  const float a_t = c.alphas_cumprod[t];
  const float a_p = (p >= 0) ? c.alphas_cumprod[p] : c.final_alpha_cumprod;
  const float b_t = 1.0f - a_t;
  const float var = ((1.0f - a_p) / (1.0f - a_t)) * (1.0f - a_t / a_p);
  DdimCoef k;
  k.std = c.eta * sqrtf(var);
  k.sqrt_at = sqrtf(a_t);
  k.sqrt_bt = sqrtf(b_t);
  k.sqrt_ap = sqrtf(a_p);
  k.dirc = sqrtf(1.0f - a_p - k.std * k.std);
  k.std_c = fmaxf(k.std, 1e-6f);
  return k;
}
