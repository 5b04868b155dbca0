/* ddpo_ppo_kl.h — C ABI of the KL penalty to the frozen pretrained policy (`--kl_coef`) of libddpo_hip.so (gfx950), versioned on its own
 * beside ddpo_hip.h like ddpo_optim.h.
 *
 * The policy at one DDIM step is N(mu_theta, sigma_c^2 I) with a variance that does not depend on the parameters, so the KL to the
 * pretrained policy N(mu_ref, sigma_c^2 I) at the same (x_t, t, context) is |mu_theta - mu_ref|^2 / (2 sigma_c^2), and mu is affine in the
 * model output: mu_theta - mu_ref = c_t (e - r), c_t = d mu / d e.  Per sample-timestep row b (KL penalty):
 *   delta = delta_u + g (delta_c - delta_u), delta_c = eps_c - ref_c, delta_u = eps_u - ref_u     (train_cfg == 0: delta = eps_c - ref_c)
 *   kl_b  = c_t^2 / (2 sigma_c^2) * mean_chw delta^2        (the KL divided by chw: the normalisation of the stored log-prob)
 *   d (kl_coef * mean_{b in micro-batch} kl_b) / d e = (kl_coef / group) * c_t^2 / (sigma_c^2 * chw) * delta
 * The differences are formed per branch, so delta is exactly 0 where the two networks agree.
 * Conventions as in ddpo_hip.h: device pointers, `stream` is a hipStream_t passed as void*, no allocation, no synchronisation; 0 on success,
 * DDPO_EINVAL (-1) for a bad argument before anything is launched, DDPO_ELAUNCH (-2) for a rejected launch.
 */
#ifndef DDPO_PPO_KL_H
#define DDPO_PPO_KL_H
#include <stddef.h>
#include <stdint.h>
#include "ddpo_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

int ddpo_ppo_kl_abi_version(void);              /* 1 */

/* Additive pass behind ddpo_ddim_logprob_ppo_fwd_bwd on the same stream, which it leaves untouched (the log-prob stays the sampler's bits).
 * Two launches: (1) one workgroup of 1024 threads per row: kl_per_sample[b] = kl_b, and the gradient above ADDED into d_eps_c (times g
 * under train_cfg) and d_eps_u (times 1 - g; train_cfg only) — the buffers the PPO launch wrote; (2) one wave per micro-batch of `group`
 * consecutive rows: kl_info[j] = mean of its kl_b, and, if loss_info is given (the PPO launch's (B/group, 3) info), column 2 of row j
 * += kl_coef * kl_info[j].  Fixed-order reductions, no atomics, nothing shared between workgroups: bit-identical from run to run, and row
 * for row what B/group separate calls give.  An increment that is exactly zero leaves its word as it is.
 * eps_u / ref_u / d_eps_u may be NULL unless train_cfg.  All float pointers of (B, chw) arrays 16-byte aligned.
 * DDPO_EINVAL: a NULL pointer (loss_info excepted), B <= 0, group <= 0, B % group, chw <= 0, chw & 3, kl_coef negative or not finite,
 * c->pred_type == DDPO_PRED_SAMPLE (only epsilon and v models are trained here). */
int ddpo_ddim_kl_ref_fwd_bwd(const float* eps_c, const float* eps_u, const float* ref_c, const float* ref_u, const int32_t* ts,
                             float guidance_scale, float kl_coef, int train_cfg, const ddpo_ddim_consts* c, float* d_eps_c,
                             float* d_eps_u, float* kl_per_sample, float* kl_info, float* loss_info, int B, int group, int chw,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif
