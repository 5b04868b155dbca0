/* ddpo_dpo.h — C ABI of the Diffusion-DPO loss on ranked pairs of stored samples (`pipeline/dpo.py`) of libddpo_hip.so (gfx950), versioned
 * on its own beside ddpo_hip.h like ddpo_pref.h.
 *
 * Diffusion-DPO (Wallace et al., "Diffusion Model Alignment Using Direct Preference Optimization"): two samples of one prompt are ranked
 * and the policy is trained so that its denoising error drops faster on the winner than on the loser, relative to the frozen pretrained
 * model.  Rows come in adjacent pairs (2p, 2p+1), as in ddpo_pref.h.  Per row b, with `target` the regression target (the DDPM noise for
 * an epsilon model, v for a v-prediction model: ddpo_rwr_noisy_latents_target) and g the guidance scale (Diffusion-DPO):
 *   e       = eps_u + g (eps_c - eps_u)                                                     (train_cfg == 0: e = eps_c)
 *   delta   = delta_u + g (delta_c - delta_u), delta_c = eps_c - ref_c, delta_u = eps_u - ref_u   (differences per branch first)
 *   a       = target - e
 *   m_b     = (1/chw) sum a^2                                                               the policy's error
 *   D_b     = m_b - r_b = -(2 sum a delta + sum delta^2) / chw       the policy's error minus the reference's (== 0.0 where delta == 0)
 *   y_p     = (pref[2p] - pref[2p+1]) / 2                                                   (pref rows: +1 winner, -1 loser, 0 tie)
 *   s_p     = -0.5 beta y_p (D_2p - D_2p+1)
 *   loss_p  = |y_p| softplus(-s_p) = |y_p| (max(-s_p, 0) + log1pf(expf(-|s_p|)))
 *   q_p     = sigmoid(-s_p) = s_p >= 0 ? t / (1 + t), t = expf(-s_p) : 1 / (1 + expf(s_p))
 *   loss    = (1/n) sum_p loss_p,  n = B / 2                                                (ties count in n)
 *   d loss / d e_2p = (0.5 beta y_p q_p / n) (-2 / chw) a;  row 2p+1: the negative coefficient, its own a
 *   d_eps_c = g * that (train_cfg == 0: 1 * that), d_eps_u = (1 - g) * that
 * Conventions as in ddpo_hip.h: device pointers, `stream` is a hipStream_t passed as void*, no allocation, no synchronisation; 0 on success,
 * DDPO_EINVAL (-1) for a bad argument before anything is launched, DDPO_ELAUNCH (-2) for a rejected launch.
 */
#ifndef DDPO_DPO_H
#define DDPO_DPO_H
#include <stddef.h>
#include <stdint.h>
#include "ddpo_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

int ddpo_dpo_abi_version(void);                 /* 1 */

/* Stands in the place of ddpo_rwr_mse_fwd_bwd: it WRITES d_eps_c / d_eps_u, it does not add.  Two launches: (1) one workgroup of 1024
 * threads per pair: per_row (B, 2) = {m_b, D_b}, per_pair (B/2, 3) = {s_p, loss_p, q_p} and the gradient above into the two rows of
 * d_eps_c (and d_eps_u under train_cfg); (2) one wave: info (5) = {loss, implicit_acc, margin, mse, ref_mse} with
 * margin = (1/n) sum -y_p (D_2p - D_2p+1), implicit_acc = (1/n) #{p : y_p != 0 and -y_p (D_2p - D_2p+1) > 0}, mse = (1/B) sum m_b and
 * ref_mse = (1/B) sum (m_b - D_b).  A pair with y_p == 0 writes loss 0 and +0.0 gradients.  Fixed-order reductions, no atomics, nothing
 * shared between workgroups: bit-identical from run to run, and per_row / per_pair are pair for pair what separate calls give.
 * eps_u / ref_u / d_eps_u may be NULL unless train_cfg.  All float pointers of (B, chw) arrays 16-byte aligned.
 * DDPO_EINVAL: a NULL pointer, B <= 0, B odd, chw <= 0, chw & 3, beta not finite or <= 0, a misaligned (B, chw) pointer. */
int ddpo_dpo_pair_fwd_bwd(const float* eps_c, const float* eps_u, const float* ref_c, const float* ref_u, const float* target,
                          const float* pref, float guidance_scale, float beta, int train_cfg,
                          float* d_eps_c, float* d_eps_u, float* per_row, float* per_pair, float* info,
                          int B, int chw, void* stream);

#ifdef __cplusplus
}
#endif
#endif
