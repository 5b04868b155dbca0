/* ddpo_cfg_rescale.h — C ABI of what v-prediction checkpoints (SD-2.1 768) need beyond ddpo_hip.h, of libddpo_hip.so (gfx950), versioned on
 * its own beside ddpo_hip.h like ddpo_dpo.h: the rescaled classifier-free guidance of `--guidance_rescale` (forward and backward) and the
 * noising pass of the offline entry points with the regression target of the model's prediction type.
 *
 * Rescaled guidance (Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed", §3.4; diffusers' `guidance_rescale`).
 * Per row b, every statistic over the row's n = chw elements, t = eps_c, u = eps_u, g = guidance_scale, phi = guidance_rescale:
 *   c     = u + g (t - u)                                   the plain combine, the expression of ddpo_ddim_step_fwd
 *   s_t   = std(t), s_c = std(c)                            unbiased (n - 1), centred: the mean first, then the squared deviations
 *   k     = (1 - phi) + phi (s_t / s_c)
 *   out   = k c
 * and, with G = dL/d out, S = sum_j G_j c_j:
 *   dL/dc_i = k G_i - S phi (s_t / s_c) (c_i - mean c) / ((n - 1) s_c^2)
 *   dL/dt_i = g dL/dc_i + S phi (t_i - mean t) / ((n - 1) s_t s_c)
 *   dL/du_i = (1 - g) dL/dc_i
 * A row whose guided prediction is constant has s_c == 0: k, out and the gradients are inf / NaN exactly as the formula gives them (a row
 * with s_t == 0 too has NaN gradients).  Nothing is special-cased, as ddpo_cosine_rows does not special-case a zero row.
 * Conventions as in ddpo_hip.h: device pointers, `stream` is a hipStream_t passed as void*, no allocation, no synchronisation; 0 on success,
 * DDPO_EINVAL (-1) for a bad argument before anything is launched, DDPO_ELAUNCH (-2) for a rejected launch.
 */
#ifndef DDPO_CFG_RESCALE_H
#define DDPO_CFG_RESCALE_H
#include <stddef.h>
#include <stdint.h>
#include "ddpo_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

int ddpo_cfg_rescale_abi_version(void);         /* 1 */

/* eps_c / eps_u / out: (B, chw); stats: (B, 4) = {mean t, s_t, mean c, s_c}.  One launch, one workgroup of 1024 threads per row, three
 * passes over the row (sums, squared deviations, write).  Fixed-order reductions, no atomics, nothing shared between workgroups: the result
 * is bit-identical from run to run, and row for row what B calls on one row give.  `out` may not alias an input.
 * DDPO_EINVAL: a NULL pointer, B <= 0, chw <= 0, chw & 3, chw < 8, an (B, chw) pointer that is not 16-byte aligned, guidance_rescale not
 * finite or outside [0, 1]. */
int ddpo_cfg_rescale_fwd(const float* eps_c, const float* eps_u, float guidance_scale, float guidance_rescale, float* out, float* stats,
                         int B, int chw, void* stream);

/* d_out: (B, chw) = dL/d out; stats: what the forward wrote for the same eps_c / eps_u / guidance_scale / guidance_rescale.  It WRITES
 * d_eps_c / d_eps_u (every element of both), it does not add.  One launch, one workgroup per row: one reduction for S, then the write pass.
 * Reproducible as the forward is.  DDPO_EINVAL: as for the forward. */
int ddpo_cfg_rescale_bwd(const float* eps_c, const float* eps_u, const float* d_out, const float* stats, float guidance_scale,
                         float guidance_rescale, float* d_eps_c, float* d_eps_u, int B, int chw, void* stream);

/* ddpo_rwr_noisy_latents (ddpo_hip.h) with the regression target of the model's prediction type: `latents` and `noisy` by the same
 * expressions (bit-equal to that entry's, same clamp of ts to [0, num_train_timesteps)), and target (B, C, h, w) NCHW =
 *   DDPO_PRED_EPSILON: noise;  DDPO_PRED_V: sqrt(acp[t]) noise - sqrt(1 - acp[t]) latents;  DDPO_PRED_SAMPLE: latents.
 * DDPO_EINVAL: a NULL pointer, B / C / hw / num_train_timesteps <= 0, pred_type none of the three. */
int ddpo_rwr_noisy_latents_target(const float* moments, const float* e1, const float* noise, const int32_t* ts,
                                  const float* alphas_cumprod, int num_train_timesteps, float scale, int pred_type, float* latents,
                                  float* noisy, float* target, int B, int C, int hw, void* stream);

#ifdef __cplusplus
}
#endif
#endif
