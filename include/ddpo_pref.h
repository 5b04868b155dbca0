/* ddpo_pref.h — C ABI of the preference-pair loss against the frozen pretrained policy (`--pg_loss d3po`) of libddpo_hip.so (gfx950),
 * versioned on its own beside ddpo_hip.h like ddpo_ppo_kl.h.
 *
 * D3PO (Yang et al., "Using Human Feedback to Fine-tune Diffusion Models without Any Reward Model"): two trajectories of one prompt are
 * ranked and a DPO loss is applied per denoising step on the policy-to-pretrained log-ratio of each stored transition.  Rows come in
 * adjacent pairs (2p, 2p+1); every row b has its own timestep.  With k = ddim_coef(c, ts[b]), c_t = d mu / d e and sigma = k.std_c as in
 * ddpo_ppo_kl.h (preference pairs):
 *   e      = eps_u + g (eps_c - eps_u)                                                     (train_cfg == 0: e = eps_c)
 *   delta  = delta_u + g (delta_c - delta_u), delta_c = eps_c - ref_c, delta_u = eps_u - ref_u   (differences per branch first)
 *   r      = x_next - ddim_mean(k, pred_type, e, x)
 *   h_b    = logp_theta(b) - logp_ref(b) = (2 c_t sum r delta + c_t^2 sum delta^2) / (2 sigma^2 chw)    (exactly 0 where delta == 0)
 *   y_p    = (pref[2p] - pref[2p+1]) / 2                                                   (pref rows: +1 winner, -1 loser, 0 tie)
 *   s_p    = beta y_p (h_2p - h_2p+1)
 *   loss_p = |y_p| softplus(-s_p) = |y_p| (max(-s_p, 0) + log1pf(expf(-|s_p|)))
 *   q_p    = sigmoid(-s_p) = s_p >= 0 ? t / (1 + t), t = expf(-s_p) : 1 / (1 + expf(s_p))
 *   loss_j = (1/n) sum_{p in micro-batch j} loss_p,  n = group / 2
 *   d loss_j / d h_2p = -beta y_p q_p / n,  d loss_j / d h_2p+1 = +beta y_p q_p / n
 *   d h_b / d e = c_t r / (sigma^2 chw);  d_eps_c = g * that (train_cfg == 0: 1 * that), d_eps_u = (1 - g) * that
 * The log-prob is the mean over chw of the stored log-prob, as in the D3PO authors' code.
 * Conventions as in ddpo_hip.h: device pointers, `stream` is a hipStream_t passed as void*, no allocation, no synchronisation; 0 on success,
 * DDPO_EINVAL (-1) for a bad argument before anything is launched, DDPO_ELAUNCH (-2) for a rejected launch.
 */
#ifndef DDPO_PREF_H
#define DDPO_PREF_H
#include <stddef.h>
#include <stdint.h>
#include "ddpo_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

int ddpo_pref_abi_version(void);                /* 1 */

/* Stands in the place of ddpo_ddim_logprob_ppo_fwd_bwd: it WRITES d_eps_c / d_eps_u, it does not add.  Two launches: (1) one workgroup of
 * 1024 threads per pair: per_pair (B/2, 4) = {h_even, h_odd, s_p, loss_p} and the gradient above into the two rows of d_eps_c (and d_eps_u
 * under train_cfg); (2) one wave per micro-batch of `group` consecutive rows: info (B/group, 3) = {pref_acc, pref_margin, loss} with
 * pref_margin = (1/n) sum y_p (h_even - h_odd) and pref_acc = (1/n) #{p : y_p != 0 and y_p (h_even - h_odd) > 0}.  The loss sits in
 * column 2, where ddpo_ddim_kl_ref_fwd_bwd (ddpo_ppo_kl.h) launched behind this call adds its penalty.  A pair with y_p == 0 writes loss 0
 * and +0.0 gradients.  Fixed-order reductions, no atomics, nothing shared between workgroups: bit-identical from run to run, and pair for
 * pair what B/group separate calls give.
 * eps_u / ref_u / d_eps_u may be NULL unless train_cfg.  All float pointers of (B, chw) arrays 16-byte aligned.
 * DDPO_EINVAL: a NULL pointer, B <= 0, B odd, group <= 0, group odd, B % group, chw <= 0, chw & 3, beta not finite or <= 0,
 * c->pred_type == DDPO_PRED_SAMPLE (only epsilon and v models are trained here), a misaligned (B, chw) pointer. */
int ddpo_ddim_pref_fwd_bwd(const float* eps_c, const float* eps_u, const float* ref_c, const float* ref_u,
                           const float* x, const float* x_next, const int32_t* ts, const float* pref,
                           float guidance_scale, float beta, int train_cfg, const ddpo_ddim_consts* c,
                           float* d_eps_c, float* d_eps_u, float* per_pair, float* info,
                           int B, int group, int chw, void* stream);

#ifdef __cplusplus
}
#endif
#endif
