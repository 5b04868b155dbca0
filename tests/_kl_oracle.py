"""Oracle (test infrastructure only) of the `--kl_coef` penalty: the KL of the policy's DDIM step to the frozen pretrained policy's, restated
in torch (differentiable, any float dtype — float64 is the ground truth) on top of oracle.unet.unet_forward and oracle.ppo.loss_and_info_torch,
and the fp32 numpy closed form the HIP pass implements (include/ddpo_ppo_kl.h).

Both policies are N(mu, sigma_c^2 I) with the sigma_c of the stored log-prob, and mu is affine in the model output e with slope c_t = d mu / d e:
    kl_b = c_t^2 / (2 sigma_c^2) * mean_chw delta^2,   delta = delta_u + g (delta_c - delta_u),  delta_c = e_c - r_c,  delta_u = e_u - r_u
(the KL of the two diagonal Gaussians divided by chw, the normalisation of the log-prob), and
    d (kl_coef * mean_{b in micro-batch} kl_b) / d e = (kl_coef / group) * c_t^2 / (sigma_c^2 chw) * delta,   d/d e_c = g * that,  d/d e_u = (1 - g) * that.
"""
import numpy as np
import torch

from oracle import ppo as OPPO, unet as OU


def coefficients(ddim, state, ts, eta, dtype=torch.float64):
    """(a_t, a_p, b_t, std, std_c, c_t) as (B, 1, 1, 1) tensors: the oracle's own coefficients (oracle.ppo._coeff_tensors) and the slope of its mean."""
    a_t, a_p, b_t, std = OPPO._coeff_tensors(ddim, state, ts, eta, dtype)
    dirc = (1 - a_p - std ** 2) ** 0.5
    if ddim.prediction_type == "epsilon":
        c_t = dirc - a_p ** 0.5 * b_t ** 0.5 / a_t ** 0.5
    elif ddim.prediction_type == "v_prediction":
        c_t = dirc * a_t ** 0.5 - a_p ** 0.5 * b_t ** 0.5
    else:
        raise ValueError("the KL penalty is defined for epsilon and v models only")
    return a_t, a_p, b_t, std, torch.clamp(std, min=1e-6), c_t


def ddim_mean_torch(ddim, state, model_output, ts, sample, eta, dtype=torch.float64):
    """The mean of oracle.ppo.log_prob_torch (scheduling_ddim_flax.py:279-327), line for line, in `dtype`."""
    a_t, a_p, b_t, std = OPPO._coeff_tensors(ddim, state, ts, eta, dtype)
    sample = sample.to(dtype)
    e = model_output.to(dtype)
    if ddim.prediction_type == "epsilon":
        x0 = (sample - b_t ** 0.5 * e) / a_t ** 0.5
    elif ddim.prediction_type == "v_prediction":
        x0 = a_t ** 0.5 * sample - b_t ** 0.5 * e
        e = a_t ** 0.5 * e + b_t ** 0.5 * sample
    else:
        raise ValueError
    return a_p ** 0.5 * x0 + (1 - a_p - std ** 2) ** 0.5 * e


def guided(e_c, e_u, guidance_scale, train_cfg):
    return e_u + guidance_scale * (e_c - e_u) if train_cfg else e_c


def kl_rows_torch(ddim, state, eps_c, eps_u, ref_c, ref_u, ts, guidance_scale, eta, train_cfg=True, dtype=torch.float64):
    """kl_b (B,), differentiable in eps_c / eps_u.  Differences per branch first: exactly 0 where the two networks agree."""
    *_, std_c, c_t = coefficients(ddim, state, ts, eta, dtype)
    d_c = eps_c.to(dtype) - ref_c.to(dtype)
    delta = d_c
    if train_cfg:
        d_u = eps_u.to(dtype) - ref_u.to(dtype)
        delta = d_u + guidance_scale * (d_c - d_u)
    B = delta.shape[0]
    return (c_t ** 2 / (2 * std_c ** 2)).reshape(B) * (delta ** 2).flatten(1).mean(1)


def kl_rows_by_distributions(ddim, state, eps_c, eps_u, ref_c, ref_u, ts, sample, guidance_scale, eta, train_cfg=True, dtype=torch.float64):
    """The same number the long way round: torch.distributions' KL of the two Gaussians around the oracle's DDIM means, mean over chw."""
    *_, std_c, _ = coefficients(ddim, state, ts, eta, dtype)
    mu = ddim_mean_torch(ddim, state, guided(eps_c.to(dtype), None if eps_u is None else eps_u.to(dtype), guidance_scale, train_cfg), ts, sample, eta, dtype)
    mu_ref = ddim_mean_torch(ddim, state, guided(ref_c.to(dtype), None if ref_u is None else ref_u.to(dtype), guidance_scale, train_cfg), ts, sample, eta, dtype)
    sig = std_c.expand_as(mu)
    kl = torch.distributions.kl_divergence(torch.distributions.Normal(mu, sig), torch.distributions.Normal(mu_ref, sig))
    return kl.flatten(1).mean(1)


def kl_grad_closed_form(ddim, state, eps_c, eps_u, ref_c, ref_u, ts, guidance_scale, eta, kl_coef, group, train_cfg=True, dtype=torch.float64):
    """(d_eps_c, d_eps_u | None) of sum_j kl_coef * mean_{b in micro-batch j} kl_b, by the formula of the module docstring."""
    *_, std_c, c_t = coefficients(ddim, state, ts, eta, dtype)
    d_c = eps_c.to(dtype) - ref_c.to(dtype)
    delta = d_c
    if train_cfg:
        d_u = eps_u.to(dtype) - ref_u.to(dtype)
        delta = d_u + guidance_scale * (d_c - d_u)
    chw = delta[0].numel()
    de = (kl_coef / group) * c_t ** 2 / (std_c ** 2 * chw) * delta
    return (guidance_scale * de, (1 - guidance_scale) * de) if train_cfg else (de, None)


def loss_and_info_torch(ddim, state, eps_c, eps_u, ref_c, ref_u, batch, guidance_scale, eta, clip_range, kl_coef, train_cfg=True,
                        dtype=torch.float64):
    """oracle.ppo.loss_and_info_torch plus kl_coef * mean_b kl_b.  Returns (loss, info with "kl_ref" and the penalised "loss", log_prob, kl_b,
    ppo_loss): one micro-batch."""
    ppo_loss, info, log_prob = OPPO.loss_and_info_torch(ddim, state, eps_c, eps_u, batch, guidance_scale, eta, clip_range, train_cfg, dtype)
    kl_b = kl_rows_torch(ddim, state, eps_c, eps_u, ref_c, ref_u, batch["ts"], guidance_scale, eta, train_cfg, dtype)
    kl = kl_b.mean()
    loss = ppo_loss + kl_coef * kl
    return loss, dict(info, loss=loss, kl_ref=kl), log_prob, kl_b, ppo_loss


def train_step_grads(params, ref_params, cfg, ddim, state, batch, guidance_scale, eta, clip_range, kl_coef, train_cfg=True, dtype=torch.float64):
    """oracle.sampler.train_step_grads with the penalty: autograd of ppo + kl_coef * kl through oracle.unet.unet_forward, the reference network
    evaluated without a graph.  Returns ({name: grad}, info floats, {name: grad of the PPO part}, {name: grad of the KL part})."""
    leaves = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in params.items()}
    frozen = {k: v.detach().to(dtype) for k, v in ref_params.items()}
    lat, ts = batch["latents"].to(dtype), batch["ts"]
    emb, unc = batch["prompt_embeds"].to(dtype), batch["uncond_embeds"].to(dtype)
    eps_c = OU.unet_forward(leaves, cfg, lat, ts, emb)
    eps_u = OU.unet_forward(leaves, cfg, lat, ts, unc) if train_cfg else None
    with torch.no_grad():
        ref_c = OU.unet_forward(frozen, cfg, lat, ts, emb)
        ref_u = OU.unet_forward(frozen, cfg, lat, ts, unc) if train_cfg else None
    loss, info, _, _, ppo_loss = loss_and_info_torch(ddim, state, eps_c, eps_u, ref_c, ref_u, batch, guidance_scale, eta, clip_range, kl_coef,
                                                     train_cfg, dtype)
    names = list(leaves)
    zero = lambda g, n: torch.zeros_like(leaves[n]) if g is None else g
    g_ppo = torch.autograd.grad(ppo_loss, [leaves[n] for n in names], retain_graph=True, allow_unused=True)
    g_kl = torch.autograd.grad(loss - ppo_loss, [leaves[n] for n in names], allow_unused=True)
    g_ppo = {n: zero(g, n) for n, g in zip(names, g_ppo)}
    g_kl = {n: zero(g, n) for n, g in zip(names, g_kl)}
    return {n: g_ppo[n] + g_kl[n] for n in names}, {k: float(v.detach()) for k, v in info.items()}, g_ppo, g_kl


def closed_form_numpy(ddim, state, eps_c, eps_u, ref_c, ref_u, ts, guidance_scale, eta, kl_coef, group, train_cfg=True):
    """The algebra of the HIP pass in fp32 numpy, for `B // group` micro-batches at once: (kl_b (B,), kl_info (B // group,), inc_c, inc_u | None),
    inc_* the increments the pass adds to the PPO gradient."""
    F = np.float32
    B = eps_c.shape[0]
    chw = int(np.prod(eps_c.shape[1:]))
    a_t, a_p, b_t, std = ddim.coefficients(state, np.asarray(ts), eta)
    sq = lambda v: np.sqrt(v).astype(F)
    dirc = sq(F(1) - a_p - std ** 2)
    if ddim.prediction_type == "epsilon":
        c_t = dirc - sq(a_p) * sq(b_t) / sq(a_t)
    elif ddim.prediction_type == "v_prediction":
        c_t = dirc * sq(a_t) - sq(a_p) * sq(b_t)
    else:
        raise ValueError
    std_c = np.maximum(std, F(1e-6))
    w = ((c_t * c_t) / (std_c * std_c)).astype(F)
    g = F(guidance_scale)
    d_c = (eps_c - ref_c).astype(F)
    delta = d_c
    if train_cfg:
        d_u = (eps_u - ref_u).astype(F)
        delta = (d_u + g * (d_c - d_u)).astype(F)
    kl_b = ((F(0.5) * w) * ((delta * delta).reshape(B, -1).sum(1, dtype=F) / F(chw))).astype(F)
    kl_info = (kl_b.reshape(B // group, group).sum(1, dtype=F) / F(group)).astype(F)
    gcoef = ((F(kl_coef) / F(group)) * (w / F(chw))).astype(F).reshape(B, *([1] * (eps_c.ndim - 1)))
    de = (gcoef * delta).astype(F)
    return kl_b, kl_info, ((g * de).astype(F) if train_cfg else de), (((F(1) - g) * de).astype(F) if train_cfg else None)
