"""Oracle (test infrastructure only) of `pipeline/dpo.py`: the Diffusion-DPO loss on ranked pairs of stored samples (Wallace et al.,
"Diffusion Model Alignment Using Direct Preference Optimization"), in the authors' form in torch (differentiable, any float dtype — float64
is the ground truth): the mean squared error of the policy and of the reference per row, their differences winner minus loser, and
-logsigmoid(-0.5 beta (model_diff - ref_diff)); and the fp32 numpy closed form the HIP pass implements (include/ddpo_dpo.h).

Rows come in adjacent pairs (2p, 2p+1):
    m_b = mean_chw (target - e)^2,  r_b = mean_chw (target - e_ref)^2,  D_b = m_b - r_b
    y_p = (pref[2p] - pref[2p+1]) / 2,  s_p = -0.5 beta y_p (D_2p - D_2p+1),  loss_p = |y_p| softplus(-s_p),  q_p = sigmoid(-s_p)
    loss = mean_p loss_p;  margin = mean_p -y_p (D_2p - D_2p+1);  implicit_acc = share of pairs with y_p != 0 and -y_p (D_2p - D_2p+1) > 0;
    mse = mean_b m_b;  ref_mse = mean_b r_b.
The closed form: D_b = -(2 sum a delta + sum delta^2) / chw with a = target - e and delta = e - e_ref (guided, the differences per branch
first), d loss / d e_2p = (0.5 beta y_p q_p / n) (-2 / chw) a.
"""
import numpy as np
import torch

from oracle import prng, unet as OU
from oracle.diffusion import SCALING

INFO_KEYS = ("loss", "implicit_acc", "margin", "mse", "ref_mse")


def guided(c, u, guidance_scale, train_cfg):
    return (u + guidance_scale * (c - u)) if train_cfg else c


def errors_rows_torch(eps_c, eps_u, ref_c, ref_u, target, guidance_scale, train_cfg=True, dtype=torch.float64):
    """(m (B,), r (B,)): the two mean squared errors per row, m differentiable in eps_c / eps_u."""
    t = lambda v: None if v is None else v.to(dtype)
    e = guided(t(eps_c), t(eps_u), guidance_scale, train_cfg)
    er = guided(t(ref_c), t(ref_u), guidance_scale, train_cfg)
    tg = target.to(dtype)
    return ((tg - e) ** 2).flatten(1).mean(1), ((tg - er) ** 2).flatten(1).mean(1)


def loss_and_info_torch(eps_c, eps_u, ref_c, ref_u, target, pref, guidance_scale, beta, train_cfg=True, dtype=torch.float64):
    """The authors' form.  Returns (loss, info {INFO_KEYS}, m (B,), D (B,), s (B/2,), loss_p (B/2,))."""
    m, r = errors_rows_torch(eps_c, eps_u, ref_c, ref_u, target, guidance_scale, train_cfg, dtype)
    y = torch.as_tensor(np.asarray(pref)).to(dtype)
    y = (y[0::2] - y[1::2]) / 2
    model_diff = m[0::2] - m[1::2]
    ref_diff = r[0::2] - r[1::2]
    s = -0.5 * beta * y * (model_diff - ref_diff)
    loss_p = y.abs() * -torch.nn.functional.logsigmoid(s)
    mrg = -y * (model_diff - ref_diff)
    loss = loss_p.mean()
    info = {"loss": loss, "implicit_acc": ((y != 0) & (mrg > 0)).to(dtype).mean(), "margin": mrg.mean(), "mse": m.mean(), "ref_mse": r.mean()}
    return loss, info, m, m - r, s, loss_p


def closed_form_numpy(eps_c, eps_u, ref_c, ref_u, target, pref, guidance_scale, beta, train_cfg=True):
    """The algebra of the HIP pass in fp32 numpy: (m (B,), D (B,), s, loss_p, q (B/2,), info (5,), d_eps_c, d_eps_u | None)."""
    F = np.float32
    B = eps_c.shape[0]
    chw = int(np.prod(eps_c.shape[1:]))
    g = F(guidance_scale)
    d_c = (eps_c - ref_c).astype(F)
    delta, e = d_c, eps_c
    if train_cfg:
        d_u = (eps_u - ref_u).astype(F)
        delta = (d_u + g * (d_c - d_u)).astype(F)
        e = (eps_u + g * (eps_c - eps_u)).astype(F)
    a = (target - e).astype(F)
    s_aa = (a * a).reshape(B, -1).sum(1, dtype=F)
    s_ad = (a * delta).reshape(B, -1).sum(1, dtype=F)
    s_dd = (delta * delta).reshape(B, -1).sum(1, dtype=F)
    m = (s_aa / F(chw)).astype(F)
    D = (-(F(2) * s_ad + s_dd) / F(chw)).astype(F)
    pref = np.asarray(pref, dtype=F)
    y = ((pref[0::2] - pref[1::2]) * F(0.5)).astype(F)
    dD = (D[0::2] - D[1::2]).astype(F)
    s = np.where(y == 0, F(0), (F(-0.5) * F(beta)) * y * dD).astype(F)
    t = np.exp(-np.abs(s)).astype(F)
    loss_p = (np.abs(y) * (np.maximum(-s, F(0)) + np.log1p(t).astype(F))).astype(F)
    q = np.where(s >= 0, t / (F(1) + t), F(1) / (F(1) + t)).astype(F)
    n = B // 2
    mrg = (-y * dD).astype(F)
    info = np.asarray([loss_p.sum(dtype=F) / F(n), ((y != 0) & (mrg > 0)).astype(F).sum(dtype=F) / F(n), mrg.sum(dtype=F) / F(n),
                       m.sum(dtype=F) / F(B), (m - D).astype(F).sum(dtype=F) / F(B)], dtype=F)
    c_even = (((F(0.5) * F(beta)) * y * q / F(n)) * (F(-2) / F(chw))).astype(F)
    coef = np.stack([c_even, -c_even], 1).reshape(B, *([1] * (eps_c.ndim - 1)))
    de = (coef * a).astype(F)
    return m, D, s, loss_p, q, info, ((g * de).astype(F) if train_cfg else de), (((F(1) - g) * de).astype(F) if train_cfg else None)


def prepare_pairs(vae_moments, train_rng, alphas_cumprod):
    """oracle.diffusion.prepare with the diffusion noise and the timestep drawn per pair (B / 2 of each, both rows of a pair use them):
    -> dict(latents, noise, timesteps, noisy_latents (all NCHW float32 / int32, B rows), new_train_rng)."""
    m = np.asarray(vae_moments, dtype=np.float32)                       # (B, h, w, 2C) NHWC
    B = m.shape[0]
    dropout_rng, sample_rng, new_train_rng = prng.split(np.asarray(train_rng, dtype=np.uint32), 3)
    C = m.shape[-1] // 2
    mean, logvar = m[..., :C], np.clip(m[..., C:], np.float32(-30.0), np.float32(20.0))
    std = np.exp(np.float32(0.5) * logvar).astype(np.float32)
    lat = (mean + std * prng.normal(sample_rng, mean.shape)).astype(np.float32)
    lat = (np.transpose(lat, (0, 3, 1, 2)) * SCALING).astype(np.float32)
    noise_rng, timestep_rng = prng.split(sample_rng)
    noise = np.repeat(prng.normal(noise_rng, (B // 2,) + lat.shape[1:]), 2, axis=0)
    ts = np.repeat(prng.randint(timestep_rng, (B // 2,), 0, len(alphas_cumprod)), 2)
    acp = np.asarray(alphas_cumprod, dtype=np.float32)[ts]
    sa = (acp ** np.float32(0.5)).reshape(-1, 1, 1, 1)
    sb = ((np.float32(1.0) - acp) ** np.float32(0.5)).reshape(-1, 1, 1, 1)
    noisy = (sa * lat + sb * noise).astype(np.float32)
    return dict(latents=lat, noise=noise, timesteps=ts.astype(np.int32), noisy_latents=noisy, new_train_rng=new_train_rng)


def network_outputs(params, cfg, prep, prompt_embeds, uncond_embeds, train_cfg=True, dtype=torch.float64):
    """(eps_c, eps_u | None) of oracle.unet.unet_forward on the prepared rows; differentiable in `params` if they require grad."""
    x = torch.from_numpy(prep["noisy_latents"]).to(dtype)
    ts = torch.from_numpy(prep["timesteps"])
    eps_c = OU.unet_forward(params, cfg, x, ts, prompt_embeds.to(dtype))
    return eps_c, (OU.unet_forward(params, cfg, x, ts, uncond_embeds.to(dtype)) if train_cfg else None)


def train_step_grads(params, ref_params, cfg, prep, prompt_embeds, uncond_embeds, pref, guidance_scale, beta, train_cfg=True,
                     dtype=torch.float64):
    """Autograd of the Diffusion-DPO loss through oracle.unet.unet_forward, the reference network evaluated without a graph.
    Returns ({name: grad}, info floats, D (B,))."""
    leaves = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in params.items()}
    frozen = {k: v.detach().to(dtype) for k, v in ref_params.items()}
    eps_c, eps_u = network_outputs(leaves, cfg, prep, prompt_embeds, uncond_embeds, train_cfg, dtype)
    with torch.no_grad():
        ref_c, ref_u = network_outputs(frozen, cfg, prep, prompt_embeds, uncond_embeds, train_cfg, dtype)
    loss, info, _, D, _, _ = loss_and_info_torch(eps_c, eps_u, ref_c, ref_u, torch.from_numpy(prep["noise"]), pref, guidance_scale, beta,
                                                 train_cfg, dtype)
    names = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[n] for n in names], allow_unused=True)
    return ({n: (torch.zeros_like(leaves[n]) if g is None else g) for n, g in zip(names, grads)},
            {k: float(v.detach()) for k, v in info.items()}, D.detach())
