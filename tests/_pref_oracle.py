"""Oracle (test infrastructure only) of `--pg_loss d3po`: the preference-pair loss on the policy-to-pretrained log-ratio of stored DDIM
transitions, restated in torch (differentiable, any float dtype — float64 is the ground truth) as oracle.ppo.log_prob_torch of the policy
minus that of the reference, and the fp32 numpy closed form the HIP pass implements (include/ddpo_pref.h).

Rows come in adjacent pairs (2p, 2p+1), every row with its own timestep:
    h_b    = logp_theta(b) - logp_ref(b)                                   (both the mean over chw of oracle.ppo.log_prob_torch)
    y_p    = (pref[2p] - pref[2p+1]) / 2,   s_p = beta y_p (h_2p - h_2p+1),   loss_p = |y_p| softplus(-s_p),   q_p = sigmoid(-s_p)
    loss_j = mean over the pairs of micro-batch j of loss_p;  pref_margin = mean of y_p (h_2p - h_2p+1);  pref_acc = share of pairs with
    y_p != 0 and y_p (h_2p - h_2p+1) > 0.
The closed form: h_b = (2 c_t sum r delta + c_t^2 sum delta^2) / (2 sigma^2 chw) with r = x' - mu_theta and delta = e - ref (guided, the
differences per branch first), d h_b / d e = c_t r / (sigma^2 chw).
"""
import numpy as np
import torch

from oracle import ppo as OPPO, unet as OU

import _kl_oracle as KO


def log_ratio_rows_torch(ddim, state, eps_c, eps_u, ref_c, ref_u, x, x_next, ts, guidance_scale, eta, train_cfg=True, dtype=torch.float64):
    """h_b (B,), differentiable in eps_c / eps_u: the oracle's log-prob under the policy minus its log-prob under the reference."""
    e = KO.guided(eps_c.to(dtype), None if eps_u is None else eps_u.to(dtype), guidance_scale, train_cfg)
    r = KO.guided(ref_c.to(dtype), None if ref_u is None else ref_u.to(dtype), guidance_scale, train_cfg)
    lp = OPPO.log_prob_torch(ddim, state, e, ts, x, x_next, eta, dtype)
    lp_ref = OPPO.log_prob_torch(ddim, state, r, ts, x, x_next, eta, dtype)
    return lp - lp_ref


def pair_terms_torch(h, pref, beta):
    """(y_p, s_p, loss_p, q_p) of the adjacent pairs of h / pref."""
    pref = torch.as_tensor(pref).to(h.dtype)
    y = (pref[0::2] - pref[1::2]) / 2
    s = beta * y * (h[0::2] - h[1::2])
    return y, s, y.abs() * torch.nn.functional.softplus(-s), torch.sigmoid(-s)


def loss_and_info_torch(ddim, state, eps_c, eps_u, ref_c, ref_u, batch, guidance_scale, eta, beta, train_cfg=True, dtype=torch.float64):
    """One micro-batch; batch["advantages"] carries pref.  Returns (loss, info {pref_acc, pref_margin, loss}, h (B,), s (B/2,), loss_p (B/2,))."""
    h = log_ratio_rows_torch(ddim, state, eps_c, eps_u, ref_c, ref_u, batch["latents"], batch["next_latents"], batch["ts"], guidance_scale, eta,
                             train_cfg, dtype)
    y, s, loss_p, _ = pair_terms_torch(h, batch["advantages"], beta)
    m = y * (h[0::2] - h[1::2])
    loss = loss_p.mean()
    info = {"pref_acc": ((y != 0) & (m > 0)).to(dtype).mean(), "pref_margin": m.mean(), "loss": loss}
    return loss, info, h, s, loss_p


def train_step_grads(params, ref_params, cfg, ddim, state, batch, guidance_scale, eta, beta, kl_coef=0.0, train_cfg=True, dtype=torch.float64):
    """Autograd of the d3po loss (+ kl_coef * KL of _kl_oracle) of one micro-batch through oracle.unet.unet_forward, the reference network
    evaluated without a graph.  Returns ({name: grad}, info floats (with "kl_ref" if kl_coef > 0))."""
    leaves = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in params.items()}
    frozen = {k: v.detach().to(dtype) for k, v in ref_params.items()}
    lat, ts = batch["latents"].to(dtype), batch["ts"]
    emb, unc = batch["prompt_embeds"].to(dtype), batch["uncond_embeds"].to(dtype)
    eps_c = OU.unet_forward(leaves, cfg, lat, ts, emb)
    eps_u = OU.unet_forward(leaves, cfg, lat, ts, unc) if train_cfg else None
    with torch.no_grad():
        ref_c = OU.unet_forward(frozen, cfg, lat, ts, emb)
        ref_u = OU.unet_forward(frozen, cfg, lat, ts, unc) if train_cfg else None
    loss, info, *_ = loss_and_info_torch(ddim, state, eps_c, eps_u, ref_c, ref_u, batch, guidance_scale, eta, beta, train_cfg, dtype)
    if kl_coef > 0:
        kl = KO.kl_rows_torch(ddim, state, eps_c, eps_u, ref_c, ref_u, ts, guidance_scale, eta, train_cfg, dtype).mean()
        loss = loss + kl_coef * kl
        info = dict(info, loss=loss, kl_ref=kl)
    names = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[n] for n in names], allow_unused=True)
    return ({n: (torch.zeros_like(leaves[n]) if g is None else g) for n, g in zip(names, grads)},
            {k: float(v.detach()) for k, v in info.items()})


def closed_form_numpy(ddim, state, eps_c, eps_u, ref_c, ref_u, x, x_next, ts, pref, guidance_scale, eta, beta, group, train_cfg=True):
    """The algebra of the HIP pass in fp32 numpy, for `B // group` micro-batches at once:
    (h (B,), s (B/2,), loss_p (B/2,), info (B // group, 3), d_eps_c, d_eps_u | None)."""
    F = np.float32
    B = eps_c.shape[0]
    chw = int(np.prod(eps_c.shape[1:]))
    nd = [1] * (eps_c.ndim - 1)
    a_t, a_p, b_t, std = (np.asarray(v, dtype=F) for v in ddim.coefficients(state, np.asarray(ts), eta))
    sq = lambda v: np.sqrt(v).astype(F)
    dirc = sq(F(1) - a_p - std ** 2)
    if ddim.prediction_type == "epsilon":
        c_t = dirc - sq(a_p) * sq(b_t) / sq(a_t)
    elif ddim.prediction_type == "v_prediction":
        c_t = dirc * sq(a_t) - sq(a_p) * sq(b_t)
    else:
        raise ValueError
    std_c = np.maximum(std, F(1e-6))
    var = (std_c * std_c).astype(F)
    g = F(guidance_scale)
    d_c = (eps_c - ref_c).astype(F)
    delta, e = d_c, eps_c
    if train_cfg:
        d_u = (eps_u - ref_u).astype(F)
        delta = (d_u + g * (d_c - d_u)).astype(F)
        e = (eps_u + g * (eps_c - eps_u)).astype(F)
    r4 = lambda v: v.reshape(B, *nd)
    if ddim.prediction_type == "epsilon":
        mean = r4(sq(a_p)) * ((x - r4(sq(b_t)) * e) / r4(sq(a_t))) + r4(dirc) * e
    else:
        x0 = r4(sq(a_t)) * x - r4(sq(b_t)) * e
        e2 = r4(sq(a_t)) * e + r4(sq(b_t)) * x
        mean = r4(sq(a_p)) * x0 + r4(dirc) * e2
    r = (x_next - mean.astype(F)).astype(F)
    s_rd = (r * delta).reshape(B, -1).sum(1, dtype=F)
    s_dd = (delta * delta).reshape(B, -1).sum(1, dtype=F)
    h = ((F(2) * c_t * s_rd + (c_t * c_t) * s_dd) / (F(2) * var * F(chw))).astype(F)
    pref = np.asarray(pref, dtype=F)
    y = ((pref[0::2] - pref[1::2]) * F(0.5)).astype(F)
    dh = (h[0::2] - h[1::2]).astype(F)
    s = (F(beta) * y * dh).astype(F)
    loss_p = (np.abs(y) * (np.maximum(-s, F(0)) + np.log1p(np.exp(-np.abs(s)).astype(F)).astype(F))).astype(F)
    t = np.exp(-np.abs(s)).astype(F)
    q = np.where(s >= 0, t / (F(1) + t), F(1) / (F(1) + t)).astype(F)
    n = group // 2
    m = (y * dh).astype(F)
    per_mb = lambda v: (v.reshape(B // group, n).sum(1, dtype=F) / F(n)).astype(F)
    info = np.stack([per_mb(((y != 0) & (m > 0)).astype(F)), per_mb(m), per_mb(loss_p)], 1)
    dl_even = (-(F(beta) * y * q) / F(n)).astype(F)
    dl = np.stack([dl_even, -dl_even], 1).reshape(B)
    coef = (dl * (c_t / (var * F(chw)))).astype(F)
    de = (r4(coef) * r).astype(F)
    return h, s, loss_p, info, ((g * de).astype(F) if train_cfg else de), (((F(1) - g) * de).astype(F) if train_cfg else None)
