"""Oracle (test infrastructure only) of `--guidance_rescale` (include/ddpo_cfg_rescale.h): the rescaled classifier-free
guidance of Lin et al., §3.4, as a float64 torch function that autograd differentiates, its closed-form gradient, the fp32 numpy
restatement of that closed form in the order of the HIP pass, the input generator of the kernel tests, and the sampler / train-step loops
assembled from the read-only pieces of oracle/ with the rescale between the network and the DDIM step.

    c = u + g (t - u);  k = 1 - phi + phi std(t) / std(c)  (unbiased, per row);  out = k c
    dL/dc_i = k G_i - S phi (s_t / s_c) (c_i - mean c) / ((n - 1) s_c^2),  S = sum_j G_j c_j
    dL/dt_i = g dL/dc_i + S phi (t_i - mean t) / ((n - 1) s_t s_c);  dL/du_i = (1 - g) dL/dc_i
"""
import numpy as np
import torch

GUIDE = 5.0
PHI = 0.7
U_NOISE = 0.33                                        # u = t + 0.33 N(0, 1)


def rescale_torch(t, u, g, phi):
    """The formula as written, on (B, ...) tensors of any float dtype; statistics per row over all other axes.  Returns (out, k (B,))."""
    c = u + g * (t - u)
    st = t.flatten(1).std(dim=1)
    sc = c.flatten(1).std(dim=1)
    k = 1.0 - phi + phi * st / sc
    return k.reshape(-1, *([1] * (t.ndim - 1))) * c, k


def grads_closed_form_torch(t, u, G, g, phi):
    """(dL/dt, dL/du) for the cotangent G of `out`, by the closed form above, in the dtype of the inputs."""
    B = t.shape[0]
    n = t[0].numel()
    col = lambda v: v.reshape(B, *([1] * (t.ndim - 1)))
    c = u + g * (t - u)
    mt, mc = col(t.flatten(1).mean(1)), col(c.flatten(1).mean(1))
    st, sc = col(t.flatten(1).std(dim=1)), col(c.flatten(1).std(dim=1))
    k = 1.0 - phi + phi * st / sc
    S = col((G * c).flatten(1).sum(1))
    dc = k * G - S * phi * (st / sc) * (c - mc) / ((n - 1) * sc ** 2)
    dt = g * dc + S * phi * (t - mt) / ((n - 1) * st * sc)
    return dt, (1.0 - g) * dc


def closed_form_numpy(t, u, G, g, phi):
    """fp32 restatement of the HIP passes, every operation rounded to fp32 (numpy's own summation order): out, stats (B, 4) =
    {mean t, s_t, mean c, s_c}, and, if G is given, (dL/dt, dL/du)."""
    F = np.float32
    t, u = np.asarray(t, dtype=F), np.asarray(u, dtype=F)
    B = t.shape[0]
    n = t[0].size
    g, phi = F(g), F(phi)
    col = lambda v: v.reshape(B, *([1] * (t.ndim - 1))).astype(F)
    c = (u + g * (t - u)).astype(F)
    rows = lambda a: a.reshape(B, -1)
    mt = (rows(t).sum(1, dtype=F) / F(n)).astype(F)
    mc = (rows(c).sum(1, dtype=F) / F(n)).astype(F)
    dvt = (t - col(mt)).astype(F)
    dvc = (c - col(mc)).astype(F)
    st = np.sqrt((rows(dvt * dvt).sum(1, dtype=F) / F(n - 1)).astype(F)).astype(F)
    sc = np.sqrt((rows(dvc * dvc).sum(1, dtype=F) / F(n - 1)).astype(F)).astype(F)
    r = (st / sc).astype(F)
    k = ((F(1.0) - phi) + phi * r).astype(F)
    out = (col(k) * c).astype(F)
    stats = np.stack([mt, st, mc, sc], 1).astype(F)
    if G is None:
        return out, stats
    G = np.asarray(G, dtype=F)
    S = rows((G * c).astype(F)).sum(1, dtype=F).astype(F)
    nm1 = F(n - 1)
    ca = ((S * phi) * r / (nm1 * (sc * sc))).astype(F)
    cb = ((S * phi) / (nm1 * (st * sc))).astype(F)
    dc = (col(k) * G - col(ca) * dvc).astype(F)
    dt = (g * dc + col(cb) * dvt).astype(F)
    du = ((F(1.0) - g) * dc).astype(F)
    return out, stats, dt, du


def inputs(B, chw, row_mean=0.0):
    """fp32 numpy (B, 4, chw / 4, 1): t ~ N(0, 1), u = t + 0.33 N(0, 1), both shifted by `row_mean`, and the cotangent G ~ N(0, 1)."""
    rng = np.random.default_rng(chw * 131 + B * 7 + 53)
    shp = (B, 4, chw // 4, 1)
    t = rng.standard_normal(shp, dtype=np.float32)
    u = (t + np.float32(U_NOISE) * rng.standard_normal(shp, dtype=np.float32)).astype(np.float32)
    G = rng.standard_normal(shp, dtype=np.float32)
    if row_mean:
        t, u = (t + np.float32(row_mean)).astype(np.float32), (u + np.float32(row_mean)).astype(np.float32)
    return t, u, G


def reference(t, u, G, g=GUIDE, phi=PHI):
    """float64 autograd of rescale_torch on the fp32 inputs: out, k (B,), stats (B, 4), dL/dt, dL/du for L = sum(G out)."""
    d = lambda a: torch.from_numpy(np.asarray(a)).double()
    tt, uu = d(t).requires_grad_(True), d(u).requires_grad_(True)
    out, k = rescale_torch(tt, uu, g, phi)
    (out * d(G)).sum().backward()
    with torch.no_grad():
        c = uu + g * (tt - uu)
        stats = torch.stack([tt.flatten(1).mean(1), tt.flatten(1).std(dim=1), c.flatten(1).mean(1), c.flatten(1).std(dim=1)], 1)
    return out.detach().numpy(), k.detach().numpy(), stats.numpy(), tt.grad.numpy(), uu.grad.numpy()


NAMES = ("out", "mean", "std", "d_t", "d_u")


def errors(ref, out, stats, dt, du):
    """In the order of NAMES: out, d_t, d_u relative to the case maximum of the float64 value; the two means relative to their row's
    standard deviation (a mean near zero has no scale of its own); the two standard deviations relative to themselves."""
    rout, _, rstats, rdt, rdu = ref
    f = lambda a: np.asarray(a, dtype=np.float64)
    stats = f(stats)
    e_mean = max(float((np.abs(stats[:, 0] - rstats[:, 0]) / rstats[:, 1]).max()), float((np.abs(stats[:, 2] - rstats[:, 2]) / rstats[:, 3]).max()))
    e_std = max(float((np.abs(stats[:, 1] - rstats[:, 1]) / rstats[:, 1]).max()), float((np.abs(stats[:, 3] - rstats[:, 3]) / rstats[:, 3]).max()))
    return (float(np.abs(f(out) - rout).max() / np.abs(rout).max()), e_mean, e_std,
            float(np.abs(f(dt) - rdt).max() / np.abs(rdt).max()), float(np.abs(f(du) - rdu).max() / np.abs(rdu).max()))


# ------------------------------------------------------------------------------------------------ sampler and train step through oracle/
def sample(unet_params, cfg, ddim, sched_state, prompt_embeds, neg_embeds, key, num_inference_steps, height, width, guidance_scale, eta,
           guidance_rescale, dtype=torch.float32):
    """oracle.sampler.sample with the rescale between the network and the DDIM step: the same key tree and fp32 trajectory, the two halves
    of oracle.unet.unet_forward combined by rescale_torch in float64 and handed to DDIMOracle.step as its ONE model output.
    Returns numpy (final_latents, latents (B,T,..), next_latents (B,T,..), log_probs (B,T), ts (B,T))."""
    from oracle import prng
    from oracle.unet import unet_forward
    B = prompt_embeds.shape[0]
    context = torch.cat([neg_embeds, prompt_embeds]).to(dtype)
    shape = (B, cfg.in_channels, height // 8, width // 8)
    rng, seed = prng.split(np.asarray(key, dtype=np.uint32))
    latents = prng.normal(seed, shape)
    state = ddim.set_timesteps(sched_state, num_inference_steps)
    latents = latents * state.init_noise_sigma
    rng, seed = prng.split(rng)
    rng = seed
    lat_t, next_t, lp_t, ts_t = [], [], [], []
    for step in range(num_inference_steps):
        t = int(state.timesteps[step])
        inp = torch.from_numpy(np.concatenate([latents] * 2)).to(dtype)
        with torch.no_grad():
            noise_pred = unet_forward(unet_params, cfg, inp, torch.full((2 * B,), t, dtype=torch.int32), context).double()
            guided = rescale_torch(noise_pred[B:], noise_pred[:B], guidance_scale, guidance_rescale)[0].to(torch.float32).numpy()
        rng, k = prng.split(rng)
        z = prng.normal(k, shape)
        new_latents, log_prob = ddim.step(state, guided, t, latents, noise=z, eta=eta)
        lat_t.append(latents); next_t.append(new_latents); lp_t.append(log_prob); ts_t.append(t)
        latents = new_latents
    ts = np.broadcast_to(np.asarray(ts_t, dtype=np.int32), (B, num_inference_steps))
    return (latents, np.stack(lat_t, 1), np.stack(next_t, 1), np.stack(lp_t, 1), ts)


def train_step_grads(unet_params, cfg, ddim, sched_state, batch, guidance_scale, eta, clip_range, guidance_rescale, dtype=torch.float64):
    """oracle.sampler.train_step_grads with the rescale: autograd of the PPO-clip loss of the RESCALED guided prediction (oracle.ppo's
    single-output form) through rescale_torch and oracle.unet.unet_forward.  Returns ({name: grad}, info floats, log_prob (B,))."""
    from oracle import ppo
    from oracle.unet import unet_forward
    leaves = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in unet_params.items()}
    lat = batch["latents"].to(dtype)
    ts = batch["ts"]
    eps_c = unet_forward(leaves, cfg, lat, ts, batch["prompt_embeds"].to(dtype))
    eps_u = unet_forward(leaves, cfg, lat, ts, batch["uncond_embeds"].to(dtype))
    guided, _ = rescale_torch(eps_c, eps_u, guidance_scale, guidance_rescale)
    loss, info, log_prob = ppo.loss_and_info_torch(ddim, sched_state, guided, None, batch, guidance_scale, eta, clip_range, False, dtype)
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    return grads, {k: float(v.detach()) for k, v in info.items()}, log_prob.detach()
