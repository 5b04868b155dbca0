"""Diffusion-DPO train step on ranked pairs of stored samples (`pipeline/dpo.py`; DESIGN.md §4, Diffusion-DPO) — the offline counterpart of
`--pg_loss d3po`, beside the RWR step of training/diffusion.py.

Wallace et al., "Diffusion Model Alignment Using Direct Preference Optimization": two samples of one prompt sit on rows (2p, 2p+1), ranked
by `pref`; both are noised with ONE diffusion noise at ONE timestep, and the policy is trained so that its denoising error drops faster on
the winner than on the loser, relative to the frozen pretrained model.  Device work: the RWR step's (threefry normals,
ddpo_rwr_noisy_latents, U-Net forward with a tape, U-Net backward, fused optimizer update) with ddpo_dpo_pair_fwd_bwd in the place of
ddpo_rwr_mse_fwd_bwd, plus one inference forward of the frozen copy (training/kl_reference.py) on the same inputs.
"""
import math

import torch

from .diffusion import noised_with_target, prepare_latents
from .policy_gradient import AccumulatingTrainState

INFO_KEYS = ("loss", "implicit_acc", "margin", "mse", "ref_mse")


def check_dpo_args(dpo_beta, train_batch_size):
    """The entrypoint's argument check, as a plain function: a message to exit with, or None."""
    beta = float(dpo_beta)
    if not (math.isfinite(beta) and beta > 0.0):
        return f"--dpo_beta must be a finite number > 0, got {beta}"
    if int(train_batch_size) % 2:
        return f"pipeline/dpo.py trains on adjacent pairs of rows: --train_batch_size must be even, got {train_batch_size}"
    return None


def prepare_pair_latents(vae_moments, train_rng, noise_scheduler_state, prediction_type=None):
    """The key tree of diffusion.prepare_latents with the diffusion noise and the timestep drawn per PAIR: vae_moments (B,h,w,2C) NHWC with
    pairs on adjacent rows -> (noise (B,C,h,w), timesteps (B,), noisy_latents, new_train_rng); rows 2p and 2p+1 share noise and timestep
    (the authors' training code), each row has its own posterior sample.  `prediction_type` given: the same draws and noisy latents, and a
    fifth result, the regression target of such a model (diffusion.prepare_latents); rows of a pair share the noise, not the target."""
    return prepare_latents(vae_moments, train_rng, noise_scheduler_state, prediction_type, pairs=True)


def forward_backward(unet, text_encoder, batch, train_rng, noise_scheduler_state, train_cfg, guidance_scale, ref, beta):
    """Everything of train_step before the optimizer update: the gradient lands in unet.grads.
    Returns (info (5,) device tensor in the order of INFO_KEYS, per_row, per_pair, new_train_rng)."""
    from .. import lib_dpo as LD
    dev = unet.device
    moments = torch.as_tensor(batch["vae"], dtype=torch.float32, device=dev)
    pref = torch.as_tensor(batch["pref"], dtype=torch.float32, device=dev).reshape(-1).contiguous()
    # `noise`: the target of the model's prediction type, against which both networks' errors are taken
    noise, ts, noisy, new_train_rng = noised_with_target(unet, moments, train_rng, noise_scheduler_state, pairs=True)
    emb = batch["prompt_embeds"] if "prompt_embeds" in batch else text_encoder(batch["input_ids"])
    b = noisy.shape[0]
    tape = []
    if train_cfg:
        unc = batch["uncond_embeds"] if "uncond_embeds" in batch else text_encoder(batch["uncond_text"])
        x, t, ctx = torch.cat([noisy, noisy]), torch.cat([ts, ts]), torch.cat([unc, emb]).contiguous()
        out = unet.forward(x, t, ctx, tape=tape)
        eps_u, eps_c = out[:b].contiguous(), out[b:].contiguous()
        rout = ref.forward(x, t, ctx)
        ref_u, ref_c = rout[:b].contiguous(), rout[b:].contiguous()
    else:
        ctx = emb.contiguous()
        eps_u, eps_c = None, unet.forward(noisy, ts, ctx, tape=tape)
        ref_u, ref_c = None, ref.forward(noisy, ts, ctx)
    d_c, d_u, per_row, per_pair, info = LD.dpo_pair_fwd_bwd(eps_c, eps_u, ref_c, ref_u, noise, pref, float(guidance_scale), float(beta),
                                                            bool(train_cfg))
    unet.backward(tape, torch.cat([d_u, d_c]) if train_cfg else d_c)
    return info, per_row, per_pair, new_train_rng


def train_step(state: AccumulatingTrainState, text_encoder, batch, train_rng, noise_scheduler_state, static_broadcasted, ref, beta):
    """One Diffusion-DPO step.  batch: "vae" (b,h,w,8) posterior moments with pairs on adjacent rows, "pref" (b,) labels (+1 winner,
    -1 loser), "input_ids" / "uncond_text" (or precomputed "prompt_embeds" / "uncond_embeds"); static_broadcasted as in
    diffusion.train_step; `ref` a KLReference of the pretrained policy.  Returns (state, info {INFO_KEYS: device scalar}, new_train_rng)."""
    noise_scheduler, te2, train_cfg, guidance_scale = static_broadcasted
    text_encoder = text_encoder if text_encoder is not None else te2
    info, _, _, new_train_rng = forward_backward(state.unet, text_encoder, batch, train_rng, noise_scheduler_state, train_cfg,
                                                 guidance_scale, ref, beta)
    state = state.apply_gradients(do_update=True)             # pmean(grad) + optimizer step, every call
    return state, {k: info[i] for i, k in enumerate(INFO_KEYS)}, new_train_rng
