"""The Diffusion-DPO step (ddpo_amd/training/diffusion_dpo.py) on the tiny U-Net, B = 2 (one pair) and B = 4 (two), 8 x 8 latents — the
recipe of tests/test_gpu_pref_train_step.py: the pair version of the RWR step's key tree against the oracle, an error difference of exactly
zero before the first update, float64 autograd with a reference that differs, and one full step."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ddpo_amd import lib as L
from oracle import diffusion as OD, prng as OP, unet as OU

import _dpo_oracle as DO

DEV = "cuda"
HW = 8
BLEND = 1e-2                      # second-seed parameters blended into the first: the reference of tests/test_gpu_kl_train_step.py
GUIDE = 5.0


def _rel(a, b):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _moments(B, seed):
    g = torch.Generator().manual_seed(seed)
    m = torch.randn(B, HW, HW, 8, generator=g)
    m[..., 4:] = m[..., 4:] * 3.0 - 4.0                  # log-variances around -4, some outside the clip range [-30, 20] below
    m[0, 0, 0, 4] = -35.0
    m[-1, -1, -1, 7] = 25.0
    return m


def _unet(op):
    from ddpo_amd.models.unet import UNet2DCondition, UNetConfig
    unet = UNet2DCondition(UNetConfig.named("tiny"), DEV)
    unet.params.load_dict(op)
    if L.current_datapath() != "fp32":
        unet.params.pack_bf16()
    return unet


def _batch(B, seed=5):
    """B / 2 pairs: the two rows of a pair are two samples (their own VAE moments) of ONE prompt; the labels alternate +1, -1 per pair."""
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn(B // 2, 77, 64, generator=g).repeat_interleave(2, dim=0).contiguous()
    unc = torch.randn(1, 77, 64, generator=g).expand(B, -1, -1).contiguous()
    y = np.resize(np.asarray([1.0, -1.0], dtype=np.float32), B // 2)
    return {"vae": _moments(B, seed + B), "prompt_embeds": emb, "uncond_embeds": unc, "pref": np.stack([y, -y], 1).reshape(B)}


def _to_dev(batch):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _blended(op, seed=1):
    op2 = OU.init_params(OU.unet_param_shapes(OU.TINY), seed=seed)
    return {n: (op[n] + BLEND * (op2[n] - op[n])).contiguous() for n in op}


@pytest.mark.parametrize("B", [2, 4])
def test_prepare_pair_latents_equals_the_oracle(B):
    from ddpo_amd.training.diffusion import DDPMNoiseScheduler
    from ddpo_amd.training.diffusion_dpo import prepare_pair_latents
    sched = DDPMNoiseScheduler()
    acp = OD.ddpm_alphas_cumprod()
    m = _moments(B, 3 + B)
    key = OP.PRNGKey(17 * B + HW)
    ref = DO.prepare_pairs(m.numpy(), key, acp)
    noise, ts, noisy, new_rng = prepare_pair_latents(m.to(DEV), key, sched.create_state(DEV))
    assert ts.dtype == torch.int32 and np.array_equal(ts.cpu().numpy(), ref["timesteps"])      # jax.random.randint: integer-exact
    assert np.array_equal(np.asarray(new_rng), ref["new_train_rng"])
    assert _rel(noise, ref["noise"]) < 2e-6                                          # Threefry words bit-equal; erfinv polynomial in fp32
    assert _rel(noisy, ref["noisy_latents"]) < 2e-6
    # rows 2p and 2p+1 share noise and timestep bit for bit; the posterior samples (and so the noisy latents) are their own
    assert torch.equal(noise[0::2].view(torch.int32), noise[1::2].view(torch.int32)) and torch.equal(ts[0::2], ts[1::2])
    assert not torch.equal(noisy[0::2], noisy[1::2])
    if B == 4:
        assert not torch.equal(noise[0], noise[2])
    # the single-row draw of the RWR step is another one: the pair step does not reuse its per-row noise
    assert np.array_equal(ref["new_train_rng"], OD.prepare(m.numpy(), key, acp)["new_train_rng"])


@pytest.mark.parametrize("datapath", ["fp32", "f16mx"])
@pytest.mark.parametrize("B", [2, 4])
def test_error_difference_is_zero_before_the_first_update(datapath, B):
    """Reference = a copy of the policy: its inference forward and the policy's training forward give the same bits, so D is exactly 0:
    margin == 0.0, the loss has the bits of log1pf(1.0f) — and the gradient is there (q = 1/2, not 0)."""
    from ddpo_amd.training.diffusion import DDPMNoiseScheduler
    from ddpo_amd.training.diffusion_dpo import forward_backward
    from ddpo_amd.training.kl_reference import KLReference
    L.DATAPATH = datapath
    op = OU.init_params(OU.unet_param_shapes(OU.TINY), seed=0)
    unet = _unet(op)
    ref = KLReference(unet)
    info, per_row, per_pair, _ = forward_backward(unet, None, _to_dev(_batch(B)), OP.PRNGKey(9), DDPMNoiseScheduler().create_state(DEV),
                                                  True, GUIDE, ref, 5000.0)
    assert bool((per_row[:, 1] == 0.0).all()) and float(info[2]) == 0.0 and float(info[1]) == 0.0
    assert torch.equal(info[0].view(torch.int32), torch.log1p(torch.ones((), device=DEV)).view(torch.int32))
    assert float(info[3]) > 0 and float(info[3]) == float(info[4])
    g = unet.grads.flat
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert ref.unet.grads is None


@pytest.mark.parametrize("train_cfg,B", [(True, 4), (False, 2)])
def test_step_with_a_different_reference_matches_float64_autograd(train_cfg, B):
    """Bounds as in tests/test_gpu_pref_train_step.py and tests/test_gpu_kl_train_step.py (the same reference, the same U-Net backward):
    1e-3 on loss, margin and gradient norm, 2e-3 of its maximum on every parameter tensor.  beta on the host: the largest |s_p| of the
    float64 oracle is 1, so q = sigmoid(-+1) is off the centre and far from saturation."""
    from ddpo_amd.training.diffusion import DDPMNoiseScheduler
    from ddpo_amd.training.diffusion_dpo import forward_backward
    from ddpo_amd.training.kl_reference import KLReference
    op = OU.init_params(OU.unet_param_shapes(OU.TINY), seed=0)
    rop = _blended(op)
    batch = _batch(B)
    key = OP.PRNGKey(23)
    prep = DO.prepare_pairs(batch["vae"].numpy(), key, OD.ddpm_alphas_cumprod())
    d = lambda p: {k: v.double() for k, v in p.items()}
    with torch.no_grad():
        ec, eu = DO.network_outputs(d(op), OU.TINY, prep, batch["prompt_embeds"], batch["uncond_embeds"], train_cfg)
        rc, ru = DO.network_outputs(d(rop), OU.TINY, prep, batch["prompt_embeds"], batch["uncond_embeds"], train_cfg)
        D = DO.loss_and_info_torch(ec, eu, rc, ru, torch.from_numpy(prep["noise"]), batch["pref"], GUIDE, 1.0, train_cfg)[3]
    beta = 1.0 / float((0.5 * (D[0::2] - D[1::2])).abs().max())
    ograds, oinfo, _ = DO.train_step_grads(op, rop, OU.TINY, prep, batch["prompt_embeds"], batch["uncond_embeds"], batch["pref"], GUIDE,
                                           beta, train_cfg)
    print(f"oracle: beta {beta:.4g}, D {D.tolist()}, " + ", ".join(f"{k} {v:.6g}" for k, v in oinfo.items()))
    unet = _unet(op)
    ref = KLReference(unet)
    ref.params.load_dict(rop)
    info, per_row, per_pair, new_rng = forward_backward(unet, None, _to_dev(batch), key, DDPMNoiseScheduler().create_state(DEV), train_cfg,
                                                        GUIDE, ref, beta)
    got = dict(zip(DO.INFO_KEYS, (float(v) for v in info)))
    G = unet.grads
    norm = lambda gs: math.sqrt(sum(float((v.double() ** 2).sum()) for v in gs.values()))
    gn_o = norm(ograds)
    gn = math.sqrt(float((G.flat.double() ** 2).sum()))
    worst = max((_rel(G[n], ograds[n]), n) for n in ograds if float(ograds[n].abs().max()) > 1e-6 * gn_o)
    print(f"device: " + ", ".join(f"{k} {v:.6g}" for k, v in got.items()) + f"; grad norm {gn:.6e} vs {gn_o:.6e}; worst tensor {worst}")
    # that file's bound on its margin, carried to n pairs: every row's D is held to 1e-3 of itself, the margin is the mean over the pairs
    # of a difference of two of them; s = 0.5 beta times that difference and |d softplus / d s| <= 1
    d_mean = float(D.abs().sum()) / (B // 2)
    print(f"errors: margin {abs(got['margin'] - oinfo['margin']):.3e} (bound {1e-3 * d_mean:.3e}), "
          f"loss {abs(got['loss'] - oinfo['loss']):.3e} (bound {0.5 * beta * 1e-3 * d_mean:.3e})")
    assert abs(got["margin"] - oinfo["margin"]) < 1e-3 * d_mean
    assert abs(got["loss"] - oinfo["loss"]) < 0.5 * beta * 1e-3 * d_mean
    assert got["implicit_acc"] == oinfo["implicit_acc"]
    assert got["mse"] == pytest.approx(oinfo["mse"], rel=1e-3) and got["ref_mse"] == pytest.approx(oinfo["ref_mse"], rel=1e-3)
    assert gn == pytest.approx(gn_o, rel=1e-3)
    assert worst[0] < 2e-3, worst
    assert np.array_equal(np.asarray(new_rng), prep["new_train_rng"])


def test_train_step_updates_and_hands_on_the_key():
    """One full train_step: the step counter advances, the gradients are cleared, the next key equals the oracle's, the parameters moved
    and the reference did not."""
    from ddpo_amd.training.diffusion import DDPMNoiseScheduler
    from ddpo_amd.training.diffusion_dpo import INFO_KEYS, train_step
    from ddpo_amd.training.kl_reference import KLReference
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdamWConfig
    B = 4
    op = OU.init_params(OU.unet_param_shapes(OU.TINY), seed=8)
    unet = _unet(op)
    ref = KLReference(unet)
    snapshot = ref.params.flat.clone()
    before = unet.params.flat.clone()
    sched = DDPMNoiseScheduler()
    state = AccumulatingTrainState(unet, AdamWConfig(learning_rate=1e-4))
    batch = _batch(B, seed=2)
    key = OP.PRNGKey(5)
    prep = DO.prepare_pairs(batch["vae"].numpy(), key, sched.alphas_cumprod)
    state, info, new_rng = train_step(state, None, _to_dev(batch), key, sched.create_state(DEV), (sched, None, True, GUIDE), ref, 5000.0)
    assert tuple(info) == INFO_KEYS and all(math.isfinite(float(v)) for v in info.values())
    assert float(info["margin"]) == 0.0                                   # the first step: the policy IS the reference
    assert np.array_equal(np.asarray(new_rng), prep["new_train_rng"])
    assert state.step == 1 and state.n_acc == 0 and float(unet.grads.flat.abs().max()) == 0.0
    assert not torch.equal(unet.params.flat, before)
    assert torch.equal(ref.params.flat.view(torch.int32), snapshot.view(torch.int32))
    # the second step sees a policy that has moved away from the reference
    state, info, _ = train_step(state, None, _to_dev(batch), new_rng, sched.create_state(DEV), (sched, None, True, GUIDE), ref, 5000.0)
    assert state.step == 2 and float(info["margin"]) != 0.0 and math.isfinite(float(info["loss"]))
