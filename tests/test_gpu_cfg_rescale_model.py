"""`guidance_rescale` through the sampler and the training step on the SD-2.1-shaped toy (`tiny21`: linear projections, v-prediction) — the
recipe and bounds of tests/test_gpu_model.py::test_sd21_shaped_config_sampler_and_train_step (128 x 128 px, T = 4, g = 5, eta = 1; 1e-3 on
final latents, log-probs and gradient norm), with phi = 0.7 and the oracle loops of tests/_cfg_rescale_oracle.py: the sampler on its
three paths, ratio == 1 before the first update, one PPO step against float64 autograd through the rescale, and the KL / D3PO passes on
the rescaled prediction."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ddpo_amd import lib as L
from ddpo_amd.diffusers_patch.pipeline_stable_diffusion import StableDiffusionPipeline
from ddpo_amd.diffusers_patch.scheduling_ddim import DDIMScheduler
from ddpo_amd.models.unet import UNet2DCondition, UNetConfig
from oracle import prng as OP, unet as OU
from oracle.ddim import DDIMOracle

import _cfg_rescale_oracle as RO

DEV = "cuda"
PHI = 0.7
GUIDE = 5.0
T = 4


def _rel(a, b):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _setup(datapath, monkeypatch, seed=4):
    monkeypatch.setattr(L, "DATAPATH", datapath)
    if datapath == "f16mx":
        monkeypatch.setattr(L, "MX_MIN_K", 256)              # as tests/test_gpu_f16mx_model.py: the toy's 3x3 convolutions become f16mx layers
    op = OU.init_params(OU.unet_param_shapes(OU.TINY21), seed=seed)
    unet = UNet2DCondition(UNetConfig.named("tiny21"), DEV)
    unet.params.load_dict(op)
    if datapath != "fp32":
        unet.params.pack_bf16()
    sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", set_alpha_to_one=False, steps_offset=1,
                          prediction_type="v_prediction")
    return op, unet, sched, StableDiffusionPipeline(unet, None, sched), sched.create_state(device=DEV)


def _prompts(B=2):
    g = torch.Generator().manual_seed(9)
    emb = torch.randn(B, 77, 96, generator=g)
    neg = torch.randn(1, 77, 96, generator=g).expand(B, -1, -1).contiguous()
    return emb, neg


@pytest.fixture(scope="module")
def oracle_run():
    """The oracle's rescaled sampling loop on the fp32 weights, once for the module: (op, outputs)."""
    op = OU.init_params(OU.unet_param_shapes(OU.TINY21), seed=4)
    emb, neg = _prompts()
    dd = DDIMOracle(prediction_type="v_prediction")
    return op, dd, RO.sample(op, OU.TINY21, dd, dd.create_state(), emb, neg, OP.PRNGKey(7), T, 128, 128, GUIDE, 1.0, PHI)


def test_sampler_matches_the_oracle_loop_on_every_path(oracle_run, monkeypatch):
    _, _, (ofinal, olat, onxt, olps, ots) = oracle_run
    op, unet, sched, pipe, state = _setup("fp32", monkeypatch)
    emb, neg = _prompts()
    args = (emb.to(DEV), neg.to(DEV), {"unet": unet.params, "scheduler": state}, OP.PRNGKey(7), T)
    kw = dict(height=128, width=128, guidance_scale=GUIDE, eta=1.0)
    eager = pipe(*args, guidance_rescale=PHI, **kw)
    final, lat, nxt, lps, ts = eager
    assert np.array_equal(ts.cpu().numpy(), ots)
    e_f, e_lp = _rel(final, ofinal), float(np.abs(lps.cpu().numpy() - olps).max())
    from conftest import parity_record
    parity_record(f"[cfg rescale tiny21 sampler T={T} phi={PHI}] final latents {e_f:.2e}  log-probs abs {e_lp:.2e}")
    assert e_f < 1e-3
    np.testing.assert_allclose(lps.cpu().numpy(), olps, rtol=1e-3, atol=1e-3)
    # the rescale is not a no-op on these rows: the plain sampler ends elsewhere
    plain = pipe(*args, **kw)
    print(f"plain sampler against the rescaled oracle: final latents {_rel(plain[0], ofinal):.2e}")
    assert not torch.equal(plain[0], final) and not torch.equal(plain[3], lps)
    # the graph path, with and without the staging kernel, gives the eager path's bits
    graphed = pipe(*args, jit=True, guidance_rescale=PHI, **kw)
    monkeypatch.setenv("DDPO_STAGE_KERNEL", "0")
    unstaged = pipe(*args, jit=True, guidance_rescale=PHI, **kw)
    for other in (graphed, unstaged):
        for a, b in zip(eager, other):
            assert torch.equal(a, b)
    # guidance_rescale = 0.0 is the call without the argument, bit for bit, and loads nothing
    zero = pipe(*args, guidance_rescale=0.0, **kw)
    for a, b in zip(plain, zero):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="guidance_rescale"):
        pipe(*args, guidance_rescale=1.5, **kw)


@pytest.mark.parametrize("datapath", ["f16mx", "fp32"])
def test_ratio_is_one_before_the_first_update(datapath, monkeypatch):
    """The engine's own stored transition, scored by the training forward of the same weights through the same rescale launch: the stored
    log-prob comes back bit for bit, ratio == 1.0, approx_kl == 0 — eagerly and under graph replay."""
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdamWConfig, train_step
    op, unet, sched, pipe, state0 = _setup(datapath, monkeypatch, seed=2)
    emb, neg = (x.to(DEV) for x in _prompts(4))
    final, lat, nxt, lps, ts = pipe(emb, neg, {"unet": unet.params, "scheduler": state0}, OP.PRNGKey(4), T, height=64, width=64,
                                    guidance_scale=GUIDE, eta=1.0, guidance_rescale=PHI)
    st = sched.set_timesteps(sched.create_state(device=DEV), T)
    state = AccumulatingTrainState(unet, AdamWConfig())
    for step, jit in ((0, False), (3, True)):
        batch = {"latents": lat[:2, step].contiguous(), "next_latents": nxt[:2, step].contiguous(), "ts": ts[:2, step].contiguous(),
                 "log_probs": lps[:2, step].contiguous(), "advantages": torch.tensor([0.5, -0.5], device=DEV), "prompt_embeds": emb[:2],
                 "uncond_embeds": neg[:2]}
        state, info = train_step(state, batch, st, sched, True, GUIDE, 1.0, 1e-4, do_opt_update=False, jit=jit, guidance_rescale=PHI)
        assert torch.equal(info["log_prob"].view(torch.int32), batch["log_probs"].view(torch.int32))
        assert float(info["approx_kl"]) == 0.0 and float(info["clipfrac"]) == 0.0
        # without the rescale the same transition is NOT the policy's: the two must be one function
        _, plain = train_step(state, batch, st, sched, True, GUIDE, 1.0, 1e-4, do_opt_update=False, jit=False)
        assert float(plain["approx_kl"]) > 0.0
    assert bool(torch.isfinite(unet.grads.flat).all()) and float(unet.grads.flat.abs().max()) > 0


def _train_batch(oracle_run):
    _, _, (ofinal, olat, onxt, olps, ots) = oracle_run
    emb, neg = _prompts()
    return {"latents": torch.from_numpy(olat[:, 1]), "next_latents": torch.from_numpy(onxt[:, 1]), "ts": torch.from_numpy(ots[:, 1].copy()),
            "log_probs": torch.from_numpy(olps[:, 1]) + torch.tensor([3e-5, -2e-5]), "advantages": torch.tensor([0.9, -1.4]),
            "prompt_embeds": emb, "uncond_embeds": neg}


@pytest.mark.parametrize("datapath", ["fp32", "bf16x3"])
def test_ppo_step_matches_float64_autograd_through_the_rescale(oracle_run, datapath, monkeypatch):
    """One PPO micro-step on the oracle's rescaled trajectory at timestep index 1: gradient norm rel 1e-3, every parameter tensor 2e-3 of
    its maximum (the bounds of tests/test_gpu_dpo_train_step.py)."""
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdamWConfig, train_step
    op, dd, _ = oracle_run
    batch = _train_batch(oracle_run)
    ost = dd.set_timesteps(dd.create_state(), T)
    ograds, oinfo, olp = RO.train_step_grads(op, OU.TINY21, dd, ost, {k: (v if k == "ts" else v.double()) for k, v in batch.items()},
                                             GUIDE, 1.0, 1e-4, PHI)
    _, unet, sched, _, state = _setup(datapath, monkeypatch)
    st4 = sched.set_timesteps(state, T)
    tstate = AccumulatingTrainState(unet, AdamWConfig())
    tstate, info = train_step(tstate, {k: v.to(DEV) for k, v in batch.items()}, st4, sched, True, GUIDE, 1.0, 1e-4, do_opt_update=False,
                              guidance_rescale=PHI)
    G = unet.grads
    gn_o = math.sqrt(sum(float((v.double() ** 2).sum()) for v in ograds.values()))
    gn = math.sqrt(float((G.flat.double() ** 2).sum()))
    worst = max((_rel(G[n], ograds[n]), n) for n in ograds if float(ograds[n].abs().max()) > 1e-6 * gn_o)
    e_lp = float((info["log_prob"].cpu().double() - olp).abs().max())
    from conftest import parity_record
    parity_record(f"[cfg rescale tiny21 train step phi={PHI}] {datapath}: grad-norm rel err {abs(gn - gn_o) / gn_o:.2e}  worst tensor "
                  f"{worst[0]:.2e} ({worst[1]})  log-prob abs {e_lp:.2e}  loss {float(info['loss']):.6g} vs {oinfo['loss']:.6g}")
    assert gn_o > 0 and e_lp < 1e-3
    assert gn == pytest.approx(gn_o, rel=1e-3)
    assert worst[0] < 2e-3, worst


@pytest.mark.parametrize("loss", ["ppo", "d3po"])
def test_kl_and_d3po_passes_see_the_rescaled_prediction(oracle_run, loss, monkeypatch):
    """Reference = a copy of the policy, rescaled by the same launch: kl_ref == 0.0 and the D3PO margin is 0.0 exactly, while the gradient
    is finite and non-zero; the fused launch of two micro-batches says the same per micro-batch."""
    from ddpo_amd.training.kl_reference import KLReference
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdamWConfig, train_step, train_steps_fused
    _, unet, sched, _, state = _setup("fp32", monkeypatch)
    ref = KLReference(unet)
    st4 = sched.set_timesteps(state, T)
    batch = {k: v.to(DEV) for k, v in _train_batch(oracle_run).items()}
    if loss == "d3po":
        batch["advantages"] = torch.tensor([1.0, -1.0], device=DEV)
    tstate = AccumulatingTrainState(unet, AdamWConfig())
    kw = dict(kl_coef=0.5, ref_unet=ref, guidance_rescale=PHI, **(dict(loss="d3po", d3po_beta=0.1) if loss == "d3po" else {}))
    tstate, info = train_step(tstate, batch, st4, sched, True, GUIDE, 1.0, 1e-4, do_opt_update=False, **kw)
    assert float(info["kl_ref"]) == 0.0
    if loss == "d3po":
        assert float(info["pref_margin"]) == 0.0
    g1 = unet.grads.flat.clone()
    assert bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0 and math.isfinite(float(info["loss"]))
    unet.grads.flat.zero_()
    tstate, infos = train_steps_fused(tstate, [batch, batch], st4, sched, True, GUIDE, 1.0, 1e-4, do_opt_update=False, jit=False, **kw)
    assert len(infos) == 2 and all(float(i["kl_ref"]) == 0.0 for i in infos)
    assert torch.allclose(unet.grads.flat, 2 * g1, rtol=1e-3, atol=1e-6 * float(g1.abs().max()))
    with pytest.raises(ValueError, match="train_cfg True"):
        train_step(tstate, batch, st4, sched, False, GUIDE, 1.0, 1e-4, do_opt_update=False, guidance_rescale=PHI)
