"""`kl_coef` through the whole training step (ddpo_amd/training/policy_gradient.py) on the tiny U-Net, b = 2, 8 x 8 latents — the recipe of
tests/test_gpu_backward.py::test_train_step_grads_match_oracle, rebuilt here: exactly no penalty before the first update, float64 autograd
of ppo + kl_coef * kl with a reference that differs, the fused step, the untouched default path, and LoRA."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ddpo_amd import lib as L

import _kl_oracle as KO

DEV = "cuda"
B, HW = 2, 8
# second-seed parameters blended into the first, and the coefficient: chosen on the host so that in the float64 oracle the KL part of the
# parameter gradient has 0.3 .. 3 times the norm of the PPO part (train_cfg: 1.62, without: 1.16; asserted below)
BLEND, KL_COEF = 1e-2, {True: 1.0, False: 3.0}


def _rel(a, b):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _sched():
    from ddpo_amd.diffusers_patch.scheduling_ddim import DDIMScheduler
    from oracle.ddim import DDIMOracle
    sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", set_alpha_to_one=False, steps_offset=1)
    st = sched.set_timesteps(sched.create_state(device=DEV), 50)
    dd = DDIMOracle()
    return sched, st, dd, dd.set_timesteps(dd.create_state(), 50)


def _unet(op):
    from ddpo_amd.models.unet import UNet2DCondition, UNetConfig
    unet = UNet2DCondition(UNetConfig.named("tiny"), DEV)
    unet.params.load_dict(op)
    if L.current_datapath() != "fp32":
        unet.params.pack_bf16()
    return unet


def _batch(op, dd, ost, train_cfg, seed=5):
    """latents, a transition sampled by the oracle from its own (guided) prediction so the ratios are near 1, old log-probs around the clip range."""
    from oracle import unet as OU
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(B, 4, HW, HW, generator=g)
    ts = torch.tensor([481, 21], dtype=torch.int32)
    emb = torch.randn(B, 77, 64, generator=g)
    unc = torch.randn(1, 77, 64, generator=g).expand(B, -1, -1).contiguous()
    with torch.no_grad():
        ec = OU.unet_forward(op, OU.TINY, lat, ts, emb)
        eu = OU.unet_forward(op, OU.TINY, lat, ts, unc)
    guided = (eu + 5.0 * (ec - eu)) if train_cfg else ec
    nxt, lp0 = dd.step(ost, guided.numpy(), ts.numpy(), lat.numpy(), noise=torch.randn(lat.shape, generator=g).numpy(), eta=1.0)
    return {"latents": lat, "next_latents": torch.from_numpy(nxt), "ts": ts, "log_probs": torch.from_numpy(lp0) + torch.tensor([2e-5, -6e-5]),
            "advantages": torch.tensor([1.3, -0.8]), "prompt_embeds": emb, "uncond_embeds": unc}


def _to_dev(batch):
    return {k: v.to(DEV) for k, v in batch.items()}


def _blended(op, seed=1):
    from oracle import unet as OU
    op2 = OU.init_params(OU.unet_param_shapes(OU.TINY), seed=seed)
    return {n: (op[n] + BLEND * (op2[n] - op[n])).contiguous() for n in op}


@pytest.mark.parametrize("datapath", ["fp32", "f16mx"])
@pytest.mark.parametrize("jit", [False, True])
def test_no_penalty_before_the_first_update(datapath, jit):
    """Reference = a copy of the policy: the inference forward of the copy and the training forward of the policy give the same bits (what
    test_sampler_ratio_is_one_before_the_first_update_tiny rests on), so kl_ref is exactly 0.0 and the gradient is the kl_coef = 0 step's, bit for bit."""
    from ddpo_amd.training.kl_reference import KLReference
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdamWConfig, train_step
    from oracle import unet as OU
    L.DATAPATH = datapath
    op = OU.init_params(OU.unet_param_shapes(OU.TINY), seed=0)
    sched, st, dd, ost = _sched()
    batch = _to_dev(_batch(op, dd, ost, True))
    unet0 = _unet(op)
    s0, info0 = train_step(AccumulatingTrainState(unet0, AdamWConfig()), batch, st, sched, True, 5.0, 1.0, 1e-4, do_opt_update=False, jit=jit)
    unet1 = _unet(op)
    ref = KLReference(unet1)
    assert ref.unet.grads is None and torch.equal(ref.params.flat, unet1.params.flat)
    s1, info1 = train_step(AccumulatingTrainState(unet1, AdamWConfig()), batch, st, sched, True, 5.0, 1.0, 1e-4, do_opt_update=False, jit=jit,
                           kl_coef=0.5, ref_unet=ref)
    assert set(info1) == set(info0) | {"kl_ref"}
    assert float(info1["kl_ref"]) == 0.0
    assert float(unet0.grads.flat.abs().max()) > 0
    assert torch.equal(unet1.grads.flat.view(torch.int32), unet0.grads.flat.view(torch.int32))
    for key in info0:
        assert torch.equal(info1[key], info0[key]), key
    assert ref.unet.grads is None


@pytest.mark.parametrize("train_cfg", [True, False])
def test_train_step_with_a_different_reference_matches_float64_autograd(train_cfg):
    from ddpo_amd.training.kl_reference import KLReference
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdamWConfig, train_step
    from oracle import unet as OU
    op = OU.init_params(OU.unet_param_shapes(OU.TINY), seed=0)
    rop = _blended(op)
    sched, st, dd, ost = _sched()
    batch = _batch(op, dd, ost, train_cfg)
    kl_coef = KL_COEF[train_cfg]
    ograds, oinfo, g_ppo, g_kl = KO.train_step_grads(op, rop, OU.TINY, dd, ost, {k: (v if k == "ts" else v.double()) for k, v in batch.items()},
                                                     5.0, 1.0, 1e-4, kl_coef, train_cfg)
    norm = lambda gs: math.sqrt(sum(float((v.double() ** 2).sum()) for v in gs.values()))
    part = norm(g_kl) / norm(g_ppo)
    print(f"oracle: |grad kl| / |grad ppo| = {part:.3f}, loss {oinfo['loss']:.6g}, kl_ref {oinfo['kl_ref']:.6g}")
    assert 0.3 < part < 3.0, part                                  # the penalty is really exercised, and so is the PPO term
    unet = _unet(op)
    ref = KLReference(unet)
    ref.params.load_dict(rop)
    state = AccumulatingTrainState(unet, AdamWConfig())
    state, info = train_step(state, _to_dev(batch), st, sched, train_cfg, 5.0, 1.0, 1e-4, do_opt_update=False, kl_coef=kl_coef, ref_unet=ref)
    assert state.n_acc == 1 and state.step == 0
    assert float(info["loss"]) == pytest.approx(oinfo["loss"], rel=1e-3, abs=1e-6)
    assert float(info["kl_ref"]) == pytest.approx(oinfo["kl_ref"], rel=1e-3)
    assert float(info["clipfrac"]) == pytest.approx(oinfo["clipfrac"], abs=1e-6)
    G = unet.grads
    gn_o = norm(ograds)
    gn = math.sqrt(float((G.flat.double() ** 2).sum()))
    assert gn == pytest.approx(gn_o, rel=1e-3)
    worst = max((_rel(G[n], ograds[n]), n) for n in ograds if float(ograds[n].abs().max()) > 1e-6 * gn_o)
    assert worst[0] < 2e-3, worst


@pytest.mark.parametrize("jit", [False, True])
def test_fused_steps_with_kl_match_separate_steps(jit):
    """k = 3 micro-steps of 2 samples, kl_coef > 0: one fused launch against three train_step calls, under the tolerances of
    tests/test_fused_micro_steps.py::test_train_steps_fused_matches_separate_train_steps."""
    from ddpo_amd.training.kl_reference import KLReference
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdamWConfig, train_step, train_steps_fused
    from oracle import unet as OU
    k = 3
    op = OU.init_params(OU.unet_param_shapes(OU.TINY), seed=4)
    rop = _blended(op, seed=6)
    sched, st, _, _ = _sched()
    g = torch.Generator().manual_seed(11)
    emb = torch.randn(B, 77, 64, generator=g).cuda()
    unc = torch.randn(1, 77, 64, generator=g).expand(B, -1, -1).contiguous().cuda()
    batches = []
    for j in range(k):
        lat = torch.randn(B, 4, HW, HW, generator=g)
        batches.append({"latents": lat.cuda(), "next_latents": (0.95 * lat + 0.1 * torch.randn(lat.shape, generator=g)).cuda(),
                        "ts": torch.tensor([[481, 21], [961, 241], [1, 701]][j], dtype=torch.int32).cuda(),
                        "log_probs": torch.tensor([-1.2, -0.9]).cuda() - 0.01 * j, "advantages": torch.tensor([0.7, -1.1]).cuda(),
                        "prompt_embeds": emb, "uncond_embeds": unc})

    def fresh():
        unet = _unet(op)
        ref = KLReference(unet)
        ref.params.load_dict(rop)
        return unet, ref, AccumulatingTrainState(unet, AdamWConfig(learning_rate=1e-3))

    unet_a, ref_a, sa = fresh()
    infos_a = []
    for j in range(k):
        sa, info = train_step(sa, batches[j], st, sched, True, 5.0, 1.0, 10.0, do_opt_update=False, jit=jit, kl_coef=0.05, ref_unet=ref_a)
        infos_a.append(info)
    unet_b, ref_b, sb = fresh()
    sb, infos_b = train_steps_fused(sb, batches, st, sched, True, 5.0, 1.0, 10.0, do_opt_update=False, jit=jit, kl_coef=0.05, ref_unet=ref_b)
    assert (sa.n_acc, sa.step) == (sb.n_acc, sb.step) == (k, 0) and len(infos_b) == k
    for ia, ib in zip(infos_a, infos_b):
        assert set(ib) == {"approx_kl", "clipfrac", "loss", "log_prob", "kl_ref"}
        for key in ("approx_kl", "clipfrac", "loss", "kl_ref"):
            assert float(ib[key]) == pytest.approx(float(ia[key]), rel=1e-5, abs=1e-7), key
        assert float(ib["kl_ref"]) > 0
        assert torch.equal(ia["log_prob"], ib["log_prob"])
    ga, gb = unet_a.grads.flat, unet_b.grads.flat
    gn = float(ga.double().norm())
    assert float((ga - gb).double().norm()) <= 2e-5 * gn, (float((ga - gb).double().norm()), gn)
    # and the penalty is in those gradients: the same steps without it differ
    unet_c, _, sc = fresh()
    sc, _ = train_steps_fused(sc, batches, st, sched, True, 5.0, 1.0, 10.0, do_opt_update=False, jit=jit)
    assert float((unet_c.grads.flat - gb).double().norm()) > 1e-3 * gn


def test_default_path_never_loads_the_binding(monkeypatch):
    """kl_coef = 0 (the default): lib_ppo_kl.load is not called, and the info dict has exactly the keys it always had."""
    from ddpo_amd import lib_ppo_kl as LK
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdamWConfig, train_step, train_steps_fused
    from oracle import unet as OU

    def boom():
        raise AssertionError("lib_ppo_kl.load() called on the default path")
    monkeypatch.setattr(LK, "load", boom)
    op = OU.init_params(OU.unet_param_shapes(OU.TINY), seed=0)
    sched, st, dd, ost = _sched()
    batch = _to_dev(_batch(op, dd, ost, True))
    state = AccumulatingTrainState(_unet(op), AdamWConfig())
    for jit in (False, True):
        state, info = train_step(state, batch, st, sched, True, 5.0, 1.0, 1e-4, do_opt_update=False, jit=jit)
        assert set(info) == {"approx_kl", "clipfrac", "loss", "log_prob"}
    state, infos = train_steps_fused(state, [batch, batch], st, sched, True, 5.0, 1.0, 1e-4, do_opt_update=False, jit=False)
    assert all(set(i) == {"approx_kl", "clipfrac", "loss", "log_prob"} for i in infos)
    with pytest.raises(ValueError, match="ref_unet"):
        train_step(state, batch, st, sched, True, 5.0, 1.0, 1e-4, do_opt_update=False, kl_coef=0.1)


def test_lora_moves_away_from_a_reference_that_stays_put():
    """lora_rank 4, learning_rate 1e-3: before the first update the adapted policy IS the pretrained one (kl_ref exactly 0), after it kl_ref > 0,
    and the reference still holds the snapshot, bit for bit."""
    from ddpo_amd.models.lora import LoraStore
    from ddpo_amd.training.kl_reference import KLReference
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdamWConfig, train_step
    from oracle import unet as OU
    op = OU.init_params(OU.unet_param_shapes(OU.TINY), seed=0)
    sched, st, dd, ost = _sched()
    batch = _to_dev(_batch(op, dd, ost, True))
    unet = _unet(op)
    ref = KLReference(unet)
    snapshot = ref.params.flat.clone()
    lora = LoraStore(unet, 4, seed=0)
    with pytest.raises(ValueError, match="before the LoraStore"):
        KLReference(unet)
    state = AccumulatingTrainState(unet, AdamWConfig(learning_rate=1e-3), lora=lora)
    state, info = train_step(state, batch, st, sched, True, 5.0, 1.0, 1e-4, do_opt_update=True, kl_coef=0.1, ref_unet=ref)
    assert state.step == 1 and float(info["kl_ref"]) == 0.0
    state, info = train_step(state, batch, st, sched, True, 5.0, 1.0, 1e-4, do_opt_update=False, kl_coef=0.1, ref_unet=ref)
    assert float(info["kl_ref"]) > 0.0 and math.isfinite(float(info["loss"]))
    assert torch.equal(ref.params.flat.view(torch.int32), snapshot.view(torch.int32))
    assert not torch.equal(unet.params.flat, snapshot)
