"""`loss="d3po"` through the whole training step (ddpo_amd/training/policy_gradient.py) on the tiny U-Net, b = 2 (one pair), 8 x 8 latents — the
recipe of tests/test_gpu_kl_train_step.py: a log-ratio of exactly zero before the first update, float64 autograd with a reference that
differs, the fused step, the preference loss together with the KL penalty, and LoRA."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ddpo_amd import lib as L

import _pref_oracle as PO

DEV = "cuda"
B, HW = 2, 8
BLEND = 1e-2                      # second-seed parameters blended into the first: the reference of tests/test_gpu_kl_train_step.py
KEYS = {"pref_acc", "pref_margin", "loss"}


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


def _batch(op, dd, ost, train_cfg, seed=5, ts=(481, 21), pref=(1.0, -1.0)):
    """One pair: two trajectories of ONE prompt at two timesteps, each transition sampled by the oracle from its own (guided) prediction.
    "advantages" carries the labels; there are no stored log-probs."""
    from oracle import unet as OU
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(B, 4, HW, HW, generator=g)
    ts = torch.tensor(ts, dtype=torch.int32)
    emb = torch.randn(1, 77, 64, generator=g).expand(B, -1, -1).contiguous()
    unc = torch.randn(1, 77, 64, generator=g).expand(B, -1, -1).contiguous()
    with torch.no_grad():
        ec = OU.unet_forward(op, OU.TINY, lat, ts, emb)
        eu = OU.unet_forward(op, OU.TINY, lat, ts, unc)
    guided = (eu + 5.0 * (ec - eu)) if train_cfg else ec
    nxt, _ = dd.step(ost, guided.numpy(), ts.numpy(), lat.numpy(), noise=torch.randn(lat.shape, generator=g).numpy(), eta=1.0)
    return {"latents": lat, "next_latents": torch.from_numpy(nxt), "ts": ts, "advantages": torch.tensor(pref), "prompt_embeds": emb,
            "uncond_embeds": unc}


def _to_dev(batch):
    return {k: v.to(DEV) for k, v in batch.items()}


def _f64(batch):
    return {k: (v if k == "ts" else v.double()) for k, v in batch.items()}


def _blended(op, seed=1):
    from oracle import unet as OU
    op2 = OU.init_params(OU.unet_param_shapes(OU.TINY), seed=seed)
    return {n: (op[n] + BLEND * (op2[n] - op[n])).contiguous() for n in op}


def _oracle_h(op, rop, dd, ost, batch, train_cfg):
    """h (B,) of the float64 oracle: both networks through oracle.unet.unet_forward, no graph."""
    from oracle import unet as OU
    f = _f64(batch)
    d = lambda p: {k: v.double() for k, v in p.items()}
    with torch.no_grad():
        outs = [OU.unet_forward(d(p), OU.TINY, f["latents"], f["ts"], f[e]) for p in (op, rop) for e in ("prompt_embeds", "uncond_embeds")]
        return PO.log_ratio_rows_torch(dd, ost, outs[0], outs[1] if train_cfg else None, outs[2], outs[3] if train_cfg else None, f["latents"],
                                       f["next_latents"], f["ts"], 5.0, 1.0, train_cfg)


def _host_beta(h, s_abs=1.0):
    """beta on the host: |s| = s_abs in the float64 oracle, so q = sigmoid(-+1) is off the centre and far from saturation."""
    return s_abs / abs(float(h[0] - h[1]))


@pytest.mark.parametrize("datapath", ["fp32", "f16mx"])
@pytest.mark.parametrize("jit", [False, True])
def test_log_ratio_is_zero_before_the_first_update(datapath, jit):
    """Reference = a copy of the policy: its inference forward and the policy's training forward give the same bits, so h is exactly 0:
    pref_margin == 0.0, the loss has the bits of log1pf(1.0f) — and the gradient is there (q = 1/2, not 0)."""
    from ddpo_amd.training.kl_reference import KLReference
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdamWConfig, train_step
    from oracle import unet as OU
    L.DATAPATH = datapath
    op = OU.init_params(OU.unet_param_shapes(OU.TINY), seed=0)
    sched, st, dd, ost = _sched()
    batch = _to_dev(_batch(op, dd, ost, True))
    unet = _unet(op)
    ref = KLReference(unet)
    state, info = train_step(AccumulatingTrainState(unet, AdamWConfig()), batch, st, sched, True, 5.0, 1.0, 1e-4, do_opt_update=False, jit=jit,
                             loss="d3po", ref_unet=ref)
    assert set(info) == KEYS and state.n_acc == 1
    assert float(info["pref_margin"]) == 0.0 and float(info["pref_acc"]) == 0.0
    assert torch.equal(info["loss"].view(torch.int32), torch.log1p(torch.ones((), device=DEV)).view(torch.int32))
    g = unet.grads.flat
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert ref.unet.grads is None


@pytest.mark.parametrize("train_cfg", [True, False])
def test_train_step_with_a_different_reference_matches_float64_autograd(train_cfg):
    """Bounds as in tests/test_gpu_kl_train_step.py (the same reference, the same U-Net backward): 1e-3 on the scalars — pref_margin is a
    difference of the two rows' h, each held to 1e-3 of itself — 1e-3 on the gradient norm, 2e-3 of its maximum on every parameter tensor."""
    from ddpo_amd.training.kl_reference import KLReference
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdamWConfig, train_step
    from oracle import unet as OU
    op = OU.init_params(OU.unet_param_shapes(OU.TINY), seed=0)
    rop = _blended(op)
    sched, st, dd, ost = _sched()
    batch = _batch(op, dd, ost, train_cfg)
    h = _oracle_h(op, rop, dd, ost, batch, train_cfg)
    beta = _host_beta(h)
    ograds, oinfo = PO.train_step_grads(op, rop, OU.TINY, dd, ost, _f64(batch), 5.0, 1.0, beta, 0.0, train_cfg)
    print(f"oracle: beta {beta:.4g}, h {h.tolist()}, margin {oinfo['pref_margin']:.6g}, loss {oinfo['loss']:.6g}")
    assert abs(beta * oinfo["pref_margin"]) == pytest.approx(1.0)
    h_sum = float(h.abs().sum())
    unet = _unet(op)
    ref = KLReference(unet)
    ref.params.load_dict(rop)
    state = AccumulatingTrainState(unet, AdamWConfig())
    state, info = train_step(state, _to_dev(batch), st, sched, train_cfg, 5.0, 1.0, 1e-4, do_opt_update=False, loss="d3po", d3po_beta=beta,
                             ref_unet=ref)
    assert state.n_acc == 1 and state.step == 0 and set(info) == KEYS
    assert abs(float(info["pref_margin"]) - oinfo["pref_margin"]) < 1e-3 * h_sum
    assert abs(float(info["loss"]) - oinfo["loss"]) < beta * 1e-3 * h_sum          # |d softplus / d s| <= 1
    assert float(info["pref_acc"]) == oinfo["pref_acc"]
    G = unet.grads
    norm = lambda gs: math.sqrt(sum(float((v.double() ** 2).sum()) for v in gs.values()))
    gn_o = norm(ograds)
    gn = math.sqrt(float((G.flat.double() ** 2).sum()))
    assert gn == pytest.approx(gn_o, rel=1e-3)
    worst = max((_rel(G[n], ograds[n]), n) for n in ograds if float(ograds[n].abs().max()) > 1e-6 * gn_o)
    assert worst[0] < 2e-3, worst


def test_preference_loss_with_a_kl_penalty_matches_autograd_of_the_sum():
    """One frozen forward, the preference pass, the KL pass behind it: loss = d3po + kl_coef * kl, kl_ref reported, gradients of the sum.
    kl_coef is chosen on the host so that the two parts of the gradient have comparable norms (asserted)."""
    from ddpo_amd.training.kl_reference import KLReference
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdamWConfig, train_step
    from oracle import unet as OU
    op = OU.init_params(OU.unet_param_shapes(OU.TINY), seed=0)
    rop = _blended(op)
    sched, st, dd, ost = _sched()
    batch = _batch(op, dd, ost, True)
    beta = _host_beta(_oracle_h(op, rop, dd, ost, batch, True))
    norm = lambda gs: math.sqrt(sum(float((v.double() ** 2).sum()) for v in gs.values()))
    g_pref, _ = PO.train_step_grads(op, rop, OU.TINY, dd, ost, _f64(batch), 5.0, 1.0, beta, 0.0, True)
    g_one, _ = PO.train_step_grads(op, rop, OU.TINY, dd, ost, _f64(batch), 5.0, 1.0, beta, 1.0, True)
    kl_coef = norm(g_pref) / norm({n: g_one[n] - g_pref[n] for n in g_one})
    ograds, oinfo = PO.train_step_grads(op, rop, OU.TINY, dd, ost, _f64(batch), 5.0, 1.0, beta, kl_coef, True)
    part = norm({n: ograds[n] - g_pref[n] for n in ograds}) / norm(g_pref)
    assert part == pytest.approx(1.0, rel=1e-6) and kl_coef > 0
    unet = _unet(op)
    ref = KLReference(unet)
    ref.params.load_dict(rop)
    state = AccumulatingTrainState(unet, AdamWConfig())
    state, info = train_step(state, _to_dev(batch), st, sched, True, 5.0, 1.0, 1e-4, do_opt_update=False, loss="d3po", d3po_beta=beta,
                             kl_coef=kl_coef, ref_unet=ref)
    assert set(info) == KEYS | {"kl_ref"}
    assert float(info["kl_ref"]) == pytest.approx(oinfo["kl_ref"], rel=1e-3)
    assert float(info["loss"]) == pytest.approx(oinfo["loss"], rel=2e-3)
    gn_o = norm(ograds)
    assert math.sqrt(float((unet.grads.flat.double() ** 2).sum())) == pytest.approx(gn_o, rel=1e-3)
    worst = max((_rel(unet.grads[n], ograds[n]), n) for n in ograds if float(ograds[n].abs().max()) > 1e-6 * gn_o)
    assert worst[0] < 2e-3, worst


@pytest.mark.parametrize("jit", [False, True])
def test_fused_steps_match_separate_steps(jit):
    """k = 3 micro-steps of one pair: one fused launch against three train_step calls, under the tolerances of
    tests/test_fused_micro_steps.py::test_train_steps_fused_matches_separate_train_steps."""
    from ddpo_amd.training.kl_reference import KLReference
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdamWConfig, train_step, train_steps_fused
    from oracle import unet as OU
    k = 3
    op = OU.init_params(OU.unet_param_shapes(OU.TINY), seed=4)
    rop = _blended(op, seed=6)
    sched, st, _, _ = _sched()
    g = torch.Generator().manual_seed(11)
    emb = torch.randn(1, 77, 64, generator=g).expand(B, -1, -1).contiguous().cuda()
    unc = torch.randn(1, 77, 64, generator=g).expand(B, -1, -1).contiguous().cuda()
    batches = []
    for j in range(k):
        lat = torch.randn(B, 4, HW, HW, generator=g)
        batches.append({"latents": lat.cuda(), "next_latents": (0.95 * lat + 0.1 * torch.randn(lat.shape, generator=g)).cuda(),
                        "ts": torch.tensor([[481, 21], [961, 241], [1, 701]][j], dtype=torch.int32).cuda(),
                        "advantages": torch.tensor([[1.0, -1.0], [-1.0, 1.0], [1.0, -1.0]][j]).cuda(), "prompt_embeds": emb, "uncond_embeds": unc})

    def fresh():
        unet = _unet(op)
        ref = KLReference(unet)
        ref.params.load_dict(rop)
        return unet, ref, AccumulatingTrainState(unet, AdamWConfig(learning_rate=1e-3))

    kw = dict(loss="d3po", d3po_beta=5.0)
    unet_a, ref_a, sa = fresh()
    infos_a = []
    for j in range(k):
        sa, info = train_step(sa, batches[j], st, sched, True, 5.0, 1.0, 10.0, do_opt_update=False, jit=jit, ref_unet=ref_a, **kw)
        infos_a.append(info)
    unet_b, ref_b, sb = fresh()
    sb, infos_b = train_steps_fused(sb, batches, st, sched, True, 5.0, 1.0, 10.0, do_opt_update=False, jit=jit, ref_unet=ref_b, **kw)
    assert (sa.n_acc, sa.step) == (sb.n_acc, sb.step) == (k, 0) and len(infos_b) == k
    for ia, ib in zip(infos_a, infos_b):
        assert set(ib) == KEYS == set(ia)
        for key in KEYS:
            assert float(ib[key]) == pytest.approx(float(ia[key]), rel=1e-5, abs=1e-7), key
        assert float(ib["pref_margin"]) != 0.0
    ga, gb = unet_a.grads.flat, unet_b.grads.flat
    gn = float(ga.double().norm())
    assert gn > 0 and float((ga - gb).double().norm()) <= 2e-5 * gn, (float((ga - gb).double().norm()), gn)
    # beta is part of the captured step: another value is another gradient, not a replay of the first graph
    unet_c, ref_c, sc = fresh()
    sc, _ = train_steps_fused(sc, batches, st, sched, True, 5.0, 1.0, 10.0, do_opt_update=False, jit=jit, ref_unet=ref_c, loss="d3po", d3po_beta=10.0)
    assert float((unet_c.grads.flat - gb).double().norm()) > 1e-2 * gn
    with pytest.raises(ValueError, match="ref_unet"):
        train_step(sc, batches[0], st, sched, True, 5.0, 1.0, 10.0, do_opt_update=False, loss="d3po")


def test_lora_adapters_receive_the_gradient():
    """lora_rank 4: before the first update the adapted policy IS the pretrained one (margin exactly 0, loss log 2) and the gradient lands in
    the adapters' buffer; one update later the log-ratio has moved, and the reference still holds the snapshot."""
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
    state = AccumulatingTrainState(unet, AdamWConfig(learning_rate=1e-3), lora=lora)
    state, info = train_step(state, batch, st, sched, True, 5.0, 1.0, 1e-4, do_opt_update=False, loss="d3po", d3po_beta=50.0, ref_unet=ref)
    assert float(info["pref_margin"]) == 0.0
    g = lora.grads.flat
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    state, _ = train_step(state, batch, st, sched, True, 5.0, 1.0, 1e-4, do_opt_update=True, loss="d3po", d3po_beta=50.0, ref_unet=ref)
    assert state.step == 1
    state, info = train_step(state, batch, st, sched, True, 5.0, 1.0, 1e-4, do_opt_update=False, loss="d3po", d3po_beta=50.0, ref_unet=ref)
    assert float(info["pref_margin"]) != 0.0 and math.isfinite(float(info["loss"]))
    assert torch.equal(ref.params.flat.view(torch.int32), snapshot.view(torch.int32))
