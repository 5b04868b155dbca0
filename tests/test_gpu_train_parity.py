"""Train-step parity of the SHIPPED datapath (lib.SHIPPED_DATAPATH — f16mx since round 4 — the default of the entrypoints and the bench;
DDPO_PARITY_DATAPATH=bf16x3 runs the full-size tests on the three-pass datapath instead) at the reference's own
`ppo_clip_range = 1e-4` (config/base.py:99) — `north_star`: fp32 rewards and grad norms within 1e-3 relative.

The batch is built the way DDPO builds it (/root/reference/pipeline/policy_gradient.py:228-305,407-441): `next_latents` is a real
DDIM transition of the policy, next = mu + sigma * z, and the stored log-prob is the sampler's own value for it (plus a few 1e-5 of
drift, well inside the clip range), so |log p| is O(1) and ratio ~ 1 as in a run.  (A transition tens of sigma away from mu makes
|log p| ~ 1e3; its fp32 rounding alone then exceeds a 1e-4 clip range on ANY datapath — that, not bf16x3, is what the round-1 test
with an arbitrary `next_latents` ran into.)

Ground truth: the CPU oracle's U-Net in float64 + torch autograd through the restated PPO loss (oracle/ppo.py, pinned to the
reference's loss closure executed in place).  Compared: loss, approx_kl, clipfrac, the global gradient norm, the gradient norm of
every top-level block of the U-Net, and the relative distance ||g - g_ref|| / ||g_ref|| over all 860 M parameters.
Every case runs the engine TWICE against that one oracle step.  "conditioned": on the transition the ORACLE drew from its own mean — the
engine's residual is then sigma z + (mu_oracle - mu_engine), so the forward's epsilon error enters dL/d(eps) and the gradient-vector figure
measures forward precision a second time.  "self-consistent": on the transition the ENGINE draws from ITS mean with the same z (sampling
forward + its own step kernel, stored log-prob = its own + drift), as a run does — both sides differentiate sigma z residuals at ratio
exp(-drift).  Same assertions on both; the backward's own error, on a shared cotangent, is tests/test_gpu_backward_budget.py's.
Sizes: tiny / tiny21 (seconds) and ONE full-size SD-1.5 step at 64x64 latents, b = 1, train_cfg (about a minute of host time)."""
import math
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ddpo_amd import lib as L
from ddpo_amd.models.unet import UNet2DCondition, UNetConfig
from ddpo_amd.diffusers_patch.scheduling_ddim import DDIMScheduler
from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdamWConfig, train_step, train_steps_fused
from oracle import ppo as OPPO, prng as OP, unet as OU
from oracle.ddim import DDIMOracle

DEV = "cuda"
CLIP = 1e-4            # the reference's ppo_clip_range
TOL = 1e-3             # north_star
SHIPPED = os.environ.get("DDPO_PARITY_DATAPATH") or L.SHIPPED_DATAPATH
# |log p - log p_oracle| budget, tighter than any north-star gate: the margin of a before-the-first-update ratio to the clip boundary is 7e-5
# (drift 3e-5 inside clip 1e-4).  bf16x3 products carry ~1e-5 relative, f16mx ~4e-5 on a U-Net forward (tests/test_gpu_f16mx_model.py).
LP_BUDGET = {"fp32": 2e-5, "bf16x3": 2e-5, "f16mx": 5e-5}


def _oracle_step(op, cfg, dd, ost, lat, ts, emb, unc, adv, drift, guidance, eta, dtype, fuse=1):
    """Oracle forward with autograd, a REAL transition sampled from it, the PPO loss on that transition, backward.
    fuse > 1: the rows are `fuse` consecutive micro-batches of b = rows / fuse samples that see the same parameters — each with its own mean
    loss, gradients summed (the reference's AccumulatingTrainState over `fuse` train_step calls without an update in between)."""
    leaves = OrderedDict((k, v.detach().clone().to(dtype).requires_grad_(True)) for k, v in op.items())
    z = OP.normal(OP.PRNGKey(123), tuple(lat.shape))
    b = lat.shape[0] // fuse
    nxt_all, old_all, infos, logps = [], [], [], []
    # one micro-batch at a time (forward, transition, loss, backward: the gradients accumulate in the leaves) — the autograd tape of ONE
    # micro-batch bounds the host memory whatever `fuse` is (16 fused micro-steps = 64 U-Net rows at 64x64 would not fit one tape)
    for j in range(fuse):
        sl = slice(j * b, (j + 1) * b)
        eps_c = OU.unet_forward(leaves, cfg, lat[sl].to(dtype), ts[sl], emb[sl].to(dtype))
        eps_u = OU.unet_forward(leaves, cfg, lat[sl].to(dtype), ts[sl], unc[sl].to(dtype))
        guided = (eps_u + guidance * (eps_c - eps_u)).detach().to(torch.float32).numpy()
        nxt, old = [], []
        for i in range(b):                              # sampling-mode step per sample (per-sample timesteps)
            n_i, lp_i = dd.step(ost, guided[i:i + 1], int(ts[sl][i]), lat[sl][i:i + 1].numpy(), noise=z[sl][i:i + 1], eta=eta)
            nxt.append(n_i); old.append(lp_i)
        mb = {"latents": lat[sl], "next_latents": torch.from_numpy(np.concatenate(nxt)), "ts": ts[sl],
              "log_probs": torch.from_numpy(np.concatenate(old)) + drift[sl], "advantages": adv[sl], "prompt_embeds": emb[sl], "uncond_embeds": unc[sl]}
        loss, info, logp = OPPO.loss_and_info_torch(dd, ost, eps_c, eps_u, mb, guidance, eta, CLIP, True, dtype)
        loss.backward()
        infos.append({k: float(v.detach()) for k, v in info.items()}); logps.append(logp.detach())
        nxt_all.append(mb["next_latents"]); old_all.append(mb["log_probs"])
        del eps_c, eps_u, loss
    batch = {"latents": lat, "next_latents": torch.cat(nxt_all), "ts": ts, "log_probs": torch.cat(old_all), "advantages": adv,
             "prompt_embeds": emb, "uncond_embeds": unc}
    grads = OrderedDict((k, v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items())
    info = {k: float(np.mean([i[k] for i in infos])) for k in infos[0]}            # per-micro-batch infos, averaged for the comparison
    return batch, grads, info, torch.cat(logps), infos, z


def _groups(named):
    out = OrderedDict()
    for n, g in named:
        out.setdefault(n.split(".")[0], []).append(g)
    return OrderedDict((k, math.sqrt(sum(float((t.double() ** 2).sum()) for t in v))) for k, v in out.items())


def _check(family, ocfg, pred, hw, b, ts, ctx_dim, T, datapath, dtype, seed, fuse=1):
    """b samples per micro-batch; fuse > 1: `fuse` micro-batches (rows = b * fuse) through ONE train_steps_fused launch."""
    old = L.DATAPATH
    L.DATAPATH = datapath
    try:
        op = OU.init_params(OU.unet_param_shapes(ocfg), seed=seed)
        unet = UNet2DCondition(UNetConfig.named(family), DEV)
        unet.params.load_dict(op)
        if datapath != "fp32":
            unet.params.pack_bf16()
        g = torch.Generator().manual_seed(100 + seed)
        n = b * fuse
        lat = torch.randn(n, 4, hw, hw, generator=g)
        emb = torch.randn(n, 77, ctx_dim, generator=g)
        unc = torch.randn(1, 77, ctx_dim, generator=g).expand(n, -1, -1).contiguous()
        ts = torch.tensor(ts, dtype=torch.int32)
        assert ts.shape[0] == n
        adv = torch.tensor(([0.7, -1.1, 0.4, -0.3, 1.3, -0.6, 0.2, -0.9] * ((n + 7) // 8))[:n])
        drift = torch.tensor(([3e-5, -2e-5, 1e-5, -3e-5] * ((n + 3) // 4))[:n])          # |log p - log p_old| stays inside the 1e-4 clip range, as before the first update
        dd = DDIMOracle(prediction_type=pred)
        ost = dd.set_timesteps(dd.create_state(), T)
        batch, ograds, oinfo, ologp, oinfos, z = _oracle_step(op, ocfg, dd, ost, lat, ts, emb, unc, adv, drift, 5.0, 1.0, dtype, fuse)
        assert oinfo["clipfrac"] == 0.0 and abs(float(ologp.abs().max())) < 20.0        # a realistic transition: |log p| is O(1)

        sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", set_alpha_to_one=False, steps_offset=1,
                              prediction_type=pred)
        st = sched.set_timesteps(sched.create_state(device=DEV), T)
        state = AccumulatingTrainState(unet, AdamWConfig())
        dbatch = {k: v.to(DEV) for k, v in batch.items()}

        def engine_pass(dbatch, kind):
            """One train_step / train_steps_fused on `dbatch` from zeroed gradients, recorded and held to the oracle's step."""
            unet.grads.flat.zero_()
            if fuse == 1:
                _, info = train_step(state, dbatch, st, sched, True, 5.0, 1.0, CLIP, do_opt_update=False, jit=False)
            else:
                _, infos = train_steps_fused(state, [{k: v[j * b:(j + 1) * b].contiguous() for k, v in dbatch.items()} for j in range(fuse)],
                                                 st, sched, True, 5.0, 1.0, CLIP, do_opt_update=False, jit=False)
                for j in range(fuse):                       # every micro-batch keeps its OWN mean loss
                    assert abs(float(infos[j]["loss"]) - oinfos[j]["loss"]) / (abs(oinfos[j]["loss"]) + 1e-30) < TOL, (j, float(infos[j]["loss"]), oinfos[j]["loss"])
                info = {k: torch.stack([torch.as_tensor(i[k], dtype=torch.float32).reshape(()) for i in infos]).mean() for k in ("approx_kl", "clipfrac", "loss")}
                info["log_prob"] = torch.cat([i["log_prob"] for i in infos])
            torch.cuda.synchronize()

            rel = lambda a, r: abs(a - r) / (abs(r) + 1e-30)
            e_loss = rel(float(info["loss"]), oinfo["loss"])
            e_lp = float((info["log_prob"].cpu().double() - ologp.double()).abs().max())
            G = unet.grads
            og, gg = _groups(ograds.items()), _groups((n, G[n]) for n in ograds)
            gn_o, gn = math.sqrt(sum(v * v for v in og.values())), math.sqrt(sum(v * v for v in gg.values()))
            err2 = OrderedDict((n, float(((G[n].cpu().double() - ograds[n].double()) ** 2).sum())) for n in ograds)
            num = sum(err2.values())
            e_dir = math.sqrt(num) / gn_o
            e_groups = {k: rel(gg[k], og[k]) for k in og}
            worst = max(e_groups, key=e_groups.get)
            # which block carries the gradient-VECTOR error: per top-level block ||g - g_ref|| / ||g_ref|| of the block and
            # its share of the squared error of the whole vector
            blk = OrderedDict()
            for n_ in ograds:
                blk[n_.split(".")[0]] = blk.get(n_.split(".")[0], 0.0) + err2[n_]
            blk_txt = "  ".join(f"{k} {math.sqrt(v) / (og[k] + 1e-300):.1e} ({100 * v / (num + 1e-300):.0f} %)" for k, v in blk.items())
            from conftest import parity_record
            parity_record(f"\n[train parity] {family} {datapath} hw={hw} b={b}{f' x {fuse} fused micro-steps' if fuse > 1 else ''} clip={CLIP}, {kind}: loss {e_loss:.2e}  log-prob abs {e_lp:.2e}  global grad-norm {rel(gn, gn_o):.2e}  "
                          f"worst block norm {worst} {e_groups[worst]:.2e}  {kind} ||g-g_ref||/||g_ref|| {e_dir:.2e}  (|g_ref| = {gn_o:.3e})\n"
                          f"    vector error by block, ||g-g_ref||/||g_ref|| (share of the squared error): {blk_txt}")
            assert float(info["clipfrac"]) == 0.0
            assert e_lp < LP_BUDGET[datapath]               # margin to the clip boundary (7e-5) is never in question
            # approx_kl = mean((log p - log p_old)^2) / 2 is QUADRATIC in differences of ~3e-5: a log-prob error e moves it by up to (|drift| e + e^2 / 2)
            # — 20 % agreement where e << drift (every three-pass case, and f16mx at SD size: e = 2e-7), bounded by the budget otherwise (the toy nets
            # under f16mx: e = 3e-5, as large as the drift itself)
            kl_slack = float(drift.abs().max()) * e_lp + 0.5 * e_lp * e_lp
            assert float(info["approx_kl"]) == pytest.approx(oinfo["approx_kl"], rel=0.2, abs=1e-10 + kl_slack)
            assert e_loss < TOL
            assert rel(gn, gn_o) < TOL
            for k, e in e_groups.items():
                assert e < TOL, (k, e)
            # the whole gradient VECTOR, not only its length.  2e-3 on the fp32-class three-pass datapaths and at full size on every datapath; the
            # toy nets under f16mx (random weights, t = 21: the worst amplifier in the suite) get 3e-3 — its attention backward carries single f16
            # terms (dO, P, dS: 2^-12 each, ddpo_attention_bwd_x16 with f16p = 1): measured 2.1e-3 there; the SD-size margins are in profiles/r04_parity_margins.log
            assert e_dir < (3 * TOL if (datapath == "f16mx" and hw < 64) else 2 * TOL)
            return info, kl_slack

        # the transition the ORACLE drew from its own mean: the engine's residual is sigma z + (mu_oracle - mu_engine), so the forward's epsilon
        # error enters dL/d(eps) ("conditioned" on the oracle's sample; the vector figure of this pass carries it)
        engine_pass(dbatch, "conditioned")

        # ... and the transition the ENGINE draws from ITS mean with the same z, as a run does ("identical prompts/seeds" in the reference,
        # pipeline/policy_gradient.py:228-305,407-441 there): the sampling forward on [lat; lat], [unc; emb], the sampler's own
        # step kernel, log_probs = its own log-prob + drift.  Both sides then differentiate sigma z residuals at ratio exp(-drift); the oracle's
        # gradients above are already the self-consistent ones.  Held to the same assertions as the first pass.
        consts = sched.kernel_consts(st, 1.0)
        z_d = torch.from_numpy(np.ascontiguousarray(z)).to(DEV)
        nxt, own = [], []
        for j in range(fuse):                           # per micro-batch slice, as the oracle does
            sl = slice(j * b, (j + 1) * b)
            lat_j, ts_j = dbatch["latents"][sl].contiguous(), dbatch["ts"][sl].contiguous()
            eps = unet.forward(torch.cat([lat_j, lat_j]), torch.cat([ts_j, ts_j]), torch.cat([dbatch["uncond_embeds"][sl], dbatch["prompt_embeds"][sl]]).contiguous())
            n_j, lp_j = L.ddim_step_fwd(eps[:b].contiguous(), eps[b:].contiguous(), lat_j, z_d[sl].contiguous(), ts_j, 5.0, consts)
            nxt.append(n_j); own.append(lp_j)
        del eps
        own = torch.cat(own)
        sbatch = dict(dbatch, next_latents=torch.cat(nxt), log_probs=own + drift.to(DEV))
        assert float((own.cpu().double() - (batch["log_probs"] - drift).double()).abs().max()) < LP_BUDGET[datapath]      # the same z: the same log-prob on both sides
        info, kl_slack = engine_pass(sbatch, "self-consistent")
        # the stored log-prob of the engine's own sample IS the scoring pass's log-prob: nothing but the drift is left in approx_kl
        assert float(info["approx_kl"]) == pytest.approx(float((drift.double() ** 2).mean()) / 2, rel=0.2, abs=1e-10 + kl_slack)
    finally:
        L.DATAPATH = old
        L.PACKED.clear()


@pytest.mark.parametrize("datapath", ["bf16x3", "fp32", "f16mx"])
@pytest.mark.parametrize("family,ocfg,pred,ctx", [("tiny", OU.TINY, "epsilon", 64), ("tiny21", OU.TINY21, "v_prediction", 96)])
def test_train_step_at_the_reference_clip_range(family, ocfg, pred, ctx, datapath, monkeypatch):
    if datapath == "f16mx":
        monkeypatch.setattr(L, "MX_MIN_K", 256)        # the toy nets have no reduction of 2560: make their 3x3 convolutions f16mx layers
    _check(family, ocfg, pred, hw=16, b=2, ts=[481, 21], ctx_dim=ctx, T=50, datapath=datapath, dtype=torch.float64, seed=3)


@pytest.mark.timeout(2400)
@pytest.mark.parametrize("fuse_default", [1, 2])
def test_train_step_sd15_full_size_shipped_datapath(fuse_default):
    """SD-1.5 train_step at 64x64 latents (512^2 px) at the REFERENCE'S micro-batch — `train.batch_size = 2` per device, train_cfg
    (/root/reference/config/base.py:61-102): 2 forwards + 2 backwards of the 860 M-parameter U-Net over a U-Net batch of 4
    on the shipped kernels (f16mx on the long reductions; 128x320 / 128x128 tiles, split-K, 4096^2 d=40 attention forward + backward,
    atomics-accumulated wgrad) against the oracle in fp32 (1e-6 of noise against the 1e-3 gates; DDPO_PARITY_F64=1: float64, twice the
    host time).  DDPO_TRAIN_PARITY_FUSE=k (default 1) runs k such micro-batches through ONE train_steps_fused launch — the shape class
    bench.py's train line times — against the oracle's k accumulated steps (k x the host time; run once per round for the record,
    profiles/r05_parity_margins.log)."""
    dtype = torch.float64 if os.environ.get("DDPO_PARITY_F64") == "1" else torch.float32
    # the suite runs the single launch AND two micro-batches through one fused launch (round 6: the driver sees the fused path at full size,
    # VERDICT r05 weak 1d); DDPO_TRAIN_PARITY_FUSE=k replaces both by k fused micro-batches (tools/r06_parity_long.sh: 16, the bench's shape)
    env_fuse = os.environ.get("DDPO_TRAIN_PARITY_FUSE")
    if env_fuse is not None and fuse_default != 1:
        pytest.skip("DDPO_TRAIN_PARITY_FUSE set: one run with that many fused micro-steps")
    fuse = int(env_fuse) if env_fuse is not None else fuse_default
    grid = [481, 21, 961, 241, 701, 121, 841, 361, 581, 61, 921, 301, 641, 181, 781, 421]          # timesteps of the 50-step grid (1 + 20 i)
    _check("sd15", OU.SD15, "epsilon", hw=64, b=2, ts=(grid * ((2 * fuse + 15) // 16))[:2 * fuse], ctx_dim=768, T=50, datapath=SHIPPED, dtype=dtype, seed=0, fuse=fuse)


@pytest.mark.timeout(1500)
def test_train_step_sd21_full_size_shipped_datapath():
    """BASELINE configs[4] (C5) at size: ONE SD-2.1 train_step at 96x96 latents (768^2 px), b = 1, train_cfg, v-prediction
    (/root/reference/ddpo/diffusers_patch/scheduling_ddim_flax.py:309-316), linear proj_in / proj_out, 1024-wide text context,
    self-attention over 9216 keys at d = 64 forward AND backward, 96x96 tile quantisation of every GEMM — same gates as the
    SD-1.5 test above (loss, per-block gradient norms < 1e-3, gradient vector < 2e-3).  The oracle runs in fp32 by default
    (1e-6 of noise against a 1e-3 gate; the 9216^2 score matrices are formed in checkpointed row blocks, oracle/unet.py);
    DDPO_PARITY_F64=1 runs it in float64 (about three times the host time)."""
    dtype = torch.float64 if os.environ.get("DDPO_PARITY_F64") == "1" else torch.float32
    _check("sd21", OU.SD21, "v_prediction", hw=96, b=1, ts=[481], ctx_dim=1024, T=50, datapath=SHIPPED, dtype=dtype, seed=0)


@pytest.mark.timeout(900)
def test_vae_sd_decode_512_matches_oracle_and_jpeg_sizes():
    """Full-size VAE decode (4x64x64 latents -> 512x512x3; generic >= 2 GiB loader, materialised 4096^2 softmax) on the bench's
    datapath vs the CPU oracle, and the reward computed from it: JPEG byte counts (reference ddpo/utils/hdf5.py:25-37) equal."""
    from ddpo_amd.models.vae import VAEDecoder, VAEConfig
    from ddpo_amd.training.callbacks import encode_jpeg
    old = L.DATAPATH
    L.DATAPATH = SHIPPED
    try:
        ovp = OU.init_params(OU.vae_decoder_param_shapes(OU.VAE_SD), seed=1)
        vae = VAEDecoder(VAEConfig.named("sd"), DEV)
        vae.params.load_dict(ovp)
        vae.params.pack_bf16(bwd=False)
        z = torch.randn(2, 4, 64, 64, generator=torch.Generator().manual_seed(8)) * 0.18215 * 4.0
        with torch.no_grad():
            ref = OU.vae_decode(ovp, OU.VAE_SD, z).numpy()
        img = vae.decode(z.to(DEV)).cpu().numpy()
        assert img.shape == ref.shape == (2, 512, 512, 3)
        err = float(np.abs(img - ref).max())
        sizes = [(len(encode_jpeg(a)), len(encode_jpeg(b))) for a, b in zip(img, ref)]
        print(f"\n[vae 512^2] max abs err {err:.2e}; jpeg bytes (engine, oracle) {sizes}; interior fraction {float(((ref > 0) & (ref < 1)).mean()):.2f}")
        assert err < 2e-4
        # The reward is the byte count / 1000.  It is integer work DOWNSTREAM of fp32 pixels: the reference's truncating
        # (x * 255).astype(uint8) flips a pixel by one LSB wherever the two decodes straddle an integer, so byte-for-byte equality is
        # not attainable from pixels that agree to 2e-5 (measured on MI355X: 34 and 25 bytes of 241 k = 1.4e-4 / 1.0e-4 relative).
        # The bar is north_star's: fp32 rewards within 1e-3 relative.
        for a, b in sizes:
            assert abs(a - b) <= 1e-3 * b, sizes
    finally:
        L.DATAPATH = old
        L.PACKED.clear()
