"""LoRA adapters on the attention projections, on the GPU: the two new kernels against float64, bit-reproducibility under graph replay,
the adapter gradients against the engine's own full-mode gradients, one optimizer update, cache coherence after a merge, and the
entry point with --lora_rank (checkpoint keys, DDPO_RESUME)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from ddpo_amd import lib as L                                           # noqa: E402
from ddpo_amd.models import lora as LO                                  # noqa: E402
from ddpo_amd.models.unet import UNet2DCondition, UNetConfig           # noqa: E402

DEV = "cuda"


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


# ------------------------------------------------------------------------------------------------ kernels
def test_lora_merge_matches_float64_one_launch():
    g = torch.Generator(device=DEV).manual_seed(0)
    shapes = [(320, 320), (640, 640), (1280, 1280), (768, 320), (1024, 640), (768, 1280), (320, 1280), (1280, 640)]
    ranks = [1, 4, 16, 64, 4, 16, 1, 64]
    layers, ref = [], []
    for (K, N), r in zip(shapes, ranks):
        w0 = torch.randn(K, N, device=DEV, generator=g) / K ** 0.5
        w = torch.empty_like(w0)
        A = torch.randn(K, r, device=DEV, generator=g) / r
        B = torch.randn(r, N, device=DEV, generator=g) * 0.01
        s = 2.0 / r
        layers.append((w0, w, A, B, s))
        ref.append(w0.double() + s * (A.double() @ B.double()))
    tab = L.lora_table(layers)
    L.lora_merge(tab)
    torch.cuda.synchronize()
    for (w0, w, A, B, s), rf in zip(layers, ref):
        assert float((w.double() - rf).abs().max() / rf.abs().max()) <= 1e-6
    for (w0, w, A, B, s) in layers:           # B = 0: W' is W0, bit for bit
        B.zero_()
        w.fill_(7.0)
    L.lora_merge(tab)
    torch.cuda.synchronize()
    assert all(torch.equal(w, w0) for (w0, w, A, B, s) in layers)


def _wgrad_ref(x, dy, A, B, s):
    x, dy, A, B = x.double(), dy.double(), A.double(), B.double()
    return s * (x.t() @ (dy @ B.t())), s * ((x @ A).t() @ dy)


@pytest.mark.parametrize("M", [1, 154, 4097, 262144])
@pytest.mark.parametrize("form", ["fp32", "planes", "planes_kblocked"])
def test_lora_wgrad_matches_float64(M, form, monkeypatch):
    K, N = (320, 320) if M == 262144 else (640, 1280)
    ranks = (4,) if M == 262144 else (1, 4, 6, 16, 64)          # 6: a partial last rank slice of 4
    g = torch.Generator(device=DEV).manual_seed(M)
    x = torch.randn(M, K, device=DEV, generator=g)
    dy = torch.randn(M, N, device=DEV, generator=g) * 1e-3
    if form == "fp32":
        xin, xv = x, x
    else:
        monkeypatch.setattr(L, "A_KBLOCKED", form == "planes_kblocked")
        xin = L.split_planes(x)
        assert xin.kblocked == (form == "planes_kblocked")
        xv = xin.float()                      # x = hi + lo: the value the forward GEMM consumed
    for r in ranks:
        A = torch.randn(K, r, device=DEV, generator=g) / r
        B = torch.randn(r, N, device=DEV, generator=g)
        s = 0.5
        dA0 = torch.randn(K, r, device=DEV, generator=g)
        dB0 = torch.randn(r, N, device=DEV, generator=g)
        ra, rb = _wgrad_ref(xv, dy, A, B, s)
        zA, zB = torch.zeros_like(dA0), torch.zeros_like(dB0)
        L.lora_wgrad(xin, dy, A, B, zA, zB, s)
        assert _rel(zA, ra) <= 1e-5 and _rel(zB, rb) <= 1e-5, (r, _rel(zA, ra), _rel(zB, rb))
        # += semantics (one fp32 rounding of the sum on top of a nonzero buffer) and bitwise reproducibility across launches
        dA, dB = dA0.clone(), dB0.clone()
        L.lora_wgrad(xin, dy, A, B, dA, dB, s)
        assert _rel(dA, dA0.double() + ra) <= 1e-6 and _rel(dB, dB0.double() + rb) <= 1e-6
        dA2, dB2 = dA0.clone(), dB0.clone()
        L.lora_wgrad(xin, dy, A, B, dA2, dB2, s)
        assert torch.equal(dA2, dA) and torch.equal(dB2, dB)


def test_lora_wgrad_bit_identical_under_graph_replay():
    M, K, N, r = 4097, 640, 640, 16
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(M, K, device=DEV, generator=g)
    dy = torch.randn(M, N, device=DEV, generator=g)
    A = torch.randn(K, r, device=DEV, generator=g)
    B = torch.randn(r, N, device=DEV, generator=g)
    dA, dB = torch.zeros(K, r, device=DEV), torch.zeros(r, N, device=DEV)
    L.lora_wgrad(x, dy, A, B, dA, dB, 1.0)
    eA, eB = dA.clone(), dB.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dA.zero_(); dB.zero_()
        L.lora_wgrad(x, dy, A, B, dA, dB, 1.0)          # warm-up on the capture stream (scratch allocation)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L.lora_wgrad(x, dy, A, B, dA, dB, 1.0)
    dA.zero_(); dB.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(dA, eA) and torch.equal(dB, eB)


def test_lora_wgrad_rejects_bad_rank():
    x = torch.zeros(4, 8, device=DEV)
    with pytest.raises(L.DdpoHipError):
        L.lora_wgrad(x, torch.zeros(4, 8, device=DEV), torch.zeros(8, 65, device=DEV), torch.zeros(65, 8, device=DEV),
                     torch.zeros(8, 65, device=DEV), torch.zeros(65, 8, device=DEV), 1.0)


# ------------------------------------------------------------------------------------------------ model
def _unet(name, seed=0, datapath="fp32"):
    L.DATAPATH = datapath
    unet = UNet2DCondition(UNetConfig.named(name), DEV)
    unet.params.init_synthetic(seed)
    if datapath != "fp32":
        unet.params.pack_bf16()
    return unet


def _batch(cfg, B=4, hw=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, hw, hw, generator=g).to(DEV)
    ts = torch.tensor([981, 741, 501, 21][:B], dtype=torch.int32).to(DEV)
    ctx = torch.randn(B, 77, cfg.cross_attention_dim, generator=g).to(DEV)
    d_out = torch.randn(B, 4, hw, hw, generator=g).to(DEV) * 1e-2
    return x, ts, ctx, d_out


def _fwd_bwd(unet, batch):
    x, ts, ctx, d_out = batch
    tape = []
    out = unet.forward(x, ts, ctx, tape=tape)
    unet.backward(tape, d_out)
    return out


def _nonzero_adapters(store, seed=5):
    g = torch.Generator().manual_seed(seed)
    for n, v in store.params.views.items():
        if n.endswith(".B"):
            v.copy_(torch.randn(v.shape, generator=g) * 0.02)


@pytest.mark.parametrize("datapath", ["fp32", L.shipped_datapath()])
def test_zero_adapter_leaves_the_sampler_bit_identical(datapath):
    from ddpo_amd.diffusers_patch.scheduling_ddim import DDIMScheduler
    from ddpo_amd.diffusers_patch.pipeline_stable_diffusion import StableDiffusionPipeline
    from oracle import prng as OP

    def run(with_lora):
        unet = _unet("tiny", datapath=datapath)
        if with_lora:
            st = LO.LoraStore(unet, 4, seed=0)
            st.merge()
        sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", set_alpha_to_one=False, steps_offset=1)
        from ddpo_amd.models.vae import VAEDecoder, VAEConfig
        vae = VAEDecoder(VAEConfig.named("tiny"), DEV)
        vae.params.init_synthetic(1)
        pipe = StableDiffusionPipeline(unet, vae, sched)
        g = torch.Generator().manual_seed(3)
        emb = torch.randn(2, 77, 64, generator=g).to(DEV)
        neg = torch.randn(1, 77, 64, generator=g).expand(2, -1, -1).contiguous().to(DEV)
        final, lat, nxt, lps, ts = pipe(emb, neg, {"unet": unet.params, "scheduler": sched.create_state(device=DEV)}, OP.PRNGKey(0), 4,
                                        height=64, width=64, guidance_scale=5.0, eta=1.0)
        return final.cpu(), lps.cpu()

    f0, l0 = run(False)
    f1, l1 = run(True)
    assert torch.equal(f0, f1) and torch.equal(l0, l1)


@pytest.mark.parametrize("name", ["tiny", "tiny21"])
@pytest.mark.parametrize("datapath", ["fp32", L.shipped_datapath()])
def test_adapter_gradients_equal_projected_full_gradients(name, datapath):
    """Same batch, same merged weights (nonzero B): dA = s G B^T, dB = s A^T G with G the engine's own full-mode gradient of W'.
    fp32: 1e-5.  Shipped datapath: G comes from the bf16x3 weight-gradient kernels (three bf16 products, the lo x lo term dropped: ~2^-16
    relative per product) while dA / dB are fp32 sums over the same operands — 1e-4 norm-relative leaves room for that and the fp32 order."""
    unet = _unet(name, datapath=datapath)
    st = LO.LoraStore(unet, 4, alpha=8, seed=1)
    _nonzero_adapters(st)
    st.merge()
    batch = _batch(unet.cfg)
    _fwd_bwd(unet, batch)                                           # LoRA mode
    assert unet.grads is None                                       # no full-size gradient buffer
    unet.lora = None
    _fwd_bwd(unet, batch)                                           # full mode, same weights
    unet.lora = st
    tol = 1e-5 if datapath == "fp32" else 1e-4
    worst = 0.0
    for n in st.targets:
        A, B, dA, dB = st.layer(n)
        G = unet.grads[n].double()
        worst = max(worst, _rel(dA, st.scale * G @ B.double().t()), _rel(dB, st.scale * A.double().t() @ G))
    assert worst <= tol, worst


def test_one_update_moves_only_the_adapters():
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdamWConfig
    from oracle.optim import AdamWBf16Mu
    unet = _unet("tiny", datapath=L.shipped_datapath())
    st = LO.LoraStore(unet, 4, seed=2)
    _nonzero_adapters(st)
    st.merge()
    tx = AdamWConfig(learning_rate=1e-3)
    state = AccumulatingTrainState(unet, tx, lora=st)
    before = unet.params.flat.clone()
    a0 = {n: v.detach().cpu().numpy().copy() for n, v in st.params.views.items()}
    _fwd_bwd(unet, _batch(unet.cfg))
    grads = {n: v.detach().cpu().numpy().copy() for n, v in st.grads.views.items()}
    state.apply_gradients(do_update=True)
    torch.cuda.synchronize()
    assert unet.grads is None and state.opt_state["mu"].numel() == st.params.flat.numel()
    # every non-adapted parameter is bit-unchanged
    for n, v in unet.params.views.items():
        o = unet.params.offsets[n]
        if n not in st.targets:
            assert torch.equal(v.reshape(-1), before[o:o + v.numel()]), n
    # the adapters follow the oracle AdamW on the adapter gradients
    names = list(a0)
    opt = AdamWBf16Mu(lr=1e-3)
    new, _, _ = opt.update([a0[n] for n in names], [grads[n] for n in names], opt.init([a0[n] for n in names]))
    for n, p in zip(names, new):
        got = st.params[n].cpu().numpy()
        assert np.abs(got - p).max() <= 1e-6 * max(1.0, np.abs(p).max()), n
    # adapted kernels equal W0 + s A' B'
    for n in st.targets:
        A, B = st.layer(n)[:2]
        ref = st.base[n].double() + st.scale * (A.double() @ B.double())
        assert float((unet.params[n].double() - ref).abs().max() / ref.abs().max()) <= 1e-6, n


def test_no_stale_caches_after_an_update():
    """After an update + merge, the sampling forward (fused q/k/v image, packed planes, cached text K/V) equals a fresh U-Net loaded with the merged
    weights and fully repacked."""
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdamWConfig
    dp = L.shipped_datapath()
    unet = _unet("tiny", datapath=dp)
    st = LO.LoraStore(unet, 4, seed=2)
    _nonzero_adapters(st)
    st.merge()
    state = AccumulatingTrainState(unet, AdamWConfig(learning_rate=1e-2), lora=st)
    x, ts, ctx, _ = _batch(unet.cfg)
    unet.precompute_context(ctx)
    unet.forward(x, ts, ctx)                                   # caches of the pre-update weights
    unet.release_context()
    _fwd_bwd(unet, _batch(unet.cfg))
    state.apply_gradients(do_update=True)
    unet.precompute_context(ctx)
    got = unet.forward(x, ts, ctx).clone()
    unet.release_context()
    fresh = UNet2DCondition(unet.cfg, DEV)
    fresh.params.flat.copy_(unet.params.flat)
    fresh.params.pack_bf16()
    fresh.precompute_context(ctx)
    want = fresh.forward(x, ts, ctx)
    fresh.release_context()
    assert torch.equal(got, want)


def test_pack_subset_equals_full_repack():
    dp = L.shipped_datapath()
    unet = _unet("tiny", datapath=dp)
    st = LO.LoraStore(unet, 4, seed=2)
    _nonzero_adapters(st)
    st.merge()                                                  # subset repack
    sub = {n: tuple(t.clone() for t in L.PACKED[unet.params[n].data_ptr()]["fwd"][:2]) for n in st.targets}
    fq = {k: v.clone() for k, v in unet.params.fused_qkv.items()}
    unet.params.pack_bf16()                                     # full repack
    for n in st.targets:
        full = L.PACKED[unet.params[n].data_ptr()]["fwd"][:2]
        assert torch.equal(sub[n][0], full[0]) and torch.equal(sub[n][1], full[1]), n
    assert all(torch.equal(fq[k], unet.params.fused_qkv[k]) for k in fq)


def test_ratio_is_one_with_a_nonzero_adapter():
    """Nonzero B, before the first update: scoring the sampled trajectory with the TRAINING forward gives the sampler's log-probs bit for bit
    (ratio == 1, approx_kl == 0) — the merged weights run the same kernels in both."""
    from ddpo_amd.diffusers_patch.scheduling_ddim import DDIMScheduler
    from ddpo_amd.diffusers_patch.pipeline_stable_diffusion import StableDiffusionPipeline
    from ddpo_amd.models.vae import VAEDecoder, VAEConfig
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdamWConfig, train_step
    from oracle import prng as OP
    unet = _unet("tiny", datapath=L.shipped_datapath())
    st_l = LO.LoraStore(unet, 4, seed=7)
    _nonzero_adapters(st_l)
    st_l.merge()
    vae = VAEDecoder(VAEConfig.named("tiny"), DEV)
    vae.params.init_synthetic(1)
    sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", set_alpha_to_one=False, steps_offset=1)
    pipe = StableDiffusionPipeline(unet, vae, sched)
    g = torch.Generator().manual_seed(9)
    emb = torch.randn(4, 77, 64, generator=g).to(DEV)
    neg = torch.randn(1, 77, 64, generator=g).expand(4, -1, -1).contiguous().to(DEV)
    final, lat, nxt, lps, ts = pipe(emb, neg, {"unet": unet.params, "scheduler": sched.create_state(device=DEV)}, OP.PRNGKey(4), 4,
                                    height=64, width=64, guidance_scale=5.0, eta=1.0)
    st = sched.set_timesteps(sched.create_state(device=DEV), 4)
    state = AccumulatingTrainState(unet, AdamWConfig(), lora=st_l)
    for step in (0, 3):
        batch = {"latents": lat[:2, step].contiguous(), "next_latents": nxt[:2, step].contiguous(), "ts": ts[:2, step].contiguous(),
                 "log_probs": lps[:2, step].contiguous(), "advantages": torch.tensor([0.5, -0.5], device=DEV), "prompt_embeds": emb[:2],
                 "uncond_embeds": neg[:2]}
        state, info = train_step(state, batch, st, sched, True, 5.0, 1.0, 1e-4, do_opt_update=False)
        assert torch.equal(info["log_prob"], lps[:2, step])
        assert float(info["approx_kl"]) == 0.0 and float(info["clipfrac"]) == 0.0
    assert float(st_l.grads.flat.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ oracle parity
def _lora_parity(family, ocfg, pred, hw, b, ts, ctx_dim, datapath, dtype, seed):
    """One LoRA train_step (train_cfg) against the CPU oracle whose adapted kernels are W0 + s * A @ B with A, B autograd LEAVES (every other
    parameter a constant): loss, the adapter gradient norm and the adapter gradient norm of every top-level block within 1e-3 (north_star)."""
    from ddpo_amd.diffusers_patch.scheduling_ddim import DDIMScheduler
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdamWConfig, train_step
    from oracle import ppo as OPPO, prng as OP, unet as OU
    from oracle.ddim import DDIMOracle
    from test_gpu_train_parity import CLIP, TOL, _groups
    L.DATAPATH = datapath
    op = OU.init_params(OU.unet_param_shapes(ocfg), seed=seed)
    unet = UNet2DCondition(UNetConfig.named(family), DEV)
    unet.params.load_dict(op)
    if datapath != "fp32":
        unet.params.pack_bf16()
    store = LO.LoraStore(unet, 4, alpha=8, seed=seed)
    _nonzero_adapters(store, seed=seed + 1)
    store.merge()
    # oracle: A, B leaves; W' = W0 + s A B built inside the graph
    leaves = {n: v.detach().cpu().to(dtype).clone().requires_grad_(True) for n, v in store.params.views.items()}
    params = {k: v.to(dtype) for k, v in op.items()}
    for n in store.targets:
        pre = n[:-len(".kernel")]
        params[n] = params[n] + store.scale * (leaves[pre + ".A"] @ leaves[pre + ".B"])
    g = torch.Generator().manual_seed(100 + seed)
    lat = torch.randn(b, 4, hw, hw, generator=g)
    emb = torch.randn(b, 77, ctx_dim, generator=g)
    unc = torch.randn(1, 77, ctx_dim, generator=g).expand(b, -1, -1).contiguous()
    ts = torch.tensor(ts, dtype=torch.int32)
    adv = torch.tensor([0.7, -1.1, 0.4, -0.3][:b])
    drift = torch.tensor([3e-5, -2e-5, 1e-5, -3e-5][:b])
    dd = DDIMOracle(prediction_type=pred)
    ost = dd.set_timesteps(dd.create_state(), 50)
    eps_c = OU.unet_forward(params, ocfg, lat.to(dtype), ts, emb.to(dtype))
    eps_u = OU.unet_forward(params, ocfg, lat.to(dtype), ts, unc.to(dtype))
    guided = (eps_u + 5.0 * (eps_c - eps_u)).detach().to(torch.float32).numpy()
    z = OP.normal(OP.PRNGKey(123), tuple(lat.shape))
    nxt, old = [], []
    for i in range(b):                                  # a REAL transition of the policy (see test_gpu_train_parity.py)
        n_i, lp_i = dd.step(ost, guided[i:i + 1], int(ts[i]), lat[i:i + 1].numpy(), noise=z[i:i + 1], eta=1.0)
        nxt.append(n_i); old.append(lp_i)
    batch = {"latents": lat, "next_latents": torch.from_numpy(np.concatenate(nxt)), "ts": ts,
             "log_probs": torch.from_numpy(np.concatenate(old)) + drift, "advantages": adv, "prompt_embeds": emb, "uncond_embeds": unc}
    loss, oinfo, _ = OPPO.loss_and_info_torch(dd, ost, eps_c, eps_u, batch, 5.0, 1.0, CLIP, True, dtype)
    loss.backward()
    ograds = {n: v.grad for n, v in leaves.items()}
    del eps_c, eps_u, loss, params
    # engine
    sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", set_alpha_to_one=False, steps_offset=1,
                          prediction_type=pred)
    st = sched.set_timesteps(sched.create_state(device=DEV), 50)
    state = AccumulatingTrainState(unet, AdamWConfig(), lora=store)
    state, info = train_step(state, {k: v.to(DEV) for k, v in batch.items()}, st, sched, True, 5.0, 1.0, CLIP, do_opt_update=False, jit=False)
    torch.cuda.synchronize()
    assert unet.grads is None
    rel = lambda a, r: abs(a - r) / (abs(r) + 1e-30)
    og, gg = _groups(ograds.items()), _groups((n, store.grads[n]) for n in ograds)
    gn_o, gn = math.sqrt(sum(v * v for v in og.values())), math.sqrt(sum(v * v for v in gg.values()))
    e_groups = {k: rel(gg[k], og[k]) for k in og}
    num = sum(float(((store.grads[n].cpu().double() - ograds[n].double()) ** 2).sum()) for n in ograds)
    e_loss = rel(float(info["loss"]), float(torch.as_tensor(oinfo["loss"]).detach()))
    from conftest import parity_record
    parity_record(f"\n[lora parity] {family} {datapath} hw={hw} b={b} r=4 s={store.scale}: loss {e_loss:.2e}  adapter grad-norm {rel(gn, gn_o):.2e}  "
                  f"worst block {max(e_groups.values()):.2e}  ||g-g_ref||/||g_ref|| {math.sqrt(num) / gn_o:.2e}  (|g_ref| = {gn_o:.3e})")
    assert float(info["clipfrac"]) == 0.0 and gn_o > 0
    assert e_loss < TOL
    assert rel(gn, gn_o) < TOL
    # per block: dA = s G B^T, dB = s A^T G exactly (test_adapter_gradients_equal_projected_full_gradients), i.e. a rank-r projection of the
    # engine's full gradient G.  The projection carries G's VECTOR error into a few dimensions, where it is no longer orthogonal to the
    # projected gradient, so a block's adapter norm inherits the vector bound the full-size step of test_gpu_train_parity.py holds G to
    # (2e-3 on the shipped datapath: 1.1-1.5e-3 per block measured there, profiles/r06_*), not the far smaller error of G's own norm.
    # fp32 datapath: 1e-3.  Measured: profiles/lora_parity.log.
    btol = TOL if datapath == "fp32" else 2 * TOL
    for k, e in e_groups.items():
        assert e < btol, (k, e)


@pytest.mark.parametrize("datapath", ["fp32", L.shipped_datapath()])
@pytest.mark.parametrize("family,pred,ctx", [("tiny", "epsilon", 64), ("tiny21", "v_prediction", 96)])
def test_lora_train_step_matches_oracle_tiny(family, pred, ctx, datapath):
    from oracle import unet as OU
    _lora_parity(family, OU.TINY if family == "tiny" else OU.TINY21, pred, hw=16, b=2, ts=[481, 21], ctx_dim=ctx, datapath=datapath,
                 dtype=torch.float64, seed=3)


@pytest.mark.timeout(2400)
def test_lora_train_step_matches_oracle_sd15_full_size():
    """SD-1.5 at 64x64 latents, b = 2, train_cfg, shipped datapath: the 64x64-level projections take plane-fed x (M = 16384 rows, K = N = 320),
    the cross-attention K = 768 text context, and the 1280-wide levels the two-column-group kernel.  Oracle in fp32 (as the full-size step of
    test_gpu_train_parity.py: ~1e-6 of noise against the 1e-3 gates)."""
    from oracle import unet as OU
    _lora_parity("sd15", OU.SD15, "epsilon", hw=64, b=2, ts=[481, 21], ctx_dim=768, datapath=L.shipped_datapath(), dtype=torch.float32, seed=0)


# ------------------------------------------------------------------------------------------------ entry point
FLAGS = ["--dataset", "compressed-animals", "--resolution", "64", "--n_inference_steps", "4", "--sample_batch_size", "2",
         "--train_batch_size", "2", "--num_train_epochs", "2", "--save_freq", "1", "--per_prompt_stats_min_count", "2",
         "--learning_rate", "1e-3", "--lora_rank", "4"]


def test_entrypoint_lora_checkpoint_and_resume(tmp_path, monkeypatch):
    monkeypatch.setenv("DDPO_MODEL_CONFIG", "tiny")
    monkeypatch.chdir(tmp_path)
    import importlib
    from safetensors.torch import load_file
    pg = importlib.import_module("pipeline.policy_gradient")
    straight = pg.main(FLAGS + ["--logbase", str(tmp_path / "a")])
    assert len(straight["mean_rewards"]) == 2 and all(np.isfinite(straight["mean_rewards"]))
    st = straight["state"]
    assert st.lora is not None and st.unet.grads is None
    info = np.load(os.path.join(straight["localpath"], "train_info/0_0_0.npy"), allow_pickle=True).item()
    assert info["approx_kl"].max() < 1e-8 and info["clipfrac"].max() == 0.0          # ratio == 1 before the first update
    ck = os.path.join(str(tmp_path / "a"), "models/pg/checkpoints")
    sd = load_file(os.path.join(ck, "lora_1.safetensors"))
    want = LO.diffusers_keys(st.unet.params.shapes, 4)
    assert list(sorted(sd)) == list(sorted(want)) and all(tuple(sd[k].shape) == want[k] for k in want)
    assert any(float(sd[k].abs().max()) > 0 for k in sd if k.endswith(".up.weight"))        # the adapters trained
    assert not os.path.exists(os.path.join(ck, "checkpoint_1.safetensors"))
    # a saved adapter can be sampled from: load_lora folds it into a fresh U-Net
    fresh = _unet("tiny", datapath=L.current_datapath())
    fresh.params.flat.copy_(st.unet.params.flat)
    for n in st.lora.targets:
        fresh.params[n].copy_(st.lora.base[n])
    LO.load_lora(fresh, os.path.join(ck, "lora_1.safetensors"))
    for n in st.lora.targets:
        assert float((fresh.params[n] - st.unet.params[n]).abs().max()) <= 1e-6 * float(st.unet.params[n].abs().max())
    # resume: run b stops after epoch 0; a resume with num_train_epochs 1 restores its bundle and trains nothing — the restored adapters, AdamW
    # moments and count must equal what run b held at the end of epoch 0, bit for bit
    one = [("1" if FLAGS[i - 1] == "--num_train_epochs" else f) for i, f in enumerate(FLAGS)]
    b0 = pg.main(one + ["--logbase", str(tmp_path / "b")])["state"]
    want = (b0.lora.params.flat.cpu(), b0.opt_state["mu"].cpu(), b0.opt_state["nu"].cpu(), b0.opt_state["count"])
    assert want[3] >= 1 and float(b0.lora.params.flat.abs().max()) > 0
    monkeypatch.setenv("DDPO_RESUME", os.path.join(str(tmp_path / "b"), "models/pg/checkpoints"))
    r0 = pg.main(one + ["--logbase", str(tmp_path / "b")])["state"]
    assert torch.equal(r0.lora.params.flat.cpu(), want[0]) and torch.equal(r0.opt_state["mu"].cpu(), want[1])
    assert torch.equal(r0.opt_state["nu"].cpu(), want[2]) and r0.opt_state["count"] == want[3] and r0.step == want[3]
    for n in r0.lora.targets:                                  # ... and merged into the U-Net's weights
        assert torch.equal(r0.unet.params[n], b0.unet.params[n]), n
    # then the second epoch from there: same prompts / noise as the uninterrupted run (epoch 0's rewards are restored from the bundle)
    resumed = pg.main(FLAGS + ["--logbase", str(tmp_path / "b")])
    assert resumed["mean_rewards"][0] == straight["mean_rewards"][0]
    # epoch 1 samples from adapters that differ by fp32 summation-order noise of the data-gradient kernels (as in test_gpu_entrypoint.py)
    assert resumed["mean_rewards"][1] == pytest.approx(straight["mean_rewards"][1], abs=0.02)
    assert resumed["state"].opt_state["count"] == st.opt_state["count"]
    # a resume with other LoRA flags, or in full mode, is refused with a clear message
    with pytest.raises(SystemExit, match="lora_rank"):
        pg.main([("8" if FLAGS[i - 1] == "--lora_rank" else f) for i, f in enumerate(FLAGS)] + ["--logbase", str(tmp_path / "b")])
    with pytest.raises(SystemExit, match="LoRA checkpoint"):
        pg.main(FLAGS[:-2] + ["--logbase", str(tmp_path / "b")])
    assert os.path.exists(os.path.join(ck, "SYNTHETIC_WEIGHTS"))
