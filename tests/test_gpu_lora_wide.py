"""LoRA on the feed-forward layers (`--lora_targets attn_ff`), on the GPU: the wide adapter-gradient kernel (csrc/lora_wide.hip) against
float64 at every size where it takes another path, bit-reproducibility under graph replay, the dispatcher between the two kernels, the
adapter gradients of a U-Net with a real-width level against the engine's own full-mode gradients, one optimizer update, cache coherence
after a merge, oracle parity of one train step, and the entry point with --lora_targets attn_ff (checkpoint keys, DDPO_RESUME)."""
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


def _wgrad_ref(x, dy, A, B, s):
    x, dy, A, B = x.double(), dy.double(), A.double(), B.double()
    return s * (x.t() @ (dy @ B.t())), s * ((x @ A).t() @ dy)


# ------------------------------------------------------------------------------------------------ kernel
# (K, N): the first sizes past each limit of the narrow kernel, the smallest real FF1 / FF2 of the wide path, a tail of a column tile on both
# sides with K no multiple of 32, and the largest real shapes (M = 154 only)
SMALL = [(2052, 320), (320, 2052), (2036, 2032), (320, 2560), (2560, 640), (2564, 644)]
LARGE = [(1280, 10240), (5120, 1280)]
SHAPES = [(K, N, M) for (K, N) in SMALL for M in (1, 17, 154)] + [(320, 2560, 4097)] + [(K, N, 154) for (K, N) in LARGE]
# x as fp32 rows, as bf16 hi / lo planes row-major, and as k-blocked planes where they exist (K % 32 == 0)
CASES = [(K, N, M, form) for (K, N, M) in SHAPES for form in ("fp32", "planes", "planes_kblocked") if form != "planes_kblocked" or K % 32 == 0]


def _check_wide(M, K, N, ranks, form, monkeypatch, fn, lddy_extra=0):
    """The bounds of test_gpu_lora.py::test_lora_wgrad_matches_float64: 1e-5 into zeroed buffers, 1e-6 for += on random buffers, bit-equal
    between two launches."""
    g = torch.Generator(device=DEV).manual_seed(M + K + N)
    x = torch.randn(M, K, device=DEV, generator=g)
    dy = (torch.randn(M, N + lddy_extra, device=DEV, generator=g) * 1e-3)[:, 4:4 + N] if lddy_extra else \
        torch.randn(M, N, device=DEV, generator=g) * 1e-3
    assert dy.stride(0) == N + lddy_extra
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
        fn(xin, dy, A, B, zA, zB, s)
        ea, eb = _rel(zA, ra), _rel(zB, rb)
        print(f"[lora wide] M={M} K={K} N={N} r={r} {form}: dA {ea:.2e} dB {eb:.2e}")
        assert ea <= 1e-5 and eb <= 1e-5, (r, ea, eb)
        dA, dB = dA0.clone(), dB0.clone()
        fn(xin, dy, A, B, dA, dB, s)
        assert _rel(dA, dA0.double() + ra) <= 1e-6 and _rel(dB, dB0.double() + rb) <= 1e-6
        dA2, dB2 = dA0.clone(), dB0.clone()
        fn(xin, dy, A, B, dA2, dB2, s)
        assert torch.equal(dA2, dA) and torch.equal(dB2, dB)


@pytest.mark.parametrize("K,N,M,form", CASES)
def test_lora_wgrad_wide_matches_float64(K, N, M, form, monkeypatch):
    from ddpo_amd import lib_lora_wide as LW
    ranks = (6, 64) if (K, N) in LARGE else (1, 4, 6, 64)          # 6: a partial last rank slice of 4
    _check_wide(M, K, N, ranks, form, monkeypatch, LW.lora_wgrad_wide)


def test_lora_wgrad_wide_takes_a_column_slice_of_dy(monkeypatch):
    from ddpo_amd import lib_lora_wide as LW
    _check_wide(154, 2564, 644, (6,), "fp32", monkeypatch, LW.lora_wgrad_wide, lddy_extra=12)


def test_lora_wgrad_wide_bit_identical_under_graph_replay():
    M, K, N, r = 4097, 320, 2560, 16
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(M, K, device=DEV, generator=g)
    dy = torch.randn(M, N, device=DEV, generator=g)
    A = torch.randn(K, r, device=DEV, generator=g)
    B = torch.randn(r, N, device=DEV, generator=g)
    dA, dB = torch.zeros(K, r, device=DEV), torch.zeros(r, N, device=DEV)
    LO.lora_wgrad(x, dy, A, B, dA, dB, 1.0)
    eA, eB = dA.clone(), dB.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dA.zero_(); dB.zero_()
        LO.lora_wgrad(x, dy, A, B, dA, dB, 1.0)          # warm-up on the capture stream (scratch allocation)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        LO.lora_wgrad(x, dy, A, B, dA, dB, 1.0)
    dA.zero_(); dB.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(dA, eA) and torch.equal(dB, eB)


def test_dispatcher_keeps_narrow_layers_on_the_old_kernel_and_refuses_bad_shapes():
    g = torch.Generator(device=DEV).manual_seed(2)
    M, K, N, r = 154, 640, 1280, 6
    x = torch.randn(M, K, device=DEV, generator=g)
    dy = torch.randn(M, N, device=DEV, generator=g) * 1e-3
    A = torch.randn(K, r, device=DEV, generator=g) / r
    B = torch.randn(r, N, device=DEV, generator=g)
    dA, dB = torch.zeros(K, r, device=DEV), torch.zeros(r, N, device=DEV)
    eA, eB = torch.zeros(K, r, device=DEV), torch.zeros(r, N, device=DEV)
    LO.lora_wgrad(x, dy, A, B, dA, dB, 0.5)
    L.lora_wgrad(x, dy, A, B, eA, eB, 0.5)
    assert torch.equal(dA, eA) and torch.equal(dB, eB) and float(dA.abs().max()) > 0
    for K, N, r in ((320, 2560, 65), (16388, 320, 4)):
        x = torch.randn(4, K, device=DEV, generator=g)
        dy = torch.randn(4, N, device=DEV, generator=g)
        A, B = torch.randn(K, r, device=DEV, generator=g), torch.randn(r, N, device=DEV, generator=g)
        dA, dB = torch.full((K, r), 3.0, device=DEV), torch.full((r, N), 5.0, device=DEV)
        with pytest.raises(L.DdpoHipError):
            LO.lora_wgrad(x, dy, A, B, dA, dB, 1.0)
        torch.cuda.synchronize()
        assert bool((dA == 3.0).all()) and bool((dB == 5.0).all())


# ------------------------------------------------------------------------------------------------ model
WIDE = UNetConfig(block_out_channels=(320, 64, 64, 64), cross_attention_dim=64)     # level 0: ff.net_0.proj (320, 2560) takes the wide kernel


def _unet(cfg, seed=0, datapath="fp32"):
    L.DATAPATH = datapath
    unet = UNet2DCondition(UNetConfig.named(cfg) if isinstance(cfg, str) else cfg, DEV)
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


def _is_ff(n):
    return ".ff." in n


@pytest.mark.parametrize("cfg", [WIDE, "tiny", "tiny21"], ids=["wide320", "tiny", "tiny21"])
@pytest.mark.parametrize("datapath", ["fp32", L.shipped_datapath()])
def test_adapter_gradients_equal_projected_full_gradients_attn_ff(cfg, datapath):
    """test_gpu_lora.py::test_adapter_gradients_equal_projected_full_gradients with targets="attn_ff": same batch, same merged weights
    (nonzero B): dA = s G B^T, dB = s A^T G with G the engine's own full-mode gradient of W'.  fp32: 1e-5.  Shipped datapath: G comes from the
    bf16x3 / f16mx weight-gradient kernels (the lo x lo term dropped: ~2^-16 relative per product) while dA / dB are fp32 sums over the same
    operands — 1e-4 norm-relative leaves room for that and the fp32 order.  wide320 is UNetConfig(block_out_channels=(320, 64, 64, 64),
    cross_attention_dim=64) at 16x16 latents, B = 4: its level-0 ff.net_0.proj (320, 2560) is outside the narrow kernel's limits; on tiny /
    tiny21 the feed-forward layers take the narrow kernel.
    Under "attn" the feed-forward adapters do not exist and the attention gradients are bit-equal to the "attn_ff" run's."""
    unet = _unet(cfg, datapath=datapath)
    st = LO.LoraStore(unet, 4, alpha=8, seed=1, targets="attn_ff")
    assert len(st.targets) == 160 and sum(_is_ff(n) for n in st.targets) == 32
    _nonzero_adapters(st)
    st.merge()
    batch = _batch(unet.cfg)
    _fwd_bwd(unet, batch)                                           # LoRA mode
    assert unet.grads is None                                       # no full-size gradient buffer
    unet.lora = None
    _fwd_bwd(unet, batch)                                           # full mode, same weights
    unet.lora = st
    tol = 1e-5 if datapath == "fp32" else 1e-4
    worst, worst_ff = 0.0, 0.0
    for n in st.targets:
        A, B, dA, dB = st.layer(n)
        G = unet.grads[n].double()
        e = max(_rel(dA, st.scale * G @ B.double().t()), _rel(dB, st.scale * A.double().t() @ G))
        worst = max(worst, e)
        if _is_ff(n):
            assert float(dA.abs().max()) > 0 and float(dB.abs().max()) > 0, n
            worst_ff = max(worst_ff, e)
    print(f"[lora attn_ff] {datapath}: worst {worst:.2e}, worst feed-forward {worst_ff:.2e}")
    assert worst <= tol, worst
    # "attn" on the same merged weights and batch: no feed-forward adapters, the attention adapter gradients bit for bit
    attn_grads = {n: tuple(t.clone() for t in st.layer(n)[2:]) for n in st.targets if not _is_ff(n)}
    merged = unet.params.flat.clone()
    unet.grads = None
    st2 = LO.LoraStore(unet, 4, alpha=8, seed=1, targets="attn")
    assert len(st2.targets) == 128 and not any(_is_ff(n) for n in st2.shapes)
    for n in st2.targets:                                           # the same adapters (seed) ...
        assert torch.equal(st2.layer(n)[0], st.layer(n)[0])
        st2.layer(n)[1].copy_(st.layer(n)[1])
    assert torch.equal(unet.params.flat, merged)                    # ... on the same weights (no merge: the feed-forward kernels stay merged)
    _fwd_bwd(unet, batch)
    for n in st2.targets:
        assert torch.equal(st2.layer(n)[2], attn_grads[n][0]) and torch.equal(st2.layer(n)[3], attn_grads[n][1]), n


def test_one_update_moves_exactly_the_adapted_kernels_and_leaves_no_stale_plane():
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdamWConfig
    unet = _unet("tiny", datapath=L.shipped_datapath())
    st = LO.LoraStore(unet, 4, seed=2, targets="attn_ff")
    _nonzero_adapters(st)
    st.merge()
    state = AccumulatingTrainState(unet, AdamWConfig(learning_rate=1e-2), lora=st)
    before = unet.params.flat.clone()
    _fwd_bwd(unet, _batch(unet.cfg))
    state.apply_gradients(do_update=True)
    torch.cuda.synchronize()
    assert unet.grads is None and state.opt_state["mu"].numel() == st.params.flat.numel()
    moved = set()
    for n, v in unet.params.views.items():
        o = unet.params.offsets[n]
        if not torch.equal(v.reshape(-1), before[o:o + v.numel()]):
            moved.add(n)
    assert moved == set(st.targets) and len(moved) == 160
    for n in st.targets:                                            # adapted kernels equal W0 + s A' B'
        A, B = st.layer(n)[:2]
        ref = st.base[n].double() + st.scale * (A.double() @ B.double())
        assert float((unet.params[n].double() - ref).abs().max() / ref.abs().max()) <= 1e-6, n
    # merge() repacked every plane the forward reads (the fused-GEGLU / f16mx planes of ff.net_0.proj among them): a forced full repack
    # changes nothing, plane for plane and in the forward's output
    x, ts, ctx, _ = _batch(unet.cfg)
    sub = {n: tuple(t.clone() for t in L.PACKED[unet.params[n].data_ptr()]["fwd"][:2]) for n in st.targets}
    unet.precompute_context(ctx)
    got = unet.forward(x, ts, ctx).clone()
    unet.release_context()
    unet.params.pack_bf16()
    for n in st.targets:
        full = L.PACKED[unet.params[n].data_ptr()]["fwd"][:2]
        assert torch.equal(sub[n][0], full[0]) and torch.equal(sub[n][1], full[1]), n
    unet.precompute_context(ctx)
    want = unet.forward(x, ts, ctx)
    unet.release_context()
    assert torch.equal(got, want)


def test_ratio_is_one_with_nonzero_feed_forward_adapters():
    """test_gpu_lora.py::test_ratio_is_one_with_a_nonzero_adapter with feed-forward adapters: the merged weights run the same kernels in the
    sampler and in the training forward, so ratio == 1 and approx_kl == 0 before the first update."""
    from ddpo_amd.diffusers_patch.scheduling_ddim import DDIMScheduler
    from ddpo_amd.diffusers_patch.pipeline_stable_diffusion import StableDiffusionPipeline
    from ddpo_amd.models.vae import VAEDecoder, VAEConfig
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdamWConfig, train_step
    from oracle import prng as OP
    unet = _unet("tiny", datapath=L.shipped_datapath())
    st_l = LO.LoraStore(unet, 4, seed=7, targets="attn_ff")
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
    ff = [n for n in st_l.shapes if _is_ff(n)]
    assert ff and all(float(st_l.grads[n].abs().max()) > 0 for n in ff)


# ------------------------------------------------------------------------------------------------ oracle parity
def _lora_parity(family, ocfg, pred, hw, b, ts, ctx_dim, datapath, dtype, seed):
    """test_gpu_lora.py::_lora_parity with targets="attn_ff": one LoRA train_step (train_cfg) against the CPU oracle whose adapted kernels are
    W0 + s * A @ B with A, B autograd LEAVES (every other parameter a constant): loss, the adapter gradient norm and the adapter gradient norm
    of every top-level block within TOL (2 TOL per block on the shipped datapath, for the reason given there)."""
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
    store = LO.LoraStore(unet, 4, alpha=8, seed=seed, targets="attn_ff")
    assert len(store.targets) == 160
    _nonzero_adapters(store, seed=seed + 1)
    store.merge()
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
    ff = [n for n in ograds if _is_ff(n)]
    ff_o = math.sqrt(sum(float((ograds[n].double() ** 2).sum()) for n in ff))
    ff_e = math.sqrt(sum(float(((store.grads[n].cpu().double() - ograds[n].double()) ** 2).sum()) for n in ff)) / ff_o
    e_loss = rel(float(info["loss"]), float(torch.as_tensor(oinfo["loss"]).detach()))
    print(f"[lora attn_ff parity] {family} {datapath}: loss {e_loss:.2e}  adapter grad-norm {rel(gn, gn_o):.2e}  worst block "
          f"{max(e_groups.values()):.2e}  feed-forward ||g-g_ref||/||g_ref|| {ff_e:.2e}")
    assert float(info["clipfrac"]) == 0.0 and gn_o > 0 and ff_o > 0
    assert e_loss < TOL
    assert rel(gn, gn_o) < TOL
    btol = TOL if datapath == "fp32" else 2 * TOL
    for k, e in e_groups.items():
        assert e < btol, (k, e)


@pytest.mark.parametrize("datapath", ["fp32", L.shipped_datapath()])
@pytest.mark.parametrize("family,pred,ctx", [("tiny", "epsilon", 64), ("tiny21", "v_prediction", 96)])
def test_lora_attn_ff_train_step_matches_oracle_tiny(family, pred, ctx, datapath):
    from oracle import unet as OU
    _lora_parity(family, OU.TINY if family == "tiny" else OU.TINY21, pred, hw=16, b=2, ts=[481, 21], ctx_dim=ctx, datapath=datapath,
                 dtype=torch.float64, seed=3)


# ------------------------------------------------------------------------------------------------ entry point
FLAGS = ["--dataset", "compressed-animals", "--resolution", "64", "--n_inference_steps", "4", "--sample_batch_size", "2",
         "--train_batch_size", "2", "--num_train_epochs", "2", "--save_freq", "1", "--per_prompt_stats_min_count", "2",
         "--learning_rate", "1e-3", "--lora_rank", "4", "--lora_targets", "attn_ff", "--kl_coef", "0.01"]


def test_entrypoint_lora_attn_ff_checkpoint_and_resume(tmp_path, monkeypatch):
    monkeypatch.setenv("DDPO_MODEL_CONFIG", "tiny")
    monkeypatch.chdir(tmp_path)
    import importlib
    from safetensors import safe_open
    from safetensors.torch import load_file
    pg = importlib.import_module("pipeline.policy_gradient")
    straight = pg.main(FLAGS + ["--logbase", str(tmp_path / "a")])
    assert len(straight["mean_rewards"]) == 2 and all(np.isfinite(straight["mean_rewards"]))
    st = straight["state"]
    assert st.lora is not None and st.lora.target_set == "attn_ff" and len(st.lora.targets) == 160 and st.unet.grads is None
    ck = os.path.join(str(tmp_path / "a"), "models/pg/checkpoints")
    path = os.path.join(ck, "lora_1.safetensors")
    sd = load_file(path)
    want = LO.diffusers_keys(st.unet.params.shapes, 4, targets="attn_ff")
    assert len(want) == 320 and list(sorted(sd)) == list(sorted(want)) and all(tuple(sd[k].shape) == want[k] for k in want)
    assert any(float(sd[k].abs().max()) > 0 for k in sd if k.endswith(".up.weight") and ".ff.net." in k)      # the FF adapters trained
    with safe_open(path, "pt") as f:
        assert f.metadata()["targets"] == "attn_ff"
    # a saved adapter can be sampled from: load_lora reads the target set from the file and folds it into a fresh U-Net
    fresh = _unet("tiny", datapath=L.current_datapath())
    fresh.params.flat.copy_(st.unet.params.flat)
    for n in st.lora.targets:
        fresh.params[n].copy_(st.lora.base[n])
    assert len(LO.load_lora(fresh, path).targets) == 160
    for n in st.lora.targets:
        assert float((fresh.params[n] - st.unet.params[n]).abs().max()) <= 1e-6 * float(st.unet.params[n].abs().max())
    # resume: run b stops after epoch 0; a resume with num_train_epochs 1 restores its bundle and trains nothing, bit for bit
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
    # a resume with the other target set is refused with a clear message
    with pytest.raises(SystemExit, match="lora_targets attn_ff; this one asks for lora_targets attn"):
        pg.main([("attn" if FLAGS[i - 1] == "--lora_targets" else f) for i, f in enumerate(FLAGS)] + ["--logbase", str(tmp_path / "b")])
