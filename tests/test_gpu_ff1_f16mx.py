"""FF1 + GEGLU as an f16mx layer (lib.pack_weights_geglu(mx=True), lib.FF1_MX): the tall 256 x 320 f16mx GEGLU instantiation
(KLoop::tall_mx_geglu: tall_mx's two-phase k-loop, tall_geglu's value / gate wave-pair output stage; ddpo_gemm_desc.epilogue = 2 on the f16mx entry
point) against the kernels that existed before it, bit for bit:
  * the 128-row f16mx GEGLU tile (epilogue = 1) on the same planes — fp32 output, emitted planes of both formats, pre-activation;
  * the plain f16mx linear on the same planes — the pre-activation; geglu(pre) is the fused output;
and against float64 next to the plain operator and bf16x3.  Where it can go wrong: the [a (160) | gate (160)] column order, the first / last k-tile of
the two-phase loop (K = 32: one k-tile; K = 64: two), a ragged last row tile (M = 6500), each of the three outputs, the tile choice.  Every shape
is the smallest at which geglu_tall_pays holds: ceil(M / 256) * N / 320 >= 200."""
import math

import pytest
import torch
import torch.nn.functional as TF

from ddpo_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _f16mx():
    old = L.DATAPATH
    L.DATAPATH = "f16mx"
    yield
    L.DATAPATH = old
    L.PACKED.clear()


def _layer(M, K, F):
    """LayerNorm output y (fp32), its f16mx planes as LayerNorm emits them, FF1 weight / bias registered as an f16mx GEGLU layer."""
    g = torch.Generator().manual_seed(M + K + F)
    x0 = (torch.randn(M, K, generator=g) * 3 + 0.5).to(DEV)
    gamma, beta = torch.randn(K, generator=g).to(DEV), torch.randn(K, generator=g).to(DEV)
    w = (torch.randn(K, 2 * F, generator=g) / math.sqrt(K)).to(DEV)
    b = torch.randn(2 * F, generator=g).to(DEV)
    y = L.layernorm(x0, gamma, beta)
    pl = L.layernorm(x0, gamma, beta, planes=2)
    sp = L.split_planes(y, fmt=1)
    assert pl.fmt == 1 and torch.equal(pl.hi, sp.hi) and torch.equal(pl.lo, sp.lo)          # the training forward's operand is the sampler's
    L.pack_weights(w, bwd=False)
    assert L.pack_weights_geglu(w, b, mx=True)
    return y, pl, sp, w, b


def _rms_err(out, ref, ref_centered):
    """tests/test_gpu_f16mx.py's datapath metric: rms error over the rms of the reference without its additive terms."""
    return float((out.double() - ref).pow(2).mean().sqrt() / ref_centered.pow(2).mean().sqrt())


SHAPES = [(6400, 32, 1280), (6400, 320, 1280), (6500, 64, 1280), (25600, 1280, 320)]


@pytest.mark.parametrize("M,K,F", SHAPES)
def test_tall_f16mx_geglu_equals_the_128_row_tile_the_plain_operator_and_float64(M, K, F, monkeypatch):
    y, pl, sp, w, b = _layer(M, K, F)
    N = 2 * F
    assert -(-M // 256) * (N // 320) >= 200
    assert L.geglu_mx_layer(w) and L.geglu_tall_pays(w, M) and not L.mx_layer(w)

    def run(p):
        c0 = L.gemm_tile_launch_counts()
        o = L.linear_geglu(p, w)
        p0 = L.linear_geglu(p, w, planes_out=1)
        p1 = L.linear_geglu(p, w, planes_out=2)
        o2, pre = L.linear_geglu(p, w, pre_out=True)
        c1 = L.gemm_tile_launch_counts()
        return (o, p0, p1, o2, pre), {k: c1[k] - c0[k] for k in c1}

    (tall, tall_p0, tall_p1, tall2, tall_pre), cnt = run(pl)
    assert cnt["tall_256x320"] == 4 and cnt["f16mx"] == 4 and cnt["t128x128"] == 0
    assert torch.equal(L.linear_geglu(y, w), tall)             # fp32 in (the training forward): split on the way in, the same tile, the same bits
    assert torch.equal(L.linear_geglu(sp, w), tall)
    assert tall_p0.fmt == 0 and tall_p1.fmt == 1
    # --- the 128-row f16mx GEGLU tile on the same planes (the tall route switched off)
    monkeypatch.setattr(L, "GEGLU_TALL", False)
    assert not L.geglu_tall_pays(w, M)
    (ref, ref_p0, ref_p1, ref2, ref_pre), cnt = run(pl)
    assert cnt["tall_256x320"] == 0 and cnt["f16mx"] == 4 and cnt["t128x128"] == 4
    monkeypatch.setattr(L, "GEGLU_TALL", True)
    assert torch.equal(tall, ref) and torch.equal(tall2, ref) and torch.equal(ref2, ref)
    assert torch.equal(tall_pre, ref_pre)
    for a_, r_ in ((tall_p0, ref_p0), (tall_p1, ref_p1)):
        assert torch.equal(a_.hi, r_.hi) and torch.equal(a_.lo, r_.lo)
    s0, s1 = L.split_planes(tall), L.split_planes(tall, fmt=1)                  # the emitted planes are the split of the fp32 result
    assert torch.equal(tall_p0.hi, s0.hi) and torch.equal(tall_p0.lo, s0.lo) and torch.equal(tall_p1.hi, s1.hi) and torch.equal(tall_p1.lo, s1.lo)
    # --- the plain f16mx operator on the same planes: the pre-activation in w's own column order
    monkeypatch.setattr(L, "MX_MIN_K", 32)
    w2 = w.clone()
    L.pack_weights(w2, bwd=False)
    assert L.mx_layer(w2)
    plain = L.linear(pl, w2, b)
    monkeypatch.setattr(L, "MX_MIN_K", 2560)
    assert tall_pre.shape == (M, N) and torch.equal(tall_pre, plain)
    assert torch.equal(L.geglu(tall_pre), tall)
    # --- float64: x @ w + b, then GEGLU
    f64 = y.double() @ w.double() + b.double()
    ref64 = f64[:, :F] * TF.gelu(f64[:, F:], approximate="tanh")
    e_plain = _rms_err(plain, f64, f64 - b.double())
    e_gate = _rms_err(L.geglu(plain), ref64, ref64)            # the plain operator's result through the same fp32 GEGLU
    e_fused = _rms_err(tall, ref64, ref64)
    with L.datapath("bf16x3"):
        e3_plain = _rms_err(L.linear(y, w2, b), f64, f64 - b.double())
        e3_fused = _rms_err(L.linear_geglu(y, w), ref64, ref64)
    print(f"\n[FF1 f16mx M={M} K={K} F={F}] rms err vs float64: plain linear {e_plain:.2e}, geglu(plain) {e_gate:.2e}, fused tall {e_fused:.2e}"
          f"  (bf16x3: plain {e3_plain:.2e}, fused {e3_fused:.2e})")
    assert e_plain < 3e-5                                       # the operator's own contract (tests/test_gpu_f16mx.py)
    assert e_fused <= e_gate + 2.0 ** -24                       # not worse than the plain operator by more than the fp32 rounding of a * gelu(g)
    # first-order propagation through a * gelu(g) with independent errors in a and g: <= (|gelu| + |a gelu'|) eps, gelu' <= 1.13 — within 2x the plain bound
    assert e_fused < 2 * 3e-5


def test_refusals_and_the_unregistered_route(monkeypatch):
    M, K, F = 6400, 64, 1280
    y, pl, sp, w, b = _layer(M, K, F)
    N = 2 * F
    t = L.PACKED[w.data_ptr()]["geglu"]["tall"]
    out = torch.empty(M, F, dtype=torch.float32, device=DEV)
    desc = lambda: L._gemm_desc(M, N, K, src=pl, ld_src=K, out=out, ld_out=F, bias=t["bias"], epilogue=2)
    L._launch_fwd(desc(), pl, t["mx"], cross=True)             # the descriptor itself is good: with the cross terms it launches ...
    assert torch.equal(out, L.linear_geglu(pl, w))
    with pytest.raises(L.DdpoHipError, match="invalid argument"):
        L._launch_fwd(desc(), pl, t["mx"], cross=False)        # ... without them (npass 5) the tall GEGLU tile does not exist
    with pytest.raises(L.DdpoHipError, match="plane-fed linear_geglu needs"):
        L.linear_geglu(L.split_planes(y), w)                   # bf16 planes handed to a registered FF1
    # registered WITHOUT the keyword: not an f16mx layer — exactly the bf16x3 route, whatever the feed; f16mx planes are refused
    L.pack_weights(w, bwd=False)
    assert L.pack_weights_geglu(w, b)
    g = L.PACKED[w.data_ptr()]["geglu"]
    assert not L.geglu_mx_layer(w) and "mx" not in g and "mx" not in g["tall"] and "hi" in g["tall"]
    c0 = L.gemm_tile_launch_counts()
    o_fp32, o_pl = L.linear_geglu(y, w), L.linear_geglu(L.split_planes(y), w)
    c1 = L.gemm_tile_launch_counts()
    assert c1["f16mx"] == c0["f16mx"] and c1["tall_256x320"] - c0["tall_256x320"] == 1
    with L.datapath("bf16x3"):
        o3 = L.linear_geglu(y, w)
    assert torch.equal(o_fp32, o3) and torch.equal(o_pl, o3)
    with pytest.raises(L.DdpoHipError, match="plane-fed linear_geglu needs"):
        L.linear_geglu(pl, w)
    # the switches: DDPO_FF1_MX=0 and DDPO_MX_CROSS=0 both leave a registered FF1 on the bf16x3 route
    for name in ("FF1_MX", "MX_CROSS"):
        monkeypatch.setattr(L, name, False)
        L.pack_weights(w, bwd=False)
        assert L.pack_weights_geglu(w, b, mx=True) and not L.geglu_mx_layer(w)
        assert torch.equal(L.linear_geglu(L.split_planes(y), w), o3)
        monkeypatch.setattr(L, name, True)


def test_tiny_unet_sampler_equals_taped_forward_and_the_switch_restores_the_bf16x3_ff1(monkeypatch):
    from ddpo_amd.models.unet import UNet2DCondition, UNetConfig
    from oracle import unet as OU
    monkeypatch.setattr(L, "MX_MIN_K", 256)        # as tests/test_gpu_f16mx_model.py: the tiny architecture's 3x3 convolutions and lower FF2s become f16mx layers
    op = OU.init_params(OU.unet_param_shapes(OU.TINY), seed=0)
    unet = UNet2DCondition(UNetConfig.named("tiny"), DEV)
    unet.params.load_dict(op)
    unet.params.pack_bf16()
    ff1 = [v for n, v in unet.params.views.items() if n.endswith(".ff.net_0.proj.kernel")]
    assert ff1 and all(L.geglu_mx_layer(v) and v.shape[0] < L.MX_MIN_K for v in ff1)          # f16mx through the registration, not through MX_MIN_K
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(4, 4, 8, 8, generator=g).to(DEV)
    ts = torch.tensor([481, 21, 981, 241], dtype=torch.int32).to(DEV)
    emb = torch.randn(4, 77, 64, generator=g).to(DEV)
    c0 = L.gemm_tile_launch_counts()["f16mx"]
    out = unet(lat, ts, emb)
    n_mx = L.gemm_tile_launch_counts()["f16mx"] - c0
    tape = []
    out_t = unet.forward(lat[:2].contiguous(), ts[:2].contiguous(), emb[:2].contiguous(), tape=tape)
    assert torch.equal(out_t, out[:2])             # training forward (fp32 LN3, split on the way in) == sampler (LN3 emits f16mx planes)
    # DDPO_FF1_MX=0: FF1 is registered as before this route existed — every FF1 launch leaves the f16mx kernel, nothing else moves
    monkeypatch.setattr(L, "FF1_MX", False)
    unet.params.pack_bf16()
    assert not any(L.geglu_mx_layer(v) for v in ff1)
    c0 = L.gemm_tile_launch_counts()["f16mx"]
    out_off = unet(lat, ts, emb)
    assert n_mx - (L.gemm_tile_launch_counts()["f16mx"] - c0) == len(ff1)
    assert not torch.equal(out_off, out) and float((out_off - out).abs().max() / out.abs().max()) < 3e-4
    tape = []
    assert torch.equal(unet.forward(lat[:2].contiguous(), ts[:2].contiguous(), emb[:2].contiguous(), tape=tape), out_off[:2])
    ref = OU.unet_forward({k: v.double() for k, v in op.items()}, OU.TINY, lat.cpu().double(), ts.cpu(), emb.cpu().double())
    rel = lambda a: float((a.detach().cpu().double() - torch.as_tensor(ref)).abs().max() / torch.as_tensor(ref).abs().max())
    print(f"\n[tiny U-Net forward, f16mx] max rel err vs float64: FF1 f16mx {rel(out):.2e}, DDPO_FF1_MX=0 {rel(out_off):.2e}")
    assert rel(out) < 3e-4                         # tests/test_gpu_f16mx_model.py's bound for this forward
