"""The CFG-shared front of the sampling U-Net, carried through the first self-attention.

Under classifier-free guidance the two halves of the U-Net batch carry the same latents and timestep and differ in the text context only, which
first enters at attn2 of down_blocks_0.attentions_0.  `UNet2DCondition.forward(cfg_dup=True)` runs everything in front of that point on one half.
Two kernel features keep the shared half from being copied where it meets the per-half data:
  * attention with a query batch period (`q_batches`, ddpo_attention_fwd, _x16, _images): batch b reads the queries of batch b % q_batches;
  * GEMM / conv output stage with a residual row period (`res_rows`, ddpo_gemm_desc.res_rows): output row m adds residual row m % res_rows.
Both only change WHERE an operand is read, so every comparison below is bit for bit (torch.equal) against the same entry point fed the
explicitly duplicated operand."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

from ddpo_amd import lib as L
from ddpo_amd.models import unet as U
from ddpo_amd.models.unet import UNet2DCondition, UNetConfig

DEV = "cuda"


def _same(a, b):
    if isinstance(a, L.Planes):
        return isinstance(b, L.Planes) and torch.equal(a.hi, b.hi) and torch.equal(a.lo, b.lo)
    return torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ kernel level: attention
@pytest.mark.parametrize("datapath", ["bf16x3", "f16mx", "fp32"])
@pytest.mark.parametrize("Nk", [77, 640])
@pytest.mark.parametrize("d", [40, 64, 80, 160])
def test_attention_query_batch_period_equals_duplicated_queries(d, Nk, datapath, monkeypatch):
    monkeypatch.setattr(L, "DATAPATH", datapath)
    B, heads, Nq = 4, 2, 200                         # Nq is no multiple of a query tile: the clamped last tile reads through the period too
    C = heads * d
    g = torch.Generator(device=DEV).manual_seed(100 + d + Nk)
    qh = torch.randn(B // 2 * Nq, C, device=DEV, generator=g)
    qd = torch.cat([qh, qh]).contiguous()
    k = torch.randn(B * Nk, C, device=DEV, generator=g)
    v = torch.randn(B * Nk, C, device=DEV, generator=g)
    outs = [False] + ([True] if L.attention_planes_ok(d) else [])
    ran = 0
    for po in outs:
        ref = L.attention(qd, k, v, B, heads, Nq, Nk, d, planes_out=po)
        assert _same(L.attention(qh, k, v, B, heads, Nq, Nk, d, planes_out=po, q_batches=B // 2), ref)
        assert _same(L.attention(qd, k, v, B, heads, Nq, Nk, d, planes_out=po, q_batches=B), ref)       # period B: the plain function
        ran += 1
        imgs = L.attention_kv_images(k, v, B, heads, Nk, d)
        if imgs is not None:                         # image-fed entry points (16-bit MFMA kernels only)
            ref_i = L.attention_from_images(qd, imgs, B, heads, Nq, Nk, d, planes_out=po)
            assert _same(ref_i, ref)
            assert _same(L.attention_from_images(qh, imgs, B, heads, Nq, Nk, d, planes_out=po, q_batches=B // 2), ref)
            ran += 1
    o, lse = L.attention(qh, k, v, B, heads, Nq, Nk, d, return_lse=True, q_batches=B // 2)      # lse stays per batch
    o_r, lse_r = L.attention(qd, k, v, B, heads, Nq, Nk, d, return_lse=True)
    assert torch.equal(o, o_r) and torch.equal(lse, lse_r)
    assert ran >= (1 if (datapath == "fp32" or d == 160) else 4)
    # the second half really attends to ITS keys: the halves of the output differ
    o = L.attention(qh, k, v, B, heads, Nq, Nk, d, q_batches=B // 2)
    assert not torch.equal(o[:B // 2 * Nq], o[B // 2 * Nq:])


def test_attention_strided_shared_queries(monkeypatch):
    """Queries as a column block of a wider buffer (ldq), the form the fused q / k / v projection hands over."""
    monkeypatch.setattr(L, "DATAPATH", "bf16x3")
    B, heads, Nq, Nk, d = 6, 2, 130, 77, 40
    C = heads * d
    g = torch.Generator(device=DEV).manual_seed(7)
    buf = torch.randn(B // 2 * Nq, 3 * C, device=DEV, generator=g)
    qh = buf[:, C:2 * C]
    k = torch.randn(B * Nk, C, device=DEV, generator=g)
    v = torch.randn(B * Nk, C, device=DEV, generator=g)
    ref = L.attention(torch.cat([qh, qh]).contiguous(), k, v, B, heads, Nq, Nk, d)
    assert torch.equal(L.attention(qh, k, v, B, heads, Nq, Nk, d, ldq=3 * C, q_batches=B // 2), ref)


def test_invalid_periods_are_rejected(monkeypatch):
    B, heads, Nq, Nk, d = 4, 2, 64, 77, 40
    C = heads * d
    q = torch.randn(B * Nq, C, device=DEV)
    k = torch.randn(B * Nk, C, device=DEV)
    x = torch.randn(256, 64, device=DEV)
    w = torch.randn(64, 64, device=DEV)
    res = torch.randn(256, 64, device=DEV)
    for dp in ("fp32", "bf16x3"):
        monkeypatch.setattr(L, "DATAPATH", dp)
        L.pack_weights(w, bwd=False)
        for bad in (0, 3, 5, 8, -2):                 # not a divisor of B = 4, or out of 1 .. B
            with pytest.raises(L.DdpoHipError):
                L.attention(q, k, k, B, heads, Nq, Nk, d, q_batches=bad)
        imgs = L.attention_kv_images(k, k, B, heads, Nk, d)
        if imgs is not None:
            with pytest.raises(L.DdpoHipError):
                L.attention_from_images(q, imgs, B, heads, Nq, Nk, d, q_batches=3)
        for bad in (3, 100, 512, -128):              # not a divisor of M = 256
            with pytest.raises(L.DdpoHipError):
                L.linear(x, w, residual=res, res_rows=bad)
        with pytest.raises(L.DdpoHipError):
            L.linear(x, w, res_rows=128)             # a period without a residual
        if dp != "fp32":
            with pytest.raises(L.DdpoHipError):
                L.linear(L.split_planes(x), w, residual=res, res_rows=3)       # the plane-fed entry point
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ kernel level: GEMM output stage
def _tiles(before):
    after = L.gemm_tile_launch_counts()
    return {k: after[k] - before[k] for k in after}


@pytest.mark.parametrize("datapath", ["bf16x3", "f16mx", "fp32"])
@pytest.mark.parametrize("shape", ["splitk", "tall", "rows128", "wide", "ragged"])
def test_gemm_residual_row_period_equals_duplicated_residual(shape, datapath, monkeypatch):
    """Every tile class the dispatcher can pick, the split-K reduce, a strided destination and the plane-emitting output stages."""
    monkeypatch.setattr(L, "DATAPATH", datapath)
    monkeypatch.setattr(L, "PLANES", True)
    monkeypatch.setattr(L, "PLANES_ALL", True)
    monkeypatch.setattr(L, "MX_MIN_K", 64)           # f16mx: every K % 32 == 0 layer below is an f16mx layer
    M, K, N, want = {"splitk": (512, 2048, 320, "splitk_reduce"),       # 128 x 64 tiles, reduction split in 8 + reduce pass
                     "tall": (51200, 64, 320, "tall_256x320"),          # 200 tall tiles (plane-fed, bf16x3 / f16mx)
                     "rows128": (4096, 128, 128, "t128x64"),
                     "wide": (32768, 320, 320, "wide_128x320"),
                     "ragged": (2 * 1001, 96, 96, "t128x64")}[shape]    # M, N no multiple of a tile; half the rows end inside a tile
    g = torch.Generator(device=DEV).manual_seed(len(shape) + K)
    x = torch.randn(M, K, device=DEV, generator=g)
    w = (torch.randn(K, N, device=DEV, generator=g) / K ** 0.5).contiguous()
    b = torch.randn(N, device=DEV, generator=g)
    rh = torch.randn(M // 2, N, device=DEV, generator=g)
    rd = torch.cat([rh, rh]).contiguous()
    if datapath != "fp32":
        L.pack_weights(w, bwd=False)
    srcs = [x]
    if datapath != "fp32" and L.planes_pay(w, K, M):
        srcs.append(L.split_planes(x, fmt=1 if L.planes_pay(w, K, M) == 2 else 0))
    ran = {}
    for src in srcs:
        before = L.gemm_tile_launch_counts()
        ref = L.linear(src, w, b, residual=rd)
        got = L.linear(src, w, b, residual=rh, res_rows=M // 2)
        for key, n in _tiles(before).items():
            ran[key] = ran.get(key, 0) + n
        assert torch.equal(got, ref)
        assert not torch.equal(got, L.linear(src, w, b))                 # the residual was applied ...
        # a quarter-period, against its explicit tiling
        if (M // 4) * 4 == M:
            assert torch.equal(L.linear(src, w, b, residual=rh[:M // 4].contiguous(), res_rows=M // 4),
                               L.linear(src, w, b, residual=torch.cat([rh[:M // 4]] * 4).contiguous()))
        # strided destination and strided (column-slice) residual
        big = torch.zeros(M, N + 64, device=DEV)
        rbig = torch.randn(M // 2, N + 32, device=DEV, generator=g)
        rs = rbig[:, 32:]
        L.linear(src, w, b, residual=rs, ld_res=N + 32, res_rows=M // 2, out=big[:, 64:], ld_out=N + 64)
        assert torch.equal(big[:, 64:], L.linear(src, w, b, residual=torch.cat([rs, rs]).contiguous())) and not big[:, :64].any()
        # plane-emitting output stages
        if datapath != "fp32" and L.planes_out_ok(w, K, M, N):
            for fmt in ((0, 2) if (datapath == "f16mx" and N % 32 == 0) else (0,)):
                o_b, p_b = L.linear(src, w, b, residual=rh, res_rows=M // 2, planes_out="both", planes_fmt=fmt)
                o_r, p_r = L.linear(src, w, b, residual=rd, planes_out="both", planes_fmt=fmt)
                assert torch.equal(o_b, ref) and torch.equal(o_r, ref) and _same(p_b, p_r)
                assert _same(L.linear(src, w, b, residual=rh, res_rows=M // 2, planes_out="only", planes_fmt=fmt), p_r)
    if datapath != "fp32":
        assert ran.get(want, 0) > 0, (want, ran)
        assert (ran.get("f16mx", 0) > 0) == (datapath == "f16mx" and K % 32 == 0 and K >= 64), ran


def test_conv_residual_row_period(monkeypatch):
    """The block's final residual: a 1x1 convolution (SD-1.x proj_out) and a 3x3 one, over a batch whose halves share the residual."""
    for dp in ("fp32", "bf16x3"):
        monkeypatch.setattr(L, "DATAPATH", dp)
        for ks in (1, 3):
            B, H, W, Cin, Cout = 4, 16, 16, 64, 96
            g = torch.Generator(device=DEV).manual_seed(ks)
            x = torch.randn(B * H * W, Cin, device=DEV, generator=g)
            w = (torch.randn(ks, ks, Cin, Cout, device=DEV, generator=g) / (ks * ks * Cin) ** 0.5).contiguous()
            b = torch.randn(Cout, device=DEV, generator=g)
            if dp != "fp32":
                L.pack_weights(w, bwd=False)
            rh = torch.randn(B // 2 * H * W, Cout, device=DEV, generator=g)
            ref, _, _ = L.conv2d(x, w, b, B, H, W, Cin, Cout, ks, residual=torch.cat([rh, rh]).contiguous())
            got, _, _ = L.conv2d(x, w, b, B, H, W, Cin, Cout, ks, residual=rh, res_rows=B // 2 * H * W)
            assert torch.equal(got, ref)


# ------------------------------------------------------------------------------------------------ model level
class _Spy:
    """Counts what reaches the attention and copy entry points of lib during a forward."""

    def __init__(self, monkeypatch):
        self.attn, self.img, self.copies, self.res_rows = [], [], 0, []
        ra, ri, rc, rg = L.attention, L.attention_from_images, L.copy_cols, L.gemm_conv

        def attn(q, k, v, B, heads, Nq, Nk, d, **kw):
            self.attn.append(dict(B=B, Nq=Nq, Nk=Nk, q_rows=q.shape[0], q_batches=kw.get("q_batches")))
            return ra(q, k, v, B, heads, Nq, Nk, d, **kw)

        def img(q, images, B, heads, Nq, Nk, d, **kw):
            self.img.append(dict(B=B, Nq=Nq, Nk=Nk, q_rows=q.shape[0], q_batches=kw.get("q_batches")))
            return ri(q, images, B, heads, Nq, Nk, d, **kw)

        def copy(*a, **kw):
            self.copies += 1
            return rc(*a, **kw)

        def gc(*a, **kw):
            if kw.get("res_rows"):
                self.res_rows.append((kw["M"], kw["res_rows"]))
            return rg(*a, **kw)

        monkeypatch.setattr(L, "attention", attn)
        monkeypatch.setattr(L, "attention_from_images", img)
        monkeypatch.setattr(L, "copy_cols", copy)
        monkeypatch.setattr(L, "gemm_conv", gc)


def _check_front_taken(spy, B, N, cached):
    """The first self-attention saw B / 2 batches; the first cross-attention a half-batch Q with the period; the two residuals of the block
    were read with the row period; the only copy of the step is the second half of conv_in's skip."""
    first_self = spy.attn[0]
    assert first_self["B"] == B // 2 and first_self["Nk"] == N and first_self["q_rows"] == B // 2 * N and first_self["q_batches"] is None, first_self
    cross = (spy.img if cached else spy.attn[1:])[0]
    assert cross["B"] == B and cross["q_batches"] == B // 2 and cross["q_rows"] == B // 2 * N and cross["Nk"] == 77, cross
    later = spy.attn[2 if not cached else 1:] + spy.img[1 if cached else 0:]
    assert later and all(a["B"] == B and a["q_batches"] is None for a in later)
    assert spy.res_rows == [(B * N, B // 2 * N)] * 2, spy.res_rows
    assert spy.copies == 1, spy.copies               # no `twice` on the ResBlock output: conv_in's skip half only


@pytest.mark.parametrize("family,ctx_dim,datapath", [("tiny", 64, "fp32"), ("tiny", 64, "bf16x3"), ("tiny21", 96, "bf16x3"), ("tiny", 64, "f16mx"),
                                                     ("tiny21", 96, "f16mx")])
@pytest.mark.parametrize("B", [6, 2])
def test_shared_front_is_taken_and_bit_identical(family, ctx_dim, datapath, B, monkeypatch):
    monkeypatch.setattr(L, "DATAPATH", datapath)
    if datapath == "f16mx":
        monkeypatch.setattr(L, "MX_MIN_K", 256)
    unet = UNet2DCondition(UNetConfig.named(family), DEV)
    unet.params.init_synthetic(3)
    if datapath != "fp32":
        unet.params.pack_bf16(bwd=False)
    g = torch.Generator().manual_seed(21)
    x1 = torch.randn(B // 2, 4, 16, 16, generator=g).to(DEV)
    x = torch.cat([x1, x1])
    t = torch.full((B,), 481, dtype=torch.int32, device=DEV)
    c = torch.randn(B, 77, ctx_dim, generator=g).to(DEV)
    ref = unet(x, t, c).clone()
    assert not torch.equal(ref[:B // 2], ref[B // 2:])                    # the contexts differ: so do the halves
    monkeypatch.setattr(U, "CFG_SHARED_FRONT", False)
    old = unet(x, t, c, cfg_dup=True).clone()                             # duplication behind the first ResBlock (the earlier extent)
    monkeypatch.setattr(U, "CFG_SHARED_FRONT", True)
    spy = _Spy(monkeypatch)
    new = unet(x, t, c, cfg_dup=True).clone()
    _check_front_taken(spy, B, 256, cached=False)
    assert torch.equal(new, ref) and torch.equal(old, ref)
    unet.precompute_context(c)                                            # cross-attention from the packed text-context images
    try:
        spy2 = _Spy(monkeypatch)
        cached = L.kv_images_fmt() is not None and (UNetConfig.named(family).block_out_channels[0] // UNetConfig.named(family).num_heads[0]) in (8, 16, 40, 64, 80)
        assert torch.equal(unet(x, t, c, cfg_dup=True), ref)
        _check_front_taken(spy2, B, 256, cached=cached)
        assert torch.equal(unet.forward_graphed(x, t, c, cfg_dup=True), ref)
    finally:
        unet.release_context()
        unet._graphs.clear()
    assert torch.equal(unet.forward(x, t, c, tape=[]), ref)               # the taped forward is untouched and keeps the same bits


def test_no_cross_attention_at_the_first_level_keeps_the_full_batch(monkeypatch):
    monkeypatch.setattr(L, "DATAPATH", "bf16x3")
    cfg = dataclasses.replace(UNetConfig.named("tiny"), cross_attn_down=(False, True, True, False))
    unet = UNet2DCondition(cfg, DEV)
    unet.params.init_synthetic(4)
    unet.params.pack_bf16(bwd=False)
    g = torch.Generator().manual_seed(22)
    x1 = torch.randn(2, 4, 16, 16, generator=g).to(DEV)
    x = torch.cat([x1, x1])
    t = torch.full((4,), 481, dtype=torch.int32, device=DEV)
    c = torch.randn(4, 77, 64, generator=g).to(DEV)
    ref = unet(x, t, c).clone()
    spy = _Spy(monkeypatch)
    assert torch.equal(unet(x, t, c, cfg_dup=True), ref)
    assert spy.res_rows == [] and spy.copies == 0 and all(a["B"] == 4 and a["q_batches"] is None for a in spy.attn)


def test_long_first_level_reduction_keeps_the_earlier_extent(monkeypatch):
    """The rule of DESIGN.md: where a K = block_out_channels[0] reduction is long enough for the dispatcher to consider a split-K (which follows
    the launch's row count), the half batch stops behind the first ResBlock as before."""
    monkeypatch.setattr(L, "DATAPATH", "bf16x3")
    monkeypatch.setattr(L, "splitk_min_ktiles", lambda: 1)
    unet = UNet2DCondition(UNetConfig.named("tiny"), DEV)
    unet.params.init_synthetic(5)
    unet.params.pack_bf16(bwd=False)
    g = torch.Generator().manual_seed(23)
    x1 = torch.randn(1, 4, 16, 16, generator=g).to(DEV)
    x = torch.cat([x1, x1])
    t = torch.full((2,), 481, dtype=torch.int32, device=DEV)
    c = torch.randn(2, 77, 64, generator=g).to(DEV)
    ref = unet(x, t, c).clone()
    spy = _Spy(monkeypatch)
    assert torch.equal(unet(x, t, c, cfg_dup=True), ref)
    assert spy.res_rows == [] and spy.copies == 3 and spy.attn[0]["B"] == 2


@pytest.mark.timeout(900)
def test_shared_front_at_sd15_headline_geometry(monkeypatch):
    """SD-1.5, 64x64 latents, U-Net batch 16, the shipped datapath, one forward: the path is taken (the first self-attention runs 8 batches of
    4096 queries) and the output equals the full-batch forward bit for bit."""
    monkeypatch.setattr(L, "DATAPATH", L.SHIPPED_DATAPATH)
    unet = UNet2DCondition(UNetConfig.named("sd15"), DEV)
    unet.params.init_synthetic(6)
    unet.params.pack_bf16(bwd=False)
    g = torch.Generator().manual_seed(24)
    x1 = torch.randn(8, 4, 64, 64, generator=g).to(DEV)
    x = torch.cat([x1, x1])
    t = torch.full((16,), 481, dtype=torch.int32, device=DEV)
    c = torch.randn(16, 77, 768, generator=g).to(DEV)
    ref = unet(x, t, c).clone()
    unet.precompute_context(c)
    try:
        spy = _Spy(monkeypatch)
        before = L.gemm_tile_launch_counts()
        out = unet(x, t, c, cfg_dup=True)
        ran = _tiles(before)
        _check_front_taken(spy, 16, 4096, cached=True)
        assert ran["tall_256x320"] > 0 and ran["splitk_reduce"] > 0, ran
        assert torch.equal(out, ref)
    finally:
        unet.release_context()
