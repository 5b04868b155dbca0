"""Folded nearest-2x up-sampler (lib.conv2d_up2x_folded: four 2x2 convolutions on the source grid, ddpo_conv_up2x_folded_fwd) against a float64
convolution of the up-sampled input, under the gates the project applies to the up-sampled (gather) case of each datapath:
  bf16x3 / bf16   max |err| / max |ref| < 5e-5 / 3e-2                    (tests/test_gpu_bf16.py::test_conv_bf16)
  bf16x3 also     < 2e-6 * sqrt(9 Cin) + 1e-6                            (tests/test_gpu_kernels.py::test_conv2d, the looser of the two)
  f16mx           rms err / rms conv < 3e-5, and max |out - product of the decoded planes| < 3e-6 * max |ref|
                                                                         (tests/test_gpu_f16mx.py::test_gemm_equals_the_product_of_the_decoded_planes)
The gather path's error on the same inputs is printed next to the folded one.  A folded layer whose reduction 4 Cin is below MX_MIN_K runs
bf16x3 under the f16mx datapath (the VAE-like 512-channel case) and is held to the bf16x3 gate."""
import math

import pytest
import torch

from ddpo_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {"bf16x3": 5e-5, "bf16": 3e-2}


@pytest.fixture
def datapath():
    old = L.DATAPATH
    yield
    L.DATAPATH = old
    L.PACKED.clear()


def _ref64(x, w, bias):
    """conv3x3(nearest_upsample_2x(x), pad 1) + bias in float64 on the device: nine shifted matrix products over the UP-SAMPLED image."""
    B, H, W, C = x.shape
    xu = x.double().repeat_interleave(2, 1).repeat_interleave(2, 2)
    xp = torch.nn.functional.pad(xu, (0, 0, 1, 1, 1, 1))
    acc = torch.zeros(B, 2 * H, 2 * W, w.shape[3], dtype=torch.float64, device=x.device)
    for ky in range(3):
        for kx in range(3):
            acc += xp[:, ky:ky + 2 * H, kx:kx + 2 * W] @ w[ky, kx].double()
    conv = acc.reshape(-1, w.shape[3])
    return conv + bias.double(), conv


def _maxrel(a, b):
    return float((a.double() - b).abs().max() / (b.abs().max() + 1e-30))


def _inputs(B, H, W, C, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, C, generator=g).to(DEV)
    w = (torch.randn(3, 3, C, N, generator=g) / math.sqrt(9 * C)).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    return x, w, bias


def _pack(w):
    L.pack_weights(w, bwd=False)
    assert L.pack_weights_up2x_folded(w) is not None


# the three U-Net up-samplers at their real channel counts, and a VAE-like 512-channel layer
# (and one NON-SQUARE source, so that H and W cannot be swapped anywhere — bounds test, pixel base, output row map — unnoticed)
LAYERS = [(2, 8, 8, 1280, 1280), (2, 16, 16, 1280, 1280), (2, 32, 32, 640, 640), (1, 32, 32, 512, 512), (2, 8, 16, 640, 640), (3, 12, 5, 640, 320)]


@pytest.mark.parametrize("mode", ["bf16x3", "bf16", "f16mx"])
@pytest.mark.parametrize("B,H,W,C,N", LAYERS)
@pytest.mark.parametrize("feed", ["fp32", "planes"])
def test_folded_upsampler_against_float64(datapath, mode, B, H, W, C, N, feed):
    L.DATAPATH = mode
    x, w, bias = _inputs(B, H, W, C, N, H + C + N)
    _pack(w)
    rows = B * H * W
    assert L.up2x_fold_ok(w, C, rows)
    fmt = L.up2x_planes_pay(w, C, rows)
    mxl = fmt == 2
    assert mxl == (mode == "f16mx" and 4 * C >= L.MX_MIN_K)
    xr = x.reshape(rows, C)
    src = L.split_planes(xr, fmt=fmt - 1) if feed == "planes" else xr
    out, oh, ow = L.conv2d_up2x_folded(src, w, bias, B, H, W, C, N)
    assert (oh, ow) == (2 * H, 2 * W) and out.shape == (4 * rows, N)
    gat, _, _ = L.conv2d(xr, w, bias, B, H, W, C, N, 3, upsample=True)
    ref, conv = _ref64(x, w, bias)
    e_fold, e_gather = _maxrel(out, ref), _maxrel(gat, ref)
    rms = lambda t: float((t.double() - ref).pow(2).mean().sqrt() / conv.pow(2).mean().sqrt())
    r_fold, r_gather = rms(out), rms(gat)
    print(f"{mode} {feed} {C}->{N} {H}x{W}: max-rel folded {e_fold:.3e} gather {e_gather:.3e}; rms-rel folded {r_fold:.3e} gather {r_gather:.3e}")
    if mxl:
        assert r_fold < 3e-5
    else:
        assert e_fold < TOL["bf16" if mode == "bf16" else "bf16x3"]
        if mode != "bf16":
            assert e_fold < 2e-6 * math.sqrt(9 * C) + 1e-6
    # fp32-fed and plane-fed are the same bits (the planes ARE the split the fp32 feed makes on the way in), and so is a second run
    again, _, _ = L.conv2d_up2x_folded(xr, w, bias, B, H, W, C, N)
    assert torch.equal(out, again)


def _dec_planes(p16, p8):
    rows, C = p16.shape
    h = p16.view(torch.float16).double()
    b = p8.view(torch.float8_e5m2).double().view(rows, C // 32, 2, 2, 16)
    return h, b[:, :, :, 0].reshape(rows, C), b[:, :, :, 1].reshape(rows, C) / 2048.0


def _dec_weights(w16, w8, scale, K, N):
    s = torch.pow(2.0, scale.double() - 127.0)
    h = w16.view(torch.float16).double().permute(0, 2, 1).reshape(-1, N)[:K]
    b = w8.view(torch.float8_e4m3fn).double().view(-1, N, 2, 2, 16)
    l8 = (b[:, :, :, 0].reshape(-1, N, 32) * s[None, :, None] / 2048.0).permute(0, 2, 1).reshape(-1, N)[:K]
    h8 = (b[:, :, :, 1].reshape(-1, N, 32) * s[None, :, None]).permute(0, 2, 1).reshape(-1, N)[:K]
    return h, h8, l8


def test_f16mx_folded_equals_the_product_of_the_decoded_planes(datapath):
    """The operator's contract (tests/test_gpu_f16mx.py): only fp32 accumulation error against the exact product of the DECODED operands —
    here the decoded source planes and the decoded planes of the four folded phase kernels."""
    L.DATAPATH = "f16mx"
    B, H, W, C, N = 2, 8, 8, 640, 640
    x, w, bias = _inputs(B, H, W, C, N, 5)
    _pack(w)
    rows = B * H * W
    pl = L.split_planes(x.reshape(rows, C), fmt=1)
    out, _, _ = L.conv2d_up2x_folded(pl, w, bias, B, H, W, C, N)
    m = L.PACKED[w.data_ptr()]["fold"]["mx"]
    ah, ah8, al8 = _dec_planes(pl.hi, pl.lo.view(torch.uint8).view(rows, C // 32, 64))
    ref = torch.zeros(B, 2 * H, 2 * W, N, dtype=torch.float64, device=DEV)
    pad = lambda a: torch.nn.functional.pad(a.view(B, H, W, C), (0, 0, 1, 1, 1, 1))
    for ph in range(4):
        py, px = ph >> 1, ph & 1
        wh, wh8, wl8 = (t.view(2, 2, C, N) for t in _dec_weights(m["w16"][ph], m["w8"][ph], m["scale"][ph], 4 * C, N))
        acc = 0
        for ty in range(2):
            for tx in range(2):
                oy, ox = ty + py, tx + px                     # (source offset + 1: index into the padded image)
                sl = lambda a: pad(a)[:, oy:oy + H, ox:ox + W]
                acc = acc + sl(ah) @ wh[ty, tx] + sl(ah8) @ wl8[ty, tx] + sl(al8) @ wh8[ty, tx]
        ref[:, py::2, px::2] = acc
    ref = ref.reshape(-1, N) + bias.double()
    err = float((out.double() - ref).abs().max())
    print(f"f16mx folded vs decoded planes: {err:.3e} (scale {float(ref.abs().max()):.3f})")
    assert err < 3e-6 * float(ref.abs().max())


# the stores of every output stage: the split-K reduce pass, the tall tile's two passes, the row stage of the 128 x 320, 128 x 128 and 128 x 64 tiles (unsplit)
@pytest.mark.parametrize("mode", ["bf16x3", "bf16", "f16mx"])
@pytest.mark.parametrize("B,H,W,C,N,cls,split", [(2, 16, 16, 640, 640, "wide_128x320", True), (8, 32, 32, 640, 640, "tall_256x320", False),
                                                 (8, 16, 32, 640, 640, "wide_128x320", False), (4, 64, 16, 512, 512, "t128x128", False),
                                                 (2, 32, 16, 512, 512, "t128x64", False)])
def test_strided_destination_leaves_the_neighbouring_columns_untouched(datapath, mode, B, H, W, C, N, cls, split):
    """out= / ld_out of an up block's concat buffer: the layer writes its N columns of every row and nothing else."""
    L.DATAPATH = mode
    x, w, bias = _inputs(B, H, W, C, N, 11)
    _pack(w)
    rows = B * H * W
    before = L.gemm_tile_launch_counts()
    L.conv2d_up2x_folded(x.reshape(rows, C), w, bias, B, H, W, C, N)
    after = L.gemm_tile_launch_counts()
    assert after[cls] == before[cls] + 1 and (after["splitk_reduce"] - before["splitk_reduce"] == int(split)), (before, after)
    cat = torch.full((4 * rows, N + 320), 7.25, dtype=torch.float32, device=DEV)
    dst = cat[:, :N]
    out, _, _ = L.conv2d_up2x_folded(x.reshape(rows, C), w, bias, B, H, W, C, N, out=dst, ld_out=int(cat.stride(0)))
    plain, _, _ = L.conv2d_up2x_folded(x.reshape(rows, C), w, bias, B, H, W, C, N)
    assert torch.equal(cat[:, :N], plain)
    assert bool((cat[:, N:] == 7.25).all())
    cat2 = torch.full((4 * rows, N + 320), 7.25, dtype=torch.float32, device=DEV)
    L.conv2d_up2x_folded(x.reshape(rows, C), w, bias, B, H, W, C, N, out=cat2[:, 320:], ld_out=int(cat2.stride(0)))
    assert torch.equal(cat2[:, 320:], plain) and bool((cat2[:, :320] == 7.25).all())
    ref, conv = _ref64(x, w, bias)
    e = _maxrel(plain, ref)
    r = float((plain.double() - ref).pow(2).mean().sqrt() / conv.pow(2).mean().sqrt())
    print(f"{mode} strided {cls} split={split}: max-rel {e:.3e} rms-rel {r:.3e}")
    assert (r < 3e-5) if (mode == "f16mx" and 4 * C >= L.MX_MIN_K) else (e < TOL["bf16" if mode == "bf16" else "bf16x3"])


@pytest.mark.parametrize("mode", ["bf16x3", "bf16", "f16mx"])
@pytest.mark.parametrize("B,H,W,C,N,cls", [(2, 8, 8, 1280, 1280, "splitk_reduce"), (8, 32, 32, 640, 640, "tall_256x320"),
                                           (2, 32, 32, 640, 512, "t128x128")])      # 256 tiles of 128x128 over the four phases, 80 k-tiles
def test_split_k_and_tall_tile_routes_are_taken_correct_and_deterministic(datapath, mode, B, H, W, C, N, cls):
    L.DATAPATH = mode
    x, w, bias = _inputs(B, H, W, C, N, 3)
    _pack(w)
    rows = B * H * W
    before = L.gemm_tile_launch_counts()
    out, _, _ = L.conv2d_up2x_folded(x.reshape(rows, C), w, bias, B, H, W, C, N)
    after = L.gemm_tile_launch_counts()
    assert after[cls] == before[cls] + 1, (before, after)
    ref, conv = _ref64(x, w, bias)
    e = _maxrel(out, ref)
    r = float((out.double() - ref).pow(2).mean().sqrt() / conv.pow(2).mean().sqrt())
    print(f"{mode} {cls}: max-rel {e:.3e} rms-rel {r:.3e}")
    assert (r < 3e-5) if mode == "f16mx" else (e < TOL[mode])
    again, _, _ = L.conv2d_up2x_folded(x.reshape(rows, C), w, bias, B, H, W, C, N)
    assert torch.equal(out, again)


@pytest.mark.parametrize("mode", ["bf16x3", "bf16", "f16mx"])
def test_folded_planes_equal_the_packer_applied_to_the_host_folded_kernel(datapath, mode):
    L.DATAPATH = mode
    C, N = 640, 320
    _, w, _ = _inputs(1, 2, 2, C, N, 9)
    _pack(w)
    fo = L.PACKED[w.data_ptr()]["fold"]
    wf = L.fold_up2x_kernel_reference(w.cpu()).to(DEV)             # fp32, sums ky then kx ascending
    for ph in range(4):
        k = wf[ph].reshape(4 * C, N).contiguous()
        ent = L.pack_weights(k, bwd=False)
        assert torch.equal(fo["hi"][ph], ent["fwd"][0].view_as(fo["hi"][ph])) and torch.equal(fo["lo"][ph], ent["fwd"][1].view_as(fo["lo"][ph]))
        if mode == "f16mx":
            m = L.pack_weights_f16mx(k)
            assert torch.equal(fo["mx"]["w16"][ph], m["w16"]) and torch.equal(fo["mx"]["w8"][ph], m["w8"]) and torch.equal(fo["mx"]["scale"][ph], m["scale"])
    assert ("mx" in fo) == (mode == "f16mx")


def test_repacking_the_kernel_marks_the_folded_planes_stale(datapath):
    """pack_weights(w) after a change of w without pack_weights_up2x_folded(w): the layer must not run on the OLD folded planes."""
    L.DATAPATH = "bf16x3"
    B, H, W, C, N = 1, 4, 4, 64, 64
    x, w, bias = _inputs(B, H, W, C, N, 1)
    _pack(w)
    assert L.up2x_fold_ok(w, C, B * H * W)
    w.mul_(2.0)
    L.pack_weights(w, bwd=False)
    assert not L.up2x_fold_ok(w, C, B * H * W)
    with pytest.raises(L.DdpoHipError):
        L.conv2d_up2x_folded(x.reshape(-1, C), w, bias, B, H, W, C, N)
    assert L.pack_weights_up2x_folded(w) is not None and L.up2x_fold_ok(w, C, B * H * W)
    out, _, _ = L.conv2d_up2x_folded(x.reshape(-1, C), w, bias, B, H, W, C, N)
    assert _maxrel(out, _ref64(x, w, bias)[0]) < TOL["bf16x3"]
