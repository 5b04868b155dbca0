"""The U-Net backward's OWN error: engine and oracle receive the same dL/d(output), so nothing of the forward's precision enters.

tests/test_gpu_train_parity.py hands the engine a transition built from the ORACLE's mean: the engine's residual is then
sigma z + (mu_oracle - mu_engine), the forward's epsilon error enters dL/d(eps) before any backward kernel runs, and its gradient-vector
figure sits on a floor of about 1e-3 that the test itself creates.  Here the cotangent is an input:

  engine:  tape = []; out = unet.forward(lat2, ts2, ctx2, tape=tape); unet.backward(tape, d_out); unet.grads[name]
  oracle:  oracle.unet.unet_forward on leaves with requires_grad; out.backward(d_out)

with the rows laid out as train_step lays them out (lat2 = [lat; lat], ts2 = [ts; ts], ctx2 = [uncond; prompt]).  What is left is the
arithmetic of dgrad, wgrad, the norm / activation / attention backward kernels and the Python orchestration around them
(UNet2DCondition.backward, resnet_backward, _transformer_backward, _attention_backward: skip gradients, dx_add chains, the time path).

Compared, all as ||g - g_ref|| / ||g_ref|| in float64 (never max over max): the whole vector, every top-level block, and every
parameter tensor — a tensor whose reference norm is under 1e-3 of the whole vector's (true gradients that cancel: conv1.bias and
time_emb_proj.* in front of one-channel GroupNorm groups) is bounded by gate * 1e-3 * ||g_ref, whole|| instead, so nothing is skipped.

Gates — none taken from the code under test:
  fp32    the oracle itself in float32 against float64 on these inputs is the yardstick (tiny 2.10e-6 / 2.5e-6 / 3.9e-6 for vector /
          worst block / worst tensor, tiny21 2.44e-6 / 3.6e-6 / 6.2e-6); the engine gets 8 x that, as tests/test_gpu_kernel_branches.py
          gives its fp32 kernels (another summation order: split-K, atomics in wgrad and dgamma; the device's exp, rsqrt, div at a few
          ulp each): 2e-5 / 3e-5 / 5e-5.  test_fp32_yardstick_of_the_oracle (no GPU) recomputes the yardstick and holds it inside a
          quarter of each gate.
  bf16x3  2e-4 everywhere: the loosest bound this datapath's backward kernels are held to one by one (test_attention_bwd_bf16x3; GEMM and
          convolution gradients: 5e-5).
  f16mx   1e-3 everywhere: TOL of tests/test_gpu_train_parity.py (north_star), and the f16p gate of test_attention_bwd_bf16x3.
Every case repeats the engine's backward with the cotangent times 2^-20 (a loss scale) against the SAME reference times 2^-20 — exact, and
gradients are linear in the cotangent, so the same gates hold: the per-slab power-of-two scaling of dO in ddpo_attention_bwd_x16 with f16p = 1 and any
underflow of the bf16 split of small gradients, through a whole network.
Measured values: profiles/r10_backward_budget.log."""
import functools
import math
from collections import OrderedDict

import pytest
import torch

from ddpo_amd import lib as L
from ddpo_amd.models.unet import UNet2DCondition, UNetConfig
from oracle import unet as OU

DEV = "cuda"
SEED = 3
SMALL = 1e-3            # a tensor under this share of the whole reference norm is bounded absolutely (see above)
#            vector, block, tensor
GATES = {"fp32": (2e-5, 3e-5, 5e-5), "bf16x3": (2e-4, 2e-4, 2e-4), "f16mx": (1e-3, 1e-3, 1e-3)}
#         oracle config, context width, samples, timesteps
NETS = {"tiny": (OU.TINY, 64, 2, (481, 21)), "tiny21": (OU.TINY21, 96, 2, (481, 21)), "sd15": (OU.SD15, 768, 1, (481,))}
HW = 16


@functools.lru_cache(maxsize=None)
def _inputs(net):
    """Weights and the rows of one train_step (b samples -> 2 b U-Net rows), plus the cotangent.  Shared and never modified."""
    ocfg, ctx_dim, b, ts = NETS[net]
    op = OU.init_params(OU.unet_param_shapes(ocfg), seed=SEED)
    g = torch.Generator().manual_seed(100 + SEED)
    lat = torch.randn(b, 4, HW, HW, generator=g)
    emb = torch.randn(b, 77, ctx_dim, generator=g)
    unc = torch.randn(1, 77, ctx_dim, generator=g).expand(b, -1, -1).contiguous()
    d_out = torch.randn(2 * b, 4, HW, HW, generator=g)
    ts = torch.tensor(ts, dtype=torch.int32)
    return op, torch.cat([lat, lat]), torch.cat([ts, ts]), torch.cat([unc, emb]).contiguous(), d_out


@functools.lru_cache(maxsize=None)
def _oracle_grads(net, dtype):
    """d <out, d_out> / d params of the oracle's U-Net in `dtype`, computed once per (net, dtype) and shared by every test."""
    op, lat2, ts2, ctx2, d_out = _inputs(net)
    leaves = OrderedDict((k, v.detach().clone().to(dtype).requires_grad_(True)) for k, v in op.items())
    out = OU.unet_forward(leaves, NETS[net][0], lat2.to(dtype), ts2, ctx2.to(dtype))
    out.backward(d_out.to(dtype))
    return OrderedDict((k, v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items())


def _errors(grad_of, ref, scale=1.0):
    """Per tensor (||g - scale * ref||^2, ||scale * ref||^2) in float64, on the device the gradients live on."""
    e2, r2 = [], []
    for n, r in ref.items():
        g = grad_of(n)
        r = r.to(g.device).double() * scale
        e2.append(((g.double() - r) ** 2).sum())
        r2.append((r ** 2).sum())
    return OrderedDict(zip(ref, zip(torch.stack(e2).cpu().tolist(), torch.stack(r2).cpu().tolist())))


def _figures(err):
    """vector, {block: error}, {tensor: error against max(||ref||, SMALL * ||ref, whole||)}, {tensor: its share of the whole norm}."""
    whole = math.sqrt(sum(r for _, r in err.values()))
    vec = math.sqrt(sum(e for e, _ in err.values())) / whole
    be, br = OrderedDict(), OrderedDict()
    for n, (e, r) in err.items():                         # the grouping of _groups in tests/test_gpu_train_parity.py
        k = n.split(".")[0]
        be[k] = be.get(k, 0.0) + e
        br[k] = br.get(k, 0.0) + r
    blocks = OrderedDict((k, math.sqrt(be[k]) / math.sqrt(br[k])) for k in be)
    tensors = OrderedDict((n, math.sqrt(e) / max(math.sqrt(r), SMALL * whole)) for n, (e, r) in err.items())
    share = OrderedDict((n, math.sqrt(r) / whole) for n, (_, r) in err.items())
    return vec, blocks, tensors, share, whole


def _record(title, err):
    vec, blocks, tensors, share, whole = _figures(err)
    wb, wt = max(blocks, key=blocks.get), max(tensors, key=tensors.get)
    rel = sum(1 for s in share.values() if s >= SMALL)
    from conftest import parity_record
    parity_record(f"\n[backward budget] {title}: ||g-g_ref||/||g_ref|| {vec:.2e}  worst block {wb} {blocks[wb]:.2e}  "
                  f"worst tensor {wt} {tensors[wt]:.2e} (its share of |g_ref| {share[wt]:.1e})  (|g_ref| = {whole:.3e}; {len(tensors)} tensors, "
                  f"{rel} held relatively, {len(tensors) - rel} under {SMALL:g} of |g_ref| held to gate x {SMALL:g} x |g_ref|)\n"
                  f"    vector error by block, ||g-g_ref||/||g_ref||: " + "  ".join(f"{k} {v:.1e}" for k, v in blocks.items()))
    return vec, blocks, tensors, share


def _over(title, err, gates):
    """Records the case and returns what is over its gate (empty: the case holds) and the tensors' shares of the whole norm."""
    vec, blocks, tensors, share = _record(title, err)
    over = [(title, "vector", vec)] if not vec < gates[0] else []
    over += [(title, k, e) for k, e in blocks.items() if not e < gates[1]]
    over += [(title, n, e, share[n]) for n, e in tensors.items() if not e < gates[2]]       # every tensor: relative, or absolute at SMALL of the whole
    return over, share


@pytest.fixture(scope="module", autouse=True)
def _release_shared():
    yield
    _oracle_grads.cache_clear()                           # the SD-1.5 weights and gradients are 3.4 GB each: not kept for the rest of the suite
    _inputs.cache_clear()


def _engine_case(net, datapath, monkeypatch):
    if datapath == "f16mx" and net != "sd15":
        monkeypatch.setattr(L, "MX_MIN_K", 256)        # the toy nets have no reduction of 2560: make their 3x3 convolutions f16mx layers
    op, lat2, ts2, ctx2, d_out = _inputs(net)
    ref = _oracle_grads(net, torch.float32 if net == "sd15" else torch.float64)
    old = L.DATAPATH
    L.DATAPATH = datapath
    try:
        unet = UNet2DCondition(UNetConfig.named(net), DEV)
        unet.params.load_dict(op)
        if datapath != "fp32":
            unet.params.pack_bf16()                      # with the backward planes
        lat2, ts2, ctx2, d_out = lat2.to(DEV), ts2.to(DEV), ctx2.to(DEV), d_out.to(DEV)
        G = unet.ensure_grads()
        over = []
        for k in (0, 20):                                # the cotangent as it is, then times 2^-20 on zeroed gradients
            G.flat.zero_()
            tape = []
            unet.forward(lat2, ts2, ctx2, tape=tape)
            unet.backward(tape, d_out * 2.0 ** -k)
            torch.cuda.synchronize()
            err = _errors(lambda n: G[n], ref, 2.0 ** -k)
            o, shares = _over(f"{net} {datapath} hw={HW} rows={lat2.shape[0]} cotangent x 2^-{k}", err, GATES[datapath])
            over += o
        assert not over, over[:20]                       # after BOTH passes are on record
        return shares
    finally:
        L.DATAPATH = old
        L.PACKED.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("datapath", ["fp32", "bf16x3", "f16mx"])
@pytest.mark.parametrize("net", ["tiny", "tiny21"])
def test_backward_of_the_toy_nets_on_the_same_cotangent(net, datapath, monkeypatch):
    shares = _engine_case(net, datapath, monkeypatch)
    assert len(shares) == 686 and sum(1 for s in shares.values() if s > 0.0) >= 600       # every tensor takes part, none with a zero reference


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("datapath", ["bf16x3", L.SHIPPED_DATAPATH])
def test_backward_of_sd15_on_the_same_cotangent(datapath, monkeypatch):
    """The real channel widths (320 / 640 / 1280, reductions up to 11520) at the smallest pixel count: dgrad, wgrad and the attention
    backward on the tile classes and split-K routes the toy nets never reach.  Two U-Net rows of 16x16 latents; the oracle in float32
    (its own error: 2e-6, a hundred times under the gates)."""
    _engine_case("sd15", datapath, monkeypatch)


@pytest.mark.parametrize("net", ["tiny", "tiny21"])
def test_fp32_yardstick_of_the_oracle(net):
    """The fp32 gates are 8 x the error of the oracle itself in float32 against float64 on these inputs.  Recomputed here, without a GPU,
    and held inside a quarter of each gate: the margin stays honest if the inputs ever change."""
    ref = _oracle_grads(net, torch.float64)
    f32 = _oracle_grads(net, torch.float32)
    err = _errors(lambda n: f32[n], ref)
    vec, blocks, tensors, share = _record(f"{net} oracle float32 against float64 hw={HW} rows=4 (the fp32 yardstick)", err)
    rel = {n: math.sqrt(e) / math.sqrt(r) for n, (e, r) in err.items() if share[n] >= 1e-6}          # purely relative, tiny tensors included
    assert len(err) == 686 and len(rel) >= 600
    gv, gb, gt = GATES["fp32"]
    assert vec <= gv / 4, vec
    assert max(blocks.values()) <= gb / 4, blocks
    assert max(rel.values()) <= gt / 4, max(rel, key=rel.get)
