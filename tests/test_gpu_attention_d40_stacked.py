"""d = 40 attention forward on the stacked K / V^T layout (csrc/attention_bf16.hip header: K rows [k_hi | k_lo | 8 zeros], one 120-long
score reduction in 8 MFMA steps; f16p: V^T hi and lo in ONE plane of 96 rows, lo rows added to hi rows in the output stage).

Shapes are the smallest at which each mechanism can go wrong; tolerances are the ones tests/test_gpu_bf16.py::test_attention_bf16x3 uses.
The same inputs also run under DDPO_ATTN_STACK=0 (the plain hi / lo planes) in ONE fresh child process — the switch is read once per
process — and both sets of errors are printed.

Which kernels must agree bit for bit: the file's rule is "identical instruction sequence -> identical bits" — the self-staging kernel
(`attn_fwd_bf16_kernel`, Nk < 256 through attention()), the register-staged image kernel (`attn_fwd_bf16_pk_kernel`) and the LDS-DMA image
kernel (`attn_fwd_bf16_dma_kernel`) all call attn_scores_tile / attn_softmax_tile* / attn_pv_tile* / attn_store_o on the same LDS picture,
so for one variant and one key set (a) attention() with a workspace == attention_from_images() (same kernel, same images), and
(b) the self-staging kernel == the image kernel on images of the same keys (the existing plane-emitting test already asserts this at
Nk = 77).  Different key sets (a prefix against the whole) are different sums and are not compared."""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from ddpo_amd import lib as L

DEV = "cuda"
D, HEADS = 40, 8
C = HEADS * D
VARIANTS = ["bf16x3", "f16mx"]
GATE = {"bf16x3": 3e-5, "f16mx": 1e-4}      # test_attention_bf16x3's gates; lse: 1e-4
# name: (B, Nq, Nk, form)
CASES = {
    "one_tile_self_staging": (1, 32, 64, "plain"),
    "cross_attention_ragged": (2, 130, 77, "plain"),
    "images_4_tiles": (1, 128, 256, "plain"),
    "images_ragged_last_tile": (2, 130, 333, "plain"),
    "fused_qkv_buffer": (1, 256, 256, "fused"),          # q / k / v are column blocks of one (rows, 3C) buffer
    "shared_queries": (2, 130, 333, "q_batches_1"),      # both batches attend with the queries of batch 0
}


def _rel(a, b):
    a = np.asarray(a.detach().cpu(), dtype=np.float64)
    b = np.asarray(b.detach().cpu(), dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs and the float64 reference of a case (computed once, shared, never modified)."""
    B, Nq, Nk, form = CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    qb = 1 if form == "q_batches_1" else B
    q, k, v = torch.randn(qb * Nq, C, generator=g), torch.randn(B * Nk, C, generator=g), torch.randn(B * Nk, C, generator=g)
    k[min(50, Nk - 1)] = q[3] * 3.0                      # a late spike: the running-maximum rescale of every accumulator register
    sp = lambda t, b, n: t.view(b, n, HEADS, D).permute(0, 2, 1, 3).double()
    s_ = sp(q, qb, Nq).expand(B, -1, -1, -1) @ sp(k, B, Nk).transpose(-1, -2) * D ** -0.5
    ref = (torch.softmax(s_, -1) @ sp(v, B, Nk)).permute(0, 2, 1, 3).reshape(B * Nq, C)
    return q, k, v, ref, torch.logsumexp(s_, -1) / math.log(2.0)


def _errors(name, variant):
    B, Nq, Nk, form = CASES[name]
    q, k, v, ref, ref_lse = _case(name)
    L.DATAPATH = variant
    if form == "fused":
        buf = torch.cat([q, k, v], 1).to(DEV)
        out, lse = L.attention(buf[:, :C], buf[:, C:2 * C], buf[:, 2 * C:], B, HEADS, Nq, Nk, D, ldq=3 * C, ldk=3 * C, ldv=3 * C, return_lse=True)
    else:
        out, lse = L.attention(q.to(DEV), k.to(DEV), v.to(DEV), B, HEADS, Nq, Nk, D, return_lse=True,
                               q_batches=1 if form == "q_batches_1" else None)
    return _rel(out, ref), _rel(lse.view(B, HEADS, Nq), ref_lse)


def _all_errors():
    old = L.DATAPATH
    try:
        return {f"{name}/{variant}": _errors(name, variant) for name in CASES for variant in VARIANTS}
    finally:
        L.DATAPATH = old


@pytest.fixture(scope="module")
def unstacked_errors():
    """The same cases on the plain layout: a fresh child process with DDPO_ATTN_STACK=0 (this process has long read the switch)."""
    env = dict(os.environ, DDPO_ATTN_STACK="0", PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.fixture
def datapath():
    old = L.DATAPATH
    yield
    L.DATAPATH = old
    L.PACKED.clear()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(CASES))
def test_stacked_d40_against_float64(datapath, unstacked_errors, name, variant):
    assert os.environ.get("DDPO_ATTN_STACK", "1")[:1] != "0", "this file tests the stacked layout: unset DDPO_ATTN_STACK"
    e_out, e_lse = _errors(name, variant)
    u_out, u_lse = unstacked_errors[f"{name}/{variant}"]
    print(f"\n[attention d=40 {variant} {name} {CASES[name][:3]}] stacked out {e_out:.2e} lse {e_lse:.2e} | DDPO_ATTN_STACK=0 out {u_out:.2e} lse {u_lse:.2e}"
          f" | gate {GATE[variant]:.0e} / 1e-04")
    assert e_out < GATE[variant]
    assert e_lse < 1e-4


@pytest.mark.parametrize("Nk,j", [(333, 5), (333, 330), (77, 3), (77, 70)])     # image path: first tile, last ragged tile; self-staging: both tiles
def test_lo_rows_are_added_to_hi_rows(datapath, Nk, j):
    """f16mx, one-hot softmax: every query is a positive multiple of one direction U and key j is c * U, so every other probability lies
    more than 40 binary orders below p_j and rounds to f16 zero.  Then O_i = v_j as the kernel holds it: f16 hi + f16 lo (exact to
    max(2^-22 |v|, 2^-25)), hi and lo rows summed and normalised in fp32 — |O - v_j| <= 2^-21 |v_j| + 2^-24 (a factor two for `inv` and the
    multiply).  A dropped or mis-paired lo row is a 2^-12 relative error, 500 times the bound."""
    L.DATAPATH = "f16mx"
    B, Nq, c = 1, 40, 8.0
    g = torch.Generator().manual_seed(7 * Nk + j)
    U = torch.randn(C, generator=g)
    q = (1.0 + torch.rand(Nq, 1, generator=g)) * U[None, :]
    k, v = torch.randn(Nk, C, generator=g), torch.randn(Nk, C, generator=g)          # v: full fp32 mantissas
    k[j] = c * U
    s2 = (q.view(Nq, HEADS, D).permute(1, 0, 2).double() @ k.view(Nk, HEADS, D).permute(1, 2, 0).double()) * D ** -0.5 / math.log(2.0)
    others = s2.clone()
    others[:, :, j] = -math.inf
    gap = float((s2[:, :, j] - others.max(-1).values).min())
    assert gap > 41.0, gap                               # the construction, not the kernel: 2^(14 - gap) rounds to f16 zero
    out = L.attention(q.to(DEV), k.to(DEV), v.to(DEV), B, HEADS, Nq, Nk, D).cpu().double()
    want = v[j].double()[None, :].expand(Nq, -1)
    err = (out - want).abs()
    bound = 2.0 ** -21 * want.abs() + 2.0 ** -24
    print(f"\n[attention d=40 f16mx one-hot Nk={Nk} j={j}] score gap {gap:.1f} log2 units, max |O - v| / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("B,Nq,Nk", [(1, 128, 256), (2, 130, 333), (1, 128, 64)])
def test_kernels_agree_bit_for_bit(datapath, monkeypatch, variant, B, Nq, Nk):
    """Pairs (a) and (b) of the module docstring.  Nk = 256, 333: attention() packs into its workspace and runs the image kernel, as
    attention_from_images() does on attention_kv_images().  Nk = 64 — the first 64 keys of the 256-key problem, same seed —: attention()
    runs the self-staging kernel, attention_from_images() the image kernel on the one (zero-padded) image of the same 64 keys.
    Plane-emitting output (row-major and k-blocked) is the split of the fp32 output."""
    L.DATAPATH = variant
    g = torch.Generator().manual_seed(256 if Nk == 64 else Nk)
    q = torch.randn(B * Nq, C, generator=g).to(DEV)
    k, v = (torch.randn(B * max(Nk, 256), C, generator=g)[:B * Nk].contiguous().to(DEV) for _ in range(2))
    out = L.attention(q, k, v, B, HEADS, Nq, Nk, D)
    img = L.attention_kv_images(k, v, B, HEADS, Nk, D)
    assert torch.equal(L.attention_from_images(q, img, B, HEADS, Nq, Nk, D), out)
    for kblocked in (False, True):
        monkeypatch.setattr(L, "A_KBLOCKED", kblocked)
        want = L.split_planes(out)
        for got in (L.attention(q, k, v, B, HEADS, Nq, Nk, D, planes_out=True), L.attention_from_images(q, img, B, HEADS, Nq, Nk, D, planes_out=True)):
            assert got.kblocked == kblocked and got.fmt == 0
            assert torch.equal(got.hi, want.hi) and torch.equal(got.lo, want.lo)


@pytest.mark.parametrize("variant", VARIANTS)
def test_image_contents(datapath, variant):
    """One (batch, head), Nk = 77 -> two tile images, decoded on the host.  K part (both variants): 64 rows of 88 bf16
    [k_hi(0..39) | k_lo(0..39) | 8 zeros] = 11264 B.  V^T part, pitch 68: f16mx — ONE plane of 96 rows (0..39 f16 hi, 40 ones, 41..47 zeros,
    48..87 f16 lo, 88..95 zeros) padded to 13312 B; bf16x3 — bf16 hi and lo planes of 64 rows each, no ones row.  Keys 77..127 are zeros."""
    assert os.environ.get("DDPO_ATTN_STACK", "1")[:1] != "0", "this file tests the stacked layout: unset DDPO_ATTN_STACK"
    L.DATAPATH = variant
    Nk, KT, LDK, LDVT = 77, 64, 88, 68
    g = torch.Generator().manual_seed(77)
    k, v = torch.randn(Nk, D, generator=g), torch.randn(Nk, D, generator=g)
    img = L.attention_kv_images(k.to(DEV), v.to(DEV), 1, 1, Nk, D).cpu().numpy()
    KP = KT * LDK * 2
    VP = 13312 if variant == "f16mx" else 2 * 64 * LDVT * 2
    assert img.size >= 2 * (KP + VP)
    bits = lambda t: t.contiguous().view(torch.int16).numpy().view(np.uint16)

    def hi_lo(x, dt):
        hi = x.to(dt)
        return bits(hi), bits((x - hi.float()).to(dt))

    kp = torch.zeros(2 * KT, D)
    kp[:Nk] = k
    vp = torch.zeros(2 * KT, D)
    vp[:Nk] = v
    k_hi, k_lo = hi_lo(kp, torch.bfloat16)
    v_hi, v_lo = hi_lo(vp, torch.float16 if variant == "f16mx" else torch.bfloat16)
    for tile in range(2):
        rows = slice(tile * KT, (tile + 1) * KT)
        base = tile * (KP + VP)
        K = img[base:base + KP].view(np.uint16).reshape(KT, LDK)
        assert np.array_equal(K[:, :D], k_hi[rows]) and np.array_equal(K[:, D:2 * D], k_lo[rows])       # chunks 0..4 hi, 5..9 lo
        assert not K[:, 2 * D:].any()                                                                 # chunk 10: the zero pad
        V = img[base + KP:base + KP + VP].view(np.uint16)
        if variant == "f16mx":
            assert not V[96 * LDVT:].any()                                                            # padding to whole KiB
            V = V[:96 * LDVT].reshape(96, LDVT)
            assert np.array_equal(V[:D, :KT], v_hi[rows].T) and np.array_equal(V[48:48 + D, :KT], v_lo[rows].T)
            assert (V[D, :KT] == 0x3C00).all()                                                        # the ones row, also over padded keys
            assert not V[D + 1:48].any() and not V[88:].any()
        else:
            V = V.reshape(2, 64, LDVT)
            assert np.array_equal(V[0, :D, :KT], v_hi[rows].T) and np.array_equal(V[1, :D, :KT], v_lo[rows].T)
            assert not V[:, D:].any()
        assert not V[..., KT:].any()                                                                  # the row pitch's 4 pad columns
    assert not k_hi[Nk:].any() and not v_hi[Nk:].any()                                                # keys 77..127 were compared as zeros


if __name__ == "__main__":          # the DDPO_ATTN_STACK=0 child of `unstacked_errors`
    L.load()
    print(json.dumps(_all_errors()))
