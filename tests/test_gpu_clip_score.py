"""CLIPScore prompt-alignment reward on the engine's own kernels: the three kernels of csrc/clip_text.hip against float64, the text tower
(models/clip_text.py) and the end-to-end score (models/clip_score.py) against transformers' torch `CLIPModel` on the CPU in float64 with
the same seeded weights, batch independence / the prompt cache, the callback contract and the entrypoint.

Bounds: causal attention max-abs error over max-abs reference < 1e-5 (what tests/test_gpu_kernels.py::test_attention holds the fp32 kernel
to); gather bit-exact; cosine 1e-6 absolute; text_embeds relative 1e-3 (the contract of tests/test_gpu_aesthetic.py); the cosine of a score
2e-3 absolute (two unit vectors each within 1e-3 move their cosine by at most 2e-3 — random-init cosines sit near zero, so a relative bound
on the score would be meaningless)."""
import ctypes
import json
import math
import os
import sys
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ddpo_amd import lib as L
from ddpo_amd.models import clip_score as CS
from ddpo_amd.models import clip_text as CT
from ddpo_amd.models.clip_vision import VisionConfig, preprocess
from ddpo_amd.models.laion import synthetic_state_dicts

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROMPTS = ["", "a dog", "a photo of a capybara riding a bicycle through a field of sunflowers at dawn, highly detailed oil painting, trending"]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


# ------------------------------------------------------------------------------------------------ kernels
def _causal_ref(q, k, v, B, heads, N, d, scale):
    q, k, v = (x.double().cpu().view(B, N, heads, d).permute(0, 2, 1, 3) for x in (q, k, v))
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale
    s = s.masked_fill(torch.triu(torch.ones(N, N, dtype=torch.bool), diagonal=1), float("-inf"))
    return torch.einsum("bhqk,bhkd->bhqd", torch.softmax(s, -1), v).permute(0, 2, 1, 3).reshape(B * N, heads * d)


def _fused_qkv(B, heads, N, d, seed, gain=1.0):
    """q, k, v as the three column blocks of ONE (B*N, 3C) buffer: strided ldq / ldk / ldv."""
    C = heads * d
    g = torch.Generator().manual_seed(seed)
    buf = (gain * torch.randn(B * N, 3 * C, generator=g)).to(DEV)
    return buf, buf[:, :C], buf[:, C:2 * C], buf[:, 2 * C:]


CAUSAL_SHAPES = [(3, 12, 77, 64), (2, 4, 77, 16)] + [(2, 3, n, 64) for n in (1, 15, 16, 17, 48, 64, 65, 77)] + [(1, 2, 80, 64), (2, 2, 33, 16)]


@pytest.mark.parametrize("B,heads,N,d", CAUSAL_SHAPES)
def test_causal_attention_matches_float64(B, heads, N, d):
    C = heads * d
    buf, q, k, v = _fused_qkv(B, heads, N, d, seed=N * 131 + d)
    out = L.attention_causal(q, k, v, B, heads, N, d, ldq=3 * C, ldk=3 * C, ldv=3 * C)
    torch.cuda.synchronize()
    want = _causal_ref(q, k, v, B, heads, N, d, d ** -0.5)
    err = _rel(out.cpu(), want)
    print(f"\n[causal attention B={B} heads={heads} N={N} d={d}] max-abs err / max-abs ref {err:.2e}")
    assert err < 1e-5
    # the first token attends to itself only: its output row is exactly its value row
    assert torch.equal(out.view(B, N, C)[:, 0], v.reshape(B, N, C)[:, 0])


def test_causal_attention_large_logits():
    """Scores of several hundred (log2 domain: beyond what exp2 of an unshifted score could hold): the row maximum must be subtracted."""
    B, heads, N, d = 2, 3, 77, 64
    C = heads * d
    buf, q, k, v = _fused_qkv(B, heads, N, d, seed=5, gain=6.0)
    out = L.attention_causal(q, k, v, B, heads, N, d, ldq=3 * C, ldk=3 * C, ldv=3 * C)
    want = _causal_ref(q, k, v, B, heads, N, d, d ** -0.5)
    s_max = float((torch.einsum("nc,mc->nm", q[:N, :d].double(), k[:N, :d].double()) * d ** -0.5).abs().max())
    err = _rel(out.cpu(), want)
    print(f"\n[causal attention large logits] max |score| {s_max:.0f}  err {err:.2e}")
    assert s_max > 100 and torch.isfinite(out).all() and err < 1e-5


def test_causal_attention_bad_arguments_return_einval_and_launch_nothing():
    B, heads, N, d = 1, 2, 77, 64
    C = heads * d
    q, k, v = (torch.randn(B * N, C, device=DEV) for _ in range(3))
    o = torch.full((B * 80, C), 7.0, device=DEV)
    fn, st = L.load().ddpo_attention_causal_fwd, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    call = lambda qp, n, dd, heads_=heads, ld=C: fn(qp, ld, p(k), ld, p(v), ld, p(o), ld, B, heads_, n, dd, 0.125, st)
    assert call(p(q), N, 40, heads_=3, ld=120) == -1          # unsupported head dim
    assert call(p(q), 81, d) == -1                           # above the stated maximum of 80 tokens
    assert call(p(q, 4), N, d) == -1                         # misaligned pointer
    assert call(ctypes.c_void_p(0), N, d) == -1              # null pointer
    assert call(p(q), 0, d) == -1 and call(p(q), N, d, ld=C + 2) == -1
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())
    with pytest.raises(L.DdpoHipError):
        L.attention_causal(q, k, v, B, heads, 81, d)


def test_gather_rows_is_bit_exact():
    g = torch.Generator().manual_seed(1)
    wide = torch.randn(500, 96, generator=g).to(DEV)
    for table in (wide[:, :64].contiguous(), wide[:, 16:80]):                       # contiguous, and a row-strided view (ld = 96)
        idx = torch.randint(0, 500, (3 * 77,), generator=g).to(torch.int32).to(DEV)
        add = torch.randn(77, 64, generator=g).to(DEV)
        got = L.gather_rows(table, idx, add=add)
        want = torch.index_select(table, 0, idx.long()) + add.repeat(3, 1)
        assert torch.equal(got, want)
        assert torch.equal(L.gather_rows(table, idx), torch.index_select(table, 0, idx.long()))
    # an out-of-range index is clamped into the table by the kernel and refused by the host-side check
    table = wide[:, :64].contiguous()
    got = L.gather_rows(table, torch.tensor([-3, 0, 499, 12345], dtype=torch.int32, device=DEV))
    assert torch.equal(got, table[[0, 0, 499, 499]])
    with pytest.raises(ValueError):
        L.check_indices(np.array([0, 500]), 500)
    assert L.load().ddpo_gather_rows(None, 64, 500, None, 4, 64, None, 0, None, None) == -1


@pytest.mark.parametrize("cols", [32, 768])
def test_cosine_rows_matches_float64(cols):
    g = torch.Generator().manual_seed(cols)
    a, b = torch.randn(9, cols, generator=g), torch.randn(9, cols, generator=g)
    b[0], b[1] = 3.0 * a[0], 0.25 * a[1]                  # parallel
    b[2], b[3] = -2.0 * a[2], -a[3]                       # antiparallel
    want = (a.double() * b.double()).sum(-1) / (a.double().norm(dim=-1) * b.double().norm(dim=-1))
    got = L.cosine_rows(a.to(DEV), b.to(DEV)).cpu().double()
    got_s = L.cosine_rows(a.to(DEV), b.to(DEV), scale=100.0).cpu().double()
    err = float((got - want).abs().max())
    print(f"\n[cosine_rows cols={cols}] max abs err {err:.2e}  scaled/100 {float((got_s / 100 - want).abs().max()):.2e}")
    assert err < 1e-6 and float((got_s / 100 - want).abs().max()) < 1e-6
    assert float((want[:2] - 1).abs().max()) < 1e-12 and float((want[2:4] + 1).abs().max()) < 1e-12
    assert torch.equal(L.cosine_rows(a.to(DEV), b.to(DEV)).cpu().double(), got)          # fixed summation order


# ------------------------------------------------------------------------------------------------ oracle: transformers' CLIPModel, float64
def _hf_model(vcfg, tcfg, state):
    from transformers import CLIPConfig, CLIPModel, CLIPTextConfig, CLIPVisionConfig
    tc = CLIPTextConfig(vocab_size=tcfg.vocab, hidden_size=tcfg.hidden, intermediate_size=tcfg.mlp, num_hidden_layers=tcfg.layers,
                        num_attention_heads=tcfg.heads, max_position_embeddings=tcfg.positions, hidden_act="quick_gelu", projection_dim=tcfg.proj,
                        layer_norm_eps=tcfg.eps, eos_token_id=tcfg.eos_token_id, bos_token_id=49406)
    vc = CLIPVisionConfig(hidden_size=vcfg.hidden, intermediate_size=vcfg.mlp, num_hidden_layers=vcfg.layers, num_attention_heads=vcfg.heads,
                          image_size=vcfg.image, patch_size=vcfg.patch, hidden_act="quick_gelu", projection_dim=vcfg.proj, layer_norm_eps=vcfg.eps)
    m = CLIPModel(CLIPConfig(text_config=tc.to_dict(), vision_config=vc.to_dict(), projection_dim=tcfg.proj))
    res = m.load_state_dict(state, strict=False)
    assert not res.unexpected_keys and all(k.endswith("position_ids") for k in res.missing_keys), (res.unexpected_keys[:3], res.missing_keys[:3])
    return m.double().eval()


def _state(config, seed):
    vcfg, tcfg = VisionConfig.named(config), CT.TextConfig.named(config)
    sd, _ = synthetic_state_dicts(vcfg, vcfg.proj, seed)
    sd.update(CT.synthetic_text_state(tcfg, seed))
    sd["logit_scale"] = torch.tensor(CS.SYNTHETIC_LOGIT_SCALE)
    return vcfg, tcfg, sd


@pytest.fixture(scope="module")
def l14():
    vcfg, tcfg, sd = _state("vit-l/14", 11)
    return vcfg, tcfg, sd, _hf_model(vcfg, tcfg, sd)


@pytest.fixture(scope="module")
def tiny():
    vcfg, tcfg, sd = _state("tiny", 12)
    return vcfg, tcfg, sd, _hf_model(vcfg, tcfg, sd)


def _oracle_text(m, ids):
    with torch.no_grad():
        pooled = m.text_model(input_ids=torch.as_tensor(ids, dtype=torch.long)).pooler_output
        return m.text_projection(pooled)


def _check_text_tower(model, datapath, name):
    vcfg, tcfg, sd, m = model
    L.DATAPATH = datapath
    from ddpo_amd.models.text import ByteTokenizer
    prompts = PROMPTS + ["a cat washing the dishes"]
    ids = np.asarray(ByteTokenizer()(prompts).input_ids)
    assert CT.eos_positions(ids, tcfg.eos_token_id).tolist() == [1, 6, 76, 25]          # empty, short, all 77 positions used
    tower = CT.ClipTextTower(tcfg, DEV)
    tower.load_state_dict(sd)
    got = tower(ids).cpu()
    want = _oracle_text(m, ids)
    err = _rel(got, want)
    print(f"\n[clip text tower {name} {datapath}] text_embeds rel {err:.2e}")
    assert got.shape == (4, tcfg.proj) and err < 1e-3
    # padding never reaches the pooled row: other tokens after the first EOS give the same bits
    ids2 = ids.copy()
    ids2[1, 7:] = 1234
    assert torch.equal(tower(ids2).cpu(), got)


@pytest.mark.parametrize("datapath", ["fp32", "bf16x3"])
def test_tiny_text_tower_matches_transformers(tiny, datapath):
    _check_text_tower(tiny, datapath, "tiny")


@pytest.mark.timeout(900)
@pytest.mark.parametrize("datapath", ["fp32", "bf16x3"])
def test_vit_l14_text_tower_matches_transformers(l14, datapath):
    """The real geometry: 12 layers, 77 tokens, 12 heads of 64, the 49408-row vocabulary."""
    _check_text_tower(l14, datapath, "ViT-L/14")


def _check_scores(model, datapath, name, imgs, logit_scale):
    vcfg, tcfg, sd, m = model
    L.DATAPATH = datapath
    prompts = (PROMPTS + ["a cat washing the dishes"])[:len(imgs)]
    scorer = CS.ClipScorer(config=name, clip_state=sd, logit_scale=logit_scale, device=DEV)
    got, cos = scorer(imgs, prompts, return_cosine=True)
    ls = float(sd["logit_scale"]) if logit_scale is None else logit_scale
    with torch.no_grad():
        m.logit_scale.data.fill_(ls)
        out = m(input_ids=torch.as_tensor(scorer.tokenize(prompts), dtype=torch.long), pixel_values=torch.from_numpy(preprocess(imgs, vcfg.image)).double())
        want = out.logits_per_image.diagonal().numpy()
    want_cos = want / math.exp(ls)
    e_cos, e_score = float(np.abs(cos - want_cos).max()), float(np.abs(got - want).max())
    print(f"\n[clip_score {name} {datapath} logit_scale {ls:.4f}] cosine abs err {e_cos:.2e}  score abs err {e_score:.2e}  scores {got}  cosines {cos}")
    assert got.shape == (len(imgs),) and got.dtype == np.float32 and cos.dtype == np.float32
    assert e_cos < 2e-3 and e_score < 2e-3 * math.exp(ls)
    return scorer


@pytest.mark.parametrize("logit_scale", [None, math.log(100.0)])
@pytest.mark.parametrize("datapath", ["fp32", "bf16x3"])
def test_tiny_scores_match_logits_per_image(tiny, datapath, logit_scale):
    imgs = np.random.default_rng(3).random((3, 80, 64, 3), dtype=np.float32)
    _check_scores(tiny, datapath, "tiny", imgs, logit_scale)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("logit_scale", [None, math.log(100.0)])
def test_vit_l14_scores_match_logits_per_image_bf16x3(l14, logit_scale):
    """ViT-L/14 on 512x512 inputs as the sampler produces them; then the same pairs in two calls of two, reversed: the same bits."""
    imgs = np.random.default_rng(5).random((4, 512, 512, 3), dtype=np.float32)
    imgs[1] = np.clip(imgs[1] * 0.2 + np.linspace(0, 0.8, 512, dtype=np.float32)[None, :, None], 0, 1)     # a smooth image as well as noise
    scorer = _check_scores(l14, "bf16x3", "vit-l/14", imgs, logit_scale)
    prompts = PROMPTS + ["a cat washing the dishes"]
    whole = scorer(imgs, prompts)
    fresh = CS.ClipScorer(config="vit-l/14", clip_state=l14[2], logit_scale=logit_scale, device=DEV)
    halves = np.concatenate([fresh(imgs[[3, 2]], [prompts[3], prompts[2]]), fresh(imgs[[1, 0]], [prompts[1], prompts[0]])])[::-1]
    assert np.array_equal(whole, halves)


# ------------------------------------------------------------------------------------------------ batch independence, cache
class _Spy:
    def __init__(self, tower):
        self.tower, self.rows = tower, []

    def __call__(self, ids):
        self.rows.append(len(ids))
        return self.tower(ids)


@pytest.mark.parametrize("datapath", ["fp32", "bf16x3"])
def test_scores_do_not_depend_on_batch_order_or_cache(tiny, datapath):
    L.DATAPATH = datapath
    sd = tiny[2]
    imgs = np.random.default_rng(8).random((6, 64, 64, 3), dtype=np.float32)
    prompts = ["a dog", "a cat riding a bike", "", "a dog", "a llama playing chess", "x" * 120]
    a = CS.ClipScorer(config="tiny", clip_state=sd, device=DEV)
    whole = a(imgs, prompts)                                                         # 6 pairs at once, cold cache
    b = CS.ClipScorer(config="tiny", clip_state=sd, device=DEV)
    o1, o2 = [4, 1, 5], [2, 3, 0]
    parts = np.empty(6, np.float32)
    parts[o1] = b(imgs[o1], [prompts[i] for i in o1])                                # the same pairs, two calls of 3, another order
    parts[o2] = b(imgs[o2], [prompts[i] for i in o2])
    b.text = _Spy(b.text)
    asked = []
    embed = b.prompts.embed
    b.prompts.embed = lambda p: (asked.append(list(p)), embed(p))[1]
    warm = b(imgs, prompts)                                                          # warm cache: every prompt is a hit
    assert np.array_equal(whole, parts) and np.array_equal(whole, warm)
    assert b.text.rows == [] and asked == [] and len(b.prompts) == 5
    assert np.isfinite(whole).all() and whole[0] != whole[3]                         # same prompt, different image


# ------------------------------------------------------------------------------------------------ callback, entrypoint
def _tiny_towers(monkeypatch):
    monkeypatch.setattr(CS.VisionConfig, "named", staticmethod(lambda name, _orig=CS.VisionConfig.named: _orig("tiny")))   # seconds, not minutes
    monkeypatch.setattr(CS.TextConfig, "named", staticmethod(lambda name, _orig=CS.TextConfig.named: _orig("tiny")))


def test_callback_contract_and_thread_safety(monkeypatch):
    """`callback_fns['clip_score']()` -> fn(images, prompts, metadata) -> ((N,1) scores, info), evaluated by a worker thread while the main
    thread keeps the GPU busy on its own stream (pipeline/policy_gradient.py submits rewards to a ThreadPoolExecutor)."""
    from ddpo_amd.training import callback_fns, evaluate_callbacks
    from ddpo_amd.models.unet import UNet2DCondition, UNetConfig
    monkeypatch.setenv("DDPO_ALLOW_SYNTHETIC", "1")
    _tiny_towers(monkeypatch)
    L.DATAPATH = "bf16x3"
    fn = callback_fns["clip_score"]()
    imgs = np.random.default_rng(9).random((5, 64, 64, 3), dtype=np.float32)
    prompts = ["a dog", "a cat", "a dog", "", "a bear washing the dishes"]
    alone, info = fn(imgs, prompts, ({},) * 5)
    assert alone.shape == (5, 1) and alone.dtype == np.float32 and bool(info["synthetic_weights"]) is True
    assert info["cosine"].shape == (5,) and np.allclose(alone[:, 0], math.exp(CS.SYNTHETIC_LOGIT_SCALE) * info["cosine"], rtol=1e-5, atol=1e-6)
    # a prompt given as a list of alternatives is reduced to one string by evaluate_callbacks before the reward sees it
    res = evaluate_callbacks({"clip_score": fn}, imgs[:2], [["a dog"], ["a cat"]], ({},) * 2)["clip_score"]
    assert np.array_equal(res[0], alone[:2])
    unet = UNet2DCondition(UNetConfig.named("tiny"), DEV)
    unet.params.init_synthetic(0)
    unet.params.pack_bf16(bwd=False)
    x, t, c = torch.randn(4, 4, 16, 16, device=DEV), torch.full((4,), 481, dtype=torch.int32, device=DEV), torch.randn(4, 77, 64, device=DEV)
    ref = unet(x, t, c).clone()
    fresh = callback_fns["clip_score"]()                       # cold cache: the worker thread runs the text tower too
    out = {}
    th = threading.Thread(target=lambda: out.setdefault("r", fresh(imgs, prompts, ({},) * 5)))
    th.start()
    for _ in range(20):
        y = unet(x, t, c)
    th.join()
    torch.cuda.synchronize()
    assert np.array_equal(out["r"][0], alone) and np.array_equal(out["r"][1]["cosine"], info["cosine"]) and torch.equal(y, ref)


def test_entrypoint_clip_nouns_activities(tmp_path, monkeypatch):
    """nouns_activities prompts + the clip_score reward, offline end to end: no server, no weights (synthetic towers, tiny U-Net)."""
    monkeypatch.setenv("DDPO_MODEL_CONFIG", "tiny")
    monkeypatch.setenv("DDPO_ALLOW_SYNTHETIC", "1")
    _tiny_towers(monkeypatch)
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, ROOT)
    import importlib
    pg = importlib.import_module("pipeline.policy_gradient")
    out = pg.main(["--dataset", "clip-nouns-activities", "--resolution", "64", "--n_inference_steps", "4", "--sample_batch_size", "2",
                   "--train_batch_size", "1", "--train_accumulation_steps", "2", "--num_train_epochs", "2", "--save_freq", "1",
                   "--per_prompt_stats_min_count", "2", "--logbase", str(tmp_path / "run")])
    lp = out["localpath"]
    assert len(out["mean_rewards"]) == 2 and all(np.isfinite(out["mean_rewards"]))
    for epoch in (0, 1):
        r = np.load(os.path.join(lp, f"rewards/0_{epoch}.npy"))
        info = np.load(os.path.join(lp, f"callback_info/0_{epoch}.npy"), allow_pickle=True).item()
        prompts = np.load(os.path.join(lp, f"prompts/0_{epoch}.npy"))
        assert r.shape == (2, 1) and np.isfinite(r).all() and all(" " in p for p in prompts)
        assert set(info) == {"cosine", "synthetic_weights"} and info["cosine"].shape == (2,) and bool(info["synthetic_weights"].all())
        assert np.allclose(r[:, 0], math.exp(CS.SYNTHETIC_LOGIT_SCALE) * info["cosine"], rtol=1e-5, atol=1e-6)
    with open(os.path.join(lp, "args.json")) as f:
        args = json.load(f)
    assert args["filter_field"] == "clip_score" and args["prompt_fn"] == "nouns_activities"
