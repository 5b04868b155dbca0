"""CPU-only checks of the CLIPScore reward's plumbing: registry and datasets, the missing-weights refusal, the EOS pooling rule, the
checkpoint-name mapping of the text tower and the prompt cache.  No device compute is launched here."""
import numpy as np
import pytest
import torch

from ddpo_amd.models import clip_text as CT
from ddpo_amd.models.text import ByteTokenizer


def test_registry_has_clip_score():
    from ddpo_amd.training import callback_fns
    from ddpo_amd.training.callbacks import clip_score_fn
    assert callback_fns["clip_score"] is clip_score_fn


@pytest.mark.parametrize("dataset,prompt_fn,kwargs", [
    ("clip-nouns-activities", "nouns_activities", {"nouns_path": "assets/common_animals.txt", "activities_path": "assets/activities_v0.txt"}),
    ("clip_animals", "from_file", {"loadpath": "assets/common_animals.txt"}),
])
def test_datasets_resolve_through_the_parser(dataset, prompt_fn, kwargs, tmp_path, monkeypatch):
    from ddpo_amd.utils.parser import Parser
    import config.base as CB
    monkeypatch.chdir(tmp_path)

    class P(Parser):
        config: str = "config.base"

    args = P(["--dataset", dataset, "--logbase", str(tmp_path / "run")]).parse_args("pg")
    assert args.filter_field == "clip_score" and args.prompt_fn == prompt_fn and dict(args.prompt_kwargs) == kwargs
    assert CB.clip_nouns_activities["common"]["prompt_kwargs"] == CB.llava_bertscore["common"]["prompt_kwargs"]
    assert CB.clip_nouns_activities["common"]["prompt_fn"] == CB.llava_bertscore["common"]["prompt_fn"]


def test_missing_weights_raise_without_a_gpu(tmp_path, monkeypatch):
    from ddpo_amd.training import callback_fns
    monkeypatch.setenv("DDPO_ALLOW_SYNTHETIC", "0")
    monkeypatch.delenv("DDPO_AESTHETIC_WEIGHTS", raising=False)
    monkeypatch.setenv("HF_HOME", str(tmp_path / "hf"))
    monkeypatch.delenv("HUGGINGFACE_HUB_CACHE", raising=False)
    monkeypatch.setenv("HOME", str(tmp_path))
    with pytest.raises(FileNotFoundError, match="openai/clip-vit-large-patch14"):
        callback_fns["clip_score"](weights_dir=str(tmp_path / "nothing"), cache=str(tmp_path / "cache"))


def test_eos_position_is_transformers_rule():
    """First occurrence of eos_token_id — on the stand-in tokenizer's output: the empty prompt, a short one, one truncated at 77 tokens."""
    tok = ByteTokenizer()
    prompts = ["", "a dog", "x" * 200]
    ids = np.asarray(tok(prompts).input_ids)
    assert ids.shape == (3, 77)
    got = CT.eos_positions(ids, tok.eos_token_id)
    want = (torch.as_tensor(ids) == tok.eos_token_id).int().argmax(dim=-1).numpy()       # transformers' CLIPTextTransformer pooling index
    assert got.tolist() == want.tolist() == [1, 6, 76]
    bad = ids.copy()
    bad[1, :] = 1000
    with pytest.raises(ValueError, match="row 1"):
        CT.eos_positions(bad, tok.eos_token_id)


def _tiny_hf_model():
    from transformers import CLIPConfig, CLIPModel, CLIPTextConfig, CLIPVisionConfig
    tc = CLIPTextConfig(vocab_size=49408, hidden_size=64, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
                        max_position_embeddings=77, hidden_act="quick_gelu", projection_dim=32, eos_token_id=49407, bos_token_id=49406)
    vc = CLIPVisionConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, image_size=56, patch_size=14,
                          hidden_act="quick_gelu", projection_dim=32)
    torch.manual_seed(0)
    return CLIPModel(CLIPConfig(text_config=tc.to_dict(), vision_config=vc.to_dict(), projection_dim=32))


def test_state_dict_mapping_consumes_every_text_key_and_fills_every_parameter():
    cfg = CT.TextConfig.named("tiny")
    sd = _tiny_hf_model().state_dict()
    tree, used = CT.text_state_to_tree(sd, cfg)
    text_keys = {k for k in sd if (k.startswith("text_model.") or k == "text_projection.weight") and not k.endswith("position_ids")}
    assert used == text_keys
    shapes = CT.text_param_shapes(cfg)
    assert set(tree) == set(shapes)
    assert all(tuple(tree[n].shape) == tuple(shapes[n]) for n in shapes)
    # dense kernels are transposed into the engine's (in, out) layout
    assert torch.equal(tree["layers.1.fc1.kernel"], sd["text_model.encoder.layers.1.mlp.fc1.weight"].t())
    assert torch.equal(tree["text_projection.kernel"], sd["text_projection.weight"].t())
    # the store itself can live on the host: every parameter is filled, the vision keys are ignored
    tower = CT.ClipTextTower(cfg, device="cpu")
    tower.load_state_dict(sd)
    assert all(torch.equal(tower.params[n], tree[n]) for n in shapes)
    assert tower.params.n_params == sum(sd[k].numel() for k in text_keys)


def test_named_configs():
    l14, tiny = CT.TextConfig.named("vit-l/14"), CT.TextConfig.named("tiny")
    assert (l14.hidden, l14.layers, l14.heads, l14.mlp, l14.positions, l14.vocab, l14.proj, l14.eps) == (768, 12, 12, 3072, 77, 49408, 768, 1e-5)
    assert (tiny.hidden, tiny.layers, tiny.heads, tiny.mlp, tiny.proj) == (64, 2, 4, 256, 32)
    from ddpo_amd.models.clip_vision import VisionConfig
    assert tiny.proj == VisionConfig.named("tiny").proj and l14.proj == VisionConfig.named("vit-l/14").proj
    assert sum(int(np.prod(s)) for s in CT.text_param_shapes(l14).values()) == 123060480 + 768 * 768      # CLIPTextModel + text_projection


def test_synthetic_text_state_leaves_the_aesthetic_draws_alone():
    """The text weights come from a generator of their own: the vision / MLP state of a seed is what it was without them."""
    from ddpo_amd.models.clip_vision import VisionConfig
    from ddpo_amd.models.laion import synthetic_state_dicts
    vcfg = VisionConfig.named("tiny")
    before, mlp_before = synthetic_state_dicts(vcfg, vcfg.proj, 3)
    text = CT.synthetic_text_state(CT.TextConfig.named("tiny"), 3)
    after, mlp_after = synthetic_state_dicts(vcfg, vcfg.proj, 3)
    assert not set(text) & set(before)
    assert all(torch.equal(before[k], after[k]) for k in before) and all(torch.equal(mlp_before[k], mlp_after[k]) for k in mlp_before)
    tree, used = CT.text_state_to_tree(text, CT.TextConfig.named("tiny"))
    assert used == set(text)


def test_prompt_cache_is_a_bounded_lru_and_embeds_each_distinct_prompt_once():
    from ddpo_amd.models.clip_score import PromptCache
    calls = []

    def embed(prompts):
        calls.append(list(prompts))
        return [torch.full((2,), float(len(p))) for p in prompts]

    c = PromptCache(embed, capacity=3)
    rows = c.lookup(["aa", "b", "aa", "aa", "b"])
    assert calls == [["aa", "b"]] and [float(r[0]) for r in rows] == [2, 1, 2, 2, 1]
    c.lookup(["ccc"])
    assert calls[-1] == ["ccc"] and len(c) == 3
    c.lookup(["aa"])                                   # a hit: no tower call, "aa" becomes the most recent
    assert len(calls) == 2
    c.lookup(["dddd"])                                 # evicts the least recently used: "b"
    assert list(c.rows) == ["ccc", "aa", "dddd"] and len(c) == 3
    c.lookup(["b", "aa"])                              # "b" is a miss again, "aa" still a hit; "ccc" goes
    assert calls[-1] == ["b"] and list(c.rows) == ["dddd", "aa", "b"]
    # more distinct prompts in one call than the cache holds: every row is still returned, the cache stays bounded
    rows = c.lookup([str(i) * (i + 1) for i in range(5)])
    assert [float(r[0]) for r in rows] == [1, 2, 3, 4, 5] and len(c) == 3
    assert c.misses == sum(len(x) for x in calls)
