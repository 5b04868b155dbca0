"""CLIP text tower on the gfx950 kernels of this library (forward only) — the prompt side of the CLIPScore reward (models/clip_score.py).

The sibling of models/clip_vision.py, for the text half of the same `openai/clip-vit-large-patch14` checkpoint:

    embedding   `ddpo_gather_rows`: token-embedding row of every id + the position embedding (period = the sequence length), one launch
    12 x layer  LayerNorm -> q / k / v GEMMs -> causal attention (d = 64, 77 tokens, `ddpo_attention_causal_fwd`) -> out-proj GEMM (+residual)
                -> LayerNorm -> fc1 GEMM -> quick-GELU -> fc2 GEMM (+residual)
    pooling     final LayerNorm -> `ddpo_gather_rows` of the row at each prompt's EOS position -> bias-free text projection GEMM

Every contraction is `lib.linear`, the norms are `lib.layernorm`, under `lib.fp32_class_datapath()`; torch only reshapes.  The EOS position is
the FIRST occurrence of `eos_token_id` in a row (transformers' rule), found on the host from the ids; a row without one raises.

No padding mask exists or is needed: under the causal mask the pooled EOS row cannot see what follows it, so the padding after the first EOS
never reaches the result (with transformers' CLIPModel in float64, changing every token after the first EOS, or passing a padding
`attention_mask`, changes `text_embeds` by exactly 0).

Weights are held in the engine's (in, out) layout; `load_state_dict` takes transformers' torch names (`text_model.…`,
`text_projection.weight`) and ignores everything else (the vision tower, `logit_scale`); an HF Flax tree goes through
`clip_vision.flax_tree_to_torch_names` first.  There is no non-HIP path.  (models/text.py, the SD prompt encoder, is a different
consumer and stays on stock torch modules.)
"""
from collections import OrderedDict

import numpy as np
import torch

from .. import lib as L
from .unet import ParamStore


class TextConfig:
    def __init__(self, hidden=768, layers=12, heads=12, mlp=3072, positions=77, vocab=49408, proj=768, eps=1e-5, eos_token_id=49407):
        self.hidden, self.layers, self.heads, self.mlp, self.positions, self.vocab, self.proj, self.eps = hidden, layers, heads, mlp, positions, vocab, proj, eps
        self.eos_token_id = eos_token_id

    @staticmethod
    def named(name):
        if name in ("vit-l/14", "openai/clip-vit-large-patch14", "l14"):
            return TextConfig()
        if name == "tiny":          # pairs with VisionConfig.named("tiny"): same projection width
            return TextConfig(hidden=64, layers=2, heads=4, mlp=256, proj=32)
        raise KeyError(name)


def text_param_shapes(cfg: TextConfig):
    """Engine layouts: dense kernels (in, out); the two embedding tables as they are stored ((vocab | positions, hidden))."""
    d = OrderedDict()
    C = cfg.hidden
    d["embeddings.token_embedding"] = (cfg.vocab, C)
    d["embeddings.position_embedding"] = (cfg.positions, C)
    for i in range(cfg.layers):
        p = f"layers.{i}."
        for n in ("layer_norm1", "layer_norm2"):
            d[p + n + ".scale"] = (C,); d[p + n + ".bias"] = (C,)
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            d[p + n + ".kernel"] = (C, C); d[p + n + ".bias"] = (C,)
        d[p + "fc1.kernel"] = (C, cfg.mlp); d[p + "fc1.bias"] = (cfg.mlp,)
        d[p + "fc2.kernel"] = (cfg.mlp, C); d[p + "fc2.bias"] = (C,)
    d["final_layer_norm.scale"] = (C,); d["final_layer_norm.bias"] = (C,)
    d["text_projection.kernel"] = (C, cfg.proj)
    return d


def text_state_to_tree(sd, cfg: TextConfig):
    """transformers torch names -> (engine tree, the set of state-dict keys it consumed).  Pure host bookkeeping: no device is touched."""
    used = set()

    def g(k):
        used.add(k)
        return torch.as_tensor(sd[k]).float()

    t = "text_model."
    tree = {"embeddings.token_embedding": g(t + "embeddings.token_embedding.weight"),
            "embeddings.position_embedding": g(t + "embeddings.position_embedding.weight")}
    for i in range(cfg.layers):
        src, dst = f"{t}encoder.layers.{i}.", f"layers.{i}."
        for n in ("layer_norm1", "layer_norm2"):
            tree[dst + n + ".scale"], tree[dst + n + ".bias"] = g(src + n + ".weight"), g(src + n + ".bias")
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            tree[dst + n + ".kernel"], tree[dst + n + ".bias"] = g(src + f"self_attn.{n}.weight").t().contiguous(), g(src + f"self_attn.{n}.bias")
        for n in ("fc1", "fc2"):
            tree[dst + n + ".kernel"], tree[dst + n + ".bias"] = g(src + f"mlp.{n}.weight").t().contiguous(), g(src + f"mlp.{n}.bias")
    tree["final_layer_norm.scale"], tree["final_layer_norm.bias"] = g(t + "final_layer_norm.weight"), g(t + "final_layer_norm.bias")
    tree["text_projection.kernel"] = g("text_projection.weight").t().contiguous()
    return tree, used


def synthetic_text_state(cfg: TextConfig, seed=0):
    """Seeded random-init text tower in the checkpoint naming.  Drawn from a generator of its own, so the vision / MLP draws of
    `laion.synthetic_state_dicts` for the same seed are what they were before the text tower existed."""
    g = torch.Generator().manual_seed(int(seed) + 0x7e87)
    rn = lambda *s: torch.randn(*s, generator=g)
    C, t, sd = cfg.hidden, "text_model.", {}
    sd[t + "embeddings.token_embedding.weight"] = 0.02 * rn(cfg.vocab, C)
    sd[t + "embeddings.position_embedding.weight"] = 0.01 * rn(cfg.positions, C)
    for i in range(cfg.layers):
        p = f"{t}encoder.layers.{i}."
        for n in ("layer_norm1", "layer_norm2"):
            sd[p + n + ".weight"], sd[p + n + ".bias"] = 1 + 0.1 * rn(C), 0.02 * rn(C)
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            sd[p + f"self_attn.{n}.weight"], sd[p + f"self_attn.{n}.bias"] = rn(C, C) / C ** 0.5, 0.02 * rn(C)
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = rn(cfg.mlp, C) / C ** 0.5, 0.02 * rn(cfg.mlp)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = rn(C, cfg.mlp) / cfg.mlp ** 0.5, 0.02 * rn(C)
    sd[t + "final_layer_norm.weight"], sd[t + "final_layer_norm.bias"] = 1 + 0.1 * rn(C), 0.02 * rn(C)
    sd["text_projection.weight"] = rn(cfg.proj, C) / C ** 0.5
    return sd


def eos_positions(input_ids, eos_token_id):
    """Position of the FIRST `eos_token_id` in every row of (n, T) ids (transformers' pooling rule); raises on a row without one."""
    ids = np.asarray(input_ids)
    if ids.ndim != 2:
        raise ValueError(f"input_ids must be (n, T), got shape {ids.shape}")
    hit = ids == eos_token_id
    missing = np.flatnonzero(~hit.any(axis=1))
    if missing.size:
        raise ValueError(f"input_ids row {int(missing[0])} holds no EOS token ({eos_token_id}): the text tower pools at the first EOS")
    return hit.argmax(axis=1).astype(np.int64)


class ClipTextTower:
    def __init__(self, cfg: TextConfig, device="cuda"):
        self.cfg = cfg
        self.device = torch.device(device)
        if cfg.positions > L.CAUSAL_MAX_N or cfg.hidden // cfg.heads not in (16, 64):
            raise ValueError(f"the causal attention kernel serves at most {L.CAUSAL_MAX_N} positions and head dims 16 / 64")
        self.params = ParamStore(text_param_shapes(cfg), self.device)

    def load_state_dict(self, sd):
        """transformers torch names (`text_model.…`, `text_projection.weight`); extra keys (the vision tower, `logit_scale`) are ignored."""
        tree, _ = text_state_to_tree(sd, self.cfg)
        self.params.load_dict(tree)
        if self.device.type == "cuda" and L.current_datapath() != "fp32":
            self.pack()

    def pack(self):
        """bf16 hi / lo planes of every contraction weight (frozen reward model: once)."""
        for n, w in self.params.views.items():
            if n.endswith(".kernel"):
                L.pack_weights(w, bwd=False)

    def forward(self, input_ids):
        """(n, T <= positions) integer ids on the host -> text_embeds (n, proj) on the device.  fp32-class datapath like the image tower."""
        with L.fp32_class_datapath():
            return self._forward(input_ids)

    def _forward(self, input_ids):
        cfg, P = self.cfg, self.params
        ids = np.asarray(input_ids)
        eos = eos_positions(ids, cfg.eos_token_id)
        n, T = ids.shape
        if not 1 <= T <= cfg.positions:
            raise ValueError(f"sequence length {T} outside [1, {cfg.positions}]")
        L.check_indices(ids, cfg.vocab, "token id")
        C, d = cfg.hidden, cfg.hidden // cfg.heads
        tok = torch.from_numpy(ids.reshape(-1).astype(np.int32)).to(self.device)
        pool = torch.from_numpy((np.arange(n) * T + eos).astype(np.int32)).to(self.device)
        h = L.gather_rows(P["embeddings.token_embedding"], tok, add=P["embeddings.position_embedding"][:T])
        for i in range(cfg.layers):
            pre = f"layers.{i}."
            w = lambda m: P[pre + m + ".kernel"]
            b = lambda m: P[pre + m + ".bias"]
            pl = all(L.planes_ok(w(m), C, n * T) for m in ("q_proj", "k_proj", "v_proj"))
            t = L.layernorm(h, P[pre + "layer_norm1.scale"], P[pre + "layer_norm1.bias"], cfg.eps, planes=pl)
            q, k, v = L.linear(t, w("q_proj"), b("q_proj")), L.linear(t, w("k_proj"), b("k_proj")), L.linear(t, w("v_proj"), b("v_proj"))
            a = L.attention_causal(q, k, v, n, cfg.heads, T, d)
            h = L.linear(a, w("out_proj"), b("out_proj"), residual=h)
            t = L.layernorm(h, P[pre + "layer_norm2.scale"], P[pre + "layer_norm2.bias"], cfg.eps, planes=L.planes_ok(w("fc1"), C, n * T))
            f = L.linear(t, w("fc1"), b("fc1"))
            L.quick_gelu(f, out=f)
            h = L.linear(f, w("fc2"), b("fc2"), residual=h)
        h = L.layernorm(h, P["final_layer_norm.scale"], P["final_layer_norm.bias"], cfg.eps)
        pooled = L.gather_rows(h, pool)
        return L.linear(pooled, P["text_projection.kernel"])

    __call__ = forward
