"""LoRA adapters on the U-Net attention projections (attn1 / attn2 . to_q / to_k / to_v / to_out_0) and, with targets "attn_ff", on the
GEGLU feed-forward layers of the transformer blocks as well (ff.net_0.proj, ff.net_2), merged-weight form.

Every adapted dense kernel W (Flax layout (K = in, N = out)) is W' = W0 + s * A B with A (K, r), B (r, N), s = alpha / r.  The U-Net's flat
ParamStore always holds W': the sampler and the training forward run exactly the kernels they run without adapters.  After each optimizer
update `merge()` rewrites every W' from a frozen copy of W0 in one launch (ddpo_lora_merge) and repacks only the adapted tensors.  The backward
computes dA / dB with ddpo_lora_wgrad and no base-weight gradient at all (UNet2DCondition.backward with `unet.lora` set).

Checkpoints use diffusers' attention-processor key layout (`…attn1.processor.to_q_lora.down.weight` (r, in) = A^T,
`…up.weight` (out, r) = B^T); the key names are derived from the Flax names with the inverse of utils/serialization.torch_to_flax_tree's
renaming.  Feed-forward adapters are written under the module's own diffusers path: `…ff.net.0.proj.lora.down.weight` / `….lora.up.weight`,
same orientation; the file's metadata names the target set.
"""
import math
import re
from collections import OrderedDict

import torch

from .. import lib as L
from .unet import ParamStore

_TARGET = re.compile(r"\.attn[12]\.(to_q|to_k|to_v|to_out_0)\.kernel$")
_TARGET_FF = re.compile(r"\.transformer_blocks_0\.ff\.(net_0\.proj|net_2)\.kernel$")
TARGET_SETS = ("attn", "attn_ff")
# ddpo_lora_wgrad (csrc/lora.hip) holds a layer's A / B slice in LDS and its columns in registers: layers past these limits (the feed-forward
# layers of the real models) take ddpo_lora_wgrad_wide (csrc/lora_wide.hip)
NARROW_MAX_DIM = 2048
NARROW_MAX_SUM = 4064


def check_targets(targets):
    if targets not in TARGET_SETS:
        raise ValueError(f"lora_targets must be one of {' / '.join(TARGET_SETS)} (got {targets!r})")
    return targets


def lora_targets(shapes, targets="attn"):
    """Flax kernel names of the adapted layers (deterministic: the U-Net's layout order): the attention projections in parameter order, then,
    under "attn_ff", the feed-forward layers in parameter order — the attention prefix is the same list under both settings."""
    check_targets(targets)
    out = [n for n in shapes if _TARGET.search(n)]
    if targets == "attn_ff":
        out += [n for n in shapes if _TARGET_FF.search(n)]
    return out


def lora_wgrad(x, dy, A, B, dA, dB, s):
    """The adapter gradients of one layer of any supported width: lib.lora_wgrad inside its limits (those layers keep their bits), the wide
    entry of lib_lora_wide.py — bound here, on first use — otherwise."""
    K, N = A.shape[0], dy.shape[1]
    if K <= NARROW_MAX_DIM and N <= NARROW_MAX_DIM and K + N <= NARROW_MAX_SUM:
        return L.lora_wgrad(x, dy, A, B, dA, dB, s)
    from .. import lib_lora_wide
    return lib_lora_wide.lora_wgrad_wide(x, dy, A, B, dA, dB, s)


def check_rank(rank):
    rank = int(rank)
    if not 1 <= rank <= L.LORA_MAX_RANK:
        raise ValueError(f"lora_rank must be in 1..{L.LORA_MAX_RANK} (got {rank}; 0 switches LoRA off)")
    return rank


def lora_scale(rank, alpha=None):
    """s = alpha / rank; alpha None means alpha = rank (s = 1)."""
    return 1.0 if alpha is None else float(alpha) / float(rank)


def adapter_shapes(shapes, rank, targets="attn"):
    """{<layer>.A: (K, r), <layer>.B: (r, N)} for every target, in target order."""
    out = OrderedDict()
    for n in lora_targets(shapes, targets):
        K, N = shapes[n]
        layer = n[:-len(".kernel")]
        out[layer + ".A"] = (K, rank)
        out[layer + ".B"] = (rank, N)
    return out


def n_adapter_params(shapes, rank, targets="attn"):
    return sum(math.prod(s) for s in adapter_shapes(shapes, rank, targets).values())


def diffusers_key(layer):
    """Flax layer name (`down_blocks_0.attentions_0.transformer_blocks_0.attn1.to_q`) -> the diffusers attention-processor prefix
    (`down_blocks.0.attentions.0.transformer_blocks.0.attn1.processor.to_q_lora`); a feed-forward layer (`….ff.net_0.proj`, `….ff.net_2`) ->
    its diffusers module path + `.lora` (`….ff.net.0.proj.lora`, `….ff.net.2.lora`)."""
    if _TARGET_FF.search(layer + ".kernel"):
        return re.sub(r"_(\d+)(?=\.|$)", r".\1", layer) + ".lora"
    stem, proj = layer.rsplit(".", 1)
    stem = re.sub(r"_(\d+)(?=\.|$)", r".\1", stem)
    return f"{stem}.processor.{'to_out' if proj == 'to_out_0' else proj}_lora"


def flax_layer(key_prefix):
    """Inverse of diffusers_key."""
    if ".processor." not in key_prefix:
        return re.sub(r"\.(\d+)(?=\.|$)", r"_\1", key_prefix[:-len(".lora")])
    stem, proc = key_prefix.rsplit(".processor.", 1)
    proj = proc[:-len("_lora")]
    stem = re.sub(r"\.(\d+)(?=\.|$)", r"_\1", stem)
    return f"{stem}.{'to_out_0' if proj == 'to_out' else proj}"


def diffusers_keys(shapes, rank, targets="attn"):
    """The state-dict keys and shapes of an adapter file: {key: shape} with down (r, in) and up (out, r) per target."""
    out = OrderedDict()
    for n in lora_targets(shapes, targets):
        K, N = shapes[n]
        pre = diffusers_key(n[:-len(".kernel")])
        out[pre + ".down.weight"] = (rank, K)
        out[pre + ".up.weight"] = (N, rank)
    return out


class LoraStore:
    """Adapters of one U-Net: A / B in one flat fp32 buffer (16-byte aligned views, ParamStore), a gradient buffer of the same layout, the frozen
    W0 copy of the adapted tensors and the merge table.  Attaching it (`unet.lora = store`) switches the U-Net's backward to adapter gradients."""

    def __init__(self, unet, rank, alpha=None, seed=0, targets="attn"):
        self.unet = unet
        self.rank = check_rank(rank)
        self.alpha = alpha
        self.scale = lora_scale(self.rank, alpha)
        self.target_set = check_targets(targets)
        self.has_ff = targets == "attn_ff"         # the backward then also takes the adapter gradients of ff.net_0.proj / ff.net_2
        self.targets = lora_targets(unet.params.shapes, targets)
        dev = unet.params.flat.device
        self.shapes = adapter_shapes(unet.params.shapes, self.rank, targets)
        self.params = ParamStore(self.shapes, dev)
        self.grads = ParamStore(self.shapes, dev)
        self.base = ParamStore(OrderedDict((n, unet.params.shapes[n]) for n in self.targets), dev)
        self.n_params = self.params.n_params
        self.init(seed)
        self.capture_base()
        self._table = None
        unet.lora = self

    def layer(self, kernel_name):
        """(A, B, dA, dB) of the adapted layer whose Flax kernel is `kernel_name`."""
        pre = kernel_name[:-len(".kernel")]
        return self.params[pre + ".A"], self.params[pre + ".B"], self.grads[pre + ".A"], self.grads[pre + ".B"]

    def init(self, seed=0):
        """diffusers' LoRALinearLayer initialisation: down ~ N(0, (1 / r)^2), up = 0 — drawn on the host from `seed`, so every rank holds the
        same adapters.  One stream in target order: the attention adapters come first, so they are the same under both target sets."""
        g = torch.Generator().manual_seed(int(seed))
        for n, v in self.params.views.items():
            if n.endswith(".A"):
                # drawn in the file layout (r, in) like nn.init.normal_(down.weight), stored transposed
                v.copy_(torch.randn(v.shape[1], v.shape[0], generator=g).mul_(1.0 / self.rank).t())
            else:
                v.zero_()
        self.grads.flat.zero_()

    def capture_base(self):
        """W0 := the adapted tensors of the U-Net as they are now (the pretrained weights; call after loading them)."""
        for n in self.targets:
            self.base[n].copy_(self.unet.params[n])

    def table(self):
        if self._table is None:
            P = self.unet.params
            self._table = L.lora_table([(self.base[n], P[n], *self.layer(n)[:2], self.scale) for n in self.targets])
        return self._table

    def merge(self):
        """W' = W0 + s A B for every target (one launch), then a repack of the adapted tensors only (bf16 datapaths)."""
        L.lora_merge(self.table())
        if L.current_datapath() != "fp32":
            self.unet.params.pack_bf16(names=self.targets)

    # ---------------------------------------------------------------------------------------------- files
    def state_dict(self):
        """Host tensors in diffusers' attention-processor layout: `<prefix>.down.weight` (r, in) = A^T, `<prefix>.up.weight` (out, r) = B^T."""
        sd = OrderedDict()
        for n in self.targets:
            A, B = self.layer(n)[:2]
            pre = diffusers_key(n[:-len(".kernel")])
            sd[pre + ".down.weight"] = A.detach().t().contiguous().cpu()
            sd[pre + ".up.weight"] = B.detach().t().contiguous().cpu()
        return sd

    def load_state_dict(self, sd):
        want = diffusers_keys(self.unet.params.shapes, self.rank, self.target_set)
        missing = [k for k in want if k not in sd]
        if missing:
            raise KeyError(f"adapter file lacks {len(missing)} keys, e.g. {missing[0]}")
        for k, shp in want.items():
            if tuple(sd[k].shape) != tuple(shp):
                raise ValueError(f"{k}: expected {shp}, got {tuple(sd[k].shape)}")
        for n in self.targets:
            A, B = self.layer(n)[:2]
            pre = diffusers_key(n[:-len(".kernel")])
            A.copy_(torch.as_tensor(sd[pre + ".down.weight"], dtype=torch.float32).t())
            B.copy_(torch.as_tensor(sd[pre + ".up.weight"], dtype=torch.float32).t())

    def save(self, path, synthetic_weights=False):
        """synthetic_weights: the base weights were random-init (recorded in the file's metadata, as in the full checkpoints)."""
        from safetensors.torch import save_file
        save_file(dict(self.state_dict()), path, metadata={"format": "diffusers-attn-processor-lora", "rank": str(self.rank),
                                                           "alpha": str(self.alpha if self.alpha is not None else self.rank),
                                                           "targets": self.target_set,
                                                           "synthetic_weights": str(bool(synthetic_weights))})
        return path


def read_lora_file(path):
    """(state dict, rank, alpha, targets) of an adapter file written by LoraStore.save.  The target set comes from the metadata, or — a file
    without the field — from the keys: feed-forward keys make it "attn_ff", an attention-only file (every older file) reads as "attn"."""
    from safetensors import safe_open
    from safetensors.torch import load_file
    sd = load_file(path)
    with safe_open(path, "pt") as f:
        meta = f.metadata() or {}
    downs = [v for k, v in sd.items() if k.endswith(".down.weight")]
    if not downs:
        raise ValueError(f"{path} holds no LoRA down weights")
    rank = int(meta.get("rank", downs[0].shape[0]))
    alpha = float(meta["alpha"]) if "alpha" in meta else float(rank)
    targets = meta.get("targets") or ("attn_ff" if any(".ff.net." in k for k in sd) else "attn")
    return sd, rank, alpha, check_targets(targets)


def load_lora(unet, path, scale=1.0):
    """Fold a saved adapter into `unet` for sampling: W' = W + scale * (alpha / r) * A B on every target, then a repack of those tensors.
    Returns the LoraStore (detached from the backward: `unet.lora` is reset)."""
    sd, rank, alpha, targets = read_lora_file(path)
    prev = getattr(unet, "lora", None)
    store = LoraStore(unet, rank, alpha=alpha * float(scale), targets=targets)
    store.load_state_dict(sd)
    store.merge()
    unet.lora = prev
    return store


def reject_lora_flags(argv):
    """The RWR fine-tuning path (pipeline/finetune.py) trains the full U-Net only: a LoRA flag there is an error, not a silent no-op."""
    bad = [a for a in argv if a.split("=", 1)[0] in ("--lora_rank", "--lora_alpha", "--lora_targets")]
    if bad:
        raise SystemExit(f"{bad[0].split('=', 1)[0]}: LoRA is available for pipeline/policy_gradient.py only; the RWR path "
                         "(pipeline/finetune.py) fine-tunes every U-Net parameter")
