"""CLIPScore prompt-alignment reward on the engine's kernels: score = exp(logit_scale) * cos(image_embeds, text_embeds), the diagonal of
transformers' `CLIPModel(...).logits_per_image`.  Image side: models/clip_vision.py (the tower of the aesthetic reward).  Text side:
models/clip_text.py.  Cosine: `ddpo_cosine_rows` (one launch instead of two normalisations and a batched dot product).

A `DeviceScorer` (models/device_scorer.py) like the aesthetic scorer: it runs on a private HIP stream.

Weights: the ONE checkpoint the aesthetic reward already uses, looked up the same way (`laion.load_clip_checkpoint`): `<weights_dir>/clip/` with
`weights_dir` = the argument, else $DDPO_AESTHETIC_WEIGHTS, then an HF cache snapshot of `openai/clip-vit-large-patch14`.  It carries both
towers, `text_projection` and `logit_scale`.  The tokenizer is transformers' `CLIPTokenizer` read from the same directory (`vocab.json` +
`merges.txt`).  Missing weights — or real weights without their vocabulary — raise before any GPU work, unless DDPO_ALLOW_SYNTHETIC=1 asks for
seeded random-init towers with the byte-level stand-in tokenizer (benchmarks / tests; `synthetic` is then True and the callback's info says
so).  With a real checkpoint the reward is exactly as real as the files found on disk; nothing is downloaded.

Prompt cache.  The prompt sets of the alignment datasets are small (nouns x activities: a few hundred strings), so the projected text embedding
of every distinct prompt is kept on the device in a bounded LRU and the text tower runs only on the misses of a batch.  A cached score is
bit-identical to an uncached one because an embedding never depends on what shares its launch: every kernel of the towers computes an output
row from that row's inputs alone (LayerNorm, the element-wise kernels and the gathers are row-wise; attention works per (sample, head); a GEMM
sums each output element over k in an order fixed by the launch shape, not by the row's position or neighbours).  The launch SHAPE does
matter on the bf16x3 datapath — tile and split-K choices follow the row count, and a different split is a different fp32 summation order — so
both towers always run on chunks of a fixed size (TEXT_CHUNK prompts, IMAGE_CHUNK images), a short chunk being padded with the empty prompt /
a repeat of its last image.  Scores therefore do not depend on batch size, batch order or cache state.
"""
import math
import os
from collections import OrderedDict

import numpy as np
import torch

from .. import lib as L
from .clip_text import ClipTextTower, TextConfig, synthetic_text_state
from .clip_vision import ClipVisionTower, VisionConfig, preprocess
from .device_scorer import DeviceScorer, device_images
from .laion import load_clip_checkpoint

TEXT_CHUNK = 8            # prompts per text-tower launch sequence (616 rows)
IMAGE_CHUNK = 4           # images per image-tower launch sequence (1028 rows at ViT-L/14)
SYNTHETIC_LOGIT_SCALE = math.log(1 / 0.07)      # CLIP's initial value; the trained checkpoint holds ln(100)


class PromptCache:
    """Bounded least-recently-used map prompt string -> embedding row.  `embed(list_of_distinct_prompts)` must return one row per prompt and
    is called at most once per `lookup`, on that call's distinct misses only (in order of first appearance)."""

    def __init__(self, embed, capacity=4096):
        if capacity < 1:
            raise ValueError("capacity must be at least 1")
        self.embed, self.capacity = embed, int(capacity)
        self.rows = OrderedDict()
        self.misses = 0                   # prompts the tower was run on so far

    def __len__(self):
        return len(self.rows)

    def lookup(self, prompts):
        prompts = [str(p) for p in prompts]
        got = {}
        for p in prompts:
            if p in self.rows and p not in got:
                self.rows.move_to_end(p)
                got[p] = self.rows[p]
        missing = list(OrderedDict.fromkeys(p for p in prompts if p not in got))
        self.misses += len(missing)
        if missing:
            new = self.embed(missing)
            if len(new) != len(missing):
                raise RuntimeError(f"embed returned {len(new)} rows for {len(missing)} prompts")
            for p, row in zip(missing, new):
                got[p] = self.rows[p] = row
                while len(self.rows) > self.capacity:
                    self.rows.popitem(last=False)
        return [got[p] for p in prompts]


def load_clip_tokenizer(clip_dir):
    """`CLIPTokenizer` from the checkpoint directory when its vocabulary files are there, else None."""
    if not clip_dir or not all(os.path.exists(os.path.join(clip_dir, f)) for f in ("vocab.json", "merges.txt")):
        return None
    from transformers import CLIPTokenizer
    return CLIPTokenizer.from_pretrained(clip_dir)


class ClipScorer(DeviceScorer):
    def __init__(self, weights_dir=None, cache="cache", seed=0, device="cuda", config="vit-l/14", clip_state=None, tokenizer=None,
                 logit_scale=None, cache_size=4096):
        """`clip_state` (+ optionally `tokenizer`, `logit_scale`): a state dict handed in directly (tests); otherwise files are looked up (see
        the module docstring).  `logit_scale` overrides the checkpoint's (the log of the factor, as the checkpoint stores it)."""
        self.vcfg, self.tcfg = VisionConfig.named(config), TextConfig.named(config)
        if self.vcfg.proj != self.tcfg.proj:
            raise ValueError(f"image and text projections differ: {self.vcfg.proj} vs {self.tcfg.proj}")
        self.synthetic = False
        if clip_state is None:
            clip_state, clip_dir, _, self.synthetic = load_clip_checkpoint("clip_score", self.vcfg, weights_dir, cache, seed)
            if self.synthetic:            # scored through the byte-level stand-in tokenizer below
                clip_state.update(synthetic_text_state(self.tcfg, seed))
                clip_state["logit_scale"] = torch.tensor(SYNTHETIC_LOGIT_SCALE)
            elif tokenizer is None:
                tokenizer = load_clip_tokenizer(clip_dir)
                if tokenizer is None:
                    raise FileNotFoundError(f"clip_score reward: the CLIP checkpoint in '{clip_dir}' has no tokenizer files (vocab.json, merges.txt); "
                                            f"real weights are never scored through the byte-level stand-in tokenizer")
        if tokenizer is None:
            from .text import ByteTokenizer
            tokenizer = ByteTokenizer()
        self.tokenizer = tokenizer
        if logit_scale is None:
            if "logit_scale" not in clip_state:
                raise KeyError("the CLIP state dict holds no `logit_scale`")
            logit_scale = float(torch.as_tensor(clip_state["logit_scale"]).double())
        self.logit_scale = float(logit_scale)
        super().__init__(device)      # (after the weight lookup: a missing-weights refusal needs no GPU)
        with self.on_stream():
            self.vision = ClipVisionTower(self.vcfg, self.device)
            self.vision.load_state_dict(clip_state)
            self.text = ClipTextTower(self.tcfg, self.device)
            self.text.load_state_dict(clip_state)
        self.prompts = PromptCache(self._embed_prompts, cache_size)

    def tokenize(self, prompts):
        return np.asarray(self.tokenizer(list(prompts), padding="max_length", max_length=self.tcfg.positions, truncation=True,
                                         return_tensors="np").input_ids)

    def _embed_prompts(self, prompts):
        """Text embeddings of distinct prompts, TEXT_CHUNK at a time (a short chunk padded with the empty prompt).  Current stream."""
        rows = []
        for i in range(0, len(prompts), TEXT_CHUNK):
            part = list(prompts[i:i + TEXT_CHUNK])
            emb = self.text(self.tokenize(part + [""] * (TEXT_CHUNK - len(part))))
            rows += [emb[j] for j in range(len(part))]
        return rows

    def _embed_images(self, px):
        """Image embeddings, IMAGE_CHUNK at a time (a short chunk padded by repeating its last image).  Current stream."""
        out = torch.empty(px.shape[0], self.vcfg.proj, dtype=torch.float32, device=self.device)
        for i in range(0, px.shape[0], IMAGE_CHUNK):
            part = px[i:i + IMAGE_CHUNK]
            m = part.shape[0]
            if m < IMAGE_CHUNK:
                part = torch.cat([part, part[-1:].expand(IMAGE_CHUNK - m, -1, -1, -1)]).contiguous()
            out[i:i + m] = self.vision(part)[:m]
        return out

    def _embed_patches(self, patches, n):
        """_embed_images for a patch matrix (lib.clip_preprocess): the same chunks of IMAGE_CHUNK images, cut out of the matrix's rows; a short
        chunk is padded by repeating the rows of its last image.  Current stream."""
        gg = self.vcfg.grid * self.vcfg.grid
        out = torch.empty(n, self.vcfg.proj, dtype=torch.float32, device=self.device)
        for i in range(0, n, IMAGE_CHUNK):
            m = min(IMAGE_CHUNK, n - i)
            part = patches[i * gg:(i + m) * gg]
            if m < IMAGE_CHUNK:
                part = torch.cat([part] + [part[-gg:]] * (IMAGE_CHUNK - m))
            out[i:i + m] = self.vision.forward_patches(part)[:m]
        return out

    def __call__(self, images, prompts, return_cosine=False, ready=None):
        """images (N,H,W,3) in [0,1]: a float32 host array (preprocessed on the host, PIL) or a CUDA tensor, float32 or uint8 (preprocessed by
        `lib.clip_preprocess`, no host trip; the same scores bit for bit), prompts: N strings -> (N,) float32 scores (host) [, (N,) float32 raw
        cosines].  A CUDA tensor is read on this scorer's stream after `ready` — an event recorded on the producing stream once the images were
        complete; default: one recorded now on the caller's current stream — and is referenced here until that work has finished."""
        if len(images) != len(prompts):
            raise ValueError(f"{len(images)} images but {len(prompts)} prompts")
        on_device = isinstance(images, torch.Tensor)
        if on_device:
            images, ready = device_images(images, ready, "ClipScorer")
        else:
            px, ready = preprocess(np.asarray(images, dtype=np.float32), self.vcfg.image), None      # host, PIL: byte-identical resize
        with self.on_stream(ready), L.fp32_class_datapath():
            if on_device:
                img = self._embed_patches(L.clip_preprocess(images, self.vcfg.image, self.vcfg.patch, self.vcfg.k_pad), images.shape[0])
            else:
                img = self._embed_images(torch.from_numpy(px).to(self.device))
            txt = torch.stack(self.prompts.lookup(prompts))
            scores = L.cosine_rows(img, txt, scale=math.exp(self.logit_scale)).cpu().numpy()
            cosine = L.cosine_rows(img, txt).cpu().numpy()
        return (scores, cosine) if return_cosine else scores
