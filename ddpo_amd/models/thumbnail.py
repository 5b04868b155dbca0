"""The thumbnail reward's device work (training/callbacks.py: thumbnail, thumbnail_device).

`ThumbnailEmbedder`: CLIP image features of every image and of its thumbnails, shrunk by FACTORS with Pillow's 8-bit bicubic resize — each from
the original, not chained (`ddpo_resize_u8`, csrc/resize_u8.hip -> `ddpo_clip_preprocess`, which scales every thumbnail back up to the tower's
input -> the vision tower of the aesthetic reward).

A `DeviceScorer` (models/device_scorer.py: private HIP stream).  Host arrays take the reference's own PIL steps for the pixels.
"""
import numpy as np
import torch

from .. import lib as L
from .clip_vision import ClipVisionTower, VisionConfig, preprocess
from .device_scorer import DeviceScorer, device_images, truncate_u8

FACTORS = (4, 8, 16)              # the order in which the reference concatenates its thumbnails, after the originals
MIN_SIDE = max(FACTORS)           # a shorter side has no thumbnail at the last factor: side // 16 == 0, which Pillow refuses too


def _check_sides(who, h, w):
    if h < MIN_SIDE or w < MIN_SIDE:
        raise ValueError(f"{who}: height and width must be at least {MIN_SIDE} pixels (the thumbnail at 1/{MIN_SIDE} would be empty), got {h} x {w}")


def thumbnail_pixel_values(images, size):
    """Host input of the tower for float images (N,H,W,3) in [0,1]: the batch truncated to bytes, then the originals followed by every image
    shrunk by PIL.Image.resize to (W // d, H // d) for d in FACTORS — block k holds all N images at FACTORS[k - 1] — all CLIP-preprocessed.
    (4N, 3, size, size) float32."""
    from PIL import Image
    u8 = truncate_u8(images)
    _check_sides("thumbnail", *u8.shape[1:3])
    h, w = u8.shape[1:3]
    pils = [Image.fromarray(im) for im in u8]
    small = [np.asarray(pil.resize((w // d, h // d), resample=Image.BICUBIC)) for d in FACTORS for pil in pils]
    return preprocess(list(u8) + small, size)                                  # PIL: byte-identical resize


class ThumbnailEmbedder(DeviceScorer):
    def __init__(self, weights_dir=None, cache="cache", seed=0, device="cuda", config="vit-l/14", clip_state=None):
        """`clip_state`: a state dict handed in directly (tests); otherwise the CLIP checkpoint is looked up exactly as ClipScorer does
        (laion.load_clip_checkpoint: missing weights raise, unless DDPO_ALLOW_SYNTHETIC=1 asks for a seeded random-init tower; `synthetic` is
        then True)."""
        from .laion import load_clip_checkpoint
        self.cfg = VisionConfig.named(config)
        self.synthetic = False
        if clip_state is None:
            clip_state, _, _, self.synthetic = load_clip_checkpoint("thumbnail", self.cfg, weights_dir, cache, seed)
        super().__init__(device)      # (after the weight lookup: a missing-weights refusal needs no GPU)
        with self.on_stream():
            self.tower = ClipVisionTower(self.cfg, self.device)
            self.tower.load_state_dict(clip_state)

    def __call__(self, images, ready=None):
        """images (N,H,W,3) in [0,1], H and W at least 16: a float host array (shrunk by PIL and preprocessed on the host, the reference's own
        steps) or a CUDA tensor, float32 or uint8 (shrunk and preprocessed on the device, no host trip; the same features bit for bit) ->
        (4N, proj) float32 features on the host: rows 0 .. N - 1 the originals, row k N + n image n shrunk by FACTORS[k - 1].
        A CUDA tensor is read on this object's stream after `ready`, as for SymmetryStats."""
        cfg = self.cfg
        if isinstance(images, torch.Tensor):
            images, ready = device_images(images, ready, "ThumbnailEmbedder")
            n, h, w = (int(s) for s in images.shape[:3])
            _check_sides("ThumbnailEmbedder", h, w)
            rows = n * cfg.grid * cfg.grid                                           # patch rows of one block
            with self.on_stream(ready), L.fp32_class_datapath():
                patches = torch.empty(4 * rows, cfg.k_pad, dtype=torch.float32, device=self.device)
                L.clip_preprocess(images, cfg.image, cfg.patch, cfg.k_pad, out=patches[:rows])
                for k, d in enumerate(FACTORS, 1):
                    small = L.resize_u8(images, h // d, w // d)                      # each from the original
                    L.clip_preprocess(small, cfg.image, cfg.patch, cfg.k_pad, out=patches[k * rows:(k + 1) * rows])
                feats = self.tower.forward_patches(patches).cpu()
        else:
            px = thumbnail_pixel_values(np.asarray(images), cfg.image)
            with self.on_stream(), L.fp32_class_datapath():
                feats = self.tower(torch.from_numpy(px).to(self.device)).cpu()
        return feats.numpy()
