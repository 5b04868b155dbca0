"""The symmetry rewards' device work (training/callbacks.py: mirror_device, mirror_corr_device, rotational_corr_device, rotational_device).

`SymmetryStats`: four exact integer sums per image (`ddpo_symmetry_stats`, csrc/symmetry.hip) from which the pixel rewards follow on the host —
the wrapped uint8 squared difference the reference optimises, the true squared difference, the correlation.  `RotationalEmbedder`: CLIP image
features of the four right-angle turns of every image (`ddpo_rotate4_u8` -> `ddpo_clip_preprocess` -> the vision tower of the aesthetic reward).

Like the other on-device scorers they run on a private HIP stream with scratch of their own: the reward callback is evaluated by a worker thread
while the main thread samples the next batch, and the two must not share a stream or scratch space.  Host arrays never need the GPU for the sums
(the serial host entries compute them) and take the reference's own PIL steps for the features.
"""
import os

import numpy as np
import torch

from .. import lib as L
from .clip_vision import ClipVisionTower, VisionConfig, device_images, preprocess

DEGREES = (0, 90, 180, 270)       # the order in which the reference concatenates its rotated copies


def rotated_pixel_values(images, size):
    """Host input of the tower for float images (N,H,W,3) in [0,1]: the batch truncated to bytes, every image turned by PIL.Image.rotate through
    DEGREES — block k holds all N images at DEGREES[k] — and CLIP-preprocessed.  (4N, 3, size, size) float32."""
    from PIL import Image
    u8 = (np.asarray(images) * 255).astype(np.uint8)
    return preprocess([np.asarray(Image.fromarray(im).rotate(angle)) for angle in DEGREES for im in u8], size)      # PIL: byte-identical resize


class SymmetryStats:
    def __init__(self, mode):
        """mode: "mirror" (the partner of a byte is its left-right mirror image) or "rot180" (its image under a half turn)."""
        if mode not in L.SYMMETRY_MODES:
            raise ValueError(f"mode must be one of {sorted(L.SYMMETRY_MODES)}, got {mode!r}")
        self.mode = mode
        self.stream = None            # created with the first device batch: host batches need no GPU
        self.workspace = None

    def _workspace(self, n, h, w, device):
        nb = L.symmetry_stats_workspace_bytes(n, h, w, self.mode)
        if self.workspace is None or self.workspace.numel() < nb or self.workspace.device != device:
            self.workspace = torch.empty(nb, dtype=torch.uint8, device=device)
        return self.workspace

    def __call__(self, images, ready=None):
        """images (N,H,W,3): a numpy array (float in [0,1], truncated to uint8 as the host rewards do, or uint8; summed on the host) or a CUDA
        tensor (float32 in [0,1] or uint8; no host trip).  Returns the (N, 4) int64 sums of lib.symmetry_stats on the host.
        A CUDA tensor is read on this object's stream after `ready` — an event recorded on the producing stream once the images were complete;
        default: one recorded now on the caller's current stream — and is referenced here until that work has finished."""
        if not isinstance(images, torch.Tensor):
            a = np.asarray(images)
            if np.issubdtype(a.dtype, np.floating):
                a = (a * 255).astype(np.uint8)                  # the reference's truncation
            return L.symmetry_stats_host(np.ascontiguousarray(a), self.mode)
        images, ready = device_images(images, ready, "SymmetryStats")
        if self.stream is None or self.stream.device != images.device:
            self.stream = torch.cuda.Stream(images.device)
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(ready)
            ws = self._workspace(*images.shape[:3], images.device)
            stats = L.symmetry_stats(images, self.mode, workspace=ws).cpu()
        self.stream.synchronize()
        del images
        return stats.numpy()


class RotationalEmbedder:
    def __init__(self, weights_dir=None, cache="cache", seed=0, device="cuda", config="vit-l/14", clip_state=None):
        """`clip_state`: a state dict handed in directly (tests); otherwise the CLIP checkpoint is looked up exactly as ClipScorer does
        (`weights_dir` / $DDPO_AESTHETIC_WEIGHTS `/clip`, else the HF cache; nothing is downloaded).  Missing weights raise, unless
        DDPO_ALLOW_SYNTHETIC=1 asks for a seeded random-init tower (`synthetic` is then True)."""
        from .laion import REPO_ROOT, _load_clip_state, find_weights, synthetic_state_dicts
        self.device = torch.device(device)
        self.cfg = VisionConfig.named(config)
        self.synthetic = False
        if clip_state is None:
            clip_dir, _ = find_weights(weights_dir, cache)
            clip_state = _load_clip_state(clip_dir) if clip_dir else None
            if clip_state is None:
                from ..utils.serialization import allow_synthetic
                if not allow_synthetic():
                    raise FileNotFoundError(
                        f"rotational reward: the CLIP ViT-L/14 checkpoint (openai/clip-vit-large-patch14) not found (looked for `clip/` in "
                        f"weights_dir / $DDPO_AESTHETIC_WEIGHTS, then for a snapshot in '{os.path.join(REPO_ROOT, cache)}' and the HF cache; nothing "
                        f"is downloaded).  Set DDPO_ALLOW_SYNTHETIC=1 to score with a seeded RANDOM-INIT tower (benchmarks / tests only)")
                print("[ models/symmetry ] WARNING: DDPO_ALLOW_SYNTHETIC=1 and no CLIP checkpoint on disk — embedding with a seeded random-init "
                      "CLIP vision tower; rewards are meaningless")
                clip_state, _ = synthetic_state_dicts(self.cfg, self.cfg.proj, seed)
                self.synthetic = True
        self.stream = torch.cuda.Stream(self.device)          # (after the weight lookup: a missing-weights refusal needs no GPU)
        with torch.cuda.stream(self.stream):
            self.tower = ClipVisionTower(self.cfg, self.device)
            self.tower.load_state_dict(clip_state)
        self.stream.synchronize()

    def __call__(self, images, ready=None):
        """images (N,H,W,3) in [0,1]: a float host array (turned by PIL and preprocessed on the host, the reference's own steps) or a square CUDA
        tensor, float32 or uint8 (turned and preprocessed on the device, no host trip; the same features bit for bit) -> (4N, proj) float32
        features on the host, row k N + n for image n turned by DEGREES[k].
        A CUDA tensor is read on this object's stream after `ready`, as for SymmetryStats."""
        cfg = self.cfg
        if isinstance(images, torch.Tensor):
            images, ready = device_images(images, ready, "RotationalEmbedder")
            with torch.cuda.stream(self.stream), L.fp32_class_datapath():
                self.stream.wait_event(ready)
                turned = L.rotate4_u8(images)                                     # ValueError for non-square images
                patches = L.clip_preprocess(turned, cfg.image, cfg.patch, cfg.k_pad)
                feats = self.tower.forward_patches(patches).cpu()
            self.stream.synchronize()
            del images
            return feats.numpy()
        px = rotated_pixel_values(images, cfg.image)
        with torch.cuda.stream(self.stream), L.fp32_class_datapath():
            feats = self.tower(torch.from_numpy(px).to(self.device)).cpu()
        self.stream.synchronize()
        return feats.numpy()
