"""The symmetry rewards' device work (training/callbacks.py: mirror_device, mirror_corr_device, rotational_corr_device, rotational_device).

`SymmetryStats`: four exact integer sums per image (`ddpo_symmetry_stats`, csrc/symmetry.hip) from which the pixel rewards follow on the host —
the wrapped uint8 squared difference the reference optimises, the true squared difference, the correlation.  `RotationalEmbedder`: CLIP image
features of the four right-angle turns of every image (`ddpo_rotate4_u8` -> `ddpo_clip_preprocess` -> the vision tower of the aesthetic reward).

Both are `DeviceScorer`s (models/device_scorer.py: private HIP stream, scratch of their own).  Host arrays never need the GPU for the sums (the
serial host entries compute them) and take the reference's own PIL steps for the features.
"""
import numpy as np
import torch

from .. import lib as L
from .clip_vision import ClipVisionTower, VisionConfig, preprocess
from .device_scorer import DeviceScorer, device_images, truncate_u8

DEGREES = (0, 90, 180, 270)       # the order in which the reference concatenates its rotated copies


def rotated_pixel_values(images, size):
    """Host input of the tower for float images (N,H,W,3) in [0,1]: the batch truncated to bytes, every image turned by PIL.Image.rotate through
    DEGREES — block k holds all N images at DEGREES[k] — and CLIP-preprocessed.  (4N, 3, size, size) float32."""
    from PIL import Image
    u8 = truncate_u8(images)
    return preprocess([np.asarray(Image.fromarray(im).rotate(angle)) for angle in DEGREES for im in u8], size)      # PIL: byte-identical resize


class SymmetryStats(DeviceScorer):
    def __init__(self, mode):
        """mode: "mirror" (the partner of a byte is its left-right mirror image) or "rot180" (its image under a half turn)."""
        if mode not in L.SYMMETRY_MODES:
            raise ValueError(f"mode must be one of {sorted(L.SYMMETRY_MODES)}, got {mode!r}")
        super().__init__()            # the stream is created with the first device batch: host batches need no GPU
        self.mode = mode
        self.workspace = None

    def _workspace(self, n, h, w):
        return self._buffer("workspace", L.symmetry_stats_workspace_bytes(n, h, w, self.mode))

    def __call__(self, images, ready=None):
        """images (N,H,W,3): a numpy array (float in [0,1], truncated to uint8 as the host rewards do, or uint8; summed on the host) or a CUDA
        tensor (float32 in [0,1] or uint8; no host trip).  Returns the (N, 4) int64 sums of lib.symmetry_stats on the host.
        A CUDA tensor is read on this object's stream after `ready` — an event recorded on the producing stream once the images were complete;
        default: one recorded now on the caller's current stream — and is referenced here until that work has finished."""
        if not isinstance(images, torch.Tensor):
            return L.symmetry_stats_host(np.ascontiguousarray(truncate_u8(images)), self.mode)
        images, ready = device_images(images, ready, "SymmetryStats")
        with self.on_stream(ready, device=images.device):
            stats = L.symmetry_stats(images, self.mode, workspace=self._workspace(*images.shape[:3])).cpu()
        return stats.numpy()


class RotationalEmbedder(DeviceScorer):
    def __init__(self, weights_dir=None, cache="cache", seed=0, device="cuda", config="vit-l/14", clip_state=None):
        """`clip_state`: a state dict handed in directly (tests); otherwise the CLIP checkpoint is looked up exactly as ClipScorer does
        (laion.load_clip_checkpoint: missing weights raise, unless DDPO_ALLOW_SYNTHETIC=1 asks for a seeded random-init tower; `synthetic` is
        then True)."""
        from .laion import load_clip_checkpoint
        self.cfg = VisionConfig.named(config)
        self.synthetic = False
        if clip_state is None:
            clip_state, _, _, self.synthetic = load_clip_checkpoint("rotational", self.cfg, weights_dir, cache, seed)
        super().__init__(device)      # (after the weight lookup: a missing-weights refusal needs no GPU)
        with self.on_stream():
            self.tower = ClipVisionTower(self.cfg, self.device)
            self.tower.load_state_dict(clip_state)

    def __call__(self, images, ready=None):
        """images (N,H,W,3) in [0,1]: a float host array (turned by PIL and preprocessed on the host, the reference's own steps) or a square CUDA
        tensor, float32 or uint8 (turned and preprocessed on the device, no host trip; the same features bit for bit) -> (4N, proj) float32
        features on the host, row k N + n for image n turned by DEGREES[k].
        A CUDA tensor is read on this object's stream after `ready`, as for SymmetryStats."""
        cfg = self.cfg
        if isinstance(images, torch.Tensor):
            images, ready = device_images(images, ready, "RotationalEmbedder")
            with self.on_stream(ready), L.fp32_class_datapath():
                turned = L.rotate4_u8(images)                                     # ValueError for non-square images
                patches = L.clip_preprocess(turned, cfg.image, cfg.patch, cfg.k_pad)
                feats = self.tower.forward_patches(patches).cpu()
        else:
            px = rotated_pixel_values(np.asarray(images, dtype=np.float32), cfg.image)
            with self.on_stream(), L.fp32_class_datapath():
                feats = self.tower(torch.from_numpy(px).to(self.device)).cpu()
        return feats.numpy()
