"""JPEG file size of a batch of images on the engine's kernels (`ddpo_jpeg_size`): the integer PIL's `Image.save(buf, "JPEG", quality=q)` would
return the length of, without producing the file and without the images leaving the device.  The reward of `compressed-animals` /
`uncompressed-animals` (training/callbacks.py: jpeg_device, neg_jpeg_device).

A `DeviceScorer` (models/device_scorer.py): private HIP stream, workspace of its own, any number of sizers at once.
"""
import numpy as np
import torch

from .. import lib as L
from .device_scorer import DeviceScorer, device_images, truncate_u8


def jpeg_images(images, ready, who):
    """The batch a JPEG scorer works on, with the event to wait for: a CUDA tensor as it is (`device_images`), a host array as contiguous bytes
    (floats in [0,1] truncated as the host reward does, callbacks.encode_jpeg) with no event — its upload is the scorer's own work."""
    if isinstance(images, torch.Tensor):
        return device_images(images, ready, who)
    a = np.asarray(images)
    if np.issubdtype(a.dtype, np.floating):
        assert np.abs(a).max() <= 1.0
    a = truncate_u8(a)
    if a.dtype != np.uint8:
        raise ValueError(f"{who} takes float or uint8 images, got {a.dtype}")
    return np.ascontiguousarray(a), None


class JpegSizer(DeviceScorer):
    def __init__(self, quality=95, device="cuda"):
        if int(quality) != quality or not 1 <= quality <= 100:
            raise ValueError(f"quality must be an integer in 1..100, got {quality!r}")
        super().__init__(device)
        self.quality = int(quality)
        self.workspace = None

    def _workspace(self, n, h, w):
        return self._buffer("workspace", L.jpeg_size_workspace_bytes(n, h, w))              # ValueError names the multiple-of-16 rule

    def __call__(self, images, ready=None):
        """images (N,H,W,3): a numpy array (float in [0,1], truncated to uint8 as the host reward does, or uint8; uploaded as uint8) or a CUDA
        tensor (float32 in [0,1] or uint8; no host trip).  Returns (N,) int64 on the host.
        A CUDA tensor is read on this scorer's stream after `ready` — an event recorded on the producing stream once the images were complete;
        default: one recorded now on the caller's current stream — and is referenced here until that work has finished."""
        images, ready = jpeg_images(images, ready, "JpegSizer")
        L._jpeg_size_args(images, self.quality)
        with self.on_stream(ready):
            if not isinstance(images, torch.Tensor):
                images = torch.from_numpy(images).to(self.device)
            sizes = L.jpeg_size(images, self.quality, workspace=self._workspace(*images.shape[:3])).cpu()
        return sizes.numpy()
