"""JPEG file size of a batch of images on the engine's kernels (`ddpo_jpeg_size`): the integer PIL's `Image.save(buf, "JPEG", quality=q)` would
return the length of, without producing the file and without the images leaving the device.  The reward of `compressed-animals` /
`uncompressed-animals` (training/callbacks.py: jpeg_device, neg_jpeg_device).

Like the other on-device scorers it runs on a private HIP stream with a workspace of its own: the reward callback is evaluated by a worker thread
while the main thread samples the next batch, and the two must not share a stream or scratch space.  The kernels keep no state outside the
workspace, so any number of sizers may run at once.
"""
import numpy as np
import torch

from .. import lib as L


class JpegSizer:
    def __init__(self, quality=95, device="cuda"):
        if int(quality) != quality or not 1 <= quality <= 100:
            raise ValueError(f"quality must be an integer in 1..100, got {quality!r}")
        self.quality = int(quality)
        self.device = torch.device(device)
        self.stream = torch.cuda.Stream(self.device)
        self.workspace = None

    def _workspace(self, n, h, w):
        nb = L.jpeg_size_workspace_bytes(n, h, w)              # ValueError names the multiple-of-16 rule
        if self.workspace is None or self.workspace.numel() < nb:
            self.workspace = torch.empty(nb, dtype=torch.uint8, device=self.device)
        return self.workspace

    def __call__(self, images, ready=None):
        """images (N,H,W,3): a numpy array (float in [0,1], truncated to uint8 as the host reward does, or uint8; uploaded as uint8) or a CUDA
        tensor (float32 in [0,1] or uint8; no host trip).  Returns (N,) int64 on the host.
        A CUDA tensor is read on this scorer's stream after `ready` — an event recorded on the producing stream once the images were complete;
        default: one recorded now on the caller's current stream — and is referenced here until that work has finished."""
        if isinstance(images, torch.Tensor):
            if not images.is_cuda:
                raise ValueError("JpegSizer takes a numpy array or a CUDA tensor")
            if not images.is_contiguous():
                raise ValueError("JpegSizer needs a contiguous N x H x W x 3 tensor")
            if ready is None:
                ready = torch.cuda.current_stream(images.device).record_event()
            dev_images = images
        else:
            a = np.asarray(images)
            if np.issubdtype(a.dtype, np.floating):
                assert np.abs(a).max() <= 1.0
                a = (a * 255).astype(np.uint8)                  # the reference's truncation (callbacks.encode_jpeg)
            if a.dtype != np.uint8:
                raise ValueError(f"JpegSizer takes float or uint8 images, got {a.dtype}")
            dev_images, ready = None, None
        shape = images.shape if dev_images is not None else a.shape
        L._jpeg_size_args(shape, self.quality)
        with torch.cuda.stream(self.stream):
            if dev_images is None:
                dev_images = torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
            else:
                self.stream.wait_event(ready)
            ws = self._workspace(*shape[:3])
            sizes = L.jpeg_size(dev_images, self.quality, workspace=ws).cpu()
        self.stream.synchronize()
        del dev_images
        return sizes.numpy()
