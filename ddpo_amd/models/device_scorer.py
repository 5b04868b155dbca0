"""What the on-device reward scorers share (JpegSizer, JpegEncoder, SymmetryStats, RotationalEmbedder, AestheticScorer, ClipScorer).

A reward callback is evaluated by a worker thread of the entrypoint while the main thread samples the next batch, and the two must not share a
stream or scratch space.  So every scorer is a `DeviceScorer`: it owns a private HIP stream and grow-only scratch buffers, reads a device batch
only after the event that says the batch is complete, and returns host values once its stream has drained.  The kernels keep no state outside
those buffers, so any number of scorers may run at once.
"""
import contextlib

import numpy as np
import torch


def device_images(images, ready, who):
    """What the on-device scorers accept as a device batch: a contiguous N x H x W x 3 CUDA tensor, float32 in [0,1] or uint8.  Returns it with the
    event its reader has to wait for (`ready`, else one recorded now on the caller's current stream)."""
    if not images.is_cuda:
        raise ValueError(f"{who} takes a numpy array or a CUDA tensor")
    if images.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"{who} takes float32 or uint8 device images, got {images.dtype}")
    if images.dim() != 4 or images.shape[3] != 3 or not images.is_contiguous():
        raise ValueError(f"{who} needs a contiguous N x H x W x 3 tensor, got shape {tuple(images.shape)}")
    if ready is None:
        ready = torch.cuda.current_stream(images.device).record_event()
    return images, ready


def truncate_u8(images):
    """Host images as bytes, the way the reference makes them: floats in [0,1] are TRUNCATED, (x * 255).astype(uint8); uint8 passes through."""
    a = np.asarray(images)
    return (a * 255).astype(np.uint8) if np.issubdtype(a.dtype, np.floating) else a


class DeviceScorer:
    def __init__(self, device=None):
        """`device`: where the private stream is created, now.  None: no GPU is touched here; the stream is created by the first
        `on_stream(device=...)` and follows the batches' device (a scorer whose host path needs no GPU).
        A scorer that looks up weights calls this after the lookup, so that a missing-weights refusal touches no GPU."""
        self.stream = self.device = None
        if device is not None:
            self._create_stream(device)

    def _create_stream(self, device):
        self.stream = torch.cuda.Stream(device)
        self.device = self.stream.device          # with its index: what tensors allocated there report

    @contextlib.contextmanager
    def on_stream(self, ready=None, device=None):
        """Run the body on this scorer's stream, after `ready` (the event of `device_images`) when the body reads a device batch, and return once
        the stream has drained: what the body copied to the host is complete, and the batch — referenced by the caller's frame until then — may
        be freed.  `device`: the batch's device, for a scorer created without one."""
        if device is not None and device != self.device:
            self._create_stream(device)
        with torch.cuda.stream(self.stream):
            if ready is not None:
                self.stream.wait_event(ready)
            yield
        self.stream.synchronize()

    def _buffer(self, name, nbytes):
        """The grow-only uint8 scratch kept as attribute `name`, at least `nbytes` long on this scorer's device: reallocated when it is too small
        or the device has changed."""
        buf = getattr(self, name, None)
        if buf is None or buf.numel() < nbytes or buf.device != self.device:
            buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            setattr(self, name, buf)
        return buf
