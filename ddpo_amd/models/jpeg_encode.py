"""JPEG files of a batch of images on the engine's kernels (`ddpo_jpeg_encode`): the bytes PIL's `Image.save(buf, "JPEG", quality=q)` writes,
byte for byte, without the images leaving the device — only the compressed files cross to the host.  What the LLaVA rewards send to their
server (training/callbacks.py: llava_bertscore_device, llava_vqa_device).

A `DeviceScorer` (models/device_scorer.py) like JpegSizer: private HIP stream, a workspace and a file buffer of its own.
"""
import torch

from .. import lib as L
from .device_scorer import DeviceScorer
from .jpeg_size import jpeg_images


class JpegEncoder(DeviceScorer):
    def __init__(self, quality=80, device="cuda", stride=None):
        """`stride`: bytes of a row of the file buffer; default H * W * 3 + 625, which only a pathological image exceeds.  A batch with a longer
        file is encoded once more with rows of lib.jpeg_encode_max_bytes (`retries` counts those)."""
        if int(quality) != quality or not 1 <= quality <= 100:
            raise ValueError(f"quality must be an integer in 1..100, got {quality!r}")
        if stride is not None and (int(stride) != stride or stride < L.JPEG_FIXED_BYTES):
            raise ValueError(f"stride must be an integer >= {L.JPEG_FIXED_BYTES}, got {stride!r}")
        super().__init__(device)
        self.quality = int(quality)
        self.stride = None if stride is None else int(stride)
        self.workspace = None
        self.files = None
        self.retries = 0

    def _workspace(self, n, h, w):
        return self._buffer("workspace", L.jpeg_size_workspace_bytes(n, h, w))              # ValueError names the multiple-of-16 rule

    def _files(self, n, stride):
        return self._buffer("files", n * stride)[:n * stride].view(n, stride)

    def _encode(self, dev_images, stride):
        """-> (files on the device, lengths on the host), on the current (this encoder's) stream"""
        n, h, w = dev_images.shape[:3]
        files, lengths = L.jpeg_encode(dev_images, self.quality, workspace=self._workspace(n, h, w), files=self._files(n, stride))
        return files, lengths.cpu()

    def __call__(self, images, ready=None):
        """images (N,H,W,3): a numpy array (float in [0,1], truncated to uint8 as the host reward does, or uint8; uploaded as uint8) or a CUDA
        tensor (float32 in [0,1] or uint8; no host trip).  Returns the N files as a list of bytes.
        A CUDA tensor is read on this encoder's stream after `ready` — an event recorded on the producing stream once the images were complete;
        default: one recorded now on the caller's current stream — and is referenced here until that work has finished."""
        images, ready = jpeg_images(images, ready, "JpegEncoder")
        n, h, w, _ = L._jpeg_encode_args(images, self.quality)
        with self.on_stream(ready):
            if not isinstance(images, torch.Tensor):
                images = torch.from_numpy(images).to(self.device)
            stride = self.stride if self.stride is not None else h * w * 3 + L.JPEG_FIXED_BYTES
            files, lengths = self._encode(images, stride)
            if int(lengths.max()) > stride:                     # rows held prefixes only: once more with rows no file exceeds
                self.retries += 1
                files, lengths = self._encode(images, L.jpeg_encode_max_bytes(h, w))
            host = files[:, :int(lengths.max())].cpu()          # narrowed to the longest file: the padding of the rows stays on the device
        host = host.numpy()
        return [host[i, :int(lengths[i])].tobytes() for i in range(n)]
