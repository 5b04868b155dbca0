"""Seeded images and cases shared by the thumbnail tests (tests/test_thumbnail_cpu.py, tests/test_gpu_thumbnail.py) and by
tests/golden/make_reference_thumbnail_goldens.py.  Images are regenerated from the case, never stored."""
import json
import os

import numpy as np

from _symmetry_cases import as_float, standin_features            # noqa: F401  (the same float images and stand-in features as `rotational`)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_thumbnail.json")

# name -> (N, H, W): the batches the golden was recorded on
CASES = {
    "kinds64": (5, 64, 64),        # noise, ramp, constant, 0 / 255 extremes, smooth
    "24x40": (2, 24, 40),          # non-square; thumbnails down to 1 x 2
    "17x23": (1, 17, 23),          # odd sizes; every thumbnail at 1/16 is 1 x 1
    "16x16": (2, 16, 16),          # the smallest image the reward takes
}

# input (H, W) -> outputs (oh, ow) of the resize itself: the kernel and its host twin against Pillow
RESIZES = [
    ((16, 16), [(4, 4), (2, 2), (1, 1)]),          # support wider than the image; a single output pixel
    ((17, 23), [(4, 5)]),                          # odd sizes; a 15-byte output row
    ((64, 64), [(16, 16), (8, 8), (4, 4)]),
    ((48, 80), [(12, 20)]),                        # non-square
    ((24, 40), [(24, 10)]),                        # identity on one axis
    ((8, 8), [(20, 12)]),                          # up-scale
    ((512, 512), [(128, 128), (64, 64), (32, 32)]),
]


def images_u8(name):
    """uint8 (N, H, W, 3) of a case."""
    n, h, w = CASES[name]
    rng = np.random.default_rng(sum(map(ord, "thumbnail" + name)))
    if name == "kinds64":
        yy, xx = np.mgrid[0:h, 0:w]
        ramp = np.stack([xx * 255 // (w - 1), yy * 255 // (h - 1), (xx + yy) * 255 // (h + w - 2)], -1)
        smooth = 127.5 + 100 * np.stack([np.sin(xx / 9.0) * np.cos(yy / 13.0), np.cos(xx / 11.0 + yy / 7.0), np.sin((xx - yy) / 15.0)], -1)
        return np.stack([rng.integers(0, 256, (h, w, 3)), ramp, np.full((h, w, 3), 77), rng.integers(0, 2, (h, w, 3)) * 255, smooth]).astype(np.uint8)
    return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def resize_input(h, w, n=1):
    """uint8 (n, h, w, 3) noise for a RESIZES entry."""
    return np.random.default_rng(1000 * h + w).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
