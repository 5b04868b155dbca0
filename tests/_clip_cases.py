"""Seeded images and geometry cases shared by the CLIP-preprocessing tests (tests/test_clip_preprocess_cpu.py, tests/test_gpu_clip_preprocess.py)
and by tests/golden/make_clip_preprocess_sha256.py.  Images are regenerated from (kind, seed, size), never stored."""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_preprocess_sha256.json")
PATCH = 14
KINDS = ("noise", "ramp", "saturated")
# (H, W) -> size, patch 14
SMALL = [
    ((64, 64), 56),        # downscale, ksize 7
    ((32, 32), 56),        # upscale, ksize 5
    ((48, 80), 56),        # crop along x
    ((80, 48), 56),        # crop along y
    ((56, 80), 56),        # no resample, crop only
    ((56, 56), 56),        # identity
    ((17, 23), 56),        # odd sizes, bounds clipped at both edges
]
LARGE = [((512, 512), 224), ((768, 768), 224)]
CASES = SMALL + LARGE


def k_pad(patch=PATCH):
    return (3 * patch * patch + 31) // 32 * 32


def make_image(kind, seed, h, w):
    """uint8 (h, w, 3)."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "ramp":
        yy, xx = np.mgrid[0:h, 0:w]
        planes = [xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 255 // max(h + w - 2, 1)]
        return np.stack(planes, -1).astype(np.uint8)
    if kind == "saturated":
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    raise KeyError(kind)


def as_float(u8):
    """float32 in [0, 1] whose reference truncation gives back the uint8 image ((k + 0.5) / 255 sits half a level away from both neighbours)."""
    return np.minimum((u8.astype(np.float32) + np.float32(0.5)) / np.float32(255), np.float32(1))


def im2col(px, patch=PATCH, ld=None):
    """(N, 3, S, S) pixel values -> the (N g g, ld) patch matrix: rows (n, gy, gx), columns (c, ky, kx), pad columns zero."""
    n, _, s, _ = px.shape
    g, ld = s // patch, ld or k_pad(patch)
    out = np.zeros((n * g * g, ld), np.float32)
    out[:, :3 * patch * patch] = px.reshape(n, 3, g, patch, g, patch).transpose(0, 2, 4, 1, 3, 5).reshape(n * g * g, 3 * patch * patch)
    return out


def pil_resized(u8, size):
    """Pillow's own bicubic resize of the short side to `size` and the centre crop, as clip_vision.preprocess asks for them: (size, size, 3) uint8."""
    from PIL import Image
    h, w = u8.shape[:2]
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    ow, oh = (new_short, new_long) if w <= h else (new_long, new_short)
    r = np.array(Image.fromarray(u8).resize((ow, oh), resample=Image.BICUBIC))
    top, left = (oh - size) // 2, (ow - size) // 2
    return np.ascontiguousarray(r[top:top + size, left:left + size])


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def case_key(kind, h, w, size):
    return f"{kind}:{h}x{w}->{size}"


def seed_of(kind, h, w):
    return 1000 * KINDS.index(kind) + 7 * h + w


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)["sha256"]
