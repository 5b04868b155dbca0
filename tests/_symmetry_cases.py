"""Seeded images and cases shared by the symmetry tests (tests/test_symmetry_cpu.py, tests/test_gpu_symmetry.py) and by
tests/golden/make_reference_symmetry_goldens.py.  Images are regenerated from the case, never stored."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_symmetry.json")
MIRROR_CORR_FACTOR = 4            # bound = factor x the recorded deviation of the reference's float32 code from the exact correlation: numpy's
                                  # pairwise summation order varies with its SIMD build

# name -> (N, H, W); what each catches is said where the GPU test uses it
CASES = {
    "1x1": (1, 1, 1),              # the one pixel is its own partner
    "3x5": (2, 3, 5),              # self-partnered centre column / row, below a wave
    "24x40": (2, 24, 40),          # non-square: rot180 pairs rows
    "7x520": (1, 7, 520),          # a row wider than a workgroup's lanes; W * 3 is no multiple of 16, H is odd
    "all255": (1, 160, 152),       # sum of a^2 = 4.74e9 > 2^32
    "kinds64": (5, 64, 64),        # noise, gradient, left-right symmetric checker, constant, 0 / 255 extremes
}
ROTATIONAL_CASES = ("kinds64", "rot40")            # square batches for `rotational`
EXTRA = {"rot40": (3, 40, 40)}


def images_u8(name):
    """uint8 (N, H, W, 3) of a case."""
    n, h, w = {**CASES, **EXTRA}[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "all255":
        return np.full((n, h, w, 3), 255, np.uint8)
    if name == "kinds64":
        yy, xx = np.mgrid[0:h, 0:w]
        gradient = np.stack([xx * 255 // (w - 1), yy * 255 // (h - 1), (xx + yy) * 255 // (h + w - 2)], -1)
        half = rng.integers(0, 256, (h, w // 2, 3))
        checker = ((yy // 8 + np.minimum(xx, w - 1 - xx) // 8) % 2 * 200 + 20)[..., None].repeat(3, -1)
        symmetric = np.where((yy < h // 2)[..., None], checker, np.concatenate([half, half[:, ::-1]], 1))
        return np.stack([rng.integers(0, 256, (h, w, 3)), gradient, symmetric, np.full((h, w, 3), 77), rng.integers(0, 2, (h, w, 3)) * 255]).astype(np.uint8)
    return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def as_float(u8):
    """float32 in [0, 1] whose truncation (x * 255).astype(uint8) gives back the bytes."""
    return np.minimum((u8.astype(np.float32) + np.float32(0.5)) / np.float32(255), np.float32(1))


def stats_numpy(u8, mode):
    """The four sums of lib.symmetry_stats restated with numpy in int64, (N, 4)."""
    a = u8.astype(np.int64)
    b = a[:, :, ::-1] if mode == "mirror" else a[:, ::-1, ::-1]
    d = (a - b) % 256
    return np.stack([((d * d) % 256).sum((1, 2, 3)), a.sum((1, 2, 3)), (a * a).sum((1, 2, 3)), (a * b).sum((1, 2, 3))], 1)


def exact_mirror_corr(u8):
    """-(correlation of the bytes with their mirror image) from integer sums, one rounding: float64 (N,), nan for a constant image."""
    out = []
    for _, sa, saa, sab in stats_numpy(u8, "mirror").tolist():
        n = u8[0].size
        num, den = n * sab - sa * sa, n * saa - sa * sa
        out.append(-(num / den) if den else float("nan"))
    return np.array(out)


def standin_features(pixel_values):
    """The stand-in for CLIP's image features the `rotational` golden was recorded with: a fixed seeded linear map of 256 pixel values to 8
    features, plus 1, summed in float64 in index order (no BLAS, so the same on every machine) and rounded to float32."""
    px = np.asarray(pixel_values, np.float32)
    flat = px.reshape(len(px), -1)
    rng = np.random.default_rng(2024)
    idx = rng.choice(flat.shape[1], 256, replace=False)
    w = rng.standard_normal((256, 8))
    acc = np.ones((len(px), 8))
    for j in range(256):
        acc = acc + flat[:, idx[j], None].astype(np.float64) * w[j][None, :]
    return acc.astype(np.float32)


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
