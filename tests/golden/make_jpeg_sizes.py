"""Writes tests/golden/jpeg_sizes.json: JPEG byte counts recorded from PIL (Pillow with libjpeg-turbo) for the seeded recipes of
tests/_jpeg_cases.py.  Images are regenerated from (recipe, seed, size), never stored.  A test box whose PIL bundles a different libjpeg shows
up as a disagreement between the live PIL and these counts, not as a kernel bug.

    python tests/golden/make_jpeg_sizes.py
"""
import json
import os
import sys

import PIL

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from _jpeg_cases import GOLDEN, RECIPES, make_image  # noqa: E402
from ddpo_amd.training.callbacks import encode_jpeg  # noqa: E402

SMALL = [(16, 16), (48, 32), (64, 64)]
QUALITIES = [25, 50, 80, 95, 100]
LARGE = [("noise", 512, 512, 95), ("smooth", 512, 512, 95)]


def cases():
    out = []
    for h, w in SMALL:
        for q in QUALITIES:
            for i, recipe in enumerate(RECIPES):
                out.append((recipe, 100 + i, h, w, q))
    return out + [(r, 7, h, w, q) for r, h, w, q in LARGE]


if __name__ == "__main__":
    rows = [dict(recipe=r, seed=s, h=h, w=w, quality=q, bytes=len(encode_jpeg(make_image(r, s, h, w), quality=q))) for r, s, h, w, q in cases()]
    with open(GOLDEN, "w") as f:
        json.dump({"encoder": f"Pillow {PIL.__version__}, PIL.Image.save(format='JPEG', quality=q)", "cases": rows}, f, indent=0)
    print(f"wrote {len(rows)} cases to {GOLDEN}")
