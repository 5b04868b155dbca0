"""Writes tests/golden/clip_preprocess_sha256.json: sha256 of the bytes Pillow's bicubic resize + centre crop returns for the seeded cases of
tests/_clip_cases.py.  A test box whose Pillow resamples differently shows up as a disagreement between the live Pillow and these hashes, not as a
kernel bug.

    python tests/golden/make_clip_preprocess_sha256.py
"""
import json
import os
import sys

import PIL

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from _clip_cases import CASES, GOLDEN, KINDS, case_key, make_image, pil_resized, seed_of, sha  # noqa: E402

if __name__ == "__main__":
    rows = {case_key(k, h, w, s): sha(pil_resized(make_image(k, seed_of(k, h, w), h, w), s)) for (h, w), s in CASES for k in KINDS}
    with open(GOLDEN, "w") as f:
        json.dump({"resampler": f"Pillow {PIL.__version__}, Image.resize(resample=BICUBIC) of an RGB image, then the centre crop", "sha256": rows}, f, indent=0)
    print(f"wrote {len(rows)} hashes to {GOLDEN}")
