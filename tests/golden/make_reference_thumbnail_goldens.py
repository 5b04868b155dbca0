#!/usr/bin/env python
"""Generates tests/golden/reference_thumbnail.json by EXECUTING the thumbnail reward of the reference in place.

Usage: `python tests/golden/make_reference_thumbnail_goldens.py <path of a checkout of the reference>`.  It reads the reference (read-only) and
writes one JSON fixture of recorded results.  Tests never touch the reference: they compare `ddpo_amd` against the committed fixture
(tests/test_thumbnail_cpu.py).

What runs from the reference, unmodified, lifted out of ddpo/training/callbacks.py with `ast` (its module-level imports — jax, flax, diffusers —
are not executed): thumbnail_fn, on the seeded images of tests/_thumbnail_cases.py.

thumbnail_fn loads CLIP ViT-L/14 through transformers and shards over jax devices.  Neither can run here, so it gets the stand-ins of
tests/golden/make_reference_symmetry_goldens.py (the processor is `ddpo_amd.models.clip_vision.preprocess`, the model's features are
tests/_symmetry_cases.py:standin_features, jit=False, `utils.shard` / `utils.unshard` are the identity) — the only part of the fixture that is
not reference code.  What this pins is everything around the model: the truncation to bytes, the thumbnail sizes, Pillow's default filter of
`Image.resize`, the order of the blocks, the reshape and the angle arithmetic.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import _thumbnail_cases as TC                                                          # noqa: E402
from make_reference_symmetry_goldens import _Model, _Processor, lift_functions, listed      # noqa: E402


def main():
    ref = sys.argv[1]
    import PIL
    from PIL import Image
    fake_tf = types.SimpleNamespace(CLIPProcessor=_Processor, FlaxCLIPModel=_Model)
    fake_utils = types.SimpleNamespace(shard=lambda x: x, unshard=lambda x: x)
    fns = lift_functions(os.path.join(ref, "ddpo/training/callbacks.py"), ["thumbnail_fn"],
                         {"np": np, "Image": Image, "transformers": fake_tf, "utils": fake_utils, "DEVICES": None})
    out = {"generated_by": "tests/golden/make_reference_thumbnail_goldens.py", "numpy_version": np.__version__, "pil_version": PIL.__version__,
           "cases": {}}
    for name in TC.CASES:
        u8 = TC.images_u8(name)
        scores, info = fns["thumbnail_fn"](jit=False)(TC.as_float(u8), None, None)
        assert info == {} and scores.shape == (len(u8),) and np.isfinite(scores).all()
        out["cases"][name] = {"shape": list(u8.shape), "thumbnail": listed(scores), "thumbnail_dtype": str(scores.dtype)}
    with open(TC.GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"wrote {TC.GOLDEN}: {len(out['cases'])} cases")
    for name, rec in out["cases"].items():
        print(name, rec["thumbnail"])


if __name__ == "__main__":
    main()
