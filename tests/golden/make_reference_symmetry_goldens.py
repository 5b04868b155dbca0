#!/usr/bin/env python
"""Generates tests/golden/reference_symmetry.json by EXECUTING the symmetry rewards of the reference in place.

Usage: `python tests/golden/make_reference_symmetry_goldens.py <path of a checkout of the reference>`.  It reads the reference (read-only) and
writes one JSON fixture of recorded results.  Tests never touch the reference: they compare `ddpo_amd` against the committed fixture
(tests/test_symmetry_cpu.py, tests/test_gpu_symmetry.py).

What runs from the reference, unmodified, lifted out of ddpo/training/callbacks.py with `ast` (its module-level imports — jax, flax, diffusers —
are not executed): mirror_symmetry_fn, cov, mirror_correlation_fn, rotational_correlation_fn and rotational_symmetry_fn, on the seeded images of
tests/_symmetry_cases.py.

rotational_symmetry_fn loads CLIP ViT-L/14 through transformers and shards over jax devices.  Neither can run here, so it gets stand-ins — the
only part of the fixture that is not reference code:
  * `transformers.CLIPProcessor.from_pretrained(...)` returns `ddpo_amd.models.clip_vision.preprocess` (which tests/test_oracle_clip_vision.py
    and the aesthetic goldens hold to the real processor), wrapped to the processor's call signature;
  * `transformers.FlaxCLIPModel.from_pretrained(...).get_image_features` is a fixed seeded linear map of the pixel values
    (tests/_symmetry_cases.py:standin_features);
  * jit=False, and `utils.shard` / `utils.unshard` are the identity.
What this pins is everything around the model: the truncation to bytes, the rotation order, the reshape and the angle arithmetic.

Also recorded: `mirror_corr_f32_dev`, the largest |float32 score of the reference - exact correlation| over the cases (constant images, whose
score is nan, excluded).  The exact value comes from integer sums (tests/_symmetry_cases.py:exact_mirror_corr).  It is the measured error of
the reference's own float32 code; the tests bound the host and the device `mirror_corr` by MIRROR_CORR_FACTOR times it.
"""
import ast
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import _symmetry_cases as SC                                    # noqa: E402
from ddpo_amd.models import clip_vision as CV                   # noqa: E402

NAMES = ["mirror_symmetry_fn", "cov", "mirror_correlation_fn", "rotational_correlation_fn", "rotational_symmetry_fn"]


def lift_functions(path, names, extra):
    """exec only the named top-level functions of a reference file (its module-level imports are not executed)."""
    tree = ast.parse(open(path).read())
    ns = {"__builtins__": __builtins__}
    ns.update(extra)
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    missing = [n for n in names if n not in ns]
    assert not missing, missing
    return ns


class _Processor:
    @classmethod
    def from_pretrained(cls, name):
        return cls()

    def __call__(self, images, return_tensors):
        assert return_tensors == "np"
        return {"pixel_values": CV.preprocess([np.asarray(im) for im in images], 224)}


class _Model:
    @classmethod
    def from_pretrained(cls, name):
        return cls()

    def get_image_features(self, pixel_values):
        return SC.standin_features(pixel_values)


def listed(x):
    """floats as a list, nan as null"""
    return [None if np.isnan(v) else float(v) for v in np.asarray(x, dtype=np.float64).reshape(-1)]


def main():
    ref = sys.argv[1]
    from PIL import Image, ImageOps
    import PIL
    fake_tf = types.SimpleNamespace(CLIPProcessor=_Processor, FlaxCLIPModel=_Model)
    fake_utils = types.SimpleNamespace(shard=lambda x: x, unshard=lambda x: x)
    fns = lift_functions(os.path.join(ref, "ddpo/training/callbacks.py"), NAMES,
                         {"np": np, "Image": Image, "ImageOps": ImageOps, "transformers": fake_tf, "utils": fake_utils, "DEVICES": None})
    out = {"generated_by": "tests/golden/make_reference_symmetry_goldens.py", "numpy_version": np.__version__, "pil_version": PIL.__version__,
           "cases": {}}
    dev = 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        for name in list(SC.CASES) + list(SC.EXTRA):
            u8 = SC.images_u8(name)
            images = SC.as_float(u8)
            rec = {"shape": list(u8.shape)}
            for key, fn in (("mirror", "mirror_symmetry_fn"), ("mirror_corr", "mirror_correlation_fn"), ("rotational_corr", "rotational_correlation_fn")):
                scores, info = fns[fn]()(images.copy(), None, None)
                assert info == {} and scores.shape == (len(u8),)
                rec[key] = listed(scores)
                rec[key + "_dtype"] = str(scores.dtype)
            exact = SC.exact_mirror_corr(u8)
            got = np.array([np.nan if v is None else v for v in rec["mirror_corr"]])
            assert np.array_equal(np.isnan(exact), np.isnan(got)), name
            if (~np.isnan(exact)).any():
                dev = max(dev, float(np.nanmax(np.abs(got - exact))))
            if name in SC.ROTATIONAL_CASES:
                scores, info = fns["rotational_symmetry_fn"](jit=False)(images.copy(), None, None)
                assert info == {} and scores.shape == (len(u8),)
                rec["rotational"] = listed(scores)
                rec["rotational_dtype"] = str(scores.dtype)
            out["cases"][name] = rec
    out["mirror_corr_f32_dev"] = dev
    import json
    with open(SC.GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"wrote {SC.GOLDEN}: {len(out['cases'])} cases, mirror_corr_f32_dev = {dev:.3e}")


if __name__ == "__main__":
    main()
