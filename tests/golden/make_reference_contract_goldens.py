#!/usr/bin/env python
"""Generates tests/golden/reference_contracts.json by EXECUTING two small pieces of the reference's own code.

`python tests/golden/make_reference_contract_goldens.py <reference checkout>` (reads the checkout read-only).
  * `FlaxStableDiffusionPipeline.prepare_inputs` (ddpo/diffusers_patch/pipeline_flax_stable_diffusion.py) is lifted with `ast` and run on
    the synthetic CLIP tokenizer of tests/test_tokenizer_contract.py over its PROMPTS: the token ids and their dtype are stored.
  * the masker classes of ddpo/utils/logger.py (`make_masker` and what it builds) are lifted with `ast` and run on the inputs of
    tests/test_rwr_pipeline.py::test_maskers_equal_the_reference_classes: every mask and every repr are stored.
The tests compare `ddpo_amd` with this fixture, so they run wherever the repository does."""
import ast
import importlib.util
import json
import os
import sys
import tempfile
import typing

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "reference_contracts.json")

# the masker cases of tests/test_rwr_pipeline.py: three draws of 16 values per case, from one RandomState(4) stream
MASKER_CASES = [["percentile", 90], ["streaming_percentile", 95], ["streaming_percentile", 0], ["threshold", 0.1]]
MASKER_SEED, MASKER_DRAWS, MASKER_ROWS = 4, 3, 16


def _lift(path, names, ns):
    tree = ast.parse(open(path).read())
    nodes = []
    for node in tree.body:
        if isinstance(node, ast.ClassDef) and node.name in names.get("classes", ()):
            nodes.append(node)
        elif isinstance(node, ast.FunctionDef) and node.name in names.get("functions", ()):
            nodes.append(node)
        elif isinstance(node, ast.ClassDef) and node.name in names.get("methods_of", {}):
            nodes += [n for n in node.body if isinstance(n, ast.FunctionDef) and n.name in names["methods_of"][node.name]]
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)
    return ns


def prepare_inputs_ids(ref):
    spec = importlib.util.spec_from_file_location("_tok_contract", os.path.join(ROOT, "tests", "test_tokenizer_contract.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from ddpo_amd.models.text import load_tokenizer
    ns = _lift(os.path.join(ref, "ddpo", "diffusers_patch", "pipeline_flax_stable_diffusion.py"),
               {"methods_of": {"FlaxStableDiffusionPipeline": ("prepare_inputs",)}}, {"Union": typing.Union, "List": typing.List})
    with tempfile.TemporaryDirectory() as d:
        mod.write_tokenizer(d)

        class Self:
            tokenizer = load_tokenizer(d)
        ids = ns["prepare_inputs"](Self(), mod.PROMPTS)
    return {"prompts": mod.PROMPTS, "dtype": str(ids.dtype), "ids": ids.tolist()}


def masker_outputs(ref):
    ns = _lift(os.path.join(ref, "ddpo", "utils", "logger.py"),
               {"classes": ("Masker", "StreamingAverage", "StreamingPercentile", "Percentile", "Threshold"), "functions": ("make_masker",)},
               {"np": np})
    r = np.random.RandomState(MASKER_SEED)
    cases = []
    for mode, param in MASKER_CASES:
        m = ns["make_masker"](mode, param)
        masks, reprs = [], []
        for _ in range(MASKER_DRAWS):
            xs = r.randn(MASKER_ROWS, 1)
            masks.append(np.asarray(m(xs)).reshape(-1).astype(bool).tolist())
            reprs.append(repr(m))
        cases.append({"mode": mode, "param": param, "masks": masks, "reprs": reprs})
    return {"seed": MASKER_SEED, "draws": MASKER_DRAWS, "rows": MASKER_ROWS, "cases": cases}


def main(ref):
    out = {"generated_by": "tests/golden/make_reference_contract_goldens.py", "reference": "jannerm/ddpo",
           "prepare_inputs": prepare_inputs_ids(ref), "maskers": masker_outputs(ref)}
    with open(OUT, "w") as f:
        json.dump(out, f)
    print("wrote", OUT)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit("usage: make_reference_contract_goldens.py <reference checkout>")
    main(sys.argv[1])
