"""What ddpo_amd/lib.py's GEMM / conv wrappers hand to the C ABI, without a GPU: the call records of tests/golden/make_lib_launch_records.py
(every ddpo_* call with its scalars, every field of every ddpo_gemm_desc, symbolic pointers, return values, PROFILE entries, exceptions, and
the routing predicates on a grid) regenerated from the code under test and compared, record by record and in order, with
tests/golden/lib_launch_records.json — recorded before the descriptor / launch / profiling helpers of lib.py were introduced.  The guards
below are asserted on the golden file itself, so that the comparison cannot be about nothing."""
import importlib.util
import json
import os

import pytest

from ddpo_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_lib_launch_records", os.path.join(ROOT, "tests", "golden", "make_lib_launch_records.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

FORWARD = ("ddpo_gemm_conv_fwd", "ddpo_gemm_conv_fwd_bf16", "ddpo_gemm_conv_fwd_bf16_planes", "ddpo_gemm_conv_fwd_f16mx_planes", "ddpo_conv_up2x_folded_fwd")
WGRAD = ("ddpo_gemm_conv_wgrad", "ddpo_gemm_conv_wgrad_bf16x3", "ddpo_gemm_conv_wgrad_bf16x3_planes")
PACK = ("ddpo_pack_weights_bf16", "ddpo_pack_weights_bf16_kblocked", "ddpo_pack_weights_bf16_kblocked_dgrad", "ddpo_pack_weights_f16mx",
        "ddpo_fold_up2x_weights")
# every DdpoHipError / ValueError the GEMM section of lib.py can raise (the beginning of its message)
RAISES = ("f16mx planes need whole 32-channel blocks", "pack_weights_up2x_folded: pack_weights(w) first", "conv2d_up2x_folded: no folded planes",
          "conv2d_up2x_folded: geometry does not match", "activation planes of the wrong format / shape for this layer (ask up2x_planes_pay)",
          "conv2d_up2x_folded needs its fp32 input", "_dgrad_fwd: one 256-row chunk", "plane-fed linear_geglu needs", "plane-emitting linear_geglu needs",
          "an f16mx layer needs its fp32 input", "activation planes of the wrong format for this layer (ask planes_pay", "yes",
          "a plane-emitting GEMM needs", "a plane-fed GEMM needs", "a column slice of k-blocked planes cannot be a wgrad operand",
          "stride-2 dgrad expects even input sizes")
PREDICATE_VALUES = dict(planes_ok="01", planes_pay="012", planes_out_ok="01", norm_planes="012", norm_planes_train="01", geglu_tall_pays="01",
                        up2x_fold_ok="01", up2x_planes_pay="012")


@pytest.fixture(scope="module")
def golden():
    with open(G.GOLDEN) as f:
        return G.expand(json.load(f))


def _calls(golden, case):
    return golden[case]["records"]


def _desc(rec):
    return rec[1]["desc"]


def _messages(v, out):
    if isinstance(v, dict):
        if "raised" in v:
            out.add(v["message"])
        for x in v.values():
            _messages(x, out)
    elif isinstance(v, list):
        for x in v:
            _messages(x, out)
    return out


def test_golden_is_not_vacuous(golden):
    symbols = {r[0] for res in golden.values() for r in res["records"]}
    assert not [s for s in FORWARD + WGRAD + PACK if s not in symbols]
    msgs = _messages(list(golden.values()), set())
    assert not [m for m in RAISES if not any(x.startswith(m) for x in msgs)]
    for name, values in PREDICATE_VALUES.items():
        seen = set().union(*(res["returned"][name] for cid, res in golden.items() if cid.endswith("/predicates")))
        assert seen == set(values), name
    # both the launches that record to PROFILE and the ones that must not
    assert any(res["profile"] for res in golden.values()) and any(res["profile"] is None for res in golden.values())
    assert golden["bf16x3/mk2560/default/ldgrad_long/profile"]["profile"] == [] and golden["bf16x3/mk2560/default/cdgrad_s1/profile"]["profile"] == []
    assert {p[1] for res in golden.values() for p in res["profile"] or []} == {"fp32", "bf16", "bf16x3", "f16mx"}


def test_every_descriptor_site_is_reached(golden):
    """The eight places of lib.py that fill a ddpo_gemm_desc, each identified by what only it produces."""
    c = lambda case: _calls(golden, case)
    assert any(r[0] == "ddpo_gemm_conv_fwd_f16mx_planes" and _desc(r).get("ksize") == 3 for r in c("fp32/mk2560/default/raw_f16mx_conv/profile"))
    assert any(r[0] == "ddpo_conv_up2x_folded_fwd" for r in c("bf16x3/mk2560/default/fold_fp32/profile"))
    assert any(r[0] == "ddpo_gemm_conv_fwd_bf16_planes" and r[7] == 0 for r in c("bf16x3/mk2560/default/ldgrad_long/profile"))           # _dgrad_fwd
    assert any(r[0] == "ddpo_gemm_conv_fwd_bf16" and _desc(r).get("epilogue") == 1 for r in c("bf16x3/mk2560/default/geglu_fp32/profile"))
    assert any(r[0] == "ddpo_gemm_conv_fwd_bf16_planes" and _desc(r).get("epilogue") == 2 for r in c("bf16x3/mk2560/default/geglu_tall/profile"))
    assert not any(_desc(r).get("epilogue") == 2 for r in c("bf16x3/mk2560/default/geglu_tall_below/profile") if r[0].startswith("ddpo_gemm"))
    assert any(r[0] == "ddpo_gemm_conv_fwd" and "w" in _desc(r) for r in c("bf16x3/mk2560/default/linear_unpacked/profile"))             # gemm_conv
    assert any(r[0] == "ddpo_gemm_conv_fwd_bf16" and "w" not in _desc(r) and r[4] == G.N                                                 # linear_dgrad, bwd
               for r in c("bf16x3/mk2560/DGRAD_FWD=0/ldgrad_small/profile"))
    assert any(r[0] == "ddpo_gemm_conv_fwd" and _desc(r).get("w_trans") == 1 for r in c("bf16x3/mk2560/default/ldgrad_unpacked/profile"))   # its gemm_conv branch
    assert any(r[0] in WGRAD for r in c("bf16x3/mk2560/default/wgrad_linear/profile"))
    assert any(r[0] == "ddpo_gemm_conv_fwd" and _desc(r).get("w_dgrad") == 1 for r in c("fp32/mk2560/default/cdgrad_s1/profile"))        # conv2d_dgrad
    assert any(r[0] == "ddpo_gemm_conv_fwd_bf16" and _desc(r).get("w_dgrad") == 1 and _desc(r).get("upsample") == 2
               for r in c("bf16x3/mk2560/DGRAD_FWD=0/cdgrad_s2/profile"))
    chunks = [r for r in c("bf16x3/mk2560/default/ldgrad_chunked/profile") if r[0] == "ddpo_gemm_conv_fwd_bf16"]                        # row chunks of a >= 2 GiB dY
    assert [_desc(r)["M"] for r in chunks] == [419328, 672] and _desc(chunks[1])["src"] == f"dy+{419328 * 1280 * 4}"


def test_records_equal_the_golden_file(golden):
    got = G.expand(G.generate())
    assert list(got) == list(golden)                       # the same cases in the same order: none skipped, none added
    wrong = [cid for cid in golden if got[cid] != golden[cid]]
    for cid in wrong[:5]:
        g, w = got[cid], golden[cid]
        print(cid)
        for k in sorted(set(g) | set(w)):
            if g.get(k) != w.get(k):
                if k == "records" and len(g[k]) == len(w[k]):
                    for a, b in zip(g[k], w[k]):
                        if a != b:
                            print("  got     ", json.dumps(a, sort_keys=True), "\n  expected", json.dumps(b, sort_keys=True))
                else:
                    print("  got     ", k, json.dumps(g.get(k), sort_keys=True)[:2000], "\n  expected", k, json.dumps(w.get(k), sort_keys=True)[:2000])
    assert not wrong, f"{len(wrong)} of {len(golden)} cases differ from tests/golden/lib_launch_records.json, the first: {wrong[:5]}"


def test_generator_leaves_lib_as_it_found_it():
    assert L._lib is None or not isinstance(L._lib, G.Recorder)
    assert L.PROFILE is None and not L.PACKED
