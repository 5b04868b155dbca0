"""LoRA on the feed-forward layers (`--lora_targets attn_ff`): target lists, the adapter-file key layout, flags and their rejections, and the
side binding of the wide adapter-gradient kernel (include/ddpo_lora_wide.h) with its host-side argument checks (no GPU needed)."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from ddpo_amd import lib as L                                       # noqa: E402
from ddpo_amd.models import lora as LO                              # noqa: E402
from ddpo_amd.models.unet import UNetConfig, unet_param_shapes      # noqa: E402

from _abi_check import check_signatures                             # noqa: E402


# ------------------------------------------------------------------------------------------------ targets and keys
@pytest.mark.parametrize("name", ["sd15", "tiny", "tiny21", "sd21"])
def test_target_lists(name):
    import re
    shapes = unet_param_shapes(UNetConfig.named(name))
    today = [n for n in shapes if re.search(r"\.attn[12]\.(to_q|to_k|to_v|to_out_0)\.kernel$", n)]
    assert LO.lora_targets(shapes) == LO.lora_targets(shapes, "attn") == today and len(today) == 128
    both = LO.lora_targets(shapes, "attn_ff")
    assert len(both) == 160 and both[:128] == today                 # the attention prefix is unchanged
    ff = both[128:]
    assert ff == [n for n in shapes if n.endswith(".ff.net_0.proj.kernel") or n.endswith(".ff.net_2.kernel")]      # parameter order
    assert not any("proj_in" in n or "proj_out" in n or "conv" in n for n in both)
    with pytest.raises(ValueError, match="attn / attn_ff"):
        LO.lora_targets(shapes, "ff")


def test_adapter_shapes_and_counts():
    shapes = unet_param_shapes(UNetConfig.named("sd15"))
    assert LO.n_adapter_params(shapes, 4) == LO.n_adapter_params(shapes, 4, "attn") == 797184
    a = LO.adapter_shapes(shapes, 4, "attn_ff")
    pre = "down_blocks_0.attentions_0.transformer_blocks_0.ff."
    assert a[pre + "net_0.proj.A"] == (320, 4) and a[pre + "net_0.proj.B"] == (4, 2560)
    assert a[pre + "net_2.A"] == (1280, 4) and a[pre + "net_2.B"] == (4, 320)
    assert a["mid_block.attentions_0.transformer_blocks_0.ff.net_0.proj.B"] == (4, 10240)
    extra = sum(4 * sum(shapes[n]) for n in LO.lora_targets(shapes, "attn_ff")[128:])
    assert LO.n_adapter_params(shapes, 4, "attn_ff") == 797184 + extra and extra > 0
    assert list(a)[:256] == list(LO.adapter_shapes(shapes, 4))


def test_feed_forward_key_round_trip_and_file_shapes():
    shapes = unet_param_shapes(UNetConfig.named("sd15"))
    keys = LO.diffusers_keys(shapes, 4, targets="attn_ff")
    assert len(keys) == 320 and list(keys)[:256] == list(LO.diffusers_keys(shapes, 4))        # attention keys stay as they are
    assert keys["down_blocks.0.attentions.0.transformer_blocks.0.ff.net.0.proj.lora.down.weight"] == (4, 320)
    assert keys["down_blocks.0.attentions.0.transformer_blocks.0.ff.net.0.proj.lora.up.weight"] == (2560, 4)
    assert keys["down_blocks.0.attentions.0.transformer_blocks.0.ff.net.2.lora.down.weight"] == (4, 1280)
    assert keys["mid_block.attentions.0.transformer_blocks.0.ff.net.2.lora.up.weight"] == (1280, 4)
    for n in LO.lora_targets(shapes, "attn_ff"):
        layer = n[:-len(".kernel")]
        pre = LO.diffusers_key(layer)
        assert LO.flax_layer(pre) == layer
        K, N = shapes[n]
        assert keys[pre + ".down.weight"] == (4, K) and keys[pre + ".up.weight"] == (N, 4)


def test_store_seed_files_and_target_inference(tmp_path):
    """The same seed gives the same attention adapters under both target sets; a file names its target set, a file without the field is
    read by its keys, and an attention-only file (every older file) reads as "attn"."""
    import torch
    from safetensors.torch import save_file
    from ddpo_amd.models.unet import UNet2DCondition
    unet = UNet2DCondition(UNetConfig.named("tiny"), "cpu")
    s_attn = LO.LoraStore(unet, 4, seed=3)
    assert s_attn.target_set == "attn" and not s_attn.has_ff and len(s_attn.targets) == 128
    s_ff = LO.LoraStore(unet, 4, seed=3, targets="attn_ff")
    assert s_ff.target_set == "attn_ff" and s_ff.has_ff and len(s_ff.targets) == 160
    for n, v in s_attn.params.views.items():
        assert torch.equal(v, s_ff.params[n]), n
    ffA = [v for n, v in s_ff.params.views.items() if ".ff." in n and n.endswith(".A")]
    assert len(ffA) == 32 and all(float(v.abs().max()) > 0 for v in ffA)
    assert all(float(v.abs().max()) == 0.0 for n, v in s_ff.params.views.items() if n.endswith(".B"))
    with pytest.raises(ValueError, match="attn / attn_ff"):
        LO.LoraStore(unet, 4, targets="all")
    p_ff = s_ff.save(str(tmp_path / "ff.safetensors"))
    p_attn = s_attn.save(str(tmp_path / "attn.safetensors"))
    sd, rank, alpha, targets = LO.read_lora_file(p_ff)
    assert (rank, alpha, targets) == (4, 4.0, "attn_ff") and set(sd) == set(LO.diffusers_keys(unet.params.shapes, 4, "attn_ff"))
    assert LO.read_lora_file(p_attn)[3] == "attn"
    old_meta = {"format": "diffusers-attn-processor-lora", "rank": "4", "alpha": "4"}          # a file from before the field existed
    save_file(dict(s_attn.state_dict()), str(tmp_path / "old.safetensors"), metadata=old_meta)
    save_file(dict(s_ff.state_dict()), str(tmp_path / "old_ff.safetensors"), metadata=old_meta)
    assert LO.read_lora_file(str(tmp_path / "old.safetensors"))[3] == "attn"
    assert LO.read_lora_file(str(tmp_path / "old_ff.safetensors"))[3] == "attn_ff"
    s_ff.init(seed=9)
    s_ff.load_state_dict(sd)
    assert torch.equal(s_ff.params["down_blocks_0.attentions_0.transformer_blocks_0.ff.net_2.A"].t().contiguous(),
                       sd["down_blocks.0.attentions.0.transformer_blocks.0.ff.net.2.lora.down.weight"])
    with pytest.raises(KeyError, match="lacks 64 keys"):
        s_ff.load_state_dict(s_attn.state_dict())


# ------------------------------------------------------------------------------------------------ flags
def test_flag_default_values_and_rejections():
    from config import base as C
    from ddpo_amd.utils.parser import Parser
    import pipeline.policy_gradient as PG
    assert C.base["pg"]["lora_targets"] == "attn"
    assert "lora_targets" not in C.base["train"] and "lora_targets" not in C.base["sample"]
    a = Parser(["--dataset", "compressed_animals", "--lora_rank", "8"]).parse_args("pg")
    assert a.lora_targets == "attn" and PG.check_lora_args(a) is None
    b = Parser(["--dataset", "compressed_animals", "--lora_rank", "4", "--lora_targets", "attn_ff"]).parse_args("pg")
    assert b.lora_targets == "attn_ff" and PG.check_lora_args(b) is None
    c = Parser(["--dataset", "compressed_animals"]).parse_args("pg")
    assert c.lora_rank == 0 and PG.check_lora_args(c) is None
    bad = Parser(["--dataset", "compressed_animals", "--lora_rank", "4", "--lora_targets", "ff"]).parse_args("pg")
    assert "must be attn or attn_ff" in PG.check_lora_args(bad)
    no_rank = Parser(["--dataset", "compressed_animals", "--lora_targets", "attn_ff"]).parse_args("pg")
    assert "needs --lora_rank > 0" in PG.check_lora_args(no_rank)
    src = open(os.path.join(ROOT, "pipeline", "policy_gradient.py")).read()
    assert "or check_lora_args(args)" in src and "lora_targets=lora.target_set" in src        # checked in main(), recorded in the bundle


def test_offline_entry_points_reject_lora_targets():
    with pytest.raises(SystemExit, match="--lora_targets: LoRA is available for pipeline/policy_gradient.py only"):
        LO.reject_lora_flags(["--dataset", "compressed-animals-rwr", "--lora_targets", "attn_ff"])
    with pytest.raises(SystemExit, match="--lora_targets"):
        LO.reject_lora_flags(["--lora_targets=attn"])
    import importlib
    for module, dataset in (("pipeline.finetune", "compressed-animals-rwr"), ("pipeline.dpo", "compressed-animals-rwr")):
        m = importlib.import_module(module)
        with pytest.raises(SystemExit, match="LoRA"):
            m.main(["--dataset", dataset, "--lora_targets", "attn_ff"])


# ------------------------------------------------------------------------------------------------ binding
def test_importing_the_engine_does_not_load_the_side_module():
    import subprocess
    code = ("import sys; import ddpo_amd; from ddpo_amd import lib; from ddpo_amd.models import lora, unet; "
            "import pipeline.policy_gradient; print('ddpo_amd.lib_lora_wide' in sys.modules)")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert out.strip().splitlines()[-1] == "False"


def test_side_binding_exports_signatures_and_refusal(monkeypatch):
    from ddpo_amd import lib_lora_wide as LW
    lib = ctypes.CDLL(L.LIB_PATH)
    assert LW.EXPORTED_SYMBOLS == ("ddpo_lora_wide_abi_version", "ddpo_lora_wgrad_wide_ws_bytes", "ddpo_lora_wgrad_wide")
    for name in LW.EXPORTED_SYMBOLS:
        assert hasattr(lib, name), f"{name} declared in ddpo_lora_wide.h but not exported"
    check_signatures(os.path.join(ROOT, "include", "ddpo_lora_wide.h"), LW._SIGS, 3)
    # the argument list is ddpo_lora_wgrad's
    assert LW._SIGS["ddpo_lora_wgrad_wide"] == L._SIGS["ddpo_lora_wgrad"]
    assert LW._SIGS["ddpo_lora_wgrad_wide_ws_bytes"] == L._SIGS["ddpo_lora_wgrad_ws_bytes"]
    # a binding newer than the library: load() names the symbol, asks for a rebuild and binds nothing (tests/test_abi_cpu.py)
    monkeypatch.setattr(LW, "_lib", None)
    monkeypatch.setitem(LW._SIGS, "ddpo_entry_of_a_later_build", (ctypes.c_int, [ctypes.c_void_p]))
    with pytest.raises(L.DdpoHipError, match="does not export ddpo_entry_of_a_later_build: rebuild"):
        LW.load()
    assert LW._lib is None
    monkeypatch.delitem(LW._SIGS, "ddpo_entry_of_a_later_build")
    monkeypatch.setattr(LW, "ABI_VERSION", 2)
    with pytest.raises(L.DdpoHipError, match="wide-LoRA ABI version 1, lib_lora_wide.py expects 2"):
        LW.load()
    monkeypatch.setattr(LW, "ABI_VERSION", 1)
    assert LW.load() is LW._lib and LW._lib is not None and LW._lib.ddpo_lora_wide_abi_version() == 1
    # the main ABI is untouched
    assert L.load().ddpo_abi_version() == L.ABI_VERSION == 15


def test_host_side_argument_checks_return_einval():
    """Every refusal is decided on the host before anything is launched: the pointers below are never dereferenced."""
    from ddpo_amd import lib_lora_wide as LW
    lib = LW.load()
    M, K, N, r = 17, 2560, 640, 6
    need = lib.ddpo_lora_wgrad_wide_ws_bytes(M, K, N, r)
    assert need >= (2 * M * 8 + (K + N) * 8) * 4                 # u, v padded to 8 ranks, at least one slab of (K + N) x 8
    p = lambda i: ctypes.c_void_p(0x10000 * (i + 1))             # distinct, 16-byte aligned, never read
    good = dict(x=p(0), ldx=K, hi=None, lo=None, ldp=0, dy=p(1), lddy=N, A=p(2), B=p(3), dA=p(4), dB=p(5), M=M, K=K, N=N, r=r, ws=p(6),
                ws_bytes=need)

    def call(**over):
        a = dict(good, **over)
        return lib.ddpo_lora_wgrad_wide(a["x"], a["ldx"], a["hi"], a["lo"], a["ldp"], a["dy"], a["lddy"], a["A"], a["B"], a["dA"], a["dB"],
                                        a["M"], a["K"], a["N"], a["r"], 0.5, a["ws"], a["ws_bytes"], None)

    for name in ("dy", "A", "B", "dA", "dB", "ws"):             # null pointers
        assert call(**{name: None}) == -1, name
    assert call(x=None) == -1                                    # neither fp32 rows nor planes
    assert call(x=None, hi=p(7)) == -1 and call(x=None, lo=p(8)) == -1
    assert call(K=K + 2, ldx=K + 4) == -1 and call(N=N + 1, lddy=N + 4) == -1          # K % 4, N % 4
    assert call(r=65) == -1 and call(r=0) == -1
    assert call(lddy=N - 4) == -1 and call(ldx=K - 4) == -1
    assert call(ws_bytes=need - 1) == -1 and call(ws_bytes=0) == -1                    # a short workspace
    assert call(K=16388, ldx=16388, ws_bytes=1 << 40) == -1 and call(N=16388, lddy=16388, ws_bytes=1 << 40) == -1
    assert call(M=0) == -1
    assert call(x=None, hi=p(7), lo=p(8), ldp=0, K=2564, ws_bytes=1 << 40) == -1       # k-blocked planes need K % 32 == 0
    assert call(x=ctypes.c_void_p(0x10004)) == -1 and call(ws=ctypes.c_void_p(0x70008)) == -1      # misaligned
    for bad in ((0, K, N, r), (M, K + 1, N, r), (M, K, 16388, r), (M, K, N, 65)):
        assert lib.ddpo_lora_wgrad_wide_ws_bytes(*bad) == 0
    # the workspace grows with the shape and the largest real layer at rank 64 stays modest
    assert lib.ddpo_lora_wgrad_wide_ws_bytes(154, 1280, 10240, 64) < (64 << 20)
