"""LoRA adapters on the attention projections: flags, targets, counts and the adapter-file key layout (no GPU needed)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from ddpo_amd.models import lora as LO                      # noqa: E402
from ddpo_amd.models.unet import UNetConfig, unet_param_shapes      # noqa: E402


def test_flag_defaults_and_parser():
    from config import base as C
    from ddpo_amd.utils.parser import Parser
    assert C.base["pg"]["lora_rank"] == 0 and C.base["pg"]["lora_alpha"] is None
    assert "lora_rank" not in C.base["train"] and "lora_rank" not in C.base["sample"]
    a = Parser(["--dataset", "compressed_animals", "--lora_rank", "8"]).parse_args("pg")
    assert a.lora_rank == 8 and a.lora_alpha is None
    b = Parser(["--dataset", "compressed_animals", "--lora_rank", "4", "--lora_alpha", "8"]).parse_args("pg")
    assert b.lora_rank == 4 and b.lora_alpha == 8 and LO.lora_scale(b.lora_rank, b.lora_alpha) == 2.0
    assert LO.lora_scale(16, None) == 1.0


@pytest.mark.parametrize("name,count", [("sd15", 797184), ("sd21", 829952), ("tiny", 78080)])
def test_targets_and_adapter_counts(name, count):
    shapes = unet_param_shapes(UNetConfig.named(name))
    t = LO.lora_targets(shapes)
    assert len(t) == 128
    assert all(n.split(".")[-3] in ("attn1", "attn2") and n.split(".")[-2] in ("to_q", "to_k", "to_v", "to_out_0") for n in t)
    assert t == [n for n in shapes if n in set(t)]                  # parameter-layout order
    assert LO.n_adapter_params(shapes, 4) == count


def test_diffusers_key_round_trip_and_file_shapes():
    import re
    shapes = unet_param_shapes(UNetConfig.named("sd15"))
    keys = LO.diffusers_keys(shapes, 4)
    assert len(keys) == 256
    first = list(keys.items())[:2]
    assert first == [("down_blocks.0.attentions.0.transformer_blocks.0.attn1.processor.to_q_lora.down.weight", (4, 320)),
                     ("down_blocks.0.attentions.0.transformer_blocks.0.attn1.processor.to_q_lora.up.weight", (320, 4))]
    assert keys["mid_block.attentions.0.transformer_blocks.0.attn2.processor.to_k_lora.down.weight"] == (4, 768)
    assert keys["up_blocks.3.attentions.2.transformer_blocks.0.attn2.processor.to_out_lora.up.weight"] == (320, 4)
    for n in LO.lora_targets(shapes):
        layer = n[:-len(".kernel")]
        pre = LO.diffusers_key(layer)
        assert LO.flax_layer(pre) == layer
        # the module path is the one utils/serialization.torch_to_flax_tree maps back to this Flax name (".<i>" -> "_<i>")
        stem = pre.rsplit(".processor.", 1)[0]
        assert re.sub(r"\.(\d+)(?=\.|$)", r"_\1", stem) == layer.rsplit(".", 1)[0]
        K, N = shapes[n]
        assert keys[pre + ".down.weight"] == (4, K) and keys[pre + ".up.weight"] == (N, 4)


def test_rank_limits_and_rwr_rejection():
    with pytest.raises(ValueError, match="1..64"):
        LO.check_rank(65)
    with pytest.raises(ValueError):
        LO.check_rank(0)
    assert LO.check_rank(64) == 64
    with pytest.raises(SystemExit, match="LoRA"):
        LO.reject_lora_flags(["--dataset", "compressed-animals-rwr", "--lora_rank", "4"])
    LO.reject_lora_flags(["--dataset", "compressed-animals-rwr"])
    import importlib
    ft = importlib.import_module("pipeline.finetune")
    with pytest.raises(SystemExit, match="LoRA"):
        ft.main(["--dataset", "compressed-animals-rwr", "--lora_rank", "4"])


def test_lora_store_init_on_host():
    """diffusers' LoRALinearLayer initialisation (down ~ N(0, 1/r^2), up = 0), seeded: identical for the same seed."""
    import torch
    from ddpo_amd.models.unet import UNet2DCondition

    unet = UNet2DCondition(UNetConfig.named("tiny"), "cpu")
    s1 = LO.LoraStore(unet, 4, seed=3)
    s2 = LO.LoraStore(unet, 4, seed=3)
    assert torch.equal(s1.params.flat, s2.params.flat)
    A = torch.cat([v.reshape(-1) for n, v in s1.params.views.items() if n.endswith(".A")])
    assert all(float(v.abs().max()) == 0.0 for n, v in s1.params.views.items() if n.endswith(".B"))
    assert abs(float(A.std()) - 0.25) < 0.01
    assert s1.n_params == 78080 and s1.params.flat.numel() % 4 == 0
    assert all(v.data_ptr() % 16 == 0 for v in s1.params.views.values())
    assert unet.lora is s2
    sd = s1.state_dict()
    s2.init(seed=4)
    s2.load_state_dict(sd)
    assert torch.equal(s1.params.flat, s2.params.flat)


@pytest.mark.parametrize("mode", ["multi_host", "single_host"])
def test_adapter_seed_is_the_same_on_every_rank(mode):
    """parser.set_seed offsets args.seed by the process index; the adapters must still start identical on every rank (their updates are
    all-reduced), so the entry point seeds them with the configured base seed."""
    from ddpo_amd.training.dp import DataParallel
    from ddpo_amd.utils.parser import Parser
    import pipeline.policy_gradient as PG
    seeds = set()
    for rank in range(4):
        dp = DataParallel(mode=mode, rank=rank, world=4)
        a = Parser(["--dataset", "compressed_animals", "--lora_rank", "4", "--seed", "11"]).parse_args("pg", process_index=dp.seed_process_index)
        seeds.add(PG.lora_seed(a, dp))
    assert seeds == {11}
