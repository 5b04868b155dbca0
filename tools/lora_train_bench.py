#!/usr/bin/env python
"""Interleaved A/B of the fused PPO train step: full fine-tuning vs LoRA adapters on the attention projections (and, `--lora_targets attn_ff`,
on the feed-forward layers), on one GPU in one process.

Both arms run bench.py's train geometry (synthetic weights, train_cfg, `--fuse` micro-steps of `--batch` samples per launch, graph-replayed
through train_steps_fused, an optimizer update every `--steps-per-update` micro-steps) on their own U-Net; the arms alternate round by round
and every round is timed with device events.  Prints one JSON line per arm: sample-timesteps/s, ms per optimizer update and the arm's own
device memory, from torch.cuda.memory_allocated / max_memory_allocated (both arms stay resident, so the process peak alone says nothing about
either): `resident_gb` = what building the arm and its warm-up update left allocated (weights, planes, gradient / optimizer buffers, the
captured graphs' pools; the engine's shared scratch counts to the arm that first grows it), `transient_peak_gb` = the largest allocation above that during its timed updates, `footprint_gb` = their sum.  Also prints the algorithmic bytes of
ddpo_lora_wgrad at the 64x64-level shape and of every ddpo_lora_wgrad_wide launch (x and dY read once), for the kernel time of a separate
`rocprofv3 --kernel-trace --stats` run.

An arm is `full`, `lora` (`--lora_targets` at `--rank`) or `<targets>:<rank>`.  Every arm keeps its own U-Net and captured graphs resident
(the graph pools of one SD-1.5 arm at the default geometry are tens of GB): two arms fit one 288 GB device, four do not, so a wider
comparison is several calls that share the `full` arm:

    python tools/lora_train_bench.py [--model sd15] [--rank 4] [--lora_targets attn] [--rounds 3] [--updates 1]
    python tools/lora_train_bench.py --arms full,attn_ff:4
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="sd15")
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--fuse", type=int, default=16)
    ap.add_argument("--steps-per-update", type=int, default=50, help="micro-steps per optimizer update (the entrypoint: n_inference_steps)")
    ap.add_argument("--rank", type=int, default=4)
    ap.add_argument("--lora_targets", default="attn", choices=("attn", "attn_ff"), help="the layers the `lora` arm adapts")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--updates", type=int, default=1, help="optimizer updates per timed round")
    ap.add_argument("--arms", default="full,lora")
    args = ap.parse_args()

    from ddpo_amd import lib as L
    from ddpo_amd.models.unet import UNet2DCondition, UNetConfig
    from ddpo_amd.models.lora import LoraStore
    from ddpo_amd.diffusers_patch.scheduling_ddim import DDIMScheduler
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdamWConfig, train_steps_fused
    assert torch.cuda.is_available(), "tools/lora_train_bench.py measures on the GPU"
    L.load()
    L.DATAPATH = L.shipped_datapath()
    dev = torch.device("cuda", 0)
    ucfg = UNetConfig.named(args.model)
    sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", set_alpha_to_one=False, steps_offset=1,
                          prediction_type=ucfg.prediction_type)
    st = sched.set_timesteps(sched.create_state(device=dev), args.steps_per_update)
    b, hw = args.batch, args.resolution // 8
    g = torch.Generator().manual_seed(3)
    lat = torch.randn(b, 4, hw, hw, generator=g).to(dev)
    batch = {"latents": lat, "next_latents": 0.98 * lat + 0.05 * torch.randn(b, 4, hw, hw, generator=g).to(dev),
             "ts": torch.tensor([481, 21, 961, 241][:b], dtype=torch.int32, device=dev), "log_probs": torch.full((b,), -1.0, device=dev),
             "advantages": torch.tensor([0.7, -1.1, 0.3, -0.2][:b], device=dev),
             "prompt_embeds": torch.randn(b, 77, ucfg.cross_attention_dim, generator=g).to(dev),
             "uncond_embeds": torch.randn(b, 77, ucfg.cross_attention_dim, generator=g).to(dev)}

    T = args.steps_per_update
    plan = []                              # launch sizes of one optimizer update: 16 + 16 + 16 + 2 at the defaults
    left = T
    while left > 0:
        plan.append(min(args.fuse, left))
        left -= plan[-1]

    def update(arm):
        for i, f in enumerate(plan):
            train_steps_fused(arm["state"], [batch] * f, st, sched, True, 5.0, 1.0, 1e-4, do_opt_update=i == len(plan) - 1)

    def arm_spec(name):                    # -> (targets, rank) of a LoRA arm, None for full fine-tuning
        if name == "full":
            return None
        if name == "lora":
            return args.lora_targets, args.rank
        targets, rank = name.split(":")
        return targets, int(rank)

    arms = {}
    for name in args.arms.split(","):     # built and warmed up one after the other: what stays allocated is the arm's own
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(dev)
        unet = UNet2DCondition(ucfg, dev)
        unet.params.init_synthetic(seed=0)
        unet.params.pack_bf16(bwd=True)
        spec = arm_spec(name)
        lora = LoraStore(unet, spec[1], seed=0, targets=spec[0]) if spec else None
        arm = arms[name] = dict(state=AccumulatingTrainState(unet, AdamWConfig(), lora=lora), times=[], transient=0, spec=spec)
        update(arm)                        # warm-up: graph capture of every launch size, first optimizer update
        torch.cuda.synchronize()
        arm["resident"] = torch.cuda.memory_allocated(dev) - before
    for _ in range(args.rounds):
        for name, arm in arms.items():
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.updates):
                update(arm)
            e1.record()
            torch.cuda.synchronize()
            arm["times"].append(e0.elapsed_time(e1) / args.updates)
            arm["transient"] = max(arm["transient"], torch.cuda.max_memory_allocated(dev) - base)
    res = {}
    for name, arm in arms.items():
        ms = sorted(arm["times"])
        med = ms[len(ms) // 2]
        res[name] = med
        print(json.dumps({"arm": name, "model": args.model, "rank": arm["spec"][1] if arm["spec"] else 0,
                          "lora_targets": arm["spec"][0] if arm["spec"] else None, "layers": len(arm["state"].lora.targets) if arm["spec"] else 0,
                          "datapath": L.DATAPATH,
                          "sample_timesteps_per_s": b * T / (med / 1e3), "ms_per_optimizer_update": med, "ms_per_update_all_rounds": arm["times"],
                          "resident_gb": arm["resident"] / 1e9, "transient_peak_gb": arm["transient"] / 1e9,
                          "footprint_gb": (arm["resident"] + arm["transient"]) / 1e9, "micro_steps_per_update": T, "launch_plan": plan,
                          "trainable_params": (arm["state"].trainable.n_params)}))
    if "full" in res:
        for name in res:
            if name != "full":
                print(json.dumps({"arm": name, "lora_speedup_vs_full": res["full"] / res[name]}))
    # algorithmic bytes of one ddpo_lora_wgrad at the 64x64 level of the fused step (U-Net batch = fuse * batch * 2 (CFG)): x and dY read once
    M = args.fuse * b * 2 * hw * hw
    C = ucfg.block_out_channels[0]
    print(json.dumps({"lora_wgrad_64x64_level": {"M": M, "K": C, "N": C, "rank": args.rank, "algorithmic_bytes": M * (C + C) * 4,
                                                 "note": "divide by the kernel time of lora_wgrad_kernel in the rocprofv3 --stats run"}}))

    # ... and of the feed-forward layers that take ddpo_lora_wgrad_wide (K, N outside the narrow kernel's limits), per resolution level
    from ddpo_amd.models.lora import NARROW_MAX_DIM, NARROW_MAX_SUM
    wide = []
    for lvl, C in enumerate(ucfg.block_out_channels):
        Ml = args.fuse * b * 2 * (hw >> lvl) ** 2
        for what, (K, N) in (("ff.net_0.proj", (C, 8 * C)), ("ff.net_2", (4 * C, C))):
            if K > NARROW_MAX_DIM or N > NARROW_MAX_DIM or K + N > NARROW_MAX_SUM:
                wide.append({"layer": what, "level": lvl, "M": Ml, "K": K, "N": N, "algorithmic_bytes": Ml * (K + N) * 4})
    print(json.dumps({"lora_wgrad_wide_layers": wide,
                      "note": "per launch; lora_wide_uv_kernel and lora_wide_outer_kernel each read x and dY once per rank slice of 4"}))


if __name__ == "__main__":
    main()
