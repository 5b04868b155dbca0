#!/usr/bin/env python
"""Adafactor against AdamW on one GPU: the update alone on a full-size flat buffer, and the peak memory of a full-size train step.

    python tools/adafactor_bench.py update [--model sd15] [--rounds 5] [--reps 4]
        Both updates on buffers laid out like the U-Net's ParamStore (random p and g, zero_grad off so that g stays defined over the repeats:
        the shipped calls also write the 4 B/param of zeros), alternating round by round, each round timed with device events.  Prints one JSON
        line per optimizer: ms per update, the algorithmic HBM bytes per update (computed here from the shapes) and their rate against the
        8 TB/s specification and the ~6.3 TB/s a streaming kernel reaches.
    python tools/adafactor_bench.py peak --optimizer adamw|adafactor [--model sd15]
        One process per optimizer: builds the engine on synthetic weights, runs one optimizer update of the entry point's geometry (fused
        micro-steps of 2 samples x CFG at 64x64 latents, graph-replayed) and prints torch.cuda.max_memory_allocated.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

HBM_SPEC_GBPS, HBM_STREAM_GBPS = 8000.0, 6300.0


def adafactor_bytes(plan):
    """Algorithmic HBM bytes of one update with zero_grad off: g read three times, p read twice and written once (24 B/param), the unfactored
    second moments read three times and written once, and per factored tensor the statistics, factor vectors and per-tile partial sums."""
    total = 0
    for _, _, t in plan.entries:
        total += 24 * t.numel
        if t.factored:
            ntr = -(-t.R // 128)
            rc = t.S * (t.R + t.C)
            total += 4 * (t.S * t.R + t.S * ntr * t.C) * 2          # row sums and per-tile column sums: written, then read
            total += 4 * rc * 3                                      # v_row / v_col: read, written, re-read for the factors
            total += 4 * rc * (1 + 2 * ntr)                          # factor vectors: written once, read by every row tile of two passes
        else:
            total += 16 * t.numel
    return total + 32 * plan.n_tiles


def bench_update(args):
    from ddpo_amd import lib as L
    from ddpo_amd import lib_optim as LO
    from ddpo_amd.models.unet import ParamStore, UNetConfig, unet_param_shapes
    L.load()
    dev = torch.device("cuda", 0)
    shapes = unet_param_shapes(UNetConfig.named(args.model))
    gen = torch.Generator(device=dev).manual_seed(1)
    p = ParamStore(shapes, dev)
    p.flat.normal_(generator=gen).mul_(0.05)
    n = p.flat.numel()
    g = torch.randn(n, generator=gen, device=dev) * 1e-3
    sq = torch.zeros(1, dtype=torch.float64, device=dev)
    L.grad_sqnorm(g, sq)
    p_adam, p_af = p.flat.clone(), p.flat
    mu = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    nu = torch.zeros(n, dtype=torch.float32, device=dev)
    plan = LO.AdafactorPlan.for_store(p).to(dev)
    v = plan.new_state()
    count = {"adamw": 0, "adafactor": 0}

    def adamw():
        count["adamw"] += 1
        L.adamw_bf16mu_step(p_adam, g, mu, nu, sq, 1.0, 1e-5, 0.9, 0.999, 1e-8, 1e-4, 1.0, count["adamw"], zero_grad=False)

    def adafactor():
        LO.adafactor_step(p_af, g, v, plan, sq, 1.0, 1e-5, count["adafactor"], 1e-4, 1.0, zero_grad=False)
        count["adafactor"] += 1

    arms = {"adamw": (adamw, 24 * n), "adafactor": (adafactor, adafactor_bytes(plan))}
    times = {k: [] for k in arms}
    for fn, _ in arms.values():
        fn()
        fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, (fn, _) in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.reps)
    assert bool(torch.isfinite(p_af).all()) and bool(torch.isfinite(p_adam).all())
    for name, (_, nbytes) in arms.items():
        ts = sorted(times[name])
        ms = ts[len(ts) // 2]
        print(json.dumps({"optimizer": name, "model": args.model, "parameters": p.n_params, "ms_per_update_median": round(ms, 3),
                          "ms_per_update_min_max": [round(ts[0], 3), round(ts[-1], 3)], "rounds": args.rounds, "reps_per_round": args.reps,
                          "algorithmic_bytes_per_update": nbytes, "gb_per_s": round(nbytes / ms / 1e6, 1),
                          "frac_of_hbm_spec": round(nbytes / ms / 1e6 / HBM_SPEC_GBPS, 3),
                          "frac_of_hbm_streaming": round(nbytes / ms / 1e6 / HBM_STREAM_GBPS, 3),
                          "state_bytes": 6 * n if name == "adamw" else 4 * plan.n_state,
                          "workspace_bytes": 0 if name == "adamw" else plan.workspace_nbytes,
                          "launches_per_update": 1 if name == "adamw" else 5, "work_items": None if name == "adamw" else plan.n_tiles}), flush=True)


def bench_peak(args):
    from ddpo_amd import lib as L
    from ddpo_amd.models.unet import UNet2DCondition, UNetConfig
    from ddpo_amd.diffusers_patch.scheduling_ddim import DDIMScheduler
    from ddpo_amd.training.policy_gradient import (AccumulatingTrainState, AdafactorConfig, AdamWConfig, train_fuse_default,
                                                   train_steps_fused)
    L.load()
    L.DATAPATH = L.shipped_datapath()
    dev = torch.device("cuda", 0)
    ucfg = UNetConfig.named(args.model)
    unet = UNet2DCondition(ucfg, dev)
    unet.params.init_synthetic(seed=0)
    unet.params.pack_bf16(bwd=True)
    sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", set_alpha_to_one=False, steps_offset=1,
                          prediction_type=ucfg.prediction_type)
    st = sched.set_timesteps(sched.create_state(device=dev), args.steps_per_update)
    b, hw = 2, args.resolution // 8
    gen = torch.Generator().manual_seed(3)
    lat = torch.randn(b, 4, hw, hw, generator=gen).to(dev)
    batch = {"latents": lat, "next_latents": 0.98 * lat + 0.05 * torch.randn(b, 4, hw, hw, generator=gen).to(dev),
             "ts": torch.tensor([481, 21], dtype=torch.int32, device=dev), "log_probs": torch.full((b,), -1.0, device=dev),
             "advantages": torch.tensor([0.7, -1.1], device=dev),
             "prompt_embeds": torch.randn(b, 77, ucfg.cross_attention_dim, generator=gen).to(dev),
             "uncond_embeds": torch.randn(b, 77, ucfg.cross_attention_dim, generator=gen).to(dev)}
    state = AccumulatingTrainState(unet, AdafactorConfig() if args.optimizer == "adafactor" else AdamWConfig())
    fuse = train_fuse_default(2 * b, hw * hw)
    left = args.steps_per_update
    while left > 0:
        f = min(fuse, left)
        left -= f
        train_steps_fused(state, [batch] * f, st, sched, True, 5.0, 1.0, 1e-4, do_opt_update=left == 0)
    torch.cuda.synchronize()
    assert state.step == 1 and bool(torch.isfinite(unet.params.flat).all())
    print(json.dumps({"optimizer": args.optimizer, "model": args.model, "resolution": args.resolution, "micro_steps_per_launch": fuse,
                      "peak_allocated_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 3),
                      "allocated_after_gb": round(torch.cuda.memory_allocated(dev) / 1e9, 3),
                      "optimizer_state_gb": round(sum(v.numel() * v.element_size() for k, v in state.opt_state.items() if k != "count") / 1e9, 4)}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["update", "peak"])
    ap.add_argument("--model", default="sd15")
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--optimizer", default="adafactor", choices=["adamw", "adafactor"])
    ap.add_argument("--steps-per-update", type=int, default=50, help="micro-steps per optimizer update (the entry point: n_inference_steps)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/adafactor_bench.py measures on the GPU"
    (bench_update if args.mode == "update" else bench_peak)(args)


if __name__ == "__main__":
    main()
