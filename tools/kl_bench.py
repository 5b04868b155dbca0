#!/usr/bin/env python
"""What `--kl_coef` costs on one GPU: the full-size fused training step with and without the KL penalty, the penalty's own pass alone, and
the device memory of the frozen reference U-Net.

    python tools/kl_bench.py [--model sd15] [--resolution 512] [--rounds 5] [--reps 2]
        Builds the engine on synthetic weights in the entry point's geometry (fused micro-steps of 2 samples x CFG, graph-replayed, no
        optimizer update), then times the step with kl_coef = 0 and kl_coef > 0 in ONE process on the same build, alternating round by round,
        each round with device events.  The reference is a copy of the policy: the work does not depend on the values.  Prints one JSON line
        per arm (sample-timesteps/s), one for ddpo_ddim_kl_ref_fwd_bwd alone on buffers of the step's shape, and one for the memory
        (torch.cuda.memory_allocated before and after the reference is built: parameters plus forward-only weight planes).
    python tools/kl_bench.py --d3po
        The same, with the `--pg_loss d3po` step (the preference-pair pass in the place of the PPO launch, the same frozen forward) in the
        place of the kl_coef = 0 arm, alternating with the kl_coef > 0 arm (two captured full-size steps fit the device's memory, three do
        not); ddpo_ddim_pref_fwd_bwd is timed alone as well.  In this mode the stored log-probs of the PPO arm are set to the policy's own
        after the warm-up (ratio 1: nothing is clipped), so that both arms send a live gradient into the U-Net backward: with the
        placeholder log-probs of the default mode every row's PPO gradient is clipped or underflows to zero, the backward multiplies
        zeros, and the device clocks higher than under a real cotangent.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="sd15")
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--kl-coef", type=float, default=0.05)
    ap.add_argument("--d3po-beta", type=float, default=0.1)
    ap.add_argument("--d3po", action="store_true", help="time the d3po step against the kl_coef > 0 step instead of kl_coef = 0 against it")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/kl_bench.py measures on the GPU"
    from ddpo_amd import lib as L
    from ddpo_amd import lib_ppo_kl as LK
    from ddpo_amd import lib_pref as LP
    from ddpo_amd.models.unet import UNet2DCondition, UNetConfig
    from ddpo_amd.diffusers_patch.scheduling_ddim import DDIMScheduler
    from ddpo_amd.training.kl_reference import KLReference
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdamWConfig, train_fuse_default, train_steps_fused
    L.load()
    L.DATAPATH = L.shipped_datapath()
    dev = torch.device("cuda", 0)
    ucfg = UNetConfig.named(args.model)
    unet = UNet2DCondition(ucfg, dev)
    unet.params.init_synthetic(seed=0)
    unet.params.pack_bf16(bwd=True)
    torch.cuda.synchronize()
    mem0 = torch.cuda.memory_allocated(dev)
    ref = KLReference(unet)
    torch.cuda.synchronize()
    mem1 = torch.cuda.memory_allocated(dev)
    sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", set_alpha_to_one=False, steps_offset=1,
                          prediction_type=ucfg.prediction_type)
    st = sched.set_timesteps(sched.create_state(device=dev), 50)
    b, hw = 2, args.resolution // 8
    gen = torch.Generator().manual_seed(3)
    lat = torch.randn(b, 4, hw, hw, generator=gen).to(dev)
    batch = {"latents": lat, "next_latents": 0.98 * lat + 0.05 * torch.randn(b, 4, hw, hw, generator=gen).to(dev),
             "ts": torch.tensor([481, 21], dtype=torch.int32, device=dev), "log_probs": torch.full((b,), -1.0, device=dev),
             "advantages": torch.tensor([0.7, -1.1], device=dev),
             "prompt_embeds": torch.randn(b, 77, ucfg.cross_attention_dim, generator=gen).to(dev),
             "uncond_embeds": torch.randn(b, 77, ucfg.cross_attention_dim, generator=gen).to(dev)}
    state = AccumulatingTrainState(unet, AdamWConfig())
    fuse = train_fuse_default(2 * b, hw * hw)
    arms = {f"kl_coef={args.kl_coef:g}": dict(kl_coef=args.kl_coef, ref_unet=ref)}
    arms = dict(arms, **{"pg_loss=d3po": dict(loss="d3po", d3po_beta=args.d3po_beta, ref_unet=ref)}) if args.d3po else dict({"kl_coef=0": {}}, **arms)
    pair = dict(batch, advantages=torch.tensor([1.0, -1.0], device=dev))      # the two samples as one preference pair

    def step(kw):
        bt = pair if kw.get("loss") == "d3po" else batch
        return train_steps_fused(state, [bt] * fuse, st, sched, True, 5.0, 1.0, 1e-4, do_opt_update=False, **kw)[1]

    for kw in arms.values():                       # graph capture, then one replay
        step(kw)
        infos = step(kw)
        if args.d3po and "loss" not in kw:         # the PPO arm: stored log-probs = the policy's own, read by the next replay
            batch["log_probs"] = infos[0]["log_prob"].clone()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(args.rounds):
        for name, kw in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                infos = step(kw)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.reps)
            assert all(bool(torch.isfinite(i["loss"])) for i in infos)
    for name in arms:
        ms, lo, hi = median(times[name])
        print(json.dumps({"arm": name, "model": args.model, "resolution": args.resolution, "micro_steps_per_launch": fuse, "samples": b,
                          "ms_per_launch_median": round(ms, 2), "ms_per_launch_min_max": [round(lo, 2), round(hi, 2)],
                          "sample_timesteps_per_s": round(b * fuse / ms * 1e3, 2), "rounds": args.rounds, "reps_per_round": args.reps}), flush=True)

    # the pass alone, on buffers of the fused step's shape
    B, chw = b * fuse, 4 * hw * hw
    ec, eu, rc, ru, dc, du = (torch.randn(B, chw, generator=torch.Generator().manual_seed(i)).to(dev) for i in range(6))
    ts = torch.tensor([481, 21] * fuse, dtype=torch.int32, device=dev)
    info = torch.zeros(fuse, 3, device=dev)
    consts = sched.kernel_consts(st, 1.0)
    call = lambda: LK.ddim_kl_ref_fwd_bwd(ec, eu, rc, ru, ts, 5.0, args.kl_coef, True, consts, dc, du, loss_info=info, group=b)
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    pass_us = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            call()
        e1.record()
        torch.cuda.synchronize()
        pass_us.append(e0.elapsed_time(e1) / 50 * 1e3)
    us, lo, hi = median(pass_us)
    nbytes = 8 * 4 * B * chw                       # four U-Net outputs read, two gradients read and written
    print(json.dumps({"pass": "ddpo_ddim_kl_ref_fwd_bwd", "rows": B, "chw": chw, "us_per_call_median": round(us, 2),
                      "us_per_call_min_max": [round(lo, 2), round(hi, 2)], "launches": 2, "bytes": nbytes,
                      "gb_per_s": round(nbytes / us / 1e3, 1)}), flush=True)
    # the preference pass alone, on the same buffers: it reads x and x_next as well and writes the gradients instead of updating them
    pref = torch.tensor([1.0, -1.0] * fuse, device=dev)
    pcall = lambda: LP.ddim_pref_fwd_bwd(ec, eu, rc, ru, dc, du, ts, pref, 5.0, args.d3po_beta, True, consts, group=b)
    for _ in range(5):
        pcall()
    torch.cuda.synchronize()
    pass_us = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            pcall()
        e1.record()
        torch.cuda.synchronize()
        pass_us.append(e0.elapsed_time(e1) / 50 * 1e3)
    us, lo, hi = median(pass_us)
    nbytes = (6 + 4 + 2) * 4 * B * chw             # six inputs read for the sums, four read again for the gradient, two gradients written
    print(json.dumps({"pass": "ddpo_ddim_pref_fwd_bwd", "rows": B, "chw": chw, "us_per_call_median": round(us, 2),
                      "us_per_call_min_max": [round(lo, 2), round(hi, 2)], "launches": 2, "bytes": nbytes,
                      "gb_per_s": round(nbytes / us / 1e3, 1)}), flush=True)
    print(json.dumps({"reference_unet": args.model, "parameters": ref.params.n_params, "parameter_bytes": ref.nbytes(),
                      "allocated_before_gb": round(mem0 / 1e9, 3), "allocated_after_gb": round(mem1 / 1e9, 3),
                      "reference_total_gb": round((mem1 - mem0) / 1e9, 3), "datapath": L.DATAPATH}), flush=True)


if __name__ == "__main__":
    main()
