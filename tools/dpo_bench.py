#!/usr/bin/env python
"""What a Diffusion-DPO step (pipeline/dpo.py) costs on one GPU next to the RWR step (pipeline/finetune.py) at the same batch.

    python tools/dpo_bench.py [--model sd15] [--resolution 512] [--batch 4] [--rounds 5] [--reps 2]
        Builds the engine on synthetic weights, then times `training.diffusion.train_step` (RWR) and `training.diffusion_dpo.train_step`
        (the same forward, backward and optimizer update, plus one inference forward of the frozen copy and the pair pass in the place of
        the MSE pass) in ONE process on the same build, alternating round by round, each round with device events; train_cfg, so the
        U-Net batch is 2 x batch.  The reference is a copy of the policy: the work does not depend on the values.  Prints one JSON line
        per arm and one for ddpo_dpo_pair_fwd_bwd alone on buffers of the step's shape.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="sd15")
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--dpo-beta", type=float, default=5000.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/dpo_bench.py measures on the GPU"
    from ddpo_amd import lib as L
    from ddpo_amd import lib_dpo as LD
    from ddpo_amd.models.unet import UNet2DCondition, UNetConfig
    from ddpo_amd.training import diffusion, diffusion_dpo
    from ddpo_amd.training.kl_reference import KLReference
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdamWConfig
    from ddpo_amd.utils import prng
    L.load()
    L.DATAPATH = L.shipped_datapath()
    dev = torch.device("cuda", 0)
    ucfg = UNetConfig.named(args.model)
    unet = UNet2DCondition(ucfg, dev)
    unet.params.init_synthetic(seed=0)
    unet.params.pack_bf16(bwd=True)
    ref = KLReference(unet)
    b, hw = args.batch, args.resolution // 8
    gen = torch.Generator().manual_seed(3)
    moments = torch.randn(b, hw, hw, 8, generator=gen)
    moments[..., 4:] = moments[..., 4:] - 4.0
    y = np.resize(np.asarray([1.0, -1.0], dtype=np.float32), b // 2)
    batch = {"vae": moments.to(dev), "pref": np.stack([y, -y], 1).reshape(b),
             "prompt_embeds": torch.randn(b, 77, ucfg.cross_attention_dim, generator=gen).to(dev),
             "uncond_embeds": torch.randn(b, 77, ucfg.cross_attention_dim, generator=gen).to(dev)}
    sched = diffusion.DDPMNoiseScheduler()
    sst = sched.create_state(dev)
    static = (sched, None, True, 5.0)
    state = AccumulatingTrainState(unet, AdamWConfig(learning_rate=1e-9))
    key = prng.PRNGKey(0)
    arms = {"rwr": lambda: diffusion.train_step(state, None, batch, key, sst, static)[1],
            "dpo": lambda: diffusion_dpo.train_step(state, None, batch, key, sst, static, ref, args.dpo_beta)[1]["loss"]}
    for step in arms.values():
        step()
        step()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(args.rounds):
        for name, step in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                loss = step()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.reps)
            assert bool(torch.isfinite(loss))
    for name in arms:
        ms, lo, hi = median(times[name])
        print(json.dumps({"arm": name, "model": args.model, "resolution": args.resolution, "batch": b, "train_cfg": True,
                          "datapath": L.DATAPATH, "ms_per_step_median": round(ms, 2), "ms_per_step_min_max": [round(lo, 2), round(hi, 2)],
                          "rounds": args.rounds, "reps_per_round": args.reps}), flush=True)

    # the pass alone, on buffers of the step's shape
    chw = 4 * hw * hw
    ec, eu, rc, ru, tg = (torch.randn(b, chw, generator=torch.Generator().manual_seed(i)).to(dev) for i in range(5))
    pref = torch.as_tensor(batch["pref"], device=dev)
    call = lambda: LD.dpo_pair_fwd_bwd(ec, eu, rc, ru, tg, pref, 5.0, args.dpo_beta, True)
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
    nbytes = (5 + 3 + 2) * 4 * b * chw             # five inputs read for the sums, three read again for the gradient, two gradients written
    print(json.dumps({"pass": "ddpo_dpo_pair_fwd_bwd", "rows": b, "chw": chw, "us_per_call_median": round(us, 2),
                      "us_per_call_min_max": [round(lo, 2), round(hi, 2)], "launches": 2, "bytes": nbytes,
                      "includes": "the binding's five output allocations"}), flush=True)


if __name__ == "__main__":
    main()
