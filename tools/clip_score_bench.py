#!/usr/bin/env python
"""Timings of the CLIPScore reward on one GPU in one process (synthetic ViT-L/14 weights; needs DDPO_ALLOW_SYNTHETIC=1 without a checkpoint).

1. `ddpo_attention_causal_fwd` next to the unmasked `ddpo_attention_fwd` at the text tower's shape (B = 8, 12 heads, N = 77, d = 64): `--launches`
   launches of each captured into a HIP graph, the replays timed with device events, arms alternating round by round.
2. Latency of one reward evaluation on `--images` images of 512 x 512, host preprocessing included (what the worker thread of the entrypoint
   spends): the `aesthetic` scorer, and the `clip_score` scorer with a cold prompt cache (every prompt distinct, cache emptied before each call)
   and with a warm one.  Scorers alternate round by round.  The callbacks of training/callbacks.py are thin wrappers of these two objects.

Prints one JSON line per measurement.

    python tools/clip_score_bench.py [--rounds 5] [--launches 200] [--images 8] [--datapath bf16x3]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def _graph_us(fn, launches):
    """Capture `launches` calls of fn into a graph; returns a callable that replays it once and gives microseconds per launch."""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fn()
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(launches):
                fn()
        g.replay()
        s.synchronize()

    def timed():
        with torch.cuda.stream(s):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches

    return timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--datapath", default="bf16x3", help="what the entrypoint's reward thread runs: fp32_class_datapath of the sampler's")
    args = ap.parse_args()

    from ddpo_amd import lib as L
    from ddpo_amd.models.clip_score import ClipScorer
    from ddpo_amd.models.laion import AestheticScorer
    L.DATAPATH = args.datapath

    # ---- 1. the causal kernel next to the unmasked fp32 kernel
    B, heads, N, d = 8, 12, 77, 64
    C = heads * d
    buf = torch.randn(B * N, 3 * C, device="cuda")
    q, k, v = buf[:, :C], buf[:, C:2 * C], buf[:, 2 * C:]
    out = torch.empty(B * N, C, device="cuda")
    with L.datapath("fp32"):          # lib.attention picks the exact-fp32 kernel only on this datapath; the causal kernel is fp32 on all
        arms = {"ddpo_attention_causal_fwd": _graph_us(lambda: L.attention_causal(q, k, v, B, heads, N, d, out=out, ldq=3 * C, ldk=3 * C, ldv=3 * C),
                                                       args.launches),
                "ddpo_attention_fwd (unmasked)": _graph_us(lambda: L.attention(q, k, v, B, heads, N, N, d, out=out, ldq=3 * C, ldk=3 * C, ldv=3 * C),
                                                           args.launches)}
    us = {n: [] for n in arms}
    for _ in range(args.rounds):
        for n, f in arms.items():
            us[n].append(f())
    for n in arms:
        print(json.dumps({"kernel": n, "B": B, "heads": heads, "N": N, "d": d, "us_per_launch_median": statistics.median(us[n]),
                          "us_per_launch_rounds": us[n], "launches_per_graph": args.launches}), flush=True)

    # ---- 2. reward latency
    imgs = np.random.default_rng(0).random((args.images, 512, 512, 3), dtype=np.float32)
    prompts = [f"a {a} {b}" for a, b in zip(("cat", "dog", "horse", "monkey", "rabbit", "zebra", "spider", "bird") * 8,
                                            ("riding a bike", "playing chess", "washing the dishes") * 22)][:args.images]
    prompts = [f"{p} {i}" for i, p in enumerate(prompts)]          # every prompt distinct
    aes, clip = AestheticScorer(), ClipScorer()

    def cold():
        clip.prompts.rows.clear()
        return clip(imgs, prompts)

    arms = {"aesthetic": lambda: aes(imgs), "clip_score cold cache": cold, "clip_score warm cache": lambda: clip(imgs, prompts)}
    for f in arms.values():
        f()
    ms = {n: [] for n in arms}
    for _ in range(args.rounds):
        for n, f in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            ms[n].append((time.perf_counter() - t0) * 1e3)
    # the host share (PIL resize of the images) is common to all three
    from ddpo_amd.models.clip_vision import preprocess
    t0 = time.perf_counter()
    preprocess(imgs, 224)
    host_ms = (time.perf_counter() - t0) * 1e3
    for n in arms:
        print(json.dumps({"reward": n, "images": args.images, "datapath": args.datapath, "synthetic_weights": True, "ms_median": statistics.median(ms[n]),
                          "ms_rounds": ms[n], "of_which_host_preprocess_ms": host_ms}), flush=True)
    a, c, w = (statistics.median(ms[n]) for n in arms)
    print(json.dumps({"clip_score_cold_over_aesthetic": c / a, "clip_score_warm_over_aesthetic": w / a, "cold_minus_warm_ms": c - w}))


if __name__ == "__main__":
    main()
