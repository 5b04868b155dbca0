#!/usr/bin/env python
"""What the two `--guidance_rescale` launches cost on one GPU: ddpo_cfg_rescale_fwd and ddpo_cfg_rescale_bwd timed INSIDE a captured HIP
graph (RUNBOOK rule 8: a Python loop around a 10 us kernel times the host), at the rows the sampler and the training step hand them.

    python tools/cfg_rescale_bench.py [--shapes 8x16384,8x36864] [--reps 200] [--rounds 7]

Each arm captures `reps` back-to-back launches on preallocated buffers into one graph, replays it `rounds` times between device events
and prints one JSON line: the median time per launch and the rate at which it moves the bytes that have to reach HBM when the re-reads of a
row are served by L2 (forward: the two inputs, the output and one re-read = four row passes; backward: three inputs, two outputs and one
re-read = six).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8x16384,8x36864")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args(argv)
    from ddpo_amd import lib as L, lib_cfg_rescale as LR
    lib = LR.load()
    dev = torch.device("cuda", 0)
    for shape in args.shapes.split(","):
        B, chw = (int(v) for v in shape.split("x"))
        g = torch.Generator().manual_seed(B + chw)
        t = torch.randn(B, chw, generator=g).to(dev)
        u = (t.cpu() + 0.33 * torch.randn(B, chw, generator=g)).to(dev)
        G = torch.randn(B, chw, generator=g).to(dev)
        out, d_t, d_u = torch.empty_like(t), torch.empty_like(t), torch.empty_like(t)
        stats = torch.empty(B, 4, device=dev)
        fwd = lambda s: lib.ddpo_cfg_rescale_fwd(L._p(t), L._p(u), 5.0, 0.7, L._p(out), L._p(stats), B, chw, s)
        bwd = lambda s: lib.ddpo_cfg_rescale_bwd(L._p(t), L._p(u), L._p(G), L._p(stats), 5.0, 0.7, L._p(d_t), L._p(d_u), B, chw, s)
        # row passes of 4 * chw bytes per row (the module docstring)
        for name, fn, passes in (("ddpo_cfg_rescale_fwd", fwd, 4), ("ddpo_cfg_rescale_bwd", bwd, 6)):
            assert fn(L._stream()) == 0
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(args.reps):
                    assert fn(L._stream()) == 0
            graph.replay()
            torch.cuda.synchronize()
            us = []
            for _ in range(args.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graph.replay()
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) / args.reps * 1e3)
            us.sort()
            nbytes = passes * 4 * B * chw
            print(json.dumps({"pass": name, "rows": B, "chw": chw, "us_per_launch_median": round(us[len(us) // 2], 2),
                              "us_per_launch_min_max": [round(us[0], 2), round(us[-1], 2)], "row_passes": passes, "bytes": nbytes,
                              "gb_per_s": round(nbytes / us[len(us) // 2] / 1e3, 1), "reps_in_graph": args.reps, "rounds": args.rounds}),
                  flush=True)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(d_t).all()) and bool(torch.isfinite(d_u).all())


if __name__ == "__main__":
    main()
