#!/usr/bin/env python
"""Timings of the aesthetic reward's input stage on one GPU in one process, for a batch of `--images` float32 images of `--resolution`^2 held on
the device (what the VAE decoder leaves), ViT-L/14 on seeded synthetic weights, the entrypoint's bf16x3 datapath.

1. `reward_host_path`: the `aesthetic` reward — blocking device-to-host copy of the batch, `clip_vision.preprocess` (PIL), upload of the pixel values,
   the tower's own im2col, tower + MLP.  Wall time of the host part (copy, PIL) and device events around the scorer's stream work.
2. `reward_device_path`: the `aesthetic_device` reward — `lib.clip_preprocess` + `forward_patches` + MLP on the scorer's stream, same events.
   Arms 1 and 2 alternate rep by rep; medians of `--reps` repetitions after `--warmup`.  The scores of the two arms must be equal.
3. `clip_preprocess_launch`: the ddpo_clip_preprocess launch alone, `--launches` of them captured into one graph (a Python loop would time the
   host), with the bytes it must move (N H W 3 x 4 in, N g g k_pad x 4 out) and their share of the 8 TB/s HBM peak.
One JSON line per measurement.

    DDPO_ALLOW_SYNTHETIC=1 python tools/clip_preprocess_bench.py [--reps 12] [--warmup 2] [--launches 20] [--images 8] [--resolution 512]
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

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--config", default="vit-l/14")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/clip_preprocess_bench.py needs a GPU")

    from ddpo_amd import lib as L
    from ddpo_amd.models.clip_vision import preprocess
    from ddpo_amd.models.laion import AestheticScorer
    L.DATAPATH = "bf16x3"
    n, r = args.images, args.resolution
    rng = np.random.default_rng(0)
    ramp = np.add.outer(np.arange(r), np.arange(r))[None, :, :, None] / (2.0 * r)
    dev = torch.from_numpy((0.7 * ramp + 0.3 * rng.random((n, r, r, 3))).astype(np.float32)).cuda()
    scorer = AestheticScorer(config=args.config)
    cfg, st = scorer.cfg, scorer.stream
    shape = {"images": n, "resolution": r, "config": args.config}

    def timed(body):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(st), L.fp32_class_datapath():
            e0.record()
            scores = body()
            e1.record()
        st.synchronize()
        return scores, e0.elapsed_time(e1)

    def host_path():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = dev.cpu().numpy()
        t1 = time.perf_counter()
        px = preprocess(h, cfg.image)
        t2 = time.perf_counter()
        scores, ev = timed(lambda: scorer._score(scorer.tower(torch.from_numpy(px).to(scorer.device))))
        t3 = time.perf_counter()
        return scores, dict(d2h_ms=(t1 - t0) * 1e3, pil_ms=(t2 - t1) * 1e3, stream_ms=ev, wall_ms=(t3 - t0) * 1e3)

    def device_path():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scores, ev = timed(lambda: scorer._score(scorer.tower.forward_patches(L.clip_preprocess(dev, cfg.image, cfg.patch, cfg.k_pad))))
        t1 = time.perf_counter()
        return scores, dict(stream_ms=ev, wall_ms=(t1 - t0) * 1e3)

    rows_a, rows_b = [], []
    for i in range(args.warmup + args.reps):
        sa, ta = host_path()
        sb, tb = device_path()
        assert np.array_equal(sa, sb), "the device path's scores differ from the host path's"
        if i >= args.warmup:
            rows_a.append(ta), rows_b.append(tb)
    med = lambda rows: {k: statistics.median(x[k] for x in rows) for k in rows[0]}
    print(json.dumps({"metric": "reward_host_path", "unit": "ms_per_batch", **med(rows_a), "wall_all": [round(x["wall_ms"], 3) for x in rows_a], **shape}))
    print(json.dumps({"metric": "reward_device_path", "unit": "ms_per_batch", **med(rows_b), "wall_all": [round(x["wall_ms"], 3) for x in rows_b], **shape}))

    g = cfg.image // cfg.patch
    out = torch.empty(n * g * g, cfg.k_pad, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(3):
            L.clip_preprocess(dev, cfg.image, cfg.patch, cfg.k_pad, out=out)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for _ in range(args.launches):
            L.clip_preprocess(dev, cfg.image, cfg.patch, cfg.k_pad, out=out)
    us = []
    for i in range(args.warmup + args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        e1.synchronize()
        if i >= args.warmup:
            us.append(e0.elapsed_time(e1) * 1e3 / args.launches)
    nbytes = n * r * r * 3 * 4 + n * g * g * cfg.k_pad * 4
    t = statistics.median(us)
    print(json.dumps({"metric": "clip_preprocess_launch", "unit": "us_per_launch", "value": t, "all": [round(x, 2) for x in us], "bytes": nbytes,
                      "GBps": nbytes / t / 1e3, "fraction_of_hbm_peak": nbytes / (t * 1e-6) / HBM_PEAK,
                      "note": "back-to-back replays re-read the same inputs: they may be served from the Infinity Cache", **shape}))


if __name__ == "__main__":
    main()
