#!/usr/bin/env python
"""Timings of the thumbnail reward on one GPU in one process, for a batch of `--images` float32 images of `--resolution`^2 held on the device
(what the VAE decoder leaves), ViT-L/14 on seeded synthetic weights, the entrypoint's bf16x3 datapath.

1. `reward_host_path`: the `thumbnail` reward — blocking device-to-host copy of the batch, truncation, 3 N `Image.resize` calls, 4 N
   `clip_vision.preprocess` (PIL), upload of the pixel values, the tower's own im2col, the tower on 4 N images.  Wall time, split into the copy,
   the PIL part and the rest (upload + tower, until the embedder's stream has drained).
2. `reward_device_path`: the `thumbnail_device` reward — three `lib.resize_u8` and four `lib.clip_preprocess` launches + `forward_patches` on
   the embedder's stream.  Wall time until the features are on the host.
   Arms 1 and 2 alternate rep by rep; medians of `--reps` repetitions after `--warmup`.  The features of the two arms must be equal.
3. `resize_u8_launches`: the three ddpo_resize_u8 launches (by 4, 8, 16) alone, `--launches` triples captured into one graph (a Python loop would
   time the host), with the bytes they must move (3 x N H W 3 x 4 in, N H W 3 x (1/16 + 1/64 + 1/256) out) and their share of the 8 TB/s HBM peak;
   then `resize_u8_launch_by_<d>`, each of the three on its own, the same way.
One JSON line per measurement.

    DDPO_ALLOW_SYNTHETIC=1 timeout -k 10 600 python tools/thumbnail_bench.py [--reps 8] [--warmup 2] [--launches 20] [--images 8] [--resolution 512]
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
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--config", default="vit-l/14")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/thumbnail_bench.py needs a GPU")

    from ddpo_amd import lib as L
    from ddpo_amd.models.thumbnail import FACTORS, ThumbnailEmbedder, thumbnail_pixel_values
    from ddpo_amd.training.callbacks import _mean_turn_angle
    L.DATAPATH = "bf16x3"
    n, r = args.images, args.resolution
    rng = np.random.default_rng(0)
    ramp = np.add.outer(np.arange(r), np.arange(r))[None, :, :, None] / (2.0 * r)
    dev = torch.from_numpy((0.7 * ramp + 0.3 * rng.random((n, r, r, 3))).astype(np.float32)).cuda()
    emb = ThumbnailEmbedder(config=args.config)
    cfg = emb.cfg
    shape = {"images": n, "resolution": r, "config": args.config, "synthetic_weights": bool(emb.synthetic)}

    def host_path():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = dev.cpu().numpy()
        t1 = time.perf_counter()
        px = thumbnail_pixel_values(h, cfg.image)
        t2 = time.perf_counter()
        with emb.on_stream(), L.fp32_class_datapath():
            feats = emb.tower(torch.from_numpy(px).to(emb.device)).cpu()
        t3 = time.perf_counter()
        return feats.numpy(), dict(d2h_ms=(t1 - t0) * 1e3, pil_ms=(t2 - t1) * 1e3, upload_tower_ms=(t3 - t2) * 1e3, wall_ms=(t3 - t0) * 1e3)

    def device_path():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        feats = emb(dev)
        t1 = time.perf_counter()
        return feats, dict(wall_ms=(t1 - t0) * 1e3)

    rows_a, rows_b = [], []
    for i in range(args.warmup + args.reps):
        fa, ta = host_path()
        fb, tb = device_path()
        assert np.array_equal(fa, fb), "the device path's features differ from the host path's"
        if i >= args.warmup:
            rows_a.append(ta), rows_b.append(tb)
    med = lambda rows: {k: statistics.median(x[k] for x in rows) for k in rows[0]}
    print(json.dumps({"metric": "reward_host_path", "unit": "ms_per_batch", **med(rows_a), "wall_all": [round(x["wall_ms"], 3) for x in rows_a], **shape}))
    print(json.dumps({"metric": "reward_device_path", "unit": "ms_per_batch", **med(rows_b), "wall_all": [round(x["wall_ms"], 3) for x in rows_b], **shape}))
    print(json.dumps({"metric": "thumbnail_scores", "value": [round(float(s), 4) for s in _mean_turn_angle(fb, n)], **shape}))

    outs = {d: torch.empty(n, r // d, r // d, 3, dtype=torch.uint8, device="cuda") for d in FACTORS}
    side = torch.cuda.Stream()

    def graph_us(factors):
        """per-repetition time of one lib.resize_u8 launch per factor, `--launches` repetitions captured into one graph"""
        def body():
            for d in factors:
                L.resize_u8(dev, r // d, r // d, out=outs[d])

        with torch.cuda.stream(side):
            for _ in range(3):
                body()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            for _ in range(args.launches):
                body()
        us = []
        for i in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.replay()
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                us.append(e0.elapsed_time(e1) * 1e3 / args.launches)
        return us

    note = "back-to-back replays re-read the same inputs: they may be served from the Infinity Cache"
    for factors in [FACTORS] + [(d,) for d in FACTORS]:
        us = graph_us(factors)
        nbytes = sum(n * r * r * 3 * 4 + outs[d].numel() for d in factors)
        t = statistics.median(us)
        name = "resize_u8_launches" if len(factors) > 1 else f"resize_u8_launch_by_{factors[0]}"
        print(json.dumps({"metric": name, "unit": "us_per_three_launches" if len(factors) > 1 else "us_per_launch", "value": t,
                          "all": [round(x, 2) for x in us], "bytes": nbytes, "GBps": nbytes / t / 1e3,
                          "fraction_of_hbm_peak": nbytes / (t * 1e-6) / HBM_PEAK, "geometry": [L.resize_u8_geometry(r, r, r // d, r // d) for d in factors],
                          "note": note, **shape}))


if __name__ == "__main__":
    main()
