#!/usr/bin/env python
"""Timings of the JPEG-size reward on one GPU in one process, for a batch of `--images` float32 images of `--resolution`^2 (seeded noise blended
with a gradient, so the stream is neither empty nor worst-case).

1. `device_launch_sequence`: the ddpo_jpeg_size launch sequence alone, `--launches` calls between two device events.
2. `reward_host`: what the `jpeg` reward costs per batch — the blocking device-to-host copy of the float32 batch the entrypoint makes, then PIL.
3. `reward_device`: what `jpeg_device` costs per batch — JpegSizer on the device tensor (its stream, the 8-byte-per-image copy back, the sync).
Arms 2 and 3 alternate round by round; medians are printed, one JSON line per measurement.  Per-kernel times: run this under
`rocprofv3 --kernel-trace --stats` with `--rounds 1` (kernels jq_transform, jq_scan, jq_emit, jq_count).

    python tools/jpeg_size_bench.py [--rounds 5] [--launches 50] [--images 8] [--resolution 512]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--resolution", type=int, default=512)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/jpeg_size_bench.py needs a GPU")

    from ddpo_amd import lib as L
    from ddpo_amd.models.jpeg_size import JpegSizer
    from ddpo_amd.training.callbacks import encode_jpeg
    n, r = args.images, args.resolution
    rng = np.random.default_rng(0)
    ramp = np.add.outer(np.arange(r), np.arange(r))[None, :, :, None] / (2.0 * r)
    host = (0.7 * ramp + 0.3 * rng.random((n, r, r, 3))).astype(np.float32)
    dev = torch.from_numpy(host).cuda()
    sizer = JpegSizer()
    want = [len(encode_jpeg(im)) for im in host]
    assert sizer(dev).tolist() == want, "device count differs from PIL"
    shape = {"images": n, "resolution": r, "mean_bytes": float(np.mean(want))}

    ws = torch.empty(L.jpeg_size_workspace_bytes(n, r, r), dtype=torch.uint8, device="cuda")
    out = torch.empty(n, dtype=torch.int64, device="cuda")
    seq = []
    for _ in range(args.rounds):
        L.jpeg_size(dev, 95, workspace=ws, out=out)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            L.jpeg_size(dev, 95, workspace=ws, out=out)
        e1.record()
        e1.synchronize()
        seq.append(e0.elapsed_time(e1) * 1e3 / args.launches)
    print(json.dumps({"metric": "device_launch_sequence", "unit": "us_per_batch", "value": statistics.median(seq), "all": seq, **shape}))

    t_copy, t_pil, t_dev = [], [], []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = dev.cpu().numpy()
        t1 = time.perf_counter()
        got = [len(encode_jpeg(im)) for im in h]
        t2 = time.perf_counter()
        got_dev = sizer(dev).tolist()
        t3 = time.perf_counter()
        assert got == got_dev == want
        t_copy.append((t1 - t0) * 1e3), t_pil.append((t2 - t1) * 1e3), t_dev.append((t3 - t2) * 1e3)
    print(json.dumps({"metric": "reward_host", "unit": "ms_per_batch", "value": statistics.median(t_copy) + statistics.median(t_pil),
                      "blocking_d2h_ms": statistics.median(t_copy), "pil_encode_ms": statistics.median(t_pil), **shape}))
    print(json.dumps({"metric": "reward_device", "unit": "ms_per_batch", "value": statistics.median(t_dev), "all": t_dev, **shape}))


if __name__ == "__main__":
    main()
