#!/usr/bin/env python
"""Timings of the on-device JPEG encoder on one GPU in one process, for a batch of `--images` float32 images of `--resolution`^2 (seeded noise
blended with a gradient, so the stream is neither empty nor worst-case), at quality 80 as the LLaVA rewards encode.

1. `launch_sequence_encode` / `launch_sequence_size`: the ddpo_jpeg_encode launch sequence (memset, jq_transform, jq_scan, jq_emit, jq_pack) next
   to the ddpo_jpeg_size one of the same build (..., jq_count), `--launches` calls between two device events each, the two in alternation round by
   round.  ddpo_jpeg_size is the yardstick; the difference is jq_pack minus jq_count.
2. `payload_host`: what a LLaVA reward's files cost per batch on the host path — the blocking device-to-host copy of the float32 batch the
   entrypoint makes, then PIL at quality 80.
3. `payload_device`: the same files from JpegEncoder on the device tensor (its stream, the copy of the lengths and of the files, the sync).
Arms 2 and 3 alternate round by round; medians are printed, one JSON line per measurement.  Per-kernel times: run this under
`rocprofv3 --kernel-trace --stats` with `--rounds 1` (kernels jq_transform, jq_scan, jq_emit, jq_count, jq_pack).

    python tools/jpeg_encode_bench.py [--rounds 5] [--launches 50] [--images 8] [--resolution 512]
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
    ap.add_argument("--quality", type=int, default=80)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/jpeg_encode_bench.py needs a GPU")

    from ddpo_amd import lib as L
    from ddpo_amd.models.jpeg_encode import JpegEncoder
    from ddpo_amd.training.callbacks import _to_jpeg_bytes
    n, r, q = args.images, args.resolution, args.quality
    rng = np.random.default_rng(0)
    ramp = np.add.outer(np.arange(r), np.arange(r))[None, :, :, None] / (2.0 * r)
    host = (0.7 * ramp + 0.3 * rng.random((n, r, r, 3))).astype(np.float32)
    dev = torch.from_numpy(host).cuda()
    encoder = JpegEncoder(quality=q)
    want = [_to_jpeg_bytes(im, q) for im in (host * 255).astype(np.uint8)]
    assert encoder(dev) == want, "device files differ from PIL's"
    shape = {"images": n, "resolution": r, "quality": q, "mean_bytes": float(np.mean([len(f) for f in want]))}

    ws = torch.empty(L.jpeg_size_workspace_bytes(n, r, r), dtype=torch.uint8, device="cuda")
    files = torch.empty((n, r * r * 3 + L.JPEG_FIXED_BYTES), dtype=torch.uint8, device="cuda")
    out = torch.empty(n, dtype=torch.int64, device="cuda")
    arms = {"encode": lambda: L.jpeg_encode(dev, q, workspace=ws, files=files), "size": lambda: L.jpeg_size(dev, q, workspace=ws, out=out)}
    seq = {k: [] for k in arms}
    for _ in range(args.rounds):
        for name, call in arms.items():
            call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                call()
            e1.record()
            e1.synchronize()
            seq[name].append(e0.elapsed_time(e1) * 1e3 / args.launches)
    for name in arms:
        print(json.dumps({"metric": "launch_sequence_" + name, "unit": "us_per_batch", "value": statistics.median(seq[name]), "all": seq[name], **shape}))

    t_copy, t_pil, t_dev = [], [], []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = dev.cpu().numpy()
        t1 = time.perf_counter()
        got = [_to_jpeg_bytes(im, q) for im in (h * 255).astype(np.uint8)]
        t2 = time.perf_counter()
        got_dev = encoder(dev)
        t3 = time.perf_counter()
        assert got == got_dev == want
        t_copy.append((t1 - t0) * 1e3), t_pil.append((t2 - t1) * 1e3), t_dev.append((t3 - t2) * 1e3)
    print(json.dumps({"metric": "payload_host", "unit": "ms_per_batch", "value": statistics.median(t_copy) + statistics.median(t_pil),
                      "blocking_d2h_ms": statistics.median(t_copy), "pil_encode_ms": statistics.median(t_pil),
                      "bytes_to_host": int(host.nbytes), **shape}))
    print(json.dumps({"metric": "payload_device", "unit": "ms_per_batch", "value": statistics.median(t_dev), "all": t_dev,
                      "bytes_to_host": int(n * (8 + max(len(f) for f in want))), **shape}))


if __name__ == "__main__":
    main()
