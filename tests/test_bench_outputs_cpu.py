"""bench.py's plain / --full split and --dump-outputs, on CPU: the options parse, the dump helper keeps the 64 MB cap with a fixed sample of
the arrays over their share (the same indices in every run), writes float32 / float64 only, and --dump-outputs outside --mode sample is refused."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_full_is_off_by_default_and_dump_outputs_takes_a_directory():
    a = bench.parse(["--steps", "3"])
    assert a.full is False and a.dump_outputs is None and a.steps == 3
    b = bench.parse(["--full", "--dump-outputs", "out"])
    assert b.full is True and b.dump_outputs == "out"


def _sd15_outputs(seed):
    g = torch.Generator().manual_seed(seed)
    return {"images": torch.rand(8, 512, 512, 3, generator=g), "final_latents": torch.randn(8, 4, 64, 64, generator=g),
            "latents": torch.randn(8, 50, 4, 64, 64, generator=g), "next_latents": torch.randn(8, 50, 4, 64, 64, generator=g),
            "log_probs": torch.randn(8, 50, generator=g), "timesteps": torch.randint(0, 1000, (8, 50), dtype=torch.int32, generator=g)}


def test_dump_outputs_keeps_the_cap_and_samples_the_same_elements_every_run(tmp_path):
    arrays = _sd15_outputs(0)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    names = sorted(f[:-4] for f in os.listdir(tmp_path / "a"))
    assert names == sorted(arrays) and sorted(os.listdir(tmp_path / "b")) == sorted(os.listdir(tmp_path / "a"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64_000_000
    for n in names:
        x, y = np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")
        assert x.dtype == (np.float64 if n == "timesteps" else np.float32) and np.array_equal(x, y)
    # small arrays whole; a sampled array holds its own elements (a subset of the flattened array, in index order)
    assert np.array_equal(np.load(tmp_path / "a" / "log_probs.npy"), arrays["log_probs"].numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "timesteps.npy"), arrays["timesteps"].numpy().astype(np.float64))
    lat = np.load(tmp_path / "a" / "latents.npy")
    flat = arrays["latents"].numpy().reshape(-1)
    assert 0 < lat.size < flat.size and np.isin(lat, flat).all()


def test_dump_outputs_is_refused_outside_the_sampling_mode():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--mode", "train", "--dump-outputs", "x"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "--dump-outputs" in r.stderr and not [l for l in r.stdout.splitlines() if l.startswith("{")]

