"""pipeline/sample.py, then pipeline/dpo.py end to end on the tiny settings of tests/test_rwr_pipeline.py::
test_sample_then_finetune_end_to_end_tiny: the sampler writes 12 reward-labelled rows (3 prompts x 4, `--identical_batch True`), the
Diffusion-DPO entry point pairs them per epoch, trains, reports and leaves a checkpoint.

Learning rate 1e-5 and ONE epoch (3 steps of 2 pairs each, at the default dpo_beta 5000), chosen for this test on one MI355X so that
the last epoch's mean loss sits below log 2, the exact loss of any policy that equals the reference.  The first step of that epoch is at
log 2 exactly; the two that follow see pairs the first update has not seen.  What was measured (epoch means of the loss, epochs 0, 1, ..):
    lr 5e-8: 0.686 0.688 0.654 0.761 0.738 0.654        lr 1e-6: 0.440 0.631 2.05 2.50 1.66 0.603 4.32 1.72
    lr 1e-7: 0.635 0.625 0.732 0.814 0.872 0.617        lr 3e-6: 0.353 0.756 1.67 6.26 6.79 1.18 19.0 5.15
    lr 2e-7: 0.624 0.584 0.832 1.011 0.875 0.579        lr 1e-5: 0.307 1.87 4.14 21.8 23.7 20.0 57.5 16.5
    lr 3e-7: 0.555 0.584 1.049 1.084 0.790 0.474        lr 3e-5: 0.269 6.25 24.1 69.7 76.1 45.9 172 6.33
    lr 5e-7: 0.521 0.614 1.436 1.407 0.831 0.495        lr 1e-4: 0.236 44.9 176 168
    lr 3e-7 with the other GPU tests before it in one process: 0.647 0.746 1.373 1.262 0.569 0.710
Epoch 0 is below log 2 in every run in a process of its own, and the further the larger the learning rate; later epochs are not: with beta = 5000 a margin of 4e-4
already is s = 1, AdamW moves every weight of the random-init tiny U-Net by about the learning rate per step whatever the gradient's size,
and twelve rows under fresh noise, timesteps and pairings per epoch are a noisy measure whose sign per epoch follows the draws, not the
learning rate.  A longer run that ends below log 2 at one learning rate and in one process does not at another (the 3e-7 rows).

The two entry points run as the command line runs them, each in a fresh interpreter: called in this process behind other GPU tests the
same flags gave other epochs than alone (the 3e-7 row above; epoch 0 at 1e-5 measured 4.0, not 0.307).  The first step was at log 2
exactly there too, so the policy and its reference agree; a sampler that wrote other rewards, and so other labels, would explain it, but
which earlier test's state is picked up was not found.  What the run leaves is read from its directory (`dpo_history.json`) and its output."""
import importlib
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from ddpo_amd.utils import bucket

pytestmark = pytest.mark.gpu

EPOCHS, LR = 1, "1e-5"


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(script, flags, cwd):
    """`python pipeline/<script> flags...` in a fresh interpreter; its output."""
    env = dict(os.environ, DDPO_ALLOW_SYNTHETIC="1", DDPO_MODEL_CONFIG="tiny")
    env.pop("DDPO_RESUME", None)
    done = subprocess.run([sys.executable, os.path.join(ROOT, "pipeline", script)] + flags, cwd=cwd, env=env, capture_output=True, text=True,
                          timeout=240)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    return done.stdout


def test_sample_then_dpo_end_to_end_tiny(tmp_path, monkeypatch):
    import torch
    monkeypatch.chdir(tmp_path)
    logbase = tmp_path / "logs"
    common = ["--dataset", "compressed_animals_dpo", "--logbase", str(logbase), "--resolution", "64", "--seed", "3"]
    _run("sample.py", common + ["--n_inference_steps", "4", "--n_samples_per_device", "4", "--max_samples", "12", "--local_size", "8",
                                "--identical_batch", "True"], tmp_path)
    rd = bucket.LocalReader(str(logbase / "samples" / "0"))
    prompts = np.asarray(rd.get(slice(0, len(rd)), "inference_prompts")).reshape(-1)
    rewards = np.asarray(rd.get(slice(0, len(rd)), "jpeg"), dtype=np.float64).reshape(-1)
    assert len(rd) == 12 and sorted(np.unique(prompts, return_counts=True)[1].tolist()) == [4, 4, 4]
    log = _run("dpo.py", common + ["--train_batch_size", "4", "--num_train_epochs", str(EPOCHS), "--learning_rate", LR, "--save_freq", "100"],
               tmp_path)
    out = json.load(open(logbase / "models" / "1" / "dpo_history.json"))
    hist = out["history"]
    print("\n[dpo end to end, tiny] " + " | ".join(f"epoch {h['epoch']}: loss {h['loss']:.6f} acc {h['implicit_acc']:.3f} margin {h['margin']:.3e}"
                                                 for h in hist))
    # the pair count the log reports is make_pairs on the store, epoch by epoch
    reported = [tuple(int(v) for v in m) for m in re.findall(r"Epoch \d+ \| pairs kept (\d+) \| ties dropped (\d+) \| rows left over (\d+)", log)]
    assert len(reported) == EPOCHS == len(hist)
    for epoch, (kept, ties, leftover) in enumerate(reported):
        idx, y = bucket.make_pairs(prompts, rewards, epoch)                         # pair_seed 0 + epoch
        assert kept == len(idx) == hist[epoch]["pairs"] and kept + ties == 6 and leftover == 0
    assert out["steps"] == sum(2 * k // 4 for k, _, _ in reported)
    for h in hist:
        assert all(math.isfinite(h[k]) for k in ("loss", "implicit_acc", "margin", "mse", "ref_mse")), h
        assert all(f"{k} {h[k]:.6g}" in log for k in ("loss", "margin"))            # the epoch means are printed
    # before the first update the policy equals the reference: D = 0 exactly on every row
    log2 = torch.log1p(torch.ones((), device="cuda")).cpu().numpy()
    assert np.float32(out["first_step"]["loss"]).view(np.int32) == log2.view(np.int32) and out["first_step"]["margin"] == 0.0
    assert hist[-1]["loss"] < math.log(2.0)
    ck = logbase / "models" / "1" / "checkpoints"
    assert any(f.startswith("checkpoint_") for f in os.listdir(ck))
    # the argument check speaks before any model is loaded
    dpo = importlib.import_module("pipeline.dpo")
    with pytest.raises(SystemExit, match="train_batch_size must be even"):
        dpo.main(common + ["--train_batch_size", "3"])
    with pytest.raises(SystemExit, match="finite number > 0"):
        dpo.main(common + ["--dpo_beta", "0"])
