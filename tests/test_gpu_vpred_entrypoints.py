"""The entry points on the v-prediction toy (`DDPO_MODEL_CONFIG=tiny21`): pipeline/policy_gradient.py --guidance_rescale on the tiny argument
set of tests/test_gpu_kl_entrypoint.py, and pipeline/sample.py --guidance_rescale, then pipeline/dpo.py on the recipe of
tests/test_gpu_dpo_entrypoint.py (each in a fresh interpreter, as the command line runs them) with the v target."""
import importlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from ddpo_amd.utils import bucket

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_policy_gradient_trains_with_rescaled_guidance(tmp_path, monkeypatch):
    monkeypatch.setenv("DDPO_MODEL_CONFIG", "tiny21")
    monkeypatch.delenv("DDPO_RESUME", raising=False)
    monkeypatch.chdir(tmp_path)
    pg = importlib.import_module("pipeline.policy_gradient")
    flags = ["--dataset", "compressed-animals", "--resolution", "64", "--n_inference_steps", "4", "--sample_batch_size", "2",
             "--train_batch_size", "2", "--save_freq", "1", "--per_prompt_stats_min_count", "2",
             "--learning_rate", "1e-4", "--logbase", str(tmp_path / "run"), "--guidance_rescale", "0.7"]
    out = pg.main(flags + ["--num_train_epochs", "2"])
    args = json.load(open(os.path.join(out["localpath"], "args.json")))
    assert args["guidance_rescale"] == 0.7 and args["kl_coef"] == 0.0
    assert len(out["mean_rewards"]) == 2 and all(np.isfinite(v) for v in out["mean_rewards"]) and out["state"].step == 2
    for epoch in (0, 1):
        info = np.load(os.path.join(out["localpath"], "train_info", f"0_{epoch}_0.npy"), allow_pickle=True).item()
        assert set(info) == {"approx_kl", "clipfrac", "loss"} and all(np.isfinite(v).all() for v in info.values())
    # the argument check speaks before any model is loaded
    with pytest.raises(SystemExit, match="needs --train_cfg True"):
        pg.main(flags + ["--train_cfg", "False"])
    with pytest.raises(SystemExit, match=r"finite number in \[0, 1\]"):
        pg.main(flags[:-1] + ["1.5"])


def _run(script, flags, cwd):
    """`python pipeline/<script> flags...` in a fresh interpreter; its output."""
    env = dict(os.environ, DDPO_ALLOW_SYNTHETIC="1", DDPO_MODEL_CONFIG="tiny21")
    env.pop("DDPO_RESUME", None)
    done = subprocess.run([sys.executable, os.path.join(ROOT, "pipeline", script)] + flags, cwd=cwd, env=env, capture_output=True, text=True,
                          timeout=240)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    return done.stdout


def test_sample_then_dpo_on_a_v_prediction_model(tmp_path, monkeypatch):
    import torch
    monkeypatch.chdir(tmp_path)
    logbase = tmp_path / "logs"
    common = ["--dataset", "compressed_animals_dpo", "--logbase", str(logbase), "--resolution", "64", "--seed", "3"]
    _run("sample.py", common + ["--n_inference_steps", "4", "--n_samples_per_device", "4", "--max_samples", "12", "--local_size", "8",
                                "--identical_batch", "True", "--guidance_rescale", "0.7"], tmp_path)
    rd = bucket.LocalReader(str(logbase / "samples" / "0"))
    assert len(rd) == 12
    meta = json.load(open(logbase / "samples" / "0" / "metadata.json"))
    assert meta["guidance_rescale"] == 0.7 and meta["guidance_scale"] == 5.0
    _run("dpo.py", common + ["--train_batch_size", "4", "--num_train_epochs", "1", "--learning_rate", "1e-5", "--save_freq", "100"], tmp_path)
    run = logbase / "models" / "1"
    args = json.load(open(run / "args.json"))
    assert args["prediction_type"] == "v_prediction" and args["dpo_beta"] == 5000.0 and args["synthetic_weights"] is True
    out = json.load(open(run / "dpo_history.json"))
    assert out["steps"] >= 1 and len(out["history"]) == 1
    for h in out["history"]:
        assert all(math.isfinite(h[k]) for k in ("loss", "implicit_acc", "margin", "mse", "ref_mse")), h
    # before the first update the policy equals the reference: D = 0 exactly on every row, against the v target as against the noise
    log2 = torch.log1p(torch.ones((), device="cuda")).cpu().numpy()
    assert np.float32(out["first_step"]["loss"]).view(np.int32) == log2.view(np.int32) and out["first_step"]["margin"] == 0.0
    assert any(f.startswith("checkpoint_") for f in os.listdir(run / "checkpoints"))
