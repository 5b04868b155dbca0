"""pipeline/policy_gradient.py --kl_coef end to end on the tiny argument set of
tests/test_gpu_adafactor.py::test_entrypoint_runs_adafactor_and_refuses_to_resume_it_as_adamw: two epochs, then one more from the checkpoints."""
import importlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_entrypoint_trains_with_a_kl_penalty_and_resumes_against_the_pretrained_weights(tmp_path, monkeypatch):
    monkeypatch.setenv("DDPO_MODEL_CONFIG", "tiny")
    monkeypatch.delenv("DDPO_RESUME", raising=False)
    monkeypatch.chdir(tmp_path)
    pg = importlib.import_module("pipeline.policy_gradient")
    flags = ["--dataset", "compressed-animals", "--resolution", "64", "--n_inference_steps", "4", "--sample_batch_size", "2",
             "--train_batch_size", "2", "--save_freq", "1", "--per_prompt_stats_min_count", "2",
             "--learning_rate", "1e-4", "--logbase", str(tmp_path / "run"), "--kl_coef", "0.1"]
    out = pg.main(flags + ["--num_train_epochs", "2"])              # main() returning is the script's exit status 0
    assert json.load(open(os.path.join(out["localpath"], "args.json")))["kl_coef"] == 0.1
    kl = out["kl_ref"]
    assert len(kl) == 2 == len(out["mean_rewards"]) and all(np.isfinite(v) and v >= 0.0 for v in kl), kl
    assert kl[1] > 0.0, kl                                          # one update in, the policy has left the pretrained weights
    assert out["state"].step == 2
    info = np.load(os.path.join(out["localpath"], "train_info", "0_1_0.npy"), allow_pickle=True).item()
    assert set(info) == {"approx_kl", "clipfrac", "loss", "kl_ref"} and float(info["kl_ref"].mean()) == pytest.approx(kl[1], rel=1e-6)
    # resumed for one more epoch: the reference is the pretrained model, not the resumed weights, so the penalty is there from its first step
    monkeypatch.setenv("DDPO_RESUME", os.path.join(str(tmp_path / "run"), "models/pg/checkpoints"))
    out2 = pg.main(flags + ["--num_train_epochs", "3"])
    assert len(out2["kl_ref"]) == 1 and np.isfinite(out2["kl_ref"][0]) and out2["kl_ref"][0] > 0.0, out2["kl_ref"]
    assert out2["state"].step == 3
    # the argument check speaks before any model is loaded
    monkeypatch.delenv("DDPO_RESUME")
    with pytest.raises(SystemExit, match="--eta 0"):
        pg.main(flags + ["--eta", "0"])
