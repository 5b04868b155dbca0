"""pipeline/policy_gradient.py --pg_loss d3po end to end on the tiny argument set of tests/test_gpu_kl_entrypoint.py: two epochs on preference
pairs, the artefacts they leave, and the argument checks that speak before any model is loaded."""
import importlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_entrypoint_trains_on_preference_pairs(tmp_path, monkeypatch):
    monkeypatch.setenv("DDPO_MODEL_CONFIG", "tiny")
    monkeypatch.delenv("DDPO_RESUME", raising=False)
    monkeypatch.chdir(tmp_path)
    pg = importlib.import_module("pipeline.policy_gradient")
    flags = ["--dataset", "compressed-animals", "--resolution", "64", "--n_inference_steps", "4", "--sample_batch_size", "2",
             "--train_batch_size", "2", "--save_freq", "1", "--per_prompt_stats_min_count", "2",
             "--learning_rate", "1e-4", "--logbase", str(tmp_path / "run"), "--pg_loss", "d3po"]
    out = pg.main(flags + ["--num_train_epochs", "2"])              # main() returning is the script's exit status 0
    args = json.load(open(os.path.join(out["localpath"], "args.json")))
    assert args["pg_loss"] == "d3po" and args["d3po_beta"] == 0.1 and args["kl_coef"] == 0.0
    assert out["state"].step == 2 and "kl_ref" not in out
    acc = out["pref_acc"]
    assert len(acc) == 2 == len(out["mean_rewards"]) and all(0.0 <= v <= 1.0 for v in acc), acc
    for epoch in range(2):
        info = np.load(os.path.join(out["localpath"], "train_info", f"0_{epoch}_0.npy"), allow_pickle=True).item()
        assert set(info) == {"pref_acc", "pref_margin", "loss"}
        assert all(np.isfinite(v).all() and len(v) >= 1 for v in info.values())
        assert float(info["pref_acc"].mean()) == pytest.approx(acc[epoch], rel=1e-6, abs=1e-12)
        # one pair per epoch, both rows of one prompt, labelled by the sign of the reward difference
        labels = np.load(os.path.join(out["localpath"], "pref_labels", f"0_{epoch}.npy"))
        rewards = np.load(os.path.join(out["localpath"], "rewards", f"0_{epoch}.npy"))
        prompts = np.load(os.path.join(out["localpath"], "prompts", f"0_{epoch}.npy"))
        assert prompts[0] == prompts[1] and labels.tolist() == [np.sign(rewards[0] - rewards[1]), -np.sign(rewards[0] - rewards[1])]
    first = np.load(os.path.join(out["localpath"], "train_info", "0_0_0.npy"), allow_pickle=True).item()
    assert not first["pref_margin"].any()                           # epoch 0 trains before the first update: the policy IS the reference
    # the argument checks speak before any model is loaded
    with pytest.raises(SystemExit, match="--eta 0"):
        pg.main(flags + ["--eta", "0"])
    with pytest.raises(SystemExit, match="sample_batch_size must be even"):
        pg.main(flags + ["--sample_batch_size", "3"])
