"""Host side of `--pg_loss d3po` (preference pairs): the labels of adjacent row pairs and the entrypoint's argument check.

Two trajectories of one prompt sit on rows (2p, 2p+1).  Only the sign of their reward difference is used, so any `filter_field` serves as the
judge and no reward scale, per-prompt tracker or advantage normalisation is involved.
"""
import math

import numpy as np


def pair_labels(rewards):
    """Labels of the rows, in the order of `rewards` (the global order DataParallel.gather_rewards returns): y = sign(r[2p] - r[2p+1]),
    row 2p gets +y and row 2p+1 gets -y — +1 winner, -1 loser, 0 for both rows of a tie.  float32 (n,)."""
    r = np.asarray(rewards, dtype=np.float64).reshape(-1)
    if r.size % 2:
        raise ValueError(f"preference pairs need an even number of rewards, got {r.size}")
    y = np.sign(r[0::2] - r[1::2])
    return (np.stack([y, -y], 1).reshape(-1) + 0.0).astype(np.float32)      # + 0.0: a tie is +0.0 on both rows


def check_d3po_args(pg_loss, d3po_beta, eta, sample_batch_size, train_batch_size):
    """The entrypoint's argument check, as a plain function: a message to exit with, or None.  With eta == 0 the DDIM step is deterministic:
    sigma is then the 1e-6 floor of the log-prob and a log-ratio in its units means nothing (the reason of kl_reference.check_kl_args)."""
    if pg_loss not in ("ppo", "d3po"):
        return f"--pg_loss must be ppo or d3po, got {pg_loss!r}"
    if pg_loss == "ppo":
        return None
    beta = float(d3po_beta)
    if not (math.isfinite(beta) and beta > 0.0):
        return f"--d3po_beta must be a finite number > 0, got {beta}"
    if float(eta) == 0.0:
        return ("--pg_loss d3po needs a stochastic sampler: with --eta 0 the policy's standard deviation is the 1e-6 floor of the log-prob "
                "and the log-ratio to the pretrained policy is meaningless")
    for name, v in (("sample_batch_size", sample_batch_size), ("train_batch_size", train_batch_size)):
        if int(v) % 2:
            return f"--pg_loss d3po trains on adjacent pairs of rows: --{name} must be even, got {v}"
    return None
