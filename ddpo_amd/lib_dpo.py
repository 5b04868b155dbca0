"""ctypes binding of include/ddpo_dpo.h: the Diffusion-DPO loss on ranked pairs of stored samples (`pipeline/dpo.py`) of libddpo_hip.so,
versioned on its own beside lib.py (ABI_VERSION here is ddpo_dpo_abi_version(), not lib.ABI_VERSION).  Bound only when that experiment is
asked for: importing pipeline/finetune.py or pipeline/policy_gradient.py loads nothing of this module.
"""
import math
from ctypes import c_float, c_int, c_void_p

import torch

from . import lib as L

ABI_VERSION = 1          # must equal ddpo_dpo_abi_version() of the loaded library (include/ddpo_dpo.h)

_SIGS = {
    "ddpo_dpo_abi_version": (c_int, []),
    "ddpo_dpo_pair_fwd_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_int,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
}
EXPORTED_SYMBOLS = tuple(_SIGS)
_lib = None


def load():
    """Bind the Diffusion-DPO entry points of libddpo_hip.so (idempotent).  A library without them is an error: there is no other path."""
    global _lib
    if _lib is None:
        _lib = L.bind_side(_SIGS, "ddpo_dpo_abi_version", ABI_VERSION, "Diffusion-DPO", "lib_dpo.py")
    return _lib


def dpo_pair_fwd_bwd(eps_c, eps_u, ref_c, ref_u, target, pref, guidance_scale, beta, train_cfg):
    """The Diffusion-DPO loss of adjacent row pairs (2p, 2p+1) and its gradient, in the place of lib.rwr_mse_fwd_bwd on the current stream.
    `target` (B, C, h, w): the regression target of the model's prediction type (the DDPM noise; v for a v-prediction model).  `pref` (B,): +1 winner, -1 loser, 0 tie.
    Returns (d_eps_c, d_eps_u | None, per_row (B, 2) = {m, D}, per_pair (B // 2, 3) = {s, loss, q},
    info (5,) = {loss, implicit_acc, margin, mse, ref_mse})."""
    B = eps_c.shape[0]
    chw = eps_c.numel() // B
    if not (math.isfinite(beta) and beta > 0):
        raise ValueError(f"beta must be finite and > 0, got {beta}")
    if B <= 0 or B % 2:
        raise ValueError(f"batch of {B} rows is not a whole number of adjacent pairs")
    L.check_rows(B, chw, train_cfg, eps_c=eps_c, ref_c=ref_c, target=target, eps_u=eps_u, ref_u=ref_u)
    if L._f32(pref, "pref").numel() != B:
        raise L.DdpoHipError(f"pref must be {B} labels, got shape {tuple(pref.shape)}")
    dev = eps_c.device
    d_c = torch.empty_like(eps_c)
    d_u = torch.empty_like(eps_c) if train_cfg else None
    per_row = torch.empty(B, 2, dtype=torch.float32, device=dev)
    per_pair = torch.empty(B // 2, 3, dtype=torch.float32, device=dev)
    info = torch.empty(5, dtype=torch.float32, device=dev)
    L._check(load().ddpo_dpo_pair_fwd_bwd(L._p(eps_c), L._p(eps_u if train_cfg else None), L._p(ref_c), L._p(ref_u if train_cfg else None),
                                          L._p(target), L._p(pref), float(guidance_scale), float(beta), int(bool(train_cfg)), L._p(d_c),
                                          L._p(d_u), L._p(per_row), L._p(per_pair), L._p(info), B, chw, L._stream()),
             "ddpo_dpo_pair_fwd_bwd")
    return d_c, d_u, per_row, per_pair, info
