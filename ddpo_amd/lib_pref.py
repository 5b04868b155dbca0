"""ctypes binding of include/ddpo_pref.h: the preference-pair loss against the frozen pretrained policy (`--pg_loss d3po`) of libddpo_hip.so,
versioned on its own beside lib.py (ABI_VERSION here is ddpo_pref_abi_version(), not lib.ABI_VERSION).  Bound only when that loss is asked
for: with the default `ppo` nothing of this module is loaded or called (training/policy_gradient.py).
"""
import math
from ctypes import POINTER, byref, c_float, c_int, c_void_p

import torch

from . import lib as L

ABI_VERSION = 1          # must equal ddpo_pref_abi_version() of the loaded library (include/ddpo_pref.h)

_SIGS = {
    "ddpo_pref_abi_version": (c_int, []),
    "ddpo_ddim_pref_fwd_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_int,
                                       POINTER(L.DdimConsts), c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
}
EXPORTED_SYMBOLS = tuple(_SIGS)
_lib = None


def load():
    """Bind the preference-loss entry points of libddpo_hip.so (idempotent).  A library without them is an error: there is no other path."""
    global _lib
    if _lib is None:
        _lib = L.bind_side(_SIGS, "ddpo_pref_abi_version", ABI_VERSION, "preference-loss", "lib_pref.py")
    return _lib


def ddim_pref_fwd_bwd(eps_c, eps_u, ref_c, ref_u, x, x_next, ts, pref, guidance_scale, beta, train_cfg, consts, group=None):
    """The D3PO loss of adjacent row pairs (2p, 2p+1) of one DDIM step and its gradient, in the place of lib.ddim_logprob_ppo_fwd_bwd on the
    current stream.  `pref` (B,): +1 winner, -1 loser, 0 tie.  `group`: rows per micro-batch (default: the whole batch), even.
    Returns (d_eps_c, d_eps_u | None, per_pair (B // 2, 4) = {h_even, h_odd, s, loss}, info (B // group, 3) or (3,) without group =
    {pref_acc, pref_margin, loss})."""
    B = eps_c.shape[0]
    chw = eps_c.numel() // B
    if not (math.isfinite(beta) and beta > 0):
        raise ValueError(f"beta must be finite and > 0, got {beta}")
    g = B if group is None else int(group)
    if B <= 0 or B % 2 or g <= 0 or g % 2 or B % g:
        raise ValueError(f"batch of {B} rows is not a whole number of micro-batches of {g} rows in adjacent pairs")
    L.check_rows(B, chw, train_cfg, eps_c=eps_c, ref_c=ref_c, x=x, x_next=x_next, eps_u=eps_u, ref_u=ref_u)
    if ts.dtype != torch.int32 or ts.numel() != B:
        raise L.DdpoHipError(f"ts must be {B} int32 timesteps, got {ts.numel()} of {ts.dtype}")
    if L._f32(pref, "pref").numel() != B:
        raise L.DdpoHipError(f"pref must be {B} labels, got shape {tuple(pref.shape)}")
    d_c = torch.empty_like(eps_c)
    d_u = torch.empty_like(eps_c) if train_cfg else None
    per_pair = torch.empty(B // 2, 4, dtype=torch.float32, device=eps_c.device)
    info = torch.empty((3,) if group is None else (B // g, 3), dtype=torch.float32, device=eps_c.device)
    L._check(load().ddpo_ddim_pref_fwd_bwd(L._p(eps_c), L._p(eps_u if train_cfg else None), L._p(ref_c), L._p(ref_u if train_cfg else None),
                                           L._p(x), L._p(x_next), L._p(ts), L._p(pref), float(guidance_scale), float(beta),
                                           int(bool(train_cfg)), byref(consts), L._p(d_c), L._p(d_u), L._p(per_pair), L._p(info), B, g, chw,
                                           L._stream()),
             "ddpo_ddim_pref_fwd_bwd")
    return d_c, d_u, per_pair, info
