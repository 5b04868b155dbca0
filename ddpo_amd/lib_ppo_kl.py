"""ctypes binding of include/ddpo_ppo_kl.h: the KL penalty to the frozen pretrained policy (`--kl_coef`) of libddpo_hip.so, versioned on its
own beside lib.py (ABI_VERSION here is ddpo_ppo_kl_abi_version(), not lib.ABI_VERSION).  Bound only when a penalty is asked for: with
kl_coef == 0 nothing of this module is loaded or called (training/policy_gradient.py).
"""
import ctypes
import math
from ctypes import POINTER, byref, c_float, c_int, c_void_p

import torch

from . import lib as L

ABI_VERSION = 1          # must equal ddpo_ppo_kl_abi_version() of the loaded library (include/ddpo_ppo_kl.h)

_SIGS = {
    "ddpo_ppo_kl_abi_version": (c_int, []),
    "ddpo_ddim_kl_ref_fwd_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_int, POINTER(L.DdimConsts),
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
}
EXPORTED_SYMBOLS = tuple(_SIGS)
_lib = None


def load():
    """Bind the KL-penalty entry points of libddpo_hip.so (idempotent).  A library without them is an error: there is no other path."""
    global _lib
    if _lib is not None:
        return _lib
    L.load()                                    # "not built" is reported once, there
    lib = ctypes.CDLL(L.LIB_PATH)
    for name, (res, args) in _SIGS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise L.DdpoHipError(f"libddpo_hip.so does not export {name}: rebuild with `python __graft_entry__.py`") from None
        fn.restype = res
        fn.argtypes = args
    if lib.ddpo_ppo_kl_abi_version() != ABI_VERSION:
        raise L.DdpoHipError(f"libddpo_hip.so has KL-penalty ABI version {lib.ddpo_ppo_kl_abi_version()}, lib_ppo_kl.py expects {ABI_VERSION}")
    _lib = lib
    return lib


def ddim_kl_ref_fwd_bwd(eps_c, eps_u, ref_c, ref_u, ts, guidance_scale, kl_coef, train_cfg, consts, d_eps_c, d_eps_u, loss_info=None,
                        group=None):
    """kl_coef * KL(policy || frozen reference) of one DDIM step, behind lib.ddim_logprob_ppo_fwd_bwd on the current stream: the penalty's
    gradient is ADDED into d_eps_c / d_eps_u (that call's outputs) and kl_coef * kl_info into column 2 of `loss_info` (its info, optional).
    `group` as there: rows per micro-batch (default: the whole batch).  Returns (kl_per_sample (B,), kl_info (B // group,) or () without group)."""
    B = eps_c.shape[0]
    chw = eps_c.numel() // B
    if not (math.isfinite(kl_coef) and kl_coef >= 0):
        raise ValueError(f"kl_coef must be finite and >= 0, got {kl_coef}")
    if group is not None and (group <= 0 or B % group):
        raise ValueError(f"batch of {B} rows is not a whole number of micro-batches of {group}")
    need = [("eps_c", eps_c), ("ref_c", ref_c), ("d_eps_c", d_eps_c)]
    if train_cfg:
        need += [("eps_u", eps_u), ("ref_u", ref_u), ("d_eps_u", d_eps_u)]
    for name, t in need:
        if t is None:
            raise L.DdpoHipError(f"{name} is required" + (" under train_cfg" if name.endswith("_u") else ""))
        L._f32(t, name)
        if t.numel() != B * chw:
            raise L.DdpoHipError(f"{name} has {t.numel()} elements, expected {B} x {chw}")
    if ts.dtype != torch.int32 or ts.numel() != B:
        raise L.DdpoHipError(f"ts must be {B} int32 timesteps, got {ts.numel()} of {ts.dtype}")
    n_mb = 1 if group is None else B // group
    if loss_info is not None and (L._f32(loss_info, "loss_info").numel() != 3 * n_mb):
        raise L.DdpoHipError(f"loss_info must be the PPO launch's ({n_mb}, 3) info, got shape {tuple(loss_info.shape)}")
    kl_per_sample = torch.empty(B, dtype=torch.float32, device=eps_c.device)
    kl_info = torch.empty(() if group is None else (n_mb,), dtype=torch.float32, device=eps_c.device)
    L._check(load().ddpo_ddim_kl_ref_fwd_bwd(L._p(eps_c), L._p(eps_u if train_cfg else None), L._p(ref_c), L._p(ref_u if train_cfg else None),
                                             L._p(ts), float(guidance_scale), float(kl_coef), int(bool(train_cfg)), byref(consts),
                                             L._p(d_eps_c), L._p(d_eps_u if train_cfg else None), L._p(kl_per_sample), L._p(kl_info),
                                             L._p(loss_info), B, B if group is None else int(group), chw, L._stream()),
             "ddpo_ddim_kl_ref_fwd_bwd")
    return kl_per_sample, kl_info
