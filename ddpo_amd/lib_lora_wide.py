"""ctypes binding of include/ddpo_lora_wide.h: the adapter gradients of LoRA layers too wide for lib.lora_wgrad (the GEGLU feed-forward
layers of `--lora_targets attn_ff`) of libddpo_hip.so, versioned on its own beside lib.py (ABI_VERSION here is
ddpo_lora_wide_abi_version(), not lib.ABI_VERSION).  Bound only when an adapted layer lies outside lib.lora_wgrad's limits: importing the
engine, or training with `--lora_targets attn`, loads nothing of this module.
"""
from ctypes import c_float, c_int, c_size_t, c_void_p

from . import lib as L

ABI_VERSION = 1          # must equal ddpo_lora_wide_abi_version() of the loaded library (include/ddpo_lora_wide.h)

_SIGS = {
    "ddpo_lora_wide_abi_version": (c_int, []),
    "ddpo_lora_wgrad_wide_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "ddpo_lora_wgrad_wide": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_int, c_int, c_int, c_int, c_float, c_void_p, c_size_t, c_void_p]),
}
EXPORTED_SYMBOLS = tuple(_SIGS)
_lib = None


def load():
    """Bind the wide adapter-gradient entry points of libddpo_hip.so (idempotent).  A library without them is an error: there is no other path."""
    global _lib
    if _lib is None:
        _lib = L.bind_side(_SIGS, "ddpo_lora_wide_abi_version", ABI_VERSION, "wide-LoRA", "lib_lora_wide.py")
    return _lib


def lora_wgrad_wide(x, dy, A, B, dA, dB, s):
    """lib.lora_wgrad for K, N up to 16384: dA (K, r) += s * x^T (dY B^T), dB (r, N) += s * (x A)^T dY.  x: fp32 (M, K) (a row-strided view is
    taken as is) or bf16 hi / lo `Planes`."""
    M, N = dy.shape
    K, r = A.shape
    for t, nm in ((dy, "dy"), (A, "A"), (B, "B"), (dA, "dA"), (dB, "dB")):
        L._f32(t, nm)
    if B.shape != (r, N) or dA.shape != A.shape or dB.shape != B.shape or not 1 <= r <= L.LORA_MAX_RANK:
        raise L.DdpoHipError(f"lora_wgrad_wide: A {tuple(A.shape)}, B {tuple(B.shape)}, dA {tuple(dA.shape)}, dB {tuple(dB.shape)}, "
                             f"dY {tuple(dy.shape)}")
    if isinstance(x, L.Planes):
        if x.fmt != 0 or x.rows != M or x.C != K:
            raise L.DdpoHipError("lora_wgrad_wide: the planes must be bf16 hi / lo planes of shape (M, K)")
        xp, ldx, hi, lo, ldp = None, 0, L._p(x.hi), L._p(x.lo), x.ld
    else:
        L._f32(x, "x")
        if tuple(x.shape) != (M, K):
            raise L.DdpoHipError(f"lora_wgrad_wide: x {tuple(x.shape)} vs dY {tuple(dy.shape)} and A {tuple(A.shape)}")
        ldx = int(x.stride(0)) if M > 1 else K
        xp, hi, lo, ldp = L._p_rows(x), None, None, 0
    lddy = int(dy.stride(0)) if M > 1 else N
    lib = load()
    nb = int(lib.ddpo_lora_wgrad_wide_ws_bytes(M, K, N, r))
    ws = L._scratch(nb, dy.device, "lora_wide")
    L._check(lib.ddpo_lora_wgrad_wide(xp, ldx, hi, lo, int(ldp), L._p_rows(dy), lddy, L._p(A), L._p(B), L._p(dA), L._p(dB), int(M), int(K),
                                      int(N), int(r), float(s), L._p(ws), ws.numel(), L._stream()), "ddpo_lora_wgrad_wide")
    return dA, dB
