"""ctypes binding of libddpo_hip.so (the C ABI declared in include/ddpo_hip.h).

PyTorch is used only as the device allocator / stream provider: every wrapper takes torch CUDA tensors, passes
their raw device pointers plus the current HIP stream to the C entry point and returns torch tensors.
There is NO fallback path: if the shared library is missing or a call fails, an exception is raised.
"""
import contextlib
import ctypes
import functools
import math
import os
import threading
from ctypes import c_void_p, c_int, c_int32, c_int64, c_uint32, c_float, c_double, c_size_t, POINTER, byref

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libddpo_hip.so")

PRED_TYPES = {"epsilon": 0, "v_prediction": 1, "sample": 2}


class LoraLayer(ctypes.Structure):
    _fields_ = [("w0", c_void_p), ("w", c_void_p), ("a", c_void_p), ("b", c_void_p), ("K", c_int), ("N", c_int), ("r", c_int), ("s", c_float)]


class DdimConsts(ctypes.Structure):
    _fields_ = [("alphas_cumprod", c_void_p), ("num_train_timesteps", c_int), ("step_ratio", c_int),
                ("final_alpha_cumprod", c_float), ("eta", c_float), ("pred_type", c_int)]


class GemmDesc(ctypes.Structure):
    _fields_ = [("src", c_void_p), ("ld_src", c_int),
                ("w", c_void_p), ("w_trans", c_int),
                ("bias", c_void_p),
                ("rowbias", c_void_p), ("rows_per_batch", c_int), ("ld_rowbias", c_int),
                ("residual", c_void_p), ("ld_res", c_int),
                ("out", c_void_p), ("ld_out", c_int),
                ("alpha", c_float),
                ("M", c_int), ("N", c_int), ("K", c_int),
                ("ksize", c_int), ("stride", c_int), ("pad", c_int), ("upsample", c_int),
                ("B", c_int), ("H", c_int), ("W", c_int), ("Cin", c_int),
                ("OH", c_int), ("OW", c_int),
                ("w_dgrad", c_int), ("ld_w", c_int), ("splits", c_int), ("accumulate", c_int), ("epilogue", c_int),
                ("out_hi", c_void_p), ("out_lo", c_void_p), ("ld_planes", c_int), ("w_layout", c_int),
                ("w_scale", c_void_p), ("planes_fmt", c_int), ("colsum", c_void_p), ("aux_out", c_void_p), ("res_rows", c_int)]


ABI_VERSION = 15         # must equal ddpo_abi_version() of the loaded library (include/ddpo_hip.h)

_SIGS = {
    "ddpo_abi_version": (c_int, []),
    "ddpo_sizeof_gemm_desc": (c_size_t, []),
    "ddpo_sizeof_ddim_consts": (c_size_t, []),
    "ddpo_gemm_tile_launch_counts": (c_int, [c_void_p, c_int]),
    "ddpo_gemm_splitk_min_ktiles": (c_int, []),
    "ddpo_threefry_bits_host": (c_int, [c_uint32, c_uint32, c_int64, c_void_p]),
    "ddpo_threefry_normal": (c_int, [c_uint32, c_uint32, c_void_p, c_void_p, c_int64, c_void_p]),
    "ddpo_ddim_step_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, POINTER(DdimConsts),
                                   c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "ddpo_ddim_logprob_ppo_fwd_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_float, c_float, c_int, POINTER(DdimConsts), c_void_p, c_void_p,
                                              c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ddpo_rwr_noisy_latents": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p, c_int, c_int, c_int,
                                       c_void_p]),
    "ddpo_rwr_mse_fwd_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                     c_void_p]),
    "ddpo_grad_sqnorm": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_void_p]),
    "ddpo_adamw_bf16mu_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_double, c_double,
                                       c_double, c_double, c_double, c_double, c_double, c_int, c_int, c_int, c_void_p]),
    "ddpo_groupnorm_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "ddpo_groupnorm_fwd": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                   c_float, c_int, c_void_p, c_void_p, c_void_p]),
    "ddpo_layernorm_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p]),
    "ddpo_gemm_conv_fwd": (c_int, [POINTER(GemmDesc), c_void_p]),
    "ddpo_gemm_conv_wgrad": (c_int, [POINTER(GemmDesc), c_void_p]),
    "ddpo_gemm_conv_fwd_bf16": (c_int, [POINTER(GemmDesc), c_void_p, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "ddpo_gemm_conv_wgrad_bf16x3": (c_int, [POINTER(GemmDesc), c_void_p]),
    "ddpo_gemm_conv_wgrad_bf16x3_planes": (c_int, [POINTER(GemmDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ddpo_gemm_conv_fwd_bf16_planes": (c_int, [POINTER(GemmDesc), c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_size_t,
                                               c_void_p]),
    "ddpo_split_planes_bf16": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p]),
    "ddpo_groupnorm_fwd_planes": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                          c_float, c_int, c_void_p, c_void_p, c_void_p]),
    "ddpo_layernorm_fwd_planes": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_int, c_void_p]),
    "ddpo_pack_weights_bf16": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ddpo_pack_weights_bf16_kblocked": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "ddpo_pack_weights_bf16_kblocked_dgrad": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "ddpo_pack_weights_f16mx": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ddpo_split_planes_f16mx": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p]),
    "ddpo_gemm_conv_fwd_f16mx_planes": (c_int, [POINTER(GemmDesc), c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    # folded nearest-2x up-sampler (additive to ABI v14)
    "ddpo_fold_up2x_weights": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "ddpo_conv_up2x_folded_fwd": (c_int, [POINTER(GemmDesc), c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    # attention forwards: q_batches after ldq; the 16-bit forms take f16p first and both output forms (o, ldo | o_hi, o_lo, ld_planes)
    "ddpo_attention_fwd": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int,
                                   c_int, c_int, c_int, c_float, c_void_p]),
    "ddpo_attention_fwd_x16_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "ddpo_attention_fwd_x16": (c_int, [c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                       c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_size_t, c_void_p]),
    "ddpo_attention_kv_images_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "ddpo_attention_pack_kv": (c_int, [c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_size_t, c_int, c_int, c_int, c_int, c_void_p]),
    "ddpo_attention_fwd_images": (c_int, [c_int, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p, c_int, c_void_p, c_void_p, c_int,
                                          c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "ddpo_attention_bwd": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "ddpo_attention_bwd_x16": (c_int, [c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "ddpo_groupnorm_stats_floats": (c_size_t, [c_int, c_int, c_int]),
    "ddpo_groupnorm_bwd_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "ddpo_groupnorm_bwd": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                   c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ddpo_layernorm_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ddpo_layernorm_bwd_ws_bytes": (c_size_t, [c_int, c_int]),
    "ddpo_geglu_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "ddpo_silu_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "ddpo_colsum_accum": (c_int, [c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "ddpo_sumpool2x2": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "ddpo_add": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "ddpo_geglu_fwd": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "ddpo_silu_fwd": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "ddpo_quick_gelu_fwd": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "ddpo_l2_normalize_rows": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "ddpo_timestep_embedding": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "ddpo_nchw_to_nhwc": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ddpo_nhwc_to_nchw": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ddpo_copy_cols": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int64, c_int, c_void_p]),
    "ddpo_stage_cfg_inputs": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "ddpo_softmax_rows": (c_int, [c_void_p, c_int64, c_int, c_float, c_void_p]),
    "ddpo_scale_shift_clip": (c_int, [c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float, c_void_p]),
    # LoRA adapters (additive to ABI v14; csrc/lora.hip)
    "ddpo_lora_merge": (c_int, [c_void_p, c_int, c_int64, c_void_p]),
    "ddpo_lora_wgrad_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "ddpo_lora_wgrad": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_int, c_int, c_int, c_int, c_float, c_void_p, c_size_t, c_void_p]),
    # CLIP text tower + CLIPScore reward (additive to ABI v14; csrc/clip_text.hip)
    "ddpo_attention_causal_fwd": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "ddpo_gather_rows": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "ddpo_cosine_rows": (c_int, [c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p]),
    # JPEG file size without the file (additive to ABI v14; csrc/jpeg_size.hip)
    "ddpo_jpeg_size_workspace_bytes": (c_int, [c_int, c_int, c_int, POINTER(c_size_t)]),
    "ddpo_jpeg_size": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p]),
    "ddpo_jpeg_size_host": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    # ... and the file itself (additive to ABI v14; the same file)
    "ddpo_jpeg_encode_max_bytes": (c_int, [c_int, c_int, POINTER(c_size_t)]),
    "ddpo_jpeg_encode": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p]),
    "ddpo_jpeg_encode_host": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    # CLIP image preprocessing into the patch matrix (additive to ABI v14; csrc/clip_preprocess.hip)
    "ddpo_clip_preprocess": (c_int, [c_void_p] + [c_int] * 10 + [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "ddpo_clip_preprocess_host": (c_int, [c_void_p] + [c_int] * 10 + [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    # symmetry rewards: exact per-image sums, the four right-angle turns (additive to ABI v14; csrc/symmetry.hip)
    "ddpo_symmetry_stats_workspace_bytes": (c_int, [c_int, c_int, c_int, c_int, POINTER(c_size_t)]),
    "ddpo_symmetry_stats": (c_int, [c_void_p] + [c_int] * 5 + [c_void_p, c_void_p, c_size_t, c_void_p]),
    "ddpo_symmetry_stats_host": (c_int, [c_void_p] + [c_int] * 5 + [c_void_p]),
    "ddpo_rotate4_u8": (c_int, [c_void_p] + [c_int] * 4 + [c_void_p, c_void_p]),
    "ddpo_rotate4_u8_host": (c_int, [c_void_p] + [c_int] * 4 + [c_void_p]),
    # 8-bit bicubic resize to bytes (additive to ABI v14; csrc/resize_u8.hip)
    "ddpo_resize_u8": (c_int, [c_void_p] + [c_int] * 6 + [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "ddpo_resize_u8_host": (c_int, [c_void_p] + [c_int] * 6 + [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGS)
_lib = None
# Contraction datapath of the GEMM / conv kernels: "fp32" (exact v_mfma_f32_32x32x2_f32), "bf16x3" (bf16-split MFMA,
# 3 passes, ~1e-5 relative) or "bf16" (single pass = XLA's TPU default precision).  The bf16 paths are used for
# weights that have been registered with `pack_weights` (ParamStore.pack_bf16); everything else stays on fp32.
DATAPATH = os.environ.get("DDPO_DATAPATH", "fp32")


DATAPATHS = ("fp32", "bf16x3", "bf16", "f16mx")
# The datapath the entrypoints (pipeline/*.py), load_unet and bench.py select when DDPO_DATAPATH is not set — since round 4 the f16mx
# operator (bf16x3 stays selectable: DDPO_DATAPATH=bf16x3).  The full-size parity tests are parametrised over this name, so whatever ships
# is what is held to the oracle (tests/test_gpu_train_parity.py, test_gpu_model.py, test_gpu_rwr.py, test_gpu_headline_geometry.py).
SHIPPED_DATAPATH = "f16mx"


def shipped_datapath():
    """DDPO_DATAPATH if set, else SHIPPED_DATAPATH."""
    name = os.environ.get("DDPO_DATAPATH") or SHIPPED_DATAPATH
    if name not in DATAPATHS:
        raise ValueError(f"DDPO_DATAPATH={name!r}: expected one of {DATAPATHS}")
    return name


# "f16mx" (round 3; the shipped default since round 4): every plane-eligible forward contraction with a LONG reduction (K >= MX_MIN_K: all 3x3 convolutions, FF2 of the
# lower levels — a property of the layer, never of the batch), and FF1 + GEGLU where the model registers it as an f16mx layer (pack_weights_geglu(mx=True);
# FF1_MX below: the one compute-bound short reduction of the step), runs on the f16 + MX-fp8 cross-term kernel (ddpo_gemm_conv_fwd_f16mx_planes); its
# activation planes come from the producing kernel (GroupNorm / LayerNorm / GEMM output stages, which ask planes_pay() for the consumer's
# format) or, when the producer wrote fp32 (training forward: the weight gradients read the fp32 tensor), from ddpo_split_planes_f16mx on the
# way in — the same bits either way, so the sampler and the training forward of a layer always take the same arithmetic.  Everything else
# (short reductions — where the f16mx kernel measured no gain —, non-eligible layers, data / weight gradients, attention) runs as under bf16x3.
# DDPO_MX_CROSS=0 (opt-in, NOT what ships; round 6): the f16mx layers run WITHOUT their cross terms — a_h * w_h on the f16 MFMA only, the single-plane
# kernels of ABI v14 on the planes' 16-bit halves.  One f16 pass per product is the reference's own arithmetic class (its TPUs run one bf16 pass) with
# f16's 11-bit significand instead of bf16's 8.  Measured (profiles/r06_parity_f16x1.log, r06_ab_f16x1.log): sampling 4.07 -> 4.80 images/s (+18 %),
# U-Net forward 7.3e-4 rms against float64 (f16mx 4e-5), and at full size the train step's block gradient norms 2.4e-3 / gradient vector 2.7e-2 —
# OUTSIDE north_star's 1e-3.  It exists to price the cross terms on this power-bound chip (bench.py `extra.f16x1`), not to be run.
MX_CROSS = os.environ.get("DDPO_MX_CROSS", "1") == "1"
MX_MIN_K = int(os.environ.get("DDPO_MX_MIN_K", "2560"))          # (the env override exists for the routing experiments of tools/; 2560 is what is validated)
_TLS = threading.local()


def current_datapath():
    """The datapath in force for the calling thread: a `with datapath(...)` override, else the process default `DATAPATH`."""
    return getattr(_TLS, "datapath", None) or DATAPATH


class datapath:
    """`with lib.datapath("bf16x3"):` — datapath override for the CALLING THREAD only (the reward models run on their own thread
    and stream next to the sampler), restored on exit."""

    def __init__(self, name):
        if name not in DATAPATHS:
            raise ValueError(f"unknown datapath {name!r}")
        self.name = name

    def __enter__(self):
        self.prev = getattr(_TLS, "datapath", None)
        _TLS.datapath = self.name
        return self

    def __exit__(self, *exc):
        _TLS.datapath = self.prev
        return False


def fp32_class_datapath():
    """Datapath for models whose PARAMETERS the reference keeps in fp32 whatever `dtype` the SD trees are cast to (the reward models:
    /root/reference/ddpo/utils/serialization.py:343-350 casts text_encoder / vae / unet only): the current one, except that the
    single-pass `bf16` selected by `load_unet(dtype=bfloat16)` is replaced by `bf16x3`."""
    cur = current_datapath()
    return datapath("bf16x3" if cur in ("bf16", "f16mx") else cur)


def _x3():
    """Three-pass class (fp32-equivalent) MFMA datapaths: bf16x3, and f16mx whose non-plane-fed layers and gradients ARE bf16x3."""
    return current_datapath() in ("bf16x3", "f16mx")


def _mx():
    return current_datapath() == "f16mx"


# Single-pass bf16 ("bf16": XLA's TPU default precision, BASELINE configs[4]'s dtype) on the PLANE-FED kernels (round 6, ABI v14): the norms and
# GEMM output stages write the same bf16 hi / lo planes as under bf16x3 and the consumer reads the hi planes only (both lo pointers NULL at
# ddpo_gemm_conv_fwd_bf16_planes) — hi = bf16(x) is exactly the operand the fp32-fed single-pass kernel forms in its loader, so the two are
# bit-identical.  DDPO_BF16_PLANES=0: the fp32-fed kernels everywhere (rounds 1-5).
BF16_PLANES = os.environ.get("DDPO_BF16_PLANES", "1") == "1"


def _planes_dp():
    """Datapaths whose contractions can be plane-fed."""
    return _x3() or (BF16_PLANES and current_datapath() == "bf16")


def mx_layer(w):
    """True when the forward contraction with weight tensor `w` runs on the f16mx kernel: f16mx datapath, f16mx weight planes registered
    (pack_weights packs them for K >= MX_MIN_K).  A property of the layer — the batch never enters."""
    if not _mx():
        return False
    ent = PACKED.get(w.data_ptr())
    return ent is not None and "mx" in ent


def splitk_min_ktiles():
    """The shortest reduction, in 32-wide k-tiles, for which the forward GEMM dispatcher considers a split-K at all — read from the library
    (ddpo_gemm_splitk_min_ktiles: the dispatcher's own constants).  Below it the k partition of a layer cannot depend on the launch's row count."""
    return int(load().ddpo_gemm_splitk_min_ktiles())


def norm_planes(w, cin, rows, training=False):
    """What a normalisation layer in front of the contraction with weight `w` should emit: 0 = the fp32 tensor, 1 = bf16 hi / lo planes,
    2 = f16mx planes (= planes_pay's answer), except that the TRAINING forward keeps fp32 in front of an f16mx layer (its weight gradient runs
    on bf16x3 from the fp32 tensor; the forward GEMM splits it on the way in) and wherever DDPO_TRAIN_PLANES is off."""
    p = planes_pay(w, cin, rows)
    if training and (p == 2 or not TRAIN_PLANES or not _x3()):      # (single-pass bf16: its weight-gradient kernels take fp32 operands)
        return 0
    return p


SPLITK_WS_BYTES = 64 << 20       # scratch for the deterministic split-K of under-filled launches
# data_ptr of an fp32 weight tensor -> dict(K, N, fwd=(hi, lo, Kp), bwd=(hi, lo) | None, w_layout) and, where registered: dg (data-gradient planes,
# _pack_dgrad_planes), mx (f16mx planes, pack_weights), geglu (pack_weights_geglu), fold (pack_weights_up2x_folded)
PACKED = {}

# Plane-fed GEMMs (bf16x3 datapath): GroupNorm / LayerNorm write their result as bf16
# hi / lo planes and the consuming conv / linear layers fetch both operands by LDS-DMA (ddpo_gemm_conv_fwd_bf16_planes).
# Bit-identical to the fp32-fed kernels (tests/test_gpu_planes.py).  ON by default since round 2 (DDPO_PLANES=0 switches it
# off): on one box, back to back, the sampling bench went 3.222 / 3.243 (off) -> 3.268 (k-loop mode 6) -> 3.297 (mode 7, three
# weight stages) -> 3.344 images/s (mode 7 + 256x320 tiles at the 64x64 level) — measured in the first session of round 2, whose log was
# lost with its container; the per-layer A/B of the final state is profiles/r02_gemm_breakdown_ab.md, the k-loop mode A/B profiles/r02_ab_apl_mode.log.
PLANES = os.environ.get("DDPO_PLANES", "1") == "1"
# The TRAINING forward writes its GroupNorm / LayerNorm results as planes too (they are consumed only by the layer's GEMM and by
# its weight gradient, ddpo_gemm_conv_wgrad_bf16x3_planes): plane-fed forward GEMMs and no activation split in the wgrad loader.
TRAIN_PLANES = os.environ.get("DDPO_TRAIN_PLANES", "1") == "1"
# FF1 + GEGLU of the sampling forward on the 256 x 320 tile where its grid fills the chip (round 5; geglu_tall_pays).  DDPO_GEGLU_TALL=0: the 128 x 128 tile everywhere.
GEGLU_TALL = os.environ.get("DDPO_GEGLU_TALL", "1") == "1"
# FF1 + GEGLU as an f16mx layer where the model registers it as one (pack_weights_geglu(mx=True)): its 107 GFLOP launches are the one compute-bound
# three-pass family of the step, and f16mx spends two matrix passes per product instead of three.  DDPO_FF1_MX=0: the bf16x3 route (the A/B).
FF1_MX = os.environ.get("DDPO_FF1_MX", "1") == "1"
# GEMM output stages that emit planes for a following GEMM (GEGLU -> FF2, block output -> down / up-sampler convolution)
PLANES_OUT = os.environ.get("DDPO_PLANES_OUT", "1") == "1"
PLANES_ALL = os.environ.get("DDPO_PLANES_ALL", "0") == "1"      # plane-feed every eligible layer, also where it is measured slower
# Forward weight planes in the k-blocked layout (ceil(K / 32), N, 32) instead of row-major (N, Kp): every LDS-DMA piece / 16-column
# group of a k-tile is 1 KiB of consecutive memory (ddpo_gemm_desc.w_layout = 1; same values, same arithmetic: bit-identical results)
W_KBLOCKED = os.environ.get("DDPO_W_KBLOCKED", "1") == "1"
# The ACTIVATION planes can be stored the same way — (C / 32, rows, 32) when C % 32 == 0 (plane row stride 0 in the C ABI), written by
# the plane-emitting producers (GroupNorm / LayerNorm / GEMM output stages / split_planes), read by the plane-fed GEMMs and wgrads;
# bit-identical (tests/test_gpu_planes.py runs both storages) — but it is OFF: interleaved A/B on one box, sampling 3.522 / 3.543
# (row-major) vs 3.555 / 3.532 (k-blocked) images/s, training 48.7 / 49.1 vs 48.9 / 48.7 (profiles/r03_ab_akblk_bench.log): the
# activation operand was just written by the previous kernel and is served from L2 / Infinity Cache either way, while the producers'
# stores get ten 64-byte segments per row instead of one 640-byte run.  The weight operand, streamed from HBM by every launch, is
# where the layout pays (+3.0 %).
A_KBLOCKED = os.environ.get("DDPO_A_KBLOCKED", "0") == "1"
# Data gradients as FORWARD contractions (round 4).  dX of y = conv(x, W) is conv(dY, W') with W'[ky, kx, co, ci] = W[k-1-ky, k-1-kx, ci, co]
# (stride 2: over the zero-inserted dY), dX of y = x W is dY W^T: pack_weights(bwd=True) registers W' / W^T as one more set of FORWARD weight
# planes (k-blocked bf16 hi / lo), and conv2d_dgrad / linear_dgrad run the plane-fed / tall-tile bf16x3 forward kernels on them with dY split
# into planes on the way in — instead of the fp32-fed kernel's `w_dgrad` addressing of row-major (K, N) planes, which had none of: LDS-DMA
# operands, k-blocked weight stream, 256x320 tiles.  (f16mx is NOT used for gradients: _pack_dgrad_planes.)
# DDPO_DGRAD_FWD=0 restores the round-3 path (bit-different, same bf16x3 arithmetic class).
DGRAD_FWD = os.environ.get("DDPO_DGRAD_FWD", "1") == "1"


class Planes:
    """An activation (rows, C) stored as bf16 hi / lo planes (two int16 buffers): x ~= hi + lo.  Storage is row-major (rows, C), or —
    when A_KBLOCKED and C % 32 == 0 — k-blocked (C / 32, rows, 32); `ld` is the plane row stride handed to the C ABI (0 = k-blocked)."""
    __slots__ = ("hi", "lo", "rows", "C", "kblocked", "fmt")

    def __init__(self, rows, C, device, fmt=0):
        self.rows, self.C = int(rows), int(C)
        # fmt 0: bf16 hi / lo; 1: f16mx (hi = the f16 plane, lo = the interleaved e5m2 chunks; same geometry, same byte counts)
        self.fmt = int(fmt or 0)
        if self.fmt == 1 and C % 32:
            raise DdpoHipError("f16mx planes need whole 32-channel blocks")
        self.kblocked = bool(A_KBLOCKED and C % 32 == 0)
        shp = (C // 32, rows, 32) if self.kblocked else (rows, C)
        self.hi = torch.empty(shp, dtype=torch.int16, device=device)
        self.lo = torch.empty(shp, dtype=torch.int16, device=device)

    @property
    def ld(self):
        return 0 if self.kblocked else self.C

    @property
    def device(self):
        return self.hi.device

    @property
    def shape(self):
        return torch.Size((self.rows, self.C))

    def data_ptr(self):
        return self.hi.data_ptr()

    def plane(self, which):
        """The hi / lo plane as a logical (rows, C) int16 tensor (tests / debugging: un-blocks the k-blocked storage)."""
        t = self.hi if which == "hi" else self.lo
        return t.permute(1, 0, 2).reshape(self.rows, self.C) if self.kblocked else t

    def float(self):
        """hi + lo as fp32 (rows, C) (tests / debugging).  f16mx planes: h + l8 / 2^11 (the exact value up to the e5m2 rounding of l)."""
        if self.fmt == 1:
            b = self.plane("lo").contiguous().view(torch.float8_e5m2).view(self.rows, self.C // 32, 2, 2, 16)
            return self.plane("hi").contiguous().view(torch.float16).float() + b[:, :, :, 1].reshape(self.rows, self.C).float() / 2048.0
        f = lambda t: (t.to(torch.int32) << 16).view(torch.float32)
        return f(self.plane("hi")) + f(self.plane("lo"))


def planes_ok(w, cin, rows):
    """True when a GEMM / conv with weight tensor `w`, `cin` reduction channels per tap and `rows` source rows (B*H*W pixels
    of a convolution's input, M of a dense layer) can take a plane-fed activation: bf16x3 datapath, weight planes registered
    (pack_weights), 32-channel k-tiles that never straddle a tap, and 31-bit byte offsets (the conditions of the
    buffer-addressed kernel, buf_path_ok() in csrc/gemm_bf16.hip — the VAE's 512x512 levels at batch 8 exceed them)."""
    return bool(PLANES and _planes_dp() and cin % 32 == 0) and _planes_fit(w, cin, rows)


def _planes_fit(w, cin, rows):
    """What planes_ok and planes_out_ok share: weight planes registered, activation and weight planes within the buffer-addressed kernels' offsets."""
    ent = PACKED.get(w.data_ptr())
    return ent is not None and _fits_buf(rows * cin * 4, ent["N"] * ent["fwd"][2] * 2)


def _buf_room(unit_bytes=1):
    """How many units of `unit_bytes` an operand of the buffer-addressed kernels can hold: their byte offsets are 31-bit (buf_path_ok() in
    csrc/gemm_bf16.hip)."""
    return (0x7FFFFFFF - 1) // unit_bytes


def _fits_buf(*nbytes):
    """True when operands of these byte counts all fit the buffer-addressed kernels.  Every count asked about is a multiple of 4 (fp32 elements,
    16-bit planes of a multiple of 8 columns), so `< 0x7FFFFFFF` here and `< 1 << 31` are the same statement."""
    return all(n <= _buf_room() for n in nbytes)


def _tall_tiles_fill(rows, N):
    """The tall-tile fill rule of the C++ dispatch (dispatch_bf16): the grid of 256 x 320 tiles over `rows` x N has at least 200 tiles and fills its
    rounds of 256 CUs within 8 % of the 128 x 320 grid's efficiency."""
    ntall, nwide = -(-rows // 256) * (N // 320), -(-rows // 128) * (N // 320)
    eff = lambda n: n / (-(-n // 256) * 256)
    return ntall >= 200 and eff(ntall) * 1.08 >= eff(nwide)


def planes_pay(w, cin, rows):
    """0 / 1 / 2 (falsy = feed fp32; 1 = bf16 hi / lo planes; 2 = f16mx planes — hand the value to the producer: groupnorm / layernorm
    `planes=`, gemm_conv / linear_geglu `planes_out` / `planes_fmt`).  Non-zero when planes_ok() AND the plane-fed kernel is the faster one for this layer in the model (tools/unet_gemm_breakdown.py --ab,
    profiles/r02_gemm_breakdown_ab.md): long reductions (every 3x3 convolution, FF2) gain 5-24 %, the 64x64-level linears 0-8 %;
    the short reductions of the 32x32 / 16x16 levels (K <= 1280 with < 32768 rows: q / k / v / proj_in, FF1) lose 2-8 % to the
    LDS-DMA loop's fill latency, so their norms keep writing fp32.  DDPO_PLANES_ALL=1 ignores the rule (tests of the kernels)."""
    if not planes_ok(w, cin, rows):
        return 0
    if mx_layer(w):                      # f16mx layer: always plane-fed, in the f16mx format (the routing must not depend on the batch)
        return 2
    if PLANES_ALL:
        return 1
    ent = PACKED[w.data_ptr()]
    if not _x3():
        # single-pass bf16 (round 6): the fp32-fed single-pass kernels already run the long reductions at 750-980 TF; the plane-fed form wins only
        # where the 256 x 320 tile with the four-stage ring (APL = 8) takes the layer — 1.15-1.27x on the 64x64-level convolutions of SD-1.5,
        # 1.12x on SD-2.1's 960-column projection — and loses 5-10 % on the 128-row tiles (profiles/r06_breakdown_bf16_planes.log).  Same rule as
        # the C++ dispatch (_tall_tiles_fill), and K >= 1280.
        # KNOWN DIFFERENCE from the dispatcher (advisor finding, left as it is here): the rule is asked about SOURCE rows, the dispatcher uses
        # output rows — an up-sampling convolution has 4x as many, a stride-2 one a quarter.
        N, K = ent["N"], ent["K"]
        return 1 if (N % 320 == 0 and K >= 1280 and _tall_tiles_fill(rows, N)) else 0
    return 1 if (ent["K"] >= 2560 or rows >= 32768) else 0


def planes_out_ok(w, cin, rows, N):
    """True when the GEMM / conv with weight `w` (reduction channels per tap `cin`, `rows` source rows, N output columns) runs on a
    buffer-addressed bf16x3 kernel, i.e. can emit its result as planes (ddpo_gemm_desc.out_hi): the conditions of planes_ok()
    except that the ACTIVATION may be fp32 (then only K % 32 and the 31-bit offsets matter), plus N % 4 == 0."""
    return bool(PLANES and PLANES_OUT and _planes_dp() and cin % 32 == 0 and N % 4 == 0) and _planes_fit(w, cin, rows)


def split_planes(x, fmt=0):
    """fp32 (rows, C) -> Planes of format `fmt` (0 bf16 hi / lo, 1 f16mx): what a plane-emitting producer writes.  x may be a row-strided
    2-D view (a column slice of a wider row-major buffer)."""
    rows, C = x.shape
    pl = Planes(rows, C, x.device, fmt=fmt)
    ldx = int(x.stride(0)) if rows > 1 else C
    if pl.fmt == 1:
        _check(load().ddpo_split_planes_f16mx(_p_rows(x), ldx, _p(pl.hi), _p(pl.lo), pl.ld, rows, C, _stream()), "ddpo_split_planes_f16mx")
    else:
        _check(load().ddpo_split_planes_bf16(_p_rows(x), ldx, _p(pl.hi), _p(pl.lo), pl.ld, rows, C, _stream()), "ddpo_split_planes_bf16")
    return pl


# ---- f16mx forward operator (ABI v7): a*b ~= a_h*b_h (f16 MFMA) + a_h8*b_l8 + a_l8*b_h8 (one block-scaled 8-bit MFMA) on the plane-fed
# kernels.  Validated operator by operator (tests/test_gpu_f16mx.py, tools/native/kernel_probe mx) and measured — 1.2-1.4x on the
# long-reduction convolutions of the 32x32 / 16x16 levels, ~1.0x at the 64x64 level, whose tiles are bound by the operand stream
# (profiles/r03_probe_mx.log).  The raw wrappers below are what the tests and tools call; the MODELS reach the kernel through
# gemm_conv / linear_geglu under the `f16mx` datapath (DATAPATHS above; the shipped default since round 4).
def pack_weights_f16mx(w):
    """fp32 weight (..., N) viewed as (K, N) -> dict(w16, w8, scale, K, N): the f16mx weight planes of ddpo_pack_weights_f16mx."""
    N = w.shape[-1]
    K = w.numel() // N
    Kb = (K + 31) // 32
    ent = dict(K=K, N=N, w16=torch.zeros(Kb, N, 32, dtype=torch.int16, device=w.device), w8=torch.zeros(Kb, N, 64, dtype=torch.uint8, device=w.device),
               scale=torch.zeros(N, dtype=torch.uint8, device=w.device))
    _check(load().ddpo_pack_weights_f16mx(_p(w), K, N, _p(ent["w16"]), _p(ent["w8"]), _p(ent["scale"]), _stream()), "ddpo_pack_weights_f16mx")
    return ent


def split_planes_f16mx(x):
    """fp32 (rows, C), C % 32 == 0 -> (p16, p8): the f16 plane (rows, C) int16 and the 8-bit plane (rows, C / 32, 64) uint8
    per 32-channel block: chunks of 16 bytes [h8 c0-15 | l8 c0-15 | h8 c16-31 | l8 c16-31], h8 = e5m2(h), l8 = e5m2(l * 2^11) (row-major storage)."""
    rows, C = x.shape
    p16 = torch.empty(rows, C, dtype=torch.int16, device=x.device)
    p8 = torch.empty(rows, C // 32, 64, dtype=torch.uint8, device=x.device)
    _check(load().ddpo_split_planes_f16mx(_p(x), C, _p(p16), _p(p8), C, rows, C, _stream()), "ddpo_split_planes_f16mx")
    return p16, p8


def gemm_conv_f16mx(planes, wp, *, M, bias=None, residual=None, conv=None, out=None, planes_out=False):
    """Plane-fed f16mx GEMM / convolution: planes = split_planes_f16mx(x), wp = pack_weights_f16mx(w); conv as in gemm_conv.
    planes_out: also return the result as f16mx planes (p16, p8) written by the output stage."""
    p16, p8 = planes
    N, K = wp["N"], wp["K"]
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=p16.device)
    opl = None
    if planes_out:
        opl = (torch.empty(M, N, dtype=torch.int16, device=p16.device), torch.empty(M, N // 32, 64, dtype=torch.uint8, device=p16.device))
    d = _gemm_desc(M, N, K, conv=conv, out=out, bias=bias, residual=residual, out_planes=opl and (opl[0], opl[1], N, 1))
    _launch_fwd(d, (p16, p8, int(p16.shape[1])), wp, cross=True, ws_device=p16.device)       # (the raw operator: cross terms whatever MX_CROSS says)
    return (out, opl) if planes_out else out


# When set to a list, every ddpo_gemm_conv_fwd launch appends (start_event, end_event, algorithmic_flops);
# used by bench.py for the live roofline measurement of the dominant kernel.
PROFILE = None


TILE_CLASSES = ("tall_256x320", "wide_128x320", "t128x128", "t128x64", "generic_loader", "splitk_reduce", "f16mx", "reserved")


def gemm_tile_launch_counts():
    """Cumulative host-side launch counts of the bf16-MFMA GEMM / conv template per tile class (ddpo_gemm_tile_launch_counts)."""
    buf = (ctypes.c_ulonglong * 8)()
    _check(load().ddpo_gemm_tile_launch_counts(ctypes.cast(buf, c_void_p), 8), "ddpo_gemm_tile_launch_counts")
    return dict(zip(TILE_CLASSES, (int(v) for v in buf)))


class DdpoHipError(RuntimeError):
    pass


def load():
    """Load libddpo_hip.so (idempotent).  Raises if it has not been built — no CPU fallback exists."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DdpoHipError(f"{LIB_PATH} not found: build it with `python __graft_entry__.py` or "
                           f"`make -C ddpo_amd/csrc` (the DDPO engine has no non-HIP path)")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.ddpo_sizeof_gemm_desc() != ctypes.sizeof(GemmDesc) or lib.ddpo_sizeof_ddim_consts() != ctypes.sizeof(DdimConsts):
        raise DdpoHipError("struct layout mismatch between include/ddpo_hip.h and ddpo_amd/lib.py")
    if lib.ddpo_abi_version() != ABI_VERSION:
        raise DdpoHipError(f"libddpo_hip.so has ABI version {lib.ddpo_abi_version()}, lib.py expects {ABI_VERSION}: rebuild with `python __graft_entry__.py`")
    _lib = lib
    return lib


def _check(rc, name):
    if rc != 0:
        raise DdpoHipError(f"{name} failed with status {rc} ({'invalid argument' if rc == -1 else 'launch failure'})")


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    """Device pointer of a CONTIGUOUS tensor (kernels index with explicit leading dimensions, never torch strides)."""
    if t is None:
        return c_void_p(0)
    if not t.is_contiguous():
        raise DdpoHipError(f"non-contiguous tensor of shape {tuple(t.shape)} / strides {t.stride()} passed to a HIP kernel")
    return c_void_p(t.data_ptr())


def _p_rows(t):
    """Pointer of a 2-D row-strided view (column slice of a row-major matrix); the caller passes the row stride."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise DdpoHipError(f"expected a row-major 2-D view, got strides {t.stride()}")
    return c_void_p(t.data_ptr())


def _pr(t, ld):
    """Pointer of an operand passed with an explicit row stride `ld` (a column slice of a wider row-major matrix) or, ld falsy, contiguous."""
    return _p_rows(t) if ld else _p(t)


def _f32(t, name="tensor"):
    if t.dtype != torch.float32 or not t.is_cuda:
        raise DdpoHipError(f"{name} must be a float32 CUDA tensor, got {t.dtype} on {t.device}")
    return t


def bind_side(sigs, version_symbol, expected, what, module):
    """The loader of the side bindings (lib_optim.py, lib_pref.py, lib_dpo.py, lib_cfg_rescale.py), each versioned on its
    own: bind the table `sigs` on libddpo_hip.so and hold `version_symbol()` to `expected`.  `what` / `module` name the binding in the
    version error.  A library without one of the entries is an error: there is no other path."""
    load()                                      # "not built" is reported once, there
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in sigs.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise DdpoHipError(f"libddpo_hip.so does not export {name}: rebuild with `python __graft_entry__.py`") from None
        fn.restype = res
        fn.argtypes = args
    have = getattr(lib, version_symbol)()
    if have != expected:
        raise DdpoHipError(f"libddpo_hip.so has {what} ABI version {have}, {module} expects {expected}")
    return lib


def check_rows(B, chw, train_cfg, **rows):
    """Shared check of the loss wrappers of the side bindings: every tensor of `rows`, in the order given, is there, float32 on the device
    and of B x chw elements.  A name ending in `_u` is the unconditional half: looked at under train_cfg only."""
    for name, t in rows.items():
        if name.endswith("_u") and not train_cfg:
            continue
        if t is None:
            raise DdpoHipError(f"{name} is required" + (" under train_cfg" if name.endswith("_u") else ""))
        _f32(t, name)
        if t.numel() != B * chw:
            raise DdpoHipError(f"{name} has {t.numel()} elements, expected {B} x {chw}")


# ------------------------------------------------------------------------------------------------ PRNG
def threefry_bits_host(key, n):
    """uint32 words of jax `random_bits(key, n)` computed on the host (key bookkeeping)."""
    import numpy as np
    out = np.empty(int(n), dtype=np.uint32)
    _check(load().ddpo_threefry_bits_host(int(key[0]), int(key[1]), int(n), out.ctypes.data_as(c_void_p)), "ddpo_threefry_bits_host")
    return out


def threefry_normal(key, shape, device="cuda", out=None, return_bits=False):
    """jax.random.normal(key, shape, float32) on the GPU.  key: 2 uint32 words."""
    n = 1
    for s in shape:
        n *= int(s)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=device)
    bits = torch.empty(n, dtype=torch.int32, device=out.device) if return_bits else None
    _check(load().ddpo_threefry_normal(int(key[0]), int(key[1]), _p(out), _p(bits), n, _stream()), "ddpo_threefry_normal")
    return (out, bits) if return_bits else out


# ------------------------------------------------------------------------------------------------ DDIM / PPO
def make_ddim_consts(alphas_cumprod_dev, step_ratio, final_alpha_cumprod, eta, prediction_type):
    c = DdimConsts()
    c.alphas_cumprod = alphas_cumprod_dev.data_ptr()
    c.num_train_timesteps = alphas_cumprod_dev.numel()
    c.step_ratio = int(step_ratio)
    c.final_alpha_cumprod = float(final_alpha_cumprod)
    c.eta = float(eta)
    c.pred_type = PRED_TYPES[prediction_type]
    c._keepalive = alphas_cumprod_dev
    return c


def ddim_step_fwd(eps_u, eps_c, x, z, ts, guidance_scale, consts, x_next=None, logp=None):
    B = x.shape[0]
    chw = x.numel() // B
    if x_next is None:
        x_next = torch.empty_like(x)
    if logp is None:
        logp = torch.empty(B, dtype=torch.float32, device=x.device)
    _check(load().ddpo_ddim_step_fwd(_p(eps_u), _p(eps_c), _p(x), _p(z), _p(ts), float(guidance_scale), byref(consts),
                                     _p(x_next), _p(logp), B, chw, _stream()), "ddpo_ddim_step_fwd")
    return x_next, logp


def ddim_logprob_ppo_fwd_bwd(eps_c, eps_u, x, x_next, ts, old_logp, advantages, guidance_scale, clip_range, train_cfg, consts,
                             group=None, out=None):
    """`group` (default: the whole batch) = rows per PPO micro-batch when several micro-batches are scored in one call:
    rows [j*group, (j+1)*group) are micro-batch j, each with its own mean loss; info comes back as (B // group, 3).
    out: optional pre-allocated (d_c, d_u, per_sample, info) of a previous call with the same geometry (the launch then allocates nothing)."""
    B = x.shape[0]
    chw = x.numel() // B
    if out is not None:
        d_c, d_u, per_sample, info = out
    else:
        d_c = torch.empty_like(eps_c)
        d_u = torch.empty_like(eps_c) if train_cfg else None
        per_sample = torch.empty(B, 4, dtype=torch.float32, device=x.device)
        info = None
    if group is not None and (group <= 0 or B % group):
        raise ValueError(f"batch of {B} rows is not a whole number of micro-batches of {group}")
    if info is None:
        info = torch.empty(*((3,) if group is None else (B // group, 3)), dtype=torch.float32, device=x.device)
    _check(load().ddpo_ddim_logprob_ppo_fwd_bwd(_p(eps_c), _p(eps_u), _p(x), _p(x_next), _p(ts), _p(old_logp), _p(advantages),
                                                float(guidance_scale), float(clip_range), int(bool(train_cfg)), byref(consts),
                                                _p(d_c), _p(d_u), _p(per_sample), _p(info), B, B if group is None else int(group), chw, _stream()),
           "ddpo_ddim_logprob_ppo_fwd_bwd")
    return d_c, d_u, per_sample, info


# ------------------------------------------------------------------------------------------------ RWR
def rwr_noisy_latents(moments, e1, noise, ts, alphas_cumprod_dev, scale=0.18215):
    """moments (B,h,w,2C) NHWC, e1 (B,h,w,C) NHWC, noise (B,C,h,w) -> (latents, noisy_latents), both (B,C,h,w)."""
    B, h, w, C2 = moments.shape
    C = C2 // 2
    lat = torch.empty(B, C, h, w, dtype=torch.float32, device=moments.device)
    noisy = torch.empty_like(lat)
    _check(load().ddpo_rwr_noisy_latents(_p(moments), _p(e1), _p(noise), _p(ts), _p(alphas_cumprod_dev), alphas_cumprod_dev.numel(),
                                         float(scale), _p(lat), _p(noisy), B, C, h * w, _stream()), "ddpo_rwr_noisy_latents")
    return lat, noisy


def rwr_noisy_latents_target(moments, e1, noise, ts, alphas_cumprod_dev, prediction_type, scale=0.18215):
    """rwr_noisy_latents plus the regression target of `prediction_type` -> (latents, noisy_latents, target).  The entry is declared in
    include/ddpo_cfg_rescale.h and bound by lib_cfg_rescale.py, which is imported only here: epsilon models never come this way."""
    from . import lib_cfg_rescale as LR
    return LR.rwr_noisy_latents_target(moments, e1, noise, ts, alphas_cumprod_dev, prediction_type, scale)


def rwr_mse_fwd_bwd(eps_c, eps_u, noise, weights, guidance_scale, train_cfg):
    """Weighted denoising MSE + its closed-form gradient.  Returns (d_eps_c, d_eps_u | None, per_sample (B,2), loss (1,))."""
    B = eps_c.shape[0]
    chw = eps_c.numel() // B
    d_c = torch.empty_like(eps_c)
    d_u = torch.empty_like(eps_c) if train_cfg else None
    per_sample = torch.empty(B, 2, dtype=torch.float32, device=eps_c.device)
    loss = torch.empty(1, dtype=torch.float32, device=eps_c.device)
    _check(load().ddpo_rwr_mse_fwd_bwd(_p(eps_c), _p(eps_u), _p(noise), _p(weights), float(guidance_scale), int(bool(train_cfg)),
                                       _p(d_c), _p(d_u), _p(per_sample), _p(loss), B, chw, _stream()), "ddpo_rwr_mse_fwd_bwd")
    return d_c, d_u, per_sample, loss


# ------------------------------------------------------------------------------------------------ optimizer
def grad_sqnorm(g, out_sq=None):
    if out_sq is None:
        out_sq = torch.zeros(1, dtype=torch.float64, device=g.device)
    _check(load().ddpo_grad_sqnorm(_p(g), g.numel(), _p(out_sq), 1, _stream()), "ddpo_grad_sqnorm")
    return out_sq


def adamw_bf16mu_step(p, g, mu, nu, sqnorm, inv_n_acc, lr, b1, b2, eps, weight_decay, max_grad_norm, step_t,
                      mu_decay_in_bf16=True, zero_grad=True):
    assert mu.dtype == torch.bfloat16 and nu.dtype == torch.float32 and sqnorm.dtype == torch.float64
    _check(load().ddpo_adamw_bf16mu_step(_p(p), _p(g), _p(mu), _p(nu), p.numel(), _p(sqnorm), float(inv_n_acc), float(lr),
                                         float(b1), float(b2), float(eps), float(weight_decay), float(max_grad_norm),
                                         int(step_t), int(mu_decay_in_bf16), int(zero_grad), _stream()), "ddpo_adamw_bf16mu_step")


# ------------------------------------------------------------------------------------------------ U-Net blocks
_ws_cache = {}


def _scratch(nbytes, device, tag):
    key = (tag, str(device), torch.cuda.current_stream().cuda_stream)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


def _conv_geom(B, H, W, Cin, ksize, stride, pad, upsample):
    """The conv dict of gemm_conv / gemm_wgrad (ddpo_gemm_desc's geometry fields); pad None = ksize // 2.  upsample: 0 / 1 = nearest 2x gather,
    2 = zero insertion (the transposed view of a stride-2 convolution, conv2d_dgrad)."""
    if pad is None:
        pad = ksize // 2
    VH, VW = (2 * H, 2 * W) if upsample else (H, W)
    OH = (VH + 2 * pad - ksize) // stride + 1
    OW = (VW + 2 * pad - ksize) // stride + 1
    return dict(ksize=ksize, stride=stride, pad=pad, upsample=int(upsample), B=B, H=H, W=W, Cin=Cin, OH=OH, OW=OW)


def _gemm_desc(M, N, K, *, conv=None, src=None, ld_src=0, out=None, ld_out=None, bias=None, residual=None, ld_res=None, res_rows=0, alpha=1.0,
               out_planes=None, aux_out=None, **fields):
    """A ddpo_gemm_desc: what is not given stays zero / NULL.  conv: the geometry fields by name (_conv_geom); ld_out / ld_res default to N;
    out_planes = (hi, lo, ld_planes, planes_fmt) of a plane-emitting output stage; **fields: any other field of the structure, as its raw value."""
    d = GemmDesc()
    d.M, d.N, d.K = int(M), int(N), int(K)
    d.alpha = float(alpha)
    for k, v in (conv or {}).items():
        setattr(d, k, int(v))
    if src is not None:
        d.src = src.data_ptr()
    d.ld_src = int(ld_src)
    if out is not None:
        d.out = out.data_ptr(); d.ld_out = int(ld_out if ld_out is not None else N)
    d.bias = bias.data_ptr() if bias is not None else None
    if residual is not None:
        d.residual = residual.data_ptr(); d.ld_res = int(ld_res if ld_res is not None else N)
    d.res_rows = int(res_rows)
    if out_planes is not None:
        hi, lo, d.ld_planes, d.planes_fmt = out_planes
        d.out_hi, d.out_lo = hi.data_ptr(), lo.data_ptr()
    d.aux_out = aux_out.data_ptr() if aux_out is not None else None
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def _launch_fwd(d, act, weights, *, w_layout=0, cross=None, ws_device=None, tag=""):
    """The one forward launch: picks the entry point from the operands.
    act: None (fp32-fed: the activation is d.src), `Planes`, or (hi, lo, ld) plane tensors.
    weights: None -> exact fp32 (ddpo_gemm_conv_fwd reads d.w); (hi, lo, ldw, npass) bf16 planes stored as `w_layout`; dict(w16, w8, scale) f16mx.
    A single bf16 pass (npass 1) reads the hi planes only: both lo pointers NULL on the plane-fed entry.  f16mx without its cross terms (`cross`,
    default MX_CROSS): both 8-bit planes NULL.  ws_device: fetch the split-K scratch there and pass it; None: no workspace (no split-K).
    tag: appended to the symbol in the error message."""
    lib = load()
    a_hi, a_lo, a_ld = (act.hi, act.lo, act.ld) if isinstance(act, Planes) else (act or (None, None, 0))
    ws = None if ws_device is None else _scratch(SPLITK_WS_BYTES, ws_device, "splitk")
    ws_args = (_p(ws), SPLITK_WS_BYTES if ws is not None else 0, _stream())
    if weights is None:
        name, rc = "ddpo_gemm_conv_fwd", lib.ddpo_gemm_conv_fwd(byref(d), _stream())
    elif isinstance(weights, dict):
        cross = MX_CROSS if cross is None else cross
        d.w_layout = 1
        d.w_scale = weights["scale"].data_ptr()
        name, rc = "ddpo_gemm_conv_fwd_f16mx_planes", lib.ddpo_gemm_conv_fwd_f16mx_planes(
            byref(d), _p(a_hi), _p(a_lo) if cross else None, a_ld, _p(weights["w16"]), _p(weights["w8"]) if cross else None, *ws_args)
    else:
        hi, lo, ldw, npass = weights
        d.w_layout = w_layout
        if a_hi is None:
            name, rc = "ddpo_gemm_conv_fwd_bf16", lib.ddpo_gemm_conv_fwd_bf16(byref(d), _p(hi), _p(lo), ldw, npass, *ws_args)
        else:
            one = npass == 1
            name, rc = "ddpo_gemm_conv_fwd_bf16_planes", lib.ddpo_gemm_conv_fwd_bf16_planes(
                byref(d), _p(a_hi), None if one else _p(a_lo), a_ld, _p(hi), None if one else _p(lo), ldw, *ws_args)
    _check(rc, name + tag)


def _family(fp32=False, mx=False):
    """Family tag of a PROFILE entry: "fp32" (exact-fp32 kernel), "f16mx" (the launch ran the f16 + MX-fp8 kernel), else the bf16 datapath's name."""
    return "fp32" if fp32 else ("f16mx" if mx else ("bf16x3" if _x3() else current_datapath()))


@contextlib.contextmanager
def _profiled(flops, io_bytes, family):
    """While PROFILE is a list: brackets the launch(es) inside with two events and appends (start, end, algorithmic flops, family, unique operand bytes)."""
    if PROFILE is None:
        yield
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    yield
    e1.record()
    PROFILE.append((e0, e1, flops, family, io_bytes))


def groupnorm(x, B, HW, gamma, beta, groups, eps, silu, out=None, ld_x=None, ld_out=None, return_stats=False, planes=False):
    """x: (B*HW, C) NHWC rows (row stride ld_x).  Returns (B*HW, C) [and the saved statistics for the backward].
    planes (the value of planes_pay / norm_planes for the consumer; 1 / True = bf16 hi / lo, 2 = f16mx): the result comes back as `Planes`
    for a plane-fed conv / linear."""
    C = gamma.numel()
    if ld_x is None and x.dim() == 2 and x.stride(0) != C:          # a column slice of a wider row-major buffer (skip-concat storage)
        ld_x = x.stride(0)
    if planes:
        pl = Planes(B * HW, C, x.device, fmt=1 if planes == 2 else 0)
        ws = _scratch(load().ddpo_groupnorm_ws_bytes(B, HW, C, groups), x.device, "gn")
        stats = torch.empty(load().ddpo_groupnorm_stats_floats(B, C, groups), dtype=torch.float32, device=x.device)
        _check(load().ddpo_groupnorm_fwd_planes(_pr(x, ld_x), int(ld_x or C), _p(pl.hi), _p(pl.lo), pl.ld, _p(gamma), _p(beta), B, HW, C, groups,
                                                float(eps), int(bool(silu)) | (2 * pl.fmt), _p(ws), _p(stats), _stream()), "ddpo_groupnorm_fwd_planes")
        return (pl, stats) if return_stats else pl
    if out is None:
        out = torch.empty(B * HW, C, dtype=torch.float32, device=x.device)
    ws = _scratch(load().ddpo_groupnorm_ws_bytes(B, HW, C, groups), x.device, "gn")
    stats = torch.empty(load().ddpo_groupnorm_stats_floats(B, C, groups), dtype=torch.float32, device=x.device)
    _check(load().ddpo_groupnorm_fwd(_pr(x, ld_x), int(ld_x or C), _p(out), int(ld_out or C), _p(gamma), _p(beta), B, HW, C, groups,
                                     float(eps), int(bool(silu)), _p(ws), _p(stats), _stream()), "ddpo_groupnorm_fwd")
    return (out, stats) if return_stats else out


def groupnorm_bwd(x, dy, stats, gamma, B, HW, groups, silu, dgamma, dbeta, dx_add=None, ld_x=None, ld_dy=None):
    C = gamma.numel()
    dx = torch.empty(B * HW, C, dtype=torch.float32, device=x.device)
    ws = _scratch(load().ddpo_groupnorm_bwd_ws_bytes(B, HW, C, groups), x.device, "gnb")
    _check(load().ddpo_groupnorm_bwd(_p(x), int(ld_x or C), _p(dy), int(ld_dy or C), _p(stats), _p(gamma), B, HW, C, groups,
                                     int(bool(silu)), _p(dx_add), C, _p(dx), C, _p(dgamma), _p(dbeta), _p(ws), _stream()),
           "ddpo_groupnorm_bwd")
    return dx


def layernorm(x, gamma, beta, eps=1e-5, out=None, planes=False):
    rows, C = x.shape
    if planes:
        pl = Planes(rows, C, x.device, fmt=1 if planes == 2 else 0)
        _check(load().ddpo_layernorm_fwd_planes(_p(x), _p(pl.hi), _p(pl.lo), _p(gamma), _p(beta), rows, C, float(eps), int(pl.kblocked) | (2 * pl.fmt), _stream()),
               "ddpo_layernorm_fwd_planes")
        return pl
    if out is None:
        out = torch.empty_like(x)
    _check(load().ddpo_layernorm_fwd(_p(x), _p(out), _p(gamma), _p(beta), rows, C, float(eps), _stream()), "ddpo_layernorm_fwd")
    return out


def pack_weights(w, bwd=True):
    """Register bf16 hi/lo planes for an fp32 weight tensor w (…, N) viewed as (K, N); re-run after w changes."""
    N = w.shape[-1]
    K = w.numel() // N
    Kp = (K + 7) // 8 * 8
    ent = PACKED.get(w.data_ptr())
    mk = lambda *s: torch.zeros(*s, dtype=torch.int16, device=w.device)
    lay = 1 if (W_KBLOCKED and N % 4 == 0) else 0
    if lay:
        Kp = (K + 31) // 32 * 32             # k-blocked planes: whole 32-wide k blocks (zero padded)
    if ent is None or ent["K"] != K or ent["N"] != N or ent.get("w_layout", 0) != lay:
        ent = dict(K=K, N=N, fwd=(mk(N, Kp), mk(N, Kp), Kp), bwd=None, w_layout=lay)
        PACKED[w.data_ptr()] = ent
    # data-gradient planes: the transposed / tap-flipped weight as a forward operand (DGRAD_FWD) where the buffer-addressed kernels can take it,
    # else the original (K, N) order for the fp32-fed kernel's w_dgrad addressing
    n_dg = w.shape[2] if w.dim() == 4 else K              # output columns of the data gradient: the layer's input channels
    dg_ok = bool(bwd and DGRAD_FWD and _x3() and W_KBLOCKED and w.dim() in (2, 4) and N % 32 == 0 and n_dg % 4 == 0)
    if dg_ok:
        _pack_dgrad_planes(w, ent)
    else:
        ent.pop("dg", None)
    if bwd and ent["bwd"] is None and not dg_ok:
        ent["bwd"] = (mk(K, N), mk(K, N))
    if "geglu" in ent:
        ent["geglu"]["stale"] = True          # re-ordered GEGLU planes (pack_weights_geglu) no longer match w
    if "fold" in ent:
        ent["fold"]["stale"] = True           # folded up-sampler planes (pack_weights_up2x_folded) no longer match w
    fh, fl, _ = ent["fwd"]
    bh, bl = ent["bwd"] if ent["bwd"] is not None else (None, None)
    if _mx() and K % 32 == 0 and K >= MX_MIN_K:            # f16mx forward planes next to the bf16 ones (mx_layer(); the backward uses the bf16 ones)
        if "mx" not in ent:
            ent["mx"] = dict(w16=torch.zeros(K // 32, N, 32, dtype=torch.int16, device=w.device), w8=torch.zeros(K // 32, N, 64, dtype=torch.uint8, device=w.device),
                             scale=torch.zeros(N, dtype=torch.uint8, device=w.device))
        m = ent["mx"]
        _check(load().ddpo_pack_weights_f16mx(_p(w), K, N, _p(m["w16"]), _p(m["w8"]), _p(m["scale"]), _stream()), "ddpo_pack_weights_f16mx")
    else:
        ent.pop("mx", None)              # re-packed under another datapath: f16mx planes of the OLD weights must not survive
    if ent["w_layout"] == 1:
        _check(load().ddpo_pack_weights_bf16_kblocked(_p(w), K, N, _p(fh), _p(fl), _stream()), "ddpo_pack_weights_bf16_kblocked")
        if bh is not None:               # data-gradient planes keep the original (K, N) order: the plain split of w, no transpose
            _check(load().ddpo_split_planes_bf16(_p(w), N, _p(bh), _p(bl), N, K, N, _stream()), "ddpo_split_planes_bf16")
    else:
        _check(load().ddpo_pack_weights_bf16(_p(w), K, N, Kp, _p(fh), _p(fl), _p(bh), _p(bl), _stream()), "ddpo_pack_weights_bf16")
    return ent


# Nearest-2x up-sampler convolutions (FlaxUpsample2D) as four 2x2 convolutions on the source grid (include/ddpo_hip.h: ddpo_conv_up2x_folded_fwd;
# the algebra is fold_up2x_kernel_reference below): 4/9 of the matrix work of the up-sampled 3x3 form.  DDPO_UP2X_FOLD=0 keeps the gather form
# (conv2d(..., upsample=True)), which also stays the fp32 datapath's and the backward's form.
UP2X_FOLD = os.environ.get("DDPO_UP2X_FOLD", "1") == "1"


def fold_up2x_kernel_reference(w):
    """The four phase kernels of a nearest-2x up-sampler's 3x3 HWIO kernel w (3, 3, Cin, Cout) -> (4, 2, 2, Cin, Cout), phase py * 2 + px,
    in w's dtype (float64 in: the exact statement; float32 in: the bits of ddpo_fold_up2x_weights — sums taken ky then kx ascending).

    Output pixel (2y + py, 2x + px) of conv3x3(nearest_upsample_2x(x)) reads virtual rows 2y + py - 1 .. 2y + py + 1, i.e. source rows
    (y - 1, y, y) for py = 0 and (y, y, y + 1) for py = 1: a 2-tap kernel at source offsets {-1, 0} with taps {w[0], w[1] + w[2]} (py = 0) or
    offsets {0, +1} with taps {w[0] + w[1], w[2]} (py = 1); the same in x.  The zero padding of the virtual image (rows -1 and 2H) coincides
    with source rows -1 and H, so borders need no special case."""
    groups = (((0,), (1, 2)), ((0, 1), (2,)))          # [phase][tap] -> 3x3 indices summed into it
    out = w.new_zeros((4, 2, 2) + tuple(w.shape[2:]))
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    acc = None
                    for ky in groups[py][ty]:
                        for kx in groups[px][tx]:
                            acc = w[ky, kx].clone() if acc is None else acc + w[ky, kx]
                    out[py * 2 + px, ty, tx] = acc
    return out


def conv_up2x_folded_reference(x, w):
    """x (B, H, W, Cin), w (3, 3, Cin, Cout) -> (B, 2H, 2W, Cout): the folded form on the host, in x's dtype (documents the kernel's geometry)."""
    B, H, W, _ = x.shape
    wf = fold_up2x_kernel_reference(w)
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))          # source rows / columns -1 and H / W are zeros
    out = x.new_zeros(B, 2 * H, 2 * W, w.shape[3])
    for py in range(2):
        for px in range(2):
            acc = 0
            for ty in range(2):
                for tx in range(2):
                    oy, ox = ty - 1 + py, tx - 1 + px            # source offset of this tap
                    acc = acc + xp[:, 1 + oy:1 + oy + H, 1 + ox:1 + ox + W] @ wf[py * 2 + px, ty, tx]
            out[:, py::2, px::2] = acc
    return out


def pack_weights_up2x_folded(w):
    """Register the folded phase planes of an up-sampler kernel w (3, 3, Cin, Cout) next to its pack_weights() planes (call after it, and
    after every change of w — pack_weights marks the folded planes stale, and a stale layer runs the gather form): PACKED[w]["fold"] = dict(K = 4 Cin, N, hi, lo (4, K / 32, N, 32) and, on the f16mx datapath for K >= MX_MIN_K,
    mx = dict(w16, w8, scale)).  Derived data (never saved).  Cin % 32 == 0 and N % 4 == 0 are needed; other layers keep the gather form."""
    ent = PACKED.get(w.data_ptr())
    if ent is None:
        raise DdpoHipError("pack_weights_up2x_folded: pack_weights(w) first")
    C, N = int(w.shape[2]), int(w.shape[3])
    if not (UP2X_FOLD and w.dim() == 4 and w.shape[0] == 3 and w.shape[1] == 3 and C % 32 == 0 and N % 4 == 0 and W_KBLOCKED):
        ent.pop("fold", None)
        return None
    K, Kb = 4 * C, 4 * C // 32
    fo = ent.get("fold")
    if fo is None or fo["K"] != K or fo["N"] != N:
        mk = lambda: torch.zeros(4, Kb, N, 32, dtype=torch.int16, device=w.device)
        fo = ent["fold"] = dict(K=K, N=N, hi=mk(), lo=mk())
    wf = torch.empty(4, K, N, dtype=torch.float32, device=w.device)       # the folded fp32 kernels: only live until they are packed
    _check(load().ddpo_fold_up2x_weights(_p(w), C, N, _p(wf), _stream()), "ddpo_fold_up2x_weights")
    mx = _mx() and K >= MX_MIN_K
    if mx and "mx" not in fo:
        fo["mx"] = dict(w16=torch.zeros(4, Kb, N, 32, dtype=torch.int16, device=w.device), w8=torch.zeros(4, Kb, N, 64, dtype=torch.uint8, device=w.device),
                        scale=torch.zeros(4, N, dtype=torch.uint8, device=w.device))
    if not mx:
        fo.pop("mx", None)
    for ph in range(4):
        _check(load().ddpo_pack_weights_bf16_kblocked(_p(wf[ph]), K, N, _p(fo["hi"][ph]), _p(fo["lo"][ph]), _stream()), "ddpo_pack_weights_bf16_kblocked")
        if mx:
            m = fo["mx"]
            _check(load().ddpo_pack_weights_f16mx(_p(wf[ph]), K, N, _p(m["w16"][ph]), _p(m["w8"][ph]), _p(m["scale"][ph]), _stream()), "ddpo_pack_weights_f16mx")
    fo["stale"] = False
    return fo


def up2x_fold_ok(w, cin, rows):
    """True when the up-sampler convolution with kernel `w` (`rows` SOURCE pixels of `cin` channels) runs folded: a bf16 / f16mx datapath,
    folded planes registered (pack_weights_up2x_folded), the buffer-addressed kernels' 31-bit offsets.  False under DDPO_MX_CROSS=0 (that
    experiment's single-pass f16 kernels have no folded form): those layers keep the gather form, like the fp32 datapath."""
    # (not a function of PLANES / BF16_PLANES: those say how activations TRAVEL, and a layer's arithmetic must not depend on that — with them
    # off the producers write fp32 and the layer splits it on the way in)
    if not UP2X_FOLD or current_datapath() == "fp32" or cin % 32 or (_mx() and not MX_CROSS):
        return False
    ent = PACKED.get(w.data_ptr())
    if ent is None or "fold" not in ent:
        return False
    fo = ent["fold"]
    if fo.get("stale", True):                 # pack_weights(w) ran since: the planes are those of the OLD weights
        return False
    if _mx() and fo["K"] >= MX_MIN_K and "mx" not in fo:      # packed under another datapath: no f16mx planes for an f16mx layer
        return False
    return _fits_buf(rows * cin * 4, 4 * fo["N"] * fo["K"] * 2, rows * 4)


def up2x_planes_pay(w, cin, rows):
    """planes_pay() for an up-sampler convolution: a folded layer is always plane-fed, f16mx (2) when its FOLDED reduction 4 * cin reaches
    MX_MIN_K, else bf16 hi / lo (1; the single-pass datapath reads the hi plane); the gather form answers as planes_pay."""
    if not up2x_fold_ok(w, cin, rows):
        return planes_pay(w, cin, rows)
    if not (PLANES and _planes_dp()):          # producers write fp32; the folded layer splits it on the way in
        return 0
    return 2 if (_mx() and "mx" in PACKED[w.data_ptr()]["fold"]) else 1


def conv2d_up2x_folded(x, w, bias, B, H, W, Cin, Cout, out=None, ld_out=None):
    """Nearest-2x up-sampling + 3x3 convolution in the folded form (check up2x_fold_ok first).  x: fp32 (B*H*W, Cin) rows (tensor or
    row-strided view; split into the layer's plane format on the way in — the same bits a plane-emitting producer writes) or Planes of the
    format up2x_planes_pay names.  Returns ((B*2H*2W, Cout), 2H, 2W); `out` / `ld_out` as in gemm_conv."""
    rows = B * H * W
    if not up2x_fold_ok(w, Cin, rows):
        raise DdpoHipError("conv2d_up2x_folded: no folded planes for this layer / datapath (check up2x_fold_ok)")
    fo = PACKED[w.data_ptr()]["fold"]
    if fo["K"] != 4 * Cin or fo["N"] != Cout:
        raise DdpoHipError("conv2d_up2x_folded: geometry does not match the registered kernel")
    mxl = _mx() and "mx" in fo
    if isinstance(x, Planes):
        pl = x
        if pl.fmt != int(mxl) or pl.rows != rows or pl.C != Cin:
            raise DdpoHipError("activation planes of the wrong format / shape for this layer (ask up2x_planes_pay)")
    else:
        if not (x.dim() == 2 and x.shape[0] == rows and x.shape[1] == Cin and x.stride(1) == 1):
            raise DdpoHipError("conv2d_up2x_folded needs its fp32 input as a (rows, channels) tensor or row-strided view")
        pl = split_planes(x, fmt=1 if mxl else 0)
    M = 4 * rows
    if out is None:
        out = torch.empty(M, Cout, dtype=torch.float32, device=pl.device)
    d = _gemm_desc(0, Cout, 0, conv=dict(B=B, H=H, W=W, Cin=Cin), out=out, ld_out=ld_out, bias=bias)      # (M, K and the taps are the kernel's own)
    one = not _x3()
    if mxl:
        m = fo["mx"]
        d.w_scale = m["scale"].data_ptr()
        wh, wl = m["w16"], m["w8"]
    else:
        wh, wl = fo["hi"], (None if one else fo["lo"])
    K = 4 * Cin                              # the FLOPs actually executed: 2 * M * 4 Cin * N
    io_bytes = 4.0 * rows * Cin + (4.0 if _x3() else 2.0) * 4 * K * Cout + 4.0 * M * Cout
    with _profiled(2.0 * M * Cout * K, io_bytes, _family(mx=mxl)):
        ws = _scratch(SPLITK_WS_BYTES, pl.device, "splitk")
        _check(load().ddpo_conv_up2x_folded_fwd(byref(d), _p(pl.hi), None if (one and not mxl) else _p(pl.lo), pl.ld, _p(wh), None if wl is None else _p(wl),
                                                int(mxl), _p(ws), SPLITK_WS_BYTES, _stream()), "ddpo_conv_up2x_folded_fwd")
    return out, 2 * H, 2 * W


def _pack_dgrad_planes(w, ent):
    """ent["dg"]: forward-style planes of the data-gradient weight of `w` — conv (kh, kw, ci, co): W'[ky, kx, co, ci] = W[kh-1-ky, kw-1-kx, ci, co],
    i.e. K' = kh * kw * co reduction rows, N' = ci output columns; dense (K, N): W^T, K' = N, N' = K."""
    taps = w.shape[0] * w.shape[1] if w.dim() == 4 else 1
    Nd, cout = (w.shape[2], w.shape[3]) if w.dim() == 4 else (w.shape[0], w.shape[1])
    Kd = taps * cout
    Kp = (Kd + 31) // 32 * 32
    dg = ent.get("dg")
    if dg is None or dg["K"] != Kd or dg["N"] != Nd:
        mk = lambda *sh: torch.zeros(*sh, dtype=torch.int16, device=w.device)
        dg = ent["dg"] = dict(K=Kd, N=Nd, hi=mk(Nd, Kp), lo=mk(Nd, Kp))
    # packed straight from w (ABI v13): no flipped / transposed fp32 copy after every optimizer update
    _check(load().ddpo_pack_weights_bf16_kblocked_dgrad(_p(w), taps, Nd, cout, _p(dg["hi"]), _p(dg["lo"]), _stream()), "ddpo_pack_weights_bf16_kblocked_dgrad")
    # NO f16mx planes for data gradients, on any datapath: the f16mx ACTIVATION planes carry no scale (f16 + e5m2 at the value's own exponent),
    # which is right for O(1) activations and wrong for dY — PPO / RWR gradients sit at 1e-7 .. 1e-3, i.e. in f16's subnormal range: measured
    # on hardware (round 4, full-size SD-1.5 / SD-2.1 train step) ||g - g_ref|| / ||g_ref|| went from 7e-5 to 1e-2 .. 4e-2 with f16mx data
    # gradients.  The data gradients therefore run bf16x3 (bf16 has fp32's range) on the plane-fed forward kernels.
    return dg


def _dgrad_fwd(dy, dg, *, M, conv=None, residual=None, ld_res=None, out=None):
    """dX = the forward contraction of dY with the registered data-gradient planes `dg` (see DGRAD_FWD).  dy: fp32 (rows, K' per tap) or Planes.
    Long reductions (K' >= 2560: every 3x3 convolution, FF1) run plane-fed — dY split into bf16 hi / lo planes on the way in (bf16x3 on every
    datapath: gradients need fp32's exponent range) —; short ones stay fp32-fed (the plane-fed loop's fill latency, planes_pay) on the k-blocked weight stream."""
    Kd, Nd = dg["K"], dg["N"]
    cin = conv["Cin"] if conv else Kd
    rows = conv["B"] * conv["H"] * conv["W"] if conv else M
    if conv is None and not _fits_buf(rows * cin * 4) and not isinstance(dy, Planes):
        # a dense dY of >= 2 GiB (FF1's (M, 8C) gradient at training batch sizes) would leave the buffer-addressed kernels: run it in row chunks
        # (the chunk is rounded DOWN to whole 256-row tiles so that it stays below the limit and can never re-enter this branch)
        step = _buf_room(cin * 4) // 256 * 256
        if step <= 0:
            raise DdpoHipError(f"_dgrad_fwd: one 256-row chunk of a {cin}-wide dY does not fit the buffer-addressed kernels")
        if out is None:
            out = torch.empty(M, Nd, dtype=torch.float32, device=dy.device)
        for r0 in range(0, rows, step):
            r1 = min(rows, r0 + step)
            assert _fits_buf((r1 - r0) * cin * 4)
            _dgrad_fwd(dy[r0:r1], dg, M=r1 - r0, residual=None if residual is None else residual[r0:r1], ld_res=ld_res, out=out[r0:r1])
        return out
    buf_ok = cin % 32 == 0 and _fits_buf(rows * cin * 4, Nd * ((Kd + 31) // 32 * 32) * 2)
    pl = dy if isinstance(dy, Planes) else None
    if pl is not None and (pl.fmt != 0 or not buf_ok):
        dy, pl = pl.float(), None
    if pl is None and buf_ok and PLANES and (Kd >= 2560 or PLANES_ALL):
        pl = split_planes(dy)                # bf16 hi / lo planes, whatever the datapath (see _pack_dgrad_planes)
    dev = pl.device if pl is not None else dy.device
    if out is None:
        out = torch.empty(M, Nd, dtype=torch.float32, device=dev)
    d = _gemm_desc(M, Nd, Kd, conv=conv, src=None if pl is not None else dy, ld_src=0 if pl is not None else cin, out=out, residual=residual, ld_res=ld_res)
    _launch_fwd(d, pl, (dg["hi"], dg["lo"], 0, 3), w_layout=1, ws_device=dev, tag="(dgrad)")
    return out


def pack_weights_geglu(w, bias, mx=False):
    """Second set of forward planes for a GEGLU feed-forward weight w (K, 2F) with its columns (and bias) re-ordered into
    interleaved 32-column blocks [a_q | gate_q], the layout ddpo_gemm_desc.epilogue = 1 expects.  Returns False when
    the shape does not qualify (the caller then keeps the unfused linear + geglu pair).
    mx: the MODEL registers the layer as an f16mx layer whatever its reduction length (the U-Net's FF1): under the f16mx datapath with its cross
    terms (MX_CROSS) and FF1_MX it gets f16mx planes in both column orders (geglu_mx_layer()).  Without the keyword nothing changes."""
    K, N = w.shape
    F = N // 2
    if current_datapath() == "fp32" or (N % 128) or (K % 32):
        return False
    ent = PACKED.get(w.data_ptr())
    if ent is None:
        return False
    mk = lambda: torch.zeros(N, K, dtype=torch.int16, device=w.device)
    if "geglu" not in ent:
        idx = torch.arange(F, device=w.device).view(F // 32, 1, 32)
        perm = torch.cat([idx, idx + F], dim=1).reshape(-1)               # [a_0 | gate_0 | a_1 | gate_1 | ...]
        ent["geglu"] = dict(perm=perm, hi=mk(), lo=mk(), bias=torch.empty(N, dtype=torch.float32, device=w.device), w_layout=1 if W_KBLOCKED else 0)
    g = ent["geglu"]
    wp = w.index_select(1, g["perm"]).contiguous()
    torch.index_select(bias, 0, g["perm"], out=g["bias"])
    if g["w_layout"] == 1:               # K % 32 == 0 here: (K / 32, N, 32) has the element count of (N, K)
        _check(load().ddpo_pack_weights_bf16_kblocked(_p(wp), K, N, _p(g["hi"]), _p(g["lo"]), _stream()), "ddpo_pack_weights_bf16_kblocked")
    else:
        _check(load().ddpo_pack_weights_bf16(_p(wp), K, N, K, _p(g["hi"]), _p(g["lo"]), None, None, _stream()), "ddpo_pack_weights_bf16")
    # second column order for the 256 x 320 GEGLU tile (ddpo_gemm_desc.epilogue = 2, ABI v13): 320-column blocks [a (160) | gate (160)]; bf16x3 layers
    # only (an FF1 registered with mx=True: the f16mx planes of the same order instead, below), k-blocked planes.  Which of the two orders a call
    # uses: geglu_tall_pays().
    ff1_mx = bool(mx and FF1_MX and MX_CROSS and _mx())           # (DDPO_MX_CROSS=0: the tall GEGLU tile has no single-pass f16 form — FF1 stays bf16x3)
    mxp = lambda: dict(w16=torch.zeros(K // 32, N, 32, dtype=torch.int16, device=w.device), w8=torch.zeros(K // 32, N, 64, dtype=torch.uint8, device=w.device),
                       scale=torch.zeros(N, dtype=torch.uint8, device=w.device))
    if GEGLU_TALL and W_KBLOCKED and _x3() and N % 320 == 0 and not (_mx() and K >= MX_MIN_K):
        if "tall" not in g:
            idx = torch.arange(F, device=w.device).view(F // 160, 1, 160)
            g["tall"] = dict(perm=torch.cat([idx, idx + F], dim=1).reshape(-1), **({} if ff1_mx else dict(hi=mk(), lo=mk())),
                             bias=torch.empty(N, dtype=torch.float32, device=w.device))
        t = g["tall"]
        wt = w.index_select(1, t["perm"]).contiguous()
        torch.index_select(bias, 0, t["perm"], out=t["bias"])
        if ff1_mx:                       # the tall column order as f16mx planes (ddpo_gemm_desc.epilogue = 2 on the f16mx entry point)
            if "mx" not in t:
                t["mx"] = mxp()
            m = t["mx"]
            _check(load().ddpo_pack_weights_f16mx(_p(wt), K, N, _p(m["w16"]), _p(m["w8"]), _p(m["scale"]), _stream()), "ddpo_pack_weights_f16mx")
        else:
            t.pop("mx", None)
            if "hi" not in t:
                t.update(hi=mk(), lo=mk())
            _check(load().ddpo_pack_weights_bf16_kblocked(_p(wt), K, N, _p(t["hi"]), _p(t["lo"]), _stream()), "ddpo_pack_weights_bf16_kblocked")
    else:
        g.pop("tall", None)
    if _mx() and (K >= MX_MIN_K or ff1_mx):
        if "mx" not in g:
            g["mx"] = mxp()
        m = g["mx"]
        _check(load().ddpo_pack_weights_f16mx(_p(wp), K, N, _p(m["w16"]), _p(m["w8"]), _p(m["scale"]), _stream()), "ddpo_pack_weights_f16mx")
    else:
        g.pop("mx", None)
    g["stale"] = False
    return True


def geglu_mx_layer(w):
    """True when the fused FF1 + GEGLU of weight `w` runs on the f16mx kernel: f16mx datapath and f16mx planes in the GEGLU column order registered
    (pack_weights_geglu: K >= MX_MIN_K, or mx=True).  A property of the layer, as mx_layer() — the caller's LayerNorm then emits f16mx planes
    (`planes=2`; the training forward keeps fp32, which linear_geglu splits on the way in)."""
    if not _mx():
        return False
    ent = PACKED.get(w.data_ptr())
    return ent is not None and "geglu" in ent and not ent["geglu"]["stale"] and "mx" in ent["geglu"]


def geglu_tall_pays(w, rows):
    """True when the fused FF1 + GEGLU of weight `w` on `rows` rows should run on the 256 x 320 tile (epilogue = 2): registered with the tall column
    order and the grid of tall tiles fills whole rounds of the 256 CUs well — the rule the C++ dispatch
    applies to the plain tall tile (_tall_tiles_fill).  The caller then feeds bf16 hi / lo PLANES
    (LayerNorm `planes=1`) — or, for an FF1 registered as an f16mx layer (geglu_mx_layer), f16mx planes (`planes=2`).  Why: at K = 320 .. 1280 the 128 x 128 GEGLU tile streams 16 MAC per operand byte and FF1 sits on the chip's L2 -> LDS
    stream (3.3 GB per launch at the 64 x 64 level = 8 TB/s); the tall tile moves 35 MAC per byte."""
    ent = PACKED.get(w.data_ptr())
    if not (GEGLU_TALL and PLANES and _x3() and ent is not None and "geglu" in ent and not ent["geglu"]["stale"] and "tall" in ent["geglu"]):
        return False
    if geglu_mx_layer(w) and "mx" not in ent["geglu"]["tall"]:      # an f16mx layer runs the tall tile on f16mx planes of the tall order only
        return False
    K, N = ent["K"], ent["N"]
    if not _fits_buf(rows * K * 4) or K % 32:
        return False
    return _tall_tiles_fill(rows, N)


def linear_geglu(x, w, out=None, planes_out=False, pre_out=False):
    """(x @ w + b)[:, :F] * gelu_tanh((x @ w + b)[:, F:]) in one launch; w must have been registered by pack_weights_geglu.
    Returns None when it was not (caller falls back to linear + geglu).  planes_out: the result comes back as `Planes` only
    (for a plane-fed second feed-forward GEMM).  pre_out: returns (result, pre) with pre = x @ w + b, (M, 2F) fp32 in w's column order —
    the tensor the GEGLU backward needs (training forward; ddpo_gemm_desc.aux_out)."""
    ent = PACKED.get(w.data_ptr())
    if current_datapath() == "fp32" or ent is None or "geglu" not in ent or ent["geglu"]["stale"]:
        return None
    g = ent["geglu"]
    M, K = x.shape
    N = w.shape[1]
    if not _fits_buf(M * K * 4):
        return None
    pl = x if isinstance(x, Planes) else None
    mxl = _mx() and "mx" in g
    if pl is None and mxl:               # an f16mx layer ALWAYS runs on the f16mx kernel (see DATAPATHS): fp32 input is split on the way in
        pl = x = split_planes(x, fmt=1)
    if pl is not None and (not _planes_dp() or K % 32 or (pl.fmt == 1) != mxl):
        raise DdpoHipError("plane-fed linear_geglu needs the bf16x3 / f16mx datapath, K % 32 == 0 and planes of the layer's format "
                           "(ask planes_pay / norm_planes for it)")
    opl = None
    if planes_out:
        if not _planes_dp():
            raise DdpoHipError("plane-emitting linear_geglu needs the bf16x3 / f16mx datapath")
        opl = Planes(M, N // 2, x.device, fmt=1 if planes_out == 2 else 0)            # planes_out = the CONSUMER's planes_pay value
    elif out is None:
        out = torch.empty(M, N // 2, dtype=torch.float32, device=x.device)
    tall = pl is not None and geglu_tall_pays(w, M) and ("mx" if mxl else "hi") in g["tall"]       # (past the check above the planes are of the layer's format: bf16 hi / lo, or f16mx for an f16mx layer)
    gw = g["tall"] if tall else g
    pre = torch.empty(M, N, dtype=torch.float32, device=x.device) if pre_out else None
    d = _gemm_desc(M, N, K, src=x, ld_src=K, out=None if planes_out else out, ld_out=N // 2, bias=gw["bias"], aux_out=pre,
                   out_planes=opl and (opl.hi, opl.lo, opl.ld, opl.fmt), epilogue=2 if tall else 1)
    with _profiled(2.0 * M * N * K, 4.0 * (M * K + K * N + M * N // 2), _family(mx=mxl)):     # (past the checks above, mxl = "pl holds f16mx planes")
        if mxl:
            _launch_fwd(d, pl, gw["mx"])
        elif pl is not None:
            _launch_fwd(d, pl, (gw["hi"], gw["lo"], K, 3 if _x3() else 1), w_layout=1 if tall else g["w_layout"])
        else:
            _launch_fwd(d, None, (g["hi"], g["lo"], K, 3 if _x3() else 1), w_layout=g["w_layout"])
    res = opl if planes_out else out
    return (res, pre) if pre_out else res


def _bf16_route(w, K, N, conv, dgrad):
    """Return (hi, lo, ldw, npass) if this contraction should run on the bf16 MFMA path, else None."""
    if current_datapath() == "fp32":
        return None
    ent = PACKED.get(w.data_ptr())
    if ent is None:
        return None
    cin = conv["Cin"] if conv else K
    if cin % 8:
        return None
    npass = 3 if _x3() else 1
    if dgrad:
        if ent["bwd"] is None or not conv:
            return None
        return ent["bwd"][0], ent["bwd"][1], 0, npass
    if ent["K"] != K or ent["N"] != N:
        return None
    return ent["fwd"][0], ent["fwd"][1], ent["fwd"][2], npass


def gemm_conv(src, w, *, M, N, K, bias=None, rowbias=None, rows_per_batch=0, residual=None, out=None, alpha=1.0,
              w_trans=False, ld_src=None, ld_out=None, ld_res=None, conv=None, planes_out=None, planes_fmt=0, res_rows=0):
    """Generic entry: conv = dict(ksize, stride, pad, upsample, B, H, W, Cin, OH, OW) or None for a dense GEMM.
    res_rows: row period of `residual` (ddpo_gemm_desc.res_rows) — output row m adds residual row m % res_rows, so the residual of a batch
    whose halves share it is held once; 0: one residual row per output row.
    planes_out: None -> returns the fp32 result; "both" -> (fp32, Planes) from ONE launch (the output stage also writes the
    bf16 hi / lo planes a plane-fed consumer reads); "only" -> Planes (no fp32 tensor is written).  Check
    planes_out_ok() first: only the buffer-addressed bf16x3 kernels have the plane-emitting output stage.  planes_fmt: the format the CONSUMER
    wants (its planes_pay value: 2 = f16mx, else bf16 hi / lo)."""
    pl = src if isinstance(src, Planes) else None
    mxl = (not w_trans) and mx_layer(w)
    if mxl:
        # an f16mx layer ALWAYS runs on the f16mx kernel; a producer that wrote fp32 (training forward, layers without a plane-emitting
        # producer) is split on the way in — the same planes its plane-emitting form would have written
        cin_ = conv["Cin"] if conv else K
        rows_ = conv["B"] * conv["H"] * conv["W"] if conv else M
        if not planes_ok(w, cin_, rows_):
            mxl = False                      # not plane-eligible (>= 2 GiB tensors): bf16x3 like every other such layer
        elif pl is None:
            # (a row-strided view — a column slice of a skip-concat buffer — is split like a contiguous tensor: the layer's arithmetic must
            # never depend on where its input is stored)
            if not (src.dim() == 2 and src.shape[0] == rows_ and src.shape[1] == cin_ and src.stride(1) == 1 and
                    (ld_src is None or ld_src == src.stride(0))):
                raise DdpoHipError("an f16mx layer needs its fp32 input as a (rows, channels) tensor or row-strided view")
            pl = src = split_planes(src, fmt=1)
            ld_src = None
    if pl is not None and (pl.fmt == 1) != bool(mxl):
        raise DdpoHipError("activation planes of the wrong format for this layer (ask planes_pay / norm_planes: 1 = bf16 hi / lo, 2 = f16mx)")
    opl = None
    if planes_out is not None:
        if planes_out not in ("both", "only"):
            raise ValueError(planes_out)
        opl = Planes(M, N, src.device, fmt=1 if planes_fmt == 2 else 0)
    if out is None and planes_out != "only":
        out = torch.empty(M, N, dtype=torch.float32, device=src.device)
    cin = conv["Cin"] if conv else K
    d = _gemm_desc(M, N, K, conv=conv, src=src, ld_src=ld_src if ld_src is not None else cin, out=out, ld_out=ld_out, bias=bias, residual=residual,
                   ld_res=ld_res, res_rows=res_rows, alpha=alpha, out_planes=opl and (opl.hi, opl.lo, opl.ld, opl.fmt),
                   w=w.data_ptr(), w_trans=int(bool(w_trans)))
    if rowbias is not None:
        d.rowbias = rowbias.data_ptr(); d.rows_per_batch = int(rows_per_batch); d.ld_rowbias = int(rowbias.shape[-1])
    route = None if w_trans else _bf16_route(w, K, N, conv, False)
    if opl is not None and (route is None or not _planes_dp()):
        raise DdpoHipError("a plane-emitting GEMM needs the bf16x3 / f16mx datapath and registered weight planes (check planes_out_ok)")
    if pl is not None and (route is None or not _planes_dp() or cin % 32 or ld_src is not None):
        raise DdpoHipError("a plane-fed GEMM needs the bf16x3 / f16mx datapath, registered weight planes (of the planes' format) and 32-channel "
                           "k-tiles (check planes_ok before asking a producer for planes)")
    a_bytes = 4.0 * (conv["B"] * conv["H"] * conv["W"] * conv["Cin"] if conv else M * K)       # unique operand bytes
    w_bytes = (4.0 if route is None else (4.0 if _x3() else 2.0)) * K * N
    io_bytes = a_bytes + w_bytes + 4.0 * N * (M + (0 if residual is None else (res_rows or M)))      # a periodic residual is read once per period
    with _profiled(2.0 * M * N * K, io_bytes, _family(fp32=route is None, mx=mxl)):            # (past the checks above, mxl = "pl holds f16mx planes")
        if mxl:
            _launch_fwd(d, pl, PACKED[w.data_ptr()]["mx"], ws_device=src.device)
        elif route is None:
            _launch_fwd(d, None, None)
        else:
            _launch_fwd(d, pl, route, w_layout=PACKED[w.data_ptr()].get("w_layout", 0), ws_device=src.device)
    if planes_out == "only":
        return opl
    return (out, opl) if planes_out == "both" else out


def conv2d(x, w, bias, B, H, W, Cin, Cout, ksize, stride=1, pad=None, upsample=False, **kw):
    """x: (B*H*W, Cin) NHWC rows; w: (ksize,ksize,Cin,Cout) HWIO.  Returns ((B*OH*OW, Cout), OH, OW)."""
    conv = _conv_geom(B, H, W, Cin, ksize, stride, pad, upsample)
    out = gemm_conv(x, w, M=B * conv["OH"] * conv["OW"], N=Cout, K=ksize * ksize * Cin, bias=bias, conv=conv, **kw)
    return out, conv["OH"], conv["OW"]


def linear(x, w, bias=None, **kw):
    """x: (M,K); w: (K,N) (Flax (in,out))."""
    M, K = x.shape
    N = w.shape[0] if kw.get("w_trans") else w.shape[1]
    return gemm_conv(x, w, M=M, N=N, K=K, bias=bias, **kw)


def attention_planes_ok(d):
    """True when the attention for head dim `d` runs on the 16-bit MFMA kernels under the current datapath — the ones whose output stage can
    emit bf16 hi / lo planes (`planes_out=True`)."""
    return current_datapath() != "fp32" and _x3() and d in (8, 16, 40, 64, 80)


def attention(q, k, v, B, heads, Nq, Nk, d, scale=None, out=None, ldq=None, ldk=None, ldv=None, ldo=None, return_lse=False, planes_out=False,
              q_batches=None):
    """planes_out (check attention_planes_ok first): the result comes back as bf16 hi / lo `Planes` of exactly the fp32 values — the operand of
    a plane-fed to_out projection; no fp32 tensor is written.
    q_batches (a divisor of B): q holds q_batches batches of Nq rows and batch b attends with the queries of batch b % q_batches (same kernels,
    same per-query arithmetic); None: one query batch per batch (q_batches = B)."""
    sc = float(scale if scale is not None else d ** -0.5)
    return _attention_shared_q(q, B if q_batches is None else q_batches, k, v, None, B, heads, Nq, Nk, d, sc, out, ldq, ldk, ldv, ldo, return_lse,
                               planes_out)


def _attention_shared_q(q, q_batches, k, v, images, B, heads, Nq, Nk, d, sc, out, ldq, ldk, ldv, ldo, return_lse, planes_out):
    """The one routing of attention() / attention_from_images() (images: K / V come packed) to the three forward entry points (q_batches = B:
    every batch has its own queries)."""
    C = heads * d
    x16 = current_datapath() != "fp32" and d in (8, 16, 40, 64, 80)
    if planes_out and (not attention_planes_ok(d) or out is not None or return_lse):
        raise DdpoHipError("plane-emitting attention needs the bf16x3 / f16mx datapath and a supported head dim, and writes planes only")
    opl = Planes(B * Nq, C, q.device) if planes_out else None
    if opl is None and out is None:
        out = torch.empty(B * Nq, C, dtype=torch.float32, device=q.device)
    lse = torch.empty(B * heads * Nq, dtype=torch.float32, device=q.device) if return_lse else None
    o_args = (None, 0, _p(opl.hi), _p(opl.lo), opl.ld) if opl is not None else (_p(out), int(ldo or C), None, None, 0)
    if images is not None:
        _check(load().ddpo_attention_fwd_images(int(_mx()), _pr(q, ldq), int(ldq or C), int(q_batches), _p(images), images.numel(), *o_args,
                                                _p(lse), B, heads, Nq, Nk, d, sc, _stream()), "ddpo_attention_fwd_images")
    elif x16:
        nb = int(load().ddpo_attention_fwd_x16_ws_bytes(B, heads, Nk, d))      # 0 for short key sequences
        ws = _scratch(nb, q.device, "attn_kv") if nb else None
        _check(load().ddpo_attention_fwd_x16(int(_mx()), _pr(q, ldq), int(ldq or C), int(q_batches), _pr(k, ldk), int(ldk or C), _pr(v, ldv),
                                             int(ldv or C), *o_args, _p(lse), B, heads, Nq, Nk, d, sc, _p(ws), nb, _stream()),
               "ddpo_attention_fwd_x16")
    else:
        _check(load().ddpo_attention_fwd(_pr(q, ldq), int(ldq or C), int(q_batches), _pr(k, ldk), int(ldk or C), _pr(v, ldv), int(ldv or C),
                                         _p(out), int(ldo or C), _p(lse), B, heads, Nq, Nk, d, sc, _stream()), "ddpo_attention_fwd")
    res = opl if opl is not None else out
    return (res, lse) if return_lse else res


CAUSAL_MAX_N = 80       # ddpo_attention_causal_fwd holds all keys of a (batch, head) in LDS


def attention_causal(q, k, v, B, heads, N, d, scale=None, out=None, ldq=None, ldk=None, ldv=None, ldo=None):
    """Causal self-attention (mask key <= query) of the CLIP text tower: N <= CAUSAL_MAX_N tokens, d in (16, 64), exact-fp32 MFMA on every
    datapath (ddpo_attention_causal_fwd).  q / k / v may be column blocks of one fused buffer (ld* = its row stride)."""
    C = heads * d
    sc = float(scale if scale is not None else d ** -0.5)
    if out is None:
        out = torch.empty(B * N, C, dtype=torch.float32, device=q.device)
    _check(load().ddpo_attention_causal_fwd(_pr(q, ldq), int(ldq or C), _pr(k, ldk), int(ldk or C), _pr(v, ldv), int(ldv or C), _pr(out, ldo), int(ldo or C),
                                            B, heads, N, d, sc, _stream()), "ddpo_attention_causal_fwd")
    return out


def attention_kv_images(k, v, B, heads, Nk, d, out=None, ldk=None, ldv=None):
    """Pack K / V (B*Nk, heads*d) once into the per-tile images of the bf16x3 attention kernels (uint8 tensor), for keys / values that
    stay constant over many attention calls (the text context over the DDIM steps).  Returns None where the datapath / head dim has no
    image kernel (the caller keeps k, v)."""
    if current_datapath() == "fp32" or d not in (8, 16, 40, 64, 80):
        if out is not None:
            out._ddpo_kv_fmt = None          # a buffer packed earlier under another datapath no longer matches k, v
        return None
    C = heads * d
    nb = int(load().ddpo_attention_kv_images_bytes(B, heads, Nk, d))
    if out is None or out.numel() < nb:
        out = torch.empty(nb, dtype=torch.uint8, device=k.device)
    _check(load().ddpo_attention_pack_kv(int(_mx()), _p(k), int(ldk or C), _p(v), int(ldv or C), _p(out), out.numel(), B, heads, Nk, d, _stream()),
           "ddpo_attention_pack_kv")
    out._ddpo_kv_fmt = kv_images_fmt()       # the two packings have the same size and incompatible contents: the images carry their format
    return out


def kv_images_fmt():
    """Packing of attention_kv_images() under the current datapath: "f16p" (f16mx datapath: V as f16 hi / lo with a row of ones), "bf16x3"
    (bf16 hi / lo), or None on the fp32 datapath (no image kernels)."""
    if current_datapath() == "fp32":
        return None
    return "f16p" if _mx() else "bf16x3"


def kv_images_valid(images):
    """True when `images` were packed by attention_kv_images() under the packing the CURRENT datapath's kernels read."""
    fmt = kv_images_fmt()
    return images is not None and fmt is not None and getattr(images, "_ddpo_kv_fmt", None) == fmt


def attention_from_images(q, images, B, heads, Nq, Nk, d, scale=None, out=None, ldq=None, ldo=None, return_lse=False, planes_out=False,
                          q_batches=None):
    """softmax(q k^T * scale) v with k, v given as attention_kv_images() — packed under the SAME datapath (the f16mx datapath's images hold V as
    f16 hi / lo with a row of ones, the bf16x3 datapath's as bf16 hi / lo).  planes_out, q_batches: as in attention()."""
    C = heads * d
    if not kv_images_valid(images):
        raise DdpoHipError(f"attention_from_images: images packed as {getattr(images, '_ddpo_kv_fmt', None)!r}, the current datapath "
                           f"({current_datapath()}) reads {kv_images_fmt()!r} — repack with attention_kv_images()")
    return _attention_shared_q(q, B if q_batches is None else q_batches, None, None, images, B, heads, Nq, Nk, d,
                               float(scale if scale is not None else d ** -0.5), out, ldq, None, None, ldo, return_lse, planes_out)


def attention_bwd(q, k, v, o, d_o, lse, B, heads, Nq, Nk, d, scale=None):
    """Returns (dq, dk, dv), contiguous (rows, heads*d)."""
    C = heads * d
    dq = torch.empty(B * Nq, C, dtype=torch.float32, device=q.device)
    dk = torch.empty(B * Nk, C, dtype=torch.float32, device=q.device)
    dv = torch.empty(B * Nk, C, dtype=torch.float32, device=q.device)
    dvec = torch.empty(B * heads * (Nq + 1), dtype=torch.float32, device=q.device)        # rowsum(dO * O) + one max-|dO| word per (batch, head) slab
    args = (_p(q), C, _p(k), C, _p(v), C, _p(o), _p(d_o), _p(lse), _p(dvec), _p(dq), _p(dk), _p(dv),
            B, heads, Nq, Nk, d, float(scale if scale is not None else d ** -0.5), _stream())
    if current_datapath() != "fp32" and d in (8, 16, 40, 64, 80):
        _check(load().ddpo_attention_bwd_x16(int(_mx()), *args), "ddpo_attention_bwd_x16")
    else:
        _check(load().ddpo_attention_bwd(*args), "ddpo_attention_bwd")
    return dq, dk, dv


def layernorm_bwd(x, dy, gamma, dgamma, dbeta, eps=1e-5, dx_add=None):
    rows, C = x.shape
    dx = torch.empty_like(x)
    ws = _scratch(load().ddpo_layernorm_bwd_ws_bytes(rows, C), x.device, "lnb")
    _check(load().ddpo_layernorm_bwd(_p(x), _p(dy), _p(gamma), rows, C, float(eps), _p(dx_add), _p(dx), _p(dgamma), _p(dbeta), _p(ws), _stream()),
           "ddpo_layernorm_bwd")
    return dx


def geglu_bwd(x, dy):
    rows, F2 = x.shape
    dx = torch.empty_like(x)
    _check(load().ddpo_geglu_bwd(_p(x), _p(dy), _p(dx), rows, F2 // 2, _stream()), "ddpo_geglu_bwd")
    return dx


def silu_bwd(x, dy):
    dx = torch.empty_like(x)
    _check(load().ddpo_silu_bwd(_p(x), _p(dy), _p(dx), x.numel(), _stream()), "ddpo_silu_bwd")
    return dx


def colsum_accum(x, out, rows_per_seg=0, ld_x=None):
    """out[seg, :] += column sums of x over each segment of rows_per_seg rows (0: all rows -> out is (cols,))."""
    rows, cols = x.shape
    _check(load().ddpo_colsum_accum(_p(x), int(ld_x or cols), rows, cols, int(rows_per_seg), _p(out), _stream()), "ddpo_colsum_accum")
    return out


def sumpool2x2(x, B, H, W, C):
    """x: (B*2H*2W, C) -> (B*H*W, C)."""
    out = torch.empty(B * H * W, C, dtype=torch.float32, device=x.device)
    _check(load().ddpo_sumpool2x2(_p(x), _p(out), B, H, W, C, _stream()), "ddpo_sumpool2x2")
    return out


def add(a, b, out=None):
    if out is None:
        out = torch.empty_like(a)
    _check(load().ddpo_add(_p(a), _p(b), _p(out), a.numel(), _stream()), "ddpo_add")
    return out


def linear_dgrad(dy, w, residual=None):
    """dx = dy @ w^T for the forward y = x @ w, w: (K, N) Flax layout."""
    M, N = dy.shape
    K = w.shape[0]
    ent = PACKED.get(w.data_ptr()) if current_datapath() != "fp32" else None
    if ent is not None and ent.get("dg") is not None and _x3():
        return _dgrad_fwd(dy, ent["dg"], M=M, residual=residual)
    if ent is not None and ent["bwd"] is not None and N % 8 == 0:
        # the original (K, N) order is exactly "output column k, reduction index n contiguous": forward-style planes with ldw = N
        out = torch.empty(M, K, dtype=torch.float32, device=dy.device)
        d = _gemm_desc(M, K, N, src=dy, ld_src=N, out=out, residual=residual)
        _launch_fwd(d, None, (ent["bwd"][0], ent["bwd"][1], int(N), 3 if _x3() else 1), ws_device=dy.device, tag="(dgrad)")
        return out
    return gemm_conv(dy, w, M=M, N=K, K=N, w_trans=True, residual=residual)


def linear_wgrad(x, dy, dw, dbias=None):
    """dw (K,N) += x^T @ dy  [and dbias (N,) += column sums of dy]."""
    M, K = x.shape
    N = dy.shape[1]
    return gemm_wgrad(x, dy, dw, M=M, N=N, K=K, dbias=dbias)


def gemm_wgrad(src, dy, dw, *, M, N, K, conv=None, ld_src=None, ld_dy=None, accumulate=True, splits=0, alpha=1.0, dbias=None):
    """dw += A^T dY.  `src` / `dy` may be `Planes` (the forward input as a plane-emitting norm wrote it, dY from a plane-emitting
    output stage): the bf16x3 kernel then skips the fp32 -> bf16 split of that operand.
    dbias: the layer's bias gradient (N,), += sum_m dY[m, :] — folded into the bf16x3 weight-gradient launch (ddpo_gemm_desc.colsum: the kernel
    sums the dY values it stages anyway) when dY is fp32; a separate ddpo_colsum_accum launch otherwise."""
    fast = current_datapath() != "fp32" and accumulate and (conv is None or (conv["stride"] in (1, 2) and conv["upsample"] in (0, 1) and
                                                                      conv["pad"] == conv["ksize"] // 2)) and K >= 64 and N >= 32
    spl = src if isinstance(src, Planes) else None
    dpl = dy if isinstance(dy, Planes) else None
    if not fast or not _x3():           # exact-fp32 / single-pass kernels take fp32 operands (small layers: conv_out, tests)
        if spl is not None:
            src, spl = spl.float(), None
        if dpl is not None:
            dy, dpl = dpl.float(), None
    if spl is not None and spl.fmt == 1:          # the weight gradients run on bf16x3: f16mx planes are decoded (tests only — the models keep
        src, spl = spl.float(), None              # fp32 activations for the backward in front of an f16mx layer, lib.norm_planes())
    if dpl is not None and dpl.fmt == 1:
        dy, dpl = dpl.float(), None
    d = _gemm_desc(M, N, K, conv=conv, src=src if spl is None else None, ld_src=ld_src if ld_src is not None else (conv["Cin"] if conv else K),
                   out=dw, alpha=alpha, ld_w=int(ld_dy if ld_dy is not None else N), accumulate=int(bool(accumulate)), splits=int(splits))
    if dpl is None:
        d.w = dy.data_ptr()
    if spl is not None:                  # plane operands carry their own layout (row stride 0 = k-blocked)
        if ld_src is not None and spl.kblocked:
            raise DdpoHipError("a column slice of k-blocked planes cannot be a wgrad operand")
        d.ld_src = spl.ld if ld_src is None else d.ld_src
    if dpl is not None:
        if ld_dy is not None and dpl.kblocked:
            raise DdpoHipError("a column slice of k-blocked planes cannot be a wgrad operand")
        d.ld_w = dpl.ld if ld_dy is None else d.ld_w
    fused_bias = dbias is not None and fast and dpl is None
    if fused_bias:
        d.colsum = dbias.data_ptr()
    elif dbias is not None:
        colsum_accum(dy if dpl is None else dpl.float(), dbias, ld_x=ld_dy)
    if fast and (spl is not None or dpl is not None):
        _check(load().ddpo_gemm_conv_wgrad_bf16x3_planes(byref(d), _p(spl.hi) if spl else None, _p(spl.lo) if spl else None,
                                                         _p(dpl.hi) if dpl else None, _p(dpl.lo) if dpl else None, _stream()),
               "ddpo_gemm_conv_wgrad_bf16x3_planes")
    elif fast:
        _check(load().ddpo_gemm_conv_wgrad_bf16x3(byref(d), _stream()), "ddpo_gemm_conv_wgrad_bf16x3")
    else:
        _check(load().ddpo_gemm_conv_wgrad(byref(d), _stream()), "ddpo_gemm_conv_wgrad")
    return dw


def conv2d_wgrad(x, dy, dw, B, H, W, Cin, Cout, ksize, stride=1, pad=None, upsample=False, ld_src=None, dbias=None):
    """dw (ksize,ksize,Cin,Cout) += im2col(x)^T @ dy, x: forward input (B*H*W, Cin), dy: (B*OH*OW, Cout)  [dbias (Cout,) += column sums of dy]."""
    conv = _conv_geom(B, H, W, Cin, ksize, stride, pad, upsample)
    return gemm_wgrad(x, dy, dw, M=B * conv["OH"] * conv["OW"], N=Cout, K=ksize * ksize * Cin, conv=conv, ld_src=ld_src, dbias=dbias)


def conv2d_dgrad(dy, w, B, H, W, Cin, Cout, ksize, stride=1, residual=None):
    """Gradient w.r.t. the input of y = conv(x, w) (pad = ksize//2, no upsample): x was (B*H*W, Cin), dy is (B*OH*OW, Cout).
    Returns (B*H*W, Cin).  stride 2 uses the zero-insert gather (transposed convolution)."""
    fwd = _conv_geom(B, H, W, Cin, ksize, stride, None, False)
    OH, OW = fwd["OH"], fwd["OW"]
    if stride == 2 and (H != 2 * OH or W != 2 * OW):
        raise DdpoHipError("stride-2 dgrad expects even input sizes")
    # the transposed view: a stride-1 convolution of dY (zero-inserted for stride 2) with the channel roles swapped, back onto the (H, W) grid
    conv = _conv_geom(B, OH, OW, Cout, ksize, 1, None, 2 if stride == 2 else 0)
    ent = PACKED.get(w.data_ptr()) if current_datapath() != "fp32" else None
    if ent is not None and ent.get("dg") is not None and _x3():
        return _dgrad_fwd(dy, ent["dg"], M=B * H * W, conv=conv, residual=residual)
    if isinstance(dy, Planes):
        dy = dy.float()
    out = torch.empty(B * H * W, Cin, dtype=torch.float32, device=dy.device)
    d = _gemm_desc(B * H * W, Cin, ksize * ksize * Cout, conv=conv, src=dy, ld_src=Cout, out=out, residual=residual, w=w.data_ptr(), w_trans=1, w_dgrad=1)
    route = _bf16_route(w, d.K, d.N, conv, True)
    _launch_fwd(d, None, route, ws_device=None if route is None else dy.device, tag="(dgrad)")
    return out


def geglu(x):
    rows, F2 = x.shape
    out = torch.empty(rows, F2 // 2, dtype=torch.float32, device=x.device)
    _check(load().ddpo_geglu_fwd(_p(x), _p(out), rows, F2 // 2, _stream()), "ddpo_geglu_fwd")
    return out


def silu(x):
    out = torch.empty_like(x)
    _check(load().ddpo_silu_fwd(_p(x), _p(out), x.numel(), _stream()), "ddpo_silu_fwd")
    return out


def quick_gelu(x, out=None):
    """x * sigmoid(1.702 x) (the OpenAI CLIP activation); in place when out is x."""
    if out is None:
        out = torch.empty_like(x)
    _check(load().ddpo_quick_gelu_fwd(_p(x), _p(out), x.numel(), _stream()), "ddpo_quick_gelu_fwd")
    return out


def l2_normalize_rows(x):
    rows, cols = x.shape
    out = torch.empty_like(x)
    _check(load().ddpo_l2_normalize_rows(_p(x), _p(out), rows, cols, _stream()), "ddpo_l2_normalize_rows")
    return out


def gather_rows(table, idx, add=None, out=None):
    """out[r] = table[idx[r]] (+ add[r % len(add)]): table (T, cols) row-major (a row-strided view is fine), idx int32 on the device, add
    (period, cols) contiguous.  The kernel clamps an out-of-range index into the table; callers that build `idx` from user data validate it
    on the host first (`check_indices`)."""
    if table.dim() != 2 or idx.dtype != torch.int32 or idx.dim() != 1:
        raise DdpoHipError("gather_rows needs a 2-D table and a 1-D int32 index tensor")
    rows, cols = idx.numel(), table.shape[1]
    if add is not None and (add.dim() != 2 or add.shape[1] != cols):
        raise DdpoHipError(f"gather_rows: add must be (period, {cols}), got {tuple(add.shape)}")
    if out is None:
        out = torch.empty(rows, cols, dtype=torch.float32, device=table.device)
    _check(load().ddpo_gather_rows(_p_rows(_f32(table, "table")), int(table.stride(0)), int(table.shape[0]), _p(idx), rows, cols, _p(add),
                                   int(add.shape[0]) if add is not None else 0, _p(out), _stream()), "ddpo_gather_rows")
    return out


def check_indices(idx, table_rows, what="index"):
    """Host-side validation of gather indices (a numpy array) before they are uploaded: raises on anything outside [0, table_rows)."""
    import numpy as np
    idx = np.asarray(idx)
    if idx.size and (idx.min() < 0 or idx.max() >= table_rows):
        bad = idx[(idx < 0) | (idx >= table_rows)]
        raise ValueError(f"{what} {int(bad.flat[0])} outside [0, {table_rows})")
    return idx


def cosine_rows(a, b, scale=1.0, out=None):
    """out[r] = scale * cos(a_r, b_r) for two (rows, cols) tensors, one wave per row (ddpo_cosine_rows)."""
    if a.shape != b.shape or a.dim() != 2:
        raise DdpoHipError(f"cosine_rows needs two equal 2-D shapes, got {tuple(a.shape)} and {tuple(b.shape)}")
    rows, cols = a.shape
    if out is None:
        out = torch.empty(rows, dtype=torch.float32, device=a.device)
    _check(load().ddpo_cosine_rows(_p(_f32(a, "a")), _p(_f32(b, "b")), rows, cols, float(scale), _p(out), _stream()), "ddpo_cosine_rows")
    return out


# ------------------------------------------------------------------------------------------------ rewards on device images
def _cuda_images(who, images, any_dtype=False):
    if not isinstance(images, torch.Tensor) or not images.is_cuda or not (any_dtype or images.dtype in (torch.float32, torch.uint8)):
        raise DdpoHipError(f"{who} needs a float32 or uint8 CUDA tensor")


def _workspace_or_scratch(who, workspace, nbytes, device, tag):
    """`workspace` checked — uint8, at least `nbytes`, on `device` — or, when None, this stream's scratch for `tag`"""
    if workspace is None:
        workspace = _scratch(nbytes, device, tag)
    if workspace.dtype != torch.uint8 or workspace.numel() < nbytes or workspace.device != device:
        raise DdpoHipError(f"{who}: the workspace must be a uint8 tensor of >= {nbytes} bytes on {device}")
    return workspace


def _images_nhwc(who, images, square=False):
    """The rules every reward entry shares, each refused by name: (N, H, W) of a float32 / uint8 contiguous N x H x W x 3 batch, a tensor or a
    numpy array, that is not empty (and square, for rotate4_u8)."""
    is_tensor = isinstance(images, torch.Tensor)
    f32, u8 = (torch.float32, torch.uint8) if is_tensor else ("float32", "uint8")
    if images.dtype not in (f32, u8):
        raise ValueError(f"{who}: the dtype must be float32 or uint8, got {images.dtype} (uint8 or float32 images only)")
    shape = tuple(images.shape)
    if len(shape) != 4 or shape[3] != 3:
        raise ValueError(f"{who} needs N x H x W x 3 images (last dimension 3), got shape {shape}")
    if shape[0] < 1 or shape[1] < 1 or shape[2] < 1:
        raise ValueError(f"{who}: empty batch or empty images, got shape {shape}")
    if not (images.is_contiguous() if is_tensor else images.flags.c_contiguous):
        raise ValueError(f"{who} needs contiguous images (N x H x W x 3 in memory order)")
    if square and shape[1] != shape[2]:
        raise ValueError(f"{who} needs square images (a right-angle turn of a {shape[1]} x {shape[2]} image has another shape)")
    return int(shape[0]), int(shape[1]), int(shape[2])


def _out_or_empty(who, out, shape, dtype, device, name="out"):
    """`out` checked — contiguous, `dtype`, `shape`, on `device`: the kernels write shape-many elements from its pointer on — or, when None, a
    new tensor"""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if out.dtype != dtype or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.device != device:
        raise DdpoHipError(f"{who}: {name} must be a contiguous {str(dtype).split('.')[-1]} {tuple(shape)} tensor on {device}")
    return out


def _np_ptr(a):
    return a.ctypes.data_as(c_void_p)


# ------------------------------------------------------------------------------------------------ JPEG file size
JPEG_FIXED_BYTES = 625        # DDPO_JPEG_FIXED_BYTES of include/ddpo_hip.h: the bytes of a file that are not entropy-coded data
JPEG_SIZE_RULE = "height and width must be multiples of 16 (the 4:2:0 MCU): edge replication and dummy blocks are not built"


def _jpeg_size_args(images, quality):
    n, h, w = _images_nhwc("jpeg_size", images)
    if h % 16 or w % 16:
        raise ValueError(f"jpeg_size: {h} x {w} images: {JPEG_SIZE_RULE}")
    if int(quality) != quality or not 1 <= quality <= 100:
        raise ValueError(f"jpeg_size: quality must be an integer in 1..100, got {quality!r}")
    return n, h, w, int(quality)


def jpeg_size_workspace_bytes(n, h, w):
    nb = c_size_t(0)
    rc = load().ddpo_jpeg_size_workspace_bytes(int(n), int(h), int(w), byref(nb))
    if rc == -1:
        raise ValueError(f"jpeg_size: {n} images of {h} x {w}: {JPEG_SIZE_RULE}")
    _check(rc, "ddpo_jpeg_size_workspace_bytes")
    return int(nb.value)


def jpeg_size(images, quality=95, workspace=None, out=None):
    """len(PIL JPEG bytes at `quality`) of every image of an N x H x W x 3 CUDA tensor — uint8, or float32 in [0, 1] truncated as
    (x * 255).astype(uint8) — as an int64 CUDA tensor, on the current stream; no file is produced (ddpo_jpeg_size).  H and W must be multiples of 16
    (ValueError).  `workspace`: a uint8 CUDA tensor of at least jpeg_size_workspace_bytes(N, H, W) bytes; default: this stream's scratch.
    `out`: a contiguous int64 CUDA tensor (N,) to write into."""
    _cuda_images("jpeg_size", images)
    n, h, w, quality = _jpeg_size_args(images, quality)
    nb = jpeg_size_workspace_bytes(n, h, w)
    workspace = _workspace_or_scratch("jpeg_size", workspace, nb, images.device, "jpeg_size")
    out = _out_or_empty("jpeg_size", out, (n,), torch.int64, images.device)
    _check(load().ddpo_jpeg_size(_p(images), int(images.dtype == torch.float32), n, h, w, quality, _p(workspace), workspace.numel(), _p(out),
                                 _stream()), "ddpo_jpeg_size")
    return out


def jpeg_size_host(images_u8, quality=95):
    """The same count computed serially on the host (ddpo_jpeg_size_host) for a uint8 N x H x W x 3 numpy array: the GPU-free reference."""
    import numpy as np
    a = np.ascontiguousarray(images_u8)
    if a.dtype != np.uint8:
        raise ValueError("jpeg_size_host needs uint8 images")
    n, h, w, quality = _jpeg_size_args(a, quality)
    out = np.zeros(n, dtype=np.int64)
    _check(load().ddpo_jpeg_size_host(_np_ptr(a), n, h, w, quality, _np_ptr(out)), "ddpo_jpeg_size_host")
    return out


# ------------------------------------------------------------------------------------------------ JPEG files
JPEG_HEADER_BYTES = 623       # DDPO_JPEG_HEADER_BYTES: everything a file holds before its scan data
JPEG_MAX_DIM = 65500          # the largest height or width libjpeg writes


def _jpeg_encode_args(images, quality):
    n, h, w, quality = _jpeg_size_args(images, quality)
    if h > JPEG_MAX_DIM or w > JPEG_MAX_DIM:
        raise ValueError(f"jpeg_encode: {h} x {w} images: a JPEG file holds at most {JPEG_MAX_DIM} rows and columns")
    return n, h, w, quality


def jpeg_encode_max_bytes(h, w):
    """Upper bound of the length of one h x w file of jpeg_encode (ddpo_jpeg_encode_max_bytes): a row stride no file exceeds."""
    nb = c_size_t(0)
    rc = load().ddpo_jpeg_encode_max_bytes(int(h), int(w), byref(nb))
    if rc == -1:
        raise ValueError(f"jpeg_encode: {h} x {w} images: {JPEG_SIZE_RULE}, and at most {JPEG_MAX_DIM}")
    _check(rc, "ddpo_jpeg_encode_max_bytes")
    return int(nb.value)


def jpeg_encode(images, quality=80, workspace=None, files=None, stride=None):
    """The bytes PIL's Image.save(buf, "JPEG", quality=q) writes for every image of an N x H x W x 3 CUDA tensor — uint8, or float32 in [0, 1]
    truncated as (x * 255).astype(uint8) — on the current stream (ddpo_jpeg_encode).  Returns (files, lengths): a uint8 CUDA tensor (N, stride)
    whose row n starts with file n, and the int64 CUDA lengths, equal to jpeg_size's.  A file longer than `stride` (default H * W * 3 + 625;
    jpeg_encode_max_bytes(H, W) is never exceeded) leaves its first `stride` bytes and still reports its full length; bytes of a row past the
    file are not written.  `files`: a contiguous uint8 CUDA tensor (N, stride) to write into.  `workspace`: as for jpeg_size."""
    _cuda_images("jpeg_encode", images)
    n, h, w, quality = _jpeg_encode_args(images, quality)
    if stride is None:
        stride = int(files.shape[1]) if files is not None and files.dim() == 2 else h * w * 3 + JPEG_FIXED_BYTES
    if int(stride) != stride or stride < JPEG_FIXED_BYTES:
        raise ValueError(f"jpeg_encode: the row stride must be an integer >= {JPEG_FIXED_BYTES}, got {stride!r}")
    stride = int(stride)
    nb = jpeg_size_workspace_bytes(n, h, w)
    workspace = _workspace_or_scratch("jpeg_encode", workspace, nb, images.device, "jpeg_size")
    files = _out_or_empty("jpeg_encode", files, (n, stride), torch.uint8, images.device, name="files")
    lengths = torch.empty(n, dtype=torch.int64, device=images.device)
    _check(load().ddpo_jpeg_encode(_p(images), int(images.dtype == torch.float32), n, h, w, quality, _p(workspace), workspace.numel(), _p(files),
                                   stride, _p(lengths), _stream()), "ddpo_jpeg_encode")
    return files, lengths


def jpeg_encode_host(images_u8, quality=80):
    """The same files produced serially on the host (ddpo_jpeg_encode_host) for a uint8 N x H x W x 3 numpy array, as a list of bytes: the
    GPU-free reference."""
    import numpy as np
    a = np.ascontiguousarray(images_u8)
    if a.dtype != np.uint8:
        raise ValueError("jpeg_encode_host needs uint8 images")
    n, h, w, quality = _jpeg_encode_args(a, quality)
    stride = jpeg_encode_max_bytes(h, w)
    files, lengths = np.empty((n, stride), dtype=np.uint8), np.zeros(n, dtype=np.int64)
    _check(load().ddpo_jpeg_encode_host(_np_ptr(a), n, h, w, quality, _np_ptr(files), stride, _np_ptr(lengths)), "ddpo_jpeg_encode_host")
    return [files[i, :lengths[i]].tobytes() for i in range(n)]


# ------------------------------------------------------------------------------------------------ CLIP image preprocessing
CLIP_PRECISION_BITS = 22      # CP_PRECISION_BITS of csrc/clip_preprocess_core.h
CLIP_LDS_LIMIT = 160 * 1024   # CP_LDS_LIMIT
CLIP_STAGE_ROWS = 8           # CP_STAGE_ROWS
CLIP_PREPROCESS_RULE = ("the input rows one patch row needs, resampled horizontally to bytes (rows x size x 3), plus 8 staged input rows "
                        "(W x 3 bytes each) and the 3 KB normalisation table must fit the 160 KB of LDS")


def _bicubic(t):
    a = -0.5
    t = abs(t)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


@functools.lru_cache(maxsize=None)
def clip_preprocess_tables(in_size, out_size):
    """(coef, bounds, ksize) of one axis of Pillow's 8-bit bicubic resize from `in_size` to `out_size` pixels, restated: coef (out_size, ksize)
    int32, the weights of output pixel xx as 22-bit fixed point (unused taps 0); bounds (out_size, 2) int32, {first input pixel, tap count}.
    Float64 scalar arithmetic in Pillow's order — weights at (x + xmin - center + 0.5) * (1 / filterscale), summed left to right, each divided
    by the sum, rounded half away from zero — so the integers are Pillow's.  An axis that keeps its size is not resampled by Pillow; it gets
    the identity table here (one tap of 2^22: (p * 2^22 + 2^21) >> 22 == p), which lets the kernel treat every axis alike.  Read-only arrays."""
    import numpy as np
    I, O = int(in_size), int(out_size)
    if I < 1 or O < 1:
        raise ValueError(f"clip_preprocess_tables: sizes must be positive, got {in_size} -> {out_size}")
    one = 1 << CLIP_PRECISION_BITS
    if I == O:
        ksize = 1
        coef = np.full((O, 1), one, dtype=np.int32)
        bounds = np.stack([np.arange(O, dtype=np.int32), np.ones(O, dtype=np.int32)], axis=1)
    else:
        scale = I / O
        fs = max(scale, 1.0)
        support = 2.0 * fs
        ksize = int(math.ceil(support)) * 2 + 1
        ss = 1.0 / fs
        coef = np.zeros((O, ksize), dtype=np.int32)
        bounds = np.zeros((O, 2), dtype=np.int32)
        for xx in range(O):
            center = (xx + 0.5) * scale
            xmin = max(int(center - support + 0.5), 0)
            xmax = min(int(center + support + 0.5), I) - xmin
            w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
            ww = 0.0
            for v in w:
                ww += v
            for x, v in enumerate(w):
                k = v / ww if ww != 0.0 else v
                coef[xx, x] = int(k * one - 0.5) if k < 0 else int(k * one + 0.5)
            bounds[xx] = (xmin, xmax)
    coef.setflags(write=False)
    bounds.setflags(write=False)
    return coef, bounds, ksize


@functools.lru_cache(maxsize=None)
def clip_norm_table(mean=None, std=None):
    """256 x 3 float32: entry (b, c) is what models.clip_vision.preprocess makes of byte b in channel c, by its very expression."""
    import numpy as np
    if mean is None or std is None:
        from .models.clip_vision import CLIP_MEAN, CLIP_STD
        mean, std = CLIP_MEAN, CLIP_STD
    mean, std = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    b = np.arange(256, dtype=np.uint8)[:, None].repeat(3, axis=1)
    f = (b.astype(np.float32) * (1 / 255)).astype(np.float32)
    t = np.ascontiguousarray(((f - mean) / std).astype(np.float32))
    t.setflags(write=False)
    return t


def _band_lds_bytes(rows, out_w, w, norm_table):
    """cp_lds_bytes of csrc/clip_preprocess_core.h"""
    up = lambda px: (px * 3 + 15) // 16 * 16
    return rows * up(out_w) + CLIP_STAGE_ROWS * up(w) + (256 * 3 * 4 if norm_table else 0)


def _band_rows(vb, first, count, band):
    """The most input rows a band of `band` output rows spans, over the output rows [first, first + count) of a vertical bound table"""
    ends = vb[:, 0] + vb[:, 1]
    return max(int(ends[y0:min(y0 + band, first + count)].max() - vb[y0, 0]) for y0 in range(first, first + count, band))


@functools.lru_cache(maxsize=None)
def clip_preprocess_geometry(h, w, size, patch, k_pad):
    """Resize and crop geometry exactly as models.clip_vision.preprocess computes it, checked: dict(oh, ow, top, left, rows) — the resized image,
    the centre-crop origin and the most input rows one patch row spans.  ValueError with the rule that is broken."""
    h, w, size, patch, k_pad = int(h), int(w), int(size), int(patch), int(k_pad)
    if h < 1 or w < 1 or size < 1 or patch < 1:
        raise ValueError(f"clip_preprocess: sizes must be positive, got {h} x {w} images, size {size}, patch {patch}")
    if size % patch:
        raise ValueError(f"clip_preprocess: size {size} is not a multiple of patch {patch}")
    if k_pad < 3 * patch * patch or k_pad % 4:
        raise ValueError(f"clip_preprocess: k_pad {k_pad} must be a multiple of 4 and at least 3 * patch * patch = {3 * patch * patch}")
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    ow, oh = (new_short, new_long) if w <= h else (new_long, new_short)
    top, left = (oh - size) // 2, (ow - size) // 2
    _, vb, _ = clip_preprocess_tables(h, oh)
    rows = max(_band_rows(vb, top, size, patch), 1)
    if _band_lds_bytes(rows, size, w, True) > CLIP_LDS_LIMIT:
        raise ValueError(f"clip_preprocess: {h} x {w} images to {size} need {rows} rows = {_band_lds_bytes(rows, size, w, True)} bytes: {CLIP_PREPROCESS_RULE}")
    return dict(oh=oh, ow=ow, top=top, left=left, rows=rows)


_clip_dev_tables = {}


def _clip_device_tables(key, make, device):
    """int32 / float32 tables as device tensors, uploaded once per (table, device) — a blocking copy, so any stream may read them afterwards."""
    key = key + (str(device),)
    ent = _clip_dev_tables.get(key)
    if ent is None:
        ent = tuple(torch.from_numpy(a.copy()).to(device) for a in make())
        _clip_dev_tables[key] = ent
    return ent


def clip_preprocess(images, size, patch, k_pad, out=None):
    """models.clip_vision.preprocess + the im2col of the patch embedding in one launch on the current stream (ddpo_clip_preprocess): an
    N x H x W x 3 CUDA tensor — float32 in [0, 1], truncated as (x * 255).astype(uint8), or uint8 — to the (N * g * g, k_pad) float32 patch
    matrix, g = size // patch, rows (n, gy, gx), columns (c, ky, kx), pad columns zero.  Equal bit for bit to the host path (Pillow's bicubic
    resize of the short side to `size`, centre crop, CLIP normalisation).  ValueError names the broken rule (CLIP_PREPROCESS_RULE for LDS)."""
    _cuda_images("clip_preprocess", images)
    n, h, w = _images_nhwc("clip_preprocess", images)
    geo = clip_preprocess_geometry(h, w, size, patch, k_pad)
    g = size // patch
    hc, hb = _clip_device_tables(("axis", w, geo["ow"]), lambda: clip_preprocess_tables(w, geo["ow"])[:2], images.device)
    vc, vb = _clip_device_tables(("axis", h, geo["oh"]), lambda: clip_preprocess_tables(h, geo["oh"])[:2], images.device)
    norm, = _clip_device_tables(("norm",), lambda: (clip_norm_table(),), images.device)
    out = _out_or_empty("clip_preprocess", out, (n * g * g, k_pad), torch.float32, images.device)
    _check(load().ddpo_clip_preprocess(_p(images), int(images.dtype == torch.float32), n, h, w, geo["oh"], geo["ow"], geo["top"], geo["left"],
                                       int(size), int(patch), _p(hc), _p(hb), hc.shape[1], _p(vc), _p(vb), vc.shape[1], geo["rows"], _p(norm),
                                       _p(out), int(k_pad), _stream()), "ddpo_clip_preprocess")
    return out


def clip_preprocess_host(images, size, patch, k_pad, return_resized=False):
    """The same patch matrix computed serially on the host (ddpo_clip_preprocess_host) for a uint8 or float32 N x H x W x 3 numpy array: the
    GPU-free reference.  return_resized: also the N x size x size x 3 uint8 image before normalisation (what Pillow's resize + crop gives)."""
    import numpy as np
    a = np.ascontiguousarray(images)
    n, h, w = _images_nhwc("clip_preprocess_host", a)
    geo = clip_preprocess_geometry(h, w, size, patch, k_pad)
    g = size // patch
    hc, hb, hk = clip_preprocess_tables(w, geo["ow"])
    vc, vb, vk = clip_preprocess_tables(h, geo["oh"])
    norm = clip_norm_table()
    out = np.full((n * g * g, k_pad), np.nan, dtype=np.float32)
    resized = np.zeros((n, size, size, 3), dtype=np.uint8)
    _check(load().ddpo_clip_preprocess_host(_np_ptr(a), int(a.dtype == np.float32), n, h, w, geo["oh"], geo["ow"], geo["top"], geo["left"],
                                            int(size), int(patch), _np_ptr(hc), _np_ptr(hb), hk, _np_ptr(vc), _np_ptr(vb), vk, _np_ptr(norm),
                                            _np_ptr(out), int(k_pad), _np_ptr(resized)), "ddpo_clip_preprocess_host")
    return (out, resized) if return_resized else out


# ------------------------------------------------------------------------------------------------ 8-bit bicubic resize to bytes
RESIZE_U8_BAND = 2            # output rows of one workgroup (measured: DESIGN.md 2e); 1 where 2 break the LDS rule
RESIZE_U8_RULE = ("the input rows one band of output rows needs (2 output rows, or 1 where 2 do not fit), resampled horizontally to bytes "
                  "(rows x ow x 3), plus 8 staged input rows (W x 3 bytes each) must fit the 160 KB of LDS")


@functools.lru_cache(maxsize=None)
def resize_u8_geometry(h, w, oh, ow):
    """dict(band, rows) of a resize of h x w images to oh x ow: the output rows one workgroup makes — RESIZE_U8_BAND, halved while the LDS rule
    is broken — and the most input rows such a band spans (by 16: 16 (band - 1) + 64).  ValueError with the rule that is broken."""
    h, w, oh, ow = int(h), int(w), int(oh), int(ow)
    if h < 1 or w < 1 or oh < 1 or ow < 1:
        raise ValueError(f"resize_u8: sizes must be positive, got {h} x {w} images to {oh} x {ow}")
    if oh > 1 << 15 or ow > 1 << 15 or h > 1 << 24 or w > 1 << 24:
        raise ValueError(f"resize_u8: {h} x {w} images to {oh} x {ow}: at most 2^24 input and 2^15 output pixels a side")
    _, vb, _ = clip_preprocess_tables(h, oh)
    band = RESIZE_U8_BAND
    while True:
        rows = _band_rows(vb, 0, oh, band)
        if _band_lds_bytes(rows, ow, w, False) <= CLIP_LDS_LIMIT:
            return dict(band=band, rows=max(rows, 1))
        if band == 1:
            raise ValueError(f"resize_u8: {h} x {w} images to {oh} x {ow} need {rows} rows = {_band_lds_bytes(rows, ow, w, False)} bytes: {RESIZE_U8_RULE}")
        band //= 2


def _resize_target(who, oh, ow):
    if int(oh) != oh or int(ow) != ow or oh < 1 or ow < 1:
        raise ValueError(f"{who}: the output height and width must be positive integers, got {oh} x {ow}")
    return int(oh), int(ow)


def resize_u8(images, oh, ow, out=None):
    """PIL.Image.resize((ow, oh), BICUBIC) of every image of an N x H x W x 3 CUDA batch — uint8, or float32 in [0, 1] truncated as
    (x * 255).astype(uint8) — as one uint8 CUDA tensor (N, oh, ow, 3), in one launch on the current stream (ddpo_resize_u8): Pillow's bytes
    exactly, up-scales included.  ValueError names the broken rule (RESIZE_U8_RULE for LDS)."""
    _cuda_images("resize_u8", images, any_dtype=True)          # _images_nhwc names the dtype rule
    n, h, w = _images_nhwc("resize_u8", images)
    oh, ow = _resize_target("resize_u8", oh, ow)
    geo = resize_u8_geometry(h, w, oh, ow)
    hc, hb = _clip_device_tables(("axis", w, ow), lambda: clip_preprocess_tables(w, ow)[:2], images.device)
    vc, vb = _clip_device_tables(("axis", h, oh), lambda: clip_preprocess_tables(h, oh)[:2], images.device)
    out = _out_or_empty("resize_u8", out, (n, oh, ow, 3), torch.uint8, images.device)
    _check(load().ddpo_resize_u8(_p(images), int(images.dtype == torch.float32), n, h, w, oh, ow, _p(hc), _p(hb), hc.shape[1], _p(vc), _p(vb),
                                 vc.shape[1], geo["band"], geo["rows"], _p(out), _stream()), "ddpo_resize_u8")
    return out


def resize_u8_host(images, oh, ow):
    """The same bytes computed serially on the host (ddpo_resize_u8_host) for a uint8 or float32 N x H x W x 3 numpy array: the GPU-free
    reference, held to Pillow itself."""
    import numpy as np
    a = np.asarray(images)
    n, h, w = _images_nhwc("resize_u8_host", a)
    oh, ow = _resize_target("resize_u8_host", oh, ow)
    geo = resize_u8_geometry(h, w, oh, ow)
    hc, hb, hk = clip_preprocess_tables(w, ow)
    vc, vb, vk = clip_preprocess_tables(h, oh)
    out = np.zeros((n, oh, ow, 3), dtype=np.uint8)
    _check(load().ddpo_resize_u8_host(_np_ptr(a), int(a.dtype == np.float32), n, h, w, oh, ow, _np_ptr(hc), _np_ptr(hb), hk, _np_ptr(vc),
                                      _np_ptr(vb), vk, geo["band"], _np_ptr(out)), "ddpo_resize_u8_host")
    return out


# ------------------------------------------------------------------------------------------------ symmetry rewards
SYMMETRY_MODES = {"mirror": 0, "rot180": 1}
SYMMETRY_MAX_W = 10880        # SY_MAX_W of csrc/symmetry_core.h
SYMMETRY_WIDTH_RULE = f"the width must be at most {SYMMETRY_MAX_W} pixels: a pair of rows is staged as bytes in 64 KB of LDS"


def _symmetry_mode(mode):
    if mode not in SYMMETRY_MODES:
        raise ValueError(f"symmetry_stats: mode must be one of {sorted(SYMMETRY_MODES)}, got {mode!r}")
    return SYMMETRY_MODES[mode]


def symmetry_stats_workspace_bytes(n, h, w, mode):
    nb = c_size_t(0)
    rc = load().ddpo_symmetry_stats_workspace_bytes(int(n), int(h), int(w), _symmetry_mode(mode), byref(nb))
    if rc == -1:
        raise ValueError(f"symmetry_stats: {n} images of {h} x {w}: sizes must be positive and {SYMMETRY_WIDTH_RULE}")
    _check(rc, "ddpo_symmetry_stats_workspace_bytes")
    return int(nb.value)


def symmetry_stats(images, mode, workspace=None, out=None):
    """Four exact sums per image of an N x H x W x 3 CUDA tensor — uint8, or float32 in [0, 1] truncated as (x * 255).astype(uint8) — as an
    int64 CUDA tensor (N, 4), on the current stream (ddpo_symmetry_stats).  With a a byte and b its partner under `mode` — "mirror":
    (y, W-1-x, c), "rot180": (H-1-y, W-1-x, c) —: [0] sum of ((a - b) mod 256)^2 mod 256 (what numpy's uint8 arithmetic makes of (a - b) ** 2),
    [1] sum of a, [2] sum of a^2, [3] sum of a b.  `workspace`: a uint8 CUDA tensor of at least symmetry_stats_workspace_bytes(N, H, W, mode)
    bytes; default: this stream's scratch.  ValueError names the broken rule."""
    _cuda_images("symmetry_stats", images, any_dtype=True)          # _images_nhwc names the dtype rule
    m = _symmetry_mode(mode)
    n, h, w = _images_nhwc("symmetry_stats", images)
    nb = symmetry_stats_workspace_bytes(n, h, w, mode)
    workspace = _workspace_or_scratch("symmetry_stats", workspace, nb, images.device, "symmetry_stats")
    out = _out_or_empty("symmetry_stats", out, (n, 4), torch.int64, images.device)
    _check(load().ddpo_symmetry_stats(_p(images), int(images.dtype == torch.float32), n, h, w, m, _p(out), _p(workspace), workspace.numel(),
                                      _stream()), "ddpo_symmetry_stats")
    return out


def symmetry_stats_host(images, mode):
    """The same sums computed serially on the host (ddpo_symmetry_stats_host) for a uint8 or float32 N x H x W x 3 numpy array, (N, 4) int64: the
    GPU-free reference."""
    import numpy as np
    a = np.asarray(images)
    m = _symmetry_mode(mode)
    n, h, w = _images_nhwc("symmetry_stats_host", a)
    if w > SYMMETRY_MAX_W:
        raise ValueError(f"symmetry_stats_host: {h} x {w} images: {SYMMETRY_WIDTH_RULE}")
    out = np.zeros((n, 4), dtype=np.int64)
    _check(load().ddpo_symmetry_stats_host(_np_ptr(a), int(a.dtype == np.float32), n, h, w, m, _np_ptr(out)), "ddpo_symmetry_stats_host")
    return out


def rotate4_u8(images, out=None):
    """The four right-angle turns of a square N x S x S x 3 CUDA batch — uint8, or float32 in [0, 1] truncated as (x * 255).astype(uint8) — as
    one uint8 CUDA tensor (4N, S, S, 3), on the current stream (ddpo_rotate4_u8): block k N + n is PIL.Image.rotate(90 k) of image n, k = 0..3.
    ValueError names the broken rule."""
    _cuda_images("rotate4_u8", images, any_dtype=True)          # _images_nhwc names the dtype rule
    n, s, _ = _images_nhwc("rotate4_u8", images, square=True)
    out = _out_or_empty("rotate4_u8", out, (4 * n, s, s, 3), torch.uint8, images.device)
    _check(load().ddpo_rotate4_u8(_p(images), int(images.dtype == torch.float32), n, s, s, _p(out), _stream()), "ddpo_rotate4_u8")
    return out


def rotate4_u8_host(images):
    """The same turns made serially on the host (ddpo_rotate4_u8_host) for a uint8 or float32 N x S x S x 3 numpy array: the GPU-free reference."""
    import numpy as np
    a = np.asarray(images)
    n, s, _ = _images_nhwc("rotate4_u8_host", a, square=True)
    out = np.zeros((4 * n, s, s, 3), dtype=np.uint8)
    _check(load().ddpo_rotate4_u8_host(_np_ptr(a), int(a.dtype == np.float32), n, s, s, _np_ptr(out)), "ddpo_rotate4_u8_host")
    return out


def timestep_embedding(ts, dim):
    B = ts.numel()
    out = torch.empty(B, dim, dtype=torch.float32, device=ts.device)
    _check(load().ddpo_timestep_embedding(_p(ts), _p(out), B, dim, _stream()), "ddpo_timestep_embedding")
    return out


def nchw_to_nhwc(x):
    B, C, H, W = x.shape
    out = torch.empty(B * H * W, C, dtype=torch.float32, device=x.device)
    _check(load().ddpo_nchw_to_nhwc(_p(x), _p(out), B, C, H * W, _stream()), "ddpo_nchw_to_nhwc")
    return out


def nhwc_to_nchw(x, B, C, H, W):
    out = torch.empty(B, C, H, W, dtype=torch.float32, device=x.device)
    _check(load().ddpo_nhwc_to_nchw(_p(x), _p(out), B, C, H * W, _stream()), "ddpo_nhwc_to_nchw")
    return out


def copy_cols(src, dst, col_off, rows, cols, ld_src=None, ld_dst=None):
    """dst[:, col_off:col_off+cols] = src[:, :cols] (dst/src are 2-D row-major; ld_src / ld_dst: row strides of row-strided views)."""
    ld_dst = int(ld_dst or dst.shape[1])
    dptr = c_void_p(dst.data_ptr() + 4 * col_off)
    _check(load().ddpo_copy_cols(_p_rows(src), int(ld_src or src.shape[1]), dptr, ld_dst, rows, cols, _stream()), "ddpo_copy_cols")


def stage_cfg_inputs(x, s_in, row_src=None, row_dst=None, ts_src=None, ts_dst=None):
    """s_in = [x; x] (+ optionally row_dst = row_src, ts_dst = ts_src) in one launch: the inputs of a CFG sampling step into a captured graph's
    static buffers (ddpo_stage_cfg_inputs)."""
    n = x.numel()
    if s_in.numel() != 2 * n or not x.is_contiguous() or not s_in.is_contiguous():
        raise DdpoHipError("stage_cfg_inputs: s_in must be the contiguous doubled batch of a contiguous x")
    rn = 0 if row_src is None else int(row_src.numel())
    tn = 0 if ts_src is None else int(ts_src.numel())
    if (row_src is not None and (row_dst is None or row_dst.numel() != rn or not row_src.is_contiguous())) or \
            (ts_src is not None and (ts_dst is None or ts_dst.numel() != tn or ts_src.dtype != torch.int32 or ts_dst.dtype != torch.int32
                                     or not ts_src.is_contiguous())):
        raise DdpoHipError("stage_cfg_inputs: row / timestep buffers must match (int32 timesteps, contiguous)")
    _check(load().ddpo_stage_cfg_inputs(_p(x), _p(s_in), n, None if row_src is None else _p(row_src), None if row_src is None else _p(row_dst), rn,
                                        None if ts_src is None else _p(ts_src), None if ts_src is None else _p(ts_dst), tn, _stream()),
           "ddpo_stage_cfg_inputs")


def softmax_rows_(x, scale=1.0):
    rows, cols = x.shape
    _check(load().ddpo_softmax_rows(_p(x), rows, cols, float(scale), _stream()), "ddpo_softmax_rows")
    return x


def scale_shift_clip(x, scale, shift, lo, hi):
    out = torch.empty_like(x)
    _check(load().ddpo_scale_shift_clip(_p(x), _p(out), x.numel(), float(scale), float(shift), float(lo), float(hi), _stream()),
           "ddpo_scale_shift_clip")
    return out


# ------------------------------------------------------------------------------------------------ LoRA adapters
LORA_MAX_RANK = 64


def lora_table(layers):
    """[(w0, w, A, B, s)] -> (device uint8 tensor holding the ddpo_lora_layer descriptors, n_layers, max K * N) for lora_merge.  Build it once per
    adapter store: the descriptors hold raw device pointers, so every tensor named must outlive the table."""
    arr = (LoraLayer * len(layers))()
    max_kn = 0
    for i, (w0, w, a, b, s) in enumerate(layers):
        K, N = w.shape[0], w.shape[-1]
        r = a.shape[1]
        if w0.shape != w.shape or a.shape != (K, r) or b.shape != (r, N) or N % 4 or not 1 <= r <= LORA_MAX_RANK:
            raise DdpoHipError(f"lora layer {i}: W {tuple(w.shape)}, W0 {tuple(w0.shape)}, A {tuple(a.shape)}, B {tuple(b.shape)} "
                               f"(need A (K, r), B (r, N), N % 4 == 0, 1 <= r <= {LORA_MAX_RANK})")
        for t in (w0, w, a, b):
            _f32(t)
            if not t.is_contiguous() or (t is not a and t.data_ptr() % 16):
                raise DdpoHipError("lora_table: W0, W' and B must be contiguous and 16-byte aligned, A contiguous")
        arr[i] = LoraLayer(w0.data_ptr(), w.data_ptr(), a.data_ptr(), b.data_ptr(), int(K), int(N), int(r), float(s))
        max_kn = max(max_kn, K * N)
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return host.to(layers[0][1].device), len(layers), max_kn


def lora_merge(table):
    """W' = W0 + s * A B for every layer of `table` (lora_table's result) in one launch."""
    dev, n, max_kn = table
    _check(load().ddpo_lora_merge(_p(dev), int(n), int(max_kn), _stream()), "ddpo_lora_merge")


def lora_wgrad(x, dy, A, B, dA, dB, s):
    """dA (K, r) += s * x^T (dY B^T), dB (r, N) += s * (x A)^T dY — the adapter gradients of y = x (W0 + s A B).  x: fp32 (M, K) (a row-strided view
    is taken as is) or the `Planes` a norm wrote in front of the layer (read natively, x = hi + lo: the operand the forward GEMM consumed)."""
    M, N = dy.shape
    K, r = A.shape
    for t, nm in ((dy, "dy"), (A, "A"), (B, "B"), (dA, "dA"), (dB, "dB")):
        _f32(t, nm)
    if B.shape != (r, N) or dA.shape != A.shape or dB.shape != B.shape or not 1 <= r <= LORA_MAX_RANK:
        raise DdpoHipError(f"lora_wgrad: A {tuple(A.shape)}, B {tuple(B.shape)}, dA {tuple(dA.shape)}, dB {tuple(dB.shape)}, dY {tuple(dy.shape)}")
    if isinstance(x, Planes):
        if x.fmt != 0 or x.rows != M or x.C != K:
            raise DdpoHipError("lora_wgrad: the planes must be bf16 hi / lo planes of shape (M, K)")
        xp, ldx, hi, lo, ldp = None, 0, _p(x.hi), _p(x.lo), x.ld
    else:
        _f32(x, "x")
        if tuple(x.shape) != (M, K):
            raise DdpoHipError(f"lora_wgrad: x {tuple(x.shape)} vs dY {tuple(dy.shape)} and A {tuple(A.shape)}")
        ldx = int(x.stride(0)) if M > 1 else K
        xp, hi, lo, ldp = _p_rows(x), None, None, 0
    lddy = int(dy.stride(0)) if M > 1 else N
    nb = int(load().ddpo_lora_wgrad_ws_bytes(M, K, N, r))
    ws = _scratch(nb, dy.device, "lora")
    _check(load().ddpo_lora_wgrad(xp, ldx, hi, lo, int(ldp), _p_rows(dy), lddy, _p(A), _p(B), _p(dA), _p(dB), int(M), int(K), int(N), int(r),
                                  float(s), _p(ws), ws.numel(), _stream()), "ddpo_lora_wgrad")
    return dA, dB
