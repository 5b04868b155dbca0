"""CPU-side ABI checks of the two period parameters behind the CFG-shared U-Net front (no device work: every call below is rejected by the
host-side argument checks before anything is launched).

What these can and cannot show: without a device there is no positive control — a call with a VALID period would launch — so `== -1` here
says that a bad period never gets past the entry point, not that the period check is the one that fired.  The descriptors and argument lists
are otherwise the ones that succeed on the GPU: tests/test_gpu_cfg_shared_front.py::test_invalid_periods_are_rejected makes the same calls
with valid and invalid periods on real buffers, and that is where the check itself is proven."""
import ctypes
import os
import re

import pytest

from ddpo_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 16-byte aligned non-NULL "device pointer": never dereferenced on the DDPO_EINVAL paths


def test_res_rows_is_the_trailing_field_of_the_descriptor():
    assert L.GemmDesc._fields_[-1] == ("res_rows", ctypes.c_int)
    assert L.load().ddpo_sizeof_gemm_desc() == ctypes.sizeof(L.GemmDesc)
    hdr = open(os.path.join(ROOT, "include", "ddpo_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", hdr[:hdr.index("} ddpo_gemm_desc;")], flags=re.S)
    assert body.rstrip().endswith("int res_rows;")
    assert L.GemmDesc().res_rows == 0               # a zeroed descriptor keeps the one-residual-row-per-output-row behaviour


def test_shared_query_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ddpo_hip.h")).read()
    for name in ("ddpo_attention_fwd", "ddpo_attention_fwd_x16", "ddpo_attention_fwd_images"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in L.EXPORTED_SYMBOLS and hasattr(L.load(), name)


def _desc(M, res_rows, residual=FAKE):
    d = L.GemmDesc()
    d.src, d.w, d.out, d.residual = FAKE, FAKE, FAKE, residual
    d.ld_src, d.ld_out, d.ld_res, d.alpha = 64, 64, 64, 1.0
    d.M, d.N, d.K = M, 64, 64
    d.res_rows = res_rows
    return d


@pytest.mark.parametrize("res_rows,residual", [(3, FAKE), (-128, FAKE), (512, FAKE), (100, FAKE), (128, None)])
def test_invalid_residual_period_is_einval(res_rows, residual):
    lib = L.load()
    d = _desc(256, res_rows, residual)
    assert lib.ddpo_gemm_conv_fwd(ctypes.byref(d), None) == -1
    assert lib.ddpo_gemm_conv_fwd_bf16(ctypes.byref(d), FAKE, FAKE, 64, 3, None, 0, None) == -1
    assert lib.ddpo_gemm_conv_fwd_bf16_planes(ctypes.byref(d), FAKE, FAKE, 64, FAKE, FAKE, 64, None, 0, None) == -1
    d.w_layout, d.w_scale = 1, FAKE
    assert lib.ddpo_gemm_conv_fwd_f16mx_planes(ctypes.byref(d), FAKE, FAKE, 64, FAKE, FAKE, None, 0, None) == -1


def test_residual_period_is_rejected_where_it_has_no_meaning():
    lib = L.load()
    d = _desc(256, 128)
    d.ld_w = 64
    assert lib.ddpo_gemm_conv_wgrad(ctypes.byref(d), None) == -1
    assert lib.ddpo_gemm_conv_wgrad_bf16x3(ctypes.byref(d), None) == -1


@pytest.mark.parametrize("q_batches", [0, -1, 3, 5, 8])
def test_invalid_query_period_is_einval(q_batches):
    lib = L.load()
    B, heads, Nq, Nk, d = 4, 2, 64, 77, 40
    C = heads * d
    assert lib.ddpo_attention_fwd(FAKE, C, q_batches, FAKE, C, FAKE, C, FAKE, C, None, B, heads, Nq, Nk, d, 1.0, None) == -1
    for f16p in (0, 1):
        assert lib.ddpo_attention_fwd_x16(f16p, FAKE, C, q_batches, FAKE, C, FAKE, C, FAKE, C, None, None, 0, None, B, heads, Nq, Nk, d,
                                          1.0, None, 0, None) == -1
        nb = lib.ddpo_attention_kv_images_bytes(B, heads, Nk, d)
        assert lib.ddpo_attention_fwd_images(f16p, FAKE, C, q_batches, FAKE, nb, FAKE, C, None, None, 0, None, B, heads, Nq, Nk, d, 1.0,
                                             None) == -1


def test_shared_query_output_forms_are_exclusive():
    lib = L.load()
    B, heads, Nq, Nk, d = 4, 2, 64, 77, 40
    C = heads * d
    # fp32 rows AND planes at once, or neither
    assert lib.ddpo_attention_fwd_x16(0, FAKE, C, 2, FAKE, C, FAKE, C, FAKE, C, FAKE, FAKE, C, None, B, heads, Nq, Nk, d, 1.0, None, 0, None) == -1
    assert lib.ddpo_attention_fwd_x16(0, FAKE, C, 2, FAKE, C, FAKE, C, None, C, None, None, 0, None, B, heads, Nq, Nk, d, 1.0, None, 0, None) == -1
