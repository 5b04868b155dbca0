"""Every kernel, loader, operand form and split edge of the bf16x3 weight gradient (ddpo_amd/csrc/gemm_bf16_wgrad.hip), each at the SMALLEST shape
that enters it, against float64.  The file holds two kernels (128 x 128 and the wide 128 x 320), two loaders (row / per-pixel) and four operand
forms: 12 instantiations chosen by the host rule in wgrad_bf16x3().  The neighbouring tests (test_gpu_bf16.py, test_gpu_planes.py) run a handful
of layer shapes from dw = zeros in a tight buffer: one fp32-fed case on the wide kernel, no plane operand there, no k-blocked plane on it, no
`nk` < 4 on the row loader, no explicit split, no alpha, no column slices, no colsum under an N tail.

The shape tables come first; beside each row stands the branch it enters and, as the last tuple, what the dispatch rule makes of it:
(kernel, loader, splits, nk of the first split, nk of the last split, valid rows of a ragged last K tile, valid columns of a ragged last N tile).
`test_wgrad_tables_enter_the_branches_they_name` (CPU) re-derives those tuples from the rule, with the rule's constants read out of the .hip file;
`test_wgrad_gates_see_the_named_defects` (CPU) shows that the gates below are far under what a dropped k-tile, an unmasked border row, a missing
pixel-pair half, a dropped colsum quad or a write to row K would cost.

Every GPU case accumulates into a running gradient g0 of O(1) that lives inside a larger buffer with SENTINEL floats on either side (bit-identical
afterwards), and is held to the project's gates (tests/test_gpu_bf16.py, tests/test_gpu_planes.py):
    max|dw - g0 - alpha * ref| / max|ref|  < 5e-5        max|db - db0 - ref_db| / max|ref_db|  < 2e-6
    a plane form against the fp32 form of the same row:  max|got - ref| <= 2e-6 * max|ref| + 1e-7
Worst values measured on an MI355X, per table (dw against its 5e-5 / db against its 2e-6 / plane form vs fp32 form as a fraction of its bound):
    ROWS       dw 5.8e-6 (conv 1 x 1 x 64, fp32)          -                      0.02 of the bound
    PIXEL      dw 7.6e-6 (dense M = 4)                    -                      0.04
    WIDE_MISS  dw 4.6e-6                                  -                      0.10
    WIDE       dw 4.9e-6 (conv 4 x 64 x 64, dY planes)    db 3.9e-7 (dense)      0.14
    COLSUM     dw 6.9e-6                                  db 1.0e-7 (N = 32)     -        (db at M = 4, sums of four terms: 5.0e-8)
    COLSUM with plane dY (ddpo_colsum_accum): 8.2e-8 of the float64 sum of the decoded planes; 2.1e-6 (M = 64) and 3.2e-6 (M = 33) of the float64
    sum of dY itself — the planes' own 2^-16 rounding, over the 2e-6 that was set for fp32 dY: that comparison is held to the number format's
    bound instead (test_wgrad_dbias_with_plane_dy_goes_through_colsum_accum).  No row found a defect in the kernels or in lib.gemm_wgrad's routing.
"""
import functools
import os
import re
import zlib
from ctypes import byref

import numpy as np
import pytest
import torch

from ddpo_amd import lib as L

gpu = pytest.mark.gpu
DEV = "cuda"
DW_GATE, DB_GATE, FORM_REL, FORM_ABS = 5e-5, 2e-6, 2e-6, 1e-7
SENTINEL = 256          # floats in front of and behind dw / dbias inside their buffers
LD_PAD = 32             # extra columns of the wider tensor a column-slice operand is cut from


# ------------------------------------------------------------------------------------------------ shape tables
def _dense(M, K, N):
    return ("dense", M, K, N)


def _conv(B, H, W, Cin=64, Cout=64, ks=3, stride=1, ups=False):
    return ("conv", B, H, W, Cin, Cout, ks, stride, ups)


def _row(geom, expect, **opts):
    """opts: splits (explicit ddpo_gemm_desc.splits), alpha, ld (operands are column slices of tensors LD_PAD columns wider)."""
    return (geom, tuple(sorted(opts.items())), expect)


# 1. the wide 128 x 320 kernel: rows_ok && N == 320 && K >= 2560 && M >= 16384 && splits <= 0 (one 320-column tile; 256 slots, 3 rounds)
WIDE = [
    _row(_dense(16384, 2560, 320), ("wide", "rows", 37, 14, 8, 0, 0)),          # every threshold at its minimum, no K tail; even nk, last split shorter (even)
    _row(_dense(16384 + 32, 2564, 320), ("wide", "rows", 12, 43, 40, 4, 0)),    # 21st K tile holds 4 rows; odd nk (odd `step` tail), last split shorter (even)
    _row(_conv(4, 64, 64, 288, 320), ("wide", "rows", 12, 43, 39, 32, 0)),      # K = 2592: 32-row K tail, taps change inside a 128-row tile (288 % 128); OW = 64, splits start mid-row
    _row(_conv(64, 16, 16, 288, 320), ("wide", "rows", 12, 43, 39, 32, 0)),     # OW < 32: two image rows per k-tile
    _row(_conv(16, 32, 32, 288, 320), ("wide", "rows", 12, 43, 39, 32, 0)),     # OW == 32: one image row per k-tile
    _row(_conv(4, 32, 128, 288, 320), ("wide", "rows", 12, 43, 39, 32, 0)),     # OW = 128: four k-tiles per image row
]
# near misses of the wide rule: the 128 x 128 kernel with the row loader (three 128-column tiles, the last with 64 columns)
WIDE_MISS = [
    _row(_dense(16352, 2560, 320), ("128", "rows", 17, 31, 15, 0, 64)),                  # M one k-tile under 16384
    _row(_dense(16384, 2556, 320), ("128", "rows", 17, 31, 16, 124, 64)),                # K one quad under 2560
    _row(_dense(16384, 2560, 320), ("128", "rows", 8, 64, 64, 0, 64), splits=8),         # an explicit split
]
# 2. the 128 x 128 kernel with the row loader at its smallest sizes
ROWS = [
    _row(_dense(32, 64, 32), ("128", "rows", 1, 1, 1, 64, 32)),                 # nk = 1: prologue only
    _row(_dense(64, 64, 32), ("128", "rows", 1, 2, 2, 64, 32)),                 # nk = 2
    _row(_dense(96, 64, 32), ("128", "rows", 1, 3, 3, 64, 32)),                 # nk = 3: both LDS stages reused
    _row(_dense(64, 132, 32), ("128", "rows", 1, 2, 2, 4, 32)),                 # one valid quad in the second K tile
    _row(_dense(64, 64, 132), ("128", "rows", 1, 2, 2, 64, 4)),                 # one valid quad in the second N tile
    _row(_conv(2, 8, 4), ("128", "rows", 1, 2, 2, 64, 64)),                     # OW = 4: eight image rows per k-tile (a k-tile is one whole image)
    _row(_conv(1, 4, 8), ("128", "rows", 1, 1, 1, 64, 64)),                     # OW = 8: four image rows per k-tile
    _row(_conv(2, 16, 16), ("128", "rows", 2, 8, 8, 64, 64)),                   # OW = 16; two splits, one per image
    _row(_conv(1, 2, 32), ("128", "rows", 1, 2, 2, 64, 64)),                    # OW = 32
    _row(_conv(1, 1, 64), ("128", "rows", 1, 2, 2, 64, 64)),                    # OW = 64, one image row: every vertical tap is masked
    _row(_conv(1, 2, 64), ("128", "rows", 1, 4, 4, 64, 64)),                    # OW = 64, two image rows
    _row(_conv(2, 8, 8, ks=1), ("128", "rows", 1, 4, 4, 64, 64)),               # 1x1: no guard offset, no mask
    _row(_dense(64, 64, 32), ("128", "rows", 1, 2, 2, 64, 32), ld=True),        # ld_src = K + 32, ld_dy = N + 32 (dense)
    _row(_conv(2, 16, 16), ("128", "rows", 2, 8, 8, 64, 64), ld=True),          # ld_src = Cin + 32, ld_dy = N + 32 (3x3: tap offsets and the guard scale with ld_src)
    _row(_dense(96, 64, 32), ("128", "rows", 1, 3, 3, 64, 32), alpha=0.5),      # alpha != 1
    _row(_dense(96, 64, 32), ("128", "rows", 1, 3, 3, 64, 32), splits=1),       # explicit splits = 1
    _row(_dense(96, 64, 32), ("128", "rows", 2, 2, 1, 64, 32), splits=2),       # explicit splits = 2: the last split is shorter
    _row(_dense(96, 64, 32), ("128", "rows", 3, 1, 1, 64, 32), splits=5),       # splits above M / 32 = 3: pixels_per_split() brings it down to 3
]
# 3. the 128 x 128 kernel with the per-pixel loader
PIXEL = [
    _row(_dense(4, 64, 32), ("128", "pixel", 1, 1, 1, 64, 32)),                 # M < 32: pixel pairs 2 .. 15 are past m_end
    _row(_dense(31, 64, 32), ("128", "pixel", 1, 1, 1, 64, 32)),                # odd M: the second pixel of the last pair is past m_end
    _row(_dense(33, 64, 32), ("128", "pixel", 1, 2, 2, 64, 32)),                # a second k-tile that holds one pixel
    _row(_dense(63, 64, 32), ("128", "pixel", 1, 2, 2, 64, 32)),                # odd M in the second k-tile
    _row(_conv(2, 8, 6), ("128", "pixel", 1, 3, 3, 64, 64)),                    # OW = 6: M % 32 == 0, but rows do not tile into k-tiles
    _row(_conv(2, 8, 10), ("128", "pixel", 1, 5, 5, 64, 64)),                   # OW = 10
    _row(_conv(2, 4, 12), ("128", "pixel", 1, 3, 3, 64, 64)),                   # OW = 12
    _row(_conv(2, 4, 20), ("128", "pixel", 1, 5, 5, 64, 64)),                   # OW = 20
    _row(_conv(4, 3, 8), ("128", "pixel", 1, 3, 3, 64, 64)),                    # OW = 8 divides 32 but OH * OW = 24 does not: k-tiles straddle images
    _row(_conv(2, 16, 16, stride=2), ("128", "pixel", 1, 4, 4, 64, 64)),        # stride 2, even source: OH = OW = 8
    _row(_conv(1, 7, 9, stride=2), ("128", "pixel", 1, 1, 1, 64, 64)),          # stride 2, odd source: OH = 4, OW = 5, M = 20
    _row(_conv(2, 8, 8, ks=1, stride=2), ("128", "pixel", 1, 1, 1, 64, 64)),    # 1x1 stride 2 (M = 32: not `simple`, so not the row loader)
    _row(_conv(2, 6, 10, ups=True), ("128", "pixel", 2, 8, 7, 64, 64)),         # nearest-2x upsample, OW = 20; two splits, the last shorter
    _row(_conv(1, 4, 4, ups=True), ("128", "pixel", 1, 2, 2, 64, 64)),          # nearest-2x upsample, OW = 8, M = 64
]
# 4. every row above runs in each of these operand forms; "kb" = both operands as k-blocked planes (plane row stride 0, lib.A_KBLOCKED)
FORMS = ["fp32", "a", "dy", "both", "kb"]
FORM_PLANES = {"fp32": (False, False), "a": (True, False), "dy": (False, True), "both": (True, True), "kb": (True, True)}
# 5. the fused bias gradient (ddpo_gemm_desc.colsum, fp32 dY); the WIDE rows carry a dbias too in their fp32-dY forms
COLSUM = [
    _row(_dense(64, 64, 32), ("128", "rows", 1, 2, 2, 64, 32)),                 # N = 32: waves 1-3 hold no valid column
    _row(_dense(64, 64, 36), ("128", "rows", 1, 2, 2, 64, 36)),                 # N tail: one quad of wave 1
    _row(_dense(64, 64, 132), ("128", "rows", 1, 2, 2, 64, 4)),                 # N tail in the second N tile
    _row(_dense(64, 64, 320), ("128", "rows", 1, 2, 2, 64, 64)),                # three N tiles, the last half full
    _row(_dense(96, 64, 36), ("128", "rows", 3, 1, 1, 64, 36), splits=3),       # three splits add into the same dbias
    _row(_dense(64, 256, 36), ("128", "rows", 1, 2, 2, 0, 36)),                 # two K tiles: only tile_m == 0 adds the sums
    _row(_dense(33, 64, 36), ("128", "pixel", 1, 2, 2, 64, 36)),                # per-pixel loader: the pixels past m_end add zeros
    _row(_conv(1, 7, 9, stride=2), ("128", "pixel", 1, 1, 1, 64, 64)),          # ... of a strided convolution
    _row(_dense(4, 64, 32), ("128", "pixel", 1, 1, 1, 64, 32)),                 # sums of four terms: db = fl(db0 + s) is half an ulp of ~4 off, 1e-7 of max|ref_db| ~ 4
]
COLSUM_PLANE_DY = [_dense(64, 64, 36), _dense(33, 64, 36)]                       # plane dY with a dbias: lib.gemm_wgrad routes it to ddpo_colsum_accum
# 6. descriptors the C entry points must refuse (-1) without touching `out`: test_wgrad_entry_points_refuse_*
EINVAL = ["colsum_with_plane_dy", "ld_src_0_fp32", "ld_w_0_ragged_n", "hi_without_lo", "k_not_quad", "pad_not_half", "upsample_2", "stride_3", "res_rows",
          "plane_misaligned_2_bytes", "planes_entry_without_planes"]

KB_MIXED = {_dense(64, 132, 32), _dense(64, 64, 132), _dense(16384 + 32, 2564, 320), _dense(16384, 2556, 320)}       # K or N not whole 32-blocks
TABLES = {"rows": ROWS, "pixel": PIXEL, "wide_miss": WIDE_MISS, "wide": WIDE, "colsum": COLSUM}


def _id(row):
    geom, opts, _ = row
    return "-".join(str(int(v) if isinstance(v, bool) else v) for v in geom) + "".join(f"-{k}{v}" for k, v in opts)


# ------------------------------------------------------------------------------------------------ the dispatch rule, restated
def _geometry(geom):
    """M, N, K, channels per tap and lib's conv dict (None: dense) of a table geometry."""
    if geom[0] == "dense":
        _, M, K, N = geom
        return M, N, K, K, None
    _, B, H, W, Cin, Cout, ks, stride, ups = geom
    conv = L._conv_geom(B, H, W, Cin, ks, stride, None, ups)
    return B * conv["OH"] * conv["OW"], Cout, ks * ks * Cin, Cin, conv


def _rule_constants():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ddpo_amd", "csrc", "gemm_bf16_wgrad.hip")).read()
    flat = " ".join(src.split())
    wide = re.search(r"const bool wide = rows_ok && d\.N == (\d+) && d\.K >= (\d+) && d\.M >= (\d+) && d\.splits <= 0;", flat)
    split = re.search(r"d\.splits > 0 \? d\.splits : \(wide \? best_split\(tiles, d\.M, (\d+), (\d+), ([\d.]+)\) : best_split\(tiles, d\.M, (\d+), (\d+), ([\d.]+)\)\)", flat)
    tiles = re.search(r"const int tiles_n = wide \? d\.N / (\d+) : \(d\.N \+ 127\) / (\d+), tiles = \(\(d\.K \+ 127\) / (\d+)\) \* tiles_n;", flat)
    cap = re.search(r"const int max_splits = \(M \+ 255\) / (\d+);", flat)
    assert wide and split and tiles and cap, "the host rule of wgrad_bf16x3() is no longer spelled as this test restates it"
    # the loader rule and the two helpers, as text: an edit there must be mirrored in _dispatch() below
    for text in ("const bool simple_ = !conv_ || (d.stride == 1 && d.upsample == 0 && d.OH == d.H && d.OW == d.W);",
                 "const bool rows_ok = simple_ && (d.M % 32) == 0 && a_bytes + (conv_ ? (int64_t)(d.W + 1) * lda_b * 4 : 0) < 0x7FFFFFF0ll && b_bytes < 0x7FFFFFF0ll && "
                 "(!conv_ || (((d.OW % 32) == 0 || (32 % d.OW) == 0) && ((d.OH * d.OW) % 32) == 0));",
                 "int cand = (slots * r) / tiles; if (cand > max_splits) cand = max_splits; if (cand < 1) cand = 1;",
                 "const double eff = (double)wgs / (double)(((wgs + slots - 1) / slots) * slots); if (eff > best_eff + margin || best_eff == 0.0) { best_eff = eff; best = cand; }",
                 "int mps = (M + splits - 1) / splits; mps = (mps + 31) / 32 * 32; splits = (M + mps - 1) / mps;"):
        assert text in flat, text
    return dict(wide_n=int(wide.group(1)), wide_k=int(wide.group(2)), wide_m=int(wide.group(3)),
                wide_split=(int(split.group(1)), int(split.group(2)), float(split.group(3))),
                split=(int(split.group(4)), int(split.group(5)), float(split.group(6))),
                wide_bn=int(tiles.group(1)), bn=int(tiles.group(2)), bm=int(tiles.group(3)), px_per_split=int(cap.group(1)))


_TODAY = dict(wide_n=320, wide_k=2560, wide_m=16384, wide_split=(256, 3, 0.04), split=(512, 4, 0.03), wide_bn=320, bn=128, bm=128, px_per_split=256)


def _best_split(tiles, M, slots, rounds, margin, px_per_split):
    max_splits = (M + 255) // px_per_split
    best, best_eff = 1, 0.0
    for r in range(1, rounds + 1):
        cand = max(1, min(slots * r // tiles, max_splits))
        wgs = tiles * cand
        eff = wgs / (-(-wgs // slots) * slots)
        if eff > best_eff + margin or best_eff == 0.0:
            best_eff, best = eff, cand
    return best


def _dispatch(row, c=_TODAY, a_planes=False, b_planes=False):
    geom, opts, _ = row
    M, N, K, Cin, conv = _geometry(geom)
    opts = dict(opts)
    splits_arg = opts.get("splits", 0)
    lda, ldb = Cin + (LD_PAD if opts.get("ld") else 0), N + (LD_PAD if opts.get("ld") else 0)
    simple = conv is None or (conv["stride"] == 1 and conv["upsample"] == 0 and conv["OH"] == conv["H"] and conv["OW"] == conv["W"])
    a_bytes, b_bytes = M * lda * (2 if a_planes else 4), M * ldb * (2 if b_planes else 4)
    rows_ok = (simple and M % 32 == 0 and a_bytes + ((conv["W"] + 1) * lda * 4 if conv else 0) < 0x7FFFFFF0 and b_bytes < 0x7FFFFFF0 and
               (conv is None or ((conv["OW"] % 32 == 0 or 32 % conv["OW"] == 0) and (conv["OH"] * conv["OW"]) % 32 == 0)))
    wide = rows_ok and N == c["wide_n"] and K >= c["wide_k"] and M >= c["wide_m"] and splits_arg <= 0
    bn = c["wide_bn"] if wide else c["bn"]
    tiles = -(-K // c["bm"]) * (N // bn if wide else -(-N // bn))
    splits = splits_arg if splits_arg > 0 else _best_split(tiles, M, *(c["wide_split"] if wide else c["split"]), c["px_per_split"])
    mps = -(-(-(-M // splits)) // 32) * 32
    splits = -(-M // mps)
    return ("wide" if wide else "128", "rows" if rows_ok else "pixel", splits, -(-min(mps, M) // 32), -(-(M - (splits - 1) * mps) // 32), K % c["bm"], N % bn)


def test_wgrad_tables_enter_the_branches_they_name():
    """The tuple beside each row is what wgrad_bf16x3()'s rule gives, with the rule's constants read from the source; the tables hold the edges
    their comments name and reach all 12 instantiations.  IF YOU CHANGE THE RULE (rows_ok, wide, best_split, pixels_per_split): mirror it in
    _dispatch() and move the rows so that each still enters the branch its comment names at the smallest such shape."""
    c = _rule_constants()
    assert c == _TODAY, c
    every = [r for t in TABLES.values() for r in t]
    for row in every:
        got = _dispatch(row, c)
        assert got == row[2], (_id(row), got)
        M, N, K, Cin, conv = _geometry(row[0])
        assert K >= 64 and N >= 32 and K % 4 == 0 and N % 4 == 0                      # lib.gemm_wgrad's `fast` rule and the kernels' quads
    # the "kb" form stores an operand k-blocked when its channel count is whole 32-blocks (lib.Planes); these rows keep ONE operand row-major in it
    assert {r[0] for r in WIDE + WIDE_MISS + ROWS + PIXEL if _geometry(r[0])[3] % 32 or _geometry(r[0])[1] % 32} == KB_MIXED
    # the wide table: all on the wide kernel, all thresholds met at their minimum by the first row, and the pipeline's parities
    assert all(r[2][0] == "wide" for r in WIDE) and all(r[2][:2] == ("128", "rows") for r in WIDE_MISS)
    assert _geometry(WIDE[0][0])[:3] == (c["wide_m"], c["wide_n"], c["wide_k"])
    nks = {nk for r in WIDE for nk in r[2][3:5]}
    assert any(nk % 2 for nk in nks) and any(nk % 2 == 0 for nk in nks), nks          # the odd / even `step` tail
    assert any(r[2][4] < r[2][3] for r in WIDE)                                       # a last split shorter than the rest
    assert min(nks) >= 3                                                              # the prologue's load_tile(1), load_tile(2) are real tiles everywhere (the rule cannot go lower)
    assert {r[2][5] for r in WIDE} == {0, 4, 32}
    assert {_geometry(r[0])[4]["OW"] for r in WIDE if r[0][0] == "conv"} == {16, 32, 64, 128}
    assert all(_geometry(r[0])[3] % c["bm"] for r in WIDE if r[0][0] == "conv")       # taps change inside a 128-row tile
    # the row loader: nk 1 / 2 / 3, the quad tails, every OW class, ld / alpha / splits rows
    assert all(r[2][:2] == ("128", "rows") for r in ROWS)
    assert {1, 2, 3} <= {r[2][3] for r in ROWS} and 4 in {r[2][5] for r in ROWS} and 4 in {r[2][6] for r in ROWS}
    assert {_geometry(r[0])[4]["OW"] for r in ROWS if r[0][0] == "conv" and r[0][6] == 3} == {4, 8, 16, 32, 64}
    assert {dict(r[1]).get("splits") for r in ROWS} == {None, 1, 2, 5} and any(dict(r[1]).get("ld") for r in ROWS) and any(dict(r[1]).get("alpha") for r in ROWS)
    # the per-pixel loader
    assert all(r[2][:2] == ("128", "pixel") for r in PIXEL)
    assert {_geometry(r[0])[0] for r in PIXEL if r[0][0] == "dense"} == {4, 31, 33, 63}
    assert {6, 10, 12, 20} <= {_geometry(r[0])[4]["OW"] for r in PIXEL if r[0][0] == "conv"}
    assert {(r[0][6], r[0][7], r[0][8]) for r in PIXEL if r[0][0] == "conv"} == {(3, 1, False), (3, 2, False), (1, 2, False), (3, 1, True)}
    # colsum
    assert {_geometry(r[0])[1] for r in COLSUM} >= {32, 36, 132, 320} and any(dict(r[1]).get("splits") == 3 for r in COLSUM)
    assert any(_geometry(r[0])[2] >= 2 * c["bm"] for r in COLSUM)
    # all 12 instantiations: gemm_wgrad_bf16_kernel<A, B, ROWL> and gemm_wgrad_bf16_wide_kernel<A, B>
    reached = {(r[2][0], r[2][1]) + FORM_PLANES[f] for r in WIDE + WIDE_MISS + ROWS + PIXEL for f in FORMS}
    assert reached == {(k, l, a, b) for k, l in (("128", "rows"), ("128", "pixel"), ("wide", "rows")) for a in (False, True) for b in (False, True)}
    for row in WIDE + ROWS + PIXEL + WIDE_MISS:                                        # plane operands change no branch at these sizes
        assert _dispatch(row, c, True, True) == row[2]


# ------------------------------------------------------------------------------------------------ float64 references
def _conv_taps(x, B, H, W, Cin, ks, stride, ups):
    """(M, Cin) matrices, one per tap in (ky, kx) order: the shifted / strided slice of the zero-padded (nearest-2x repeated) input."""
    pad = ks // 2
    img = x.reshape(B, H, W, Cin)
    if ups:
        img = img.repeat_interleave(2, 1).repeat_interleave(2, 2)
    VH, VW = img.shape[1], img.shape[2]
    OH, OW = (VH + 2 * pad - ks) // stride + 1, (VW + 2 * pad - ks) // stride + 1
    padded = torch.zeros(B, VH + 2 * pad, VW + 2 * pad, Cin, dtype=img.dtype, device=img.device)
    padded[:, pad:pad + VH, pad:pad + VW] = img
    return [padded[:, ky:ky + stride * (OH - 1) + 1:stride, kx:kx + stride * (OW - 1) + 1:stride].reshape(B * OH * OW, Cin)
            for ky in range(ks) for kx in range(ks)]


def _on_device(geom):
    M, N, K, _, _ = _geometry(geom)
    return M * K * N > 1 << 30          # the wide geometries: 13 GMAC of float64 is slow on the host and instant on the device


@functools.lru_cache(maxsize=4)
def _inputs(geom):
    """x (source rows, Cin) and dY (M, N), fp32 on the device, randn from a seed of the geometry."""
    M, N, K, Cin, conv = _geometry(geom)
    g = torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(geom).encode()))
    rows = conv["B"] * conv["H"] * conv["W"] if conv else M
    return torch.randn(rows, Cin, device=DEV, generator=g), torch.randn(M, N, device=DEV, generator=g)


@functools.lru_cache(maxsize=None)
def _reference(geom):
    """float64 dW = A^T dY as (K, N) and db = column sums of dY; on the host but for the wide geometries.  Never modified."""
    x, dy = _inputs(geom)
    if not _on_device(geom):
        x, dy = x.cpu(), dy.cpu()
    x, dy = x.double(), dy.double()
    if geom[0] == "dense":
        dw = x.t() @ dy
    else:
        dw = torch.cat([a.t() @ dy for a in _conv_taps(x, *geom[1:5], *geom[6:9])], 0)
    return dw, dy.sum(0)


@functools.lru_cache(maxsize=None)
def _running(n, seed):
    return torch.randn(n + 2 * SENTINEL, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _sentinels_intact(before, after):
    """The SENTINEL words on either side of the payload are bit-identical (numpy or torch, fp32)."""
    ends = lambda t: torch.cat([t[:SENTINEL], t[-SENTINEL:]]).cpu().numpy() if torch.is_tensor(t) else np.asarray(t, dtype=np.float32)
    b, a = (ends(t).view(np.int32) for t in (before, after))
    return bool(np.array_equal(b[:SENTINEL], a[:SENTINEL]) and np.array_equal(b[-SENTINEL:], a[-SENTINEL:]))


def _operand(t, planes, ld, kblocked, monkeypatch):
    """The tensor as the form wants it: (operand, explicit row stride or None).  `ld`: a column slice of a tensor LD_PAD columns wider — columns
    LD_PAD.. of it for fp32; for planes the first columns of the wider planes (a plane pointer is the start of its buffer).  The other columns
    hold O(1) noise.  k-blocked planes have no row stride: that form runs on the compact tensor."""
    rows, C = t.shape
    if planes:
        monkeypatch.setattr(L, "A_KBLOCKED", bool(kblocked))
    if not ld or (planes and kblocked):
        return (L.split_planes(t) if planes else t), None
    noise = torch.randn(rows, LD_PAD, device=DEV, generator=torch.Generator(device=DEV).manual_seed(rows + C))
    if planes:
        return L.split_planes(torch.cat([t, noise], 1)), C + LD_PAD
    return torch.cat([noise, t], 1)[:, LD_PAD:], C + LD_PAD


def _launch(row, form, monkeypatch, with_db):
    """One call on the bf16x3 datapath into a running gradient inside a sentinel-fenced buffer.  Returns (dw buffer before, after, db before, after)."""
    geom, opts, _ = row
    opts = dict(opts)
    M, N, K, Cin, conv = _geometry(geom)
    L.DATAPATH = "bf16x3"
    x, dy = _inputs(geom)
    a_pl, b_pl = FORM_PLANES[form]
    a, ld_src = _operand(x, a_pl, opts.get("ld"), form == "kb", monkeypatch)
    b, ld_dy = _operand(dy, b_pl, opts.get("ld"), form == "kb", monkeypatch)
    if form == "kb":
        assert a.kblocked == (Cin % 32 == 0) and b.kblocked == (N % 32 == 0) and (a.kblocked or b.kblocked)
        assert a.ld == (0 if a.kblocked else Cin) and b.ld == (0 if b.kblocked else N)
    seed = zlib.crc32(_id(row).encode())
    buf0, dbuf0 = _running(K * N, seed), _running(N, seed + 1)
    buf, dbuf = buf0.clone(), dbuf0.clone()
    dw = buf[SENTINEL:SENTINEL + K * N].view(K, N)
    db = dbuf[SENTINEL:SENTINEL + N] if with_db else None
    if opts:
        L.gemm_wgrad(a, b, dw, M=M, N=N, K=K, conv=conv, ld_src=ld_src, ld_dy=ld_dy, splits=opts.get("splits", 0), alpha=opts.get("alpha", 1.0), dbias=db)
    elif conv is None:
        L.linear_wgrad(a, b, dw, dbias=db)
    else:
        L.conv2d_wgrad(a, b, dw, conv["B"], conv["H"], conv["W"], Cin, N, conv["ksize"], stride=conv["stride"], upsample=bool(conv["upsample"]), dbias=db)
    torch.cuda.synchronize()
    return buf0, buf, dbuf0, dbuf


def _payload(buf):
    return buf[SENTINEL:-SENTINEL]


@functools.lru_cache(maxsize=None)
def _fp32_form_result(table, index):
    """dw of the row's fp32 / fp32 form (from the same running gradient): what the plane forms of the row are compared with."""
    return _payload(_launch(TABLES[table][index], "fp32", None, False)[1]).clone()          # (no plane operand: nothing to patch)


def _check_row(table, index, form, monkeypatch, with_db):
    row = TABLES[table][index]
    geom, opts, expect = row
    alpha = dict(opts).get("alpha", 1.0)
    ref_dw, ref_db = _reference(geom)
    buf0, buf, dbuf0, dbuf = _launch(row, form, monkeypatch, with_db)
    assert _sentinels_intact(buf0, buf), "a write outside dw"
    assert _sentinels_intact(dbuf0, dbuf), "a write outside dbias"
    to = (lambda t: t.double()) if _on_device(geom) else (lambda t: t.cpu().double())
    e_dw = float(((to(_payload(buf)) - to(_payload(buf0))).view_as(ref_dw) - alpha * ref_dw).abs().max() / ref_dw.abs().max())
    line = f"{table} {_id(row)} [{form}] {expect[0]}/{expect[1]} splits {expect[2]} nk {expect[3]}/{expect[4]}: dw {e_dw:.2e} (gate {DW_GATE:.0e})"
    e_db = None
    if with_db:
        e_db = float((to(_payload(dbuf)) - to(_payload(dbuf0)) - ref_db).abs().max() / ref_db.abs().max())
        line += f"; db {e_db:.2e} (gate {DB_GATE:.0e})"
    else:
        assert torch.equal(dbuf, dbuf0)
    e_form = None
    if form != "fp32":
        base = _fp32_form_result(table, index)
        e_form = float((_payload(buf) - base).abs().max())
        bound = FORM_REL * float(base.abs().max()) + FORM_ABS
        line += f"; vs fp32 form {e_form:.2e} (bound {bound:.2e}, x{e_form / bound:.3f})"
    from conftest import parity_record
    parity_record("[wgrad branches] " + line)
    assert e_dw < DW_GATE, e_dw
    if with_db:
        assert e_db < DB_GATE, e_db
    if e_form is not None:
        assert e_form <= bound, (e_form, bound)


def _params(table):
    return pytest.mark.parametrize("index", range(len(TABLES[table])), ids=[_id(r) for r in TABLES[table]])


# ------------------------------------------------------------------------------------------------ 2. - 4. the 128 x 128 kernel, both loaders, five forms
@gpu
@pytest.mark.parametrize("form", FORMS)
@_params("rows")
def test_wgrad_row_loader_matches_float64(index, form, monkeypatch):
    _check_row("rows", index, form, monkeypatch, False)


@gpu
@pytest.mark.parametrize("form", FORMS)
@_params("pixel")
def test_wgrad_pixel_loader_matches_float64(index, form, monkeypatch):
    _check_row("pixel", index, form, monkeypatch, False)


# ------------------------------------------------------------------------------------------------ 5. the fused bias gradient
@gpu
@pytest.mark.parametrize("form", ["fp32", "a"])
@_params("colsum")
def test_wgrad_colsum_matches_float64(index, form, monkeypatch):
    _check_row("colsum", index, form, monkeypatch, True)


@gpu
@pytest.mark.parametrize("geom", COLSUM_PLANE_DY, ids=lambda g: "-".join(map(str, g)))
@pytest.mark.parametrize("form", ["dy", "both"])
def test_wgrad_dbias_with_plane_dy_goes_through_colsum_accum(geom, form, monkeypatch):
    """Plane dY cannot feed the fused sums (they add the fp32 registers): lib.gemm_wgrad sums the decoded planes with ddpo_colsum_accum.  What that
    launch adds is held to the float64 sum of the DECODED planes at the db gate.  Against the float64 sum of dY itself the planes' own rounding comes
    on top: hi = bf16(x), lo = bf16(x - hi), each to nearest with unit roundoff 2^-8, so |x - hi - lo| <= 2^-16 |x| per element and a column's sum
    is off by at most 2^-16 * sum_m |dY[m, n]| — the bound below, per column, from the number format alone (at these sizes the expected plane error
    is 1e-6 .. 2e-6 of max|ref_db|: ON the db gate, which was set for fp32 dY)."""
    row = next(r for r in COLSUM if r[0] == geom)
    buf0, buf, dbuf0, dbuf = _launch(row, form, monkeypatch, True)
    assert _sentinels_intact(buf0, buf) and _sentinels_intact(dbuf0, dbuf)
    monkeypatch.setattr(L, "A_KBLOCKED", False)
    dy = _inputs(geom)[1]
    dec = L.split_planes(dy).float().cpu().double().sum(0)
    ref_dw, ref_db = _reference(geom)
    got = _payload(dbuf).cpu().double() - _payload(dbuf0).cpu().double()
    e_dec, e_db = float((got - dec).abs().max() / dec.abs().max()), float((got - ref_db).abs().max() / ref_db.abs().max())
    e_dw = float(((_payload(buf).cpu().double() - _payload(buf0).cpu().double()).view_as(ref_dw) - ref_dw).abs().max() / ref_dw.abs().max())
    from conftest import parity_record
    parity_record(f"[wgrad branches] colsum_accum {_id(row)} [{form}]: db vs decoded planes {e_dec:.2e} (gate {DB_GATE:.0e}), vs dY {e_db:.2e}; dw {e_dw:.2e}")
    assert e_dec < DB_GATE and e_dw < DW_GATE
    assert bool(((got - ref_db).abs() <= DB_GATE * ref_db.abs().max() + 2.0 ** -16 * dy.cpu().double().abs().sum(0)).all())


# ------------------------------------------------------------------------------------------------ 1. the wide kernel and its near misses
@gpu
@pytest.mark.parametrize("form", FORMS)
@_params("wide_miss")
def test_wgrad_wide_near_misses_match_float64(index, form, monkeypatch):
    _check_row("wide_miss", index, form, monkeypatch, False)


@gpu
@pytest.mark.parametrize("form", FORMS)
@_params("wide")
def test_wgrad_wide_kernel_matches_float64(index, form, monkeypatch):
    _check_row("wide", index, form, monkeypatch, with_db=not FORM_PLANES[form][1])      # fused colsum in the fp32-dY forms: waves 0-3 sum three tasks, 4-7 two


# ------------------------------------------------------------------------------------------------ 6. refused descriptors
def _einval_call(case):
    """(entry point name, descriptor, plane pointers or None, `out` tensor) of one refused call; every other field is valid, so that the named
    check is the one that refuses.  Keeps the tensors alive through the returned tuple."""
    M, K, N = 64, 64, 64
    g = torch.Generator(device=DEV).manual_seed(7)
    x, dy = torch.randn(M, K + 4, device=DEV, generator=g), torch.randn(M, N, device=DEV, generator=g)
    out, cs = torch.randn(K + 4, N, device=DEV, generator=g), torch.randn(N, device=DEV, generator=g)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(L, "A_KBLOCKED", False)
        xp, dyp = L.split_planes(x[:, :K].contiguous()), L.split_planes(dy)
    conv = None
    if case in ("pad_not_half", "upsample_2", "stride_3"):
        conv = dict(ksize=3, stride=1, pad=1, upsample=0, B=1, H=8, W=8, Cin=K, OH=8, OW=8)
        if case == "pad_not_half":
            conv.update(pad=0, H=10, W=10)                       # OH = OW = 8: M still equals B * OH * OW
        elif case == "upsample_2":
            conv.update(upsample=2)
        else:
            conv.update(stride=3, H=24, W=24)                    # (24 + 2 - 3) // 3 + 1 = 8
        x = torch.randn(conv["B"] * conv["H"] * conv["W"], K, device=DEV, generator=g)
    Kd = 9 * K if conv else K
    if conv:
        out = torch.randn(Kd, N, device=DEV, generator=g)
    d = L._gemm_desc(M, N, Kd, conv=conv, src=x, ld_src=x.shape[1], out=out, ld_w=N, accumulate=1)
    d.w = dy.data_ptr()
    planes = None
    nul = lambda: [None, None, None, None]
    ptr = lambda pl: [L._p(pl.hi), L._p(pl.lo)]
    if case == "colsum_with_plane_dy":
        d.w, d.colsum, planes = None, cs.data_ptr(), [None, None] + ptr(dyp)
    elif case == "ld_src_0_fp32":
        d.ld_src = 0
    elif case == "ld_w_0_ragged_n":
        d.N, d.ld_w, d.w, planes = 36, 0, None, [None, None] + ptr(dyp)
    elif case == "hi_without_lo":
        d.src, planes = None, [L._p(xp.hi), None, None, None]
    elif case == "k_not_quad":
        d.K = K + 2                                              # ld_src = K + 4 stays a multiple of 4
    elif case == "res_rows":
        d.res_rows = 1
    elif case == "plane_misaligned_2_bytes":
        d.src, planes = None, [xp.hi.data_ptr() + 2, L._p(xp.lo), None, None]
    elif case == "planes_entry_without_planes":
        planes = nul()
    return d, planes, out, (x, dy, cs, xp, dyp)


@gpu
@pytest.mark.parametrize("case", EINVAL)
def test_wgrad_entry_points_refuse_and_leave_out_untouched(case):
    d, planes, out, keep = _einval_call(case)
    before, cs_before = out.clone(), keep[2].clone()
    lib = L.load()
    if planes is None:
        rc = lib.ddpo_gemm_conv_wgrad_bf16x3(byref(d), L._stream())
    else:
        rc = lib.ddpo_gemm_conv_wgrad_bf16x3_planes(byref(d), *planes, L._stream())
    torch.cuda.synchronize()
    assert rc == -1, (case, rc)
    assert torch.equal(out, before) and torch.equal(keep[2], cs_before)


@gpu
def test_wgrad_refused_descriptors_are_valid_but_for_the_named_field():
    """The descriptor the EINVAL cases start from is accepted by both entry points: each case is refused for its own field alone."""
    d, _, out, keep = _einval_call("planes_entry_without_planes")
    x, dy, _, xp, dyp = keep
    ref = x[:, :64].double().t() @ dy.double()
    lib = L.load()
    out.zero_()
    assert lib.ddpo_gemm_conv_wgrad_bf16x3(byref(d), L._stream()) == 0
    assert float((out[:64].double() - ref).abs().max() / ref.abs().max()) < DW_GATE and float(out[64:].abs().max()) == 0.0
    out.zero_()
    d.src = None
    d.ld_src = 64
    assert lib.ddpo_gemm_conv_wgrad_bf16x3_planes(byref(d), L._p(xp.hi), L._p(xp.lo), None, None, L._stream()) == 0
    assert float((out[:64].double() - ref).abs().max() / ref.abs().max()) < DW_GATE and float(out[64:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ the gates are not slack (CPU)
def _np_inputs(geom, seed=0):
    M, N, K, Cin, conv = _geometry(geom)
    rng = np.random.default_rng(zlib.crc32(repr(geom).encode()) + seed)
    rows = conv["B"] * conv["H"] * conv["W"] if conv else M
    return rng.standard_normal((rows, Cin)), rng.standard_normal((M, N))


def _np_scale(geom, x, dy):
    """max|dW| from a float32 evaluation (the scale the dw gate divides by; a float64 product of the wide geometries is slow on a host)."""
    x32, dy32 = torch.from_numpy(x).float(), torch.from_numpy(dy).float()
    if geom[0] == "dense":
        return float((x32.t() @ dy32).abs().max())
    return max(float((a.t() @ dy32).abs().max()) for a in _conv_taps(x32, *geom[1:5], *geom[6:9]))


def test_wgrad_gates_see_the_named_defects():
    """What a defective kernel would return, formed in float64 numpy for one row per table: each defect moves the result by at least 10 x its gate,
    or lands on a sentinel.  (No defective kernel is built or run.)"""
    seen = {}
    # (a) the last k-tile of the last split dropped: the row loader's nk = 3 row, and the wide kernel's first row
    for name, geom in (("rows", ROWS[2][0]), ("wide", WIDE[0][0])):
        x, dy = _np_inputs(geom)
        seen[f"last k-tile dropped ({name})"] = (np.abs(x[-32:].T @ dy[-32:]).max() / _np_scale(geom, x, dy), DW_GATE)
    # (b) one border row of one tap not masked: the linear address of tap (ky = 0, kx = 1) at output row 0 of image 1 is the last row of image 0
    # (row loader, 3x3 16 x 16); for the per-pixel loader at stride 2, tap (1, 0) at output column 0 reads column -1 = the previous row's last column
    geom = ROWS[7][0]
    x, dy = _np_inputs(geom)
    B, H, W, Cin = geom[1:5]
    img, gy = x.reshape(B, H, W, Cin), dy.reshape(B, H, W, -1)
    seen["border row unmasked (rows)"] = (np.abs(img[0, H - 1].T @ gy[1, 0]).max() / _np_scale(geom, x, dy), DW_GATE)
    geom = PIXEL[9][0]
    x, dy = _np_inputs(geom)
    B, H, W, Cin = geom[1:5]
    img, gy = x.reshape(B, H, W, Cin), dy.reshape(B, H // 2, W // 2, -1)
    leak = sum(img[0, 2 * oy - 1, W - 1][:, None] * gy[0, oy, 0][None, :] for oy in range(1, H // 2))
    seen["border column unmasked (pixel)"] = (np.abs(leak).max() / _np_scale(geom, x, dy), DW_GATE)
    # (c) the wide tile's third dY task (columns 256 .. 319, waves 0-3) missing one pixel-pair half: pixels 16 .. 31 of every k-tile
    geom = WIDE[0][0]
    x, dy = _np_inputs(geom)
    half = (np.arange(x.shape[0]) % 32) >= 16
    seen["columns 256..319 miss a pixel-pair half (wide)"] = (np.abs(x[half][:, :128].T @ dy[half][:, 256:]).max() / _np_scale(geom, x, dy), DW_GATE)
    # (d) the colsum of the N tail quad dropped (N = 36: columns 32 .. 35)
    geom = COLSUM[1][0]
    _, dy = _np_inputs(geom)
    db = dy.sum(0)
    seen["colsum of the N tail quad dropped"] = (np.abs(db[32:]).max() / np.abs(db.astype(np.float32)).max(), DB_GATE)
    for what, (err, gate) in seen.items():
        print(f"[wgrad branches] defect: {what}: {err:.2e} = {err / gate:.0f} x the gate {gate:.0e}")
        assert err >= 10 * gate, (what, err, gate)
    # (e) one write to row K: the first float behind dw, whatever the column
    M, N, K, _, _ = _geometry(ROWS[0][0])
    before = np.random.default_rng(5).standard_normal(K * N + 2 * SENTINEL).astype(np.float32)
    for col in (0, N - 1):
        after = before.copy()
        after[SENTINEL + K * N + col] += np.float32(1e-3)
        assert not _sentinels_intact(before, after)
    after = before.copy()
    after[SENTINEL:SENTINEL + K * N] += 1.0
    assert _sentinels_intact(before, after)
