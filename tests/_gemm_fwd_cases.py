"""Tables, exact operand builder and dispatch re-derivation for tests/test_gpu_gemm_fwd_routes.py (the forward bf16 / f16mx GEMM family of
ddpo_amd/csrc/gemm_bf16.hip), and the f16mx plane decoders test_gpu_f16mx.py shares with it.  Nothing here touches a device at import time."""
import os
import re
import zlib

import torch

from ddpo_amd import lib as L

WS_BYTES = 64 << 20          # lib.SPLITK_WS_BYTES: the scratch every launch of the tables gets
BK = 32
LIMIT = float(1 << 24)       # exactly representable integers of fp32


# ------------------------------------------------------------------------------------------------ geometry
def dense(M, K, N):
    return ("dense", M, K, N)


def conv(B, H, W, Cin, Cout, ks=3, stride=1, ups=False):
    return ("conv", B, H, W, Cin, Cout, ks, stride, ups)


def geometry(geom):
    """M, N, K, channels per tap, lib's conv dict (None: dense) and the source rows of a table geometry."""
    if geom[0] == "dense":
        _, M, K, N = geom
        return M, N, K, K, None, M
    _, B, H, W, Cin, Cout, ks, stride, ups = geom
    c = L._conv_geom(B, H, W, Cin, ks, stride, None, ups)
    return B * c["OH"] * c["OW"], Cout, ks * ks * Cin, Cin, c, B * H * W


def gid(geom):
    return "x".join(str(int(v) if isinstance(v, bool) else v) for v in geom)


# ------------------------------------------------------------------------------------------------ the host rule, restated
_TODAY = dict(min128=32, minwide=16, tall_min=200, wide_blk_max=192, grid128_max=192, tall_margin=1.08, wide_min=200, wide_rows_min=512,
              wide_split_min_nk=64, wide_short_nk=16, wide_short_n=1280, mid_tiles=512, mid_nk=64, big_tiles=256, want128=384, wantwide=256)


def rule_constants():
    """The constants of dispatch_bf16 / wide_splits / splits_128 read out of gemm_bf16.hip; the text of the rules they sit in is asserted, so an
    edit of the rule that this file does not mirror fails the CPU test instead of silently re-routing the tables."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ddpo_amd", "csrc", "gemm_bf16.hip")).read()
    flat = " ".join(src.split())
    pats = dict(
        min128=r"constexpr int SPLITK_MIN_KTILES_128 = (\d+);",
        minwide=r"constexpr int SPLITK_MIN_KTILES_WIDE = (\d+);",
        tall=r"bool tall = PLANES && d\.N % 320 == 0 && ntall >= (\d+) && eff_tall \* ([\d.]+) >= eff_wide;",
        wide=r"\} else if \(d\.N % 320 == 0 && \(long\)NPH \* d\.M >= (\d+) && buf_path_ok\(d, ldw\) && !\(d\.K / BF_BK < (\d+) && d\.N > (\d+)\) && "
             r"\(long\)NPH \* \(\(d\.M \+ 127\) / 128\) \* \(d\.N / 320\) \* wsplits >= (\d+) && !\(wsplits > 1 && d\.K / BF_BK < (\d+)\)\) \{",
        mid=r"const bool mid_short = t128 < (\d+) && d\.K / BF_BK <= (\d+);",
        big=r"const bool big = \(d\.N % 128 == 0\) && t128 >= (\d+) && !mid_short;",
        s128=r"if \(have_ws && ngrid < (\d+) && nk_total >= SPLITK_MIN_KTILES_128 && \(d\.N & 3\) == 0 && d\.epilogue == 0\) \{ splits = \((\d+) \+ ngrid - 1\) / ngrid;",
        swide=r"if \(have_ws && nblk <= (\d+) && nk_total >= SPLITK_MIN_KTILES_WIDE\) \{ splits = \((\d+) \+ nblk / 2\) / nblk;",
    )
    m = {k: re.search(p, flat) for k, p in pats.items()}
    assert all(m.values()), "the host rule of dispatch_bf16() is no longer spelled as this test restates it: " + str([k for k, v in m.items() if not v])
    for text in ("if (splits > 8) splits = 8; if (splits > nk_total / 8) splits = nk_total / 8;",
                 "while (splits > 1 && (size_t)nph * splits * d.M * d.N * sizeof(float) > ws_bytes) --splits;",
                 "int ktps = (nk_total + splits - 1) / splits; ktps = (ktps + 1) & ~1; splits = (nk_total + ktps - 1) / ktps;",
                 "const int ngrid = NPH * ((d.M + 127) / 128) * ((d.N + (big ? 127 : 63)) / (big ? 128 : 64));",
                 "if (d.ksize > 0) { if (d.Cin % BF_BK) return false;", "} else { if (d.K % BF_BK) return false;",
                 "if (!T::SPLITK) splits = 1;", "constexpr bool GENERIC = KL == KLoop::regs && T::BN <= 128;",
                 "Route{d.epilogue == 2 ? RT_TALL_GEGLU : RT_128, 1}"):
        assert text in flat, text
    g = lambda k, i=1: m[k].group(i)
    return dict(min128=int(g("min128")), minwide=int(g("minwide")), tall_min=int(g("tall")), tall_margin=float(g("tall", 2)),
                wide_rows_min=int(g("wide")), wide_short_nk=int(g("wide", 2)), wide_short_n=int(g("wide", 3)), wide_min=int(g("wide", 4)),
                wide_split_min_nk=int(g("wide", 5)), mid_tiles=int(g("mid")), mid_nk=int(g("mid", 2)), big_tiles=int(g("big")),
                grid128_max=int(g("s128")), want128=int(g("s128", 2)), wide_blk_max=int(g("swide")), wantwide=int(g("swide", 2)))


def kernel_table():
    """(tile, k-loop, datapath, FOLD) of every instantiation kernel_exists() admits, from the enums of the .hip file: the coverage universe."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ddpo_amd", "csrc", "gemm_bf16.hip")).read()
    dps = re.findall(r"^\s+(\w+) = \d+,", re.search(r"enum class Datapath : int \{(.*?)\};", src, re.S).group(1), re.M)
    kls = re.findall(r"^\s+(\w+) = \d+,", re.search(r"enum class KLoop : int \{(.*?)\};", src, re.S).group(1), re.M)
    out = set()
    for tile in ("tall", "wide", "128", "64"):
        for kl in kls:
            for dp in dps:
                for fold in (False, True):
                    if fold and (dp == "f16x1" or kl in ("regs", "tall_geglu", "tall_mx_geglu")):
                        continue
                    if tile == "tall":
                        ok = kl in (("tall", "tall_geglu") if dp == "bf16x3" else ("tall_mx", "tall_mx_geglu") if dp == "f16mx" else ("tall_ring",))
                    else:
                        ok = kl == "planes3w" or (kl == "regs" and dp in ("bf16x1", "bf16x3"))
                    if ok:
                        out.add((tile, kl, dp, fold))
    return dps, kls, out


def buf_path_ok(K, cin, is_conv):
    return (cin if is_conv else K) % BK == 0          # (every table operand is far below the 31-bit offsets)


def _splits(want, nblk, nk, M, N, nph, ws):
    s = min(want, 8, nk // 8)
    s = max(s, 1)
    while s > 1 and nph * s * M * N * 4 > ws:
        s -= 1
    return s


def dispatch(M, N, K, cin, is_conv, planes, c=_TODAY, nph=1, epilogue=0, ws=WS_BYTES):
    """(tile class, generic?, splits after rounding, k-tiles of the first split, of the last split, rows in the last M tile, columns in the
    last N tile) — dispatch_bf16 + launch_tile, for a launch with a 64 MiB workspace.  nph = 4: the folded up-sampler."""
    nk, nkf = -(-K // BK), K // BK
    buf = buf_path_ok(K, cin, is_conv)
    cd = lambda a, b: -(-a // b)
    if epilogue:
        tile, splits = ("tall" if epilogue == 2 else "128"), 1
    else:
        ntall, nwide = nph * cd(M, 256) * (N // 320), nph * cd(M, 128) * (N // 320)
        eff = lambda n: n / (cd(n, 256) * 256) if n else 0.0
        tall = planes and N % 320 == 0 and ntall >= c["tall_min"] and eff(ntall) * c["tall_margin"] >= eff(nwide)
        nblk = nph * cd(M, 128) * cd(N, 320)
        ws_ = 1
        if nblk <= c["wide_blk_max"] and nkf >= c["minwide"]:
            ws_ = _splits((c["wantwide"] + nblk // 2) // nblk, nblk, nkf, M, N, nph, ws)
        if tall:
            tile, splits = "tall", 1
        elif (N % 320 == 0 and nph * M >= c["wide_rows_min"] and buf and not (nkf < c["wide_short_nk"] and N > c["wide_short_n"]) and
              nwide * ws_ >= c["wide_min"] and not (ws_ > 1 and nkf < c["wide_split_min_nk"])):
            tile, splits = "wide", ws_
        else:
            t128 = nph * cd(M, 128) * cd(N, 128)
            mid_short = t128 < c["mid_tiles"] and nkf <= c["mid_nk"]
            big = N % 128 == 0 and t128 >= c["big_tiles"] and not mid_short
            ngrid = nph * cd(M, 128) * cd(N, 128 if big else 64)
            splits = 1
            if ngrid < c["grid128_max"] and nk >= c["min128"] and N % 4 == 0:
                splits = _splits(cd(c["want128"], ngrid), ngrid, nk, M, N, nph, ws)
            tile = "128" if big else "64"
    bm, bn = {"tall": (256, 320), "wide": (128, 320), "128": (128, 128), "64": (128, 64)}[tile]
    if tile == "tall":
        splits = 1
    first = last = nk
    if tile != "tall":
        ktps = (cd(nk, splits) + 1) & ~1
        splits = cd(nk, ktps)
        first, last = min(ktps, nk), nk - (splits - 1) * ktps
    generic = (not buf) and not planes and tile in ("128", "64")
    return (tile, generic, splits, first, last, M - (cd(M, bm) - 1) * bm, N - (cd(N, bn) - 1) * bn)


# ------------------------------------------------------------------------------------------------ output-stage option sets
# name -> dict(bias, rowbias, residual, res_rows (True: M / 2, ld_res = N + 32), alpha, ld_pad (ld_out = N + 64), unaligned (out starts one float off
# a 16-byte boundary: the scalar stage of the buffer-addressed kernels), planes = (mode, k-blocked, fmt))
OPTS = {
    "plain": {},
    "bias": dict(bias=True),
    "rowbias": dict(rowbias=True),
    "res": dict(residual=True),
    "both": dict(bias=True, rowbias=True, residual=True),
    "period": dict(residual=True, res_rows=True),
    "alpha": dict(alpha=0.5, bias=True),
    "ldout": dict(ld_pad=64, bias=True),
    "unaligned": dict(unaligned=True, bias=True, residual=True),
    "p_both": dict(planes=("both", False, 0), bias=True),
    "p_only": dict(planes=("only", False, 0), residual=True),
    "p_both_kb": dict(planes=("both", True, 0), alpha=0.5),
    "p_only_kb": dict(planes=("only", True, 0), rowbias=True),
    "p_both_mx": dict(planes=("both", False, 1), bias=True),
    "p_only_mxkb": dict(planes=("only", True, 1), residual=True, res_rows=True),
}
PLAIN_OPTS = ["plain", "bias", "rowbias", "res", "both", "period", "alpha", "ldout"]
REQUIRED = ["bias", "rowbias", "res", "both", "period", "alpha", "ldout"]          # what the issue wants on each of the four output stages
PLANE_OPTS = ["p_both", "p_only", "p_both_kb", "p_only_kb", "p_both_mx", "p_only_mxkb"]


def row_opts(geom, expect):
    """The option sets a row can take (a period needs an even M; plane outputs need the vector stage, whole 32-column blocks for k-blocked / f16mx
    planes and the buffer-addressed kernels)."""
    M, N, K, cin, cv, _ = geometry(geom)
    names = [n for n in PLAIN_OPTS if not (OPTS[n].get("res_rows") and M % 2)]
    if expect[1] or N % 4:
        return names                                                    # generic kernel / N % 4: the scalar stage whatever the alignment
    names.append("unaligned")
    for n in PLANE_OPTS:
        _, kb, fmt = OPTS[n]["planes"]
        if (kb or fmt) and N % 32:
            continue
        if OPTS[n].get("res_rows") and M % 2:
            continue
        names.append(n)
    return names


def stage_of(expect, optname, N):
    """The output stage a (row, option set) ends in: scalar, vector, reduce (split-K) or tall."""
    if expect[2] > 1:
        return "reduce"
    if expect[1] or N % 4 or OPTS[optname].get("unaligned"):
        return "scalar"
    return "tall" if expect[0] == "tall" else "vector"


# ------------------------------------------------------------------------------------------------ shape tables
# (geometry, feeds, expectation tuple); feeds: "f" fp32-fed, "p" row-major planes, "k" k-blocked planes
def _r(geom, feeds, expect):
    return (geom, feeds, expect)


TALL = [       # plane-fed only: 200 tall tiles; nk = 1 .. 5 on tall (bf16x3), tall_mx (f16mx) and tall_ring (bf16 / f16 single pass)
    _r(dense(25600, 32, 640), "pk", ("tall", False, 1, 1, 1, 256, 320)),
    _r(dense(25600, 64, 640), "pk", ("tall", False, 1, 2, 2, 256, 320)),
    _r(dense(25600, 96, 640), "pk", ("tall", False, 1, 3, 3, 256, 320)),
    _r(dense(25600, 128, 640), "pk", ("tall", False, 1, 4, 4, 256, 320)),
    _r(dense(25600, 160, 640), "pk", ("tall", False, 1, 5, 5, 256, 320)),
    _r(dense(50945, 64, 320), "pk", ("tall", False, 1, 2, 2, 1, 320)),            # the last tall tile holds ONE row
    _r(dense(51123, 96, 320), "pk", ("tall", False, 1, 3, 3, 179, 320)),          # ragged last tile, odd nk
    _r(conv(1, 226, 226, 32, 320), "pk", ("tall", False, 1, 9, 9, 132, 320)),     # a 3x3 convolution on the tall tile: a tap per k-tile, ragged last tile
]
WIDE = [
    _r(dense(25595, 96, 320), "fpk", ("wide", False, 1, 3, 3, 123, 320)),         # 200 wide tiles, ragged M, nk = 3; plane-fed: ntall = 100, so not tall
    _r(dense(6400, 96, 1280), "fpk", ("wide", False, 1, 3, 3, 128, 320)),         # four column tiles
    _r(dense(3200, 2080, 320), "fpk", ("wide", False, 7, 10, 5, 128, 320)),       # 7 splits of 10, the last 5 (odd)
    _r(dense(3197, 2144, 320), "fpk", ("wide", False, 7, 10, 7, 125, 320)),       # 7 splits, the last 7, ragged M
    _r(conv(2, 40, 40, 256, 320), "fpk", ("wide", False, 8, 10, 2, 128, 320)),    # a 3x3 convolution on the wide split route: splits start inside a tap (256 / 32 = 8 k-tiles per tap)
]
T128 = [
    _r(dense(4096, 2080, 1024), "fpk", ("128", False, 1, 65, 65, 128, 128)),      # 256 tiles, nk = 65 (odd), unsplit
    _r(dense(8192, 64, 1024), "fpk", ("128", False, 1, 2, 2, 128, 128)),          # 512 tiles, nk = 2
]
T64 = [
    _r(dense(512, 32, 64), "fpk", ("64", False, 1, 1, 1, 128, 64)),               # nk = 1: prologue only
    _r(dense(130, 96, 72), "fpk", ("64", False, 1, 3, 3, 2, 8)),                  # two rows in the last M tile, an 8-column N tail
    _r(dense(40, 64, 8), "fpk", ("64", False, 1, 2, 2, 40, 8)),                   # N = 8: one quad pair
    _r(dense(130, 96, 70), "fpk", ("64", False, 1, 3, 3, 2, 6)),                  # N % 4 != 0: the scalar stage of the buffer-addressed kernel
    _r(dense(256, 1056, 128), "fpk", ("64", False, 4, 10, 3, 128, 64)),           # 4 splits of 10, the last 3
    _r(dense(384, 2080, 68), "fpk", ("64", False, 7, 10, 5, 128, 4)),             # 7 splits, the last 5; a 4-column N tail under split-K
    _r(dense(100, 2048, 320), "fpk", ("64", False, 8, 8, 8, 100, 64)),            # 8 x 8; M < one tile (N % 320 == 0 but M < 512: not wide)
]
GENERIC = [    # Cin % 8 == 0 but % 32 != 0: the pointer-addressed kernel, fp32-fed only
    _r(dense(130, 40, 72), "f", ("64", True, 1, 2, 2, 2, 8)),                     # a K tail of 8 in the last k-tile
    _r(dense(256, 1064, 128), "f", ("64", True, 4, 10, 4, 128, 64)),              # 34 k-tiles (the last holds 8): 4 splits through the generic `part` path
    _r(conv(2, 8, 8, 8, 64), "f", ("64", True, 1, 3, 3, 128, 64)),                # AFFINE, Cin = 8: four taps per k-tile
    _r(conv(3, 5, 7, 24, 72), "f", ("64", True, 1, 7, 7, 105, 8)),                # AFFINE, non-square, Cin = 24: k-tiles straddle taps
    _r(conv(2, 8, 8, 40, 64, 3, 2), "f", ("64", True, 1, 12, 12, 32, 64)),        # AFFINE, stride 2, Cin = 40
    _r(conv(1, 6, 6, 24, 64, 3, 1, True), "f", ("64", True, 1, 7, 7, 16, 64)),    # non-AFFINE: nearest-2x in the gather
    _r(conv(2, 8, 8, 24, 64, 1), "f", ("64", True, 1, 1, 1, 128, 64)),            # 1 x 1, a K tail of 24
]
CONV = [       # buffer path: tap changes inside and between k-tiles' runs, masked border rows
    _r(conv(2, 16, 16, 32, 64), "fpk", ("64", False, 1, 9, 9, 128, 64)),          # Cin = 32: a tap per k-tile, odd nk = 9
    _r(conv(2, 16, 16, 96, 64), "fpk", ("64", False, 1, 27, 27, 128, 64)),        # Cin = 96: three k-tiles per tap, odd nk = 27
    _r(conv(2, 16, 16, 96, 72, 1), "fpk", ("64", False, 1, 3, 3, 128, 8)),        # 1 x 1
    _r(conv(2, 16, 16, 32, 64, 3, 2), "fpk", ("64", False, 1, 9, 9, 128, 64)),    # stride 2
    _r(conv(2, 16, 16, 64, 64, 1, 2), "fpk", ("64", False, 1, 2, 2, 128, 64)),    # 1 x 1 stride 2
    _r(conv(2, 8, 8, 32, 64, 3, 1, True), "fpk", ("64", False, 1, 9, 9, 128, 64)),        # nearest-2x in the gather
    _r(conv(3, 5, 7, 32, 64), "fpk", ("64", False, 1, 9, 9, 105, 64)),            # non-square, M < one tile
]
TABLES = {"tall": TALL, "wide": WIDE, "t128": T128, "t64": T64, "generic": GENERIC, "conv": CONV}
# data gradients (lib.conv2d_dgrad) of two CONV rows: w_dgrad addressing of the fp32-fed kernel (lib.DGRAD_FWD off) and the forward form on the
# registered data-gradient planes; stride 2 = zero insertion (upsample == 2)
DGRAD = [conv(2, 16, 16, 32, 64), conv(2, 16, 16, 32, 64, 3, 2), conv(2, 8, 8, 16, 24), conv(2, 8, 8, 16, 24, 3, 2)]
# folded up-sampler (B, H, W, C, N) -> (tile, splits, first, last); only the k-loop tails are new here (tests/test_gpu_upsample_fold.py covers the routes)
FOLD = [
    ((1, 8, 8, 32, 64), ("64", False, 1, 4, 4, 64, 64)),                          # 128x64 unsplit, nk = 4
    ((13, 32, 32, 32, 320), ("tall", False, 1, 4, 4, 256, 320)),                  # 4 x 52 tall tiles, nk = 4
    ((2, 16, 16, 288, 320), ("64", False, 4, 10, 6, 128, 64)),                    # 128x64, 4 splits of 10, the last 6
    ((1, 6, 10, 32, 64), ("64", False, 1, 4, 4, 60, 64)),                         # non-square, M < one tile
]
# GEGLU (M, K, F): epilogue 1 on the 128 x 128 tile, epilogue 2 (planes; bf16x3 and f16mx) on the tall tile
GEGLU_128 = [((300, 128, 64), ("128", False, 1, 4, 4, 44, 128)), ((130, 32, 64), ("128", False, 1, 1, 1, 2, 128)), ((130, 96, 64), ("128", False, 1, 3, 3, 2, 128))]
GEGLU_TALL = [((25600 - 77, 32, 320), ("tall", False, 1, 1, 1, 179, 320)), ((25600 - 77, 96, 320), ("tall", False, 1, 3, 3, 179, 320))]

# ------------------------------------------------------------------------------------------------ variants: (feed, weight layout k-blocked?, datapath, operand class)
# datapaths: "bf16" (single pass), "bf16x3", "f16mx", "f16x1" (f16mx without its cross terms)
DP_ENUM = {"bf16": "bf16x1", "bf16x3": "bf16x3", "f16mx": "f16mx", "f16x1": "f16x1"}


def variants(feeds):
    v = []
    if "f" in feeds:
        v += [("f", True, "bf16", "hi"), ("f", True, "bf16x3", "hi"), ("f", False, "bf16x3", "hi"), ("f", False, "bf16", "a_lo"),
              ("f", True, "bf16x3", "a_lo"), ("f", True, "bf16x3", "w_lo"), ("f", True, "bf16x3", "both_lo"), ("f", True, "bf16", "w_lo")]
    for feed in "pk":
        if feed in feeds:
            v += [(feed, True, "bf16", "hi"), (feed, True, "bf16x3", "hi"), (feed, True, "f16mx", "hi"), (feed, True, "f16x1", "hi"),
                  (feed, True, "bf16x3", "a_lo"), (feed, True, "bf16x3", "w_lo"), (feed, True, "bf16x3", "both_lo"), (feed, True, "f16mx", "mx_lo")]
    if "p" in feeds:
        v += [("p", False, "bf16x3", "hi"), ("p", False, "bf16", "a_lo"), ("p", False, "bf16x3", "both_lo"), ("p", True, "bf16", "w_lo")]
    return v


def cases(table):
    """(row index, variant, option set name): every variant of the row once, the row's option sets dealt round over them (and, where a row has
    more option sets than variants, every option set once)."""
    out = []
    for i, (geom, feeds, expect) in enumerate(TABLES[table]):
        vs, os_ = variants(feeds), row_opts(geom, expect)
        for j in range(max(len(vs), len(os_))):
            out.append((i, vs[j % len(vs)], os_[(j + i) % len(os_)]))
    return out


def kloop_of(tile, feed, dp, geglu=False):
    if feed == "f":
        return "regs"
    if tile != "tall":
        return "planes3w"
    if geglu:
        return "tall_geglu" if dp == "bf16x3" else "tall_mx_geglu"
    return {"bf16x3": "tall", "f16mx": "tall_mx"}.get(dp, "tall_ring")


# ------------------------------------------------------------------------------------------------ exact operands
# class -> (|a| max, a unit, |w| max, w unit): integers times a power of two
CLASSES = {"hi": (255, 2.0 ** -8, 15, 2.0 ** -3), "a_lo": (1023, 2.0 ** -10, 7, 2.0 ** -2), "w_lo": (7, 2.0 ** -2, 1023, 2.0 ** -10),
           "both_lo": (1023, 2.0 ** -6, 1023, 2.0 ** -6), "mx_lo": (255, 2.0 ** -8, 15, 2.0 ** -3)}
EPI_UNIT = 2.0 ** -4         # bias / row bias / residual: integers in +-63 times 2^-4 (a multiple of every product unit above)
WIDE_DENSITY = (16, 32)      # both_lo: one activation in 16 and one weight in 32 is 10-11 bits wide (512 .. 1023), the others are +-3


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _ints(gen, shape, lim, device):
    return torch.randint(-lim, lim + 1, shape, generator=gen, device=device, dtype=torch.int64).double()


def build_operands(geom, cls, device="cpu", tile=0):
    """(a (source rows, Cin), w (K, N)) float64 holding exactly fp32-representable values: integers times the class's units.
    both_lo: a product of two 10-bit operands has 20 bits, so only K = 16 of them would fit 2^24 — most entries are therefore +-3 and one in
    16 (activations) / 32 (weights) is 512 .. 1023 wide; the guard (exactness_bound) is asserted on the actual draw.
    mx_lo: the hi draw, except that k-tile `tile` (of every tap-free reduction index 32 tile .. 32 tile + 31) holds f16 hi parts of 8 .. 16
    (activations) / 16 .. 32 (weights) with non-zero low parts of 1 .. 3 times 2^-10 / 2^-9: below half an f16 ulp, exact in e5m2 / e4m3."""
    M, N, K, cin, cv, rows = geometry(geom)
    ga, gw = (torch.Generator(device=device).manual_seed(_seed(geom, cls, s)) for s in "aw")
    alim, au, wlim, wu = CLASSES[cls]
    if cls == "both_lo":
        def draw(gen, shape, dens):
            small = _ints(gen, shape, 3, device)
            wide = (512 + torch.randint(0, 512, shape, generator=gen, device=device)).double() * (torch.randint(0, 2, shape, generator=gen, device=device) * 2 - 1).double()
            return torch.where(torch.randint(0, dens, shape, generator=gen, device=device) == 0, wide, small)
        return draw(ga, (rows, cin), WIDE_DENSITY[0]) * au, draw(gw, (K, N), WIDE_DENSITY[1]) * wu
    a, w = _ints(ga, (rows, cin), alim, device) * au, _ints(gw, (K, N), wlim, device) * wu
    if cls == "mx_lo":
        k0 = 32 * (tile % (K // 32))
        c0 = k0 % cin                                              # the k-tile's channels (a k-tile never straddles a tap: cin % 32 == 0)
        sgn = lambda gen, shape: (torch.randint(0, 2, shape, generator=gen, device=device) * 2 - 1).double()
        ah = torch.randint(128, 256, (rows, 32), generator=ga, device=device).double() / 16.0 * sgn(ga, (rows, 32))
        al = torch.randint(1, 4, (rows, 32), generator=ga, device=device).double() * 2.0 ** -10 * sgn(ga, (rows, 32))
        wh = torch.randint(8, 16, (32, N), generator=gw, device=device).double() * 2.0 * sgn(gw, (32, N))
        wl = torch.randint(1, 4, (32, N), generator=gw, device=device).double() * 2.0 ** -9 * sgn(gw, (32, N))
        # (a 3x3 convolution reads the activation's channels under every tap: its low parts meet nine k-tiles, the weight's low parts one)
        a[:, c0:c0 + 32] = ah + al
        w[k0:k0 + 32] = wh + wl
    return a, w


def build_epilogue(geom, optname, device="cpu"):
    """dict(bias (N), rowbias (nb, N), rows_per_batch, residual (rows, ld_res), res_rows, ld_res, alpha) as float64, each None / 0 when the option
    set does not hold it."""
    M, N, K, cin, cv, rows = geometry(geom)
    o = OPTS[optname]
    g = torch.Generator(device=device).manual_seed(_seed(geom, optname))
    e = dict(bias=None, rowbias=None, rows_per_batch=0, residual=None, res_rows=0, ld_res=N, alpha=float(o.get("alpha", 1.0)))
    if o.get("bias"):
        e["bias"] = _ints(g, (N,), 63, device) * EPI_UNIT
    if o.get("rowbias"):
        rpb = max(1, M // 3)
        e["rows_per_batch"] = rpb
        e["rowbias"] = _ints(g, (-(-M // rpb), N), 63, device) * EPI_UNIT
    if o.get("residual"):
        if o.get("res_rows"):
            e["res_rows"], e["ld_res"] = M // 2, N + 32
        e["residual"] = _ints(g, (e["res_rows"] or M, e["ld_res"]), 63, device) * EPI_UNIT
    return e


def apply_epilogue(prod, e):
    """alpha * prod + bias + rowbias[m / rows_per_batch] + residual[m % res_rows], float64."""
    M, N = prod.shape
    out = e["alpha"] * prod
    if e["bias"] is not None:
        out = out + e["bias"]
    if e["rowbias"] is not None:
        out = out + e["rowbias"][torch.arange(M, device=prod.device) // e["rows_per_batch"]]
    if e["residual"] is not None:
        r = e["residual"][:, :N]
        out = out + (r[torch.arange(M, device=prod.device) % e["res_rows"]] if e["res_rows"] else r)
    return out


def conv_taps(x, B, H, W, Cin, ks, stride, ups):
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


def product(geom, a, w, k_weight=None):
    """The contraction of a table geometry in a's dtype: a @ w, or the sum over taps of the gathered activations times the tap's weights.
    k_weight (K,): a factor per reduction index — the defects of the CPU test (0 drops an index, 2 counts it twice)."""
    if k_weight is not None:
        w = w * k_weight[:, None]
    if geom[0] == "dense":
        return a @ w
    _, B, H, W, Cin, Cout, ks, stride, ups = geom
    return sum(t @ w[i * Cin:(i + 1) * Cin] for i, t in enumerate(conv_taps(a, B, H, W, Cin, ks, stride, ups)))


def exactness_bound(geom, cls, absprod_max, e):
    """An upper bound of max over the output of (alpha * sum_k |a_k| |w_k| + |bias| + |rowbias| + |residual|) in the common unit, as a fraction of
    2^24: below 1 every partial sum, in any order, is an fp32 integer multiple of that unit.  absprod_max = max(|a| @ |w|) of the draw.  (The
    bf16 planes of an operand are bounded by 1 + 2^-7 times the operand, of both by 1.016: the 1.02.)"""
    _, au, _, wu = CLASSES[cls]
    unit = au * wu * (0.5 if e["alpha"] == 0.5 else 1.0)
    assert EPI_UNIT / unit == int(EPI_UNIT / unit)
    extra = sum(63 * EPI_UNIT for k in ("bias", "rowbias", "residual") if e[k] is not None)
    return (e["alpha"] * 1.02 * absprod_max + extra) / unit / LIMIT


def bf16_round(t):
    """bf16(x), round to nearest even, as float64: the hi plane of the split."""
    return t.float().to(torch.bfloat16).double()


# ------------------------------------------------------------------------------------------------ f16mx plane decoders (shared with test_gpu_f16mx.py)
def dec_planes(p16, p8):
    """(h, h8, l8) as float64 (rows, C) from the row-major f16mx activation planes."""
    rows, C = p16.shape
    h = p16.view(torch.float16).double()
    b = p8.view(torch.float8_e5m2).double().view(rows, C // 32, 2, 2, 16)      # per block: [k half][h8 | l8][16]
    return h, b[:, :, :, 0].reshape(rows, C), b[:, :, :, 1].reshape(rows, C) / 2048.0


def dec_weights(wp):
    """(h, h8, l8) as float64 (K, N) from the f16mx weight planes (zero padded rows dropped)."""
    K, N = wp["K"], wp["N"]
    s = torch.pow(2.0, wp["scale"].double() - 127.0)                      # (N,)
    h = wp["w16"].view(torch.float16).double().permute(0, 2, 1).reshape(-1, N)[:K]      # (Kb, N, 32) -> (Kb*32, N)
    b = wp["w8"].view(torch.float8_e4m3fn).double().view(-1, N, 2, 2, 16)      # (Kb, N, k half, [l8 | h8], 16)
    l8 = (b[:, :, :, 0].reshape(-1, N, 32) * s[None, :, None] / 2048.0).permute(0, 2, 1).reshape(-1, N)[:K]
    h8 = (b[:, :, :, 1].reshape(-1, N, 32) * s[None, :, None]).permute(0, 2, 1).reshape(-1, N)[:K]
    return h, h8, l8
