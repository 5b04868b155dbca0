"""Writes tests/golden/lib_launch_records.json: what ddpo_amd/lib.py's GEMM / conv wrappers hand to the C ABI, recorded WITHOUT a GPU.

`L._lib` is replaced by a stand-in that answers every ddpo_* call with 0 (sizes / constants: a fixed value) and records the symbol, every scalar
argument and, for a ddpo_gemm_desc argument, the value of every field.  Pointers are recorded as null or as `label+byte offset` of the tensor
they point into (tensors the wrappers allocate themselves are labelled by dtype, shape and allocation ordinal, the fp32 decoding of planes
by the planes' label; any other temporary is `ext`), so a record does not depend on addresses.  Per case the file also holds what the wrapper returned, what it appended to
lib.PROFILE, and the type and message of an exception.  Only lib.py's PUBLIC functions and switches are used, so the file generated before a
refactor of lib.py must be reproduced byte for byte after it (tests/test_lib_launch_records_cpu.py).

    python tests/golden/make_lib_launch_records.py

Identical results are stored once (`results`) and the cases index into them (`cases`), which keeps the file small.
"""
import ctypes
import hashlib
import json
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from ddpo_amd import lib as L  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "lib_launch_records.json")
SWITCHES = ("PLANES", "PLANES_ALL", "PLANES_OUT", "TRAIN_PLANES", "BF16_PLANES", "GEGLU_TALL", "W_KBLOCKED", "A_KBLOCKED", "DGRAD_FWD",
            "UP2X_FOLD", "MX_CROSS")
DEFAULTS = dict(PLANES=True, PLANES_ALL=False, PLANES_OUT=True, TRAIN_PLANES=True, BF16_PLANES=True, GEGLU_TALL=True, W_KBLOCKED=True,
                A_KBLOCKED=False, DGRAD_FWD=True, UP2X_FOLD=True, MX_CROSS=True)
FIXED = {"ddpo_abi_version": 15, "ddpo_gemm_splitk_min_ktiles": 40, "ddpo_groupnorm_ws_bytes": 4096, "ddpo_groupnorm_stats_floats": 512,
         "ddpo_groupnorm_bwd_ws_bytes": 4096}
LIM = 0x7FFFFFFF
_DT = {torch.float32: "f32", torch.int16: "i16", torch.uint8: "u8"}        # labels of tensors a wrapper allocates: dtype:shape#ordinal


def configs():
    """(name, datapath, MX_MIN_K, {switch: value}): every datapath x (all defaults + each switch alone off its default); f16mx at both MX_MIN_K."""
    out = []
    for dp in ("fp32", "bf16", "bf16x3", "f16mx"):
        for mk in ((2560, 64) if dp == "f16mx" else (2560,)):
            out.append((f"{dp}/mk{mk}/default", dp, mk, {}))
            for s in SWITCHES:
                out.append((f"{dp}/mk{mk}/{s}={int(not DEFAULTS[s])}", dp, mk, {s: not DEFAULTS[s]}))
    return out


# ---------------------------------------------------------------------------------------------------------------- recording
class Registry:
    """Address -> label.  Holds every tensor it knows alive for the length of a case, so that no address is ever reused."""

    def __init__(self):
        self.spans, self.keep, self.counts = [], [], {}

    def add(self, t, label):
        st = t.untyped_storage()
        self.spans.append((st.data_ptr(), st.data_ptr() + max(st.nbytes(), 1), label))
        self.keep.append(t)
        return t

    def add_span(self, base, nbytes, label):
        self.spans.append((base, base + nbytes, label))

    def alloc(self, t):
        if isinstance(t, torch.Tensor) and t.numel():
            key = f"{_DT.get(t.dtype, t.dtype)}:{'x'.join(map(str, t.shape))}"
            k = self.counts[key] = self.counts.get(key, 0) + 1
            self.add(t, f"{key}#{k}")
        return t

    def ptr(self, v):
        if isinstance(v, ctypes.c_void_p):
            v = v.value
        if not v:
            return "null"
        for a, b, label in self.spans:
            if a <= v < b:
                return label if v == a else f"{label}+{v - a}"
        return "ext"                                # a temporary nobody registered (its address may be reused: no ordinal)


class Recorder:
    def __init__(self):
        self.reg, self.records = Registry(), []

    def __getattr__(self, name):
        if not name.startswith("ddpo_"):
            raise AttributeError(name)

        def call(*args):
            self.records.append([name] + [self.arg(a) for a in args])
            if name == "ddpo_sizeof_gemm_desc":
                return ctypes.sizeof(L.GemmDesc)
            if name == "ddpo_sizeof_ddim_consts":
                return ctypes.sizeof(L.DdimConsts)
            return FIXED.get(name, 0)
        return call

    def arg(self, a):
        if a is None or isinstance(a, ctypes.c_void_p):
            return self.reg.ptr(a)
        if isinstance(a, bool) or isinstance(a, int):
            return int(a)
        if isinstance(a, float):
            return float(a)
        obj = getattr(a, "_obj", None)              # ctypes.byref(...)
        if isinstance(obj, L.GemmDesc):
            d = {}
            for f, ty in L.GemmDesc._fields_:
                v = getattr(obj, f)
                v = self.reg.ptr(v) if ty is ctypes.c_void_p else v
                if v not in (0, 0.0, "null"):       # a field that is absent here IS zero / null: every field is compared
                    d[f] = v
            return {"desc": d}
        if isinstance(a, ctypes.Array) or hasattr(a, "value"):
            return self.reg.ptr(ctypes.cast(a, ctypes.c_void_p))
        return int(a)                               # numpy / torch integer scalars


class _Stream:
    cuda_stream = 0


class _Event:
    def __init__(self, enable_timing=False):
        pass

    def record(self):
        pass


class FakeRows:
    """Stand-in for a (rows, C) row-major fp32 tensor too large to allocate: shape, strides, address arithmetic and row slicing."""
    dtype = torch.float32
    device = torch.device("cpu")
    is_cuda = False

    def __init__(self, rows, C, base):
        self.shape, self._base = (int(rows), int(C)), base

    def dim(self):
        return 2

    def stride(self, i=None):
        s = (self.shape[1], 1)
        return s if i is None else s[i]

    def is_contiguous(self):
        return True

    def numel(self):
        return self.shape[0] * self.shape[1]

    def data_ptr(self):
        return self._base

    def __getitem__(self, sl):
        r0, r1, st = sl.indices(self.shape[0])
        assert st == 1
        return FakeRows(r1 - r0, self.shape[1], self._base + r0 * self.shape[1] * 4)


class FakeWeight:
    """Stand-in for a weight tensor in the predicate grid (only its address and shape are read); its PACKED entry is planted."""

    def __init__(self, ptr, shape):
        self._ptr, self.shape = ptr, tuple(shape)

    def data_ptr(self):
        return self._ptr

    def dim(self):
        return len(self.shape)


class Ctx:
    """One case: a fresh recorder / registry, lib's state reset, the config's switches set; everything restored on exit."""

    def __init__(self, dp, mk, sw, profile):
        self.dp, self.mk, self.sw, self.profile = dp, mk, sw, profile

    def __enter__(self):
        self.rec = Recorder()
        self.saved = {k: getattr(L, k) for k in SWITCHES + ("DATAPATH", "MX_MIN_K", "PROFILE", "_lib")}
        self.tsaved = (torch.empty, torch.zeros, torch.empty_like, torch.cuda.current_stream, torch.cuda.Event)
        for k, v in {**DEFAULTS, **self.sw}.items():
            setattr(L, k, v)
        L.DATAPATH, L.MX_MIN_K, L._lib = self.dp, self.mk, self.rec
        L.PROFILE = [] if self.profile else None
        L.PACKED.clear()
        L._ws_cache.clear()
        e, z, el = self.tsaved[:3]
        reg = self.rec.reg
        torch.empty = lambda *a, **k: reg.alloc(e(*a, **k))
        torch.zeros = lambda *a, **k: reg.alloc(z(*a, **k))
        torch.empty_like = lambda *a, **k: reg.alloc(el(*a, **k))
        torch.cuda.current_stream = lambda *a, **k: _Stream()
        torch.cuda.Event = _Event
        self.pfloat = L.Planes.float
        L.Planes.float = lambda pl: reg.add(self.pfloat(pl), f"float({reg.ptr(pl.hi.data_ptr())})")
        return self

    def __exit__(self, *exc):
        L.Planes.float = self.pfloat
        torch.empty, torch.zeros, torch.empty_like, torch.cuda.current_stream, torch.cuda.Event = self.tsaved
        for k, v in self.saved.items():
            setattr(L, k, v)
        L.PACKED.clear()
        L._ws_cache.clear()
        return False

    def t(self, label, *shape, dtype=torch.float32):
        return self.rec.reg.add(self.tsaved[1](*shape, dtype=dtype), label)

    def fake(self, label, rows, C):
        base = (1 << 56) + (len(self.rec.reg.spans) << 44)
        self.rec.reg.add_span(base, rows * C * 4, label)
        return FakeRows(rows, C, base)

    def w(self, label, *shape, bwd=True, pack=True):
        w = self.t(label, *shape)
        if pack:
            L.pack_weights(w, bwd=bwd)
        return w

    def ret(self, v):
        if isinstance(v, L.Planes):
            return {"planes": [v.rows, v.C, v.fmt, int(v.kblocked)], "hi": self.rec.reg.ptr(v.hi.data_ptr()), "lo": self.rec.reg.ptr(v.lo.data_ptr())}
        if isinstance(v, torch.Tensor):
            return {"tensor": list(v.shape), "dtype": str(v.dtype)[6:], "at": self.rec.reg.ptr(v.data_ptr())}
        if isinstance(v, (tuple, list)):
            return [self.ret(x) for x in v]
        if isinstance(v, dict):
            return {str(k): self.ret(x) for k, x in sorted(v.items(), key=lambda kv: str(kv[0]))}
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        return repr(type(v))


# ---------------------------------------------------------------------------------------------------------------- launch scenarios
M, K, N = 48, 64, 96
B, H, W, CI, CO = 2, 6, 6, 32, 64
ROWS = B * H * W
SCENARIOS = {}


def scenario(f):
    SCENARIOS[f.__name__] = f
    return f


def _entry_view(ent):
    """A PACKED entry without its tensors: keys, scalars and tensor shapes."""
    if isinstance(ent, dict):
        return {k: _entry_view(v) for k, v in sorted(ent.items())}
    if isinstance(ent, (tuple, list)):
        return [_entry_view(v) for v in ent]
    if isinstance(ent, torch.Tensor):
        return f"{str(ent.dtype)[6:]}{list(ent.shape)}"
    return ent


SCENARIOS["pack_dense"] = lambda cx: [_entry_view(L.pack_weights(cx.t("w", K, N), bwd=b)) for b in (True, False)] + [_entry_view(L.pack_weights(cx.t("w2", 40, 18)))]
SCENARIOS["pack_conv"] = lambda cx: [_entry_view(L.pack_weights(cx.t(f"w{int(b)}", 3, 3, CI, CO), bwd=b)) for b in (True, False)]


@scenario
def pack_repack(cx):
    w = cx.w("w", K, N)
    return _entry_view(L.pack_weights(w, bwd=False))


@scenario
def pack_geglu(cx):
    out = []
    for n in (256, 640, 96):
        w = cx.w(f"w{n}", K, n)
        out.append(L.pack_weights_geglu(w, cx.t(f"b{n}", n)))
        out.append(_entry_view(L.PACKED[w.data_ptr()]))
    out.append(L.pack_weights_geglu(cx.t("wu", K, 256), cx.t("bu", 256)))
    return out


@scenario
def pack_fold(cx):
    w = cx.w("w", 3, 3, CI, CO)
    r = [_entry_view(L.pack_weights_up2x_folded(w)), _entry_view(L.pack_weights_up2x_folded(cx.w("w16", 3, 3, 16, CO)))]
    L.pack_weights(w)
    return r + [_entry_view(L.PACKED[w.data_ptr()])]


SCENARIOS["pack_fold_unregistered"] = lambda cx: L.pack_weights_up2x_folded(cx.t("w", 3, 3, CI, CO))
SCENARIOS["pack_f16mx"] = lambda cx: _entry_view(L.pack_weights_f16mx(cx.t("w", K, N)))
SCENARIOS["linear_packed"] = lambda cx: L.linear(cx.t("x", M, K), cx.w("w", K, N), cx.t("b", N))
SCENARIOS["linear_unpacked"] = lambda cx: L.linear(cx.t("x", M, K), cx.t("w", K, N))
SCENARIOS["linear_k40"] = lambda cx: L.linear(cx.t("x", M, 40), cx.w("w", 40, 20), cx.t("b", 20))
SCENARIOS["linear_k36"] = lambda cx: L.linear(cx.t("x", M, 36), cx.w("w", 36, 20))
SCENARIOS["linear_w_trans"] = lambda cx: L.linear(cx.t("x", M, N), cx.w("w", K, N), w_trans=True)
SCENARIOS["gemm_rowbias_residual"] = lambda cx: L.gemm_conv(cx.t("x", M, K), cx.w("w", K, N), M=M, N=N, K=K, bias=cx.t("b", N), rowbias=cx.t("rb", 2, N), rows_per_batch=24,
                       residual=cx.t("res", 24, N), res_rows=24, alpha=0.5)


@scenario
def gemm_strided(cx):
    xb, ob, rb = cx.t("xbuf", M, 128), cx.t("obuf", M, 160), cx.t("rbuf", M, 192)
    return L.gemm_conv(xb[:, 16:16 + K], cx.w("w", K, N), M=M, N=N, K=K, ld_src=128, out=ob[:, 32:32 + N], ld_out=160, residual=rb[:, 8:8 + N], ld_res=192)


SCENARIOS["gemm_strided_view_no_ld"] = lambda cx: L.gemm_conv(cx.t("xbuf", M, 128)[:, 16:16 + K], cx.w("w", K, N), M=M, N=N, K=K)
SCENARIOS["gemm_huge_rows"] = lambda cx: L.gemm_conv(cx.t("x", M, K), cx.w("w", K, N), M=1 << 25, N=N, K=K, out=cx.t("o", M, N))
SCENARIOS["gemm_bad_src_3d"] = lambda cx: L.gemm_conv(cx.t("x", 2, 24, K), cx.w("w", K, N), M=M, N=N, K=K)


@scenario
def gemm_planes_out(cx):
    w = cx.w("w", K, N)
    return [L.gemm_conv(cx.t(f"x{i}", M, K), w, M=M, N=N, K=K, planes_out=po, planes_fmt=pf)
            for i, (po, pf) in enumerate((("both", 0), ("only", 0), ("both", 2), ("only", 2)))]


SCENARIOS["gemm_planes_out_unpacked"] = lambda cx: L.gemm_conv(cx.t("x", M, K), cx.t("w", K, N), M=M, N=N, K=K, planes_out="only")
SCENARIOS["gemm_planes_out_bad_value"] = lambda cx: L.gemm_conv(cx.t("x", M, K), cx.w("w", K, N), M=M, N=N, K=K, planes_out="yes")
SCENARIOS["gemm_planes_out_fmt2_n20"] = lambda cx: L.gemm_conv(cx.t("x", M, 40), cx.w("w", 40, 20), M=M, N=20, K=40, planes_out="both", planes_fmt=2)
SCENARIOS["gemm_planes_in_fmt0"] = lambda cx: L.linear(L.split_planes(cx.t("x", M, K), 0), cx.w("w", K, N), cx.t("b", N))
SCENARIOS["gemm_planes_in_fmt1"] = lambda cx: L.linear(L.split_planes(cx.t("x", M, K), 1), cx.w("w", K, N), cx.t("b", N), planes_out="both", planes_fmt=1)
SCENARIOS["gemm_planes_in_k40"] = lambda cx: L.linear(L.split_planes(cx.t("x", M, 40), 0), cx.w("w", 40, 20))
SCENARIOS["gemm_planes_in_unpacked"] = lambda cx: L.linear(L.split_planes(cx.t("x", M, K), 0), cx.t("w", K, N))


def _conv(cx, ksize, stride=1, upsample=False, cin=CI, cout=CO, src=None, **kw):
    x = cx.t("x", ROWS, cin) if src is None else src
    return L.conv2d(x, cx.w("w", ksize, ksize, cin, cout), cx.t("b", cout), B, H, W, cin, cout, ksize, stride=stride, upsample=upsample, **kw)


SCENARIOS["conv_1x1"] = lambda cx: _conv(cx, 1)
SCENARIOS["conv_3x3"] = lambda cx: _conv(cx, 3)
SCENARIOS["conv_3x3_pad0"] = lambda cx: _conv(cx, 3, pad=0)
SCENARIOS["conv_3x3_s2"] = lambda cx: _conv(cx, 3, stride=2)
SCENARIOS["conv_3x3_up"] = lambda cx: _conv(cx, 3, upsample=True)
SCENARIOS["conv_in_cin4"] = lambda cx: _conv(cx, 3, cin=4)
SCENARIOS["conv_out_n4"] = lambda cx: _conv(cx, 3, cout=4)
SCENARIOS["conv_3x3_planes"] = lambda cx: [_conv(cx, 3, src=L.split_planes(cx.t(f"x{f}", ROWS, CI), f), planes_out="only", planes_fmt=2 * f) for f in (0, 1)]
SCENARIOS["conv_3x3_residual_view"] = lambda cx: _conv(cx, 3, src=cx.t("xbuf", ROWS, 96)[:, 32:64], ld_src=96, residual=cx.t("res", ROWS, CO))


def _geglu(cx, n, rows=M, fmt=None, **kw):
    w = cx.w("w", K, n)
    L.pack_weights_geglu(w, cx.t("b", n))
    x = cx.t("x", rows, K)
    return L.linear_geglu(x if fmt is None else L.split_planes(x, fmt), w, **kw)


SCENARIOS["geglu_fp32"] = lambda cx: _geglu(cx, 256)
SCENARIOS["geglu_fp32_pre_out"] = lambda cx: _geglu(cx, 256, pre_out=True, out=cx.t("o", M, 128))
SCENARIOS["geglu_fp32_planes_out"] = lambda cx: [_geglu(cx, 256, planes_out=1), L.linear_geglu(cx.t("x2", M, K), cx.t("wu", K, 256))]
SCENARIOS["geglu_planes_fmt0"] = lambda cx: _geglu(cx, 640, fmt=0, planes_out=2, pre_out=True)
SCENARIOS["geglu_planes_fmt1"] = lambda cx: _geglu(cx, 640, fmt=1)
SCENARIOS["geglu_tall"] = lambda cx: _geglu(cx, 640, rows=25600, fmt=0, planes_out=1)
SCENARIOS["geglu_tall_below"] = lambda cx: _geglu(cx, 640, rows=25344, fmt=0)


@scenario
def geglu_stale(cx):
    w = cx.w("w", K, 256)
    L.pack_weights_geglu(w, cx.t("b", 256))
    L.pack_weights(w)
    return L.linear_geglu(cx.t("x", M, K), w)


@scenario
def geglu_two_gib(cx):
    w = cx.w("w", K, 256)
    L.pack_weights_geglu(w, cx.t("b", 256))
    return L.linear_geglu(cx.fake("x", 1 << 23, K), w)


def _fold(cx, x=None, cout=CO, pack=True, **kw):
    w = cx.w("w", 3, 3, CI, CO)
    if pack:
        L.pack_weights_up2x_folded(w)
    return L.conv2d_up2x_folded(cx.t("x", ROWS, CI) if x is None else x, w, cx.t("b", CO), B, H, W, CI, cout, **kw)


SCENARIOS["fold_fp32"] = lambda cx: _fold(cx)
SCENARIOS["fold_out_ld"] = lambda cx: _fold(cx, x=cx.t("xbuf", ROWS, 96)[:, 32:64], out=cx.t("obuf", 4 * ROWS, 128)[:, :CO], ld_out=128)


@scenario
def fold_planes(cx):
    r = []
    for f in (0, 1):
        with_err(r, lambda: _fold(cx, x=L.split_planes(cx.t(f"x{f}", ROWS, CI), f)))
    return r


SCENARIOS["fold_bad_geometry"] = lambda cx: _fold(cx, cout=CO // 2)
SCENARIOS["fold_bad_input"] = lambda cx: _fold(cx, x=cx.t("x", B, H * W, CI))
SCENARIOS["fold_unregistered"] = lambda cx: _fold(cx, pack=False)


def with_err(out, f):
    """Several launches in one scenario where any may raise: the exception is recorded in place and the scenario goes on."""
    try:
        out.append(f())
    except (L.DdpoHipError, ValueError) as e:
        out.append({"raised": type(e).__name__, "message": str(e)})


@scenario
def raw_f16mx_dense(cx):
    wp = L.pack_weights_f16mx(cx.t("w", K, N))
    pl = L.split_planes_f16mx(cx.t("x", M, K))
    return [L.gemm_conv_f16mx(pl, wp, M=M, bias=cx.t("b", N), residual=cx.t("res", M, N)), L.gemm_conv_f16mx(pl, wp, M=M, planes_out=True, out=cx.t("o", M, N))]


@scenario
def raw_f16mx_conv(cx):
    wp = L.pack_weights_f16mx(cx.t("w", 3, 3, CI, CO))
    conv = dict(ksize=3, stride=1, pad=1, upsample=0, B=B, H=H, W=W, Cin=CI, OH=H, OW=W)
    return L.gemm_conv_f16mx(L.split_planes_f16mx(cx.t("x", ROWS, CI)), wp, M=ROWS, conv=conv)


SCENARIOS["ldgrad_small"] = lambda cx: L.linear_dgrad(cx.t("dy", M, N), cx.w("w", K, N), residual=cx.t("res", M, K))
SCENARIOS["ldgrad_long"] = lambda cx: L.linear_dgrad(cx.t("dy", M, 2560), cx.w("w", 32, 2560))


@scenario
def ldgrad_planes(cx):
    w = cx.w("w", K, N)
    return [L.linear_dgrad(L.split_planes(cx.t(f"dy{f}", M, N), f), w) for f in (0, 1)] if L.current_datapath() != "fp32" and "dg" in L.PACKED[w.data_ptr()] \
        else L.linear_dgrad(cx.t("dy", M, N), w)


SCENARIOS["ldgrad_n20"] = lambda cx: L.linear_dgrad(cx.t("dy", M, 20), cx.w("w", 40, 20))
SCENARIOS["ldgrad_unpacked"] = lambda cx: L.linear_dgrad(cx.t("dy", M, N), cx.t("w", K, N), residual=cx.t("res", M, K))
SCENARIOS["ldgrad_fwd_only_pack"] = lambda cx: L.linear_dgrad(cx.t("dy", M, N), cx.w("w", K, N, bwd=False))


@scenario
def ldgrad_chunked(cx):
    rows = 420000
    return L.linear_dgrad(cx.fake("dy", rows, 1280), cx.w("w", 32, 1280), residual=cx.rec.reg.add(cx.tsaved[0](rows, 32), "res"))


@scenario
def ldgrad_chunk_too_wide(cx):
    w = FakeWeight(1 << 40, (32, 1 << 22))
    L.PACKED[w.data_ptr()] = dict(K=32, N=1 << 22, fwd=(None, None, 32), bwd=None, w_layout=1, dg=dict(K=1 << 22, N=32, hi=cx.t("dgh", 8), lo=cx.t("dgl", 8)))
    return L.linear_dgrad(cx.fake("dy", 128, 1 << 22), w)


def _cdgrad(cx, stride, h=H, pack=True, bwd=True, planes=None, res=False, cin=CI, cout=CO):
    oh = (h + 2 - 3) // stride + 1
    dy = cx.t("dy", B * oh * oh, cout)
    return L.conv2d_dgrad(dy if planes is None else L.split_planes(dy, planes), cx.w("w", 3, 3, cin, cout, pack=pack, bwd=bwd), B, h, h, cin, cout, 3,
                          stride=stride, residual=cx.t("res", B * h * h, cin) if res else None)


SCENARIOS["cdgrad_s1"] = lambda cx: _cdgrad(cx, 1, res=True)
SCENARIOS["cdgrad_s2"] = lambda cx: _cdgrad(cx, 2)
SCENARIOS["cdgrad_s2_odd"] = lambda cx: _cdgrad(cx, 2, h=5)
SCENARIOS["cdgrad_unpacked"] = lambda cx: _cdgrad(cx, 1, pack=False, res=True)
SCENARIOS["cdgrad_fwd_only_pack"] = lambda cx: _cdgrad(cx, 2, bwd=False)
SCENARIOS["cdgrad_planes"] = lambda cx: [_cdgrad(cx, 1, planes=0), _cdgrad(cx, 1, planes=1)]
SCENARIOS["cdgrad_cin4"] = lambda cx: _cdgrad(cx, 1, cin=4)
SCENARIOS["cdgrad_cout4"] = lambda cx: _cdgrad(cx, 1, cout=4)
SCENARIOS["wgrad_linear"] = lambda cx: L.linear_wgrad(cx.t("x", M, K), cx.t("dy", M, N), cx.t("dw", K, N), dbias=cx.t("db", N))
SCENARIOS["wgrad_small"] = lambda cx: [L.linear_wgrad(cx.t("x", M, 32), cx.t("dy", M, 16), cx.t("dw", 32, 16), dbias=cx.t("db", 16)),
            L.linear_wgrad(cx.t("x2", M, 64), cx.t("dy2", M, 16), cx.t("dw2", 64, 16)),
            L.linear_wgrad(cx.t("x3", M, 32), cx.t("dy3", M, 32), cx.t("dw3", 32, 32))]


@scenario
def wgrad_planes(cx):
    r = []
    for fs, fd in ((0, None), (1, None), (None, 0), (None, 1), (0, 0)):
        x, dy = cx.t(f"x{fs}{fd}", M, K), cx.t(f"dy{fs}{fd}", M, N)
        r.append(L.linear_wgrad(x if fs is None else L.split_planes(x, fs), dy if fd is None else L.split_planes(dy, fd), cx.t(f"dw{fs}{fd}", K, N),
                                dbias=cx.t(f"db{fs}{fd}", N)))
    return r


@scenario
def wgrad_planes_column_slice(cx):
    r = []
    with_err(r, lambda: L.gemm_wgrad(L.split_planes(cx.t("x", M, 128), 0), cx.t("dy", M, N), cx.t("dw", K, N), M=M, N=N, K=K, ld_src=128))
    with_err(r, lambda: L.gemm_wgrad(cx.t("x2", M, K), L.split_planes(cx.t("dy2", M, 128), 0), cx.t("dw2", K, N), M=M, N=N, K=K, ld_dy=128))
    return r


SCENARIOS["wgrad_options"] = lambda cx: [L.gemm_wgrad(cx.t("x", M, K), cx.t("dy", M, N), cx.t("dw", K, N), M=M, N=N, K=K, accumulate=False, alpha=2.0, dbias=cx.t("db", N)),
            L.gemm_wgrad(cx.t("xb", M, 128)[:, :K], cx.t("dyb", M, 128)[:, :N], cx.t("dw2", K, N), M=M, N=N, K=K, ld_src=128, ld_dy=128, splits=4,
                         dbias=cx.t("db2", N))]


@scenario
def wgrad_conv(cx):
    r = []
    for i, (s, up, pad) in enumerate(((1, False, None), (2, False, None), (1, True, None), (1, False, 0))):
        oh = ((2 * H if up else H) + 2 * (1 if pad is None else pad) - 3) // s + 1
        r.append(L.conv2d_wgrad(cx.t(f"x{i}", ROWS, CI), cx.t(f"dy{i}", B * oh * oh, CO), cx.t(f"dw{i}", 3, 3, CI, CO), B, H, W, CI, CO, 3, stride=s, pad=pad,
                                upsample=up, dbias=cx.t(f"db{i}", CO)))
    r.append(L.conv2d_wgrad(cx.t("xb", ROWS, 96)[:, 32:64], L.split_planes(cx.t("dyp", ROWS, CO), 0), cx.t("dwp", 3, 3, CI, CO), B, H, W, CI, CO, 3, ld_src=96))
    return r


@scenario
def groupnorm_forms(cx):
    g, b = cx.t("gamma", CI), cx.t("beta", CI)
    xb = cx.t("xbuf", ROWS, 96)
    return [L.groupnorm(cx.t("x", ROWS, CI), B, H * W, g, b, 8, 1e-5, True, return_stats=True),
            L.groupnorm(xb[:, 32:64], B, H * W, g, b, 8, 1e-5, False, out=cx.t("obuf", ROWS, 64), ld_out=64),
            L.groupnorm(xb[:, 32:64], B, H * W, g, b, 8, 1e-5, True, planes=1, return_stats=True),
            L.groupnorm(cx.t("x2", ROWS, CI), B, H * W, g, b, 8, 1e-5, False, planes=2, ld_x=CI)]


SCENARIOS["tile_counts"] = lambda cx: L.gemm_tile_launch_counts()
# ---------------------------------------------------------------------------------------------------------------- predicate grid


def layer_table():
    """(K, N, cin, dim) of every distinct conv / linear of the SD-1.5 and SD-2.1 U-Nets (cin = reduction channels per tap)."""
    pairs = [(4, 320), (320, 320), (320, 640), (640, 640), (640, 1280), (1280, 1280), (2560, 1280), (1920, 1280), (1920, 640), (1280, 640), (960, 640),
             (960, 320), (640, 320), (320, 4)]
    t = {(9 * ci, co, ci, 4) for ci, co in pairs}
    t |= {(ci, co, ci, 4) for ci, co in pairs[2:13] if ci != co}                                  # 1x1 shortcuts
    for c in (320, 640, 1280):
        t |= {(c, c, c, 2), (c, c, c, 4), (768, c, 768, 2), (1024, c, 1024, 2), (c, 8 * c, c, 2), (4 * c, c, 4 * c, 2), (1280, c, 1280, 2)}
    t |= {(320, 1280, 320, 2)}
    return sorted(t)


def row_table():
    return sorted({b * hw for b in (1, 2, 8, 16, 32) for hw in (64, 256, 1024, 4096)} | {77, 77 * 16})


def plant(K, N, cin, dim, ptr):
    """A FakeWeight and the PACKED entry the pack functions would leave for it (keys and scalars only: the predicates read nothing else)."""
    shape = (K, N) if dim == 2 else ((3, 3, cin, N) if K == 9 * cin else (1, 1, cin, N))
    w = FakeWeight(ptr, shape)
    lay = 1 if (L.W_KBLOCKED and N % 4 == 0) else 0
    ent = dict(K=K, N=N, fwd=(None, None, (K + 31) // 32 * 32 if lay else (K + 7) // 8 * 8), bwd=None, w_layout=lay)
    if K % 32 == 0 and K >= L.MX_MIN_K:
        ent["mx"] = {}
    if dim == 2 and N % 128 == 0 and K % 32 == 0:
        ent["geglu"] = dict(stale=False, w_layout=1, **({"tall": {}} if N % 320 == 0 else {}))
    if dim == 4 and K == 9 * cin and cin % 32 == 0 and N % 4 == 0:
        ent["fold"] = dict(K=4 * cin, N=N, stale=False, **({"mx": {}} if 4 * cin >= L.MX_MIN_K else {}))
    L.PACKED[ptr] = ent
    return w


def predicate_points():
    """(K, N, cin, dim, rows): the layer table at every row count, then points straddling each threshold."""
    pts = [(k, n, c, d, r) for k, n, c, d in layer_table() for r in row_table()]
    for k in (1279, 1280, 2559, 2560, 1248, 2528, 2592):
        pts += [(k, 1280, k, 2, r) for r in (32767, 32768, 4096)] + [(k, 1280, k, 4, 32768)]
    for n in (320, 640, 960, 1280, 2560, 5120, 10240):                                                 # 199 / 200 tall tiles, the 8 % efficiency edge
        per = n // 320
        for tiles in (199, 200, 201, 256, 257, 276, 277, 300, 384, 474, 475, 512, 513, 553, 554):
            r = -(-tiles // per) * 256
            pts += [(1280, n, 1280, 2, rr) for rr in (r - 256, r - 255, r, r + 1)] + [(320, n, 320, 2, r)]
    for c, k in ((320, 320), (320, 2880), (32, 32), (4, 36)):                                            # rows * cin * 4 at the 31-bit limit
        edge = -(-LIM // (c * 4))
        pts += [(k, 320, c, 4 if k != c else 2, r) for r in (edge - 1, edge, edge + 1)]
    pts += [(32, 320, 32, 4, r) for r in (LIM // 4, LIM // 4 + 1, (1 << 29) - 1, 1 << 29)]                # rows * 4 (folded up-sampler)
    pts += [(k, n, k, 2, 4096) for k, n in ((32768, 32767), (32768, 32768), (16384, 65535), (16384, 65536))]      # N * Kp * 2 at the limit
    pts += [(16384 * 9, n, 16384, 4, 4096) for n in (7280, 7284)]
    for n in (318, 319, 321, 322, 324, 640, 641, 642, 644):                                            # N % 320, N % 4
        pts += [(1280, n, 1280, 2, 65536), (2880, n, 320, 4, 65536)]
    for c in (8, 16, 24, 40, 48, 72, 96):                                                              # cin % 32
        pts += [(9 * c, 320, c, 4, 4096), (c, 320, c, 2, 65536)]
    return pts


def run_predicates(cx):
    pts = predicate_points()
    out = {k: [] for k in ("planes_ok", "planes_pay", "planes_out_ok", "norm_planes", "norm_planes_train", "geglu_tall_pays", "up2x_fold_ok", "up2x_planes_pay")}
    for i, (k, n, c, d, r) in enumerate(pts):
        w = plant(k, n, c, d, (1 << 40) + i * 64)
        out["planes_ok"].append(L.planes_ok(w, c, r))
        out["planes_pay"].append(L.planes_pay(w, c, r))
        out["planes_out_ok"].append(L.planes_out_ok(w, c, r, n))
        out["norm_planes"].append(L.norm_planes(w, c, r))
        out["norm_planes_train"].append(L.norm_planes(w, c, r, training=True))
        out["geglu_tall_pays"].append(L.geglu_tall_pays(w, r))
        out["up2x_fold_ok"].append(L.up2x_fold_ok(w, c, r))
        out["up2x_planes_pay"].append(L.up2x_planes_pay(w, c, r))
    unknown = FakeWeight(1 << 41, (64, 64))
    extra = [L.planes_ok(unknown, 64, 64), L.planes_pay(unknown, 64, 64), L.planes_out_ok(unknown, 64, 64, 64), L.geglu_tall_pays(unknown, 1 << 20),
             L.up2x_fold_ok(unknown, 64, 64), L.up2x_planes_pay(unknown, 64, 64), L.mx_layer(unknown), L.splitk_min_ktiles()]
    stale = plant(2880, 320, 320, 4, 1 << 42)
    L.PACKED[stale.data_ptr()]["fold"]["stale"] = True
    L.PACKED[stale.data_ptr()]["fold"].pop("mx", None)
    nomx = plant(2880, 640, 320, 4, (1 << 42) + 64)
    L.PACKED[nomx.data_ptr()]["fold"].pop("mx", None)
    extra += [L.up2x_fold_ok(stale, 320, 4096), L.up2x_fold_ok(nomx, 320, 4096), L.up2x_planes_pay(nomx, 320, 4096)]
    return {"points": len(pts), "extra": [int(v) for v in extra], **{k: "".join(str(int(v)) for v in vs) for k, vs in out.items()}}


# ---------------------------------------------------------------------------------------------------------------- driver


def run_case(dp, mk, sw, profile, fn):
    with Ctx(dp, mk, sw, profile) as cx:
        res = {}
        try:
            res["returned"] = cx.ret(fn(cx))
        except (L.DdpoHipError, ValueError) as e:
            res["raised"], res["message"] = type(e).__name__, str(e)
        res["records"] = cx.rec.records
        if profile:
            assert all(isinstance(p[0], _Event) and isinstance(p[1], _Event) and p[0] is not p[1] and len(p) == 5 for p in L.PROFILE)
            res["profile"] = [list(p[2:]) for p in L.PROFILE]                # (start event, end event, flops, family, io_bytes): the last three
        return res


def _rle(v, back=False):
    """Run-length coding of a predicate's answers over the grid: "0001" <-> "3a1b" (a / b / c = 0 / 1 / 2)."""
    if back:
        return "".join(str("abc".index(c)) * int(n) for n, c in re.findall(r"(\d+)([abc])", v))
    return "".join(f"{len(m.group(0))}{'abc'[int(m.group(1))]}" for m in re.finditer(r"(\d)\1*", v))


TABLES = ("descs", "records", "strings", "outcomes", "profiles", "results")


def generate():
    """The document that is written.  Everything distinct is stored once, in a table, and referred to by its index there: descriptors (`descs`),
    call records (`records`, a descriptor argument as {"desc": index}), predicate answer strings (`strings`, run-length coded), what a case
    returned or raised (`outcomes`), what it appended to PROFILE (`profiles`; null under PROFILE None) and `results` = [[record index, ...],
    outcome index, profile index]; "cases": {config: [result index, one per case]}.
    The cases of a config, in order: each scenario with PROFILE a list, for the all-default configs each scenario once more with PROFILE None,
    then the predicate grid."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                    # tiny tensors: a thread team per torch.zeros costs more than everything else here
    doc = {"scenarios": list(SCENARIOS), **{k: [] for k in TABLES}, "cases": {}}
    seen = {k: {} for k in TABLES}

    def intern(table, v):
        key = json.dumps(v, sort_keys=True)
        if key not in seen[table]:
            seen[table][key] = len(doc[table])
            doc[table].append(v)
        return seen[table][key]

    def put(name, res):
        recs = [intern("records", [{"desc": intern("descs", a["desc"])} if isinstance(a, dict) else a for a in r]) for r in res.pop("records")]
        ret = res.pop("returned", None)
        if isinstance(ret, dict) and "points" in ret:
            ret = {k: ({"string": intern("strings", _rle(v))} if isinstance(v, str) else v) for k, v in ret.items()}
        out = {"raised": [res["raised"], res["message"]]} if "raised" in res else {"returned": ret}
        doc["cases"].setdefault(name, []).append(intern("results", [recs, intern("outcomes", out), intern("profiles", res.get("profile"))]))

    try:
        for name, dp, mk, sw in configs():
            for profile in ((True,) if sw else (True, False)):
                for fn in SCENARIOS.values():
                    put(name, run_case(dp, mk, sw, profile, fn))
            put(name, run_case(dp, mk, sw, False, run_predicates))
    finally:
        torch.set_num_threads(threads)
    return doc


def expand(doc):
    """{case id: {"records", "returned" | "raised" + "message", "profile"}} of a generate() document, written out in full."""
    out = {}
    for name, ids in doc["cases"].items():
        names = [f"{s}/profile" for s in doc["scenarios"]]
        names += [f"{s}/noprofile" for s in doc["scenarios"]] if len(ids) > len(names) + 1 else []
        for cid, i in zip(names + ["predicates"], ids, strict=True):
            recs, outcome, profile = doc["results"][i]
            res = {"records": [[{"desc": doc["descs"][a["desc"]]} if isinstance(a, dict) else a for a in doc["records"][r]] for r in recs],
                   "profile": doc["profiles"][profile]}
            o = doc["outcomes"][outcome]
            if "raised" in o:
                res["raised"], res["message"] = o["raised"]
            else:
                ret = o["returned"]
                if isinstance(ret, dict) and "points" in ret:
                    ret = {k: (_rle(doc["strings"][v["string"]], back=True) if isinstance(v, dict) else v) for k, v in ret.items()}
                res["returned"] = ret
            out[f"{name}/{cid}"] = res
    return out


def dumps(doc):
    """Compact JSON, wrapped between table entries into lines of about 2000 characters."""
    js = lambda v: json.dumps(v, sort_keys=True, separators=(",", ":"))

    def wrapped(items):
        lines, cur = [], ""
        for it in items:
            if cur and len(cur) + len(it) > 2000:
                lines.append(cur)
                cur = ""
            cur += ("," if cur else "") + it
        return ",\n".join(lines + [cur])

    body = [f'"{k}":[\n{wrapped([js(r) for r in doc[k]])}\n]' for k in TABLES]
    cases = "{\n" + wrapped([f"{js(k)}:{js(v)}" for k, v in doc["cases"].items()]) + "\n}"
    return "{" + f'"scenarios":{js(doc["scenarios"])},\n' + ",\n".join(body) + f',\n"cases":{cases}' + "}\n"


if __name__ == "__main__":
    doc = generate()
    with open(GOLDEN, "w") as f:
        f.write(dumps(doc))
    print(f"wrote {sum(map(len, doc['cases'].values()))} cases ({len(doc['results'])} distinct results, {len(doc['records'])} distinct calls) to {GOLDEN}")
