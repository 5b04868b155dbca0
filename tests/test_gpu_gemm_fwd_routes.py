"""Every route, k-loop tail and output stage of the forward bf16 / f16mx GEMM family (ddpo_amd/csrc/gemm_bf16.hip: 36 instantiations of
gemm_conv_bf16_buf_kernel, the pointer-addressed gemm_conv_bf16_kernel, splitk_reduce_kernel, four output stages and the host rule that picks among
them), each at the smallest shape that enters it, held to EQUALITY with a float64 reference.

The method.  The operands are small integers times a power of two (tests/_gemm_fwd_cases.py: CLASSES), so every product and every partial sum is an
fp32-representable multiple of one unit and ANY summation order — of the k loop, of the split-K reduction, of the MFMA's lane halves — gives the same
bits.  The gate is `torch.equal(out, ref.float())`; one dropped, doubled or misplaced k-tile, row, column or fold phase breaks it on every datapath,
single-pass bf16 (whose 3e-2 gate elsewhere sees none of these) included.  The condition — sum_k |a_k||w_k| + |bias| + |rowbias| + |residual| below
2^24 units for every output element — is asserted on the draw before anything is launched.  Operand classes: `hi` (8 significant bits each; all four
datapaths), `a_lo` / `w_lo` (one operand 10-11 bits, the other 3: the a_lo w_hi / a_hi w_lo pass of bf16x3 carries data; single-pass bf16 is held to
bf16(a) bf16(w)), `both_lo` (bf16x3 against a_h w_h + a_h w_l + a_l w_h of the planes; the draw is sparse, see build_operands) and `mx_lo` (f16mx with
non-zero 8-bit low parts in ONE k-tile, cycled over the cases — not exact, held to the operator's contract of tests/test_gpu_f16mx.py:
max|out - product of the decoded planes| < 3e-6 max|ref|).  The gated GEGLU value is not exact (gelu_tanh_f is not): there the pre-activation must be
exact, the fused value bit-identical to lib.geglu(pre) and the emitted planes bit-identical to lib.split_planes(fused).

Every GPU case also checks: the tile-class counters (exactly one launch of the class the table names, generic_loader / splitk_reduce / f16mx as named),
sentinels around and in the padding columns of every output (fp32 rows, planes, aux_out), emitted planes == lib.split_planes(result), and that a second
launch into a fresh buffer gives the same bits.  `test_fwd_tables_enter_the_routes_they_name` (CPU) re-derives each row's expectation tuple from the
host rule with its constants read out of the .hip file and asserts that the tables reach every tile class, Datapath, KLoop and instantiation;
`test_fwd_gates_see_the_named_defects` (CPU) shows that each named defect is rejected by the gate of the case it would hit.

Branches of the host rule that no geometry reaches (none was given a shape): (1) splits_128 on the 128 x 128 tile — `big` implies t128 >= 256, the
grid it is asked about is that same count, and a split needs ngrid < 192, so a 128 x 128 grid is never split (the folded up-sampler counts all four
phases in both numbers alike; the GEGLU route asks for 1 split outright); (2) `if (splits < 1) splits = 1;` in wide_splits — under nblk <= 192 and
nk_total >= 16 both (256 + nblk / 2) / nblk and nk_total / 8 are at least 1.  The FOLD instantiations of the 128 x 320 and 128 x 128 tiles are
reachable but not entered here: the U-Net's real up-samplers in tests/test_gpu_upsample_fold.py run them, and only the k-loop tails are new in this file.
Expectation tuples that differ from the issue's table: none.  Rows added to it: a 3x3 convolution on the tall tile, N = 70 (the scalar stage of the
buffer-addressed kernel; the `unaligned` option set reaches the same stage on every other row, the tall tile included), a 1x1 generic convolution
with a K tail of 24, and data gradients with 24 output channels (the pointer-addressed kernel's `w_dgrad` addressing, AFFINE and zero-inserting).

Observed on an MI355X (941 tests of this file, 3.6 s wall):
    tall, wide, t128, t64, generic, conv (804 cases), data gradients (24), folded up-sampler (24), GEGLU 128 / tall (63 / 24 cases):
        every exact case bit-equal to the float64 reference on the first run, every emitted plane equal to lib.split_planes(result), every
        pre-activation exact, every fused GEGLU value equal to lib.geglu(pre), every sentinel intact, every counter delta as the tables name it,
        every second launch identical.  No defect was found in gemm_bf16.hip or in lib.py's launch path; nothing was changed there.
    f16mx low-part class (58 cases), worst max|out - decoded product| / max|ref| as a fraction of the 3e-6 gate, per table:
        tall 0.106 (3x3 convolution, nk = 9)   wide 0.068   t128 0.018   t64 0.003   conv 0.105
    (a lost cross-term k-tile is 70 - 94 x the gate on the two rows of the CPU defect test).
"""
import functools
import zlib

import pytest
import torch

import _gemm_fwd_cases as C
from _gemm_fwd_cases import OPTS, TABLES, geometry, gid
from ddpo_amd import lib as L

gpu = pytest.mark.gpu
DEV = "cuda"
SENT = 256                    # sentinel words in front of and behind every output
MX_GATE = 3e-6                # tests/test_gpu_f16mx.py: max|out - product of the decoded planes| < 3e-6 * max|ref|
TILE_KEYS = {"tall": "tall_256x320", "wide": "wide_128x320", "128": "t128x128", "64": "t128x64"}


# ------------------------------------------------------------------------------------------------ CPU: the tables enter the routes they name
def _row_dispatches(row):
    geom, feeds, expect = row
    M, N, K, cin, cv, _ = geometry(geom)
    return {feed: C.dispatch(M, N, K, cin, cv is not None, feed != "f", C.rule_constants()) for feed in feeds}


def test_fwd_tables_enter_the_routes_they_name():
    """The tuple beside each row is what dispatch_bf16() / launch_tile() make of it, with the rule's constants read from the source.  IF YOU CHANGE
    THE RULE: mirror it in _gemm_fwd_cases.dispatch() and move the rows so that each still enters the branch its comment names."""
    c = C.rule_constants()
    assert c == C._TODAY, c
    for name, table in TABLES.items():
        for row in table:
            for feed, got in _row_dispatches(row).items():
                assert got == row[2], (name, gid(row[0]), feed, got)
            M, N, K, cin, cv, _ = geometry(row[0])
            assert cin % 8 == 0 and ("f" in row[1] or cin % 32 == 0)
    for (B, H, W, Cc, N), expect in C.FOLD:
        assert C.dispatch(B * H * W, N, 4 * Cc, Cc, True, True, c, nph=4) == expect, (B, H, W, Cc, N)
    for (M, K, F), expect in C.GEGLU_128:
        assert C.dispatch(M, 2 * F, K, K, False, False, c, epilogue=1) == expect
    for (M, K, F), expect in C.GEGLU_TALL:
        assert C.dispatch(M, 2 * F, K, K, False, True, c, epilogue=2) == expect
        assert L._tall_tiles_fill(M, 2 * F)                               # lib.geglu_tall_pays' rule sends these rows to the tall tile
    # the edges the tables are there for
    exp = lambda t: [r[2] for r in TABLES[t]]
    assert {e[3] for e in exp("tall")} >= {1, 2, 3, 4, 5} and {e[5] for e in exp("tall")} >= {1, 179, 256}
    assert all(e[0] == "tall" for e in exp("tall")) and all(e[0] == "wide" for e in exp("wide")) and all(e[0] == "128" for e in exp("t128"))
    assert any(e[2] > 1 and e[4] % 2 and e[4] < e[3] for e in exp("wide")) and any(e[2] > 1 and e[5] < 128 for e in exp("wide"))     # an odd, short last split; ragged M under split-K
    assert any(e[2] == 1 and e[5] < 128 for e in exp("wide")) and any(geometry(r[0])[1] > 320 for r in TABLES["wide"])
    assert any(e[3] % 2 and e[3] > 64 for e in exp("t128")) and any(e[3] == 2 for e in exp("t128"))
    assert {e[3] for e in exp("t64") if e[2] == 1} >= {1, 2, 3} and {e[6] for e in exp("t64")} >= {4, 6, 8, 64}
    assert any(e[2] > 1 and e[6] == 4 for e in exp("t64")) and any(e[2] > 1 and e[4] == 3 for e in exp("t64")) and any(e[2] == 8 and e[5] < 128 for e in exp("t64"))
    assert all(e[1] for e in exp("generic")) and not any(e[1] for t in TABLES if t != "generic" for e in exp(t))
    assert any(e[2] > 1 for e in exp("generic")) and any(geometry(r[0])[2] % 32 == 8 for r in TABLES["generic"])
    gconv = [r[0] for r in TABLES["generic"] if r[0][0] == "conv"]
    assert {g[4] for g in gconv} >= {8, 24, 40} and any(g[7] == 2 for g in gconv) and any(g[8] for g in gconv) and any(g[2] != g[3] for g in gconv)
    bconv = [r[0] for r in TABLES["conv"]]
    assert {(g[6], g[7], bool(g[8])) for g in bconv} == {(3, 1, False), (1, 1, False), (3, 2, False), (1, 2, False), (3, 1, True)}
    assert {g[4] for g in bconv} >= {32, 96} and any(g[2] != g[3] for g in bconv)
    # every option the issue names on each of the four output stages
    seen = {}
    for name in TABLES:
        for i, variant, opt in C.cases(name):
            geom, _, expect = TABLES[name][i]
            seen.setdefault(C.stage_of(expect, opt, geometry(geom)[1]), set()).add(opt)
    for stage in ("scalar", "vector", "reduce", "tall"):
        assert set(C.REQUIRED) <= seen[stage], (stage, set(C.REQUIRED) - seen[stage])
    for stage in ("vector", "reduce", "tall"):
        assert set(C.PLANE_OPTS) <= seen[stage], (stage, set(C.PLANE_OPTS) - seen[stage])
    # coverage: every tile class, Datapath, KLoop and instantiation of the table at the head of the kernel
    dps, kls, universe = C.kernel_table()
    assert len(universe) == 36, len(universe)
    reached = set()
    for name in TABLES:
        for i, (feed, wkb, dp, cls), opt in C.cases(name):
            tile = TABLES[name][i][2][0]
            reached.add((tile, C.kloop_of(tile, feed, dp), C.DP_ENUM[dp], False))
    for _, expect in C.FOLD:
        for dp in FOLD_DPS:
            reached.add((expect[0], C.kloop_of(expect[0], "p", dp), C.DP_ENUM[dp], True))
    for dp in ("bf16", "bf16x3", "f16mx"):
        reached.add(("128", "planes3w", C.DP_ENUM[dp], False))
    for dp in ("bf16x3", "f16mx"):
        reached.add(("tall", C.kloop_of("tall", "p", dp, geglu=True), C.DP_ENUM[dp], False))
    assert reached <= universe, reached - universe
    assert {t for t, _, _, _ in reached} == {"tall", "wide", "128", "64"}
    assert {d for _, _, d, _ in reached} == set(dps) and {k for _, k, _, _ in reached} == set(kls)
    # FOLD instantiations of the wide and 128 x 128 tiles are left to tests/test_gpu_upsample_fold.py (the U-Net's real up-samplers)
    missing = universe - reached
    assert all(fold and tile in ("wide", "128") for tile, _, _, fold in missing), missing


# ------------------------------------------------------------------------------------------------ CPU: the gates see the defects
def _cpu_case(geom, cls, optname, tile=0):
    a, w = C.build_operands(geom, cls, "cpu", tile)
    e = C.build_epilogue(geom, optname, "cpu")
    return a, w, e, C.apply_epilogue(C.product(geom, a, w), e)


def test_fwd_gates_see_the_named_defects():
    """What a defective kernel would return, formed in float64 for two small rows: for the exact classes each defect changes the fp32 image of the
    result (the gate is equality); for the f16mx low-part class a lost cross-term tile is at least 4 x the 3e-6 gate.  (No defective kernel is built.)"""
    dgeom = C.dense(256, 1056, 128)            # T64 split row: 4 splits of 10 k-tiles, the last 3
    cgeom = C.conv(2, 16, 16, 32, 64)          # CONV row: a tap per k-tile
    for cls in ("hi", "a_lo", "both_lo"):
        a, w, e, ref = _cpu_case(dgeom, cls, "both")
        M, N, K = 256, 128, 1056
        good = ref.float()
        assert torch.equal(good.double(), ref), "the reference itself is not fp32-exact"
        kw = torch.ones(K, dtype=torch.float64)
        defects = {}
        for name, (k0, k1, f) in dict(dropped=(320, 352, 0.0), twice=(320, 352, 2.0), tail=(1024, 1056, 0.0)).items():
            k = kw.clone(); k[k0:k1] = f
            defects["k-tile " + name] = C.apply_epilogue(C.product(dgeom, a, w, k), e)
        defects["rowbias skipped next to a residual"] = C.apply_epilogue(C.product(dgeom, a, w), dict(e, rowbias=None))
        ea = C.build_epilogue(dgeom, "alpha", "cpu")
        defects["alpha ignored"] = (C.apply_epilogue(C.product(dgeom, a, w), dict(ea, alpha=1.0)), C.apply_epilogue(C.product(dgeom, a, w), ea))
        ep = C.build_epilogue(dgeom, "period", "cpu")
        defects["wrong residual period"] = (C.apply_epilogue(C.product(dgeom, a, w), dict(ep, res_rows=M // 4)), C.apply_epilogue(C.product(dgeom, a, w), ep))
        for what, bad in defects.items():
            bad, want = bad if isinstance(bad, tuple) else (bad, ref)
            n = int((bad.float() != want.float()).sum())
            print(f"[gemm fwd routes] defect ({cls}): {what}: {n} of {want.numel()} elements differ")
            assert n > 0, (cls, what)
    # a border row unmasked: tap (ky = 0, kx = 1) of output row 0 of image 1 reads the last row of image 0 instead of zeros
    a, w, e, ref = _cpu_case(cgeom, "hi", "bias")
    B, H, W, Cin = cgeom[1:5]
    leak = ref.clone().view(B, H, W, -1)
    leak[1, 0] += a.view(B, H, W, Cin)[0, H - 1] @ w[1 * Cin:2 * Cin]
    assert not torch.equal(leak.view_as(ref).float(), ref.float())
    # one fold phase swapped: phases 1 and 2 of the folded up-sampler written to each other's pixels
    Bf, Hf, Wf, Cf, Nf = C.FOLD[0][0]
    x, wf = _fold_operands(C.FOLD[0][0], "cpu")
    full = _fold_reference(x, wf).view(Bf, 2 * Hf, 2 * Wf, Nf)
    swapped = full.clone()
    swapped[:, 0::2, 1::2], swapped[:, 1::2, 0::2] = full[:, 1::2, 0::2], full[:, 0::2, 1::2]
    assert not torch.equal(swapped.float(), full.float())
    # one row written past M: the first float behind the output, and a padding column, are sentinels
    buf0 = torch.randn(2 * SENT + 4 * 8)
    for pos in (SENT + 32, SENT + 6):
        buf = buf0.clone()
        buf[pos] += 1e-3
        out = buf[SENT:SENT + 32].view(4, 8)
        out[:, :6] = buf0[SENT:SENT + 32].view(4, 8)[:, :6]                       # the payload restored: what _restore_and_compare does
        assert not torch.equal(buf.view(torch.int32), buf0.view(torch.int32))
    # f16mx low parts: a lost cross-term k-tile against the 3e-6 gate (host emulation of the planes' rounding: f16 / e5m2 / column-scaled e4m3)
    for geom in (dgeom, cgeom):
        worst = None
        M, N, K, cin, cv, rows = geometry(geom)
        for tile in range(0, K // 32, max(1, K // 32 // 3)):
            a, w = C.build_operands(geom, "mx_lo", "cpu", tile)
            ah, ah8, al8 = _mx_split_host(a)
            wh, wh8, wl8 = _mx_split_host_w(w)
            ref = C.product(geom, ah, wh) + C.product(geom, ah8, wl8) + C.product(geom, al8, wh8)
            kw = torch.ones(K, dtype=torch.float64)
            kw[32 * tile:32 * tile + 32] = 0.0
            lost = (C.product(geom, ah8, wl8) + C.product(geom, al8, wh8)) - (C.product(geom, ah8, wl8, kw) + C.product(geom, al8, wh8, kw))
            ratio = float(lost.abs().max() / (MX_GATE * ref.abs().max()))
            worst = ratio if worst is None else min(worst, ratio)
        print(f"[gemm fwd routes] defect (mx_lo) {gid(geom)}: a lost cross-term k-tile is {worst:.1f} x the gate")
        assert worst >= 4.0, (gid(geom), worst)


def _mx_split_host(a):
    """(h, h8, l8) float64 of the f16mx activation planes of a (float64 holding fp32 values), as ddpo_split_planes_f16mx forms them."""
    a32 = a.float()
    h = a32.half()
    l = (a32 - h.float()) * 2048.0
    return h.double(), h.float().to(torch.float8_e5m2).double(), l.to(torch.float8_e5m2).double() / 2048.0


def _mx_split_host_w(w):
    """(h, h8, l8) float64 of the f16mx weight planes of w (K, N): e4m3 at the column's scale 2^(floor(log2 max|w|) - 7)."""
    w32 = w.float()
    h = w32.half()
    s = torch.pow(2.0, torch.floor(torch.log2(w32.abs().amax(0).clamp_min(2.0 ** -95))) - 7)
    q = lambda v: ((v / s).to(torch.float8_e4m3fn).float() * s).double()
    return h.double(), q(h.float()), q((w32 - h.float()) * 2048.0) / 2048.0


# ------------------------------------------------------------------------------------------------ GPU: operands, references (cached, never modified)
@functools.lru_cache(maxsize=3)
def _operands(geom, cls, tile):
    a, w = C.build_operands(geom, cls, DEV, tile)
    a32, w32 = a.float().contiguous(), w.float().contiguous()
    assert torch.equal(a32.double(), a) and torch.equal(w32.double(), w)
    return a, w, a32, w32


def _split64(t):
    """bf16 hi / lo planes of t as float64: hi = bf16(t), lo = bf16(t - hi)."""
    hi = C.bf16_round(t)
    return hi, C.bf16_round(t - hi)


@functools.lru_cache(maxsize=4)
def _product(geom, cls, kind, tile):
    """The float64 contraction the datapath `kind` owes: "full" a w; "hh" bf16(a) bf16(w); "x3" a_h w_h + a_h w_l + a_l w_h."""
    a, w, _, _ = _operands(geom, cls, tile)
    if kind == "full":
        return C.product(geom, a, w)
    (ah, al), (wh, wl) = _split64(a), _split64(w)
    if kind == "hh":
        return C.product(geom, ah, wh)
    return C.product(geom, ah, wh) + C.product(geom, ah, wl) + C.product(geom, al, wh)


@functools.lru_cache(maxsize=None)
def _absprod_max(geom, cls):
    a, w, _, _ = _operands(geom, cls, 0)
    return float(C.product(geom, a.abs(), w.abs()).max())


def _fenced(n, dtype, seed, shift=0):
    """(buffer, payload view of n elements): random words with SENT of them on either side of the payload (shift: payload one element further)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    if dtype == torch.float32:
        buf = torch.randn(n + 2 * SENT + 1, device=DEV, generator=g)
    else:
        buf = torch.randint(-32768, 32768, (n + 2 * SENT + 1,), device=DEV, generator=g, dtype=torch.int32).to(torch.int16)
    return buf, buf[SENT + shift:SENT + shift + n]


def _restore_and_compare(buf, before, payload, payload_before, ncols=None):
    """Takes the written part out of `payload` (all of it, or its first ncols columns), puts the old words back and compares the WHOLE buffer bit for
    bit: whatever else the launch wrote — in front, behind, in the padding columns — shows.  Returns the written part."""
    got = (payload if ncols is None else payload[:, :ncols]).clone()
    if ncols is None:
        payload.copy_(payload_before)
    else:
        payload[:, :ncols] = payload_before[:, :ncols]
    bits = torch.int32 if buf.dtype == torch.float32 else torch.int16
    assert torch.equal(buf.view(bits), before.view(bits)), "a write outside the output"
    return got


def _counts_delta(before, after):
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def _expected_counts(expect, dp):
    want = {TILE_KEYS[expect[0]]: 1}
    if expect[1]:
        want["generic_loader"] = 1
    if expect[2] > 1:
        want["splitk_reduce"] = 1
    if dp == "f16mx":
        want["f16mx"] = 1
    return want


def _where(bad):
    """Which rows / columns of a result differ: the pattern that locates a defect."""
    r, c = bad.any(1).nonzero().flatten(), bad.any(0).nonzero().flatten()
    return f"{int(bad.sum())} elements differ: rows {int(r[0])}..{int(r[-1])} ({r.numel()}), columns {int(c[0])}..{int(c[-1])} ({c.numel()})"


def _weights(w32, dp, wkb, monkeypatch):
    """(weights argument of lib._launch_fwd, w_layout)."""
    monkeypatch.setattr(L, "W_KBLOCKED", bool(wkb))
    if dp in ("f16mx", "f16x1"):
        return L.pack_weights_f16mx(w32), 1
    L.DATAPATH = dp
    ent = L.pack_weights(w32, bwd=False)
    assert ent["w_layout"] == (1 if wkb and w32.shape[1] % 4 == 0 else 0)
    return (ent["fwd"][0], ent["fwd"][1], ent["fwd"][2], 3 if dp == "bf16x3" else 1), ent["w_layout"]


def _launch(geom, variant, e, o, a32, weights, w_layout, monkeypatch, seed):
    """One launch into fenced outputs.  Returns (result (M, N) fp32 or None, (hi, lo) flat int16 plane payloads or None)."""
    feed, wkb, dp, cls = variant
    M, N, K, cin, cv, rows = geometry(geom)
    mx = dp in ("f16mx", "f16x1")
    monkeypatch.setattr(L, "A_KBLOCKED", feed == "k")
    act = None if feed == "f" else L.split_planes(a32, fmt=1 if mx else 0)
    if act is not None:
        assert act.kblocked == (feed == "k")
    dev = lambda t: None if t is None else t.float().contiguous()
    bias, rowbias, residual = dev(e["bias"]), dev(e["rowbias"]), dev(e["residual"])
    planes = o.get("planes")
    ld_out = N + o.get("ld_pad", 0)
    out_buf = out = None
    if not planes or planes[0] == "both":
        out_buf, flat = _fenced(M * ld_out, torch.float32, seed, 1 if o.get("unaligned") else 0)
        out = flat.view(M, ld_out)
        out_before, out0 = out_buf.clone(), out.clone()
    opl = None
    if planes:
        _, pkb, pfmt = planes
        pbufs = [_fenced(M * N, torch.int16, seed + 1 + i) for i in range(2)]
        pbefore = [(b.clone(), p.clone()) for b, p in pbufs]
        opl = (pbufs[0][1], pbufs[1][1], 0 if pkb else N, pfmt)
    d = L._gemm_desc(M, N, K, conv=cv, src=a32 if feed == "f" else None, ld_src=cin if feed == "f" else 0, out=out, ld_out=ld_out, bias=bias,
                     residual=residual, ld_res=e["ld_res"], res_rows=e["res_rows"], alpha=e["alpha"], out_planes=opl)
    if rowbias is not None:
        d.rowbias, d.rows_per_batch, d.ld_rowbias = rowbias.data_ptr(), e["rows_per_batch"], N
    monkeypatch.delenv("DDPO_MX_TALL", raising=False)
    L._launch_fwd(d, act, weights, w_layout=w_layout, cross=(dp == "f16mx") if mx else None, ws_device=a32.device)
    torch.cuda.synchronize()
    res = None if out is None else _restore_and_compare(out_buf, out_before, out, out0, N)
    pl = None
    if planes:
        pl = tuple(_restore_and_compare(b, b0, p, p0) for (b, p), (b0, p0) in zip(pbufs, pbefore))
    return res, pl


def _run_case(table, index, variant, optname, monkeypatch):
    from conftest import parity_record
    geom, feeds, expect = TABLES[table][index]
    feed, wkb, dp, cls = variant
    M, N, K, cin, cv, rows = geometry(geom)
    o = dict(OPTS[optname])
    if cls == "mx_lo" and o.get("planes", ("both",))[0] == "only":
        o["planes"] = ("both",) + o["planes"][1:]                      # the inexact class is compared through its fp32 result
    tile = zlib.crc32(repr((geom, optname)).encode()) % (K // 32) if cls == "mx_lo" else 0
    a, w, a32, w32 = _operands(geom, cls, tile)
    e = C.build_epilogue(geom, optname, DEV)
    weights, w_layout = _weights(w32, dp, wkb, monkeypatch)
    # ---- the reference and the input guard
    if cls == "mx_lo":
        monkeypatch.setattr(L, "A_KBLOCKED", False)
        ah, ah8, al8 = C.dec_planes(*L.split_planes_f16mx(a32))
        wh, wh8, wl8 = C.dec_weights(weights)
        assert float(al8.abs().max()) > 0 and float(wl8.abs().max()) > 0 and int((al8 != 0).any(0).sum()) == 32 and int((wl8 != 0).any(1).sum()) == 32
        ref = C.apply_epilogue(C.product(geom, ah, wh) + C.product(geom, ah8, wl8) + C.product(geom, al8, wh8), e)
    else:
        frac = C.exactness_bound(geom, cls, _absprod_max(geom, cls), e)
        assert frac < 1.0, f"the draw is not exact in fp32: {frac:.2f} of 2^24"
        kind = "hh" if dp == "bf16" and cls != "hi" else ("x3" if cls == "both_lo" else "full")
        if cls == "both_lo":                                           # the planes the kernel is fed are the split this reference assumes
            f = lambda t: (t.to(torch.int32) << 16).view(torch.float32).double()
            monkeypatch.setattr(L, "A_KBLOCKED", False)
            pa = L.split_planes(a32)
            (ah, al), (wh, wl) = _split64(a), _split64(w)
            assert torch.equal(f(pa.hi), ah) and torch.equal(f(pa.lo), al)
            unpack = (lambda t: f(t).reshape(-1, N, 32).permute(0, 2, 1).reshape(-1, N)[:K]) if w_layout == 1 else (lambda t: f(t).t()[:K])
            assert torch.equal(unpack(weights[0]), wh) and torch.equal(unpack(weights[1]), wl)
        ref = C.apply_epilogue(_product(geom, cls, kind, tile), e)
        assert torch.equal(ref.float().double(), ref), "the reference is not fp32-representable"
    # ---- launch, counters, sentinels (inside _launch)
    before = L.gemm_tile_launch_counts()
    res, pl = _launch(geom, variant, e, o, a32, weights, w_layout, monkeypatch, zlib.crc32(repr((geom, variant, optname)).encode()))
    delta = _counts_delta(before, L.gemm_tile_launch_counts())
    assert delta == _expected_counts(expect, dp), (delta, expect)
    # ---- result
    line = f"{table} {gid(geom)} [{feed} w{'kb' if wkb else 'rm'} {dp} {cls} {optname}] {expect[0]}{' generic' if expect[1] else ''} splits {expect[2]} nk {expect[3]}/{expect[4]}"
    if cls == "mx_lo":
        err = float((res.double() - ref).abs().max() / ref.abs().max())
        parity_record(f"[gemm fwd routes] {line}: k-tile {tile}: {err:.2e} = {err / MX_GATE:.3f} of the gate")
        assert err < MX_GATE, err
        want = res
    else:
        want = ref.float()
        if res is not None:
            bad = res != want
            assert not bool(bad.any()), line + ": " + _where(bad)
    if pl is not None:
        monkeypatch.setattr(L, "A_KBLOCKED", bool(o["planes"][1]))
        exp = L.split_planes(want.contiguous(), fmt=o["planes"][2])
        assert exp.kblocked == bool(o["planes"][1])
        for got, plane, name in ((pl[0], exp.hi, "hi"), (pl[1], exp.lo, "lo")):
            bad = got != plane.reshape(-1)
            assert not bool(bad.any()), f"{line}: {name} plane: {int(bad.sum())} words differ, first at {int(bad.nonzero()[0])}"
    # ---- determinism: a second launch into fresh buffers
    res2, pl2 = _launch(geom, variant, e, o, a32, weights, w_layout, monkeypatch, 12345)
    assert (res is None and res2 is None) or torch.equal(res, res2)
    assert pl is None or (torch.equal(pl[0], pl2[0]) and torch.equal(pl[1], pl2[1]))


def _case_params(table):
    cs = C.cases(table)
    ids = [f"{gid(TABLES[table][i][0])}-{v[0]}-{'wkb' if v[1] else 'wrm'}-{v[2]}-{v[3]}-{o}" for i, v, o in cs]
    return pytest.mark.parametrize("index,variant,optname", cs, ids=ids)


@gpu
@_case_params("tall")
def test_fwd_tall_tile_is_exact(index, variant, optname, monkeypatch):
    _run_case("tall", index, variant, optname, monkeypatch)


@gpu
@_case_params("wide")
def test_fwd_wide_tile_is_exact(index, variant, optname, monkeypatch):
    _run_case("wide", index, variant, optname, monkeypatch)


@gpu
@_case_params("t128")
def test_fwd_128x128_tile_is_exact(index, variant, optname, monkeypatch):
    _run_case("t128", index, variant, optname, monkeypatch)


@gpu
@_case_params("t64")
def test_fwd_128x64_tile_is_exact(index, variant, optname, monkeypatch):
    _run_case("t64", index, variant, optname, monkeypatch)


@gpu
@_case_params("generic")
def test_fwd_pointer_addressed_kernel_is_exact(index, variant, optname, monkeypatch):
    _run_case("generic", index, variant, optname, monkeypatch)


@gpu
@_case_params("conv")
def test_fwd_buffer_path_convolutions_are_exact(index, variant, optname, monkeypatch):
    _run_case("conv", index, variant, optname, monkeypatch)


# ------------------------------------------------------------------------------------------------ data gradients
@gpu
@pytest.mark.parametrize("fwd_form", [False, True], ids=["w_dgrad", "dgrad_fwd"])
@pytest.mark.parametrize("cls", ["hi", "a_lo", "w_lo"])
@pytest.mark.parametrize("geom", C.DGRAD, ids=gid)
def test_fwd_data_gradient_is_exact(geom, cls, fwd_form, monkeypatch):
    """lib.conv2d_dgrad on bf16x3: the fp32-fed kernel's `w_dgrad` addressing of the (K, N) planes (lib.DGRAD_FWD off; stride 2: zero insertion in
    the gather) and the forward form on the registered data-gradient planes, on the buffer-addressed kernel (Cout = 64) and on both forms of the
    pointer-addressed one (Cout = 24: AFFINE at stride 1, not at stride 2), against dX = conv_transpose(dY, W) in float64."""
    _, B, H, W, Cin, Cout, ks, stride, _ = geom
    M, N, K, cin, cv, rows = geometry(geom)
    monkeypatch.setattr(L, "DGRAD_FWD", fwd_form)
    monkeypatch.setattr(L, "A_KBLOCKED", False)
    L.DATAPATH = "bf16x3"
    # dY (M, Cout) takes the activation's role, W (3, 3, Cin, Cout) the weight's
    dy, w, dy32, w32 = _operands(C.conv(B, cv["OH"], cv["OW"], Cout, Cin, ks), cls, 0)
    w4 = w.view(ks, ks, Cout, Cin).permute(0, 1, 3, 2).contiguous()                  # an HWIO kernel (ks, ks, Cin, Cout) with the drawn values
    w4_32 = w4.float().contiguous()
    ent = L.pack_weights(w4_32, bwd=True)
    buf = Cout % 32 == 0                                # the reduction channels of the data gradient are the layer's OUTPUT channels
    assert ("dg" in ent) == (fwd_form and buf)          # (lib.pack_weights registers forward-form planes only for whole 32-channel blocks)
    ct = lambda t, k: torch.nn.functional.conv_transpose2d(t.cpu().view(B, cv["OH"], cv["OW"], Cout).permute(0, 3, 1, 2), k.cpu().permute(3, 2, 0, 1), stride=stride,
                                                           padding=ks // 2, output_padding=stride - 1).permute(0, 2, 3, 1).reshape(B * H * W, Cin).to(DEV)
    ref, bound = ct(dy, w4), float(ct(dy.abs(), w4.abs()).max())
    _, au, _, wu = C.CLASSES[cls]
    assert 1.02 * bound / (au * wu) < C.LIMIT
    before = L.gemm_tile_launch_counts()
    dx = L.conv2d_dgrad(dy32, w4_32, B, H, W, Cin, Cout, ks, stride=stride)
    torch.cuda.synchronize()
    delta = _counts_delta(before, L.gemm_tile_launch_counts())
    assert delta == ({"t128x64": 1} if buf else {"t128x64": 1, "generic_loader": 1}), delta
    bad = dx != ref.float()
    assert not bool(bad.any()), _where(bad)
    assert torch.equal(dx, L.conv2d_dgrad(dy32, w4_32, B, H, W, Cin, Cout, ks, stride=stride))


# ------------------------------------------------------------------------------------------------ folded up-sampler
FOLD_DPS = ("bf16", "bf16x3", "f16mx")


def _fold_operands(case, device):
    B, H, W, Cc, N = case
    a, w = C.build_operands(C.conv(B, H, W, Cc, N, 3, 1, True), "hi", device)
    return a.view(B, H, W, Cc), w.view(3, 3, Cc, N)


def _fold_reference(x, w):
    """conv3x3(nearest_upsample_2x(x)) in float64: (B 2H 2W, N)."""
    B, H, W, Cc = x.shape
    return C.product(C.conv(B, H, W, Cc, w.shape[3], 3, 1, True), x.reshape(-1, Cc), w.reshape(-1, w.shape[3]))


@gpu
@pytest.mark.parametrize("feed", ["p", "k"])
@pytest.mark.parametrize("dp", FOLD_DPS)
@pytest.mark.parametrize("case,expect", C.FOLD, ids=[gid(c) for c, _ in C.FOLD])
def test_fwd_folded_upsampler_tails_are_exact(case, expect, dp, feed, monkeypatch):
    """The folded up-sampler's four-phase launches at the k-loop tails the tables name (hi class: the pre-summed phase kernels are sums of at most
    four integers below 16, still 8 bits), into a strided destination with sentinels."""
    B, H, W, Cc, N = case
    monkeypatch.setattr(L, "A_KBLOCKED", feed == "k")
    monkeypatch.setattr(L, "MX_MIN_K", 32)
    L.DATAPATH = dp
    x, w = _fold_operands(case, DEV)
    x32, w32 = x.float().reshape(-1, Cc).contiguous(), w.float().contiguous()
    L.pack_weights(w32, bwd=False)
    assert L.pack_weights_up2x_folded(w32) is not None and L.up2x_fold_ok(w32, Cc, B * H * W)
    fmt = L.up2x_planes_pay(w32, Cc, B * H * W)
    assert fmt == (2 if dp == "f16mx" else 1)
    bias = (torch.randint(-63, 64, (N,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(N)).double() * C.EPI_UNIT)
    ref = _fold_reference(x, w) + bias
    bound = float(_fold_reference(x.abs(), w.abs()).max()) + 4.0
    assert 1.02 * bound / (2.0 ** -11) < C.LIMIT
    M, ld = 4 * B * H * W, N + 64
    results = []
    for seed in (1, 2):
        buf, flat = _fenced(M * ld, torch.float32, seed)
        out = flat.view(M, ld)
        buf0, out0 = buf.clone(), out.clone()
        before = L.gemm_tile_launch_counts()
        L.conv2d_up2x_folded(L.split_planes(x32, fmt=fmt - 1), w32, bias.float(), B, H, W, Cc, N, out=out, ld_out=ld)
        torch.cuda.synchronize()
        delta = _counts_delta(before, L.gemm_tile_launch_counts())
        assert delta == _expected_counts(expect, dp), (delta, expect)
        results.append(_restore_and_compare(buf, buf0, out, out0, N))
    bad = results[0] != ref.float()
    assert not bool(bad.any()), _where(bad)
    assert torch.equal(results[0], results[1])


# ------------------------------------------------------------------------------------------------ GEGLU output stages
def _geglu_case(M, K, F, dp, tall, feed, planes_out, monkeypatch):
    """FF1 + GEGLU through the descriptor lib.linear_geglu builds, with fenced out / planes / aux_out.  Returns nothing: asserts."""
    N = 2 * F
    monkeypatch.setattr(L, "A_KBLOCKED", feed == "k")
    monkeypatch.delenv("DDPO_MX_TALL", raising=False)
    L.DATAPATH = dp
    a, w, a32, w32 = _operands(C.dense(M, K, N), "hi", 0)
    bias = torch.randint(-63, 64, (N,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(K + F)).double() * C.EPI_UNIT
    pre_ref = a @ w + bias
    assert (1.02 * _absprod_max(C.dense(M, K, N), "hi") + 4.0) / 2.0 ** -11 < C.LIMIT and torch.equal(pre_ref.float().double(), pre_ref)
    mx = dp == "f16mx"
    L.pack_weights(w32, bwd=False)
    assert L.pack_weights_geglu(w32, bias.float().contiguous(), mx=mx)
    g = L.PACKED[w32.data_ptr()]["geglu"]
    assert L.geglu_mx_layer(w32) == mx
    gw = g["tall"] if tall else g
    if tall:
        assert L.geglu_tall_pays(w32, M)
    act = None if feed == "f" else L.split_planes(a32, fmt=1 if mx else 0)
    results = []
    for seed in (3, 4):
        (obuf, oflat), (abuf, aflat) = _fenced(M * F, torch.float32, seed), _fenced(M * N, torch.float32, seed + 10)
        out, aux = oflat.view(M, F), aflat.view(M, N)
        pbufs = [_fenced(M * F, torch.int16, seed + 20 + i) for i in range(2)] if planes_out else None
        keep = [(obuf.clone(), out.clone()), (abuf.clone(), aux.clone())] + [(b.clone(), p.clone()) for b, p in (pbufs or [])]
        pfmt = 1 if planes_out == 2 else 0
        d = L._gemm_desc(M, N, K, src=a32 if feed == "f" else None, ld_src=K if feed == "f" else 0, out=out, ld_out=F, bias=gw["bias"], aux_out=aux,
                         out_planes=(pbufs[0][1], pbufs[1][1], 0 if feed == "k" else F, pfmt) if planes_out else None, epilogue=2 if tall else 1)
        before = L.gemm_tile_launch_counts()
        if mx:
            L._launch_fwd(d, act, gw["mx"], cross=True)
        else:
            L._launch_fwd(d, act, (gw["hi"], gw["lo"], K, 3 if dp == "bf16x3" else 1), w_layout=1 if tall else g["w_layout"])
        torch.cuda.synchronize()
        delta = _counts_delta(before, L.gemm_tile_launch_counts())
        assert delta == _expected_counts(("tall" if tall else "128", False, 1), dp), delta
        fused = _restore_and_compare(obuf, keep[0][0], out, keep[0][1])
        pre = _restore_and_compare(abuf, keep[1][0], aux, keep[1][1])
        pls = [_restore_and_compare(b, b0, p, p0) for (b, p), (b0, p0) in zip(pbufs, keep[2:])] if planes_out else None
        results.append((fused, pre, pls))
    fused, pre, pls = results[0]
    bad = pre != pre_ref.float()
    assert not bool(bad.any()), "pre-activation: " + _where(bad)
    assert torch.equal(fused, L.geglu(pre.contiguous())), "the fused value is not lib.geglu(pre)"
    if planes_out:
        exp = L.split_planes(fused.contiguous(), fmt=pfmt)
        assert torch.equal(pls[0], exp.hi.reshape(-1)) and torch.equal(pls[1], exp.lo.reshape(-1))
    for x, y in zip(results[0][:2], results[1][:2]):
        assert torch.equal(x, y)


@gpu
@pytest.mark.parametrize("planes_out", [0, 1, 2])
@pytest.mark.parametrize("feed,dp", [("f", "bf16"), ("f", "bf16x3"), ("p", "bf16"), ("p", "bf16x3"), ("k", "bf16x3"), ("p", "f16mx"), ("k", "f16mx")])
@pytest.mark.parametrize("shape,expect", C.GEGLU_128, ids=[gid(s) for s, _ in C.GEGLU_128])
def test_fwd_geglu_on_the_128_tile(shape, expect, feed, dp, planes_out, monkeypatch):
    if planes_out and shape[2] % 32:
        planes_out = 0
    _geglu_case(*shape, dp, False, feed, planes_out, monkeypatch)


@gpu
@pytest.mark.parametrize("planes_out", [0, 1, 2])
@pytest.mark.parametrize("feed,dp", [("p", "bf16x3"), ("k", "bf16x3"), ("p", "f16mx"), ("k", "f16mx")])
@pytest.mark.parametrize("shape,expect", C.GEGLU_TALL, ids=[gid(s) for s, _ in C.GEGLU_TALL])
def test_fwd_geglu_on_the_tall_tile(shape, expect, feed, dp, planes_out, monkeypatch):
    _geglu_case(*shape, dp, True, feed, planes_out, monkeypatch)
