"""The attention backward (ddpo_attention_bwd: fp32; ddpo_attention_bwd_x16: bf16x3 and f16mx) held to float64 per (batch, head) slab, on every tail
of its sweeps, with per-slab dO scales, through the C entry points with sentinels around every output.

The reference is the kernels' contract (tests/_attention_bwd_cases.py: reference()): P is recomputed from the GIVEN lse, D taken from the GIVEN o,
and nothing requires either to come from a softmax.  That makes exact inputs possible.

Tier 1, `torch.equal` (frozen probabilities: q = 0, lse = 6, integer k, v, o, dO times a power of two per slab; _attention_bwd_cases.tier1).  S = 0,
P = 2^-6, every operand a single exact 16-bit term and every partial sum exact in fp32, so dQ, dV and the D vector are bit-equal to float64 on all three
datapaths and dK is exactly 0.  Runs: every (Nq, Nk) of TAILS x every head dim of both dispatch switches, B = 2, heads = 3, with six different dO
scales on the six slabs (2^-30, 2^-12, 1, 2^12, 2^20, all zero) arranged so that every small slab has a larger neighbour both in b and in h — a
mis-indexed, stale or racing amax zeroes that slab, which a whole-tensor max-norm cannot see — once more in the reverse order, and once with q, k, v
as column blocks of (rows, 3C) buffers.  One case grid-strides the dvec pre-pass (2,098,384 rows > 8192 x 256).  The one hardware assumption:
v_exp_f32 / exp2f is exact at an integer argument (8 on f16mx, -6 elsewhere).
Every GPU case of every tier also asserts: each output word in range written, each guard word in front of and behind dq, dk, dv and dvec untouched,
the B * heads words behind dvec untouched (fp32, bf16x3) or equal to the float bits of each slab's max |dO| (f16mx), and — tier 1 — a second launch
into fresh buffers bit-identical (no atomics in the sweeps).

Tier 2, per slab max |err| / max |ref of the slab| <= 2^-18 (f16mx, fp32) / 2^-15 (bf16x3): tier 1's lse, o, v; q and k full-mantissa randn on
disjoint channels (S still 0, P', dO', dS' still single exact terms), so dQ = dS K and dK = dS^T Q' show the hi + lo split of K and Q'; variant `full`:
full-mantissa dO, gating dV = P'^T dO' (hi + lo dO') only.  The gate: f16 hi + lo keeps 22 bits, bf16 hi + lo 16, so one operand is off by 2^-22 / 2^-17
of itself; 16 x / 4 x that leaves room for fp32 accumulation over <= 333 terms.  NOT covered, here or by any contract-level test: V's lo term in
dP = dO' V^T — it is followed at once by the one-term rounding of dS' and sits below it.

Tier 3, the project's own gates (2e-5 fp32, 2e-4 bf16x3, 1e-3 f16mx) applied PER SLAB: real softmax, o and lse from the float64 forward, dO = randn x
2^(7 slab - 20).  The first place dK is non-trivial.  A draw is kept when the CPU model's error against float64 is within 0.7 of the gate (fixed
seeds, at most one draw in five replaced: test_draws_satisfy_their_conditions).

CPU tests: the model is bit-equal to float64 on every tier 1 draw; the draws satisfy their conditions; the tables reach every head dim of both
dispatch switches (read out of the .hip files) and every tail class; each named defect, injected into the model, breaks the gate of its tier.

Observed on an MI355X (487 tests of this file: 482 GPU cases + 5 CPU tests, 6.2 s wall):
    tier 1 (289 cases + 3 grid-stride cases): every case bit-equal to float64 on the first run on fp32, bf16x3 and f16mx — exp2 IS exact at the
        integer arguments the draws use, no case failed by that or by anything else; every sentinel intact, every second launch identical.
        No defect was found in attention_bwd.hip, attention_bwd_bf16.hip or attention_dvec.h; nothing was changed there.
    tier 2 (102 cases), worst slab ratio, measured against float64 (and as a fraction of the gate):
        fp32 9.4e-7 (0.25, d = 8, 200 x 333, int)    bf16x3 5.7e-6 (0.19, d = 16, 130 x 129, full)    f16mx 3.9e-7 (0.10, d = 80, 200 x 333, int)
    tier 3 (85 cases), worst slab ratio against float64 (fraction of the gate):
        fp32 2.0e-6 (0.10, d = 160, 200 x 333)    bf16x3 4.1e-5 (0.20, d = 16, 200 x 333)    f16mx 6.8e-4 (0.69, d = 8, 33 x 33)
        The 16-bit kernels land on the CPU model to three digits (model: 4.08e-5 / 6.85e-4); fp32's model says 4.8e-7 — it sums in float64 what
        the kernel accumulates in fp32 over up to 333 terms.  f16mx at d = 8 is the thin one: its MODEL sits at
        6e-4 .. 1.2e-3 of a slab's maximum, so 4 of the 25 f16mx draws are the second or third seed and the d = 8 row runs 129 x 65 in place of
        129 x 77 (_attention_bwd_cases.TIER3_SHAPE_FOR_D); no draw of fp32 or bf16x3 was replaced.
    defects injected into the model (test_gates_see_the_named_defects): a neighbour's amax in b or in h — NaN / a lost slab (tier 1 is equality);
        one global amax — 100 % of the small slabs; D not multiplied by omul — 1.8e4 x a slab's maximum; last query tile skipped — 21 %; last partial
        key wave not stored — unwritten words; lo planes dropped — 24 .. 35 x the tier 2 gate in EVERY slab; dK without ln 2 — 442 x (f16mx),
        2213 x (bf16x3), 22135 x (fp32) the tier 3 gate.
"""
import gc
import math

import pytest
import torch

import _attention_bwd_cases as C
from _attention_bwd_cases import case_id
from ddpo_amd import lib as L

gpu = pytest.mark.gpu
DEV = "cuda"
SENT = 0x7FC0DEAD             # a NaN bit pattern no kernel computes
GUARD = 64                    # sentinel words in front of and behind every output (keeps the outputs 16-byte aligned)


@pytest.fixture(scope="module", autouse=True)
def _leave_the_process_as_found():
    """The draws and references are computed once and shared by the tests of this file (the grid-stride case alone holds ~1 GB on the host and
    leaves as much in torch's device cache): none of it outlives the file."""
    yield
    for cached in (C.tier1, C.tier1_ref, C.tier2, C.tier3, C.stride_case):
        cached.cache_clear()
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ CPU: model, draws, tables, defects
def _tier1_draws():
    return sorted({(d, Nq, Nk, order) for _, d, Nq, Nk, order, _ in C.tier1_cases()})


def test_model_is_float64_bitwise_on_tier1_draws():
    """On every tier 1 draw (each asserts its own conditions when it is built) the rounding model of each datapath equals the float64 algebra bit for
    bit, and float64 exp2 is exact where the draws need it."""
    assert float(torch.exp2(torch.tensor(-6.0, dtype=torch.float64))) == 2.0 ** -6
    n = 0
    for d, Nq, Nk, order in _tier1_draws():
        draw, ref = C.tier1(Nq, Nk, d, order), C.tier1_ref(Nq, Nk, d, order)
        for dp in C.DATAPATHS:
            if d in C.HEAD_DIMS[dp]:
                got = C.model(dp, draw)
                assert all(torch.equal(got[k], ref[k]) for k in ("dq", "dk", "dv", "dvec", "amax")), (dp, d, Nq, Nk, order)
                n += 1
    # the scales of the slabs really are far apart, and the zero slab is there
    amax = C.tier1_ref(33, 33, 16)["amax"]
    assert sorted(amax.flatten().tolist()) == [0.0, 2.0 ** -28, 2.0 ** -10, 4.0, 2.0 ** 14, 2.0 ** 22]
    print(f"\n[attention bwd tier 1] model == float64 on {n} (datapath, draw) pairs")


def test_model_is_float64_bitwise_on_the_grid_stride_case():
    draw, ref = C.stride_case()
    Bn, heads, Nq, Nk, d = draw.dims
    assert Bn * heads * Nq > 8192 * 256 and len(set(ref["amax"].flatten().tolist())) == 2
    got = C.model("f16mx", draw)
    assert all(torch.equal(got[k], ref[k]) for k in ("dq", "dk", "dv", "dvec", "amax"))


def test_draws_satisfy_their_conditions():
    """Tier 2: S exactly 0 and (variant int) the exactness conditions of dS' — asserted when each draw is built — and the model itself is inside the
    gate.  Tier 3: every draw's MODEL error against float64 is within 0.7 of the gate, with at most one draw in five replaced by its next seed."""
    worst2 = dict.fromkeys(C.DATAPATHS, 0.0)
    for dp, d, Nq, Nk, variant in C.tier2_cases():
        draw = C.tier2(Nq, Nk, d, variant)
        r = C.worst_ratio(C.model(dp, draw), C.reference(draw), ("dv",) if variant == "full" else ("dq", "dk", "dv"))
        worst2[dp] = max(worst2[dp], r)
        assert r <= C.TIER2_GATE[dp], (dp, d, Nq, Nk, variant, r)
    worst3, replaced, total = dict.fromkeys(C.DATAPATHS, 0.0), dict.fromkeys(C.DATAPATHS, 0), dict.fromkeys(C.DATAPATHS, 0)
    for dp, d, Nq, Nk in C.tier3_cases():
        draw, _, r = C.tier3(dp, Nq, Nk, d)
        assert r <= C.TIER3_KEEP * C.TIER3_GATE[dp]
        worst3[dp] = max(worst3[dp], r)
        replaced[dp] += draw.meta["attempt"] > 0
        total[dp] += 1
    print("\n[attention bwd model] worst tier 2 ratio " + "  ".join(f"{k} {v:.2e}" for k, v in worst2.items()))
    print("[attention bwd model] worst tier 3 ratio " + "  ".join(f"{k} {v:.2e} ({replaced[k]}/{total[k]} replaced)" for k, v in worst3.items()))
    assert all(5 * replaced[dp] <= total[dp] for dp in C.DATAPATHS), replaced


def test_tables_cover_the_dispatch_switches_and_the_tails():
    """Every head dim of both `switch (d)` lists (read out of the sources) is run on every tier, and TAILS holds every tail class of both kernel
    geometries.  IF YOU ADD A HEAD DIM OR CHANGE A TILE: mirror it in _attention_bwd_cases.HEAD_DIMS / GEOMETRY."""
    sw = C.dispatch_head_dims()
    assert sw["fp32"] == C.HEAD_DIMS["fp32"] and sw["x16"] == C.HEAD_DIMS["bf16x3"] == C.HEAD_DIMS["f16mx"], sw
    for cases in (C.tier1_cases(), C.tier2_cases(), C.tier3_cases()):
        assert {(c[0], c[1]) for c in cases} == {(dp, d) for dp in C.DATAPATHS for d in C.HEAD_DIMS[dp]}
    for dp in C.DATAPATHS:
        for d in C.HEAD_DIMS[dp]:
            dense = {(c[2], c[3]) for c in C.tier1_cases() if c[:2] == (dp, d) and c[4:] == ("fwd", "dense")}
            assert dense == set(C.TAILS)
    assert (1, 1) in C.TAILS
    for geo in ({"wg": 64, "wave": 16, "tile": 64}, {"wg": 128, "wave": 32, "tile": 64}):
        assert geo in C.GEOMETRY.values()
        for side in (0, 1):                           # the owning side of the dq kernel (queries) and of the dkdv kernel (keys)
            own = [t[side] for t in C.TAILS]
            assert any(n > geo["wave"] and n % geo["wave"] == 1 for n in own)                 # one token in the last wave
            assert geo["wg"] + 1 in own                                                       # one token in the second workgroup
            assert any(n < geo["wave"] for n in own) and any(n == geo["tile"] for n in own)
            swept = [t[1 - side] for t in C.TAILS]
            assert any(n > geo["tile"] and n % geo["tile"] for n in swept) and any(n < geo["tile"] for n in swept)   # a ragged last swept tile
    assert any(nq % 64 and nk % 128 and nq > 128 and nk > 128 for nq, nk in C.TAILS)          # both ragged on the x16 kernels
    # every small slab has a larger neighbour both in b and in h, in both orders
    for sc in (C.SLAB_SCALES, C.SLAB_SCALES_REV):
        assert sorted(x for row in sc for x in row) == [0.0, 2.0 ** -30, 2.0 ** -12, 1.0, 2.0 ** 12, 2.0 ** 20]
        for b in range(C.B):
            for h in range(C.HEADS):
                if sc[b][h] < 1.0:
                    assert sc[1 - b][h] > sc[b][h] and max(sc[b][(h + 1) % 3], sc[b][(h + 2) % 3]) > sc[b][h]


def _fmt(r):
    return "inf" if math.isinf(r) else f"{r:.2e}"


def test_gates_see_the_named_defects():
    """Each defect the tiers are there for, injected into the model, breaks the gate of the tier meant to catch it.  Tier 1's gate is equality: the
    figure printed is the worst slab's max |err| / max |ref| (inf: NaN, or a non-zero value in the zero slab); tiers 2 and 3: that figure / the gate."""
    lines = []
    for defect in ("amax_b", "amax_h", "amax_global", "d_unscaled"):                       # tier 1, f16mx (no other datapath scales dO)
        for order in ("fwd", "rev"):
            draw, ref = C.tier1(130, 129, 40, order), C.tier1_ref(130, 129, 40, order)
            got = C.model("f16mx", draw, defect)
            assert not all(torch.equal(got[k], ref[k]) for k in ("dq", "dk", "dv")), (defect, order)
            lines.append(f"tier 1 f16mx {order} {defect}: {_fmt(C.worst_ratio(got, ref))}")
            assert C.worst_ratio(got, ref) > 0.5                                           # not a last-bit matter: some slab is lost outright
    for defect in ("skip_last_q_tile", "no_last_key_wave"):                                # tier 1, every datapath
        for dp in C.DATAPATHS:
            draw, ref = C.tier1(130, 129, 16), C.tier1_ref(130, 129, 16)
            got = C.model(dp, draw, defect)
            assert not all(torch.equal(got[k], ref[k]) for k in ("dq", "dk", "dv")), (defect, dp)
            lines.append(f"tier 1 {dp} {defect}: {_fmt(C.worst_ratio(got, ref))}")
    for dp in ("bf16x3", "f16mx"):                                                         # tier 2: lo planes of the wide operands
        for variant, names in (("int", ("dq", "dk")), ("full", ("dv",))):
            for name in names:
                worst = math.inf
                for Nq, Nk in C.TIER2_SHAPES:
                    draw = C.tier2(Nq, Nk, 16, variant)
                    worst = min(worst, float(C.slab_ratio(C.model(dp, draw, "drop_lo")[name], C.reference(draw)[name]).min()) / C.TIER2_GATE[dp])
                lines.append(f"tier 2 {dp} {variant} drop_lo, {name}: least slab {worst:.1f} x gate")
                assert worst > 1.0, (dp, variant, name, worst)                             # EVERY slab of every shape sees it
    for dp in C.DATAPATHS:                                                                 # tier 3: dK is non-trivial
        draw, ref, _ = C.tier3(dp, 33, 33, 8)
        r = float(C.slab_ratio(C.model(dp, draw, "dk_no_ln2")["dk"], ref["dk"]).min()) / C.TIER3_GATE[dp]
        lines.append(f"tier 3 {dp} dk_no_ln2: least slab {r:.0f} x gate")
        assert r > 1.0
    print("\n[attention bwd defects]\n  " + "\n  ".join(lines))


# ------------------------------------------------------------------------------------------------ GPU harness
class Guarded:
    """n output words (+ `tail` more the call may own) between two runs of GUARD sentinel words."""

    def __init__(self, n, tail=0):
        self.n, self.tail = n, tail
        self.buf = torch.full((n + tail + 2 * GUARD,), SENT, dtype=torch.int32, device=DEV)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * GUARD

    def bits(self):
        return self.buf[GUARD:GUARD + self.n]

    def tail_bits(self):
        return self.buf[GUARD + self.n:GUARD + self.n + self.tail]

    def values(self):
        return self.bits().view(torch.float32)

    def guards_intact(self):
        return bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[GUARD + self.n + self.tail:] == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())


def _entry(dp):
    lib = L.load()
    if dp == "fp32":
        return lib.ddpo_attention_bwd
    return lambda *a: lib.ddpo_attention_bwd_x16(int(dp == "f16mx"), *a)


def _operands(draw, layout):
    """Device q, k, v as (pointer, ld) — dense, or ('ld3c') column blocks of (rows, 3C) buffers whose other blocks are non-zero — and what keeps them alive."""
    Bn, heads, Nq, Nk, d = draw.dims
    Cc = heads * d
    if layout == "dense":
        t = [x.to(DEV) for x in (draw.q, draw.k, draw.v)]
        return [(x.data_ptr(), Cc) for x in t], t
    assert layout == "ld3c"
    if Nq == Nk:                                       # [q | k | v] in one buffer
        buf = torch.cat([draw.q, draw.k, draw.v], 1).to(DEV)
        return [(buf.data_ptr() + 4 * Cc * i, 3 * Cc) for i in range(3)], [buf]
    bq = torch.cat([torch.full_like(draw.q, 7.0), draw.q, torch.full_like(draw.q, -5.0)], 1).to(DEV)          # [junk | q | junk]
    bkv = torch.cat([draw.k, torch.full_like(draw.k, 9.0), draw.v], 1).to(DEV)                                # [k | junk | v]
    return [(bq.data_ptr() + 4 * Cc, 3 * Cc), (bkv.data_ptr(), 3 * Cc), (bkv.data_ptr() + 8 * Cc, 3 * Cc)], [bq, bkv]


def _outputs(draw):
    Bn, heads, Nq, Nk, d = draw.dims
    Cc = heads * d
    return dict(dq=Guarded(Bn * Nq * Cc), dk=Guarded(Bn * Nk * Cc), dv=Guarded(Bn * Nk * Cc), dvec=Guarded(Bn * heads * Nq, tail=Bn * heads))


def launch(dp, draw, layout="dense"):
    """One call of the C entry point into sentinel-guarded buffers -> {'dq', 'dk', 'dv', 'dvec': Guarded}."""
    Bn, heads, Nq, Nk, d = draw.dims
    (pq, pk, pv), keep = _operands(draw, layout)
    o, do, lse = draw.o.to(DEV), draw.do.to(DEV), draw.lse.contiguous().to(DEV)
    out = _outputs(draw)
    rc = _entry(dp)(pq[0], pq[1], pk[0], pk[1], pv[0], pv[1], L._p(o), L._p(do), L._p(lse), out["dvec"].ptr, out["dq"].ptr, out["dk"].ptr,
                    out["dv"].ptr, Bn, heads, Nq, Nk, d, draw.scale, L._stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    del keep
    return out


def check_frame(dp, draw, ref, out):
    """Every word in range written, every guard word untouched, the slab maxima behind dvec as the datapath's contract says."""
    for name, g in out.items():
        assert g.guards_intact(), f"{name}: a guard word was written"
        unwritten = int((g.bits() == SENT).sum())
        assert unwritten == 0, f"{name}: {unwritten} words in range never written"
    tail = out["dvec"].tail_bits().cpu()
    if dp == "f16mx":
        assert torch.equal(tail, ref["amax"].float().flatten().view(torch.int32)), "slab maxima behind dvec"
    else:
        assert bool((tail == SENT).all()), "the words behind dvec belong to the caller on this datapath"


def slab_outputs(draw, out):
    Bn, heads, Nq, Nk, d = draw.dims
    got = {n: C.slabs(out[n].values().cpu().view(-1, heads * d), Bn, N, heads, d) for n, N in (("dq", Nq), ("dk", Nk), ("dv", Nk))}
    got["dvec"] = out["dvec"].values().cpu().view(Bn, heads, Nq).double()
    return got


def assert_exact(dp, draw, ref, out, what=""):
    got = slab_outputs(draw, out)
    for name in ("dq", "dk", "dv", "dvec"):
        if not torch.equal(got[name], ref[name]):
            r = C.slab_ratio(got[name], ref[name])
            raise AssertionError(f"{what} {name} differs from float64; per-slab max |err| / max |ref|:\n{r}\n(slab scales {draw.meta['scales']})")


# ------------------------------------------------------------------------------------------------ GPU: tier 1
@gpu
@pytest.mark.parametrize("case", C.tier1_cases(), ids=case_id)
def test_tier1_exact(case):
    """Tails x slab scales x sentinels (x reverse order, x ld = 3C): bit-equal to float64, slab by slab; the zero slab exactly zero; a second launch
    into fresh buffers identical."""
    dp, d, Nq, Nk, order, layout = case
    draw, ref = C.tier1(Nq, Nk, d, order), C.tier1_ref(Nq, Nk, d, order)
    out = launch(dp, draw, layout)
    check_frame(dp, draw, ref, out)
    assert_exact(dp, draw, ref, out, case_id(case))
    again = launch(dp, draw, layout)
    assert all(torch.equal(out[n].buf, again[n].buf) for n in out), "a second launch gave other bits"


@gpu
@pytest.mark.parametrize("dp", C.DATAPATHS)
def test_dvec_grid_stride_exact(dp):
    """B heads Nq = 2,098,384 rows: the pre-pass runs its grid-stride loop (and, on f16mx, the atomic max from every block) — D, the slab maxima,
    dQ and dV bit-equal to float64, two dO scales across the 16 heads."""
    draw, ref = C.stride_case()
    out = launch(dp, draw)
    check_frame(dp, draw, ref, out)
    assert_exact(dp, draw, ref, out, f"grid-stride {dp}")


@gpu
@pytest.mark.parametrize("dp", C.DATAPATHS)
def test_argument_refusals_run_nothing(dp):
    """An ld that is no multiple of 4, an unsupported d and a null dvec return -1 and leave every output word as it was."""
    draw = C.tier1(17, 17, 8)
    Bn, heads, Nq, Nk, d = draw.dims
    Cc = heads * d
    q, k, v, o, do, lse = (x.contiguous().to(DEV) for x in (draw.q, draw.k, draw.v, draw.o, draw.do, draw.lse))
    out = _outputs(draw)
    fn = _entry(dp)

    def call(ld=(Cc, Cc, Cc), dd=d, dvec=out["dvec"].ptr):
        return fn(L._p(q), ld[0], L._p(k), ld[1], L._p(v), ld[2], L._p(o), L._p(do), L._p(lse), dvec, out["dq"].ptr, out["dk"].ptr, out["dv"].ptr,
                  Bn, heads, Nq, Nk, dd, draw.scale, L._stream())
    for i in range(3):
        assert call(ld=tuple(Cc + 2 * (i == j) for j in range(3))) == -1
    for dd in ((4, 160, 12, 32) if dp != "fp32" else (12, 32, 2)):
        assert call(dd=dd) == -1
    assert call(dvec=None) == -1
    torch.cuda.synchronize()
    assert all(g.untouched() for g in out.values())


# ------------------------------------------------------------------------------------------------ GPU: tiers 2 and 3
@gpu
@pytest.mark.parametrize("case", C.tier2_cases(), ids=case_id)
def test_tier2_wide_operand_lo_terms(case):
    """hi + lo of K and Q' (variant int: dQ, dK; dV exact by the way) and of dO' (variant full: dV only), per slab, at three slab scales."""
    dp, d, Nq, Nk, variant = case
    draw = C.tier2(Nq, Nk, d, variant)
    ref = C.reference(draw)
    out = launch(dp, draw)
    check_frame(dp, draw, ref, out)
    got = slab_outputs(draw, out)
    names = ("dv",) if variant == "full" else ("dq", "dk", "dv")
    ratios = {n: C.slab_ratio(got[n], ref[n]) for n in names}
    worst = max(float(r.max()) for r in ratios.values())
    print(f"\n[attention bwd tier2 {case_id(case)}] worst slab ratio {worst:.3e} = {worst / C.TIER2_GATE[dp]:.3f} of the gate")
    assert worst <= C.TIER2_GATE[dp], ratios


@gpu
@pytest.mark.parametrize("case", C.tier3_cases(), ids=case_id)
def test_tier3_softmax_per_slab(case):
    """A real softmax with dO scales 2^-20 .. 2^15 across the six slabs: the project's gate on each slab's own maximum; D within the fp32 bound of a
    d-term dot product, (d + 2) 2^-24 sum |o dO|."""
    dp, d, Nq, Nk = case
    draw, ref, model_ratio = C.tier3(dp, Nq, Nk, d)
    out = launch(dp, draw)
    check_frame(dp, draw, ref, out)
    got = slab_outputs(draw, out)
    ratios = {n: C.slab_ratio(got[n], ref[n]) for n in ("dq", "dk", "dv")}
    worst = max(float(r.max()) for r in ratios.values())
    print(f"\n[attention bwd tier3 {case_id(case)}] worst slab ratio {worst:.3e} = {worst / C.TIER3_GATE[dp]:.3f} of the gate (model {model_ratio:.3e})")
    assert worst <= C.TIER3_GATE[dp], ratios
    _, _, _, o, do, _ = draw.slab_inputs()
    assert bool(((got["dvec"] - ref["dvec"]).abs() <= (d + 2) * 2.0 ** -24 * (o * do).abs().sum(-1)).all())
