"""CPU-only checks of the `--pg_loss d3po` boundary: include/ddpo_pref.h against lib_pref._SIGS and the library's exports (its own ABI
version, nothing of it in ddpo_hip.h), the entry's argument validation (which returns before any launch), the closed form of the log-ratio
and of the gradient against float64 autograd of log-prob minus log-prob (tests/_pref_oracle.py), and the host side of pairs: prompts, labels,
both shuffles, the flags and the entry point's argument check.  No device compute is launched here."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

from ddpo_amd import lib as L
from oracle.ddim import DDIMOracle

import _pref_oracle as PO
from _abi_check import check_signatures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "ddpo_pref.h")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def test_signatures_match_the_header_prototypes():
    """tests/test_abi_cpu.py::test_signatures_match_the_header_prototypes, applied to include/ddpo_pref.h and lib_pref._SIGS."""
    from ddpo_amd import lib_pref as LP
    check_signatures(HDR, LP._SIGS, 2, returns=("int",))


def test_library_exports_every_declared_symbol_under_its_own_version():
    from ddpo_amd import lib_pref as LP
    declared = set(re.findall(r"\b(ddpo_[a-z0-9_]+)\s*\(", _header()))
    assert declared == set(LP.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in ddpo_pref.h but not exported"
    assert LP.load().ddpo_pref_abi_version() == LP.ABI_VERSION == 1
    # versioned on its own: ddpo_hip.h, lib.ABI_VERSION and lib._SIGS know nothing of it
    main = open(os.path.join(ROOT, "include", "ddpo_hip.h")).read()
    for name in LP.EXPORTED_SYMBOLS:
        assert name not in main and name not in L._SIGS


def test_binding_refuses_a_version_mismatch(monkeypatch):
    from ddpo_amd import lib_pref as LP
    monkeypatch.setattr(LP, "_lib", None)
    monkeypatch.setattr(LP, "ABI_VERSION", 2)
    with pytest.raises(L.DdpoHipError, match="preference-loss ABI version 1.*expects 2"):
        LP.load()
    assert LP._lib is None


def test_entry_rejects_bad_arguments_before_any_launch():
    """Every DDPO_EINVAL case of include/ddpo_pref.h on host buffers: the checks come before the first launch, so no device is touched."""
    from ddpo_amd import lib_pref as LP
    fn = LP.load().ddpo_ddim_pref_fwd_bwd
    B, group, chw = 4, 2, 8
    bufs = [np.zeros(B * chw + 4, dtype=np.float32) for _ in range(8)]
    a16 = lambda a: a.ctypes.data + (-a.ctypes.data % 16)                  # 16-byte aligned address inside the buffer
    ec, eu, rc, ru, x, xn, dc, du = (ctypes.c_void_p(a16(a)) for a in bufs)
    ts = np.ones(B, dtype=np.int32)
    tsp = ctypes.c_void_p(ts.ctypes.data)
    pref = np.asarray([1, -1, -1, 1], dtype=np.float32)
    small = [np.zeros(B // 2 * 4, dtype=np.float32), np.zeros(B // group * 3, dtype=np.float32)]
    pp, inf = (ctypes.c_void_p(a.ctypes.data) for a in small)
    prp = ctypes.c_void_p(pref.ctypes.data)
    acp = np.ones(1000, dtype=np.float32)

    def call(ec=ec, eu=eu, rc=rc, ru=ru, x=x, xn=xn, ts=tsp, pref=prp, beta=0.1, cfg=1, c=None, dc=dc, du=du, pp=pp, inf=inf, B=B, group=group,
             chw=chw, pred=0):
        cc = L.DdimConsts(acp.ctypes.data, 1000, 20, 1.0, 1.0, pred)
        return fn(ec, eu, rc, ru, x, xn, ts, pref, 5.0, beta, cfg, ctypes.byref(cc) if c is None else c, dc, du, pp, inf, B, group, chw, None)

    null = ctypes.c_void_p(0)
    off = lambda p: ctypes.c_void_p(p.value + 4)
    cases = [dict(ec=null), dict(rc=null), dict(x=null), dict(xn=null), dict(ts=null), dict(pref=null), dict(dc=null), dict(pp=null),
             dict(inf=null), dict(c=ctypes.POINTER(L.DdimConsts)()),
             dict(eu=null), dict(ru=null), dict(du=null),                              # required under train_cfg
             dict(B=0), dict(B=-4), dict(B=3, group=3), dict(group=0), dict(group=-2), dict(group=1), dict(B=6, group=3), dict(B=6, group=4),
             dict(chw=0), dict(chw=-4), dict(chw=6),
             dict(beta=0.0), dict(beta=-0.1), dict(beta=float("nan")), dict(beta=float("inf")),
             dict(pred=L.PRED_TYPES["sample"]),
             dict(ec=off(ec)), dict(rc=off(rc)), dict(x=off(x)), dict(xn=off(xn)), dict(dc=off(dc)),      # float4 access: 16-byte alignment
             dict(eu=off(eu)), dict(ru=off(ru)), dict(du=off(du)),
             dict(cfg=0, ec=off(ec))]
    for kw in cases:
        assert call(**kw) == -1, kw
    for a in bufs + small:
        assert not a.any()


# ------------------------------------------------------------------------------------------------ the closed form against float64 autograd
TS = [981, 1, 481, 21, 961, 501]


def _case(pred, train_cfg, B=6, shape=(4, 6, 6), seed=0):
    dd = DDIMOracle(prediction_type=pred)
    st = dd.set_timesteps(dd.create_state(), 50)
    g = torch.Generator().manual_seed(seed + 7 * (pred == "epsilon") + int(train_cfg))
    ec, eu, x, z = (torch.randn(B, *shape, generator=g, dtype=torch.float64) for _ in range(4))
    rc = ec + 1e-2 * torch.randn(B, *shape, generator=g, dtype=torch.float64)
    ru = eu + 1e-2 * torch.randn(B, *shape, generator=g, dtype=torch.float64)
    ts = np.asarray(TS, dtype=np.int32)[:B]
    guided = (eu + 5.0 * (ec - eu)) if train_cfg else ec
    xn, _ = dd.step(st, guided.numpy().astype(np.float32), ts, x.numpy().astype(np.float32), noise=z.numpy().astype(np.float32), eta=1.0)
    pref = np.asarray([1, -1, -1, 1, 0, 0], dtype=np.float32)[:B]
    return dd, st, ec, (eu if train_cfg else None), rc, (ru if train_cfg else None), x, torch.from_numpy(xn).double(), ts, pref


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("train_cfg", [True, False])
def test_closed_form_equals_float64_autograd_of_the_log_prob_difference(pred, train_cfg):
    dd, st, ec, eu, rc, ru, x, xn, ts, pref = _case(pred, train_cfg)
    group = 6
    with torch.no_grad():                 # beta on the host, so that the larger |s_p| is 2: the sigmoid is off its centre and q enters the gradient
        h0 = PO.log_ratio_rows_torch(dd, st, ec, eu, rc, ru, x, xn, ts, 5.0, 1.0, train_cfg)
    beta = 2.0 / float((h0[0:4:2] - h0[1:4:2]).abs().max())
    tec = ec.clone().requires_grad_(True)
    teu = eu.clone().requires_grad_(True) if train_cfg else None
    batch = {"ts": ts, "latents": x, "next_latents": xn, "advantages": torch.from_numpy(pref)}
    loss, info, h, s, loss_p = PO.loss_and_info_torch(dd, st, tec, teu, rc, ru, batch, 5.0, 1.0, beta, train_cfg)
    loss.backward()
    assert float(loss_p[2].detach()) == 0.0 and float(s[2].detach()) == 0.0      # the tie
    assert float(s.detach().abs().max()) == pytest.approx(2.0)
    # the same numbers from the closed form, evaluated in float64 by handing float64 arrays to the algebra below
    *_, std_c, c_t = PO.KO.coefficients(dd, st, ts, 1.0)
    e = PO.KO.guided(ec, eu, 5.0, train_cfg)
    delta = PO.KO.guided(ec - rc, None if eu is None else eu - ru, 5.0, train_cfg)
    r = xn - PO.KO.ddim_mean_torch(dd, st, e, ts, x, 1.0)
    chw = r[0].numel()
    B = r.shape[0]
    ct, var = c_t.reshape(B), (std_c ** 2).reshape(B)
    h_cf = (2 * ct * (r * delta).flatten(1).sum(1) + ct ** 2 * (delta ** 2).flatten(1).sum(1)) / (2 * var * chw)
    # log-prob minus log-prob cancels |logp| ~ 1 against |h| ~ 1e-2 .. 1 in float64: 1e-16 / 1e-2
    np.testing.assert_allclose(h_cf.numpy(), h.detach().numpy(), rtol=1e-11, atol=1e-14)
    y, _, _, q = PO.pair_terms_torch(h_cf, pref, beta)
    dl_even = -beta * y * q / (group // 2)
    dl = torch.stack([dl_even, -dl_even], 1).reshape(B)
    de = (dl * ct / (var * chw)).reshape(B, 1, 1, 1) * r
    gc = 5.0 * de if train_cfg else de
    np.testing.assert_allclose(gc.numpy(), tec.grad.numpy(), rtol=1e-9, atol=1e-15 * float(tec.grad.abs().max()))
    assert float(tec.grad[4:].abs().max()) == 0.0 and float(tec.grad[:4].abs().min()) > 0.0
    if train_cfg:
        np.testing.assert_allclose(((1 - 5.0) * de).numpy(), teu.grad.numpy(), rtol=1e-9, atol=1e-15 * float(teu.grad.abs().max()))
    # and the fp32 restatement of the HIP pass says the same to fp32 accuracy
    f = lambda t: None if t is None else t.numpy().astype(np.float32)
    t64 = lambda a: None if a is None else torch.from_numpy(a).double()
    h32, s32, lp32, info32, dc32, du32 = PO.closed_form_numpy(dd, st, f(ec), f(eu), f(rc), f(ru), f(x), f(xn), ts, pref, 5.0, 1.0, beta, group, train_cfg)
    tec2 = t64(f(ec)).requires_grad_(True)
    teu2 = t64(f(eu)).requires_grad_(True) if train_cfg else None
    b32 = {"ts": ts, "latents": t64(f(x)), "next_latents": t64(f(xn)), "advantages": torch.from_numpy(pref)}
    loss2, info2, h2, s2, lp2 = PO.loss_and_info_torch(dd, st, tec2, teu2, t64(f(rc)), t64(f(ru)), b32, 5.0, 1.0, beta, train_cfg)
    loss2.backward()
    hmax = float(h2.detach().abs().max())
    assert float(np.abs(h32 - h2.detach().numpy()).max()) < 2e-5 * hmax
    assert float(np.abs(s32 - s2.detach().numpy()).max()) < 2e-5 * beta * hmax
    assert float(np.abs(lp32 - lp2.detach().numpy()).max()) < 2e-5 * max(1.0, beta * hmax)
    assert info32.shape == (1, 3) and info32[0, 0] == float(info2["pref_acc"])
    assert float(abs(info32[0, 1] - float(info2["pref_margin"]))) < 2e-5 * hmax
    assert float(np.abs(dc32 - tec2.grad.numpy()).max() / tec2.grad.abs().max()) < 5e-5
    if train_cfg:
        assert float(np.abs(du32 - teu2.grad.numpy()).max() / teu2.grad.abs().max()) < 5e-5


def test_oracle_is_exactly_zero_where_the_networks_agree():
    dd, st, ec, eu, rc, ru, x, xn, ts, pref = _case("epsilon", True)
    h = PO.log_ratio_rows_torch(dd, st, ec, eu, ec, eu, x, xn, ts, 5.0, 1.0, True)
    assert float(h.abs().max()) == 0.0
    f = lambda t: t.numpy().astype(np.float32)
    h32, s32, lp32, info32, dc32, _ = PO.closed_form_numpy(dd, st, f(ec), f(eu), f(ec), f(eu), f(x), f(xn), ts, pref, 5.0, 1.0, 0.1, 2, True)
    assert not h32.any() and not s32.any() and info32[0, 1] == 0.0
    assert lp32[0] == np.log1p(np.float32(1.0)) and lp32[2] == 0.0 and np.abs(dc32[:4]).min() > 0 and not dc32[4:].any()


# ------------------------------------------------------------------------------------------------ pairs on the host
def test_prompts_in_pairs():
    from ddpo_amd.training import prompts as P
    from ddpo_amd.training.dp import DataParallel
    random.seed(3)
    want = [P.imagenet_animals() for _ in range(4)]
    random.seed(3)
    p, t, m = P.make_prompts("imagenet_animals", 8, pairs=True)
    assert len(p) == len(t) == len(m) == 8
    assert p == [w[0] for w in want for _ in range(2)] and list(t) == [w[1] for w in want for _ in range(2)]
    assert len(set(p)) > 1
    random.seed(3)
    assert P.make_prompts("imagenet_animals", 8)[0][:4] == [w[0] for w in want]            # the default draw is what it was: one per row
    with pytest.raises(ValueError, match="even"):
        P.make_prompts("imagenet_animals", 3, pairs=True)
    random.seed(3)
    a = P.make_prompts("imagenet_animals", 4, True, pairs=True)
    random.seed(3)
    assert a == P.make_prompts("imagenet_animals", 4, True) and len(set(a[0])) == 1           # identical_batch is unchanged
    # through DataParallel: multi_host draws its own batch, single_host the global one and keeps its block; pairs never straddle ranks
    random.seed(3)
    assert DataParallel("multi_host", 0, 1).make_prompts("imagenet_animals", 8, pairs=True)[0] == p
    blocks = []
    for r in range(2):
        random.seed(3)
        blocks += DataParallel("single_host", r, 2).make_prompts("imagenet_animals", 4, pairs=True)[0]
    assert blocks == p


def test_labels_including_a_tie():
    from ddpo_amd.training.preference import pair_labels
    y = pair_labels(np.asarray([0.3, 0.1, -2.0, 5.0, 1.5, 1.5, 7.0, 7.5]))
    assert y.dtype == np.float32 and y.tolist() == [1.0, -1.0, -1.0, 1.0, 0.0, 0.0, -1.0, 1.0]
    assert not np.signbit(y[4:6]).any()                                           # a tie is +0.0 on both rows
    assert pair_labels(np.asarray([1e-3, 2e-3])).tolist() == [-1.0, 1.0]          # only the sign: no scale
    with pytest.raises(ValueError, match="even"):
        pair_labels(np.zeros(3))


def _devs(total, T):
    """Values that name their (row, step): row * 1000 + step; row 2p and 2p+1 are a pair."""
    rs = torch.arange(total)[:, None] * 1000 + torch.arange(T)[None]
    return {"log_probs": rs.float(), "ts": rs.clone(), "latents": rs[..., None].float(), "next_latents": rs[..., None].float() + 0.5,
            "advantages": torch.arange(total).float(), "embeds": torch.arange(total)[:, None].float()}


def _check_paired(out, total_in, T):
    rows, steps = out["ts"] // 1000, out["ts"] % 1000
    assert bool((rows == rows[:, :1]).all())                                      # a row stays one trajectory
    r = rows[:, 0]
    assert bool((r[0::2] % 2 == 0).all()) and bool((r[1::2] == r[0::2] + 1).all())     # pairs adjacent, even row first
    assert torch.equal(steps[0::2], steps[1::2])                                  # both rows of a pair: the same step at every index
    assert all(sorted(s.tolist()) == list(range(T)) for s in steps)
    assert torch.equal(out["advantages"].long(), r) and torch.equal(out["embeds"][:, 0].long(), r)
    assert torch.equal(out["log_probs"].long(), out["ts"]) and torch.equal(out["latents"][..., 0].long(), out["ts"])
    return r


def test_both_shuffles_keep_pairs_and_agree():
    from ddpo_amd.training.dp import DataParallel
    total, T, tb = 16, 5, 2
    devs = _devs(total, T)
    full = DataParallel.shuffle(devs, np.random.RandomState(7), pairs=True)
    r = _check_paired(full, total, T)
    assert sorted(r.tolist()) == list(range(total)) and r.tolist() != list(range(total))
    assert not torch.equal(full["ts"][0] % 1000, full["ts"][2] % 1000)            # one time permutation per pair, not one for all
    # the default draws are what they were
    rs = np.random.RandomState(7)
    perm = rs.permutation(total)
    perms = np.array([rs.permutation(T) for _ in range(total)])
    plain = DataParallel.shuffle(devs, np.random.RandomState(7))
    assert torch.equal(plain["ts"], devs["ts"][torch.as_tensor(perm)][torch.arange(total)[:, None], torch.as_tensor(perms)])
    for world in (1, 2, 4):
        seen = []
        for rank in range(world):
            dp = DataParallel("single_host", rank, world)
            mine = dp.shuffled_rows(devs, tb, np.random.RandomState(7), pairs=True)
            want = dp.my_rows(full, tb)
            for k in devs:
                assert torch.equal(mine[k], want[k]), (world, rank, k)
            seen += _check_paired(mine, total, T).tolist()
        assert sorted(seen) == list(range(total))                                 # the rank slices partition the set
    mh = DataParallel("multi_host", 1, 2).shuffled_rows(devs, tb, np.random.RandomState(7), pairs=True)
    assert all(torch.equal(mh[k], full[k]) for k in devs)                         # multi_host: every row is mine
    with pytest.raises(ValueError, match="even"):
        DataParallel("single_host", 0, 2).shuffled_rows(_devs(6, T), 3, np.random.RandomState(7), pairs=True)
    with pytest.raises(ValueError, match="even"):
        DataParallel.shuffle(_devs(5, T), np.random.RandomState(7), pairs=True)


# ------------------------------------------------------------------------------------------------ flags
def test_config_defaults_parser_and_argument_checks(tmp_path, monkeypatch):
    """The checks are plain functions of the parsed arguments: main() calls them before load_unet."""
    import inspect
    import config.base as C
    from ddpo_amd.training.preference import check_d3po_args
    from pipeline import policy_gradient as pg
    monkeypatch.chdir(tmp_path)
    assert C.base["pg"]["pg_loss"] == "ppo" and C.base["pg"]["d3po_beta"] == 0.1
    assert "pg_loss" not in C.base["sample"] and "pg_loss" not in C.base["train"]
    common = ["--dataset", "compressed-animals", "--logbase", str(tmp_path / "run")]
    a0 = pg.Parser(common).parse_args("pg")
    assert a0.pg_loss == "ppo" and pg.check_d3po_args(a0) is None
    a1 = pg.Parser(common + ["--pg_loss", "d3po", "--d3po_beta", "0.5"]).parse_args("pg")
    assert a1.pg_loss == "d3po" and a1.d3po_beta == 0.5 and isinstance(a1.d3po_beta, float) and pg.check_d3po_args(a1) is None
    bad = lambda *f: pg.check_d3po_args(pg.Parser(common + ["--pg_loss", "d3po"] + list(f)).parse_args("pg"))
    assert "--eta 0" in bad("--eta", "0")
    assert "sample_batch_size must be even" in bad("--sample_batch_size", "3", "--train_batch_size", "1")
    assert "train_batch_size must be even" in bad("--sample_batch_size", "6", "--train_batch_size", "3")
    assert "finite number > 0" in bad("--d3po_beta", "0") and "finite number > 0" in bad("--d3po_beta", "-1")
    assert "finite number > 0" in check_d3po_args("d3po", float("nan"), 1.0, 2, 2) and "finite number > 0" in check_d3po_args("d3po", float("inf"), 1.0, 2, 2)
    assert "ppo or d3po" in check_d3po_args("dpo", 0.1, 1.0, 2, 2)
    assert check_d3po_args("ppo", float("nan"), 0.0, 3, 3) is None                # nothing of it is looked at by default
    src = inspect.getsource(pg.main)
    assert 0 < src.index("check_d3po_args(args)") < src.index("load_unet(")      # before any model is loaded
    assert "pg_loss" not in open(os.path.join(ROOT, "pipeline", "finetune.py")).read()


def test_default_path_never_imports_the_binding():
    """--pg_loss ppo: a fresh interpreter that imports the training step and the entry point has neither the binding nor the label module."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import ddpo_amd.training.policy_gradient, pipeline.policy_gradient; "
            "assert 'ddpo_amd.lib_pref' not in sys.modules and 'ddpo_amd.training.preference' not in sys.modules" % ROOT)
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
    from ddpo_amd.training import policy_gradient as TP
    with pytest.raises(ValueError, match="one of"):
        TP._loss_kwargs(0.0, None, "dpo", None)
    assert TP._loss_kwargs(0.0, None, "ppo", None) == {}
