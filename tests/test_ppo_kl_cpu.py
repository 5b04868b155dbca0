"""CPU-only checks of the `--kl_coef` boundary: include/ddpo_ppo_kl.h against lib_ppo_kl._SIGS and the library's exports (its own ABI version,
nothing of it in ddpo_hip.h), the flag in the configuration and the entry point's argument check, the entry's argument validation (which
returns before any launch), and the float64 oracle of the penalty (tests/_kl_oracle.py) against torch.distributions and against its own
autograd.  No device compute is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from ddpo_amd import lib as L
from ddpo_amd import lib_ppo_kl as LK
from oracle.ddim import DDIMOracle

import _kl_oracle as KO
from _abi_check import check_signatures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "ddpo_ppo_kl.h")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def test_signatures_match_the_header_prototypes():
    """tests/test_abi_cpu.py::test_signatures_match_the_header_prototypes, applied to include/ddpo_ppo_kl.h and lib_ppo_kl._SIGS."""
    check_signatures(HDR, LK._SIGS, 2)


def test_library_exports_every_declared_symbol_under_its_own_version():
    declared = set(re.findall(r"\b(ddpo_[a-z0-9_]+)\s*\(", _header()))
    assert declared == set(LK.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in ddpo_ppo_kl.h but not exported"
    assert LK.load().ddpo_ppo_kl_abi_version() == LK.ABI_VERSION == 1
    # versioned on its own: ddpo_hip.h, lib.ABI_VERSION and lib._SIGS know nothing of it
    main = open(os.path.join(ROOT, "include", "ddpo_hip.h")).read()
    for name in LK.EXPORTED_SYMBOLS:
        assert name not in main and name not in L._SIGS


def test_binding_refuses_a_version_mismatch(monkeypatch):
    monkeypatch.setattr(LK, "_lib", None)
    monkeypatch.setattr(LK, "ABI_VERSION", 2)
    with pytest.raises(L.DdpoHipError, match="KL-penalty ABI version 1.*expects 2"):
        LK.load()
    assert LK._lib is None


def test_config_default_and_parser(tmp_path, monkeypatch):
    import config.base as C
    from pipeline import policy_gradient as pg
    monkeypatch.chdir(tmp_path)
    assert C.base["pg"]["kl_coef"] == 0.0
    assert "kl_coef" not in C.base["sample"] and "kl_coef" not in C.base["train"]
    common = ["--dataset", "compressed-animals", "--logbase", str(tmp_path / "run")]
    assert pg.Parser(common).parse_args("pg").kl_coef == 0.0
    args = pg.Parser(common + ["--kl_coef", "0.05"]).parse_args("pg")
    assert args.kl_coef == 0.05 and isinstance(args.kl_coef, float)
    assert pg.check_kl_args(args) is None


def test_argument_check_rejects_negative_and_deterministic_sampling(tmp_path, monkeypatch):
    from ddpo_amd.training.kl_reference import check_kl_args
    from pipeline import policy_gradient as pg
    assert check_kl_args(0.0, 1.0) is None and check_kl_args(0.0, 0.0) is None and check_kl_args(0.1, 1.0) is None
    assert "finite number >= 0" in check_kl_args(-0.1, 1.0)
    assert "finite number >= 0" in check_kl_args(float("nan"), 1.0) and "finite number >= 0" in check_kl_args(float("inf"), 1.0)
    assert "--eta 0" in check_kl_args(0.1, 0.0)
    monkeypatch.chdir(tmp_path)
    common = ["--dataset", "compressed-animals", "--logbase", str(tmp_path / "run")]
    assert "finite number >= 0" in pg.check_kl_args(pg.Parser(common + ["--kl_coef", "-1"]).parse_args("pg"))
    assert "--eta 0" in pg.check_kl_args(pg.Parser(common + ["--kl_coef", "0.1", "--eta", "0"]).parse_args("pg"))


def test_entry_rejects_bad_arguments_before_any_launch():
    """Every DDPO_EINVAL case of include/ddpo_ppo_kl.h on host buffers: the checks come before the first launch, so no device is touched."""
    fn = LK.load().ddpo_ddim_kl_ref_fwd_bwd
    B, group, chw = 4, 2, 8
    bufs = [np.zeros(B * chw + 4, dtype=np.float32) for _ in range(6)]
    a16 = lambda a: a.ctypes.data + (-a.ctypes.data % 16)                  # 16-byte aligned address inside the buffer
    ec, eu, rc, ru, dc, du = (ctypes.c_void_p(a16(a)) for a in bufs)
    ts = np.ones(B, dtype=np.int32)
    tsp = ctypes.c_void_p(ts.ctypes.data)
    small = [np.zeros(B, dtype=np.float32) for _ in range(2)]
    kp, ki = (ctypes.c_void_p(a.ctypes.data) for a in small)
    acp = np.ones(1000, dtype=np.float32)

    def consts(pred=0):
        return L.DdimConsts(acp.ctypes.data, 1000, 20, 1.0, 1.0, pred)

    def call(ec=ec, eu=eu, rc=rc, ru=ru, ts=tsp, g=5.0, kl=0.1, cfg=1, c=None, dc=dc, du=du, kp=kp, ki=ki, B=B, group=group, chw=chw, pred=0):
        cc = consts(pred)
        return fn(ec, eu, rc, ru, ts, g, kl, cfg, ctypes.byref(cc) if c is None else c, dc, du, kp, ki, None, B, group, chw, None)

    null = ctypes.c_void_p(0)
    for kw in (dict(ec=null), dict(rc=null), dict(ts=null), dict(dc=null), dict(kp=null), dict(ki=null), dict(c=ctypes.POINTER(L.DdimConsts)()),
               dict(eu=null), dict(ru=null), dict(du=null),                       # required under train_cfg
               dict(B=0), dict(B=-4), dict(group=0), dict(group=3), dict(chw=0), dict(chw=6),
               dict(kl=-0.1), dict(kl=float("nan")), dict(kl=float("inf")),
               dict(pred=L.PRED_TYPES["sample"]),
               dict(ec=ctypes.c_void_p(ec.value + 4))):                            # float4 access: 16-byte alignment
        assert call(**kw) == -1, kw
    for a in bufs + small:
        assert not a.any()


# ------------------------------------------------------------------------------------------------ the oracle checks itself
def _case(pred, train_cfg, B=5, shape=(4, 6, 6), seed=0):
    dd = DDIMOracle(prediction_type=pred)
    st = dd.set_timesteps(dd.create_state(), 50)
    g = torch.Generator().manual_seed(seed + 7 * (pred == "epsilon") + int(train_cfg))
    ec, eu, x = (torch.randn(B, *shape, generator=g, dtype=torch.float64) for _ in range(3))
    rc = ec + 1e-2 * torch.randn(B, *shape, generator=g, dtype=torch.float64)
    ru = eu + 1e-2 * torch.randn(B, *shape, generator=g, dtype=torch.float64)
    ts = np.asarray([981, 1, 481, 21, 961], dtype=np.int32)[:B]
    return dd, st, ec, (eu if train_cfg else None), rc, (ru if train_cfg else None), x, ts


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("train_cfg", [True, False])
def test_oracle_kl_is_the_kl_of_the_two_gaussians(pred, train_cfg):
    dd, st, ec, eu, rc, ru, x, ts = _case(pred, train_cfg)
    kl = KO.kl_rows_torch(dd, st, ec, eu, rc, ru, ts, 5.0, 1.0, train_cfg)
    ref = KO.kl_rows_by_distributions(dd, st, ec, eu, rc, ru, ts, x, 5.0, 1.0, train_cfg)
    assert kl.shape == (5,) and float(kl.min()) > 0
    # mu_theta - mu_ref cancels ~1e-2 |c_t| out of |mu| ~ 1 in float64: 1e-16 / 1e-2 / c_t, squared terms -> a few 1e-11 relative at t = 1
    np.testing.assert_allclose(kl.numpy(), ref.numpy(), rtol=1e-9, atol=0)
    # the restated mean is the oracle's: DDIMOracle.step with zero noise returns it (fp32)
    mu = KO.ddim_mean_torch(dd, st, KO.guided(ec, eu, 5.0, train_cfg), ts, x, 1.0)
    guided32 = KO.guided(ec, eu, 5.0, train_cfg).numpy().astype(np.float32)
    step_mean, _ = dd.step(st, guided32, ts, x.numpy().astype(np.float32), noise=np.zeros(x.shape, dtype=np.float32), eta=1.0)
    np.testing.assert_allclose(step_mean, mu.numpy(), rtol=0, atol=2e-5)
    # equal networks: exactly zero, not merely small
    assert float(KO.kl_rows_torch(dd, st, ec, eu, ec, eu, ts, 5.0, 1.0, train_cfg).abs().max()) == 0.0


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("train_cfg", [True, False])
def test_oracle_autograd_equals_the_closed_form_gradient(pred, train_cfg):
    dd, st, ec, eu, rc, ru, x, ts = _case(pred, train_cfg, B=4, seed=3)
    group, kl_coef = 2, 0.3
    tec = ec.clone().requires_grad_(True)
    teu = eu.clone().requires_grad_(True) if train_cfg else None
    kl = KO.kl_rows_torch(dd, st, tec, teu, rc, ru, ts, 5.0, 1.0, train_cfg)
    (kl_coef * kl.reshape(-1, group).mean(1).sum()).backward()
    gc, gu = KO.kl_grad_closed_form(dd, st, ec, eu, rc, ru, ts, 5.0, 1.0, kl_coef, group, train_cfg)
    np.testing.assert_allclose(tec.grad.numpy(), gc.numpy(), rtol=1e-12, atol=0)
    if train_cfg:
        np.testing.assert_allclose(teu.grad.numpy(), gu.numpy(), rtol=1e-12, atol=0)
    # and the fp32 restatement of the HIP pass says the same to fp32 accuracy
    f = lambda t: None if t is None else t.numpy().astype(np.float32)
    kb, ki, ic, iu = KO.closed_form_numpy(dd, st, f(ec), f(eu), f(rc), f(ru), ts, 5.0, 1.0, kl_coef, group, train_cfg)
    t64 = lambda a: None if a is None else torch.from_numpy(a).double()
    kl32 = KO.kl_rows_torch(dd, st, t64(f(ec)), t64(f(eu)), t64(f(rc)), t64(f(ru)), ts, 5.0, 1.0, train_cfg)
    np.testing.assert_allclose(kb, kl32.numpy(), rtol=2e-5)
    np.testing.assert_allclose(ki, kl32.reshape(-1, group).mean(1).numpy(), rtol=2e-5)
    gc32, _ = KO.kl_grad_closed_form(dd, st, t64(f(ec)), t64(f(eu)), t64(f(rc)), t64(f(ru)), ts, 5.0, 1.0, kl_coef, group, train_cfg)
    assert float(np.abs(ic - gc32.numpy()).max() / np.abs(gc32.numpy()).max()) < 2e-5


def test_default_training_step_does_not_touch_the_binding():
    """kl_coef == 0: a fresh interpreter that imports the training step and the entry point has neither the binding nor the reference module."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import ddpo_amd.training.policy_gradient, pipeline.policy_gradient; "
            "assert 'ddpo_amd.lib_ppo_kl' not in sys.modules and 'ddpo_amd.training.kl_reference' not in sys.modules" % ROOT)
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
