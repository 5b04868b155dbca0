"""CPU-only checks of the Adafactor boundary: include/ddpo_optim.h against lib_optim._SIGS and the library's exports (its own ABI version,
nothing of it in ddpo_hip.h), the host-built tensor table against an independent statement of optax's factoring rule on the three U-Net
inventories, the plan validator, and the entry point's optimizer dispatch and resume check.  No device compute is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

from ddpo_amd import lib as L
from ddpo_amd import lib_optim as LO
from oracle import unet as OU

from _abi_check import check_signatures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "ddpo_optim.h")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def test_signatures_match_the_header_prototypes():
    """tests/test_abi_cpu.py::test_signatures_match_the_header_prototypes, applied to include/ddpo_optim.h and lib_optim._SIGS."""
    check_signatures(HDR, LO._SIGS, 4)


def test_library_exports_every_declared_symbol_under_its_own_version():
    declared = set(re.findall(r"\b(ddpo_[a-z0-9_]+)\s*\(", _header()))
    assert declared == set(LO.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in ddpo_optim.h but not exported"
    assert LO.load().ddpo_optim_abi_version() == LO.ABI_VERSION == 1
    # the optimizer is versioned on its own: ddpo_hip.h, lib.ABI_VERSION and lib._SIGS know nothing of it
    main = open(os.path.join(ROOT, "include", "ddpo_hip.h")).read()
    for name in LO.EXPORTED_SYMBOLS:
        assert name not in main and name not in L._SIGS


def test_struct_mirror_and_header_constants():
    assert LO.load().ddpo_sizeof_adafactor_tensor() == ctypes.sizeof(LO.AdafactorTensor)
    hdr = _header()
    body = hdr[hdr.index("typedef struct"):hdr.index("} ddpo_adafactor_tensor;")].split("{", 1)[1]
    names = []
    for stmt in body.split(";"):
        stmt = re.sub(r"^\s*(int64_t|int32_t)\s+", "", stmt.strip())
        names += [n.strip() for n in stmt.split(",") if n.strip()]
    assert names == [f[0] for f in LO.AdafactorTensor._fields_]
    assert int(re.search(r"#define DDPO_ADAFACTOR_TILE_ROWS (\d+)", hdr).group(1)) == LO.TILE_ROWS
    assert int(re.search(r"#define DDPO_ADAFACTOR_CHUNK (\d+)", hdr).group(1)) == LO.CHUNK


def _offsets(shapes):
    off, out = 0, {}
    for n, s in shapes.items():
        out[n] = off
        off += (int(np.prod(s)) + 3) // 4 * 4
    return out, off


@pytest.mark.parametrize("name,ocfg,n_state", [("sd15", OU.SD15, 1887940), ("sd21", OU.SD21, 1896132), ("tiny", OU.TINY, 1687780)])
def test_plan_follows_the_argsort_rule(name, ocfg, n_state):
    shapes = OU.unet_param_shapes(ocfg)
    offsets, numel = _offsets(shapes)
    plan = LO.AdafactorPlan(shapes, offsets, numel)
    assert plan.n_state == n_state and len(plan.entries) == len(shapes)
    tile = state = n_fact = 0
    for (pname, shape, t), (sname, sshape) in zip(plan.entries, shapes.items()):
        assert pname == sname and tuple(shape) == tuple(sshape)
        # optax's rule, restated here: factor over the two largest axes when the second largest is at least 128
        order = np.argsort(sshape, kind="stable")
        factored = len(sshape) >= 2 and sshape[order[-2]] >= 128
        assert bool(t.factored) == factored, pname
        n = int(np.prod(sshape))
        assert (t.off, t.numel, t.first_tile, t.v_off) == (offsets[pname], n, tile, state)
        if factored:
            d1, d0 = int(order[-2]), int(order[-1])
            assert {d1, d0} == {len(sshape) - 2, len(sshape) - 1}
            assert (t.R, t.C, t.S) == (sshape[-2], sshape[-1], n // (sshape[-2] * sshape[-1]))
            assert t.norm_rows == int(d0 == len(sshape) - 1) and t.vc_off == state + t.S * t.R
            assert t.n_tiles == t.S * -(-t.R // 128)
            state += n // sshape[d0] + n // sshape[d1]          # v_row and v_col
            n_fact += 1
        else:
            assert (t.S, t.R, t.C) == (1, 1, n) and t.n_tiles == -(-n // 4096)
            state += n
        tile += t.n_tiles
    assert (tile, state) == (plan.n_tiles, plan.n_state) and n_fact == plan.n_factored
    # the work list: every (tensor, tile) once, then every (tensor, slab) of the factored tensors in table order
    work = [tuple(w) for w in plan.work[:plan.n_tiles]]
    assert sorted(work) == [(i, k) for i, (_, _, t) in enumerate(plan.entries) for k in range(t.n_tiles)]
    assert [tuple(w) for w in plan.work[plan.n_tiles:]] == [(i, s) for i, (_, _, t) in enumerate(plan.entries) if t.factored for s in range(t.S)]
    if name == "sd15":
        assert n_fact == 280 and len(shapes) == 686
    if name == "tiny":
        assert n_fact == 105
    assert plan.workspace_bytes() > 0               # the C validator accepts what the builder made


def test_plan_refuses_factored_axes_that_are_not_the_last_two():
    with pytest.raises(ValueError, match="last two"):
        LO.AdafactorPlan({"w": (130, 3, 140)}, {"w": 0}, 130 * 3 * 140)
    LO.AdafactorPlan({"w": (3, 130, 140)}, {"w": 0}, 3 * 130 * 140)
    plan = LO.AdafactorPlan({"a": (3, 3, 8, 12), "b": (12, 8)}, {"a": 0, "b": 864}, 960, min_dim_size_to_factor=8)
    assert [(t.S, t.R, t.C, t.norm_rows) for _, _, t in plan.entries] == [(9, 8, 12, 1), (1, 12, 8, 0)]
    assert LO.AdafactorPlan({"a": (64, 4), "b": (4, 320)}, {"a": 0, "b": 256}, 1536).n_factored == 0       # LoRA adapters, r < 128


def test_validator_rejects_inconsistent_plans_and_step_rejects_bad_arguments():
    def plan():
        return LO.AdafactorPlan({"a": (130, 257), "b": (5,)}, {"a": 0, "b": 33412}, 33420)
    assert plan().workspace_bytes() > 0
    for field, value in (("off", 16), ("numel", 5), ("v_off", 1 << 40), ("vc_off", -1), ("ws_off", 4), ("R", 131), ("norm_rows", 0),
                         ("first_tile", 1), ("n_tiles", 3), ("factored", 2), ("reserved", 1)):
        p = plan()
        setattr(p.tensors[0], field, value)
        with pytest.raises(L.DdpoHipError):
            p.workspace_bytes()
    p = plan()
    p.tensors[1].off = 33416                                    # 5 elements from 33416 run past the flat buffer
    with pytest.raises(L.DdpoHipError):
        p.workspace_bytes()
    p = plan()
    p.work[0, 1] = 1                                            # the work list must name every tile exactly once (here: one twice)
    with pytest.raises(L.DdpoHipError):
        p.workspace_bytes()
    p = plan()
    p.work[-1, 0] = 1                                           # the slab list too
    with pytest.raises(L.DdpoHipError):
        p.workspace_bytes()
    lib = LO.load()
    assert lib.ddpo_adafactor_workspace_bytes(None, 1, None, 1, 0, 4, 4) == 0
    assert lib.ddpo_adafactor_step(None, None, None, None, 1, None, 1, 0, 4, None, 1.0, 1e-2, 0.0, 1e-30, 1.0, 1e-3, 0.0, 1.0, 1,
                                   None, 0, None) == -1


def test_beta_is_zero_on_the_first_update():
    assert LO.beta_t(0) == 0.0
    assert LO.beta_t(1) == float(np.float32(1) - np.float32(2) ** np.float32(-0.8))


def test_parser_and_train_state_accept_adafactor(tmp_path, monkeypatch):
    import torch
    from ddpo_amd.models.unet import UNet2DCondition, UNetConfig
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdafactorConfig, AdamWConfig
    from pipeline import policy_gradient as pg
    monkeypatch.chdir(tmp_path)
    args = pg.Parser(["--dataset", "compressed-animals", "--optimizer", "adafactor", "--learning_rate", "1e-4", "--logbase",
                      str(tmp_path / "run")]).parse_args("pg")
    tx = pg.make_optimizer(args)
    assert isinstance(tx, AdafactorConfig) and tx.name == "adafactor"
    assert (tx.learning_rate, tx.weight_decay, tx.max_grad_norm, tx.min_dim_size_to_factor) == (1e-4, args.weight_decay, args.max_grad_norm, 128)
    args.set("optimizer", "adamw")
    assert isinstance(pg.make_optimizer(args), AdamWConfig)
    args.set("optimizer", "lion")
    with pytest.raises(NotImplementedError, match="lion"):
        pg.make_optimizer(args)
    unet = UNet2DCondition(UNetConfig.named("tiny"), "cpu")
    state = AccumulatingTrainState(unet, tx)
    assert set(state.opt_state) == {"count", "v"} and state.opt_state["count"] == 0
    assert state.opt_state["v"].dtype == torch.float32 and state.opt_state["v"].numel() == 1687780 == state.plan.n_state
    assert set(AccumulatingTrainState(unet, AdamWConfig()).opt_state) == {"count", "mu", "nu"}


def test_resume_refuses_a_bundle_of_the_other_optimizer():
    from ddpo_amd.training.policy_gradient import AdafactorConfig, AdamWConfig
    from pipeline import policy_gradient as pg
    pg.check_resume_optimizer({"epoch": 0, "optimizer": "adafactor"}, AdafactorConfig(), "run/checkpoints")
    pg.check_resume_optimizer({"epoch": 0}, AdamWConfig(), "run/checkpoints")           # bundles from before the field are AdamW's
    with pytest.raises(SystemExit, match="--optimizer adafactor.*--optimizer adamw"):
        pg.check_resume_optimizer({"epoch": 3, "optimizer": "adafactor"}, AdamWConfig(), "run/checkpoints")
    with pytest.raises(SystemExit, match="--optimizer adamw.*--optimizer adafactor"):
        pg.check_resume_optimizer({"epoch": 3}, AdafactorConfig(), "run/checkpoints")
