"""Adafactor on the GPU: the five-launch update against the float32 numpy restatement of optax's chain (tests/_adafactor_oracle.py) on every
orientation, tail and branch; bit-reproducibility; the lowered factoring threshold; the train state in full and LoRA mode; the entry point."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from ddpo_amd import lib as L                                           # noqa: E402
from ddpo_amd import lib_optim as LO                                    # noqa: E402
from ddpo_amd.models.unet import ParamStore, UNet2DCondition, UNetConfig   # noqa: E402
from oracle.optim import AccumulatingState                              # noqa: E402
from _adafactor_oracle import Adafactor, state_from_flat                # noqa: E402

DEV = "cuda"
F = np.float32
# the AdamW gates of tests/test_gpu_kernel_branches.py::test_adamw_tail_and_grid_stride for p; rtol 1e-5 for the state
P_RTOL, P_ATOL, V_RTOL = 1e-6, 1e-7, 1e-5
LR, WD, MAX_NORM, INV_N = 1e-2, 1e-4, 1.0, 0.5

# both orientations of a 3x3 conv and of a dense kernel with a partial row tile (130, 136 and 257 rows against tiles of 128) and partial column
# passes (130 and 136 columns against 256; 257 = one pass + 1; 130 and 257 columns are no multiple of 4: the scalar path); a square that
# fills exactly one tile; second-largest dimension 127 and a conv with 4 input channels: unfactored, the first over 10 chunks of 4096;
# vectors with tails of 2, 1 and 1 elements, the 5-vector with p = 0 (min_scale)
SHAPES = [(3, 3, 136, 130), (3, 3, 130, 136), (1, 1, 128, 128), (130, 257), (257, 130), (127, 300), (3, 3, 4, 130), (130,), (5,), (1,)]
ZERO_P, ZERO_G_ON_SECOND = 8, 2                 # indices into SHAPES
# global norm ~2e4, ~0.2, ~2e6: clipped, not clipped, clipped.  The second update's gradient is far below the first's second moment (block RMS of
# u well under 1), the third's far above it (u ~ (1 - beta)^(-1/2) = 1.55: block RMS over 1)
GRAD_SCALE = [1.0, 1e-5, 1e2]
PAD, PAD_G = 7.5, 0.015625                      # sentinels in the alignment padding between tensors, parameters and gradients


def _case(shapes, seed, zero_p=None, zero_g=None):
    """(params, [grads of update 1, 2, 3]) as float32 numpy lists.  |g| spreads over four decades inside every tensor."""
    rng = np.random.default_rng(seed)
    params = [rng.standard_normal(s).astype(F) for s in shapes]
    if zero_p is not None:
        params[zero_p][...] = 0
    grads = []
    for k, scale in enumerate(GRAD_SCALE):
        gs = [(rng.standard_normal(s) * 10.0 ** rng.uniform(-2, 2, s) * scale).astype(F) for s in shapes]
        if k == 1 and zero_g is not None:
            gs[zero_g][...] = 0
        grads.append(gs)
    return params, grads


def _stores(shapes, params):
    named = {f"t{i}": s for i, s in enumerate(shapes)}
    p, g = ParamStore(named, DEV), ParamStore(named, DEV)
    p.flat.fill_(PAD)
    g.flat.fill_(PAD_G)
    for i, a in enumerate(params):
        p[f"t{i}"].copy_(torch.from_numpy(a))
    return p, g


def _pad_mask(store):
    m = torch.ones(store.flat.numel(), dtype=torch.bool)
    for n, o in store.offsets.items():
        m[o:o + store[n].numel()] = False
    return m


def _run_device(shapes, params, grads, min_dim, zero_grad=(True, True, False)):
    """Three updates; returns per update (p flat, v flat, g flat) on the host, the plan and the stores."""
    p, g = _stores(shapes, params)
    plan = LO.AdafactorPlan.for_store(p, min_dim).to(DEV)
    v = plan.new_state()
    sq = torch.zeros(1, dtype=torch.float64, device=DEV)
    out = []
    for k, gs in enumerate(grads):
        for i, a in enumerate(gs):
            g[f"t{i}"].copy_(torch.from_numpy(a) / INV_N)          # the accumulated SUM; the kernel scales by inv_n (exact: 0.5)
        # the padding of g holds the sentinel: ddpo_grad_sqnorm reads the whole flat buffer, so the norm the kernel clips by includes it
        L.grad_sqnorm(g.flat, sq)
        LO.adafactor_step(p.flat, g.flat, v, plan, sq, INV_N, LR, k, WD, MAX_NORM, zero_grad=zero_grad[k])
        torch.cuda.synchronize()
        out.append((p.flat.cpu(), v.cpu(), g.flat.cpu()))
    return out, plan, p, g


def _oracle_grads(shapes, grads, store):
    """The gradients the oracle is fed: the test's, plus one extra 'tensor' holding the sentinel padding of the flat gradient buffer, which the
    global norm of the device path includes (its parameter is never compared)."""
    npad = int(_pad_mask(store).sum())
    return [gs + [np.full((npad,), PAD_G * INV_N, F)] for gs in grads] if npad else grads


def _check_against_oracle(shapes, seed, min_dim, zero_p=None, zero_g=None, want_branches=False):
    params, grads = _case(shapes, seed, zero_p, zero_g)
    dev, plan, pstore, gstore = _run_device(shapes, params, grads, min_dim)
    pad = _pad_mask(pstore)
    npad = int(pad.sum())
    ogr = _oracle_grads(shapes, grads, pstore)
    oparams = params + [np.zeros((npad,), F)] if npad else params
    o32, o64 = Adafactor(LR, WD, MAX_NORM, min_dim), Adafactor(LR, WD, MAX_NORM, min_dim, dtype=np.float64)
    s32, s64 = o32.init(oparams), o64.init(oparams)
    p32, p64 = oparams, [a.astype(np.float64) for a in oparams]
    worst_v = worst_o = 0.0
    for k in range(3):
        p32, s32, _ = o32.update(p32, ogr[k], s32)
        p64, s64, _ = o64.update(p64, ogr[k], s64)
        pf, vf, gf = dev[k]
        for i, s in enumerate(shapes):
            o = pstore.offsets[f"t{i}"]
            got = pf[o:o + p32[i].size].numpy().reshape(s)
            np.testing.assert_allclose(got, p32[i], rtol=P_RTOL, atol=P_ATOL, err_msg=f"p, tensor {i} {s}, update {k + 1}")
            # lr = 1e-2: the applied update is at least 1e3 x the gate wherever the parameter is of order 1
        got_v = state_from_flat(plan, vf.numpy())
        for i, s in enumerate(shapes):
            for key, ref in s32["v"][i].items():
                gv = got_v[i][key]
                worst_v = max(worst_v, float(np.max(np.abs(gv - ref) / np.abs(ref))))
                worst_o = max(worst_o, float(np.max(np.abs(ref - s64["v"][i][key]) / np.abs(s64["v"][i][key]))))
                np.testing.assert_allclose(gv, ref, rtol=V_RTOL, atol=0, err_msg=f"{key}, tensor {i} {s}, update {k + 1}")
        # g is zeroed exactly when asked (updates 1 and 2), kept on update 3; the padding of p and g is never touched
        gt = gf[~pad]
        assert bool((gt == 0).all()) == (k < 2)
        if k == 2:
            want = torch.cat([torch.from_numpy(a).reshape(-1) for a in grads[2]]) / INV_N
            assert torch.equal(gt, want)
        assert bool((pf[pad] == PAD).all()) and bool((gf[pad] == PAD_G).all())
    print(f"adafactor state: device vs float32 oracle max rel {worst_v:.3e}; float32 vs float64 oracle max rel {worst_o:.3e}")
    if want_branches:
        tr = o32.trace
        assert [t["global_clip"] for t in tr] == [True, False, True], [t["grad_norm"] for t in tr]
        clips = [c for t in tr for c in t["block_rms_clip"][:len(shapes)]]
        assert any(clips) and not all(clips)
        floors = [t["min_scale"][:len(shapes)] for t in tr]
        assert all(f[ZERO_P] for f in floors[:1]) and not any(f[i] for f in floors for i in range(len(shapes)) if i != ZERO_P)
        kinds = [bool(t.factored) for _, _, t in plan.entries]
        assert kinds == [True, True, True, True, True, False, False, False, False, False]
        assert [t.norm_rows for _, _, t in plan.entries][:5] == [0, 1, 1, 1, 0]
    return dev


def test_three_updates_match_the_float32_oracle_on_every_branch():
    _check_against_oracle(SHAPES, 0, 128, zero_p=ZERO_P, zero_g=ZERO_G_ON_SECOND, want_branches=True)


def test_updates_are_bit_identical_from_run_to_run():
    params, grads = _case(SHAPES, 1, ZERO_P, ZERO_G_ON_SECOND)
    a = _run_device(SHAPES, params, grads, 128)[0]
    b = _run_device(SHAPES, params, grads, 128)[0]
    for (pa, va, _), (pb, vb, _) in zip(a, b):
        assert torch.equal(pa, pb) and torch.equal(va, vb)


def test_lower_threshold_reaches_small_tiles_and_both_orientations():
    """min_dim_size_to_factor = 8: (3,3,8,12) factors as 9 slabs of 8 x 12 (row statistics normalised), (12,8) with the column statistics normalised."""
    _check_against_oracle([(3, 3, 8, 12), (12, 8)], 2, 8)


def _unet(seed=0):
    unet = UNet2DCondition(UNetConfig.named("tiny"), DEV)
    unet.params.init_synthetic(seed)
    return unet


def _fwd_bwd(unet, seed, B=2, hw=8):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, hw, hw, generator=g).to(DEV)
    ts = torch.tensor([981, 21][:B], dtype=torch.int32).to(DEV)
    ctx = torch.randn(B, 77, unet.cfg.cross_attention_dim, generator=g).to(DEV)
    d_out = torch.randn(B, 4, hw, hw, generator=g).to(DEV)
    tape = []
    unet.forward(x, ts, ctx, tape=tape)
    unet.backward(tape, d_out)


def _compare_store(store, plan, v, names, ostate):
    got_v = state_from_flat(plan, v.cpu().numpy())
    for i, n in enumerate(names):
        np.testing.assert_allclose(store[n].cpu().numpy(), ostate.params[i], rtol=P_RTOL, atol=P_ATOL, err_msg=n)
        for key, ref in ostate.opt_state["v"][i].items():
            np.testing.assert_allclose(got_v[i][key], ref, rtol=V_RTOL, atol=0, err_msg=f"{n} {key}")


def test_train_state_accumulates_then_updates_like_the_oracle():
    """Two micro-steps, the second closing an update, against oracle.optim.AccumulatingState driving the numpy Adafactor on the engine's own gradients."""
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdafactorConfig
    unet = _unet()
    state = AccumulatingTrainState(unet, AdafactorConfig(learning_rate=LR))
    assert state.plan.n_factored == 105 and state.opt_state["v"].numel() == 1687780
    names = list(unet.params.views)
    ostate = AccumulatingState([unet.params[n].cpu().numpy() for n in names], Adafactor(LR, 1e-4, 1.0))
    before = unet.params.flat.clone()
    _fwd_bwd(unet, 1)
    g0 = {n: unet.grads[n].cpu() for n in names}
    ostate.apply_gradients([g0[n].numpy() for n in names], do_update=False)
    state.apply_gradients(do_update=False)
    _fwd_bwd(unet, 2)
    # the second micro-step's own gradient: what the buffer gained (the oracle adds it back to the first in float32, as the kernels did)
    ostate.apply_gradients([(unet.grads[n].cpu().double() - g0[n].double()).float().numpy() for n in names], do_update=True)
    state.apply_gradients(do_update=True)
    torch.cuda.synchronize()
    assert state.step == 1 and state.n_acc == 0 and state.opt_state["count"] == 1 and float(unet.grads.flat.abs().max()) == 0.0
    assert float(state.last_grad_norm) == pytest.approx(float(ostate.last_grad_norm), rel=1e-3)
    assert not torch.equal(unet.params.flat, before)
    _compare_store(unet.params, state.plan, state.opt_state["v"], names, ostate)


def test_lora_mode_updates_the_adapters_through_the_same_table():
    from ddpo_amd.models.lora import LoraStore
    from ddpo_amd.training.policy_gradient import AccumulatingTrainState, AdafactorConfig
    unet = _unet()
    st = LoraStore(unet, 4, seed=2)
    g = torch.Generator().manual_seed(5)
    for n, v in st.params.views.items():
        if n.endswith(".B"):
            v.copy_(torch.randn(v.shape, generator=g) * 0.02)
    st.merge()
    state = AccumulatingTrainState(unet, AdafactorConfig(learning_rate=LR), lora=st)
    assert state.plan.n_factored == 0 and state.opt_state["v"].numel() == st.n_params       # (K, 4) and (4, N): unfactored
    names = list(st.params.views)
    ostate = AccumulatingState([st.params[n].cpu().numpy() for n in names], Adafactor(LR, 1e-4, 1.0))
    before = unet.params.flat.clone()
    _fwd_bwd(unet, 3)
    ostate.apply_gradients([st.grads[n].cpu().numpy() for n in names], do_update=True)
    state.apply_gradients(do_update=True)
    torch.cuda.synchronize()
    assert float(state.last_grad_norm) == pytest.approx(float(ostate.last_grad_norm), rel=1e-3)
    _compare_store(st.params, state.plan, state.opt_state["v"], names, ostate)
    for n, v in unet.params.views.items():                    # only the adapted kernels moved, to W0 + s A' B'
        o = unet.params.offsets[n]
        if n not in st.targets:
            assert torch.equal(v.reshape(-1), before[o:o + v.numel()]), n
    for n in st.targets:
        A, B = st.layer(n)[:2]
        ref = st.base[n].double() + st.scale * (A.double() @ B.double())
        assert float((unet.params[n].double() - ref).abs().max() / ref.abs().max()) <= 1e-6, n


def test_entrypoint_runs_adafactor_and_refuses_to_resume_it_as_adamw(tmp_path, monkeypatch):
    """One epoch of pipeline/policy_gradient.py --optimizer adafactor on the argument set of tests/test_gpu_entrypoint.py::test_entrypoint_single_process;
    main() returning is the script's exit status 0 (a SystemExit or any other exception fails the test)."""
    import importlib
    import json
    from ddpo_amd.utils.serialization import load_unet
    monkeypatch.setenv("DDPO_MODEL_CONFIG", "tiny")
    monkeypatch.chdir(tmp_path)
    pg = importlib.import_module("pipeline.policy_gradient")
    flags = ["--dataset", "compressed-animals", "--resolution", "64", "--n_inference_steps", "4", "--sample_batch_size", "2",
             "--train_batch_size", "2", "--num_train_epochs", "1", "--save_freq", "1", "--per_prompt_stats_min_count", "2",
             "--learning_rate", "1e-4", "--logbase", str(tmp_path / "run")]
    args = pg.Parser(flags).parse_args("pg")
    pipe0, _ = load_unet(None, epoch=args.load_epoch, pretrained_model=args.pretrained_model, dtype=args.dtype, cache=args.cache,
                         device=torch.device("cuda", 0), seed=0)
    w0 = pipe0.unet.params.flat.clone()
    out = pg.main(flags + ["--optimizer", "adafactor"])
    state = out["state"]
    assert len(out["mean_rewards"]) == 1 and np.isfinite(out["mean_rewards"][0])
    assert state.step == 1 and set(state.opt_state) == {"count", "v"}
    assert bool(torch.isfinite(state.params.flat).all()) and not torch.equal(state.params.flat, w0)        # the optimizer moved the weights
    assert json.load(open(os.path.join(out["localpath"], "args.json")))["optimizer"] == "adafactor"
    ck = os.path.join(str(tmp_path / "run"), "models/pg/checkpoints")
    rs = torch.load(os.path.join(ck, "resume_0.pt"), map_location="cpu", weights_only=False)
    assert rs["optimizer"] == "adafactor" and "mu" not in rs and "nu" not in rs
    assert rs["v"].dtype == torch.float32 and rs["v"].numel() == 1687780 and torch.equal(rs["v"], state.opt_state["v"].cpu())
    assert float(rs["v"].min()) > 0.0
    monkeypatch.setenv("DDPO_RESUME", ck)
    with pytest.raises(SystemExit, match="--optimizer adafactor.*--optimizer adamw"):
        pg.main(flags + ["--optimizer", "adamw"])
