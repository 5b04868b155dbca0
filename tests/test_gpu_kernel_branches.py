"""Every host-dispatch branch, grid-stride loop and ragged tail of the PPO / DDIM log-prob kernels, the optimizer kernels and the small
element-wise kernels (ddpo_amd/csrc/elementwise.hip and the element-wise half of backward.hip), each at the SMALLEST shape that enters it, against
float64 references.  The neighbouring tests (test_gpu_kernels.py, test_gpu_backward.py, test_fused_micro_steps.py, test_gpu_rwr.py) run one small
shape per kernel: one rung of the PPO ladder, one grid-stride iteration, no `n % 4` tail.

The shape tables come first; beside each row stands the branch it enters.  `test_ppo_tables_cover_every_rung` (CPU) re-derives those branches from
the dispatch rule and from the ladder spelled in elementwise.hip.
"""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

from ddpo_amd import lib as L
from oracle import diffusion as OD, ppo as OPPO
from oracle.ddim import DDIMOracle
from oracle.optim import AdamWBf16Mu, AccumulatingState

gpu = pytest.mark.gpu
DEV = "cuda"

# ------------------------------------------------------------------------------------------------ shape tables
# ddpo_ddim_logprob_ppo_fwd_bwd: nv = ceil(chw / 4 / 1024); cluster kernel ppo_cluster_kernel<NV> for B <= 64 and nv <= 16 with
# NV the first of {1, 2, 4, 8, 12, 16} that holds nv, else ppo_fwd_bwd_kernel + ppo_info_kernel.  Rows: (B, group, chw, branch).
PPO_CHW_TABLE = [
    (4, 4, 4, 1),                       # NV1, one float4: slices 1-3 of the four-workgroup cluster are empty
    (4, 4, 1028, 1),                    # NV1, slice 1 holds one float4
    (4, 4, 4096, 1),                    # NV1, full
    (4, 4, 4100, 2),                    # NV2, the second tile holds one float4
    (4, 4, 8196, 4),                    # NV4 (nv = 3)
    (4, 4, 16388, 8),                   # NV8 (nv = 5)
    (4, 4, 32772, 12),                  # NV12 (nv = 9)
    (4, 4, 49156, 16),                  # NV16 (nv = 13)
    (4, 4, 65536, 16),                  # NV16, full
    (4, 4, 65540, "fallback-by-size"),  # nv = 17: ppo_fwd_bwd_kernel + ppo_info_kernel
]
PPO_B_TABLE = [
    (64, 64, 256, 1),                   # the cluster kernel's documented batch limit, one micro-batch: 256 resident workgroups
    (64, 1, 256, 1),                    # ... 64 micro-batches of one row (every row completes its own info row)
    (65, 5, 256, "fallback-by-batch"),  # B > PPO_MAXB
]
PPO_BIT_CHW = [1028, 4100, 32772, 65536]        # cluster (B = 5) against fallback (the same rows tiled to B = 65): NV1 / NV2 / NV12 / NV16
PPO_STEP_CHW = [4, 4100, 65540]                 # ddim_step_kernel: one float4 / second loop iteration holds one float4 / 17th iteration
PPO_REARM = [(64, 1, 256), (6, 3, 4100), (64, 64, 256), (32, 8, 16388), (5, 5, 4), (65, 5, 256)]      # back to back on one stream

# optimizer: sqnorm_kernel caps its grid at 2048 blocks of 256 float4 lanes, adamw_kernel at 4096; thread 0 of block 0 runs the n % 4 tail
SQNORM_N = [
    1, 3,                               # no float4 at all: tail only
    4,                                  # one float4, no tail
    5,                                  # one float4 + tail of 1
    1027,                               # 256 float4 (one full block) + tail of 3
    2 * 2048 * 256 * 4 + 4 * 300 + 3,   # past the cap: 300 lanes run three iterations, the rest two; tail of 3
]
ADAMW_N = [
    1, 3,                               # tail only
    7,                                  # one float4 + tail of 3
    1026,                               # 256 float4 + tail of 2
    4096 * 256 * 4 + 4 * 100 + 3,       # past the cap: 100 lanes run a second iteration; tail of 3
]

QUICK_GELU_N = [1, 2, 3, 4, 7, 1025, 4096 * 256 * 4 + 6]      # tail only x3 / one float4 / +3 / 256 float4 + 1 / past the 4096-block cap + tail of 2
L2_SHAPES = [(1, 1), (5, 63), (7, 64), (9, 65), (6, 768), (1030, 3)]      # one lane / under, at, over one wave pass / 12 passes / 258 blocks, last one ragged
STAGE_CASES = [
    (4, 1200, 300),                     # one block: row (300 float4) and ts (300) loops run past the grid's first stride of 256; row_n > n
    (1024 * 256 * 4 + 8, 1280, 1024 * 256 + 5),     # past the 1024-block cap: main loop runs twice for two lanes; ts_n > the first stride
]
SOFTMAX_SHAPES = [(3, 1), (5, 255), (5, 256), (5, 257), (4, 4100), (65536 + 3, 8)]      # column loop under / at / over 256 threads, 17 passes; row loop past 65535 blocks
COLSUM_ROWS_PER_SEG = [1, 511, 512, 513, 1100]      # chunks of CS_ROWS = 512 per segment: 1 (one row), 1 ragged, 1 full, 2 (second holds one row), 3
COLSUM_COLS = [4, 60, 64, 68]                       # one float4 column lane / 15 of 16 / one full column block / a second column block with one lane
RWR_CHW = [4, 4100, 65540]                          # 1024-thread loop: one float4 / a second pass with one float4 / a 17th pass
TEMB_CASES = [(1, 2), (1, 6), (1, 320), (3, 320), (5, 6), (259, 2)]       # (B, dim): B * dim / 2 = 1, 3, 160, 480 (two blocks, ragged), 15, 259
# (kernel, block cap) of the plain grid-stride kernels: one case each at cap * 256 + 77 work items (a second iteration for 77 lanes) and one minimal case
STREAM_CAPS = {"geglu": 8192, "geglu_bwd": 8192, "silu": 4096, "silu_bwd": 4096, "add": 8192, "scale_shift_clip": 4096, "sumpool2x2": 16384,
               "copy_cols": 8192, "layout": 4096}

TS8 = [981, 1, 481, 21, 961, 501, 41, 241]
# old log-prob = log-prob + offset: +-3e-5 is well inside, +-3e-4 well outside clip_range = 1e-4.  With the advantages below rows 0 / 4 / 7 are
# inside the range, rows 1 / 2 / 5 outside it with the unclipped branch active (1 and 2 at +-ADV_CLIP_MAX), rows 3 / 6 clipped from above / below
# (zero gradient).  The advantages are mostly positive on purpose: a micro-batch whose +10 and -10 terms cancel has a loss of a few tenths made of
# terms of 10, and its RELATIVE error is then 30 x that of a ratio; here every micro-batch of the tables has |loss| >= 1.
OFF8 = [3e-5, 3e-4, -3e-4, -3e-4, -3e-5, 3e-4, 3e-4, -3e-5]
ADV8 = [8.0, 12.0, -20.0, 6.0, 5.0, 7.0, -3.0, 14.0]
# At chw = 4 the log-prob of the t = 1 row (sigma = 0.02, |mean| ~ 1) averages four terms that each carry ~5e-6 of fp32 rounding error (half an ulp
# of the mean over sigma): an fp32 evaluation is inside a quarter of the log-prob bound there for about one draw in five, and for all four of
# {epsilon, v_prediction} x {train_cfg, not} for about one seed in 500.  The seed of that row is such a one, found with the closed form on the host
# (asserted below, like for every other row).  The B = 65 row (eight t = 1 rows of 256 terms) has the closed form at 4e-7 .. 6e-7 of the 6.25e-7
# for most seeds and 3 % over for its plain one: it takes the next but one.  Every other row uses its plain seed.
PPO_SEED_SALT = {(4, 4): 851, (65, 256): 2}
GUIDE, CLIP = 5.0, 1e-4

# bounds of the PPO checks: 8 x the worst error of the fp32 closed form (oracle.ppo.closed_form_numpy) against float64 autograd on these inputs
# (log-prob 3.1e-7, gradient 5.9e-6 of max|grad|): a different summation order plus the device's sqrt / div / exp, a few ulp each.  The closed
# form itself has to sit inside a quarter of each bound, so the margin stays honest when the inputs change.
LP_ATOL, GRAD_REL, LOSS_REL = 2.5e-6, 5e-5, 1e-5


def _rel(a, b):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _record(line):
    from conftest import parity_record
    parity_record("[kernel branches] " + line)


def _ordered(a, bits=32):
    """Sign-magnitude float words (fp32, or bf16 as int16) -> integers in value order: a difference of two is a distance in ulp."""
    i = np.asarray(a).astype(np.int64)
    mask = (1 << (bits - 1)) - 1
    return np.where(i < 0, -(i & mask), i)


def _ulp_dist(a, b):
    return int(np.abs(_ordered(a.detach().cpu().numpy().view(np.int32)) - _ordered(b.detach().cpu().numpy().view(np.int32))).max())


# ------------------------------------------------------------------------------------------------ 4. guard on the PPO tables (CPU)
def _ppo_branch(B, chw, ladder=(1, 2, 4, 8, 12, 16), max_b=64):
    nv = -(-(chw // 4) // 1024)
    if B > max_b:
        return "fallback-by-batch"
    if nv > ladder[-1]:
        return "fallback-by-size"
    return next(r for r in ladder if nv <= r)


def test_ppo_tables_cover_every_rung():
    """The branch noted beside each row of the PPO tables is the one the dispatch rule gives, and the tables reach every rung and both fall-backs.
    IF YOU CHANGE THE LADDER (the PPO_LAUNCH chain, PPO_MAXB or the 1024-float4 tile of ddpo_ddim_logprob_ppo_fwd_bwd in
    ddpo_amd/csrc/elementwise.hip): move the `chw` rows of PPO_CHW_TABLE / PPO_BIT_CHW / PPO_REARM so that every rung still has a row whose LAST
    tile is ragged (one float4), plus a full one for the first and the last rung, and keep B at PPO_MAXB / PPO_MAXB + 1 in PPO_B_TABLE."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ddpo_amd", "csrc", "elementwise.hip")).read()
    ladder = tuple(int(v) for v in re.findall(r"PPO_LAUNCH\((\d+)\)", src))
    max_b = int(re.search(r"#define PPO_MAXB (\d+)", src).group(1))
    assert ladder == (1, 2, 4, 8, 12, 16) and max_b == 64, (ladder, max_b)
    for B, group, chw, branch in PPO_CHW_TABLE + PPO_B_TABLE:
        assert B % group == 0 and chw % 4 == 0
        assert _ppo_branch(B, chw) == branch == _ppo_branch(B, chw, ladder, max_b), (B, chw, branch)
    assert {r[3] for r in PPO_CHW_TABLE + PPO_B_TABLE} == {1, 2, 4, 8, 12, 16, "fallback-by-size", "fallback-by-batch"}
    assert [_ppo_branch(5, c) for c in PPO_BIT_CHW] == [1, 2, 12, 16] and all(_ppo_branch(65, c) == "fallback-by-batch" for c in PPO_BIT_CHW)
    assert {_ppo_branch(B, c) for B, _, c in PPO_REARM} == {1, 2, 8, "fallback-by-batch"}
    assert {B for B, _, _, _ in PPO_B_TABLE} == {max_b, max_b + 1}


# ------------------------------------------------------------------------------------------------ 1. PPO / DDIM log-prob dispatch
@functools.lru_cache(maxsize=None)
def _oracle_sched(pred):
    dd = DDIMOracle(prediction_type=pred)
    return dd, dd.set_timesteps(dd.create_state(), 50)


@functools.lru_cache(maxsize=None)
def _device_consts(pred):
    from ddpo_amd.diffusers_patch.scheduling_ddim import DDIMScheduler
    s = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", set_alpha_to_one=False, steps_offset=1,
                      prediction_type=pred)
    return s.kernel_consts(s.set_timesteps(s.create_state(device=DEV), 50), 1.0)


@functools.lru_cache(maxsize=8)
def _ppo_inputs(pred, train_cfg, B, chw):
    """eps_c, eps_u, x, z, x_next (the oracle's DDIM step from the guided prediction, or from the conditional one without train_cfg), ts,
    old log-probs, advantages: fp32 numpy, shape (B, 4, chw / 4, 1) (the wrapper only uses numel // B)."""
    dd, ost = _oracle_sched(pred)
    rng = np.random.default_rng(chw * 131 + B * 7 + 3 * (pred == "v_prediction") + int(train_cfg) + 1000003 * PPO_SEED_SALT.get((B, chw), 0))
    ec, eu, x, z = (rng.standard_normal((B, 4, chw // 4, 1), dtype=np.float32) for _ in range(4))
    ts = np.resize(np.asarray(TS8, dtype=np.int32), B)
    guided = (eu + np.float32(GUIDE) * (ec - eu)).astype(np.float32) if train_cfg else ec
    xn, lp0 = dd.step(ost, guided, ts, x, noise=z, eta=1.0)
    old = (lp0 + np.resize(np.asarray(OFF8, dtype=np.float32), B)).astype(np.float32)
    adv = np.resize(np.asarray(ADV8, dtype=np.float32), B)
    return ec, eu, x, z, xn, ts, old, adv


@functools.lru_cache(maxsize=4)
def _ppo_reference(pred, train_cfg, B, group, chw):
    """float64 autograd of the sum of the per-micro-batch losses (tests/test_fused_micro_steps.py::
    test_oracle_grouped_loss_is_sum_of_micro_batch_losses): log-probs, ratios, info rows (approx_kl, clipfrac, loss), d_eps_c, d_eps_u."""
    dd, ost = _oracle_sched(pred)
    ec, eu, x, z, xn, ts, old, adv = _ppo_inputs(pred, train_cfg, B, chw)
    tec = torch.from_numpy(ec).double().requires_grad_(True)
    teu = torch.from_numpy(eu).double().requires_grad_(True)
    total, lps, infos = 0.0, [], []
    for j in range(B // group):
        sl = slice(j * group, (j + 1) * group)
        batch = {"ts": ts[sl], "latents": torch.from_numpy(x[sl]), "next_latents": torch.from_numpy(xn[sl]),
                 "advantages": torch.from_numpy(adv[sl]), "log_probs": torch.from_numpy(old[sl])}
        loss, info, lp = OPPO.loss_and_info_torch(dd, ost, tec[sl], teu[sl], batch, GUIDE, 1.0, CLIP, train_cfg, dtype=torch.float64)
        total = total + loss
        lps.append(lp.detach().numpy())
        infos.append([float(info["approx_kl"].detach()), float(info["clipfrac"]), float(info["loss"].detach())])
    total.backward()
    lp = np.concatenate(lps)
    return lp, np.exp(lp - old.astype(np.float64)), np.asarray(infos), tec.grad.numpy(), teu.grad.numpy() if train_cfg else None


def _closed_form(pred, train_cfg, B, group, chw):
    """The fp32 closed form per micro-batch (what `B // group` separate launches compute)."""
    dd, ost = _oracle_sched(pred)
    ec, eu, x, z, xn, ts, old, adv = _ppo_inputs(pred, train_cfg, B, chw)
    lps, infos, dcs, dus = [], [], [], []
    for j in range(B // group):
        sl = slice(j * group, (j + 1) * group)
        loss, info, lp, dc, du = OPPO.closed_form_numpy(dd, ost, ec[sl], eu[sl], x[sl], xn[sl], ts[sl], old[sl], adv[sl], GUIDE, 1.0, CLIP, train_cfg)
        lps.append(lp); dcs.append(dc); dus.append(du)
        infos.append([float(info["approx_kl"]), float(info["clipfrac"]), float(info["loss"])])
    return np.concatenate(lps), np.asarray(infos), np.concatenate(dcs), np.concatenate(dus)


def _ppo_errors(ref, group, train_cfg, lp, infos, d_c, d_u):
    """(log-prob abs error, gradient error / max|grad_ref|, loss relative error) of one result against the float64 reference; asserts the exact
    clipfrac and today's approx_kl tolerance on the way."""
    rlp, _, rinfo, rdc, rdu = ref
    e_lp = float(np.abs(np.asarray(lp, dtype=np.float64) - rlp).max())
    e_g = float(np.abs(np.asarray(d_c, dtype=np.float64) - rdc).max() / np.abs(rdc).max())
    if train_cfg:
        e_g = max(e_g, float(np.abs(np.asarray(d_u, dtype=np.float64) - rdu).max() / np.abs(rdu).max()))
    infos = np.asarray(infos, dtype=np.float64).reshape(-1, 3)
    e_loss = float((np.abs(infos[:, 2] - rinfo[:, 2]) / np.abs(rinfo[:, 2])).max())
    assert np.array_equal(np.rint(infos[:, 1] * group).astype(np.int64), np.rint(rinfo[:, 1] * group).astype(np.int64))      # clipfrac: exact
    np.testing.assert_allclose(infos[:, 0], rinfo[:, 0], rtol=1e-2, atol=1e-9)                                              # approx_kl
    return e_lp, e_g, e_loss


def _ppo_device_call(pred, train_cfg, B, group, chw):
    ec, eu, x, z, xn, ts, old, adv = _ppo_inputs(pred, train_cfg, B, chw)
    t = lambda a: torch.from_numpy(a).to(DEV)
    return L.ddim_logprob_ppo_fwd_bwd(t(ec), t(eu) if train_cfg else None, t(x), t(xn), t(ts), t(old), t(adv), GUIDE, CLIP, train_cfg,
                                      _device_consts(pred), group=group)


@gpu
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("train_cfg", [True, False])
@pytest.mark.parametrize("B,group,chw,branch", PPO_CHW_TABLE + PPO_B_TABLE)
def test_ppo_dispatch_branch_matches_float64(pred, train_cfg, B, group, chw, branch):
    ref = _ppo_reference(pred, train_cfg, B, group, chw)
    # the inputs put every float64 ratio well away from either clip bound: no fp32-vs-float64 flip of a clip decision is possible
    margin = float(np.minimum(np.abs(ref[1] - (1.0 - CLIP)), np.abs(ref[1] - (1.0 + CLIP))).min())
    assert margin > 6.5e-5, margin
    assert np.abs(ref[3]).max() > 0
    # the fp32 closed form sits inside a quarter of each bound
    clp, cinfo, cdc, cdu = _closed_form(pred, train_cfg, B, group, chw)
    c_lp, c_g, c_loss = _ppo_errors(ref, group, train_cfg, clp, cinfo, cdc, cdu)
    assert c_lp < LP_ATOL / 4 and c_g < GRAD_REL / 4 and c_loss < LOSS_REL / 4, (c_lp, c_g, c_loss)
    # the kernel
    d_c, d_u, per, info = _ppo_device_call(pred, train_cfg, B, group, chw)
    assert info.shape == (B // group, 3) and (d_u is None) == (not train_cfg)
    per = per.cpu().numpy()
    k_lp, k_g, k_loss = _ppo_errors(ref, group, train_cfg, per[:, 0], info.cpu().numpy(), d_c.cpu().numpy(),
                                    d_u.cpu().numpy() if train_cfg else None)
    _record(f"ppo {pred} train_cfg={int(train_cfg)} B={B} group={group} chw={chw} ({branch}): log-prob abs {k_lp:.2e} (bound {LP_ATOL:.1e}, "
            f"closed form {c_lp:.2e}); grad/max|grad| {k_g:.2e} (bound {GRAD_REL:.0e}, closed form {c_g:.2e}); loss rel {k_loss:.2e} "
            f"(bound {LOSS_REL:.0e}, closed form {c_loss:.2e})")
    assert k_lp < LP_ATOL, k_lp
    assert k_g < GRAD_REL, k_g
    assert k_loss < LOSS_REL, k_loss
    # per-sample columns: ratio, max(unclipped, clipped), clipped flag
    np.testing.assert_allclose(per[:, 1], ref[1], rtol=0, atol=LP_ATOL + 4 * 2.0 ** -23)        # exp of a log-prob difference within LP_ATOL, a few ulp of 1
    assert np.array_equal(per[:, 3] != 0, np.abs(ref[1] - 1.0) > CLIP)


def _step_inputs_dev(pred, train_cfg, chw, B=4):
    ec, eu, x, z, xn, ts, old, adv = _ppo_inputs(pred, train_cfg, B, chw)
    t = lambda a: torch.from_numpy(a).to(DEV)
    return t(ec), t(eu), t(x), t(z), t(ts), t(adv)


@gpu
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("train_cfg", [True, False])
@pytest.mark.parametrize("chw", [r[2] for r in PPO_CHW_TABLE])
def test_ppo_scores_the_step_kernels_own_sample_with_ratio_one(pred, train_cfg, chw):
    """Bit contract (a) of the comment above ppo_cluster_kernel: a transition sampled by ddim_step_kernel and scored before the first update has
    the sampler's log-prob bit for bit, on every rung and on the fall-back: the ratio is exactly 1."""
    ec, eu, x, z, ts, adv = _step_inputs_dev(pred, train_cfg, chw)
    consts = _device_consts(pred)
    xn, logp = L.ddim_step_fwd(eu if train_cfg else ec, ec, x, z, ts, GUIDE, consts)
    d_c, d_u, per, info = L.ddim_logprob_ppo_fwd_bwd(ec, eu if train_cfg else None, x, xn, ts, logp, adv, GUIDE, CLIP, train_cfg, consts)
    assert torch.equal(per[:, 0], logp)
    assert torch.equal(per[:, 1], torch.ones_like(logp))
    assert float(per[:, 3].abs().max()) == 0.0 and float(info[1]) == 0.0 and float(info[0]) == 0.0


@gpu
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("train_cfg", [True, False])
@pytest.mark.parametrize("chw", PPO_BIT_CHW)
def test_ppo_cluster_and_fallback_kernels_agree_bitwise(pred, train_cfg, chw):
    """Bit contract (b): five rows as B = 5, group 5 (cluster kernel) and tiled 13 times as B = 65, group 5 (fall-back kernels) give the same
    per-sample rows and info rows, and the same gradients: the two kernels spell the same expressions."""
    ec, eu, x, z, xn, ts, old, adv = (torch.from_numpy(a).to(DEV) for a in _ppo_inputs(pred, train_cfg, 5, chw))
    consts = _device_consts(pred)
    dc5, du5, per5, info5 = L.ddim_logprob_ppo_fwd_bwd(ec, eu if train_cfg else None, x, xn, ts, old, adv, GUIDE, CLIP, train_cfg, consts, group=5)
    tile = lambda a: a.repeat(13, *([1] * (a.dim() - 1))).contiguous()
    dc65, du65, per65, info65 = L.ddim_logprob_ppo_fwd_bwd(tile(ec), tile(eu) if train_cfg else None, tile(x), tile(xn), tile(ts), tile(old),
                                                           tile(adv), GUIDE, CLIP, train_cfg, consts, group=5)
    assert info5.shape == (1, 3) and info65.shape == (13, 3)
    assert torch.equal(per65, tile(per5))
    assert torch.equal(info65, info5.expand(13, 3))
    assert float(dc5.abs().max()) > 0
    ulp = _ulp_dist(dc65, tile(dc5))
    if train_cfg:
        ulp = max(ulp, _ulp_dist(du65, tile(du5)))
    _record(f"ppo cluster vs fallback {pred} train_cfg={int(train_cfg)} chw={chw}: gradients differ by at most {ulp} fp32 ulp")
    assert torch.equal(dc65, tile(dc5))
    if train_cfg:
        assert torch.equal(du65, tile(du5))


def _ddim_step_float64(pred, guided, ts, x, z):
    """scheduling_ddim_flax.py:279-359 in sampling mode on float64 (per-sample coefficients as the fp32 schedule gives them)."""
    dd, ost = _oracle_sched(pred)
    a_t, a_p, b_t, std = (np.asarray(v, dtype=np.float64).reshape(-1, 1, 1, 1) for v in dd.coefficients(ost, ts, 1.0))
    if pred == "epsilon":
        x0, e = (x - np.sqrt(b_t) * guided) / np.sqrt(a_t), guided
    else:
        x0, e = np.sqrt(a_t) * x - np.sqrt(b_t) * guided, np.sqrt(a_t) * guided + np.sqrt(b_t) * x
    mean = np.sqrt(a_p) * x0 + np.sqrt(1.0 - a_p - std ** 2) * e
    xn = mean + std * z
    std_c = np.maximum(std, 1e-6)
    lp = -((xn - mean) ** 2) / (2.0 * std_c ** 2) - np.log(std_c) - math.log(math.sqrt(2.0 * math.pi))
    return xn, lp.reshape(x.shape[0], -1).mean(1)


@gpu
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("chw", PPO_STEP_CHW)
def test_ddim_step_loop_tails_match_float64(pred, chw):
    """(c) ddim_step_kernel alone against the float64 DDIM step."""
    ec, eu, x, z, _, ts, _, _ = _ppo_inputs(pred, True, 4, chw)
    t = lambda a: torch.from_numpy(a).to(DEV)
    xn, logp = L.ddim_step_fwd(t(eu), t(ec), t(x), t(z), t(ts), GUIDE, _device_consts(pred))
    e64, c64 = eu.astype(np.float64), ec.astype(np.float64)
    rxn, rlp = _ddim_step_float64(pred, e64 + GUIDE * (c64 - e64), ts, x.astype(np.float64), z.astype(np.float64))
    e_x, e_lp = _rel(xn, rxn), float(np.abs(logp.cpu().numpy().astype(np.float64) - rlp).max())
    _record(f"ddim_step {pred} chw={chw}: x_next rel-to-max {e_x:.2e} (bound 1e-5); log-prob abs {e_lp:.2e} (bound {LP_ATOL:.1e})")
    assert e_x < 1e-5
    assert e_lp < LP_ATOL


@gpu
def test_ppo_counters_rearm_across_launches_of_different_geometry():
    """g_ppo_cnt / g_ppo_done / g_ppo_grp are device globals that the last reader of a launch re-arms: launches of different (B, group, chw),
    cluster and fall-back mixed, queued back to back on one stream with nothing waiting in between, repeat bit for bit and equal the same call
    made on its own."""
    consts = _device_consts("epsilon")
    calls = []
    for i, (B, group, chw) in enumerate(PPO_REARM):
        train_cfg = i % 2 == 0
        ec, eu, x, z, xn, ts, old, adv = (torch.from_numpy(a).to(DEV) for a in _ppo_inputs("epsilon", train_cfg, B, chw))
        calls.append(((ec, eu if train_cfg else None, x, xn, ts, old, adv, GUIDE, CLIP, train_cfg, consts), group))
    torch.cuda.synchronize()
    passes = [[L.ddim_logprob_ppo_fwd_bwd(*a, group=g) for a, g in calls] for _ in range(2)]        # 12 launches, no synchronisation
    torch.cuda.synchronize()
    same = lambda p, q: all((u is None and v is None) or torch.equal(u, v) for u, v in zip(p, q))
    for first, second in zip(*passes):
        assert same(first, second)
    for (a, g), first in zip(calls, passes[0]):
        alone = L.ddim_logprob_ppo_fwd_bwd(*a, group=g)
        torch.cuda.synchronize()
        assert same(first, alone)
        assert bool(torch.isfinite(first[3]).all()) and float(first[0].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 2. optimizer
@gpu
@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("n", SQNORM_N)
def test_grad_sqnorm_tail_and_grid_stride(n, offset):
    """Bound: each fp32 lane partial carries at most 4 roundings of 2^-24 at these sizes before it is widened to double -> relative 1e-6 with room.
    offset 4: the buffer is a 16-byte aligned slice at a non-zero offset of a larger allocation (its neighbours must not be summed)."""
    g = torch.Generator().manual_seed(n)
    big = torch.randn(n + 8, generator=g) * 3
    dev = big.to(DEV)[offset:offset + n]
    assert dev.data_ptr() % 16 == 0
    out = torch.full((1,), 123.0, dtype=torch.float64, device=DEV)          # the entry zeroes it first
    sq = L.grad_sqnorm(dev, out)
    want = float(np.sum(big[offset:offset + n].numpy().astype(np.float64) ** 2))
    assert float(sq.item()) == pytest.approx(want, rel=1e-6)


def _bf16_words(t):
    if torch.is_tensor(t):
        return t.view(torch.int16).cpu().numpy()
    return (np.ascontiguousarray(t, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16).view(np.int16)


@gpu
@pytest.mark.parametrize("mu_bf16", [True, False])
@pytest.mark.parametrize("n", ADAMW_N)
def test_adamw_tail_and_grid_stride(n, mu_bf16):
    """Three steps as in test_gpu_kernels.py::test_adamw_matches_oracle (the first clips, the second does not), the last with zero_grad=False.
    The n % 4 tail and the final grid-stride iteration are asserted on their own."""
    rng = np.random.default_rng(3 + n)
    p0 = rng.standard_normal(n).astype(np.float32)
    opt = AdamWBf16Mu(mu_decay_in_bf16=mu_bf16)
    ost = AccumulatingState([p0], opt)
    p = torch.from_numpy(p0.copy()).to(DEV)
    g = torch.zeros(n, device=DEV)
    mu = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    nu = torch.zeros(n, device=DEV)
    n4, stride = n >> 2, 4096 * 256
    parts = {"all": slice(0, n)}
    if n & 3:
        parts["n % 4 tail"] = slice(n4 * 4, n)
    if n4 > stride:
        parts["final grid-stride iteration"] = slice(((n4 - 1) // stride) * stride * 4, n4 * 4)
    for step in range(1, 4):
        # the first step has to clip and the second must not, whatever n is: a handful of elements gets a larger first gradient, millions a smaller second
        scale = [3.0 if n > 100 else 30.0, 1e-3 if n < 1000000 else 2e-4, 0.5][step - 1]
        g1 = (rng.standard_normal(n) * scale).astype(np.float32)
        g2 = (rng.standard_normal(n) * scale).astype(np.float32)
        ost.apply_gradients([g1], False)
        ost.apply_gradients([g2], True)
        g += torch.from_numpy(g1).to(DEV)
        g += torch.from_numpy(g2).to(DEV)
        sq = L.grad_sqnorm(g)
        norm = math.sqrt(float(sq.item())) * 0.5
        assert norm == pytest.approx(float(ost.last_grad_norm), rel=1e-5)
        assert norm > 1.5 if step == 1 else norm < 0.5 if step == 2 else True, (step, norm)      # clipped, not clipped, either
        g_before = g.clone()
        L.adamw_bf16mu_step(p, g, mu, nu, sq, 0.5, 1e-5, 0.9, 0.999, 1e-8, 1e-4, 1.0, step, mu_decay_in_bf16=mu_bf16, zero_grad=step < 3)
        if step < 3:
            assert float(g.abs().max()) == 0.0 and not bool(torch.isnan(g).any())      # the tail elements included
        else:
            assert torch.equal(g, g_before)                                             # zero_grad=False leaves g alone
        pk, nuk = p.cpu().numpy(), nu.cpu().numpy()
        muk, muo = mu.float().cpu().numpy(), ost.opt_state["mu"][0]
        dmu = np.abs(_ordered(_bf16_words(mu), 16) - _ordered(_bf16_words(ost.opt_state["mu"][0]), 16))
        for name, sl in parts.items():
            assert pk[sl].size > 0
            np.testing.assert_allclose(pk[sl], ost.params[0][sl], rtol=1e-6, atol=1e-7, err_msg=f"p, {name}, step {step}")
            np.testing.assert_allclose(nuk[sl], ost.opt_state["nu"][0][sl], rtol=1e-5, atol=1e-12, err_msg=f"nu, {name}, step {step}")
            if n < 100000:
                assert int(dmu[sl].max()) <= 1, (name, step)           # bf16 first moment: identical except 1-ulp rounding ties
            else:
                # a tie of an earlier step moves the decayed term by one bf16 ulp OF THE OLD moment, which is several ulp of a new moment that
                # the gradient term nearly cancels: on a part, hold the values to one bf16 ulp (2^-8) of the moments' size, elementwise
                np.testing.assert_allclose(muk[sl], muo[sl], rtol=2.0 ** -7, atol=2.0 ** -8 * float(np.abs(muo).max()), err_msg=f"mu, {name}, step {step}")
        if n >= 100000:
            assert float((dmu != 0).mean()) < 1e-3                     # a condition, not a measurement


# ------------------------------------------------------------------------------------------------ 3. small kernels
@gpu
@pytest.mark.parametrize("n", QUICK_GELU_N)
def test_quick_gelu_tail_and_grid_stride(n):
    g = torch.Generator().manual_seed(n)
    x = (torch.rand(n, generator=g) * 24 - 12)
    x[0] = 12.0 if n > 1 else -3.0
    x[-1] = -12.0 if n > 1 else x[-1]
    y = L.quick_gelu(x.to(DEV)).cpu().double()
    ref = x.double() * torch.sigmoid(1.702 * x.double())
    assert _rel(y, ref) < 2e-6                      # __expf: relative to max|y|
    small = ref.abs() < 1e-3
    if bool(small.any()):
        assert float((y - ref)[small].abs().max()) < 2e-6
    xin = x.to(DEV)
    assert torch.equal(L.quick_gelu(xin, out=xin).cpu().double(), y)      # in place


@gpu
@pytest.mark.parametrize("rows,cols", L2_SHAPES)
def test_l2_normalize_rows_shapes(rows, cols):
    g = torch.Generator().manual_seed(rows * 1000 + cols)
    x = torch.randn(rows, cols, generator=g) * 3
    y = L.l2_normalize_rows(x.to(DEV)).cpu().double()
    ref = x.double() / x.double().norm(dim=1, keepdim=True)
    assert _rel(y, ref) < 1e-5
    assert float((y.norm(dim=1) - 1.0).abs().max()) < 1e-6


@gpu
@pytest.mark.parametrize("with_row", [True, False])
@pytest.mark.parametrize("with_ts", [True, False])
@pytest.mark.parametrize("n,row_n,ts_n", STAGE_CASES)
def test_stage_cfg_inputs_copies_exactly_and_nothing_else(n, row_n, ts_n, with_row, with_ts):
    G = 64                                           # guard band (elements) on both sides of every destination
    gen = torch.Generator(device=DEV).manual_seed(n)
    x = torch.randn(n, generator=gen, device=DEV)
    s_all = torch.full((2 * n + 2 * G,), -7.25, device=DEV)
    s_in = s_all[G:G + 2 * n]
    row_src = torch.randn(row_n, generator=gen, device=DEV)
    row_all = torch.full((row_n + 2 * G,), -7.25, device=DEV)
    ts_src = torch.randint(0, 1000, (ts_n,), generator=gen, device=DEV, dtype=torch.int32)
    ts_all = torch.full((ts_n + 2 * G,), -77, device=DEV, dtype=torch.int32)
    L.stage_cfg_inputs(x, s_in, row_src if with_row else None, row_all[G:G + row_n] if with_row else None,
                       ts_src if with_ts else None, ts_all[G:G + ts_n] if with_ts else None)
    assert torch.equal(s_in[:n], x) and torch.equal(s_in[n:], x)
    assert bool((s_all[:G] == -7.25).all()) and bool((s_all[G + 2 * n:] == -7.25).all())
    if with_row:
        assert torch.equal(row_all[G:G + row_n], row_src)
        assert bool((row_all[:G] == -7.25).all()) and bool((row_all[G + row_n:] == -7.25).all())
    else:
        assert bool((row_all == -7.25).all())
    if with_ts:
        assert torch.equal(ts_all[G:G + ts_n], ts_src)
        assert bool((ts_all[:G] == -77).all()) and bool((ts_all[G + ts_n:] == -77).all())
    else:
        assert bool((ts_all == -77).all())


@gpu
@pytest.mark.parametrize("scale", [0.7, -1.3])
@pytest.mark.parametrize("rows,cols", SOFTMAX_SHAPES)
def test_softmax_rows_loops(rows, cols, scale):
    g = torch.Generator().manual_seed(rows + cols)
    s = torch.randn(rows, cols, generator=g) * 3
    sm = L.softmax_rows_(s.clone().to(DEV), scale).cpu().double()
    assert _rel(sm, torch.softmax(s.double() * scale, -1)) < 1e-5
    assert float((sm.sum(-1) - 1.0).abs().max()) < 1e-6


@gpu
@pytest.mark.parametrize("scale", [0.7, -1.3])
def test_softmax_rows_large_logits_in_one_row(scale):
    """One row of logits of magnitude 80 among ordinary ones: the row maximum keeps it finite (not an overflow hunt)."""
    g = torch.Generator().manual_seed(80)
    s = torch.randn(5, 257, generator=g) * 3
    s[2] = (torch.rand(257, generator=g) * 2 - 1) * 80
    s[2, 100], s[2, 256] = 80.0, -80.0
    sm = L.softmax_rows_(s.clone().to(DEV), scale).cpu().double()
    assert bool(torch.isfinite(sm).all())
    assert _rel(sm, torch.softmax(s.double() * scale, -1)) < 1e-5
    assert float((sm.sum(-1) - 1.0).abs().max()) < 1e-6


@gpu
@pytest.mark.parametrize("cols", COLSUM_COLS)
@pytest.mark.parametrize("rows_per_seg", COLSUM_ROWS_PER_SEG)
def test_colsum_accum_chunks_strided_rows_and_accumulation(rows_per_seg, cols):
    """Three segments; x is a column slice (row stride cols + 8) of a wider matrix; out holds values on entry and the kernel adds to them.
    lib.colsum_accum takes the pointer of a CONTIGUOUS x whatever ld_x says (it refuses the slice: tests/golden/lib_launch_records.json pins that
    refusal for gemm_wgrad's bias-gradient call), so the strided operand goes to the C entry point itself."""
    g = torch.Generator().manual_seed(rows_per_seg * 100 + cols)
    rows = 3 * rows_per_seg
    wide = torch.randn(rows, cols + 8, generator=g)
    out0 = torch.randn(3, cols, generator=g)
    wide_dev = wide.to(DEV)
    x = wide_dev[:, 4:4 + cols]
    assert x.data_ptr() % 16 == 0 and x.stride() == (cols + 8, 1)

    def colsum(out, rps):
        L._check(L.load().ddpo_colsum_accum(L._p_rows(x), cols + 8, rows, cols, rps, L._p(out), L._stream()), "ddpo_colsum_accum")
        return out

    ref = wide[:, 4:4 + cols].double().view(3, rows_per_seg, cols).sum(1)
    assert _rel(colsum(out0.clone().to(DEV), rows_per_seg), out0.double() + ref) < 1e-5
    assert _rel(colsum(out0[0].clone().to(DEV), 0), out0[0].double() + ref.sum(0)) < 1e-5         # rows_per_seg = 0: all rows are one segment
    # and through the wrapper on the contiguous copy (ld_x = cols)
    assert _rel(L.colsum_accum(x.contiguous(), out0.clone().to(DEV), rows_per_seg=rows_per_seg), out0.double() + ref) < 1e-5


def _randn_dev(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV) * scale


def _geglu_ref(x, F):
    return x[:, :F] * torch.nn.functional.gelu(x[:, F:], approximate="tanh")


# The float64 references of the cases past a block cap are evaluated by torch on the device (tens of millions of elements), the minimal ones on the host.
@gpu
@pytest.mark.parametrize("rows", [1, STREAM_CAPS["geglu"] * 256 + 77])
def test_geglu_fwd_bwd_grid_stride(rows):
    F = 4
    x, dy = _randn_dev(rows, rows, 2 * F, scale=2.0), _randn_dev(rows + 1, rows, F)
    xd = x.double().requires_grad_(True)
    ref = _geglu_ref(xd, F)
    ref.backward(dy.double())
    assert _rel(L.geglu(x), ref) < 1e-5
    assert _rel(L.geglu_bwd(x, dy), xd.grad) < 1e-5


@gpu
@pytest.mark.parametrize("n", [1, STREAM_CAPS["silu"] * 256 + 77])
def test_silu_fwd_bwd_grid_stride(n):
    x, dy = _randn_dev(n, n, scale=3.0), _randn_dev(n + 1, n)
    xd = x.double().requires_grad_(True)
    ref = torch.nn.functional.silu(xd)
    ref.backward(dy.double())
    assert _rel(L.silu(x), ref) < 1e-5
    assert _rel(L.silu_bwd(x, dy), xd.grad) < 1e-5


@gpu
@pytest.mark.parametrize("n", [1, STREAM_CAPS["add"] * 256 + 77])
def test_add_and_scale_shift_clip_grid_stride(n):
    a, b = _randn_dev(n, n), _randn_dev(n + 1, n)
    assert torch.equal(L.add(a, b).cpu().double(), (a.double() + b.double()).float().cpu().double())     # one rounding of the exact sum
    c = L.scale_shift_clip(a, 0.5, 0.5, 0.0, 1.0)                                                       # n > 4096 * 256 + 77 as well
    assert _rel(c, (a.double() * 0.5 + 0.5).clamp(0.0, 1.0)) < 1e-5
    assert float(c.min()) >= 0.0 and float(c.max()) <= 1.0


@gpu
@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (3, 1183, 1183)])       # 3 * 1183 * 1183 = 16384 * 256 + 4163 float4 outputs (C = 4)
def test_sumpool2x2_grid_stride(B, H, W):
    C = 4
    assert B * H * W == 1 or B * H * W > STREAM_CAPS["sumpool2x2"] * 256 and (B * H * W) % 2 == 1
    u = _randn_dev(B * H * W, B * 2 * H * 2 * W, C)
    sp = L.sumpool2x2(u, B, H, W, C)
    ref = u.view(B, H, 2, W, 2, C).double().sum((2, 4)).reshape(B * H * W, C)
    assert _rel(sp, ref) < 1e-5


@gpu
@pytest.mark.parametrize("rows", [1, STREAM_CAPS["copy_cols"] * 256 + 77])
def test_copy_cols_grid_stride(rows):
    cols = 4
    src = _randn_dev(rows, rows, 8)                                  # ld_src = 8: only the first four columns are copied
    dst = torch.full((rows, 12), -7.25, device=DEV)
    L.copy_cols(src, dst, 4, rows, cols)
    assert torch.equal(dst[:, 4:8], src[:, :4])
    assert bool((dst[:, :4] == -7.25).all()) and bool((dst[:, 8:] == -7.25).all())


@gpu
@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (3, 1, 349551)])         # 3 * 349551 = 4096 * 256 + 77 pixels
def test_layout_pair_grid_stride(B, H, W):
    C = 3
    assert B * H * W == 1 or B * H * W == STREAM_CAPS["layout"] * 256 + 77
    a = _randn_dev(W, B, C, H, W)
    nhwc = L.nchw_to_nhwc(a)
    assert torch.equal(nhwc.view(B, H, W, C), a.permute(0, 2, 3, 1))
    assert torch.equal(L.nhwc_to_nchw(nhwc, B, C, H, W), a)


@gpu
@pytest.mark.parametrize("train_cfg", [True, False])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("chw", RWR_CHW)
def test_rwr_mse_loop_tails_match_float64(chw, weighted, train_cfg):
    B, g_scale = 5, 3.0
    g = torch.Generator().manual_seed(chw + int(train_cfg) + 2 * int(weighted))
    ec, eu, noise = (torch.randn(B, 4, chw // 4, 1, generator=g) for _ in range(3))
    w = torch.softmax(torch.randn(B, generator=g), 0) if weighted else None
    ecd = ec.double().requires_grad_(True)
    eud = eu.double().requires_grad_(True)
    loss_ref, per_ref = OD.loss_torch(ecd, eud if train_cfg else None, noise.double(), None if w is None else w.double(), g_scale, train_cfg)
    loss_ref.backward()
    d_c, d_u, per, loss = L.rwr_mse_fwd_bwd(ec.to(DEV), eu.to(DEV) if train_cfg else None, noise.to(DEV), None if w is None else w.to(DEV),
                                           g_scale, train_cfg)
    assert float(loss[0]) == pytest.approx(float(loss_ref.detach()), rel=2e-6)
    assert _rel(per[:, 0], per_ref.detach()) < 2e-6
    assert _rel(d_c, ecd.grad) < 2e-6
    if train_cfg:
        assert _rel(d_u, eud.grad) < 2e-6
    else:
        assert d_u is None


@gpu
@pytest.mark.parametrize("B,dim", TEMB_CASES)
def test_timestep_embedding_shapes(B, dim):
    ts = torch.as_tensor(np.resize(np.asarray([981, 1, 500, 21, 961], dtype=np.int32), B))
    emb = L.timestep_embedding(ts.to(DEV), dim).cpu().numpy()
    half = dim // 2
    arg = ts.double().numpy()[:, None] * np.exp(-math.log(10000.0) * np.arange(half, dtype=np.float64) / half)[None, :]
    np.testing.assert_allclose(emb, np.concatenate([np.cos(arg), np.sin(arg)], axis=-1), rtol=0, atol=2e-4)
