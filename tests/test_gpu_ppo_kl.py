"""ddpo_ddim_kl_ref_fwd_bwd (ddpo_amd/csrc/ppo_kl.hip), the additive KL pass behind the PPO launch, at the kernel level: against the float64
oracle of tests/_kl_oracle.py on every pass count of its 1024-thread float4 loop and on one, two and thirteen micro-batches, its exactness
contracts (a reference equal to the policy changes nothing, bit for bit; run-to-run and grouped-vs-separate bit equality) and every
DDPO_EINVAL case of include/ddpo_ppo_kl.h.

Shapes: chw = 4 is one float4, 4100 a second pass holding one float4, 65540 a 17th pass (the ladder of RWR_CHW in test_gpu_kernel_branches.py);
(B, group) = (4, 4) one micro-batch, (6, 3) two, (65, 5) thirteen on more rows than the PPO launch's cluster form takes (B > 64: its
fall-back kernels pre-fill the gradient).  The timesteps cycle through TS8, so t = 1 (sigma = 0.02) and t = 981 are always present.  A group
of 65 rows, one more than the info kernel's wave covers in one pass of its stride loop, is checked on its own.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from ddpo_amd import lib as L
from oracle import ppo as OPPO
from oracle.ddim import DDIMOracle

import _kl_oracle as KO

gpu = pytest.mark.gpu
DEV = "cuda"

KL_CHW = [4, 4100, 65540]
KL_BG = [(4, 4), (6, 3), (65, 5)]
# the per-row tables of tests/test_gpu_kernel_branches.py (timesteps, old log-prob offsets around clip_range = 1e-4, advantages)
TS8 = [981, 1, 481, 21, 961, 501, 41, 241]
OFF8 = [3e-5, 3e-4, -3e-4, -3e-4, -3e-5, 3e-4, 3e-4, -3e-5]
ADV8 = [8.0, 12.0, -20.0, 6.0, 5.0, 7.0, -3.0, 14.0]
GUIDE, CLIP = 5.0, 1e-4
REF_NOISE = 1e-2                    # r = e + 1e-2 N(0, 1)
# kl_coef by train_cfg.  The PPO gradient of these rows is large (advantages of 5 .. 10 over sigma = 0.02 at t = 1) and the guided difference
# is (1 + 2 g (g - 1))^0.5 = 6.4 times the unguided one, so the coefficients are large and differ: with them the penalty's part of d_eps_c is
# 0.3 .. 2 times the PPO part in max norm in every case (asserted), i.e. neither summand of the final gradient hides behind the other.
KL_COEF = {True: 15.0, False: 100.0}

# Bounds (the house rule of tests/test_gpu_kernel_branches.py:95-98): 8 x the worst error, over all 36 cases below and on these very inputs, of
# the fp32 numpy restatement of the closed form (oracle.ppo.closed_form_numpy + _kl_oracle.closed_form_numpy, summed in fp32) against float64
# autograd, computed on the host: kl_b 1.81e-6 relative per row (c_t is a difference of two fp32 products that cancels a digit, and it enters
# squared; already 1.5e-6 at chw = 4), kl_info 6.0e-7 relative per micro-batch, penalised loss 1.96e-6 relative per micro-batch, final
# gradient 7.2e-6 of max|grad| (the PPO closed form alone: 5.9e-6, test_gpu_kernel_branches.py).  The restatement has to sit inside a
# quarter of each bound, so the margin stays honest when the inputs change.
KL_REL, KLINFO_REL, LOSS_REL, GRAD_REL = 1.45e-5, 4.8e-6, 1.57e-5, 5.7e-5


def _record(line):
    from conftest import parity_record
    parity_record("[ppo kl] " + line)


@functools.lru_cache(maxsize=None)
def _oracle_sched(pred):
    dd = DDIMOracle(prediction_type=pred)
    return dd, dd.set_timesteps(dd.create_state(), 50)


@functools.lru_cache(maxsize=None)
def _device_consts(pred, eta=1.0):
    from ddpo_amd.diffusers_patch.scheduling_ddim import DDIMScheduler
    s = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", set_alpha_to_one=False, steps_offset=1,
                      prediction_type=pred)
    return s.kernel_consts(s.set_timesteps(s.create_state(device=DEV), 50), eta)


@functools.lru_cache(maxsize=4)
def _inputs(pred, train_cfg, B, chw):
    """fp32 numpy, shape (B, 4, chw / 4, 1): eps_c, eps_u, ref_c, ref_u, x, x_next (the oracle's DDIM step from the guided prediction), ts,
    old log-probs, advantages."""
    dd, ost = _oracle_sched(pred)
    rng = np.random.default_rng(chw * 131 + B * 7 + 3 * (pred == "v_prediction") + int(train_cfg) + 17)
    shp = (B, 4, chw // 4, 1)
    ec, eu, x, z = (rng.standard_normal(shp, dtype=np.float32) for _ in range(4))
    rc = (ec + np.float32(REF_NOISE) * rng.standard_normal(shp, dtype=np.float32)).astype(np.float32)
    ru = (eu + np.float32(REF_NOISE) * rng.standard_normal(shp, dtype=np.float32)).astype(np.float32)
    ts = np.resize(np.asarray(TS8, dtype=np.int32), B)
    guided = (eu + np.float32(GUIDE) * (ec - eu)).astype(np.float32) if train_cfg else ec
    xn, lp0 = dd.step(ost, guided, ts, x, noise=z, eta=1.0)
    old = (lp0 + np.resize(np.asarray(OFF8, dtype=np.float32), B)).astype(np.float32)
    adv = np.resize(np.asarray(ADV8, dtype=np.float32), B)
    return ec, eu, rc, ru, x, xn, ts, old, adv


@functools.lru_cache(maxsize=2)
def _reference(pred, train_cfg, B, group, chw):
    """float64 autograd of sum_j (ppo_j + KL_COEF * kl_j): kl_b, kl_info, penalised loss per micro-batch, d_eps_c, d_eps_u, the ratios, and the
    max norms of the PPO and the KL part of d_eps_c."""
    dd, ost = _oracle_sched(pred)
    ec, eu, rc, ru, x, xn, ts, old, adv = _inputs(pred, train_cfg, B, chw)
    d = lambda a: torch.from_numpy(a).double()
    tec, teu = d(ec).requires_grad_(True), d(eu).requires_grad_(True)
    total, ppo_total, klb, kli, loss, lps = 0.0, 0.0, [], [], [], []
    for j in range(B // group):
        sl = slice(j * group, (j + 1) * group)
        batch = {"ts": ts[sl], "latents": d(x[sl]), "next_latents": d(xn[sl]), "advantages": d(adv[sl]), "log_probs": d(old[sl])}
        l, info, lp, kl_b, ppo = KO.loss_and_info_torch(dd, ost, tec[sl], teu[sl] if train_cfg else None, d(rc[sl]), d(ru[sl]) if train_cfg else None,
                                                        batch, GUIDE, 1.0, CLIP, KL_COEF[train_cfg], train_cfg)
        total, ppo_total = total + l, ppo_total + ppo
        klb.append(kl_b.detach().numpy()); kli.append(float(info["kl_ref"].detach())); loss.append(float(l.detach())); lps.append(lp.detach().numpy())
    g_ppo = torch.autograd.grad(ppo_total, tec, retain_graph=True)[0]
    total.backward()
    ratio = np.exp(np.concatenate(lps) - old.astype(np.float64))
    return (np.concatenate(klb), np.asarray(kli), np.asarray(loss), tec.grad.numpy(), teu.grad.numpy() if train_cfg else None, ratio,
            float(g_ppo.abs().max()), float((tec.grad - g_ppo).abs().max()))


def _restatement(pred, train_cfg, B, group, chw):
    """The fp32 closed forms, per micro-batch for the PPO part as B // group separate launches compute it, summed in fp32 like the pass does."""
    dd, ost = _oracle_sched(pred)
    ec, eu, rc, ru, x, xn, ts, old, adv = _inputs(pred, train_cfg, B, chw)
    F = np.float32
    loss, dcs, dus = [], [], []
    for j in range(B // group):
        sl = slice(j * group, (j + 1) * group)
        l, _, _, dc, du = OPPO.closed_form_numpy(dd, ost, ec[sl], eu[sl], x[sl], xn[sl], ts[sl], old[sl], adv[sl], GUIDE, 1.0, CLIP, train_cfg)
        loss.append(l); dcs.append(dc); dus.append(du)
    kb, ki, ic, iu = KO.closed_form_numpy(dd, ost, ec, eu, rc, ru, ts, GUIDE, 1.0, KL_COEF[train_cfg], group, train_cfg)
    loss = (np.asarray(loss, dtype=F) + F(KL_COEF[train_cfg]) * ki).astype(F)
    return kb, ki, loss, (np.concatenate(dcs) + ic).astype(F), ((np.concatenate(dus) + iu).astype(F) if train_cfg else None)


def _errors(ref, train_cfg, kb, ki, loss, dc, du):
    rkb, rki, rloss, rdc, rdu = ref[:5]
    f = lambda a: np.asarray(a, dtype=np.float64)
    e_kb = float((np.abs(f(kb) - rkb) / rkb).max())
    e_ki = float((np.abs(f(ki).reshape(-1) - rki) / rki).max())
    e_loss = float((np.abs(f(loss).reshape(-1) - rloss) / np.abs(rloss)).max())
    e_g = float(np.abs(f(dc) - rdc).max() / np.abs(rdc).max())
    if train_cfg:
        e_g = max(e_g, float(np.abs(f(du) - rdu).max() / np.abs(rdu).max()))
    return e_kb, e_ki, e_loss, e_g


def _device_call(pred, train_cfg, B, group, chw, kl_coef=None, ref_is_eps=False):
    """The PPO launch, then the KL pass on its outputs.  Returns (d_c, d_u, info, kl_b, kl_info) after the pass and clones of (d_c, d_u, info)
    from before it."""
    from ddpo_amd import lib_ppo_kl as LK
    ec, eu, rc, ru, x, xn, ts, old, adv = (torch.from_numpy(a).to(DEV) for a in _inputs(pred, train_cfg, B, chw))
    if not train_cfg:
        eu = ru = None
    if ref_is_eps:
        rc, ru = ec, eu
    consts = _device_consts(pred)
    kl_coef = KL_COEF[train_cfg] if kl_coef is None else kl_coef
    d_c, d_u, per, info = L.ddim_logprob_ppo_fwd_bwd(ec, eu, x, xn, ts, old, adv, GUIDE, CLIP, train_cfg, consts, group=group)
    before = (d_c.clone(), None if d_u is None else d_u.clone(), info.clone())
    kl_b, kl_info = LK.ddim_kl_ref_fwd_bwd(ec, eu, rc, ru, ts, GUIDE, kl_coef, train_cfg, consts, d_c, d_u, loss_info=info, group=group)
    return (d_c, d_u, info, kl_b, kl_info), before


def _bits(t):
    return t.contiguous().view(torch.int32)


@gpu
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("train_cfg", [True, False])
@pytest.mark.parametrize("B,group", KL_BG)
@pytest.mark.parametrize("chw", KL_CHW)
def test_kl_pass_matches_float64(pred, train_cfg, B, group, chw):
    ref = _reference(pred, train_cfg, B, group, chw)
    ratio, m_ppo, m_kl = ref[5:]
    # no fp32-vs-float64 flip of a clip decision: that would take a log-prob error of 2e-5, eight times what the PPO kernel is held to
    assert float(np.minimum(np.abs(ratio - (1.0 - CLIP)), np.abs(ratio - (1.0 + CLIP))).min()) > 2e-5
    assert m_ppo > 0 and 0.3 < m_kl / m_ppo < 2.0, (m_ppo, m_kl)         # both summands of the final gradient are really there
    c = _errors(ref, train_cfg, *_restatement(pred, train_cfg, B, group, chw))
    assert c[0] < KL_REL / 4 and c[1] < KLINFO_REL / 4 and c[2] < LOSS_REL / 4 and c[3] < GRAD_REL / 4, c
    (d_c, d_u, info, kl_b, kl_info), _ = _device_call(pred, train_cfg, B, group, chw)
    assert kl_b.shape == (B,) and kl_info.shape == (B // group,) and info.shape == (B // group, 3)
    k = _errors(ref, train_cfg, kl_b.cpu().numpy(), kl_info.cpu().numpy(), info[:, 2].cpu().numpy(), d_c.cpu().numpy(),
                d_u.cpu().numpy() if train_cfg else None)
    _record(f"{pred} train_cfg={int(train_cfg)} B={B} group={group} chw={chw}: kl_b rel {k[0]:.2e} (bound {KL_REL:.1e}, closed form {c[0]:.2e}); "
            f"kl_info rel {k[1]:.2e} (bound {KLINFO_REL:.1e}, closed form {c[1]:.2e}); loss rel {k[2]:.2e} (bound {LOSS_REL:.1e}, closed form "
            f"{c[2]:.2e}); grad/max|grad| {k[3]:.2e} (bound {GRAD_REL:.1e}, closed form {c[3]:.2e}); max|kl part| / max|ppo part| {m_kl / m_ppo:.2f}")
    assert k[0] < KL_REL, k[0]
    assert k[1] < KLINFO_REL, k[1]
    assert k[2] < LOSS_REL, k[2]
    assert k[3] < GRAD_REL, k[3]


@gpu
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("train_cfg", [True, False])
@pytest.mark.parametrize("B,group,chw", [(6, 3, 4), (6, 3, 4100), (65, 5, 4100), (4, 4, 65540)])
def test_reference_equal_to_the_policy_changes_nothing(pred, train_cfg, B, group, chw):
    """ref_* is eps_*: the differences are exactly 0, so kl is exactly 0.0 and the PPO gradient and info keep their bits (signed zeros included:
    rows 3 and 6 of the tables are clipped, their PPO gradient is +-0.0)."""
    (d_c, d_u, info, kl_b, kl_info), (d_c0, d_u0, info0) = _device_call(pred, train_cfg, B, group, chw, kl_coef=0.5, ref_is_eps=True)
    assert float(kl_b.abs().max()) == 0.0 and float(kl_info.abs().max()) == 0.0
    assert torch.equal(_bits(d_c), _bits(d_c0)) and torch.equal(_bits(info), _bits(info0))
    if train_cfg:
        assert torch.equal(_bits(d_u), _bits(d_u0))
    if chw > 4:
        assert bool((_bits(d_c0) == -2 ** 31).any())      # the inputs do hold a -0.0 that a plain `+= 0.0f` would have flipped


@gpu
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("train_cfg", [True, False])
@pytest.mark.parametrize("B,group,chw", [(6, 3, 4100), (65, 5, 4), (4, 4, 65540)])
def test_two_identical_calls_give_identical_bits(pred, train_cfg, B, group, chw):
    a, _ = _device_call(pred, train_cfg, B, group, chw)
    b, _ = _device_call(pred, train_cfg, B, group, chw)
    for u, v in zip(a, b):
        assert (u is None and v is None) or torch.equal(_bits(u), _bits(v))


@gpu
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("train_cfg", [True, False])
@pytest.mark.parametrize("k,b,chw", [(2, 3, 4100), (13, 5, 4), (3, 2, 65540)])
def test_grouped_call_equals_separate_calls_bitwise(pred, train_cfg, k, b, chw):
    """group = b over k concatenated micro-batches against k calls of one micro-batch each, from the same PPO gradient: kl_per_sample, the
    kl_info rows, the penalised loss rows and the gradients are the same bits."""
    from ddpo_amd import lib_ppo_kl as LK
    B = k * b
    (d_c, d_u, info, kl_b, kl_info), (d_c0, d_u0, info0) = _device_call(pred, train_cfg, B, b, chw)
    ec, eu, rc, ru, x, xn, ts, old, adv = (torch.from_numpy(a).to(DEV) for a in _inputs(pred, train_cfg, B, chw))
    consts = _device_consts(pred)
    for j in range(k):
        sl = slice(j * b, (j + 1) * b)
        c = lambda t: t[sl].contiguous().clone()
        dcj, duj, infoj = c(d_c0), (c(d_u0) if train_cfg else None), info0[j].clone()
        klbj, klij = LK.ddim_kl_ref_fwd_bwd(c(ec), c(eu) if train_cfg else None, c(rc), c(ru) if train_cfg else None, c(ts), GUIDE, KL_COEF[train_cfg],
                                            train_cfg, consts, dcj, duj, loss_info=infoj)
        assert klij.shape == () and torch.equal(_bits(klij), _bits(kl_info[j])) and torch.equal(_bits(klbj), _bits(kl_b[sl]))
        assert torch.equal(_bits(dcj), _bits(d_c[sl])) and torch.equal(_bits(infoj), _bits(info[j]))
        if train_cfg:
            assert torch.equal(_bits(duj), _bits(d_u[sl]))
    assert not torch.equal(d_c, d_c0)


@gpu
@pytest.mark.parametrize("train_cfg", [True, False])
def test_info_row_of_a_group_longer_than_one_wave(train_cfg):
    """group = 65: lane 0 of the info kernel's wave takes a second row in its stride loop.  kl_info is the mean of the kernel's own kl_b and the
    loss column moves by kl_coef times it: 65 positive fp32 terms, each addition within 2^-24 of the partial sum -> 65 * 6e-8 = 3.9e-6
    relative at the very most."""
    (d_c, d_u, info, kl_b, kl_info), (_, _, info0) = _device_call("epsilon", train_cfg, 130, 65, 4)
    want = kl_b.double().reshape(2, 65).mean(1)
    assert float(want.min()) > 0
    assert float(((kl_info.double() - want).abs() / want).max()) < 3.9e-6
    # loss column: fp32(loss + fp32(kl_coef * kl_info)) — one rounding of the product, one of the sum (half an ulp each, an ulp allowed)
    moved = info[:, 2].double() - info0[:, 2].double()
    inc = KL_COEF[train_cfg] * kl_info.double()
    assert float(inc.min()) > 0
    assert bool(((moved - inc).abs() <= 2.0 ** -23 * (torch.maximum(info[:, 2].abs(), info0[:, 2].abs()).double() + inc)).all())
    assert torch.equal(info[:, :2], info0[:, :2])


@gpu
def test_every_bad_argument_returns_einval_and_writes_nothing():
    from ddpo_amd import lib_ppo_kl as LK
    fn = LK.load().ddpo_ddim_kl_ref_fwd_bwd
    B, group, chw = 4, 2, 8
    g = torch.Generator().manual_seed(0)
    ec, eu, rc, ru, dc, du = (torch.randn(B, chw + 4, generator=g).to(DEV)[:, :chw].contiguous() for _ in range(6))
    ts = torch.tensor([981, 1, 481, 21], dtype=torch.int32, device=DEV)
    kp, ki, li = torch.full((B,), 7.0, device=DEV), torch.full((B // group,), 7.0, device=DEV), torch.full((B // group, 3), 7.0, device=DEV)
    keep = [t.clone() for t in (dc, du, kp, ki, li)]
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    null = ctypes.c_void_p(0)
    eps_consts = _device_consts("epsilon")
    sample_consts = L.DdimConsts(eps_consts.alphas_cumprod, eps_consts.num_train_timesteps, eps_consts.step_ratio, eps_consts.final_alpha_cumprod,
                                 eps_consts.eta, L.PRED_TYPES["sample"])

    def call(ec=P(ec), eu=P(eu), rc=P(rc), ru=P(ru), ts=P(ts), kl=0.1, cfg=1, c=ctypes.byref(eps_consts), dc=P(dc), du=P(du), kp=P(kp), ki=P(ki),
             B=B, group=group, chw=chw):
        return fn(ec, eu, rc, ru, ts, GUIDE, kl, cfg, c, dc, du, kp, ki, P(li), B, group, chw, L._stream())

    for kw in (dict(ec=null), dict(rc=null), dict(ts=null), dict(dc=null), dict(kp=null), dict(ki=null), dict(c=ctypes.POINTER(L.DdimConsts)()),
               dict(eu=null), dict(ru=null), dict(du=null),
               dict(B=0), dict(B=-4), dict(group=0), dict(group=3), dict(chw=0), dict(chw=6),
               dict(kl=-0.1), dict(kl=float("nan")), dict(kl=float("inf")),
               dict(c=ctypes.byref(sample_consts)),
               dict(ec=ctypes.c_void_p(ec.data_ptr() + 4))):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    for t, t0 in zip((dc, du, kp, ki, li), keep):
        assert torch.equal(t, t0)
    # the same arguments unbroken are accepted (NULL u pointers without train_cfg included), and then the outputs do change
    assert call(cfg=0, eu=null, ru=null, du=null) == 0 and call() == 0
    torch.cuda.synchronize()
    assert not torch.equal(dc, keep[0]) and not torch.equal(du, keep[1]) and not torch.equal(kp, keep[2]) and not torch.equal(li, keep[4])
