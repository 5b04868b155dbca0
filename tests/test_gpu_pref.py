"""ddpo_ddim_pref_fwd_bwd (ddpo_amd/csrc/ppo_pref.hip), the preference-pair pass that stands in the place of the PPO launch, at the kernel
level: against the float64 oracle of tests/_pref_oracle.py (log-prob of the policy minus log-prob of the reference, autograd) on every pass
count of its 1024-thread float4 loop and on one, two and twenty-two micro-batches, and its exactness contracts (a reference equal to the
policy gives h = 0 exactly, ties give +0.0 gradients, run-to-run / grouped-vs-separate / swapped-pair bit equality).

Shapes: chw = 4 is one float4, 4100 a second pass holding one float4, 65540 a 17th pass (only with B <= 8); (B, group) = (2, 2) one pair,
(8, 4) two micro-batches of two pairs, (132, 6) twenty-two of three, (130, 130) one micro-batch of 65 pairs: one more than the info kernel's
wave covers in one pass of its stride loop.  The timesteps cycle per ROW through TS8, so the two rows of a pair always differ in t (using one
row's coefficients for both shows) and t = 1 (sigma = 0.02) and t = 981 are present.  The labels cycle per pair through (+1, -1, tie).
beta is chosen per case on the host so that the largest |s_p| of the float64 oracle is 2: that pair's q_p = sigmoid(-+2) = 0.12 / 0.88 lies
inside (0.05, 0.95) and outside (0.2, 0.8), i.e. the sigmoid is neither saturated nor at its centre (asserted, with both signs of y).
"""
import functools

import numpy as np
import pytest
import torch

from oracle.ddim import DDIMOracle

import _pref_oracle as PO

gpu = pytest.mark.gpu
DEV = "cuda"

TS8 = [981, 1, 481, 21, 961, 501, 41, 241]            # the per-row table of tests/test_gpu_ppo_kl.py
GUIDE = 5.0
REF_NOISE = 1e-2                                      # r = e + 1e-2 N(0, 1)
S_MAX = 2.0
SHAPES = [(2, 2, 4), (2, 2, 4100), (2, 2, 65540), (8, 4, 4), (8, 4, 4100), (8, 4, 65540), (132, 6, 4), (132, 6, 4100), (130, 130, 4)]

# Bounds (the house rule of tests/test_gpu_kernel_branches.py:95-98): 8 x the worst error, over all 36 cases below and on these very inputs, of
# the fp32 numpy restatement of the closed form (_pref_oracle.closed_form_numpy) against float64 autograd of log-prob minus log-prob, computed
# on the host, each quantity relative to its case maximum: h 7.99e-6 of max|h| (r = x' - mu cancels |x'| ~ 1 down to sigma = 0.02 at t = 1, and
# sum r delta is a sum of both signs: worst at B = 2, chw = 4100 without CFG, where |h| is 1e-4), s 6.42e-6 of max|s| = 2, loss_p 5.45e-6 of
# max loss_p, pref_margin 6.44e-6 of the largest |y_p (h_2p - h_2p+1)|, the loss column 5.29e-6 of max loss_p, the gradient 8.90e-6 of
# max|grad|.  pref_acc is a count over n: equal.  The restatement has to sit inside a quarter of each bound, so the margin stays honest when
# the inputs change.
H_REL, S_REL, LOSS_REL, MARGIN_REL, INFO_LOSS_REL, GRAD_REL = 6.4e-5, 5.1e-5, 4.4e-5, 5.1e-5, 4.2e-5, 7.1e-5


def _record(line):
    from conftest import parity_record
    parity_record("[ppo pref] " + line)


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
    """fp32 numpy, shape (B, 4, chw / 4, 1): eps_c, eps_u, ref_c, ref_u, x, x_next (the oracle's DDIM step from the guided prediction), ts, pref."""
    dd, ost = _oracle_sched(pred)
    rng = np.random.default_rng(chw * 131 + B * 7 + 3 * (pred == "v_prediction") + int(train_cfg) + 29)
    shp = (B, 4, chw // 4, 1)
    ec, eu, x, z = (rng.standard_normal(shp, dtype=np.float32) for _ in range(4))
    rc = (ec + np.float32(REF_NOISE) * rng.standard_normal(shp, dtype=np.float32)).astype(np.float32)
    ru = (eu + np.float32(REF_NOISE) * rng.standard_normal(shp, dtype=np.float32)).astype(np.float32)
    ts = np.resize(np.asarray(TS8, dtype=np.int32), B)
    guided = (eu + np.float32(GUIDE) * (ec - eu)).astype(np.float32) if train_cfg else ec
    xn, _ = dd.step(ost, guided, ts, x, noise=z, eta=1.0)
    y = np.resize(np.asarray([1.0, -1.0, 0.0], dtype=np.float32), B // 2)
    pref = (np.stack([y, -y], 1).reshape(B) + np.float32(0)).astype(np.float32)
    return ec, eu, rc, ru, x, xn.astype(np.float32), ts, pref


@functools.lru_cache(maxsize=None)
def _beta(pred, train_cfg, B, chw):
    """The fp32 beta at which the largest |y_p (h_2p - h_2p+1)| of the float64 oracle gives |s_p| = S_MAX."""
    dd, ost = _oracle_sched(pred)
    ec, eu, rc, ru, x, xn, ts, pref = _inputs(pred, train_cfg, B, chw)
    d = lambda a: torch.from_numpy(a).double()
    h = PO.log_ratio_rows_torch(dd, ost, d(ec), d(eu) if train_cfg else None, d(rc), d(ru) if train_cfg else None, d(x), d(xn), ts, GUIDE, 1.0,
                                train_cfg).numpy()
    y = (pref[0::2] - pref[1::2]) / 2
    return float(np.float32(S_MAX / np.abs(y * (h[0::2] - h[1::2])).max()))


@functools.lru_cache(maxsize=2)
def _reference(pred, train_cfg, B, group, chw):
    """float64 autograd of sum_j loss_j: h (B,), s, loss_p, q (B/2,), info (B/group, 3), d_eps_c, d_eps_u."""
    dd, ost = _oracle_sched(pred)
    ec, eu, rc, ru, x, xn, ts, pref = _inputs(pred, train_cfg, B, chw)
    beta = _beta(pred, train_cfg, B, chw)
    d = lambda a: torch.from_numpy(a).double()
    tec, teu = d(ec).requires_grad_(True), d(eu).requires_grad_(True)
    total, hs, ss, ls, infos = 0.0, [], [], [], []
    for j in range(B // group):
        sl = slice(j * group, (j + 1) * group)
        batch = {"ts": ts[sl], "latents": d(x[sl]), "next_latents": d(xn[sl]), "advantages": torch.from_numpy(pref[sl])}
        l, info, h, s, lp = PO.loss_and_info_torch(dd, ost, tec[sl], teu[sl] if train_cfg else None, d(rc[sl]), d(ru[sl]) if train_cfg else None,
                                                   batch, GUIDE, 1.0, beta, train_cfg)
        total = total + l
        hs.append(h.detach().numpy()); ss.append(s.detach().numpy()); ls.append(lp.detach().numpy())
        infos.append([float(info[k].detach()) for k in ("pref_acc", "pref_margin", "loss")])
    total.backward()
    s = np.concatenate(ss)
    return (np.concatenate(hs), s, np.concatenate(ls), 1.0 / (1.0 + np.exp(s)), np.asarray(infos), tec.grad.numpy(),
            teu.grad.numpy() if train_cfg else None)


def _restatement(pred, train_cfg, B, group, chw):
    dd, ost = _oracle_sched(pred)
    ec, eu, rc, ru, x, xn, ts, pref = _inputs(pred, train_cfg, B, chw)
    return PO.closed_form_numpy(dd, ost, ec, eu, rc, ru, x, xn, ts, pref, GUIDE, 1.0, _beta(pred, train_cfg, B, chw), group, train_cfg)


def _errors(ref, pref, train_cfg, h, s, loss_p, info, dc, du):
    """(h, s, loss_p, margin, info loss, gradient) errors, each relative to its case maximum; pref_acc has to be equal."""
    rh, rs, rl, _, rinfo, rdc, rdu = ref
    f = lambda a: np.asarray(a, dtype=np.float64)
    y = (pref[0::2] - pref[1::2]) / 2
    m_max = np.abs(y * (rh[0::2] - rh[1::2])).max()
    info = f(info).reshape(-1, 3)
    assert np.array_equal(info[:, 0].astype(np.float32), rinfo[:, 0].astype(np.float32)), (info[:, 0], rinfo[:, 0])    # a count / n: one rounding
    e_g = float(np.abs(f(dc) - rdc).max() / np.abs(rdc).max())
    if train_cfg:
        e_g = max(e_g, float(np.abs(f(du) - rdu).max() / np.abs(rdu).max()))
    return (float(np.abs(f(h) - rh).max() / np.abs(rh).max()), float(np.abs(f(s) - rs).max() / np.abs(rs).max()),
            float(np.abs(f(loss_p) - rl).max() / rl.max()), float(np.abs(info[:, 1] - rinfo[:, 1]).max() / m_max),
            float(np.abs(info[:, 2] - rinfo[:, 2]).max() / rl.max()), e_g)


BOUNDS = (H_REL, S_REL, LOSS_REL, MARGIN_REL, INFO_LOSS_REL, GRAD_REL)
NAMES = ("h", "s", "loss_p", "pref_margin", "loss", "grad")


def _device_call(pred, train_cfg, B, group, chw, ref_is_eps=False, swap=False, rows=None, beta=None):
    """(d_c, d_u, per_pair, info).  swap: the rows of every pair and their labels change places.  rows: a slice, as one call of its own."""
    from ddpo_amd import lib_pref as LP
    arrs = list(_inputs(pred, train_cfg, B, chw))
    if swap:
        arrs = [a.reshape(B // 2, 2, *a.shape[1:])[:, ::-1].reshape(a.shape).copy() for a in arrs]
    if rows is not None:
        arrs = [np.ascontiguousarray(a[rows]) for a in arrs]
    ec, eu, rc, ru, x, xn, ts, pref = (torch.from_numpy(a).to(DEV) for a in arrs)
    if not train_cfg:
        eu = ru = None
    if ref_is_eps:
        rc, ru = ec, eu
    return LP.ddim_pref_fwd_bwd(ec, eu, rc, ru, x, xn, ts, pref, GUIDE, _beta(pred, train_cfg, B, chw) if beta is None else beta, train_cfg,
                                _device_consts(pred), group=group)


def _bits(t):
    return t.contiguous().view(torch.int32)


@gpu
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("train_cfg", [True, False])
@pytest.mark.parametrize("B,group,chw", SHAPES)
def test_pref_pass_matches_float64(pred, train_cfg, B, group, chw):
    ref = _reference(pred, train_cfg, B, group, chw)
    pref = _inputs(pred, train_cfg, B, chw)[7]
    y = (pref[0::2] - pref[1::2]) / 2
    q = ref[3][y != 0]
    assert ((q > 0.05) & (q < 0.95)).any() and ((q < 0.2) | (q > 0.8)).any(), q       # neither saturated nor at the centre
    if (y != 0).sum() >= 2:
        assert (y > 0).any() and (y < 0).any()
    c = _errors(ref, pref, train_cfg, *_restatement(pred, train_cfg, B, group, chw))
    assert all(e < b / 4 for e, b in zip(c, BOUNDS)), c
    d_c, d_u, per_pair, info = _device_call(pred, train_cfg, B, group, chw)
    assert per_pair.shape == (B // 2, 4) and info.shape == (B // group, 3) and d_c.shape[0] == B and (d_u is None) == (not train_cfg)
    pp = per_pair.cpu().numpy()
    k = _errors(ref, pref, train_cfg, pp[:, :2].reshape(-1), pp[:, 2], pp[:, 3], info.cpu().numpy(), d_c.cpu().numpy(),
                d_u.cpu().numpy() if train_cfg else None)
    _record(f"{pred} train_cfg={int(train_cfg)} B={B} group={group} chw={chw} beta={_beta(pred, train_cfg, B, chw):.4g}: " +
            "; ".join(f"{n} {e:.2e} (bound {b:.1e}, closed form {r:.2e})" for n, e, b, r in zip(NAMES, k, BOUNDS, c)))
    for n, e, b in zip(NAMES, k, BOUNDS):
        assert e < b, (n, e, b)


@gpu
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("train_cfg", [True, False])
@pytest.mark.parametrize("B,group,chw", [(8, 4, 4), (8, 4, 4100), (132, 6, 4100), (2, 2, 65540)])
def test_reference_equal_to_the_policy(pred, train_cfg, B, group, chw):
    """ref_* is eps_*: every h is exactly 0.0, an untied pair's loss has the bits of log1pf(1.0f), pref_margin is exactly 0.0 — and the
    gradient is not zero: it is -+ beta y / (2 n) * d h / d e, checked against float64."""
    dd, ost = _oracle_sched(pred)
    beta = 0.1
    d_c, d_u, per_pair, info = _device_call(pred, train_cfg, B, group, chw, ref_is_eps=True, beta=beta)
    ec, eu, _, _, x, xn, ts, pref = _inputs(pred, train_cfg, B, chw)
    y = torch.from_numpy((pref[0::2] - pref[1::2]) / 2).to(DEV)
    assert bool((per_pair[:, :3] == 0.0).all()) and bool((info[:, :2] == 0.0).all())
    log2 = torch.log1p(torch.ones(1, device=DEV))
    assert abs(float(log2) - float(np.log1p(np.float32(1.0)))) <= 2.0 ** -24        # the device's log1pf(1.0f): within an ulp of the host's
    assert torch.equal(_bits(per_pair[:, 3][y != 0]), _bits(log2.expand(int((y != 0).sum()))))
    assert bool((_bits(per_pair[:, 3][y == 0]) == 0).all())
    d = lambda a: torch.from_numpy(a).double()
    tec, teu = d(ec).requires_grad_(True), d(eu).requires_grad_(True)
    total = 0.0
    for j in range(B // group):
        sl = slice(j * group, (j + 1) * group)
        batch = {"ts": ts[sl], "latents": d(x[sl]), "next_latents": d(xn[sl]), "advantages": torch.from_numpy(pref[sl])}
        total = total + PO.loss_and_info_torch(dd, ost, tec[sl], teu[sl] if train_cfg else None, d(ec[sl]), d(eu[sl]) if train_cfg else None, batch,
                                               GUIDE, 1.0, beta, train_cfg)[0]
    total.backward()
    gmax = float(tec.grad.abs().max())
    assert gmax > 0 and float(d_c.abs().max()) > 0
    assert float(np.abs(d_c.cpu().numpy() - tec.grad.numpy()).max()) < GRAD_REL * gmax
    if train_cfg:
        assert float(np.abs(d_u.cpu().numpy() - teu.grad.numpy()).max()) < GRAD_REL * float(teu.grad.abs().max())


@gpu
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("train_cfg", [True, False])
@pytest.mark.parametrize("B,group,chw", [(8, 4, 4100), (132, 6, 4), (8, 4, 65540)])
def test_tied_pairs_have_zero_loss_and_all_zero_gradient_bits(pred, train_cfg, B, group, chw):
    d_c, d_u, per_pair, info = _device_call(pred, train_cfg, B, group, chw)
    pref = _inputs(pred, train_cfg, B, chw)[7]
    tie = torch.from_numpy(pref[0::2] == pref[1::2]).to(DEV)
    assert bool(tie.any()) and bool((~tie).any())
    assert bool((_bits(per_pair[:, 2:])[tie] == 0).all())                            # s and loss: +0.0
    assert bool((per_pair[:, :2][tie] != 0).all())                                   # h is still reported
    rows = tie.repeat_interleave(2)
    assert bool((_bits(d_c)[rows] == 0).all()) and bool((d_c[~rows] != 0).any())
    if train_cfg:
        assert bool((_bits(d_u)[rows] == 0).all())


@gpu
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("train_cfg", [True, False])
@pytest.mark.parametrize("B,group,chw", [(8, 4, 4100), (132, 6, 4), (8, 4, 65540)])
def test_two_identical_calls_give_identical_bits(pred, train_cfg, B, group, chw):
    a = _device_call(pred, train_cfg, B, group, chw)
    b = _device_call(pred, train_cfg, B, group, chw)
    for u, v in zip(a, b):
        assert (u is None and v is None) or torch.equal(_bits(u), _bits(v))


@gpu
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("train_cfg", [True, False])
@pytest.mark.parametrize("B,group,chw", [(8, 4, 4100), (132, 6, 4), (8, 4, 65540)])
def test_grouped_call_equals_separate_calls_bitwise(pred, train_cfg, B, group, chw):
    d_c, d_u, per_pair, info = _device_call(pred, train_cfg, B, group, chw)
    for j in range(B // group):
        sl = slice(j * group, (j + 1) * group)
        dcj, duj, ppj, infoj = _device_call(pred, train_cfg, B, None, chw, rows=sl)
        assert infoj.shape == (3,) and torch.equal(_bits(infoj), _bits(info[j]))
        assert torch.equal(_bits(ppj), _bits(per_pair[j * group // 2:(j + 1) * group // 2])) and torch.equal(_bits(dcj), _bits(d_c[sl]))
        if train_cfg:
            assert torch.equal(_bits(duj), _bits(d_u[sl]))


@gpu
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("train_cfg", [True, False])
@pytest.mark.parametrize("B,group,chw", [(8, 4, 4100), (132, 6, 4), (8, 4, 65540)])
def test_swapped_pairs(pred, train_cfg, B, group, chw):
    """The rows of every pair and their labels change places: s_p and loss_p keep their bits, h and the gradients are swapped bitwise."""
    d_c, d_u, per_pair, info = _device_call(pred, train_cfg, B, group, chw)
    s_c, s_u, s_pair, s_info = _device_call(pred, train_cfg, B, group, chw, swap=True)
    sw = lambda t: t.reshape(B // 2, 2, *t.shape[1:]).flip(1).reshape(t.shape)
    assert torch.equal(_bits(s_pair[:, 2:]), _bits(per_pair[:, 2:])) and torch.equal(_bits(s_pair[:, :2]), _bits(per_pair[:, :2].flip(1)))
    assert torch.equal(_bits(s_c), _bits(sw(d_c))) and not torch.equal(_bits(s_c), _bits(d_c))
    if train_cfg:
        assert torch.equal(_bits(s_u), _bits(sw(d_u)))
    assert torch.equal(_bits(s_info), _bits(info))
