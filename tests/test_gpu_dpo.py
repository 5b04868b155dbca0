"""ddpo_dpo_pair_fwd_bwd (ddpo_amd/csrc/dpo_pair.hip), the Diffusion-DPO pass that stands in the place of the RWR loss launch, at the kernel
level: against the float64 oracle of tests/_dpo_oracle.py (the authors' form: two mean squared errors per row, logsigmoid, autograd) on
every pass count of its 1024-thread float4 loop and on one, four and sixty-five pairs, and its exactness contracts (a reference equal to
the policy gives D = 0 exactly, ties give +0.0 gradients, run-to-run / batched-vs-separate / swapped-pair bit equality).

Shapes: chw = 4 is one float4, 4100 a second pass holding one float4, 65540 a 17th pass (only with B <= 8); B = 2 one pair, 8 four pairs,
130 sixty-five pairs: one more than the info kernel's wave covers in one pass of its stride loop.  The labels cycle per pair through
(+1, -1, tie); ref = eps + 1e-2 N(0, 1).  beta is chosen per case on the host so that the largest |s_p| of the float64 oracle is 2: that
pair's q_p = sigmoid(-+2) = 0.12 / 0.88 lies inside (0.05, 0.95) and outside (0.2, 0.8), i.e. the sigmoid is neither saturated nor at its
centre (asserted, with both signs of y where there are two ranked pairs).

Bounds (the house rule of tests/test_gpu_kernel_branches.py:95-98): 8 x the worst error, over all 16 cases below and on these very inputs, of
the fp32 numpy restatement of the closed form (_dpo_oracle.closed_form_numpy) against float64 autograd of the authors' form, computed on the
host, each quantity relative to its case maximum: D 5.20e-7 of max|D| (sum a delta is a sum of both signs), s 1.47e-6 of max|s| = 2
(D_2p - D_2p+1 cancels: worst at B = 2, chw = 65540 under CFG), loss_p 2.85e-6 of max loss_p, the loss column 2.85e-6 of max loss_p,
margin 1.41e-6 of the largest |y_p (D_2p - D_2p+1)|, mse 8.44e-8 and ref_mse 9.67e-8 of themselves, the gradient 2.61e-6 of max|grad|.
implicit_acc is a count over n: equal.  The restatement has to sit inside a quarter of each bound, so the margin stays honest when the
inputs change.  Measured on one MI355X (profiles/dpo_parity.log), the pass's worst over the 16 cases: D 6.81e-7, s 9.23e-7, loss_p 1.75e-6,
loss 1.75e-6, margin 9.22e-7, mse 9.17e-8, ref_mse 7.44e-8, grad 1.56e-6.
"""
import functools

import numpy as np
import pytest
import torch

import _dpo_oracle as DO

gpu = pytest.mark.gpu
DEV = "cuda"

GUIDE = 5.0
REF_NOISE = 1e-2                                      # ref = eps + 1e-2 N(0, 1)
S_MAX = 2.0
SHAPES = [(2, 4), (2, 4100), (2, 65540), (8, 4), (8, 4100), (8, 65540), (130, 4), (130, 4100)]

# the worst error of the restatement per quantity, measured on the host (the module docstring); the bound is 8 x that
NAMES = ("D", "s", "loss_p", "loss", "margin", "mse", "ref_mse", "grad")
WORST = dict(D=5.20e-7, s=1.47e-6, loss_p=2.85e-6, loss=2.85e-6, margin=1.41e-6, mse=8.44e-8, ref_mse=9.67e-8, grad=2.61e-6)
BOUNDS = tuple(8.0 * WORST[n] for n in NAMES)


def _record(line):
    from conftest import parity_record
    parity_record("[dpo pair] " + line)


@functools.lru_cache(maxsize=4)
def _inputs(train_cfg, B, chw):
    """fp32 numpy, shape (B, 4, chw / 4, 1): eps_c, eps_u, ref_c, ref_u, target, and pref (B,)."""
    rng = np.random.default_rng(chw * 131 + B * 7 + int(train_cfg) + 41)
    shp = (B, 4, chw // 4, 1)
    ec, eu, tg = (rng.standard_normal(shp, dtype=np.float32) for _ in range(3))
    rc = (ec + np.float32(REF_NOISE) * rng.standard_normal(shp, dtype=np.float32)).astype(np.float32)
    ru = (eu + np.float32(REF_NOISE) * rng.standard_normal(shp, dtype=np.float32)).astype(np.float32)
    y = np.resize(np.asarray([1.0, -1.0, 0.0], dtype=np.float32), B // 2)
    pref = (np.stack([y, -y], 1).reshape(B) + np.float32(0)).astype(np.float32)
    return ec, eu, rc, ru, tg, pref


def _t64(train_cfg, B, chw):
    ec, eu, rc, ru, tg, pref = _inputs(train_cfg, B, chw)
    d = lambda a: torch.from_numpy(a).double()
    return d(ec), (d(eu) if train_cfg else None), d(rc), (d(ru) if train_cfg else None), d(tg), pref


@functools.lru_cache(maxsize=None)
def _beta(train_cfg, B, chw):
    """The fp32 beta at which the largest |0.5 y_p (D_2p - D_2p+1)| of the float64 oracle gives |s_p| = S_MAX."""
    ec, eu, rc, ru, tg, pref = _t64(train_cfg, B, chw)
    with torch.no_grad():
        D = DO.loss_and_info_torch(ec, eu, rc, ru, tg, pref, GUIDE, 1.0, train_cfg)[3].numpy()
    y = (pref[0::2] - pref[1::2]) / 2
    return float(np.float32(S_MAX / np.abs(0.5 * y * (D[0::2] - D[1::2])).max()))


@functools.lru_cache(maxsize=2)
def _reference(train_cfg, B, chw):
    """float64 autograd of the authors' form: D (B,), s, loss_p, q (B/2,), info {5}, d_eps_c, d_eps_u."""
    ec, eu, rc, ru, tg, pref = _t64(train_cfg, B, chw)
    tec = ec.requires_grad_(True)
    teu = eu.requires_grad_(True) if train_cfg else None
    loss, info, m, D, s, lp = DO.loss_and_info_torch(tec, teu, rc, ru, tg, pref, GUIDE, _beta(train_cfg, B, chw), train_cfg)
    loss.backward()
    s = s.detach().numpy()
    return (D.detach().numpy(), s, lp.detach().numpy(), 1.0 / (1.0 + np.exp(s)), {k: float(v.detach()) for k, v in info.items()},
            tec.grad.numpy(), teu.grad.numpy() if train_cfg else None)


def _restatement(train_cfg, B, chw):
    """closed_form_numpy in the order of the device's outputs: (D, s, loss_p, info, d_c, d_u)."""
    ec, eu, rc, ru, tg, pref = _inputs(train_cfg, B, chw)
    m, D, s, lp, q, info, dc, du = DO.closed_form_numpy(ec, eu if train_cfg else None, rc, ru if train_cfg else None, tg, pref, GUIDE,
                                                        _beta(train_cfg, B, chw), train_cfg)
    return D, s, lp, info, dc, du


def _errors(ref, pref, train_cfg, D, s, loss_p, info, dc, du):
    """The errors in the order of NAMES, each relative to its case maximum; implicit_acc has to be equal."""
    rD, rs, rl, _, rinfo, rdc, rdu = ref
    f = lambda a: np.asarray(a, dtype=np.float64)
    y = (pref[0::2] - pref[1::2]) / 2
    m_max = np.abs(y * (rD[0::2] - rD[1::2])).max()
    info = f(info).reshape(5)
    assert np.float32(info[1]) == np.float32(rinfo["implicit_acc"]), (info[1], rinfo["implicit_acc"])          # a count / n: one rounding
    e_g = float(np.abs(f(dc) - rdc).max() / np.abs(rdc).max())
    if train_cfg:
        e_g = max(e_g, float(np.abs(f(du) - rdu).max() / np.abs(rdu).max()))
    return (float(np.abs(f(D) - rD).max() / np.abs(rD).max()), float(np.abs(f(s) - rs).max() / np.abs(rs).max()),
            float(np.abs(f(loss_p) - rl).max() / rl.max()), float(abs(info[0] - rinfo["loss"]) / rl.max()),
            float(abs(info[2] - rinfo["margin"]) / m_max), float(abs(info[3] - rinfo["mse"]) / rinfo["mse"]),
            float(abs(info[4] - rinfo["ref_mse"]) / rinfo["ref_mse"]), e_g)


def _device_call(train_cfg, B, chw, ref_is_eps=False, swap=False, rows=None, beta=None):
    """(d_c, d_u, per_row, per_pair, info).  swap: the rows of every pair and their labels change places.  rows: a slice, as one call."""
    from ddpo_amd import lib_dpo as LD
    arrs = list(_inputs(train_cfg, B, chw))
    if swap:
        arrs = [a.reshape(B // 2, 2, *a.shape[1:])[:, ::-1].reshape(a.shape).copy() for a in arrs]
    if rows is not None:
        arrs = [np.ascontiguousarray(a[rows]) for a in arrs]
    ec, eu, rc, ru, tg, pref = (torch.from_numpy(a).to(DEV) for a in arrs)
    if not train_cfg:
        eu = ru = None
    if ref_is_eps:
        rc, ru = ec.clone(), (None if eu is None else eu.clone())          # bit-equal, in other buffers
    return LD.dpo_pair_fwd_bwd(ec, eu, rc, ru, tg, pref, GUIDE, _beta(train_cfg, B, chw) if beta is None else beta, train_cfg)


def _bits(t):
    return t.contiguous().view(torch.int32)


@gpu
@pytest.mark.parametrize("train_cfg", [True, False])
@pytest.mark.parametrize("B,chw", SHAPES)
def test_dpo_pass_matches_float64(train_cfg, B, chw):
    ref = _reference(train_cfg, B, chw)
    pref = _inputs(train_cfg, B, chw)[5]
    y = (pref[0::2] - pref[1::2]) / 2
    top = int(np.abs(ref[1]).argmax())
    assert abs(ref[1][top]) == pytest.approx(S_MAX, rel=1e-6) and y[top] != 0
    assert 0.05 < ref[3][top] < 0.95 and not 0.2 < ref[3][top] < 0.8, ref[3][top]     # neither saturated nor at the centre
    if (y != 0).sum() >= 2:
        assert (y > 0).any() and (y < 0).any()
    c = _errors(ref, pref, train_cfg, *_restatement(train_cfg, B, chw))
    print(f"closed form train_cfg={int(train_cfg)} B={B} chw={chw}: " + "; ".join(f"{n} {e:.2e}" for n, e in zip(NAMES, c)))
    assert all(e < b / 4 for e, b in zip(c, BOUNDS)), c
    d_c, d_u, per_row, per_pair, info = _device_call(train_cfg, B, chw)
    assert per_row.shape == (B, 2) and per_pair.shape == (B // 2, 3) and info.shape == (5,) and d_c.shape[0] == B
    assert (d_u is None) == (not train_cfg)
    pp = per_pair.cpu().numpy()
    k = _errors(ref, pref, train_cfg, per_row[:, 1].cpu().numpy(), pp[:, 0], pp[:, 1], info.cpu().numpy(), d_c.cpu().numpy(),
                d_u.cpu().numpy() if train_cfg else None)
    _record(f"train_cfg={int(train_cfg)} B={B} chw={chw} beta={_beta(train_cfg, B, chw):.4g}: " +
            "; ".join(f"{n} {e:.2e} (bound {b:.1e}, closed form {r:.2e})" for n, e, b, r in zip(NAMES, k, BOUNDS, c)))
    assert float(np.abs(pp[:, 2] - ref[3]).max()) < BOUNDS[1] * S_MAX                  # |d sigmoid / d s| <= 1/4
    for n, e, b in zip(NAMES, k, BOUNDS):
        assert e < b, (n, e, b)


@gpu
@pytest.mark.parametrize("train_cfg", [True, False])
@pytest.mark.parametrize("B,chw", [(8, 4), (8, 4100), (130, 4100), (2, 65540)])
def test_reference_equal_to_the_policy(train_cfg, B, chw):
    """ref_* has the bits of eps_*: every D is exactly 0.0, a ranked pair's loss has the bits of log1pf(1.0f), q = 0.5, margin is exactly
    0.0 — and the gradient is not zero: it is (0.25 beta y / n) (-2 / chw) a, checked against float64."""
    beta = 5000.0
    d_c, d_u, per_row, per_pair, info = _device_call(train_cfg, B, chw, ref_is_eps=True, beta=beta)
    ec, eu, _, _, tg, pref = _t64(train_cfg, B, chw)
    y = torch.from_numpy((pref[0::2] - pref[1::2]) / 2).to(DEV)
    assert bool((per_row[:, 1] == 0.0).all()) and bool((per_pair[:, 0] == 0.0).all()) and float(info[2]) == 0.0 and float(info[1]) == 0.0
    assert bool((per_pair[:, 2] == 0.5).all())
    log2 = torch.log1p(torch.ones(1, device=DEV))
    assert abs(float(log2) - float(np.log1p(np.float32(1.0)))) <= 2.0 ** -24        # the device's log1pf(1.0f): within an ulp of the host's
    assert torch.equal(_bits(per_pair[:, 1][y != 0]), _bits(log2.expand(int((y != 0).sum()))))
    assert bool((_bits(per_pair[:, 1][y == 0]) == 0).all())
    assert float(info[3]) == float(info[4])                                         # mse and ref_mse: m - D with D = 0
    tec = ec.requires_grad_(True)
    teu = eu.requires_grad_(True) if train_cfg else None
    DO.loss_and_info_torch(tec, teu, ec.detach(), None if eu is None else eu.detach(), tg, pref, GUIDE, beta, train_cfg)[0].backward()
    gmax = float(tec.grad.abs().max())
    assert gmax > 0 and float(d_c.abs().max()) > 0 and bool(torch.isfinite(d_c).all())
    assert float(np.abs(d_c.cpu().numpy() - tec.grad.numpy()).max()) < BOUNDS[-1] * gmax
    if train_cfg:
        assert bool(torch.isfinite(d_u).all())
        assert float(np.abs(d_u.cpu().numpy() - teu.grad.numpy()).max()) < BOUNDS[-1] * float(teu.grad.abs().max())


EXACT = [(8, 4100), (130, 4), (8, 65540)]


@gpu
@pytest.mark.parametrize("train_cfg", [True, False])
@pytest.mark.parametrize("B,chw", EXACT)
def test_tied_pairs_have_zero_loss_and_all_zero_gradient_bits(train_cfg, B, chw):
    d_c, d_u, per_row, per_pair, info = _device_call(train_cfg, B, chw)
    pref = _inputs(train_cfg, B, chw)[5]
    tie = torch.from_numpy(pref[0::2] == pref[1::2]).to(DEV)
    assert bool(tie.any()) and bool((~tie).any())
    assert bool((_bits(per_pair[:, :2])[tie] == 0).all())                            # s and loss: +0.0
    rows = tie.repeat_interleave(2)
    assert bool((per_row[rows] != 0).all())                                          # m and D are still reported
    assert bool((_bits(d_c)[rows] == 0).all()) and bool((d_c[~rows] != 0).any())
    if train_cfg:
        assert bool((_bits(d_u)[rows] == 0).all())


@gpu
@pytest.mark.parametrize("train_cfg", [True, False])
@pytest.mark.parametrize("B,chw", EXACT)
def test_two_identical_calls_give_identical_bits(train_cfg, B, chw):
    a = _device_call(train_cfg, B, chw)
    b = _device_call(train_cfg, B, chw)
    for u, v in zip(a, b):
        assert (u is None and v is None) or torch.equal(_bits(u), _bits(v))


@gpu
@pytest.mark.parametrize("train_cfg", [True, False])
@pytest.mark.parametrize("chw", [4, 4100, 65540])
def test_one_call_equals_separate_calls_per_pair_bitwise(train_cfg, chw):
    """per_row / per_pair of a B = 8 call equal those of four B = 2 calls bit for bit (the gradient carries 1 / n and differs)."""
    B = 8
    d_c, d_u, per_row, per_pair, info = _device_call(train_cfg, B, chw)
    for p in range(B // 2):
        _, _, rowp, pairp, _ = _device_call(train_cfg, B, chw, rows=slice(2 * p, 2 * p + 2))
        assert torch.equal(_bits(rowp), _bits(per_row[2 * p:2 * p + 2])) and torch.equal(_bits(pairp), _bits(per_pair[p:p + 1]))


@gpu
@pytest.mark.parametrize("train_cfg", [True, False])
@pytest.mark.parametrize("B,chw", EXACT)
def test_swapped_pairs(train_cfg, B, chw):
    """The rows of every pair and their labels change places: per_pair keeps its bits, per_row and the gradients are swapped bitwise."""
    d_c, d_u, per_row, per_pair, info = _device_call(train_cfg, B, chw)
    s_c, s_u, s_row, s_pair, s_info = _device_call(train_cfg, B, chw, swap=True)
    sw = lambda t: t.reshape(B // 2, 2, *t.shape[1:]).flip(1).reshape(t.shape)
    assert torch.equal(_bits(s_pair), _bits(per_pair)) and torch.equal(_bits(s_row), _bits(sw(per_row)))
    assert torch.equal(_bits(s_c), _bits(sw(d_c))) and not torch.equal(_bits(s_c), _bits(d_c))
    if train_cfg:
        assert torch.equal(_bits(s_u), _bits(sw(d_u)))
    assert torch.equal(_bits(s_info), _bits(info))
