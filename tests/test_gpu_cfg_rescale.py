"""ddpo_cfg_rescale_fwd / ddpo_cfg_rescale_bwd (ddpo_amd/csrc/cfg_rescale.hip), the rescaled classifier-free guidance of
`--guidance_rescale`, at the kernel level: against float64 torch autograd of the formula as written (tests/_cfg_rescale_oracle.py) on every
pass count of the 1024-thread float4 loops, and the exactness contracts (run-to-run, batched-vs-separate, no launch on a bad argument).

Shapes, from the kernels' own loop (`for i = 4 tid; i < chw; i += 4096`): chw = 8 two float4 (the smallest row the entry takes), 4096 one
full pass, 4100 a second pass holding one float4, 1028 one pass that a quarter of the threads take, 16384 the SD latent (four passes),
65540 a 17th pass (only with B = 2); B = 1 and 5.  Inputs: t ~ N(0, 1), u = t + 0.33 N(0, 1), cotangent ~ N(0, 1), g = 5, phi = 0.7,
default_rng(chw * 131 + B * 7 + 53); one case with a row mean of 3 covers the centring.  Every row's k of the float64 side lies in
(0.4, 0.9) (asserted): 0.464 .. 0.737 over the cases below.  chw = 8 runs at B = 5 only: its B = 1 draw has k = 0.920.

Bounds (the house rule of tests/test_gpu_kernel_branches.py:95-98): 8 x the worst error, over all cases below and on these very inputs, of
the fp32 numpy restatement of the closed form (_cfg_rescale_oracle.closed_form_numpy) against the float64 reference, computed on the host:
out 1.61e-7, d_t 1.66e-7, d_u 1.46e-7 of the case maximum; the two means 1.06e-7 of their row's standard deviation (the row-mean-3 case;
5.8e-9 without a mean); the two standard deviations 7.52e-8 of themselves.  The restatement has to sit inside a quarter of each bound.
Measured on one MI355X (profiles/cfg_rescale_parity.log), the kernels' worst over the cases: out 1.61e-7, means 1.06e-7, standard
deviations 7.52e-8, d_t 1.80e-7 (B = 2, chw = 65540), d_u 1.42e-7.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _cfg_rescale_oracle as RO

gpu = pytest.mark.gpu
DEV = "cuda"

CASES = [(5, 8, 0.0), (1, 4096, 0.0), (5, 4096, 0.0), (1, 4100, 0.0), (5, 4100, 0.0), (5, 1028, 0.0), (2, 16384, 0.0), (5, 16384, 0.0),
         (2, 65540, 0.0), (5, 4100, 3.0)]
WORST = dict(out=1.61e-7, mean=1.06e-7, std=7.52e-8, d_t=1.66e-7, d_u=1.46e-7)
BOUNDS = tuple(8.0 * WORST[n] for n in RO.NAMES)


def _record(line):
    from conftest import parity_record
    parity_record("[cfg rescale] " + line)


@functools.lru_cache(maxsize=None)
def _inputs(B, chw, row_mean):
    return RO.inputs(B, chw, row_mean)


@functools.lru_cache(maxsize=None)
def _reference(B, chw, row_mean):
    return RO.reference(*_inputs(B, chw, row_mean))


def _device_call(B, chw, row_mean, rows=None):
    """(out, stats, d_t, d_u) of the two launches; rows: a slice, as one call."""
    from ddpo_amd import lib_cfg_rescale as LR
    arrs = _inputs(B, chw, row_mean)
    if rows is not None:
        arrs = [np.ascontiguousarray(a[rows]) for a in arrs]
    t, u, G = (torch.from_numpy(a).to(DEV) for a in arrs)
    out, stats = LR.cfg_rescale_fwd(t, u, RO.GUIDE, RO.PHI)
    d_t, d_u = LR.cfg_rescale_bwd(t, u, G, stats, RO.GUIDE, RO.PHI)
    return out, stats, d_t, d_u


def _bits(t):
    return t.contiguous().view(torch.int32)


@gpu
@pytest.mark.parametrize("B,chw,row_mean", CASES)
def test_rescale_matches_float64(B, chw, row_mean):
    ref = _reference(B, chw, row_mean)
    k = ref[1]
    assert k.shape == (B,) and 0.4 < k.min() and k.max() < 0.9, k                      # neither a no-op nor degenerate
    t, u, G = _inputs(B, chw, row_mean)
    c = RO.errors(ref, *RO.closed_form_numpy(t, u, G, RO.GUIDE, RO.PHI))
    print(f"closed form B={B} chw={chw} mean={row_mean:g}: " + "; ".join(f"{n} {e:.2e}" for n, e in zip(RO.NAMES, c)))
    assert all(e < b / 4 for e, b in zip(c, BOUNDS)), c
    out, stats, d_t, d_u = _device_call(B, chw, row_mean)
    assert out.shape == t.shape and stats.shape == (B, 4) and d_t.shape == t.shape and d_u.shape == t.shape
    e = RO.errors(ref, out.cpu().numpy(), stats.cpu().numpy(), d_t.cpu().numpy(), d_u.cpu().numpy())
    _record(f"B={B} chw={chw} mean={row_mean:g} k {k.min():.3f}..{k.max():.3f}: " +
            "; ".join(f"{n} {x:.2e} (bound {b:.1e}, closed form {r:.2e})" for n, x, b, r in zip(RO.NAMES, e, BOUNDS, c)))
    for n, x, b in zip(RO.NAMES, e, BOUNDS):
        assert x < b, (n, x, b)


EXACT = [(5, 8, 0.0), (5, 4100, 3.0), (5, 16384, 0.0), (2, 65540, 0.0)]


@gpu
@pytest.mark.parametrize("B,chw,row_mean", EXACT)
def test_two_identical_calls_give_identical_bits(B, chw, row_mean):
    a = _device_call(B, chw, row_mean)
    b = _device_call(B, chw, row_mean)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))


@gpu
@pytest.mark.parametrize("chw,row_mean", [(8, 0.0), (4100, 3.0), (16384, 0.0)])
def test_one_call_equals_separate_calls_per_row_bitwise(chw, row_mean):
    """Outputs, stats and both gradients of a B = 5 call equal those of five B = 1 calls bit for bit: nothing depends on B."""
    B = 5
    whole = _device_call(B, chw, row_mean)
    for b in range(B):
        one = _device_call(B, chw, row_mean, rows=slice(b, b + 1))
        for x, y in zip(whole, one):
            assert torch.equal(_bits(x[b:b + 1]), _bits(y))


@gpu
def test_bad_arguments_return_without_a_launch():
    """DDPO_EINVAL on device buffers: the outputs keep the pattern they were filled with."""
    from ddpo_amd import lib as L, lib_cfg_rescale as LR
    lib = LR.load()
    B, chw = 2, 16
    t, u, G = (torch.randn(B, chw, device=DEV) for _ in range(3))
    out, d_t, d_u = (torch.full((B, chw + 4), 7.0, device=DEV) for _ in range(3))
    stats = torch.full((B, 4), 7.0, device=DEV)
    p = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)
    s = L._stream()
    fwd = lambda ec=p(t), eu=p(u), phi=0.7, o=p(out), st=p(stats), B=B, chw=chw: lib.ddpo_cfg_rescale_fwd(ec, eu, 5.0, phi, o, st, B, chw, s)
    bwd = lambda ec=p(t), g=p(G), phi=0.7, dc=p(d_t), du=p(d_u), B=B, chw=chw: lib.ddpo_cfg_rescale_bwd(ec, p(u), g, p(stats), 5.0, phi, dc, du,
                                                                                                   B, chw, s)
    for kw in (dict(ec=None), dict(o=None), dict(st=None), dict(B=0), dict(chw=4), dict(chw=18), dict(chw=-16), dict(phi=1.01), dict(phi=-1e-3),
               dict(phi=float("nan")), dict(phi=float("inf")), dict(ec=p(t, 4)), dict(o=p(out, 4))):
        assert fwd(**kw) == -1, kw
    for kw in (dict(ec=None), dict(g=None), dict(dc=None), dict(du=None), dict(B=-1), dict(chw=4), dict(chw=18), dict(phi=2.0),
               dict(phi=float("nan")), dict(g=p(G, 4)), dict(dc=p(d_t, 4)), dict(du=p(d_u, 4))):
        assert bwd(**kw) == -1, kw
    torch.cuda.synchronize()
    for x in (out, d_t, d_u, stats):
        assert bool((x == 7.0).all())
    assert fwd() == 0 and bwd() == 0                                                   # and the good call is taken
    torch.cuda.synchronize()
    assert bool((out[0, :chw] != 7.0).all())
