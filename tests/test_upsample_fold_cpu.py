"""The algebra behind the folded nearest-2x up-sampler (lib.conv2d_up2x_folded / ddpo_conv_up2x_folded_fwd), on the CPU in float64:
conv3x3(nearest_upsample_2x(x), pad 1) equals four 2x2 convolutions on the source grid with pre-summed kernels, borders included."""
import pytest
import torch
import torch.nn.functional as TF

from ddpo_amd import lib as L


def _gather_form(x, w):
    xin = TF.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
    return TF.conv2d(xin, w.permute(3, 2, 0, 1), None, padding=1).permute(0, 2, 3, 1)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 1, 1, 3, 2), (2, 3, 5, 4, 6), (1, 8, 8, 5, 3), (2, 5, 3, 2, 2), (1, 1, 4, 3, 3), (1, 7, 1, 2, 4)])
def test_folded_form_equals_upsample_then_conv3x3_in_float64(B, H, W, Cin, Cout):
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(B, H, W, Cin, generator=g, dtype=torch.float64)
    w = torch.randn(3, 3, Cin, Cout, generator=g, dtype=torch.float64)
    ref = _gather_form(x, w)
    out = L.conv_up2x_folded_reference(x, w)
    assert out.shape == ref.shape == (B, 2 * H, 2 * W, Cout)
    rel = float((out - ref).abs().max() / ref.abs().max())
    print(f"fold vs gather, {H}x{W}: {rel:.3e}")
    assert rel <= 1e-12


def test_phase_kernels_are_the_tap_sums():
    w = torch.arange(9, dtype=torch.float64).view(3, 3, 1, 1) + 1.0          # w[ky, kx] = 3 ky + kx + 1
    wf = L.fold_up2x_kernel_reference(w)[..., 0, 0]
    assert wf.shape == (4, 2, 2)
    # phase (0, 0): offsets {-1, 0} per axis: rows {0 | 1 + 2}, columns {0 | 1 + 2}
    assert wf[0].tolist() == [[1.0, 2.0 + 3.0], [4.0 + 7.0, 5.0 + 6.0 + 8.0 + 9.0]]
    # phase (1, 1): offsets {0, +1}: rows {0 + 1 | 2}, columns {0 + 1 | 2}
    assert wf[3].tolist() == [[1.0 + 2.0 + 4.0 + 5.0, 3.0 + 6.0], [7.0 + 8.0, 9.0]]
    # every phase uses each of the nine taps exactly once
    assert all(float(wf[p].sum()) == 45.0 for p in range(4))


def test_fp32_fold_sums_ky_then_kx_ascending():
    g = torch.Generator().manual_seed(0)
    w = torch.randn(3, 3, 4, 4, generator=g)
    wf = L.fold_up2x_kernel_reference(w)
    assert wf.dtype == torch.float32
    assert torch.equal(wf[0, 1, 1], ((w[1, 1] + w[1, 2]) + w[2, 1]) + w[2, 2])
    assert torch.equal(wf[3, 0, 0], ((w[0, 0] + w[0, 1]) + w[1, 0]) + w[1, 1])
    assert torch.equal(wf[1, 0, 1], w[0, 2]) and torch.equal(wf[2, 1, 0], w[2, 0])
