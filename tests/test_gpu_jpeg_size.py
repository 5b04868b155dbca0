"""The JPEG byte counter on the GPU (csrc/jpeg_size.hip) against PIL called here and against the counts recorded in tests/golden/jpeg_sizes.json —
exact integers, no tolerance — and the jpeg_device / neg_jpeg_device rewards built on it, up to the entrypoint."""
import os
import sys

import numpy as np
import pytest
import torch

from _jpeg_cases import RECIPES, load_golden, make_image, to_u8
from ddpo_amd import lib as L
from ddpo_amd.training import callbacks as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [(16, 16), (48, 32), (64, 64)]
QUALITIES = [25, 50, 80, 95, 100]


def _pil(img, q):
    return len(C.encode_jpeg(img, quality=q))


def _as_float(img):
    """float32 whose reference truncation gives back the uint8 image ((k + 0.5) / 255 sits half a level away from both neighbours)."""
    return img if img.dtype == np.float32 else np.minimum((img.astype(np.float32) + np.float32(0.5)) / np.float32(255), np.float32(1))


@pytest.mark.parametrize("h,w", SMALL)
def test_kernel_equals_pil_and_the_recorded_counts(h, w):
    gold = load_golden()
    imgs = [make_image(r, 100 + i, h, w) for i, r in enumerate(RECIPES)]
    u8 = torch.from_numpy(np.stack([to_u8(im) for im in imgs])).cuda()
    f32 = torch.from_numpy(np.stack([_as_float(im) for im in imgs])).cuda()
    assert np.array_equal((f32.cpu().numpy() * 255).astype(np.uint8), u8.cpu().numpy())
    for q in QUALITIES:
        want = [_pil(im, q) for im in imgs]
        assert want == [gold[(r, 100 + i, h, w, q)] for i, r in enumerate(RECIPES)], "the live PIL and the recorded counts disagree: another libjpeg?"
        got_u8, got_f32 = L.jpeg_size(u8, q), L.jpeg_size(f32, q)
        assert got_u8.dtype == torch.int64 and got_u8.is_cuda
        assert got_u8.tolist() == want, (h, w, q, "uint8")
        assert got_f32.tolist() == want, (h, w, q, "float32")
        assert L.jpeg_size_host(u8.cpu().numpy(), q).tolist() == want


def test_images_of_a_batch_do_not_see_each_other():
    """Per-image scan and DC predictors: every image of a mixed batch gets the count it gets alone."""
    recipes = ["noise", "const", "sparse", "checker", "smooth"]
    imgs = [to_u8(make_image(r, 40 + i, 64, 64)) for i, r in enumerate(recipes)]
    batch = L.jpeg_size(torch.from_numpy(np.stack(imgs)).cuda(), 95).tolist()
    alone = [int(L.jpeg_size(torch.from_numpy(im[None]).cuda(), 95)[0]) for im in imgs]
    assert batch == alone == [_pil(im, 95) for im in imgs]


def test_512_pair_reaches_the_32_bit_offset_range():
    gold = load_golden()
    imgs = [make_image(r, 7, 512, 512) for r in ("noise", "smooth")]
    want = [_pil(im, 95) for im in imgs]
    assert want == [gold[(r, 7, 512, 512, 95)] for r in ("noise", "smooth")]
    assert (want[0] - 625) * 8 > 2_000_000                                 # megabits of scan data in the noise image
    u8 = torch.from_numpy(np.stack(imgs)).cuda()
    assert L.jpeg_size(u8, 95).tolist() == want
    assert L.jpeg_size(torch.from_numpy(np.stack([_as_float(im) for im in imgs])).cuda(), 95).tolist() == want


def test_two_sizers_on_two_streams():
    from ddpo_amd.models.jpeg_size import JpegSizer
    a, b = JpegSizer(), JpegSizer()
    assert a.stream != b.stream
    xa = torch.from_numpy(np.stack([make_image("noise", 60 + i, 64, 64) for i in range(4)])).cuda()
    xb = torch.from_numpy(np.stack([make_image("smooth", 70 + i, 64, 64) for i in range(4)])).cuda()
    torch.cuda.synchronize()
    got = []
    for s, x in ((a, xa), (b, xb)):                                        # back to back, nothing in between waits
        with torch.cuda.stream(s.stream):
            got.append(L.jpeg_size(x, 95, workspace=s._workspace(*x.shape[:3])))
    torch.cuda.synchronize()
    assert a.workspace.data_ptr() != b.workspace.data_ptr()
    want = [[_pil(im, 95) for im in x.cpu().numpy()] for x in (xa, xb)]
    assert [g.tolist() for g in got] == want
    assert a(xa).tolist() == want[0] and b(xb.cpu().numpy()).tolist() == want[1]


def test_wrapper_refuses_sizes_off_the_mcu_grid():
    from ddpo_amd.models.jpeg_size import JpegSizer
    bad = torch.zeros(1, 24, 40, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="multiples of 16"):
        L.jpeg_size(bad, 95)
    with pytest.raises(ValueError, match="multiples of 16"):
        JpegSizer()(bad)
    with pytest.raises(ValueError, match="multiples of 16"):
        JpegSizer()(np.zeros((1, 24, 40, 3), np.float32))


def test_floats_outside_the_unit_interval_follow_the_documented_rule():
    """float32 -> byte is "truncated as (uint8)(x * 255.0f), clamped; NaN -> 0" for every float, not only those in [0, 1]."""
    special = {np.nan: 0, np.inf: 255, -np.inf: 0, 1e30: 255, -1e30: 0, -0.0: 0, 1 + 2.0 ** -23: 255, -2.0 ** -149: 0}
    rng = np.random.default_rng(5)
    x = rng.random((1, 16, 16, 3), dtype=np.float32)
    u8 = (x * 255).astype(np.uint8)
    for i, (v, b) in enumerate(special.items()):
        for c in range(3):
            x[0, i, (5 * i + 7 * c) % 16, c], u8[0, i, (5 * i + 7 * c) % 16, c] = v, b
    assert np.isnan(x).sum() == 3 and np.isinf(x).sum() == 6 and (x == np.float32(1 + 2.0 ** -23)).sum() == 3
    dev = torch.from_numpy(x).cuda()
    for q in (50, 95):
        assert L.jpeg_size(dev, q).tolist() == L.jpeg_size(torch.from_numpy(u8).cuda(), q).tolist() == L.jpeg_size_host(u8, q).tolist()
        files, lengths = L.jpeg_encode(dev, q)
        assert bytes(files[0, :int(lengths[0])].cpu().numpy()) == L.jpeg_encode_host(u8, q)[0]


def test_wrapper_refuses_an_out_it_would_overrun():
    x = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device="cuda")
    for bad in (torch.full((2,), 7, dtype=torch.int32, device="cuda"), torch.full((1,), 7, dtype=torch.int64, device="cuda"),
                torch.full((2, 2), 7, dtype=torch.int64, device="cuda")[:, 0]):
        with pytest.raises(L.DdpoHipError, match="out must be"):
            L.jpeg_size(x, 95, out=bad)
        torch.cuda.synchronize()
        assert bool((bad == 7).all())                                      # nothing was launched
    good = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    assert L.jpeg_size(x, 95, out=good) is good and good.tolist() == L.jpeg_size(x, 95).tolist()


def test_device_callbacks_equal_the_host_callbacks():
    imgs = np.stack([_as_float(make_image(r, 80 + i, 64, 64)) for i, r in enumerate(RECIPES)])
    prompts = ["x"] * len(imgs)
    for name in ("jpeg", "neg_jpeg"):
        want, _ = C.evaluate_callbacks({name: C.callback_fns[name]()}, imgs, prompts, None)[name]
        fn = C.callback_fns[name + "_device"]()
        assert fn.wants_device_images
        got_np, info = C.evaluate_callbacks({name: fn}, imgs, prompts, None)[name]
        got_dev, _ = C.evaluate_callbacks_device({name: fn}, torch.from_numpy(imgs).cuda(), prompts, None)[name]
        assert info == {}
        for got in (got_np, got_dev):
            assert got.dtype == np.float64 and got.shape == want.shape == (len(imgs), 1) and np.array_equal(got, want)


def test_entrypoint_with_jpeg_device_equals_jpeg(tmp_path, monkeypatch):
    """tests/test_gpu_entrypoint.py's run (tiny model, 64 px, 4 steps, batch 2), one epoch, with the reward counted on the device."""
    monkeypatch.setenv("DDPO_MODEL_CONFIG", "tiny")
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, ROOT)
    import importlib
    pg = importlib.import_module("pipeline.policy_gradient")
    flags = ["--dataset", "compressed-animals", "--resolution", "64", "--n_inference_steps", "4", "--sample_batch_size", "2", "--train_batch_size", "2",
             "--num_train_epochs", "1", "--save_freq", "1", "--per_prompt_stats_min_count", "2", "--learning_rate", "1e-4"]
    host = pg.main(flags + ["--logbase", str(tmp_path / "host")])
    dev = pg.main(flags + ["--filter_field", "jpeg_device", "--logbase", str(tmp_path / "dev")])
    r_host = np.load(os.path.join(host["localpath"], "rewards/0_0.npy"))
    r_dev = np.load(os.path.join(dev["localpath"], "rewards/0_0.npy"))
    assert r_dev.shape == (2, 1) and r_dev.dtype == np.float64 and np.array_equal(r_dev, r_host)
    assert dev["mean_rewards"] == host["mean_rewards"]
    with open(os.path.join(host["localpath"], "samples/0_0_0.png"), "rb") as f, open(os.path.join(dev["localpath"], "samples/0_0_0.png"), "rb") as g:
        assert f.read() == g.read()                                        # the inspection image is the same file
