"""The resize kernel (csrc/resize_u8.hip) against its serial host twin, which tests/test_thumbnail_cpu.py holds to Pillow — bytes, so
`array_equal` and no tolerance — and what is built on it: ThumbnailEmbedder and the `thumbnail_device` reward against their host twins, bit for
bit."""
import threading

import numpy as np
import pytest
import torch

import _thumbnail_cases as TC
from ddpo_amd import lib as L
from ddpo_amd.models import clip_vision as CV
from ddpo_amd.models import thumbnail as TH
from ddpo_amd.models.laion import synthetic_state_dicts
from ddpo_amd.training import callbacks as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64


def _misaligned(a):
    """The same values one element past an aligned base: the kernel's element-wise loads instead of the 4-element ones."""
    buf = torch.empty(a.size + 1, dtype=torch.from_numpy(a[:0]).dtype, device=DEV)
    buf[1:] = torch.from_numpy(a).to(DEV).reshape(-1)
    return buf[1:].view(a.shape)


def _resized(x, oh, ow, shift=0):
    """lib.resize_u8 into a slice, `shift` bytes past an aligned base, of a larger buffer pre-filled with 0xAB: every output byte must be written
    and the guard bytes on both sides left alone.  Returns the output on the host."""
    n = x.shape[0] * oh * ow * 3
    buf = torch.full((GUARD + shift + n + GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    out = buf[GUARD + shift:GUARD + shift + n].view(x.shape[0], oh, ow, 3)
    assert L.resize_u8(x, oh, ow, out=out) is out
    host = buf.cpu().numpy()
    assert (host[:GUARD + shift] == 0xAB).all() and (host[GUARD + shift + n:] == 0xAB).all(), "guard bytes were written"
    return host[GUARD + shift:GUARD + shift + n].reshape(x.shape[0], oh, ow, 3)


@pytest.mark.parametrize("shape,outs", TC.RESIZES, ids=[f"{h}x{w}" for (h, w), _ in TC.RESIZES])
def test_resize_kernel_equals_host_twin(shape, outs):
    """The shapes of tests/test_thumbnail_cpu.py (there against Pillow), two images each.  uint8 and float32; an aligned base (16-byte loads where
    W % 4 == 0: all but 17x23) and one element past it (element-wise loads); an output that starts on a 4-byte boundary and one byte past it
    (head bytes before the packed stores); one image sliced out of the batch."""
    u8 = TC.resize_input(*shape, n=2)
    f32 = TC.as_float(u8)
    for oh, ow in outs:
        want = L.resize_u8_host(u8, oh, ow)
        for x in (u8, f32):
            assert np.array_equal(_resized(torch.from_numpy(x).to(DEV), oh, ow), want), (oh, ow, x.dtype)
            assert np.array_equal(_resized(_misaligned(x), oh, ow, shift=1), want), (oh, ow, x.dtype, "misaligned")
        assert np.array_equal(_resized(torch.from_numpy(f32).to(DEV)[1:2], oh, ow, shift=3), want[1:2]), (oh, ow, "one image of the batch")
        assert np.array_equal(L.resize_u8(torch.from_numpy(u8).to(DEV), oh, ow).cpu().numpy(), want)            # an output of its own


def test_more_output_rows_than_one_band():
    """300 x 52 -> 75 x 13: 38 bands of 2 output rows, the last of 1; a band's 20 input rows are two full stages of CP_STAGE_ROWS and one of 4,
    and the image's last band stops at row 300, no multiple of 8; 39-byte output rows, so every band starts off a 4-byte boundary or ends off
    one.  150 x 16 -> 140 x 12: bands that need fewer input rows than one stage."""
    u8 = TC.resize_input(300, 52, n=2)
    geo = L.resize_u8_geometry(300, 52, 75, 13)
    assert geo["band"] == L.RESIZE_U8_BAND == 2 and 75 % geo["band"] and geo["rows"] > L.CLIP_STAGE_ROWS
    assert geo["rows"] % L.CLIP_STAGE_ROWS and 300 % L.CLIP_STAGE_ROWS
    want = L.resize_u8_host(u8, 75, 13)
    for x in (u8, TC.as_float(u8)):
        assert np.array_equal(_resized(torch.from_numpy(x).to(DEV), 75, 13), want), x.dtype
        assert np.array_equal(_resized(_misaligned(x), 75, 13, shift=2), want), (x.dtype, "misaligned")
    small = TC.resize_input(150, 16, n=1)
    assert L.resize_u8_geometry(150, 16, 140, 12)["rows"] < L.CLIP_STAGE_ROWS
    assert np.array_equal(_resized(torch.from_numpy(small).to(DEV), 140, 12), L.resize_u8_host(small, 140, 12))


def test_arbitrary_floats_are_truncated_like_the_reference():
    x = np.random.default_rng(3).random((2, 32, 40, 3), dtype=np.float32)
    x[0, 0, 0] = (1.0, 0.0, np.float32(254.999) / np.float32(255))
    u8 = (x * 255).astype(np.uint8)
    assert (u8 != np.rint(x * 255)).any()
    assert np.array_equal(_resized(torch.from_numpy(x).to(DEV), 8, 10), L.resize_u8_host(u8, 8, 10))
    assert np.array_equal(_resized(torch.from_numpy(x).to(DEV), 32, 40), u8)


def test_wrapper_refusals():
    x = torch.zeros(2, 24, 40, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="contiguous"):
        L.resize_u8(x.permute(0, 2, 1, 3), 6, 10)
    with pytest.raises(ValueError, match="dtype must be float32 or uint8"):
        L.resize_u8(x.double(), 6, 10)
    with pytest.raises(ValueError, match="last dimension 3"):
        L.resize_u8(x[..., :2].contiguous(), 6, 10)
    with pytest.raises(ValueError, match="empty batch"):
        L.resize_u8(x[:0], 6, 10)
    with pytest.raises(ValueError, match="positive integers"):
        L.resize_u8(x, 0, 10)
    with pytest.raises(ValueError, match="must fit the 160 KB of LDS"):
        L.resize_u8(torch.zeros(1, 16, 7000, 3, dtype=torch.uint8, device=DEV), 4, 1750)
    with pytest.raises(L.DdpoHipError, match="CUDA tensor"):
        L.resize_u8(x.cpu(), 6, 10)
    for bad in (torch.empty(2, 6, 10, 3, dtype=torch.float32, device=DEV), torch.empty(2, 10, 6, 3, dtype=torch.uint8, device=DEV),
                torch.empty(2, 6, 10, 3, dtype=torch.uint8)):
        with pytest.raises(L.DdpoHipError, match="out must be"):
            L.resize_u8(x, 6, 10, out=bad)


# ------------------------------------------------------------------------------------------------ embedder and callbacks
def _embedder(monkeypatch, datapath, seed=5):
    monkeypatch.setattr(L, "DATAPATH", datapath)
    cfg = CV.VisionConfig.named("tiny")
    return TH.ThumbnailEmbedder(config="tiny", clip_state=synthetic_state_dicts(cfg, cfg.proj, seed)[0], device=DEV)


def _both(images, **kw):
    """(`thumbnail` through evaluate_callbacks, `thumbnail_device` through evaluate_callbacks_device on the CUDA batch)"""
    n = len(images)
    host = C.evaluate_callbacks({"t": C.callback_fns["thumbnail"](**kw)}, images, ["p"] * n, ({},) * n)["t"]
    fn = C.callback_fns["thumbnail_device"](**kw)
    assert fn.wants_device_images
    dev = C.evaluate_callbacks_device({"t": fn}, torch.from_numpy(images).to(DEV), ["p"] * n, ({},) * n)["t"]
    return host, dev


def _images(n, h, w):
    images = np.random.default_rng(h * w).random((n, h, w, 3), dtype=np.float32)
    ramp = np.linspace(0, 0.8, w, dtype=np.float32)[None, :, None]
    images[-1] = np.clip(images[-1] * 0.2 + ramp, 0, 1)                                  # one smooth image: a smaller angle than noise
    return images


@pytest.mark.parametrize("datapath", ["fp32", "bf16x3"])
def test_thumbnail_on_device_images_equals_host_images(datapath, monkeypatch):
    """64 x 64 and 48 x 80 images on the tiny tower (56-pixel input): thumbnails of 16, 8, 4 and of 12 x 20, 6 x 10, 3 x 5 pixels, which
    lib.clip_preprocess scales back UP to 56 on the short side."""
    emb = _embedder(monkeypatch, datapath)
    for n, h, w in [(3, 64, 64), (2, 48, 80)]:
        images = _images(n, h, w)
        feats = emb(images)
        assert feats.shape == (4 * n, emb.cfg.proj) and feats.dtype == np.float32 and np.isfinite(feats).all()
        assert np.array_equal(emb(torch.from_numpy(images).to(DEV)), feats)
        (want, want_info), (got, info) = _both(images, embedder=emb)
        assert got.dtype == want.dtype == np.float32 and got.shape == (n,) and np.array_equal(got, want)
        assert (got <= 0).all() and len(set(got.tolist())) > 1
        assert set(info) == set(want_info) and not info["synthetic_weights"]
    for shape in [(1, 15, 64, 3), (1, 64, 15, 3)]:
        with pytest.raises(ValueError, match="at least 16 pixels"):
            emb(torch.zeros(shape, device=DEV))
        with pytest.raises(ValueError, match="at least 16 pixels"):
            emb(np.zeros(shape, np.float32))


def test_thumbnail_device_from_a_worker_thread_while_the_main_stream_is_busy(monkeypatch):
    """The entrypoint's arrangement: the producer records `ready` on its stream, a worker thread evaluates the reward on its own stream, the main
    thread keeps its stream busy meanwhile."""
    emb = _embedder(monkeypatch, "bf16x3")
    fns = {"thumbnail_device": C.callback_fns["thumbnail_device"](embedder=emb)}
    host = _images(4, 64, 64)
    want = {k: fn(host, ["p"] * 4, ({},) * 4) for k, fn in fns.items()}
    a = torch.randn(1024, 1024, device=DEV)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        images = torch.from_numpy(host).to(DEV) * 1.0
        ready = side.record_event()
    out = {}
    th = threading.Thread(target=lambda: out.setdefault("r", C.evaluate_callbacks_device(fns, images, ["p"] * 4, ({},) * 4, ready=ready)))
    th.start()
    for _ in range(50):
        a = (a @ a).clamp_(-1, 1)
    th.join()
    torch.cuda.synchronize()
    assert set(out["r"]) == set(fns)
    assert np.array_equal(out["r"]["thumbnail_device"][0], want["thumbnail_device"][0])


def test_entrypoint_with_thumbnail_device_equals_thumbnail(tmp_path, monkeypatch):
    """tests/test_gpu_entrypoint.py's run (tiny model, 64 px, 4 steps, batch 2), one epoch, learning rate 0: the reward computed from the decoder's
    device tensor is the reward computed from the host copy, on a synthetic tiny tower."""
    import importlib
    import os
    from ddpo_amd.models import clip_text as CT
    monkeypatch.setenv("DDPO_MODEL_CONFIG", "tiny")
    monkeypatch.setenv("DDPO_ALLOW_SYNTHETIC", "1")
    monkeypatch.setattr(CV.VisionConfig, "named", staticmethod(lambda name, _orig=CV.VisionConfig.named: _orig("tiny")))
    monkeypatch.setattr(CT.TextConfig, "named", staticmethod(lambda name, _orig=CT.TextConfig.named: _orig("tiny")))
    monkeypatch.chdir(tmp_path)
    monkeypatch.syspath_prepend(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    pg = importlib.import_module("pipeline.policy_gradient")
    flags = ["--dataset", "a-animals", "--resolution", "64", "--n_inference_steps", "4", "--sample_batch_size", "2", "--train_batch_size", "1",
             "--train_accumulation_steps", "2", "--num_train_epochs", "1", "--save_freq", "1", "--per_prompt_stats_min_count", "2",
             "--learning_rate", "0"]
    runs = {f: pg.main(flags + ["--filter_field", f, "--logbase", str(tmp_path / f)]) for f in ("thumbnail", "thumbnail_device")}
    load = lambda f, what: np.load(os.path.join(runs[f]["localpath"], f"{what}/0_0.npy"), allow_pickle=True)
    r_host, r_dev = load("thumbnail", "rewards"), load("thumbnail_device", "rewards")
    assert r_dev.shape == (2,) and r_dev.dtype == r_host.dtype == np.float32 and np.array_equal(r_dev, r_host)
    assert np.isfinite(r_dev).all() and (r_dev <= 0).all()
    assert runs["thumbnail_device"]["mean_rewards"] == runs["thumbnail"]["mean_rewards"]
    for f in runs:
        assert load(f, "callback_info").item()["synthetic_weights"].all()
