"""CLIP preprocessing on the GPU (csrc/clip_preprocess.hip) against its serial host twin and against `clip_vision.preprocess` (Pillow called here) —
bit for bit, no tolerance — and what is built on it: the device-tensor paths of AestheticScorer / ClipScorer, the aesthetic_device /
clip_score_device rewards, up to the entrypoint."""
import os
import sys

import numpy as np
import pytest
import torch

from _clip_cases import CASES, KINDS, LARGE, PATCH, as_float, im2col, k_pad, make_image, seed_of
from ddpo_amd import lib as L
from ddpo_amd.models import clip_score as CS
from ddpo_amd.models import clip_text as CT
from ddpo_amd.models import clip_vision as CV
from ddpo_amd.models.laion import AestheticScorer, synthetic_state_dicts
from ddpo_amd.training import callbacks as C
from oracle import clip_vision as OC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
KP = k_pad()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _device(x, size):
    """lib.clip_preprocess into a destination pre-filled with NaN: an unwritten pad column or row shows up."""
    g = size // PATCH
    out = torch.full((x.shape[0] * g * g, KP), float("nan"), dtype=torch.float32, device=DEV)
    assert L.clip_preprocess(x, size, PATCH, KP, out=out) is out
    return out


@pytest.mark.parametrize("hw,size", CASES, ids=[f"{h}x{w}-{s}" for (h, w), s in CASES])
def test_kernel_equals_host_twin_and_preprocess(hw, size):
    h, w = hw
    kinds = ("noise",) if (hw, size) in LARGE else KINDS                         # 3 different images per batch at the small sizes
    u8 = np.stack([make_image(k, seed_of(k, h, w), h, w) for k in kinds])
    f32 = as_float(u8)
    assert np.array_equal((f32 * 255).astype(np.uint8), u8)
    host = L.clip_preprocess_host(u8, size, PATCH, KP)
    want = im2col(CV.preprocess(u8, size))
    assert np.array_equal(host.view(np.uint32), want.view(np.uint32))
    want = torch.from_numpy(want).to(DEV)
    gg = (size // PATCH) ** 2
    for x in (torch.from_numpy(u8).to(DEV), torch.from_numpy(f32).to(DEV)):
        got = _device(x, size)
        assert _same_bits(got, want), str(x.dtype)
        assert not got[:, 3 * PATCH * PATCH:].view(torch.int32).any()              # pad columns: +0, every bit
        for i in range(len(kinds)):                                                # each image of the batch alone (a view: another base alignment)
            assert _same_bits(_device(x[i:i + 1], size), want[i * gg:(i + 1) * gg]), (str(x.dtype), i)


def test_arbitrary_floats_are_truncated_like_the_reference():
    x = np.random.default_rng(3).random((3, 40, 56, 3), dtype=np.float32)
    x[0, 0, 0] = (1.0, 0.0, np.float32(254.999) / np.float32(255))
    assert ((x * 255).astype(np.uint8) != np.rint(x * 255)).any()
    want = torch.from_numpy(im2col(CV.preprocess(x, 28))).to(DEV)
    assert _same_bits(_device(torch.from_numpy(x).to(DEV), 28), want)


def test_wrapper_refusals():
    x = torch.zeros(1, 64, 64, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="not a multiple of patch"):
        L.clip_preprocess(x, 50, PATCH, KP)
    with pytest.raises(ValueError, match="at least 3 \\* patch \\* patch"):
        L.clip_preprocess(x, 56, PATCH, 3 * PATCH * PATCH - 4)
    with pytest.raises(ValueError, match="must fit the 160 KB of LDS"):
        L.clip_preprocess(torch.zeros(1, 2400, 2400, 3, dtype=torch.uint8, device=DEV), 56, PATCH, KP)
    with pytest.raises(ValueError, match="N x H x W x 3"):
        L.clip_preprocess(x[..., :2].contiguous(), 56, PATCH, KP)
    wide = torch.full(((56 // PATCH) ** 2, 2 * KP), 7.0, dtype=torch.float32, device=DEV)
    with pytest.raises(L.DdpoHipError, match="out must be"):             # the right shape, but rows 2 KP apart: the kernel strides by KP
        L.clip_preprocess(x, 56, PATCH, KP, out=wide[:, :KP])
    torch.cuda.synchronize()
    assert bool((wide == 7.0).all())                                       # nothing was launched


# ------------------------------------------------------------------------------------------------ scorers
def _aesthetic(datapath="bf16x3", seed=4):
    """Tiny tower on seeded synthetic states, as tests/test_gpu_aesthetic.py:_setup."""
    L.DATAPATH = datapath
    params = OC.init_params(OC.vision_param_shapes(OC.VIT_TINY), seed=seed)
    mlp = OC.init_params(OC.mlp_param_shapes(OC.VIT_TINY.proj), seed=seed + 1)
    mlp["layers.7.bias"] = mlp["layers.7.bias"] + 5.0
    return AestheticScorer(config="tiny", clip_state=params, mlp_state=mlp, device=DEV)


def _images(seed, n, h, w):
    x = np.random.default_rng(seed).random((n, h, w, 3), dtype=np.float32)
    x[-1] = np.clip(x[-1] * 0.2 + np.linspace(0, 0.8, w, dtype=np.float32)[None, :, None], 0, 1)          # a smooth image as well as noise
    return x


@pytest.mark.parametrize("datapath", ["fp32", "bf16x3"])
def test_aesthetic_scorer_on_device_images_equals_host_images(datapath):
    scorer = _aesthetic(datapath)
    for shape in [(5, 80, 64), (2, 56, 56), (3, 32, 48)]:
        x = _images(3, *shape)
        want = scorer(x)
        got = scorer(torch.from_numpy(x).to(DEV))
        assert got.dtype == np.float32 and got.shape == (shape[0],) and np.array_equal(got, want), shape
    u8 = (x * 255).astype(np.uint8)
    assert np.array_equal(scorer(torch.from_numpy(u8).to(DEV)), want)
    with pytest.raises(ValueError, match="CUDA tensor"):
        scorer(torch.from_numpy(x))
    with pytest.raises(ValueError, match="contiguous"):
        scorer(torch.from_numpy(x).to(DEV).permute(0, 2, 1, 3))


def _clip_scorer(datapath, seed=12):
    L.DATAPATH = datapath
    vcfg, tcfg = CV.VisionConfig.named("tiny"), CT.TextConfig.named("tiny")
    sd, _ = synthetic_state_dicts(vcfg, vcfg.proj, seed)
    sd.update(CT.synthetic_text_state(tcfg, seed))
    sd["logit_scale"] = torch.tensor(CS.SYNTHETIC_LOGIT_SCALE)
    return CS.ClipScorer(config="tiny", clip_state=sd, device=DEV)


@pytest.mark.parametrize("datapath", ["fp32", "bf16x3"])
def test_clip_scorer_on_device_images_equals_host_images(datapath):
    scorer = _clip_scorer(datapath)
    prompts = ["a dog", "a cat riding a bike", "", "a dog", "a llama playing chess", "x" * 120]
    assert len(prompts) % CS.IMAGE_CHUNK and len(prompts) > CS.IMAGE_CHUNK         # a full chunk and a padded one
    x = _images(8, len(prompts), 64, 80)
    want, want_cos = scorer(x, prompts, return_cosine=True)
    got, got_cos = scorer(torch.from_numpy(x).to(DEV), prompts, return_cosine=True)
    assert np.array_equal(got, want) and np.array_equal(got_cos, want_cos) and np.isfinite(got).all()
    assert np.array_equal(scorer(torch.from_numpy(x[:3]).to(DEV), prompts[:3]), want[:3])      # chunked scores do not depend on the batch
    assert np.array_equal(scorer(torch.from_numpy(x[:4]).to(DEV), prompts[:4]), want[:4])


def test_vit_l14_geometry_patches_feed_the_tower():
    """224 / 14 / 608 columns / 257 tokens / 16 heads of 64 from 512 x 512 images, two layers deep: the embeddings from the kernel's patch matrix
    equal those from preprocess + the tower's own im2col."""
    L.DATAPATH = "bf16x3"
    cfg = CV.VisionConfig(layers=2)
    assert (cfg.image, cfg.patch, cfg.k_pad, cfg.tokens) == (224, 14, 608, 257)
    tower = CV.ClipVisionTower(cfg, DEV)
    tower.load_state_dict(synthetic_state_dicts(cfg, cfg.proj, 7)[0])
    x = _images(5, 2, 512, 512)
    want = tower(torch.from_numpy(CV.preprocess(x, 224)).to(DEV))
    got = tower.forward_patches(L.clip_preprocess(torch.from_numpy(x).to(DEV), 224, 14, cfg.k_pad))
    assert got.shape == (2, cfg.proj) and torch.isfinite(got).all() and torch.equal(got, want)


def test_two_scorers_on_two_streams():
    a, b = _aesthetic(), _aesthetic()
    assert a.stream != b.stream
    xa, xb = torch.from_numpy(_images(60, 4, 64, 64)).to(DEV), torch.from_numpy(_images(70, 4, 80, 48)).to(DEV)
    torch.cuda.synchronize()
    got = []
    for s, x in ((a, xa), (b, xb)):                                                # back to back, nothing in between waits
        with torch.cuda.stream(s.stream):
            got.append(s.tower.forward_patches(L.clip_preprocess(x, 56, PATCH, KP)))
    torch.cuda.synchronize()
    for s, x, g in ((a, xa, got[0]), (b, xb, got[1])):
        with torch.cuda.stream(s.stream):
            want = s.features(torch.from_numpy(CV.preprocess(x.cpu().numpy(), 56)).to(DEV))
        s.stream.synchronize()
        assert torch.equal(g, want)
    assert np.array_equal(a(xa), a(xa.cpu().numpy())) and np.array_equal(b(xb.cpu().numpy()), b(xb))
    # an event recorded by the producer is what the scorer's stream waits for
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        y = xa * 0.5
        ready = side.record_event()
    assert np.array_equal(a(y, ready=ready), a(y.cpu().numpy()))


# ------------------------------------------------------------------------------------------------ callbacks, entrypoint
def _tiny_towers(monkeypatch):
    monkeypatch.setenv("DDPO_ALLOW_SYNTHETIC", "1")
    monkeypatch.setattr(CV.VisionConfig, "named", staticmethod(lambda name, _orig=CV.VisionConfig.named: _orig("tiny")))   # seconds, not minutes
    monkeypatch.setattr(CT.TextConfig, "named", staticmethod(lambda name, _orig=CT.TextConfig.named: _orig("tiny")))


def test_device_callbacks_equal_the_host_callbacks(monkeypatch):
    _tiny_towers(monkeypatch)
    L.DATAPATH = "bf16x3"
    imgs = _images(9, 5, 64, 64)
    prompts = ["a dog", "a cat", "a dog", "", "a bear washing the dishes"]
    for name in ("aesthetic", "clip_score"):
        want, want_info = C.evaluate_callbacks({name: C.callback_fns[name]()}, imgs, prompts, ({},) * 5)[name]
        fn = C.callback_fns[name + "_device"]()
        assert fn.wants_device_images
        got_np, info_np = C.evaluate_callbacks({name: fn}, imgs, prompts, ({},) * 5)[name]
        got_dev, info_dev = C.evaluate_callbacks_device({name: fn}, torch.from_numpy(imgs).to(DEV), prompts, ({},) * 5)[name]
        for got, info in ((got_np, info_np), (got_dev, info_dev)):
            assert got.dtype == want.dtype and got.shape == want.shape == (5, 1) and np.array_equal(got, want), name
            assert set(info) == set(want_info) and all(np.array_equal(info[k], want_info[k]) for k in info), name


def test_entrypoint_with_aesthetic_device_equals_aesthetic(tmp_path, monkeypatch):
    """tests/test_gpu_entrypoint.py's run (tiny model, 64 px, 4 steps, batch 2) with the tiny vision tower, two epochs: the reward computed from
    the decoder's device tensor gives the same mean rewards as the reward computed from the host copy.

    The learning rate is 0.  Two runs of this entrypoint do not reach epoch 1 with the same weights whatever the reward: the weight gradients are
    summed with fp32 atomics (test_entrypoint_resume_continues_the_run compares its epoch-1 rewards with a tolerance for that reason).  Seen here
    with --learning_rate 1e-5, epoch 0 equal in every bit and epoch 1 -0.0615919 (aesthetic) against -0.0616726 (aesthetic_device).  With the
    update switched off both epochs sample from the same weights — with different prompts and noise — and the comparison stays exact."""
    monkeypatch.setenv("DDPO_MODEL_CONFIG", "tiny")
    _tiny_towers(monkeypatch)
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, ROOT)
    import importlib
    pg = importlib.import_module("pipeline.policy_gradient")
    flags = ["--dataset", "a-animals", "--resolution", "64", "--n_inference_steps", "4", "--sample_batch_size", "2", "--train_batch_size", "1",
             "--train_accumulation_steps", "2", "--num_train_epochs", "2", "--save_freq", "1", "--per_prompt_stats_min_count", "2",
             "--learning_rate", "0"]
    host = pg.main(flags + ["--filter_field", "aesthetic", "--logbase", str(tmp_path / "host")])
    dev = pg.main(flags + ["--filter_field", "aesthetic_device", "--logbase", str(tmp_path / "dev")])
    print(f"\n[entrypoint] mean rewards host {host['mean_rewards']}  device {dev['mean_rewards']}")
    r_host = np.load(os.path.join(host["localpath"], "rewards/0_0.npy"))
    r_dev = np.load(os.path.join(dev["localpath"], "rewards/0_0.npy"))
    assert r_dev.shape == (2, 1) and r_dev.dtype == r_host.dtype and np.array_equal(r_dev, r_host)
    assert len(dev["mean_rewards"]) == 2 and dev["mean_rewards"] == host["mean_rewards"]
    r1_host, r1_dev = (np.load(os.path.join(o["localpath"], "rewards/0_1.npy")) for o in (host, dev))
    assert np.array_equal(r1_dev, r1_host) and not np.array_equal(r1_dev, r_dev)                # a second, different batch
    with open(os.path.join(host["localpath"], "samples/0_0_0.png"), "rb") as f, open(os.path.join(dev["localpath"], "samples/0_0_0.png"), "rb") as g:
        assert f.read() == g.read()                                                # the inspection image is the same file
