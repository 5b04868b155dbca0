"""The symmetry kernels (csrc/symmetry.hip) against their serial host twins and against Pillow — integers and bytes, so `array_equal` and no
tolerance — and what is built on them: SymmetryStats, RotationalEmbedder and the four `*_device` rewards against their host twins.  The one
tolerance is mirror_corr's (exact sums against the reference's float32 sums): MIRROR_CORR_FACTOR times the deviation recorded in
tests/golden/reference_symmetry.json."""
import threading

import numpy as np
import pytest
import torch
from PIL import Image

import _symmetry_cases as SC
from ddpo_amd import lib as L
from ddpo_amd.models import clip_vision as CV
from ddpo_amd.models import symmetry as SY
from ddpo_amd.models.laion import synthetic_state_dicts
from ddpo_amd.training import callbacks as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
CORR_BOUND = SC.MIRROR_CORR_FACTOR * SC.load_golden()["mirror_corr_f32_dev"]
MODES = ("mirror", "rot180")


def _stats(x, mode):
    """lib.symmetry_stats into a destination pre-filled with -1: an unwritten sum shows up."""
    out = torch.full((x.shape[0], 4), -1, dtype=torch.int64, device=DEV)
    assert L.symmetry_stats(x, mode, out=out) is out
    return out.cpu().numpy()


def _misaligned(a):
    """The same values one element past an aligned base: the kernels' element-wise loads instead of the 4-element ones."""
    buf = torch.empty(a.size + 1, dtype=torch.from_numpy(a[:0]).dtype, device=DEV)
    buf[1:] = torch.from_numpy(a).to(DEV).reshape(-1)
    return buf[1:].view(a.shape)


@pytest.mark.parametrize("name", list(SC.CASES))
def test_stats_kernel_equals_host_twin(name):
    """1x1 and 3x5: a pixel, a centre column and a centre row that are their own partners, below one wave.  24x40: not square, rot180 pairs rows.
    7x520: a row of 1560 bytes, wider than the 256 lanes and no multiple of 16; an odd H has a self-paired middle row.  all255: the sum of
    a^2 is 4.74e9, beyond 32 bits.  kinds64: five different images in one batch, among them a symmetric one (sum 0) and a constant one."""
    u8 = SC.images_u8(name)
    f32 = SC.as_float(u8)
    for mode in MODES:
        want = L.symmetry_stats_host(u8, mode)
        assert np.array_equal(want, SC.stats_numpy(u8, mode))
        for x in (u8, f32):
            assert np.array_equal(_stats(torch.from_numpy(x).to(DEV), mode), want), (mode, x.dtype)
            assert np.array_equal(_stats(_misaligned(x), mode), want), (mode, x.dtype, "misaligned")
        if len(u8) > 1:                                                             # one image of the batch alone
            assert np.array_equal(_stats(torch.from_numpy(f32).to(DEV)[1:2], mode), want[1:2]), mode
    if name == "all255":
        assert want[0, 2] == 160 * 152 * 3 * 255 * 255 > 2 ** 32
    if name == "kinds64":
        assert L.symmetry_stats_host(u8, "mirror")[2, 0] == 0 and want[3, 0] == 0


def test_more_rows_than_workgroups_per_image():
    """512 rows over 64 workgroups per image (8 rows each), 150 row pairs over 64 (3 each, the last workgroups idle)."""
    for shape in [(2, 512, 12), (1, 300, 8)]:
        u8 = np.random.default_rng(shape[1]).integers(0, 256, shape + (3,), dtype=np.uint8)
        for mode in MODES:
            assert np.array_equal(_stats(torch.from_numpy(u8).to(DEV), mode), L.symmetry_stats_host(u8, mode)), (shape, mode)


def test_arbitrary_floats_are_truncated_like_the_reference():
    x = np.random.default_rng(3).random((3, 20, 28, 3), dtype=np.float32)
    x[0, 0, 0] = (1.0, 0.0, np.float32(254.999) / np.float32(255))
    u8 = (x * 255).astype(np.uint8)
    assert (u8 != np.rint(x * 255)).any()
    for mode in MODES:
        assert np.array_equal(_stats(torch.from_numpy(x).to(DEV), mode), SC.stats_numpy(u8, mode))
    sq = np.ascontiguousarray(x[:, :, :20])
    assert np.array_equal(L.rotate4_u8(torch.from_numpy(sq).to(DEV)).cpu().numpy(), L.rotate4_u8_host((sq * 255).astype(np.uint8)))


@pytest.mark.parametrize("s,n", [(1, 1), (5, 1), (56, 1), (72, 3)])
def test_rotate4_equals_pillow(s, n):
    """72: two tiles a side, the second 8 wide — no multiple of a 32- or 64-wide tile."""
    u8 = np.random.default_rng(s).integers(0, 256, (n, s, s, 3), dtype=np.uint8)
    want = np.stack([np.array(Image.fromarray(u8[i]).rotate(90 * k)) for k in range(4) for i in range(n)])
    assert np.array_equal(L.rotate4_u8_host(u8), want)
    for x in (u8, SC.as_float(u8)):
        for t in (torch.from_numpy(x).to(DEV), _misaligned(x)):
            out = torch.full((4 * n, s, s, 3), 0xAB, dtype=torch.uint8, device=DEV)
            assert L.rotate4_u8(t, out=out) is out
            assert np.array_equal(out.cpu().numpy(), want), x.dtype


def test_wrapper_refusals():
    x = torch.zeros(2, 24, 40, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="square"):
        L.rotate4_u8(x)
    with pytest.raises(ValueError, match="contiguous"):
        L.symmetry_stats(x.permute(0, 2, 1, 3), "mirror")
    with pytest.raises(ValueError, match="dtype must be float32 or uint8"):
        L.symmetry_stats(x.double(), "mirror")
    with pytest.raises(ValueError, match="last dimension 3"):
        L.rotate4_u8(x[..., :2].contiguous())
    with pytest.raises(ValueError, match="empty batch"):
        L.symmetry_stats(x[:0], "rot180")
    with pytest.raises(ValueError, match="mode must be one of"):
        L.symmetry_stats(x, 1)
    with pytest.raises(L.DdpoHipError, match="workspace"):
        L.symmetry_stats(x, "mirror", workspace=torch.empty(8, dtype=torch.uint8, device=DEV))


# ------------------------------------------------------------------------------------------------ callbacks
def _both(name, images, **kw):
    """(host callback through evaluate_callbacks, device twin through evaluate_callbacks_device on the CUDA batch)"""
    n = len(images)
    host = C.evaluate_callbacks({name: C.callback_fns[name](**kw)}, images, ["p"] * n, ({},) * n)[name]
    fn = C.callback_fns[name + "_device"](**kw)
    assert fn.wants_device_images
    dev = C.evaluate_callbacks_device({name: fn}, torch.from_numpy(images).to(DEV), ["p"] * n, ({},) * n)[name]
    return host, dev


@pytest.mark.parametrize("case", ["kinds64", "24x40", "7x520"])
def test_pixel_rewards_on_device_images_equal_the_host_rewards(case):
    u8 = SC.images_u8(case)
    images = SC.as_float(u8)
    for name in ("mirror", "rotational_corr"):
        (want, want_info), (got, info) = _both(name, images)
        assert got.dtype == want.dtype == np.float64 and got.shape == want.shape == (len(u8),) and np.array_equal(got, want), name
        assert set(info) == set(want_info) == {"mse"} and np.array_equal(info["mse"], want_info["mse"]), name
    (want, _), (got, info) = _both("mirror_corr", images)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape and info == {}
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    err = np.abs(got[ok].astype(np.float64) - want[ok])
    print(f"\n[mirror_corr {case}] max |device - host| = {err.max():.3e}, bound {CORR_BOUND:.3e}")
    assert (err <= CORR_BOUND).all()                                                           # the independent check: the float32 host value
    # consistency only: the twin's own formula restated in _symmetry_cases on numpy sums — shows the device sums reach the score unrounded
    assert np.array_equal(got[ok], SC.exact_mirror_corr(u8)[ok].astype(np.float32))
    if case == "kinds64":
        assert np.isnan(got[3]) and got[2] == -1                                               # constant; symmetric


def _embedder(monkeypatch, datapath, seed=5):
    monkeypatch.setattr(L, "DATAPATH", datapath)
    cfg = CV.VisionConfig.named("tiny")
    return SY.RotationalEmbedder(config="tiny", clip_state=synthetic_state_dicts(cfg, cfg.proj, seed)[0], device=DEV)


@pytest.mark.parametrize("datapath", ["fp32", "bf16x3"])
def test_rotational_on_device_images_equals_host_images(datapath, monkeypatch):
    emb = _embedder(monkeypatch, datapath)
    for s in (56, 112):                                                             # no resample; a 2x downscale
        images = np.random.default_rng(s).random((3, s, s, 3), dtype=np.float32)
        images[2] = np.clip(images[2] * 0.2 + np.linspace(0, 0.8, s, dtype=np.float32)[None, :, None], 0, 1)
        feats = emb(images)
        assert feats.shape == (12, emb.cfg.proj) and feats.dtype == np.float32 and np.isfinite(feats).all()
        assert np.array_equal(emb(torch.from_numpy(images).to(DEV)), feats)
        (want, want_info), (got, info) = _both("rotational", images, embedder=emb)
        assert got.dtype == want.dtype == np.float32 and got.shape == (3,) and np.array_equal(got, want) and (got < 0).all()
        assert set(info) == set(want_info) and not info["synthetic_weights"]
    with pytest.raises(ValueError, match="square"):
        emb(torch.zeros(1, 56, 84, 3, device=DEV))


def test_device_rewards_from_a_worker_thread_while_the_main_stream_is_busy(monkeypatch):
    """The entrypoint's arrangement: the producer records `ready` on its stream, a worker thread evaluates the rewards on their own streams, the
    main thread keeps its stream busy meanwhile."""
    emb = _embedder(monkeypatch, "bf16x3")
    fns = {"mirror_device": C.callback_fns["mirror_device"](), "rotational_corr_device": C.callback_fns["rotational_corr_device"](),
           "mirror_corr_device": C.callback_fns["mirror_corr_device"](), "rotational_device": C.callback_fns["rotational_device"](embedder=emb)}
    host = np.random.default_rng(11).random((4, 56, 56, 3), dtype=np.float32)
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
    for k in fns:
        assert np.array_equal(out["r"][k][0], want[k][0], equal_nan=True), k


def test_entrypoint_with_mirror_device_equals_mirror(tmp_path, monkeypatch):
    """tests/test_gpu_entrypoint.py's run (tiny model, 64 px, 4 steps, batch 2), one epoch, learning rate 0: the reward computed from the decoder's
    device tensor is the reward computed from the host copy, and `rotational_device` runs from the same tensor on a synthetic tiny tower."""
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
    runs = {f: pg.main(flags + ["--filter_field", f, "--logbase", str(tmp_path / f)]) for f in ("mirror", "mirror_device", "rotational_device")}
    load = lambda f, what: np.load(os.path.join(runs[f]["localpath"], f"{what}/0_0.npy"), allow_pickle=True)
    r_host, r_dev = load("mirror", "rewards"), load("mirror_device", "rewards")
    assert r_dev.shape == (2,) and r_dev.dtype == r_host.dtype == np.float64 and np.array_equal(r_dev, r_host) and (r_dev < 0).all()
    assert np.array_equal(load("mirror_device", "callback_info").item()["mse"], load("mirror", "callback_info").item()["mse"])
    assert runs["mirror_device"]["mean_rewards"] == runs["mirror"]["mean_rewards"]
    r_rot = load("rotational_device", "rewards")
    assert r_rot.shape == (2,) and r_rot.dtype == np.float32 and np.isfinite(r_rot).all() and (r_rot <= 0).all()
    assert load("rotational_device", "callback_info").item()["synthetic_weights"].all()
