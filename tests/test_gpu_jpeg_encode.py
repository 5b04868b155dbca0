"""The JPEG file writer on the GPU (csrc/jpeg_size.hip: the counter's kernels + jq_pack) against PIL called here and against the serial host entry —
bytes, no tolerance — and what is built on it: JpegEncoder, the llava_bertscore_device / llava_vqa_device rewards, the entrypoint.  Every file buffer
is pre-filled with 0xA5 and read back whole, so a byte written where none belongs shows as a wrong byte, not as a fault."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from _jpeg_cases import RECIPES, make_image, to_u8
from _llava_cases import fixture_images, same_result, scripted_post
from ddpo_amd import lib as L
from ddpo_amd.training import callbacks as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [(16, 16), (48, 32), (64, 64)]
QUALITIES = [25, 50, 80, 95, 100]
FILL = 0xA5


def _pil(img, q):
    return bytes(C.encode_jpeg(img, quality=q))


def _as_float(img):
    """float32 whose reference truncation gives back the uint8 image ((k + 0.5) / 255 sits half a level away from both neighbours)."""
    return img if img.dtype == np.float32 else np.minimum((img.astype(np.float32) + np.float32(0.5)) / np.float32(255), np.float32(1))


def _encode(x, q, stride=None, spare=1):
    """L.jpeg_encode into rows of a pre-filled buffer that is `spare` rows longer -> (the whole buffer on the host as (N + spare, stride), lengths)"""
    n, h, w, _ = x.shape
    stride = h * w * 3 + L.JPEG_FIXED_BYTES if stride is None else stride
    whole = torch.full(((n + spare) * stride,), FILL, dtype=torch.uint8, device="cuda")
    rows = whole[:n * stride].view(n, stride)
    files, lengths = L.jpeg_encode(x, q, files=rows)
    assert files.data_ptr() == whole.data_ptr() and lengths.dtype == torch.int64 and lengths.is_cuda
    return whole.cpu().numpy().reshape(n + spare, stride), lengths.tolist()


def _check_rows(buf, lengths, want, tag):
    """every row: the file's first min(length, stride) bytes, then the fill; the spare rows: the fill"""
    stride = buf.shape[1]
    assert lengths == [len(f) for f in want], tag
    for i, f in enumerate(want):
        k = min(len(f), stride)
        assert buf[i, :k].tobytes() == f[:k], (tag, i)
        assert (buf[i, k:] == FILL).all(), (tag, i, "bytes past the file were written")
    assert (buf[len(want):] == FILL).all(), (tag, "the row after the last one was written")


@pytest.mark.parametrize("h,w", SMALL)
def test_kernel_files_equal_pil_and_the_host_entry(h, w):
    imgs = [make_image(r, 100 + i, h, w) for i, r in enumerate(RECIPES)]
    u8_host = np.stack([to_u8(im) for im in imgs])
    u8 = torch.from_numpy(u8_host).cuda()
    f32 = torch.from_numpy(np.stack([_as_float(im) for im in imgs])).cuda()
    assert np.array_equal((f32.cpu().numpy() * 255).astype(np.uint8), u8_host)
    for q in QUALITIES:
        want = [_pil(im, q) for im in imgs]
        assert L.jpeg_encode_host(u8_host, q) == want
        for x, tag in ((u8, "uint8"), (f32, "float32")):
            buf, lengths = _encode(x, q)
            _check_rows(buf, lengths, want, (h, w, q, tag))
            assert L.jpeg_size(x, q).tolist() == lengths


def test_several_passes_and_the_padded_last_byte():
    """128 x 96 noise and checkerboard at 95 and 100: scans of about 25 kB, several passes of the pack loop; and the 800-byte file whose padded last
    byte becomes 0xFF (it ends FF 00 FF D9)."""
    imgs = [make_image("noise", 100, 128, 96), make_image("checker", 103, 128, 96)]
    x = torch.from_numpy(np.stack(imgs)).cuda()
    for q in (95, 100):
        want = [_pil(im, q) for im in imgs]
        assert max(len(f) for f in want) - L.JPEG_FIXED_BYTES > 3 * 4096
        buf, lengths = _encode(x, q)
        _check_rows(buf, lengths, want, ("128x96", q))
        assert L.jpeg_size(x, q).tolist() == lengths
    img = make_image("noise", 1, 16, 16)
    want = _pil(img, 80)
    assert len(want) == 800 and want[-4:] == b"\xff\x00\xff\xd9"
    for x in (torch.from_numpy(img[None]).cuda(), torch.from_numpy(_as_float(img)[None]).cuda()):
        buf, lengths = _encode(x, 80)
        _check_rows(buf, lengths, [want], "padded 0xFF")


def test_images_of_a_batch_do_not_see_each_other():
    recipes = ["noise", "const", "sparse", "checker", "smooth"]
    imgs = [to_u8(make_image(r, 40 + i, 64, 64)) for i, r in enumerate(recipes)]
    want = [_pil(im, 95) for im in imgs]
    buf, lengths = _encode(torch.from_numpy(np.stack(imgs)).cuda(), 95)
    _check_rows(buf, lengths, want, "batch")                               # the fill between the files survives
    for im, f in zip(imgs, want):
        alone, n = _encode(torch.from_numpy(im[None]).cuda(), 95)
        _check_rows(alone, n, [f], "alone")


@pytest.mark.parametrize("case", [("noise", 100, 48, 32, 95), ("noise", 1, 16, 16, 80), ("checker", 103, 128, 96, 100)])
def test_stride_rules_on_the_device(case):
    img = to_u8(make_image(*case[:4]))
    want, q = _pil(img, case[4]), case[4]
    x = torch.from_numpy(img[None]).cuda()
    for stride in (len(want), len(want) - 1, L.JPEG_FIXED_BYTES, len(want) + 3):
        buf, lengths = _encode(x, q, stride=stride, spare=2)
        _check_rows(buf, lengths, [want], (case, stride))
    # two files of different lengths in rows of the shorter one's length, at an odd stride: row 1 keeps a prefix and ends where row 2 would begin
    other = to_u8(make_image("smooth", 101, *case[2:4]))
    short = _pil(other, q)
    assert len(short) < len(want)
    buf, lengths = _encode(torch.from_numpy(np.stack([other, img, other])).cuda(), q, stride=len(short) | 1)
    _check_rows(buf, lengths, [short, want, short], (case, "batch"))
    with pytest.raises(ValueError, match="stride"):
        L.jpeg_encode(x, q, stride=L.JPEG_FIXED_BYTES - 1)


def test_512_pair_reaches_the_32_bit_offset_range():
    imgs = [make_image(r, 7, 512, 512) for r in ("noise", "smooth")]
    want = [_pil(im, 95) for im in imgs]
    assert (len(want[0]) - 625) * 8 > 2_000_000                            # megabits of scan data in the noise image
    for x in (torch.from_numpy(np.stack(imgs)).cuda(), torch.from_numpy(np.stack([_as_float(im) for im in imgs])).cuda()):
        files, lengths = L.jpeg_encode(x, 95)
        assert tuple(files.shape) == (2, 512 * 512 * 3 + 625) and lengths.tolist() == [len(f) for f in want]
        host = files.cpu().numpy()
        assert [host[i, :len(f)].tobytes() for i, f in enumerate(want)] == want


def test_two_encoders_on_two_streams_and_the_retry():
    from ddpo_amd.models.jpeg_encode import JpegEncoder
    a, b = JpegEncoder(quality=95), JpegEncoder(quality=95)
    assert a.stream != b.stream
    xa = torch.from_numpy(np.stack([make_image("noise", 60 + i, 64, 64) for i in range(4)])).cuda()
    xb = torch.from_numpy(np.stack([make_image("smooth", 70 + i, 64, 64) for i in range(4)])).cuda()
    want = [[_pil(im, 95) for im in x.cpu().numpy()] for x in (xa, xb)]
    torch.cuda.synchronize()
    got = []
    for s, x in ((a, xa), (b, xb)):                                        # back to back, nothing in between waits
        with torch.cuda.stream(s.stream):
            got.append(L.jpeg_encode(x, 95, workspace=s._workspace(*x.shape[:3]), files=s._files(4, 64 * 64 * 3 + 625)))
    torch.cuda.synchronize()
    assert a.workspace.data_ptr() != b.workspace.data_ptr() and a.files.data_ptr() != b.files.data_ptr()
    for (files, lengths), w in zip(got, want):
        host = files.cpu().numpy()
        assert lengths.tolist() == [len(f) for f in w] and [host[i, :len(f)].tobytes() for i, f in enumerate(w)] == w
    assert a(xa) == want[0] and b(xb.cpu().numpy()) == want[1] and a.retries == b.retries == 0
    assert a((xa.float() + 0.5) / 255) == want[0]
    small = JpegEncoder(quality=95, stride=1000)                           # the noise files are longer: rows of prefixes, then once more
    assert small(xa) == want[0] and small.retries == 1
    flat = np.full((2, 16, 16, 3), 77, np.uint8)                           # files of a few bytes of scan data: they fit, no second round
    assert small(torch.from_numpy(flat).cuda()) == [_pil(im, 95) for im in flat] and small.retries == 1
    with pytest.raises(ValueError, match="multiples of 16"):
        a(torch.zeros(1, 24, 40, 3, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="multiples of 16"):
        a(np.zeros((1, 24, 40, 3), np.float32))
    with pytest.raises(ValueError, match="quality"):
        JpegEncoder(quality=0)


def _run_llava(name, images, prompts, metadata, monkeypatch, device):
    import requests
    captured = []
    monkeypatch.setattr(requests.Session, "post", scripted_post(captured))
    fn = C.callback_fns[name + "_device" if device else name]()
    if device:
        out = C.evaluate_callbacks_device({name: fn}, torch.from_numpy(images).cuda(), prompts, metadata)[name]
    else:
        out = C.evaluate_callbacks({name: fn}, images, prompts, metadata)[name]
    return captured, out


@pytest.mark.parametrize("name", ["llava_bertscore", "llava_vqa"])
def test_device_callbacks_equal_the_host_callbacks(name, monkeypatch):
    images = np.concatenate([fixture_images(5, 12, 64), np.stack([_as_float(make_image(r, 80 + i, 64, 64)) for i, r in enumerate(RECIPES)])])
    prompts = [f"a cat doing thing {i}" for i in range(len(images))]
    metadata = [{"questions": ["what animal is this?", "what is it doing?"], "answers": ["Cat", "bike"]} for _ in images]
    req_host, out_host = _run_llava(name, images, prompts, metadata, monkeypatch, device=False)
    req_dev, out_dev = _run_llava(name, images, prompts, metadata, monkeypatch, device=True)
    assert req_dev == req_host and sum(len(r["images_len"]) for r in req_dev) == len(images)
    assert same_result(out_dev, out_host)
    assert len(set(np.asarray(out_host[0]).tolist())) > 1                  # the scripted scores do depend on the bytes


@pytest.mark.parametrize("name", ["llava_bertscore", "llava_vqa"])
def test_device_callbacks_send_the_reference_requests(name, monkeypatch):
    import PIL
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_host_logic.json")))
    if PIL.__version__ != gold["jpeg_rewards"]["pil_version"]:
        pytest.skip("JPEG bytes depend on the PIL build the fixture was produced with")
    ref = gold[name]
    images = fixture_images(ref["seed"], 20, ref["hw"])[:ref["n"]]
    captured, _ = _run_llava(name, images, ref.get("prompts", [""] * ref["n"]), ref.get("metadata"), monkeypatch, device=True)
    assert json.loads(json.dumps(captured)) == ref["requests"]


def test_entrypoint_with_llava_bertscore_device_equals_llava_bertscore(tmp_path, monkeypatch):
    """tests/test_gpu_entrypoint.py's llava-bertscore run (tiny model, 64 px, 4 steps, batch 2), one epoch, against a scripted server whose scores
    are a function of the bytes it receives: the files encoded on the device earn what PIL's earn."""
    import requests
    monkeypatch.setenv("DDPO_MODEL_CONFIG", "tiny")
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, ROOT)
    import importlib
    pg = importlib.import_module("pipeline.policy_gradient")
    flags = ["--dataset", "llava-bertscore", "--resolution", "64", "--n_inference_steps", "4", "--sample_batch_size", "2", "--train_batch_size", "1",
             "--train_accumulation_steps", "2", "--num_train_epochs", "1", "--save_freq", "1", "--per_prompt_stats_min_count", "2"]
    seen = {}
    for arm, extra in (("host", []), ("dev", ["--filter_field", "llava_bertscore_device"])):
        seen[arm] = []
        monkeypatch.setattr(requests.Session, "post", scripted_post(seen[arm]))
        seen[arm + "_out"] = pg.main(flags + extra + ["--logbase", str(tmp_path / arm)])
    host, dev = seen["host_out"], seen["dev_out"]
    assert seen["dev"] == seen["host"] and len(seen["host"]) >= 1
    r_host = np.load(os.path.join(host["localpath"], "rewards/0_0.npy"))
    r_dev = np.load(os.path.join(dev["localpath"], "rewards/0_0.npy"))
    assert r_dev.shape == (2,) and r_dev.dtype == r_host.dtype and np.array_equal(r_dev, r_host)
    assert dev["mean_rewards"] == host["mean_rewards"]
    with open(os.path.join(host["localpath"], "samples/0_0_0.png"), "rb") as f, open(os.path.join(dev["localpath"], "samples/0_0_0.png"), "rb") as g:
        assert f.read() == g.read()                                        # the inspection image is the same file
