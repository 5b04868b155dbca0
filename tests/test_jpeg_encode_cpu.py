"""The JPEG file writer without a GPU: the serial host entry `ddpo_jpeg_encode_host` — the very functions the pack kernel of csrc/jpeg_size.hip
runs (csrc/jpeg_size_core.h: the header bytes, the byte-stuffing step) — against PIL, called here, on bytes, with no tolerance.  PIL's own files are
parsed so that the cases provably contain what makes packing hard: stuffed bytes, a 0xFF in the last byte of a word, streams that end on a byte
boundary and streams that do not, scans of several passes, a padded last byte that becomes 0xFF."""
import ctypes
import io
import os
import re

import numpy as np
import pytest
from PIL import Image

from _jpeg_cases import RECIPES, make_image, parse_jpeg, to_u8
from _llava_cases import fixture_images, same_result, scripted_post
from ddpo_amd import lib as L
from ddpo_amd.training import callbacks as C

SIZES = [(16, 16), (16, 32), (48, 32), (64, 64), (128, 96)]
QUALITIES = [25, 50, 80, 95, 100]
CASES = [(r, 100 + i, h, w, q) for h, w in SIZES for i, r in enumerate(RECIPES) for q in QUALITIES]
CASES += [(r, 100 + i, 48, 32, q) for i, r in enumerate(RECIPES) for q in (1, 5)]          # quantisation tables clamped at 255
PADDED_FF = ("noise", 1, 16, 16, 80)                                                     # 800 bytes, ends FF 00 FF D9
CASES += [PADDED_FF]
HEADER = 623


@pytest.fixture(scope="module")
def pil_files():
    """{case: PIL's file} — encoded once for the whole module."""
    return {c: bytes(C.encode_jpeg(make_image(*c[:4]), quality=c[4])) for c in CASES}


def _raw(lib, u8, q, buf, stride):
    """the C entry on a caller's buffer -> (return code, lengths)"""
    n, h, w, _ = u8.shape
    lengths = np.full(n, -7, np.int64)
    rc = lib.ddpo_jpeg_encode_host(u8.ctypes.data_as(ctypes.c_void_p), n, h, w, q, buf.ctypes.data_as(ctypes.c_void_p), stride,
                                   lengths.ctypes.data_as(ctypes.c_void_p))
    return rc, lengths


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("recipe", RECIPES)
def test_host_entry_equals_pil(recipe, h, w, pil_files):
    seed = 100 + RECIPES.index(recipe)
    u8 = to_u8(make_image(recipe, seed, h, w))
    for q in QUALITIES + ([1, 5] if (h, w) == (48, 32) else []):
        got = L.jpeg_encode_host(u8[None], q)
        assert len(got) == 1 and type(got[0]) is bytes
        assert got[0] == pil_files[(recipe, seed, h, w, q)], (recipe, h, w, q)
        assert len(got[0]) == int(L.jpeg_size_host(u8[None], q)[0])


def test_host_entry_takes_a_batch_and_the_named_case(pil_files):
    ims = np.stack([to_u8(make_image(r, 100 + i, 48, 32)) for i, r in enumerate(RECIPES)])
    got = L.jpeg_encode_host(ims, 80)
    assert got == [pil_files[(r, 100 + i, 48, 32, 80)] for i, r in enumerate(RECIPES)]
    assert [len(f) for f in got] == L.jpeg_size_host(ims, 80).tolist()
    want = pil_files[PADDED_FF]
    assert len(want) == 800 and want[-4:] == b"\xff\x00\xff\xd9"
    assert L.jpeg_encode_host(make_image(*PADDED_FF[:4])[None], 80) == [want]


def test_header_is_a_function_of_size_and_quality(pil_files):
    a, b = pil_files[("noise", 100, 64, 64, 80)], pil_files[("smooth", 101, 64, 64, 80)]
    assert a[:HEADER] == b[:HEADER] and a[HEADER:] != b[HEADER:]
    q1 = pil_files[("noise", 100, 48, 32, 1)]
    assert parse_jpeg(q1)["segments"] == [(0xE0, 16), (0xDB, 67), (0xDB, 67), (0xC0, 17), (0xC4, 31), (0xC4, 181), (0xC4, 31), (0xC4, 181), (0xDA, 12)]
    assert max(q1[25:89]) == 255 and max(q1[94:158]) == 255                  # 8-bit tables, clamped
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ddpo_hip.h")).read()
    assert int(re.search(r"#define\s+DDPO_JPEG_HEADER_BYTES\s+(\d+)", hdr).group(1)) == HEADER == L.JPEG_HEADER_BYTES == L.JPEG_FIXED_BYTES - 2


def test_cases_are_not_vacuous(pil_files):
    facts = {c: parse_jpeg(f) for c, f in pil_files.items()}
    assert all(f["header_bytes"] == HEADER for f in facts.values())
    raws = {c: f[HEADER:-2].replace(b"\xff\x00", b"\xff") for c, f in pil_files.items()}
    assert any(f["stuffed"] >= 1 for f in facts.values())
    assert any(any(i % 4 == 3 for i, b in enumerate(r) if b == 0xFF) for r in raws.values())      # the stuffed zero lands in the next word
    assert any(f["bits"] % 8 == 0 for f in facts.values()) and any(f["bits"] % 8 != 0 for f in facts.values())
    assert any(len(f) - HEADER - 2 > 4096 for f in pil_files.values())                             # more than one pass of a 1024-word pack loop
    assert any(f[-4:] == b"\xff\x00\xff\xd9" for c, f in pil_files.items() if c != PADDED_FF)
    assert pil_files[PADDED_FF][-4:] == b"\xff\x00\xff\xd9" and facts[PADDED_FF]["bits"] % 8 != 0


@pytest.mark.parametrize("case", [("noise", 100, 48, 32, 95), PADDED_FF, ("const", 102, 16, 16, 50)])
def test_stride_rules(case, pil_files):
    lib = L.load()
    want = pil_files[case]
    n = len(want)
    u8 = to_u8(make_image(*case[:4]))[None]
    q = case[4]
    # stride == length: the row is the file, the rest of the buffer is untouched
    buf = np.full(2 * n + 64, 0xA5, np.uint8)
    rc, lengths = _raw(lib, u8, q, buf, n)
    assert rc == 0 and lengths.tolist() == [n]
    assert buf[:n].tobytes() == want and (buf[n:] == 0xA5).all()
    # a longer row: bytes past the file are not written
    buf[:] = 0xA5
    rc, lengths = _raw(lib, u8, q, buf, n + 40)
    assert rc == 0 and lengths.tolist() == [n] and buf[:n].tobytes() == want and (buf[n:] == 0xA5).all()
    # shorter rows: the file's prefix, the full length reported, the next row untouched
    for stride in (n - 1, 625):
        buf[:] = 0xA5
        rc, lengths = _raw(lib, u8, q, buf, stride)
        assert rc == 0 and lengths.tolist() == [n], stride
        assert buf[:min(stride, n)].tobytes() == want[:stride] and (buf[min(stride, n):] == 0xA5).all(), stride


def test_stride_rules_in_a_batch(pil_files):
    """Two files of different lengths in rows of the shorter one's length: row 0 whole, row 1 a prefix, the third row untouched."""
    cases = [("smooth", 101, 48, 32, 95), ("noise", 100, 48, 32, 95)]
    want = [pil_files[c] for c in cases]
    stride = len(want[0])
    assert len(want[1]) > stride
    u8 = np.stack([to_u8(make_image(*c[:4])) for c in cases])
    buf = np.full(3 * stride, 0xA5, np.uint8)
    rc, lengths = _raw(L.load(), u8, 95, buf, stride)
    assert rc == 0 and lengths.tolist() == [len(w) for w in want]
    assert buf[:stride].tobytes() == want[0] and buf[stride:2 * stride].tobytes() == want[1][:stride] and (buf[2 * stride:] == 0xA5).all()


def test_refusals():
    lib = L.load()
    bad, ok = np.zeros((1, 24, 40, 3), np.uint8), np.zeros((1, 16, 16, 3), np.uint8)
    buf = np.full(4096, 0xA5, np.uint8)
    with pytest.raises(ValueError, match="multiples of 16"):
        L.jpeg_encode_host(bad, 80)
    with pytest.raises(ValueError, match="multiples of 16"):
        L.jpeg_encode_max_bytes(24, 40)
    with pytest.raises(ValueError):
        L.jpeg_encode_max_bytes(16, 65504)                                  # on the grid, above libjpeg's 65500
    assert _raw(lib, bad, 80, buf, 4096)[0] == -1
    nb = ctypes.c_size_t(0)
    assert lib.ddpo_jpeg_encode_max_bytes(24, 40, ctypes.byref(nb)) == -1
    assert lib.ddpo_jpeg_encode_max_bytes(16, 65504, ctypes.byref(nb)) == -1
    assert lib.ddpo_jpeg_encode_max_bytes(16, 16, None) == -1
    assert lib.ddpo_jpeg_encode_max_bytes(16, 16, ctypes.byref(nb)) == 0 and nb.value == 625 + 2 * (6 * 1664 // 8) == L.jpeg_encode_max_bytes(16, 16)
    for q in (0, 101):
        assert _raw(lib, ok, q, buf, 4096)[0] == -1
        with pytest.raises(ValueError, match="quality"):
            L.jpeg_encode_host(ok, q)
    assert _raw(lib, ok, 80, buf, 624)[0] == -1                             # a row too small for the fixed bytes
    assert _raw(lib, ok, 80, buf, 625)[0] == 0
    assert lib.ddpo_jpeg_encode_host(None, 1, 16, 16, 80, buf.ctypes.data_as(ctypes.c_void_p), 4096, None) == -1
    assert lib.ddpo_jpeg_encode(None, 0, 1, 16, 16, 80, None, 0, None, 4096, None, None) == -1
    with pytest.raises(ValueError, match="uint8"):
        L.jpeg_encode_host(np.zeros((1, 16, 16, 3), np.float32), 80)
    from ddpo_amd.models.jpeg_encode import JpegEncoder
    with pytest.raises(ValueError, match="stride"):
        JpegEncoder(stride=624)                                             # refused before anything touches a device
    with pytest.raises(ValueError, match="quality"):
        JpegEncoder(quality=101)


@pytest.mark.parametrize("case", [("noise", 100, 64, 64, 80), ("ulp", 105, 48, 32, 95), ("checker", 103, 128, 96, 100)])
def test_round_trip(case, pil_files):
    ours = L.jpeg_encode_host(to_u8(make_image(*case[:4]))[None], case[4])[0]
    im = Image.open(io.BytesIO(ours))
    im.load()
    assert im.size == (case[3], case[2]) and im.mode == "RGB"
    assert np.array_equal(np.asarray(im), np.asarray(Image.open(io.BytesIO(pil_files[case]))))


def test_registry_and_wire_format(monkeypatch):
    """The *_device callbacks given host arrays: the same requests, scores and info as the host callbacks (no socket, no GPU)."""
    import requests
    for name in ("llava_bertscore_device", "llava_vqa_device"):
        assert name in C.callback_fns
    assert not getattr(C.callback_fns["llava_bertscore"](), "wants_device_images", False)
    images = fixture_images(5, 20, 32)
    prompts = np.array([f"a cat doing thing {i}" for i in range(20)])
    metadata = [{"questions": ["what animal is this?", "what is it doing?"], "answers": ["Cat", "bike"]} for _ in range(20)]
    for name, args, sizes in (("llava_bertscore", (prompts, None), [10, 10]), ("llava_vqa", (None, metadata), [4, 4, 4, 4, 4])):
        results, requests_seen = [], []
        for key in (name, name + "_device"):
            captured = []
            monkeypatch.setattr(requests.Session, "post", scripted_post(captured))
            fn = C.callback_fns[key]()
            assert bool(getattr(fn, "wants_device_images", False)) == key.endswith("_device")
            results.append(fn(images, *args))
            requests_seen.append(captured)
        assert requests_seen[0] == requests_seen[1] and [len(r["images_len"]) for r in requests_seen[0]] == sizes
        assert same_result(results[0], results[1]) and len(results[0][0]) == 20
        assert len(set(results[0][0].tolist())) > 1                         # the scripted scores do depend on the bytes
