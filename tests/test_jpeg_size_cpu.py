"""The JPEG byte counter without a GPU: the serial host entry `ddpo_jpeg_size_host` — the very functions the kernels of csrc/jpeg_size.hip run
(csrc/jpeg_size_core.h) — against PIL, called here, on integers, with no tolerance.  PIL's own stream is parsed so that the cases provably
contain what makes a byte count hard: stuffed 0xFF bytes, ZRL symbols, a padded last byte."""
import ctypes
import os
import re

import numpy as np
import pytest

from _jpeg_cases import RECIPES, load_golden, make_image, parse_jpeg, to_u8
from ddpo_amd import lib as L
from ddpo_amd.training import callbacks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(16, 16), (16, 32), (48, 32), (64, 64), (128, 96)]
QUALITIES = [25, 50, 80, 95, 100]
CASES = [(r, 100 + i, h, w) for h, w in SIZES for i, r in enumerate(RECIPES)]


@pytest.fixture(scope="module")
def pil_streams():
    """{(recipe, seed, h, w, q): (PIL's file length, facts parsed from PIL's file)} — encoded once for the whole module."""
    out = {}
    for r, s, h, w in CASES:
        img = make_image(r, s, h, w)
        for q in QUALITIES:
            data = C.encode_jpeg(img, quality=q)
            out[(r, s, h, w, q)] = (len(data), parse_jpeg(data))
    return out


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("recipe", RECIPES)
def test_host_entry_equals_pil(recipe, h, w, pil_streams):
    seed = 100 + RECIPES.index(recipe)
    u8 = to_u8(make_image(recipe, seed, h, w))
    for q in QUALITIES:
        got = int(L.jpeg_size_host(u8[None], q)[0])
        assert got == pil_streams[(recipe, seed, h, w, q)][0], (recipe, h, w, q)


def test_host_entry_takes_a_batch():
    ims = np.stack([to_u8(make_image(r, 5, 48, 32)) for r in RECIPES])
    got = L.jpeg_size_host(ims, 95)
    assert got.dtype == np.int64 and got.tolist() == [len(C.encode_jpeg(im, quality=95)) for im in ims]


def test_host_entry_equals_the_recorded_counts():
    """The golden file was written from PIL where the project is developed: a PIL with another libjpeg shows up as live != recorded."""
    gold = load_golden()
    small = [(k, v) for k, v in gold.items() if k[2] * k[3] <= 64 * 64]
    assert len(small) >= 90
    for (r, s, h, w, q), want in small:
        img = make_image(r, s, h, w)
        assert int(L.jpeg_size_host(to_u8(img)[None], q)[0]) == want == len(C.encode_jpeg(img, quality=q)), (r, s, h, w, q)


def test_cases_are_not_vacuous(pil_streams):
    facts = [f for _, f in pil_streams.values()]
    assert any(f["stuffed"] >= 1 for f in facts)
    assert any(f["zrl"] >= 1 for f in facts)
    assert any(f["bits"] % 8 != 0 for f in facts)
    assert any(f["max_ac_size"] == 10 for f in facts)                      # the top AC size category (checkerboard at quality 100)
    assert any(f["eob"] == 6 * (h // 16) * (w // 16) and f["max_ac_size"] == 0 for (r, s, h, w, q), (_, f) in pil_streams.items() if r == "const")
    ulp = make_image("ulp", 1, 16, 16)
    assert (to_u8(ulp) != np.rint(ulp * 255)).any()                       # truncation and rounding differ on the float recipe


def test_format_facts_and_the_fixed_byte_constant(pil_streams):
    hdr = open(os.path.join(ROOT, "include", "ddpo_hip.h")).read()
    fixed = int(re.search(r"#define\s+DDPO_JPEG_FIXED_BYTES\s+(\d+)", hdr).group(1))
    assert fixed == L.JPEG_FIXED_BYTES
    for key, (n, f) in pil_streams.items():
        assert f["header_bytes"] + 2 == fixed, key
        assert f["sampling"] == (0x22, 0x11, 0x11) and f["dht_lengths"] == [33, 183, 33, 183] and f["scans"] == 1 and f["restart_markers"] == 0
        assert f["pad_ok"]
        assert n == fixed + (f["bits"] + 7) // 8 + f["stuffed"], key


def test_callback_contract():
    assert "jpeg_device" in C.callback_fns and "neg_jpeg_device" in C.callback_fns
    from ddpo_amd import training
    assert training.evaluate_callbacks_device is C.evaluate_callbacks_device
    host_fn = C.jpeg_fn()
    assert not getattr(host_fn, "wants_device_images", False)
    with pytest.raises(ValueError, match="do not take device images"):
        C.evaluate_callbacks_device({"jpeg": host_fn}, None, ["a"], None)


def test_sizes_off_the_mcu_grid_are_refused():
    bad = np.zeros((1, 24, 40, 3), np.uint8)
    with pytest.raises(ValueError, match="multiples of 16"):
        L.jpeg_size_host(bad, 95)
    with pytest.raises(ValueError, match="multiples of 16"):
        L.jpeg_size_workspace_bytes(1, 24, 40)
    lib = L.load()
    out = np.zeros(1, np.int64)
    assert lib.ddpo_jpeg_size_host(bad.ctypes.data_as(ctypes.c_void_p), 1, 24, 40, 95, out.ctypes.data_as(ctypes.c_void_p)) == -1
    nb = ctypes.c_size_t(0)
    assert lib.ddpo_jpeg_size_workspace_bytes(1, 24, 40, ctypes.byref(nb)) == -1
    assert lib.ddpo_jpeg_size(None, 0, 1, 24, 40, 95, None, 0, None, None) == -1
    ok = np.zeros((1, 16, 16, 3), np.uint8)
    for q in (0, 101):
        assert lib.ddpo_jpeg_size_host(ok.ctypes.data_as(ctypes.c_void_p), 1, 16, 16, q, out.ctypes.data_as(ctypes.c_void_p)) == -1
        with pytest.raises(ValueError, match="quality"):
            L.jpeg_size_host(ok, q)
