"""The thumbnail reward without a GPU: the serial host entry `ddpo_resize_u8_host` — the very functions the kernel of csrc/resize_u8.hip runs
(csrc/clip_preprocess_core.h) — against Pillow with no tolerance, the host callbacks against results recorded from the reference's own code
(tests/golden/reference_thumbnail.json), what the wrappers refuse, and the registry."""
import ctypes

import numpy as np
import pytest
from PIL import Image

import _thumbnail_cases as TC
from ddpo_amd import lib as L
from ddpo_amd.models import thumbnail as TH
from ddpo_amd.training import callbacks as C

GOLD = TC.load_golden()


def _pillow(u8, oh, ow):
    return np.stack([np.asarray(Image.fromarray(im).resize((ow, oh))) for im in u8])           # Pillow's default filter for RGB: bicubic


def _standin_embedder(images, ready=None):
    assert ready is None
    return TC.standin_features(TH.thumbnail_pixel_values(images, 224))


def _run(key, images, **kw):
    return C.evaluate_callbacks({key: C.callback_fns[key](**kw)}, images, ["a prompt"] * len(images), ({},) * len(images))[key]


def _ulps_f32(a, b):
    """distance in float32 units in the last place (both finite, same sign or zero)"""
    ia, ib = (np.abs(x.astype(np.float32)).view(np.int32).astype(np.int64) * np.where(np.signbit(x), -1, 1) for x in (a, b))
    return np.abs(ia - ib)


@pytest.mark.parametrize("shape,outs", TC.RESIZES, ids=[f"{h}x{w}" for (h, w), _ in TC.RESIZES])
def test_resize_host_equals_pillow(shape, outs):
    """16x16: the filter's support is wider than the image, down to one output pixel.  17x23 -> 4x5: odd sizes, a 15-byte output row.  24x40 ->
    24x10: the height keeps its size (identity table).  8x8 -> 20x12: an up-scale.  512x512: the sizes of the reward at the shipped resolution."""
    u8 = TC.resize_input(*shape, n=1 if shape[0] >= 512 else 2)
    for oh, ow in outs:
        want = _pillow(u8, oh, ow)
        assert np.array_equal(want, np.stack([np.asarray(Image.fromarray(im).resize((ow, oh), resample=Image.BICUBIC)) for im in u8]))
        for x in (u8, TC.as_float(u8)):
            got = L.resize_u8_host(x, oh, ow)
            assert got.dtype == np.uint8 and got.shape == (len(u8), oh, ow, 3) and np.array_equal(got, want), (oh, ow, x.dtype)


def test_floats_are_truncated_like_the_reference():
    x = np.random.default_rng(3).random((2, 32, 40, 3), dtype=np.float32)
    x[0, 0, 0] = (1.0, 0.0, np.float32(254.999) / np.float32(255))
    u8 = (x * 255).astype(np.uint8)
    assert (u8 != np.rint(x * 255)).any()
    assert np.array_equal(L.resize_u8_host(x, 8, 10), _pillow(u8, 8, 10))
    assert not np.array_equal(L.resize_u8_host(x, 8, 10), _pillow(np.rint(x * 255).astype(np.uint8), 8, 10))
    assert np.array_equal(L.resize_u8_host(x, 32, 40), u8)                                   # both axes keep their size: the truncated bytes


@pytest.mark.parametrize("name", list(TC.CASES))
def test_thumbnail_reproduces_the_reference_given_the_same_features(name):
    """The recording ran the reference's own wrapper around stand-in features (see tests/golden/make_reference_thumbnail_goldens.py); here the
    same stand-in sits behind the `embedder` seam, so the truncation, the thumbnail sizes and filter, the order of the blocks, the reshape and the
    angle arithmetic are what is compared.  Equal to the recording bit for bit under the numpy that made it (`numpy_version` in the fixture);
    only under another numpy, whose arccos may round differently, is 1 float32 ulp allowed — the rule of tests/test_symmetry_cpu.py for
    `rotational`."""
    u8 = TC.images_u8(name)
    images = TC.as_float(u8)
    rec = GOLD["cases"][name]
    assert list(u8.shape) == rec["shape"] and np.array_equal((images * 255).astype(np.uint8), u8)
    want = np.array(rec["thumbnail"], dtype=rec["thumbnail_dtype"])
    for key in ("thumbnail", "thumbnail_device"):
        scores, info = _run(key, images, embedder=_standin_embedder)
        assert scores.dtype == want.dtype == np.float32 and scores.shape == (len(images),)
        if np.__version__ == GOLD["numpy_version"]:
            assert np.array_equal(scores, want), (key, scores, want)
        else:
            assert (_ulps_f32(scores, want) <= 1).all(), (key, scores, want)
        assert not info["synthetic_weights"]
    if name == "kinds64":
        assert want[2] == 0                                                              # a constant image looks the same at every size
        assert ((want < 0) & (want > -90)).sum() >= 3                                    # neither zero nor saturated by the cosine clip


def test_pixel_values_are_the_reference_s_blocks():
    """Block 0 the originals, block k every image shrunk by FACTORS[k - 1] from the original (not chained), all preprocessed alike."""
    from ddpo_amd.models.clip_vision import preprocess
    u8 = TC.images_u8("24x40")
    px = TH.thumbnail_pixel_values(TC.as_float(u8), 56)
    assert px.shape == (8, 3, 56, 56) and px.dtype == np.float32 and TH.FACTORS == (4, 8, 16)
    assert np.array_equal(px[:2], preprocess(list(u8), 56))
    for k, d in enumerate(TH.FACTORS, 1):
        small = L.resize_u8_host(u8, 24 // d, 40 // d)
        assert np.array_equal(px[2 * k:2 * k + 2], preprocess(list(small), 56)), d


def test_refusals_name_the_rule():
    for shape in [(1, 15, 64, 3), (1, 64, 15, 3)]:
        with pytest.raises(ValueError, match="at least 16 pixels"):
            TH.thumbnail_pixel_values(np.zeros(shape, np.float32), 224)
        with pytest.raises(ValueError, match="at least 16 pixels"):
            _run("thumbnail", np.zeros(shape, np.float32), embedder=_standin_embedder)
    u8 = TC.images_u8("24x40")
    with pytest.raises(ValueError, match="dtype must be float32 or uint8"):
        L.resize_u8_host(u8.astype(np.float64), 6, 10)
    with pytest.raises(ValueError, match="last dimension 3"):
        L.resize_u8_host(u8[0], 6, 10)
    with pytest.raises(ValueError, match="last dimension 3"):
        L.resize_u8_host(u8[..., :2].copy(), 6, 10)
    with pytest.raises(ValueError, match="contiguous"):
        L.resize_u8_host(u8[:, :, ::2], 6, 10)
    with pytest.raises(ValueError, match="empty batch"):
        L.resize_u8_host(u8[:0], 6, 10)
    for oh, ow in [(0, 10), (6, 0), (-1, 10), (6.5, 10)]:
        with pytest.raises(ValueError, match="positive integers"):
            L.resize_u8_host(u8, oh, ow)
    # the LDS rule: 8 staged rows of 7000 x 3 bytes alone are beyond 160 KB; 768^2 and 512^2 by 4, 8, 16 are inside it
    with pytest.raises(ValueError, match="must fit the 160 KB of LDS") as err:
        L.resize_u8_host(np.zeros((1, 16, 7000, 3), np.uint8), 4, 1750)
    assert L.RESIZE_U8_RULE in str(err.value)
    for s in (512, 768):
        for d in TH.FACTORS:
            geo = L.resize_u8_geometry(s, s, s // d, s // d)
            assert geo["band"] == L.RESIZE_U8_BAND and geo["rows"] == d * (geo["band"] - 1) + 4 * d      # by 16: 16 (R - 1) + 64 rows

    # the raw entries return -1 before they touch anything
    lib, p = L.load(), lambda a: a.ctypes.data_as(ctypes.c_void_p)
    (hc, hb, hk), (vc, vb, vk) = L.clip_preprocess_tables(40, 10), L.clip_preprocess_tables(24, 6)
    out = np.zeros((2, 6, 10, 3), np.uint8)
    host = lambda **kw: lib.ddpo_resize_u8_host(*{**dict(im=p(u8), f=0, n=2, h=24, w=40, oh=6, ow=10, hc=p(hc), hb=p(hb), hk=hk, vc=p(vc), vb=p(vb),
                                                         vk=vk, band=2, out=p(out)), **kw}.values())
    assert host() == 0 and np.array_equal(out, _pillow(u8, 6, 10))
    assert host(im=None) == -1 and host(out=None) == -1 and host(hc=None) == -1 and host(vb=None) == -1
    assert host(n=0) == -1 and host(oh=0) == -1 and host(ow=0) == -1 and host(band=0) == -1 and host(hk=0) == -1
    assert host(h=20) == -1                                                             # the vertical table reads rows the image does not have
    assert lib.ddpo_resize_u8(p(u8), 0, 2, 24, 40, 6, 10, p(hc), p(hb), hk, p(vc), p(vb), vk, 8, 0, p(out), None) == -1       # rows < 1
    assert lib.ddpo_resize_u8(p(u8), 0, 2, 24, 40, 6, 10, p(hc), p(hb), hk, p(vc), p(vb), vk, 8, 25, p(out), None) == -1      # rows > H
    assert lib.ddpo_resize_u8(p(u8), 0, 2, 24, 40, 6, 10, p(hc), p(hb), hk, p(vc), p(vb), vk, 8, 24, None, None) == -1
    assert lib.ddpo_resize_u8(p(u8), 0, 1, 16, 7000, 4, 1750, p(hc), p(hb), hk, p(vc), p(vb), vk, 8, 16, p(out), None) == -1  # the LDS rule


def test_registry_and_device_twin_on_host_arrays():
    assert "thumbnail" in C.callback_fns and "thumbnail_device" in C.callback_fns
    images = TC.as_float(TC.images_u8("kinds64"))
    host_fn, dev_fn = (C.callback_fns[n](embedder=_standin_embedder) for n in ("thumbnail", "thumbnail_device"))
    assert not getattr(host_fn, "wants_device_images", False) and dev_fn.wants_device_images is True
    want, want_info = C.evaluate_callbacks({"t": host_fn}, images, ["p"] * 5, ({},) * 5)["t"]
    got, info = C.evaluate_callbacks({"t": dev_fn}, images, ["p"] * 5, ({},) * 5)["t"]
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (5,) and np.array_equal(got, want)
    assert set(info) == set(want_info) == {"synthetic_weights"}
    with pytest.raises(ValueError, match="do not take device images"):
        C.evaluate_callbacks_device({"thumbnail": host_fn}, None, ["p"], ({},))
