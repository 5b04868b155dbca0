"""The symmetry rewards without a GPU: the host callbacks (mirror, mirror_corr, rotational_corr, rotational) against results recorded from the
reference's own code (tests/golden/reference_symmetry.json), the serial host entries `ddpo_symmetry_stats_host` / `ddpo_rotate4_u8_host` — the
very functions the kernels of csrc/symmetry.hip run (csrc/symmetry_core.h) — against numpy and Pillow with no tolerance, what the wrappers
refuse, and the registry."""
import ctypes

import numpy as np
import pytest
from PIL import Image

import _symmetry_cases as SC
from ddpo_amd import lib as L
from ddpo_amd.models import symmetry as SY
from ddpo_amd.training import callbacks as C

GOLD = SC.load_golden()
ALL = list(SC.CASES) + list(SC.EXTRA)
CORR_BOUND = SC.MIRROR_CORR_FACTOR * GOLD["mirror_corr_f32_dev"]
HOST = ("mirror", "mirror_corr", "rotational_corr", "rotational")


def _recorded(name, key):
    rec = GOLD["cases"][name]
    return np.array([np.nan if v is None else v for v in rec[key]], dtype=rec[key + "_dtype"])


def _standin_embedder(images, ready=None):
    assert ready is None
    return SC.standin_features(SY.rotated_pixel_values(images, 224))


def _run(key, images, **kw):
    return C.evaluate_callbacks({key: C.callback_fns[key](**kw)}, images, ["a prompt"] * len(images), ({},) * len(images))[key]


def _ulps_f32(a, b):
    """distance in float32 units in the last place (both finite, same sign or zero)"""
    ia, ib = (np.abs(x.astype(np.float32)).view(np.int32).astype(np.int64) * np.where(np.signbit(x), -1, 1) for x in (a, b))
    return np.abs(ia - ib)


@pytest.mark.parametrize("name", ALL)
def test_host_callbacks_reproduce_the_reference(name):
    u8 = SC.images_u8(name)
    images = SC.as_float(u8)
    assert list(u8.shape) == GOLD["cases"][name]["shape"] and np.array_equal((images * 255).astype(np.uint8), u8)
    for key in ("mirror", "rotational_corr"):
        scores, info = _run(key, images)
        want = _recorded(name, key)
        assert scores.dtype == want.dtype == np.float64 and scores.shape == (len(u8),) and np.array_equal(scores, want), key
        # the reward is NOT the mean squared error: uint8 arithmetic wraps.  info["mse"] is the unwrapped one
        b = u8[:, :, ::-1] if key == "mirror" else u8[:, ::-1, ::-1]
        true = ((u8.astype(np.int64) - b) ** 2).sum(axis=(1, 2, 3)) / u8[0].size
        assert set(info) == {"mse"} and info["mse"].dtype == np.float64 and np.array_equal(info["mse"], true)
    scores, info = _run("mirror_corr", images)
    want = _recorded(name, "mirror_corr")
    assert scores.dtype == want.dtype == np.float32 and scores.shape == (len(u8),) and info == {}
    assert np.array_equal(np.isnan(scores), np.isnan(want))                              # a constant image: nan, as there
    ok = ~np.isnan(want)
    assert (np.abs(scores[ok].astype(np.float64) - want[ok]) <= CORR_BOUND).all(), np.abs(scores[ok].astype(np.float64) - want[ok]).max()


def test_wrapped_reward_differs_from_the_true_mse():
    scores, info = _run("mirror", SC.as_float(SC.images_u8("kinds64")))
    assert -scores[0] < 128 < info["mse"][0]                                             # noise: the wrapped mean stays below 128, the true one is ~10^4
    assert scores[2] == 0 and info["mse"][2] == 0 and scores[3] == 0                     # the symmetric and the constant image
    assert -scores[4] < 1 and info["mse"][4] > 1e4                                       # 0 / 255 extremes: 255^2 mod 256 = 1


@pytest.mark.parametrize("name", SC.ROTATIONAL_CASES)
def test_rotational_reproduces_the_reference_given_the_same_features(name):
    """The recording ran the reference's own wrapper around stand-in features (see tests/golden/make_reference_symmetry_goldens.py); here the same
    stand-in sits behind the `embedder` seam, so the rotation order, the reshape and the angle arithmetic are what is compared.  Equal to the
    recording bit for bit under the numpy that made it (`numpy_version` in the fixture); only under another numpy, whose arccos may round
    differently, is 1 float32 ulp allowed."""
    images = SC.as_float(SC.images_u8(name))
    want = _recorded(name, "rotational")
    for key in ("rotational", "rotational_device"):
        scores, info = _run(key, images, embedder=_standin_embedder)
        assert scores.dtype == want.dtype == np.float32 and scores.shape == (len(images),)
        if np.__version__ == GOLD["numpy_version"]:
            assert np.array_equal(scores, want), (key, scores, want)
        else:
            assert (_ulps_f32(scores, want) <= 1).all(), (key, scores, want)
        assert not info["synthetic_weights"]
    assert want[3] == 0 if name == "kinds64" else True                                   # a constant image looks the same under every turn


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("mode", ["mirror", "rot180"])
def test_stats_host_equals_numpy(name, mode):
    u8 = SC.images_u8(name)
    want = SC.stats_numpy(u8, mode)
    got = L.symmetry_stats_host(u8, mode)
    assert got.dtype == np.int64 and got.shape == (len(u8), 4) and np.array_equal(got, want)
    b = u8[:, :, ::-1] if mode == "mirror" else u8[:, ::-1, ::-1]
    true_sq = ((u8.astype(np.int64) - b) ** 2).sum(axis=(1, 2, 3))
    assert np.array_equal(2 * got[:, 2] - 2 * got[:, 3], true_sq)
    assert np.array_equal(L.symmetry_stats_host(SC.as_float(u8), mode), want)            # float input = its truncated bytes
    if name == "all255":
        assert got[0, 2] > 2 ** 32                                                       # what a 32-bit accumulator loses


@pytest.mark.parametrize("s,n", [(1, 1), (5, 2), (56, 1), (72, 3)])
def test_rotate4_host_equals_pillow(s, n):
    u8 = np.random.default_rng(s).integers(0, 256, (n, s, s, 3), dtype=np.uint8)
    got = L.rotate4_u8_host(u8)
    assert got.dtype == np.uint8 and got.shape == (4 * n, s, s, 3)
    for k in range(4):
        for i in range(n):
            assert np.array_equal(got[k * n + i], np.array(Image.fromarray(u8[i]).rotate(90 * k))), (k, i)
            assert np.array_equal(got[k * n + i], np.rot90(u8[i], k))
    assert np.array_equal(L.rotate4_u8_host(SC.as_float(u8)), got)


def test_floats_are_truncated_like_the_reference():
    x = np.random.default_rng(3).random((2, 12, 12, 3), dtype=np.float32)
    x[0, 0, 0] = (1.0, 0.0, np.float32(254.999) / np.float32(255))
    u8 = (x * 255).astype(np.uint8)
    assert (u8 != np.rint(x * 255)).any()
    for mode in ("mirror", "rot180"):
        assert np.array_equal(L.symmetry_stats_host(x, mode), SC.stats_numpy(u8, mode))
    assert np.array_equal(L.rotate4_u8_host(x), L.rotate4_u8_host(u8)) and np.array_equal(L.rotate4_u8_host(x)[:2], u8)


def test_refusals_name_the_rule():
    u8 = SC.images_u8("24x40")
    with pytest.raises(ValueError, match="dtype must be float32 or uint8"):
        L.symmetry_stats_host(u8.astype(np.float64), "mirror")
    with pytest.raises(ValueError, match="contiguous"):
        L.symmetry_stats_host(u8[:, :, ::2], "mirror")
    with pytest.raises(ValueError, match="last dimension 3"):
        L.symmetry_stats_host(u8[..., :2].copy(), "mirror")
    with pytest.raises(ValueError, match="last dimension 3"):
        L.rotate4_u8_host(u8[0])
    with pytest.raises(ValueError, match="empty batch"):
        L.symmetry_stats_host(u8[:0], "rot180")
    with pytest.raises(ValueError, match="mode must be one of"):
        L.symmetry_stats_host(u8, "rot90")
    with pytest.raises(ValueError, match="square"):
        L.rotate4_u8_host(u8)
    with pytest.raises(ValueError, match="at most 10880 pixels"):
        L.symmetry_stats_host(np.zeros((1, 1, L.SYMMETRY_MAX_W + 1, 3), np.uint8), "mirror")
    with pytest.raises(ValueError, match="at most 10880 pixels"):
        L.symmetry_stats_workspace_bytes(1, 4, L.SYMMETRY_MAX_W + 1, "mirror")
    assert L.symmetry_stats_workspace_bytes(3, 512, 512, "mirror") == 3 * 64 * 32 and L.symmetry_stats_workspace_bytes(2, 5, 8, "rot180") == 2 * 3 * 32
    with pytest.raises(ValueError, match="mode must be one of"):
        SY.SymmetryStats("flip")

    # the raw entries return -1 before they touch anything
    lib, p = L.load(), lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out, rot = np.zeros((2, 4), np.int64), np.zeros((8, 24, 40, 3), np.uint8)
    assert lib.ddpo_symmetry_stats_host(p(u8), 0, 2, 24, 40, 0, p(out)) == 0
    assert lib.ddpo_symmetry_stats_host(None, 0, 2, 24, 40, 0, p(out)) == -1 and lib.ddpo_symmetry_stats_host(p(u8), 0, 2, 24, 40, 0, None) == -1
    assert lib.ddpo_symmetry_stats_host(p(u8), 0, 2, 24, 40, 2, p(out)) == -1 and lib.ddpo_symmetry_stats_host(p(u8), 0, 0, 24, 40, 0, p(out)) == -1
    assert lib.ddpo_rotate4_u8_host(p(u8), 0, 2, 24, 40, p(rot)) == -1                   # not square
    assert lib.ddpo_rotate4_u8(p(u8), 0, 2, 24, 40, p(rot), None) == -1
    assert lib.ddpo_symmetry_stats(p(u8), 0, 2, 24, 40, 0, p(out), p(rot), 63, None) == -1      # a workspace of 63 bytes where 2 x 24 x 32 are needed
    assert lib.ddpo_symmetry_stats(p(u8), 0, 2, 24, 40, 3, p(out), p(rot), rot.size, None) == -1
    assert lib.ddpo_symmetry_stats(p(u8), 0, 2, 24, 40, 0, None, p(rot), rot.size, None) == -1


def test_registry_and_device_twins_on_host_arrays():
    names = HOST + tuple(n + "_device" for n in HOST)
    assert all(n in C.callback_fns for n in names)
    images = SC.as_float(SC.images_u8("kinds64"))
    for name in HOST:
        kw = {"embedder": _standin_embedder} if name == "rotational" else {}
        host_fn, dev_fn = C.callback_fns[name](**kw), C.callback_fns[name + "_device"](**kw)
        assert not getattr(host_fn, "wants_device_images", False) and dev_fn.wants_device_images is True
        want, want_info = C.evaluate_callbacks({name: host_fn}, images, ["p"] * 5, ({},) * 5)[name]
        got, info = C.evaluate_callbacks({name: dev_fn}, images, ["p"] * 5, ({},) * 5)[name]
        assert got.dtype == want.dtype and got.shape == want.shape == (5,) and set(info) == set(want_info)
        if name == "mirror_corr":                                                        # exact sums against float32 sums: the one tolerance
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[3])
            ok = ~np.isnan(want)
            assert (np.abs(got[ok].astype(np.float64) - want[ok]) <= CORR_BOUND).all()
            # consistency only (the same formula restated in _symmetry_cases): the twin rounds once.  Correctness is the bound above
            assert np.array_equal(got[ok], SC.exact_mirror_corr(SC.images_u8("kinds64"))[ok].astype(np.float32))
        else:
            assert np.array_equal(got, want), name
            assert all(np.array_equal(info[k], want_info[k]) for k in info), name
    with pytest.raises(ValueError, match="do not take device images"):
        C.evaluate_callbacks_device({"mirror": C.callback_fns["mirror"]()}, None, ["p"], ({},))
