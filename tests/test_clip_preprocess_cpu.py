"""CLIP preprocessing without a GPU: the serial host entry `ddpo_clip_preprocess_host` — the very functions the kernel of csrc/clip_preprocess.hip
runs (csrc/clip_preprocess_core.h) — against Pillow called here and against `clip_vision.preprocess`, bit for bit, with no tolerance; the
coefficient tables; and what the wrappers and the raw entries refuse."""
import ctypes

import numpy as np
import pytest

from _clip_cases import CASES, KINDS, PATCH, as_float, case_key, im2col, k_pad, load_golden, make_image, pil_resized, seed_of, sha
from ddpo_amd import lib as L
from ddpo_amd.models import clip_vision as CV

KP = k_pad()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("hw,size", CASES, ids=[f"{h}x{w}-{s}" for (h, w), s in CASES])
def test_host_entry_equals_pillow_and_preprocess(hw, size):
    """Stage by stage, so a failure says which stage broke: the resized bytes against Pillow's resize itself, then the normalised patch matrix
    against the im2col of `preprocess`, as fp32 bit patterns, pad columns exactly +0."""
    h, w = hw
    for kind in KINDS:
        u8 = make_image(kind, seed_of(kind, h, w), h, w)
        got, resized = L.clip_preprocess_host(u8[None], size, PATCH, KP, return_resized=True)
        assert np.array_equal(resized[0], pil_resized(u8, size)), (kind, "resize")
        want = im2col(CV.preprocess(u8[None], size))
        assert got.dtype == np.float32 and got.shape == want.shape == ((size // PATCH) ** 2, KP)
        assert np.array_equal(_bits(got), _bits(want)), (kind, "normalise / layout")
        assert not _bits(got)[:, 3 * PATCH * PATCH:].any(), (kind, "pad columns")
        f32 = as_float(u8)
        assert np.array_equal((f32 * 255).astype(np.uint8), u8)
        assert np.array_equal(_bits(L.clip_preprocess_host(f32[None], size, PATCH, KP)), _bits(want)), (kind, "float32 input")
        assert np.array_equal(_bits(want), _bits(im2col(CV.preprocess(f32[None], size))))


def test_host_entry_takes_a_batch_and_truncates_floats():
    ims = np.stack([make_image(k, 5 + i, 48, 80) for i, k in enumerate(KINDS)])
    got = L.clip_preprocess_host(ims, 56, PATCH, KP)
    assert np.array_equal(_bits(got), _bits(im2col(CV.preprocess(ims, 56))))
    x = np.random.default_rng(3).random((2, 40, 40, 3), dtype=np.float32)          # arbitrary floats: truncation, not rounding
    x[0, 0, 0] = (1.0, 0.0, np.float32(254.999) / np.float32(255))
    assert ((x * 255).astype(np.uint8) != np.rint(x * 255)).any()
    assert np.array_equal(_bits(L.clip_preprocess_host(x, 28, PATCH, KP)), _bits(im2col(CV.preprocess(x, 28))))


def test_recorded_hashes_tell_another_pillow_from_a_bug():
    gold = load_golden()
    assert len(gold) == len(CASES) * len(KINDS)
    for (h, w), size in CASES:
        for kind in KINDS:
            u8 = make_image(kind, seed_of(kind, h, w), h, w)
            live = sha(pil_resized(u8, size))
            assert live == gold[case_key(kind, h, w, size)], "the live Pillow and the recorded hashes disagree: another resampler?"
            assert sha(L.clip_preprocess_host(u8[None], size, PATCH, KP, return_resized=True)[1][0]) == live


def _raw_host_args(u8, size, patch, ld):
    n, h, w = u8.shape[:3]
    geo = L.clip_preprocess_geometry(h, w, size, patch, ld)
    hc, hb, hk = L.clip_preprocess_tables(w, geo["ow"])
    vc, vb, vk = L.clip_preprocess_tables(h, geo["oh"])
    out = np.zeros((n * (size // patch) ** 2, ld), np.float32)
    keep = [u8, hc, hb, vc, vb, L.clip_norm_table(), out]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    args = dict(images=p(u8), is_float32=0, N=n, H=h, W=w, rh=geo["oh"], rw=geo["ow"], top=geo["top"], left=geo["left"], size=size, patch=patch,
                hcoef=p(hc), hbounds=p(hb), hk=hk, vcoef=p(vc), vbounds=p(vb), vk=vk, norm=p(keep[5]), out=p(out), ld=ld, resized=None)
    return args, geo, keep


def test_tables_and_refusals():
    for (i, o), ksize in {(512, 224): 11, (768, 224): 15, (32, 56): 5}.items():
        coef, bounds, k = L.clip_preprocess_tables(i, o)
        assert k == ksize and coef.shape == (o, ksize) and coef.dtype == np.int32 and bounds.shape == (o, 2)
        assert (np.abs(coef.astype(np.int64).sum(1) - (1 << 22)) <= ksize).all()              # each weight is rounded once: the sum is off by < ksize
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= i).all() and (bounds[:, 1] <= ksize).all() and (bounds[:, 1] >= 1).all()
        assert (np.diff(bounds[:, 0]) >= 0).all()
        assert not coef[np.arange(ksize)[None, :] >= bounds[:, 1:2]].any()                     # taps past the count are zero
    coef, bounds, k = L.clip_preprocess_tables(56, 56)                                         # an axis that keeps its size: the identity
    assert k == 1 and (coef == 1 << 22).all() and np.array_equal(bounds[:, 0], np.arange(56)) and (bounds[:, 1] == 1).all()
    t = L.clip_norm_table()
    mean, std = np.asarray(CV.CLIP_MEAN, np.float32), np.asarray(CV.CLIP_STD, np.float32)
    assert t.shape == (256, 3) and t.dtype == np.float32 and np.array_equal(_bits(t[255]), _bits((np.float32(255) * np.float32(1 / 255) - mean) / std))

    # the wrapper names the rule that is broken
    u8 = make_image("noise", 1, 64, 64)[None]
    with pytest.raises(ValueError, match="not a multiple of patch"):
        L.clip_preprocess_host(u8, 50, PATCH, KP)
    with pytest.raises(ValueError, match="at least 3 \\* patch \\* patch"):
        L.clip_preprocess_host(u8, 56, PATCH, 3 * PATCH * PATCH - 4)
    with pytest.raises(ValueError, match="multiple of 4"):
        L.clip_preprocess_host(u8, 56, PATCH, 3 * PATCH * PATCH + 2)
    with pytest.raises(ValueError, match="N x H x W x 3"):
        L.clip_preprocess_host(u8[..., :2], 56, PATCH, KP)
    with pytest.raises(ValueError, match="uint8 or float32"):
        L.clip_preprocess_host(u8.astype(np.float64), 56, PATCH, KP)
    big = np.zeros((1, 2400, 2400, 3), np.uint8)                                               # one patch row of 56 spans > 700 input rows
    with pytest.raises(ValueError, match="must fit the 160 KB of LDS") as exc:
        L.clip_preprocess_host(big, 56, PATCH, KP)
    assert L.CLIP_PREPROCESS_RULE in str(exc.value)

    # the raw entries return -1 for each of them
    lib = L.load()
    host = lambda a: lib.ddpo_clip_preprocess_host(*a.values())
    args, geo, keep = _raw_host_args(u8, 56, PATCH, KP)
    assert host(args) == 0
    for name in ("images", "hcoef", "hbounds", "vcoef", "vbounds", "norm", "out"):
        assert host({**args, name: None}) == -1, name
    assert host({**args, "size": 50}) == -1                                                    # not a multiple of patch
    assert host({**args, "ld": 3 * PATCH * PATCH - 4}) == -1
    assert host({**args, "ld": 3 * PATCH * PATCH + 2}) == -1
    assert host({**args, "top": geo["oh"] - 56 + 1}) == -1 and host({**args, "left": -1}) == -1      # crop window outside the resized image
    assert host({**args, "rw": 55}) == -1
    bad = keep[2].copy()
    bad[3, 0] = 64                                                                             # a bound past the image
    assert host({**args, "hbounds": bad.ctypes.data_as(ctypes.c_void_p)}) == -1
    # the LDS rule: a 4096 x 56 image passes with its rows kept (identity table, 14 rows per patch row) ...
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    tall, out_t = np.zeros((1, 4096, 56, 3), np.uint8), np.zeros((16, KP), np.float32)
    hc, hb, hk = L.clip_preprocess_tables(56, 56)
    vc, vb, vk = L.clip_preprocess_tables(4096, 4096)
    fits = dict(args, images=p(tall), H=4096, W=56, rh=4096, rw=56, top=2020, left=0, hcoef=p(hc), hbounds=p(hb), hk=hk, vcoef=p(vc),
                vbounds=p(vb), vk=vk, out=p(out_t))
    assert host(fits) == 0
    # ... and is refused squeezed to 56 rows, where one patch row needs more than 1000 of them
    vc2, vb2, vk2 = L.clip_preprocess_tables(4096, 56)
    assert host(dict(fits, rh=56, top=0, vcoef=p(vc2), vbounds=p(vb2), vk=vk2)) == -1

    # the device entry refuses the same before it touches the GPU
    order = ["images", "is_float32", "N", "H", "W", "rh", "rw", "top", "left", "size", "patch", "hcoef", "hbounds", "hk", "vcoef", "vbounds", "vk",
             "rows", "norm", "out", "ld"]

    def device(**kw):
        a = {**args, "rows": geo["rows"], **kw}
        return lib.ddpo_clip_preprocess(*[a[k] for k in order], None)

    assert device(images=None) == -1 and device(out=None) == -1 and device(norm=None) == -1
    assert device(size=50) == -1 and device(ld=3 * PATCH * PATCH - 4) == -1 and device(top=1) == -1
    assert device(rows=100000) == -1 and device(rows=0) == -1
    assert device(H=4096, rows=1000) == -1                                                     # the LDS rule: 1000 x 176 B > 160 KB


def test_callback_registry():
    from ddpo_amd.training import callbacks as C
    assert "aesthetic_device" in C.callback_fns and "clip_score_device" in C.callback_fns
    assert hasattr(CV.ClipVisionTower, "forward_patches")
