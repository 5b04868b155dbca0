"""Shared by tests/test_jpeg_encode_cpu.py and tests/test_gpu_jpeg_encode.py: a stand-in for `requests.Session.post` (no socket) that records every
LLaVA request in the format of tests/golden/reference_host_logic.json and scripts a reply that is a function of the image bytes it received, so a
single wrong byte in a file changes the scores; and the fixture's image recipe."""
import hashlib
import pickle
import types
import zlib

import numpy as np


def scripted_post(captured):
    def fake_post(self, url, data=None, timeout=None, **kw):
        req = pickle.loads(data)
        crc = [zlib.crc32(b) for b in req["images"]]
        captured.append({"url": url, "timeout": timeout, "keys": sorted(req), "queries": req["queries"], "answers": req.get("answers"),
                         "images_sha256": [hashlib.sha256(b).hexdigest() for b in req["images"]], "images_len": [len(b) for b in req["images"]]})
        if "answers" in req:                                # bertscore
            rep = {"recall": [[(c % 1000) / 1000.0] for c in crc], "precision": [[(c % 997) / 997.0] for c in crc],
                   "f1": [[(c % 991) / 991.0] for c in crc], "outputs": [[f"a picture of thing {c}"] for c in crc]}
        else:                                               # vqa
            rep = {"outputs": [[("It is a Cat." if (c + j) % 3 == 0 else "riding a bike") for j in range(len(q))] for c, q in zip(crc, req["queries"])]}
        return types.SimpleNamespace(content=pickle.dumps(rep), status_code=200)
    return fake_post


def fixture_images(seed, n, hw):
    """Same recipe as tests/golden/make_reference_goldens.py:jpeg_test_images."""
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, hw), np.linspace(0, 1, hw), indexing="ij")
    imgs = []
    for i in range(n):
        base = np.stack([yy, xx, 0.5 + 0.5 * np.sin(6.0 * (xx + yy) + i)], axis=-1)
        img = np.clip(base + rng.randn(hw, hw, 3) * 0.05 * (i + 1), 0.0, 1.0)
        imgs.append(img.astype(np.float32))
    return np.stack(imgs)


def same_result(a, b):
    """(scores, info) pairs equal: values, shapes and dtypes"""
    (sa, ia), (sb, ib) = a, b
    ok = np.array_equal(sa, sb) and np.asarray(sa).dtype == np.asarray(sb).dtype and sorted(ia) == sorted(ib)
    return ok and all(np.array_equal(ia[k], ib[k]) and np.asarray(ia[k]).dtype == np.asarray(ib[k]).dtype for k in ia)
