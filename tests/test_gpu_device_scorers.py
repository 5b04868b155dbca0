"""What the six on-device scorers get from their base class (models/device_scorer.py), one case per class: a device batch that is still being
produced on another stream is read only after its `ready` event, the result equals — exactly — the same scorer's result on the batch's host copy,
and every instance has a stream of its own.  A scorer that did not wait would read the zeros the batch buffer holds until the copy lands."""
import numpy as np
import pytest
import torch

import _symmetry_cases as SC
from _jpeg_cases import make_image
from ddpo_amd import lib as L
from ddpo_amd.models import clip_score as CS
from ddpo_amd.models.clip_text import TextConfig, synthetic_text_state
from ddpo_amd.models.clip_vision import VisionConfig
from ddpo_amd.models.jpeg_encode import JpegEncoder
from ddpo_amd.models.jpeg_size import JpegSizer
from ddpo_amd.models.laion import AestheticScorer, synthetic_state_dicts
from ddpo_amd.models.symmetry import RotationalEmbedder, SymmetryStats

pytestmark = pytest.mark.gpu
DEV = "cuda"
PROMPTS = ["a dog", "a cat riding a bike", "", "a dog"]


def _tiny_states(seed=6):
    vcfg = VisionConfig.named("tiny")
    return synthetic_state_dicts(vcfg, vcfg.proj, seed)


def _clip_scorer():
    clip_state, _ = _tiny_states()
    clip_state.update(synthetic_text_state(TextConfig.named("tiny"), 6))
    return CS.ClipScorer(config="tiny", clip_state=clip_state, logit_scale=CS.SYNTHETIC_LOGIT_SCALE, device=DEV)


SCORERS = {
    "JpegSizer": lambda: JpegSizer(quality=95),
    "JpegEncoder": lambda: JpegEncoder(quality=80),
    "SymmetryStats": lambda: SymmetryStats("mirror"),
    "RotationalEmbedder": lambda: RotationalEmbedder(config="tiny", clip_state=_tiny_states()[0], device=DEV),
    "AestheticScorer": lambda: AestheticScorer(config="tiny", clip_state=_tiny_states()[0], mlp_state=_tiny_states()[1], device=DEV),
    "ClipScorer": _clip_scorer,
}


def _call(scorer, images, **kw):
    if isinstance(scorer, CS.ClipScorer):
        return scorer(images, PROMPTS, return_cosine=True, **kw)
    return scorer(images, **kw)


@pytest.fixture(scope="module")
def host_batch():
    """4 x 64 x 64 x 3 float32 in [0, 1]: noise and the left-right symmetric image of the symmetry cases, a smooth and a checkered JPEG case."""
    kinds = SC.images_u8("kinds64")
    return SC.as_float(np.stack([kinds[0], kinds[2], make_image("smooth", 70, 64, 64), make_image("checker", 71, 64, 64)]))


def _same(got, want):
    if isinstance(want, (tuple, list)):
        return type(got) is type(want) and len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want))
    if isinstance(want, bytes):
        return got == want
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("name", list(SCORERS))
def test_scorer_waits_for_the_batch_and_equals_its_host_path(name, host_batch, monkeypatch):
    monkeypatch.setattr(L, "DATAPATH", "bf16x3")
    scorer, other = SCORERS[name](), SCORERS[name]()
    want = _call(scorer, host_batch)

    src = torch.from_numpy(host_batch).to(DEV)
    batch = torch.zeros_like(src)
    busy = torch.randn(8192, 8192, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(4):                                                           # queued in front of the copy: the batch is late
            busy = torch.matmul(busy, busy) * (1 / 8192)
        batch.copy_(src)
        ready = side.record_event()
    got = _call(scorer, batch, ready=ready)                                          # from the default stream, which waits for nothing
    assert _same(got, want)

    torch.cuda.synchronize()
    assert _same(_call(scorer, batch), want)                                         # ready=None: an event on the caller's stream, now
    assert _same(_call(other, batch), want)
    assert scorer.stream is not None and other.stream is not None and scorer.stream != other.stream
