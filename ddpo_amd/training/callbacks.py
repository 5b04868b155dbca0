"""`filter_field` plugin surface: reward callbacks.

Behavioural mirror of the registry / calling convention of /root/reference/ddpo/training/callbacks.py:
  callback_fns[name](**factory_kwargs) -> fn(images, prompts, metadata) -> (scores, info)       (:549-564)
  evaluate_callbacks(fns, images, prompts, metadata) -> {name: (scores, info)}                  (:540-546)
images: float32 (N,H,W,3) in [0,1]; scores: (N,) or (N,1) numpy; info: dict of numpy arrays.
Callbacks run in a worker thread of the entrypoint (ThreadPoolExecutor, max_workers=2) next to the sampling of the
following batch, so they must not touch the sampler's HIP stream: the host ones below are pure CPU code and the
on-device ones (aesthetic, clip_score, rotational, thumbnail and every `*_device` name) use their own streams.

In scope (BASELINE.json configs): jpeg, neg_jpeg (+ jpeg_device, neg_jpeg_device: the same rewards counted on the device), aesthetic, llava_bertscore (+ its sibling llava_vqa wire format), and clip_score: the
prompt-alignment reward that needs no server (CLIPScore on the engine's own CLIP towers; not in the reference, which aligns through LLaVA).
aesthetic_device / clip_score_device are aesthetic / clip_score with the CLIP preprocessing done on the device too, so the decoded batch never
leaves HBM (`wants_device_images`).  llava_bertscore_device / llava_vqa_device are the LLaVA rewards with the JPEG files they send encoded on the
device (models/jpeg_encode.py): only the compressed files cross to the host.
The symmetry family of the reference — mirror, mirror_corr, rotational_corr (pixel rewards; the first and the last in uint8 arithmetic that
wraps, reproduced to the bit) and rotational (CLIP features of the four right-angle turns) — is here too, each with a `*_device` twin that reads the
decoded batch where it is (models/symmetry.py, csrc/symmetry.hip): exact integer sums per image instead of PIL copies, turns and CLIP
preprocessing on the device instead of 4N PIL rotations and resizes.
thumbnail (scale invariance: CLIP features of an image against those of its thumbnails at 1/4, 1/8 and 1/16) has its `thumbnail_device` twin as
well: the thumbnails are made by an 8-bit bicubic resize kernel that outputs Pillow's bytes (models/thumbnail.py, csrc/resize_u8.hip).
The remaining reward ideas of the reference (consistency, diversity, BLIP-2 vqa, arange) are not part of any benchmark config; add
them as plugins with `register`.
"""
import io
import pickle
import random

import numpy as np
from PIL import Image

from ..models.device_scorer import truncate_u8


def register(name):
    def deco(factory):
        callback_fns[name] = factory
        return factory
    return deco


# ------------------------------------------------------------------------------------------------ host / device twins
# A reward with a `*_device` twin is ONE body(images, prompts, metadata, ready=None) over a scorer that takes a host array or a CUDA tensor
# (models/device_scorer.py); `_callback` makes either registry entry of it.
def _callback(body, device):
    """`device`: the body itself, flagged `wants_device_images` — the entrypoint then keeps the decoder's batch in HBM and hands it over with the
    event that says it is complete (evaluate_callbacks_device); host arrays are taken too.  Otherwise the plain three-argument callback."""
    if device:
        body.wants_device_images = True
        return body
    return lambda images, prompts, metadata: body(images, prompts, metadata)


def _negated(fn):
    def _fn(*args, **kwargs):
        scores, info = fn(*args, **kwargs)
        return -scores, info

    return _callback(_fn, device=True) if getattr(fn, "wants_device_images", False) else _fn


# ------------------------------------------------------------------------------------------------ jpeg compressibility
def encode_jpeg(x, quality=95):
    """float [0,1] or uint8 HxWx3 -> JPEG bytes as a uint8 array (reference ddpo/utils/hdf5.py:25-37: floats are
    TRUNCATED to uint8 via (x*255).astype(uint8), PIL quality 95)."""
    x = np.asarray(x)
    if np.issubdtype(x.dtype, np.floating):
        assert np.abs(x).max() <= 1.0
    buf = io.BytesIO()
    Image.fromarray(truncate_u8(x)).save(buf, "JPEG", quality=quality)
    return np.frombuffer(buf.getvalue(), dtype=np.uint8)


def jpeg_fn(devices=None, jit=False):
    """reward = -(JPEG size in kB): compressibility (reference :143-153).  Returns (N,1) float64."""
    assert not jit

    def _fn(images, prompts, metadata):
        del prompts, metadata
        kb = [len(encode_jpeg(im)) / 1000.0 for im in images]
        return -np.array(kb)[:, None], {}

    return _fn


def neg_jpeg_fn(*a, **kw):
    """reward = +(JPEG size in kB): incompressibility (reference :156-163)."""
    return _negated(jpeg_fn(*a, **kw))


def jpeg_device_fn(devices=None, jit=False, quality=95):
    """`jpeg` computed on the device: the same reward — -(len of PIL's JPEG at quality 95) / 1000, (N,1) float64, equal to `jpeg`'s byte for
    byte — from the engine's JPEG byte counter (models/jpeg_size.py, csrc/jpeg_size.hip) on a private HIP stream, without producing the files.
    Takes host images like every callback, or a CUDA tensor straight from the VAE decoder (`wants_device_images`: the entrypoint then keeps the
    batch in HBM, see evaluate_callbacks_device).  Image height and width must be multiples of 16."""
    del devices, jit
    from ..models.jpeg_size import JpegSizer
    sizer = JpegSizer(quality=quality)

    def _fn(images, prompts, metadata, ready=None):
        del prompts, metadata
        return -(sizer(images, ready=ready) / 1000.0)[:, None], {}

    return _callback(_fn, device=True)


def neg_jpeg_device_fn(*a, **kw):
    """`neg_jpeg` computed on the device: +(JPEG size in kB), see jpeg_device_fn."""
    return _negated(jpeg_device_fn(*a, **kw))


# ------------------------------------------------------------------------------------------------ LAION aesthetic
def _aesthetic(device, rng, cache, weights_dir):
    from ..models.laion import AestheticScorer
    scorer = AestheticScorer(weights_dir=weights_dir, cache=cache, seed=rng)

    def _fn(images, prompts, metadata, ready=None):
        del prompts, metadata
        return scorer(images, ready=ready)[:, None], {"synthetic_weights": np.array(scorer.synthetic)}

    return _callback(_fn, device)


def aesthetic_fn(devices=None, rng=0, cache="cache", jit=True, weights_dir=None):
    """CLIP ViT-L/14 image features -> L2-normalise -> LAION aesthetic MLP (reference :60-95, ddpo/models/laion.py), on the engine's
    own kernels (models/clip_vision.py, models/laion.py), on a private HIP stream.  Weights: `weights_dir` or $DDPO_AESTHETIC_WEIGHTS
    (`clip/` in HF format + `sac+logos+ava1-l14-linearMSE.pth`), else the HF cache and `<repo>/<cache>/` where the reference keeps the
    `.pth`; nothing is downloaded.  Missing weights RAISE — an `a_*` run must not silently optimise a random reward — unless
    DDPO_ALLOW_SYNTHETIC=1, in which case info['synthetic_weights'] is True."""
    del devices, jit
    return _aesthetic(False, rng, cache, weights_dir)


def aesthetic_device_fn(devices=None, rng=0, cache="cache", jit=True, weights_dir=None):
    """`aesthetic` without the host trip: the same scores and info, bit for bit.  A CUDA tensor straight from the VAE decoder (`wants_device_images`:
    the entrypoint then keeps the batch in HBM, see evaluate_callbacks_device) is truncated to bytes, resized, cropped, normalised and laid out as
    the patch matrix by one kernel (lib.clip_preprocess, csrc/clip_preprocess.hip) on the scorer's private stream; host arrays take `aesthetic`'s
    own path (PIL).  Weights as for `aesthetic`."""
    del devices, jit
    return _aesthetic(True, rng, cache, weights_dir)


# ------------------------------------------------------------------------------------------------ CLIPScore prompt alignment
def _clip_score(device, rng, cache, weights_dir):
    from ..models.clip_score import ClipScorer
    scorer = ClipScorer(weights_dir=weights_dir, cache=cache, seed=rng)

    def _fn(images, prompts, metadata, ready=None):
        del metadata
        scores, cosine = scorer(images, [str(p) for p in prompts], return_cosine=True, ready=ready)
        return scores[:, None], {"cosine": cosine, "synthetic_weights": np.array(scorer.synthetic)}

    return _callback(_fn, device)


def clip_score_fn(devices=None, rng=0, cache="cache", jit=True, weights_dir=None):
    """reward = exp(logit_scale) * cos(CLIP image embedding, CLIP text embedding of the prompt) — the diagonal of transformers'
    `CLIPModel.logits_per_image` — on the engine's own kernels (models/clip_score.py), on a private HIP stream.  Weights: the
    `openai/clip-vit-large-patch14` checkpoint, looked up exactly like the aesthetic reward's (`weights_dir` or $DDPO_AESTHETIC_WEIGHTS
    `/clip`, else the HF cache); nothing is downloaded.  Missing weights RAISE unless DDPO_ALLOW_SYNTHETIC=1, in which case
    info['synthetic_weights'] is True.  Uses `prompts` (one string per image); `metadata` is ignored.  info['cosine'] is the raw cosine."""
    del devices, jit
    return _clip_score(False, rng, cache, weights_dir)


def clip_score_device_fn(devices=None, rng=0, cache="cache", jit=True, weights_dir=None):
    """`clip_score` without the host trip: the same scores and info (`cosine`, `synthetic_weights`), bit for bit; see aesthetic_device_fn."""
    del devices, jit
    return _clip_score(True, rng, cache, weights_dir)


# ------------------------------------------------------------------------------------------------ symmetry
# The pixel rewards of the reference subtract and square uint8 arrays, so both operations WRAP modulo 256 before the mean: the reward is not the
# mean squared error.  The host callbacks below reproduce that number (held to results recorded from the reference,
# tests/golden/reference_symmetry.json); the device twins get it from an exact integer sum (lib.symmetry_stats, column 0); both report the true
# mean squared difference beside it (info["mse"]).  Partners are array views: u8[:, :, ::-1] is what PIL's ImageOps.mirror returns and
# u8[:, ::-1, ::-1] what Image.rotate(180) returns, for any height and width.  These pairs keep two bodies: numpy there, SymmetryStats here.
def _partner(u8, mode):
    return u8[:, :, ::-1] if mode == "mirror" else u8[:, ::-1, ::-1]


def _wrapped_and_true_mse(u8, mode):
    """(mean of the uint8 square of the uint8 difference — each wraps modulo 256 —, mean of the true squared difference), both (N,) float64 and
    exact: integer sums below 2^53, divided once."""
    other = _partner(u8, mode)
    diff = u8 - other                                           # uint8: modulo 256
    wide = u8.astype(np.int64) - other
    return (diff * diff).mean(axis=(1, 2, 3)), (wide * wide).sum(axis=(1, 2, 3)) / u8[0].size


def _wrapped_mse_fn(mode):
    def _fn(images, prompts, metadata):
        del prompts, metadata
        wrapped, true = _wrapped_and_true_mse(truncate_u8(images), mode)
        return -wrapped, {"mse": true}

    return _fn


def mirror_symmetry_fn(devices=None, jit=False):
    """reward = -mean((image - left-right mirror image) ** 2) over the image's bytes, in uint8 arithmetic that wraps (reference :244-260).
    Returns (N,) float64; info["mse"] is the same mean without the wrap."""
    del devices, jit
    return _wrapped_mse_fn("mirror")


def rotational_correlation_fn(devices=None, jit=False):
    """reward = -mean((image - image turned by 180 degrees) ** 2), in uint8 arithmetic that wraps (reference :216-241: its list of angles holds
    the one turn, so its average over turns is this one term).  Returns (N,) float64; info["mse"] is the same mean without the wrap."""
    del devices, jit
    return _wrapped_mse_fn("rot180")


def mirror_correlation_fn(devices=None, jit=False):
    """reward = -(Pearson correlation of the image's bytes with their left-right mirror image) in float32, as the reference computes it
    (:263-292).  The mirror image is a permutation of the image, so it has the image's mean and variance: the image is centred once, in float32,
    and the correlation is sum(centred * mirrored centred) / sum(centred ** 2).  Returns (N,) float32; a constant image gives nan (0 / 0), as
    there.  Float32 sums: within a few 1e-8 of the exact value."""
    del devices, jit

    def _fn(images, prompts, metadata):
        del prompts, metadata
        x = truncate_u8(images).astype(np.float32) / np.float32(255)
        n = len(x)
        centred = x - x.reshape(n, -1).mean(axis=1).reshape(n, 1, 1, 1)
        cross = (centred * _partner(centred, "mirror")).reshape(n, -1).sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return -(cross / (centred * centred).reshape(n, -1).sum(axis=1)), {}

    return _fn


def _symmetry_stats_of(mode):
    from ..models.symmetry import SymmetryStats
    return SymmetryStats(mode)


def _wrapped_mse_device_fn(mode):
    stats_of = _symmetry_stats_of(mode)

    def _fn(images, prompts, metadata, ready=None):
        del prompts, metadata
        n = int(np.prod(images.shape[1:]))
        stats = stats_of(images, ready=ready)
        return -(stats[:, 0] / n), {"mse": (2 * stats[:, 2] - 2 * stats[:, 3]) / n}

    return _callback(_fn, device=True)


def mirror_symmetry_device_fn(devices=None, jit=False):
    """`mirror` computed on the device: the same (N,) float64 scores and info["mse"], equal to `mirror`'s exactly — every sum is an integer below
    2^53 that is divided once, which is what `ndarray.mean` of a uint8 array computes (models/symmetry.py, csrc/symmetry.hip), on a private HIP
    stream.  Takes host images like every callback, or a CUDA tensor straight from the VAE decoder (`wants_device_images`: the entrypoint then
    keeps the batch in HBM, see evaluate_callbacks_device)."""
    del devices, jit
    return _wrapped_mse_device_fn("mirror")


def rotational_correlation_device_fn(devices=None, jit=False):
    """`rotational_corr` computed on the device: the same scores and info["mse"] exactly; see mirror_symmetry_device_fn."""
    del devices, jit
    return _wrapped_mse_device_fn("rot180")


def mirror_correlation_device_fn(devices=None, jit=False):
    """`mirror_corr` from exact sums: with n bytes a and their mirror partners b, correlation = (n sum(a b) - sum(a)^2) / (n sum(a^2) - sum(a)^2)
    in integer arithmetic, rounded once — the mirror image is a permutation of the image, so both variances are the same.  Returns (N,) float32,
    nan for a constant image; close to `mirror_corr`'s float32 sums, not bit-equal."""
    del devices, jit
    stats_of = _symmetry_stats_of("mirror")

    def _fn(images, prompts, metadata, ready=None):
        del prompts, metadata
        n = int(np.prod(images.shape[1:]))
        scores = []
        for _, sa, saa, sab in stats_of(images, ready=ready).tolist():            # Python integers: no overflow, no rounding before the division
            num, den = n * sab - sa * sa, n * saa - sa * sa
            scores.append(-np.float32(num / den) if den else np.float32("nan"))
        return np.array(scores, dtype=np.float32), {}

    return _callback(_fn, device=True)


def _mean_turn_angle(feats, n_images):
    """Features (B N, proj), block 0 the N images as they are and every further block the same images changed one way (`rotational`: turned by
    90, 180, 270 degrees; `thumbnail`: shrunk by 4, 8, 16) -> (N,) float32: minus the mean, over the B - 1 changes, of the angle in degrees
    between an image's features and the changed image's.  Cosines outside [0, 1] are clipped, so an angle is at most 90."""
    blocks = feats.reshape(-1, n_images, feats.shape[-1])
    upright, turned = blocks[0], blocks[1:]
    lengths = np.linalg.norm(upright, axis=-1)[None] * np.linalg.norm(turned, axis=-1)
    cosines = np.clip((upright[None] * turned).sum(axis=-1) / lengths, 0, 1)
    degrees = np.arccos(cosines) * 180 / np.pi
    return -(degrees.sum(axis=0) / len(turned))


def _mean_angle_callback(device, emb):
    """The one body of `rotational` and `thumbnail`, host and device: `emb` makes the blocks of features, _mean_turn_angle the score."""
    def _fn(images, prompts, metadata, ready=None):
        del prompts, metadata
        feats = emb(images) if ready is None else emb(images, ready=ready)
        return _mean_turn_angle(np.asarray(feats), len(images)), {"synthetic_weights": np.array(getattr(emb, "synthetic", False))}

    return _callback(_fn, device)


def _rotational(device, embedder, rng, cache, weights_dir):
    emb = embedder
    if emb is None:
        from ..models.symmetry import RotationalEmbedder
        emb = RotationalEmbedder(weights_dir=weights_dir, cache=cache, seed=rng)
    return _mean_angle_callback(device, emb)


def rotational_symmetry_fn(devices=None, jit=True, embedder=None, rng=0, cache="cache", weights_dir=None):
    """reward = -(mean angle, in degrees, between the CLIP ViT-L/14 image features of an image and of its turns by 90, 180 and 270 degrees)
    (reference :166-213), the features on the engine's own kernels (models/symmetry.py:RotationalEmbedder, on a private HIP stream).  Weights as
    for `clip_score`; missing weights RAISE unless DDPO_ALLOW_SYNTHETIC=1, in which case info['synthetic_weights'] is True.  `embedder`: anything
    called as embedder(images) -> (4 N, proj) features in the reference's order (tests).  Returns (N,) float32."""
    del devices, jit
    return _rotational(False, embedder, rng, cache, weights_dir)


def rotational_symmetry_device_fn(devices=None, jit=True, embedder=None, rng=0, cache="cache", weights_dir=None):
    """`rotational` without the host trip: the same scores and info, bit for bit.  A square CUDA tensor straight from the VAE decoder
    (`wants_device_images`) is truncated to bytes and turned by one kernel (lib.rotate4_u8, csrc/symmetry.hip) and preprocessed by another
    (lib.clip_preprocess) on the embedder's private stream; host arrays take `rotational`'s own path (PIL).  `embedder` is called as
    embedder(images, ready=ready) when the caller hands an event over."""
    del devices, jit
    return _rotational(True, embedder, rng, cache, weights_dir)


# ------------------------------------------------------------------------------------------------ thumbnail
def _thumbnail(device, embedder, rng, cache, weights_dir):
    emb = embedder
    if emb is None:
        from ..models.thumbnail import ThumbnailEmbedder
        emb = ThumbnailEmbedder(weights_dir=weights_dir, cache=cache, seed=rng)
    return _mean_angle_callback(device, emb)


def thumbnail_fn(devices=None, jit=True, embedder=None, rng=0, cache="cache", weights_dir=None):
    """reward = -(mean angle, in degrees, between the CLIP ViT-L/14 image features of an image and of its thumbnails, shrunk by 4, 8 and 16 with
    Pillow's bicubic resize, each from the original) (reference :295-344): scale invariance.  The features are computed on the engine's own
    kernels (models/thumbnail.py:ThumbnailEmbedder, on a private HIP stream).  Weights as for `clip_score`; missing weights RAISE unless
    DDPO_ALLOW_SYNTHETIC=1, in which case info['synthetic_weights'] is True.  `embedder`: anything called as embedder(images) -> (4 N, proj)
    features in the reference's order (tests).  Height and width must be at least 16.  Returns (N,) float32."""
    del devices, jit
    return _thumbnail(False, embedder, rng, cache, weights_dir)


def thumbnail_device_fn(devices=None, jit=True, embedder=None, rng=0, cache="cache", weights_dir=None):
    """`thumbnail` without the host trip: the same scores and info, bit for bit.  A CUDA tensor straight from the VAE decoder
    (`wants_device_images`) is truncated to bytes and shrunk by three launches of one kernel (lib.resize_u8, csrc/resize_u8.hip), and the
    originals and the thumbnails are preprocessed by another (lib.clip_preprocess) on the embedder's private stream; host arrays take
    `thumbnail`'s own path (PIL).  `embedder` is called as embedder(images, ready=ready) when the caller hands an event over."""
    del devices, jit
    return _thumbnail(True, embedder, rng, cache, weights_dir)


# ------------------------------------------------------------------------------------------------ LLaVA over HTTP
def _to_jpeg_bytes(image_u8, quality=80):
    buf = io.BytesIO()
    Image.fromarray(image_u8).save(buf, format="JPEG", quality=quality)
    return buf.getvalue()


def _llava_session():
    import requests
    from requests.adapters import HTTPAdapter, Retry
    sess = requests.Session()
    sess.mount("http://", HTTPAdapter(max_retries=Retry(total=1000, backoff_factor=1, status_forcelist=[500], allowed_methods=False)))
    return sess


def _bertscore_requests(sess, url, timeout, batch_size, files, prompts, metadata):
    """The request / reply loop of llava_bertscore over the images' JPEG files (a list of bytes), batched as np.array_split batches the images."""
    del metadata
    nb = int(np.ceil(len(files) / batch_size))
    scores, info = [], {"precision": [], "f1": [], "outputs": []}
    for idx_b, prm_b in zip(np.array_split(np.arange(len(files)), nb), np.array_split(np.asarray(prompts), nb)):
        payload = {"images": [files[i] for i in idx_b],
                   "queries": [["Answer concisely: what is going on in this image?"]] * len(idx_b),
                   "answers": [[f"The image contains {p}"] for p in prm_b]}
        reply = pickle.loads(sess.post(url, data=pickle.dumps(payload), timeout=timeout).content)
        scores += np.array(reply["recall"]).squeeze().reshape(-1).tolist()
        for k in info:
            info[k] += np.array(reply[k]).squeeze().reshape(-1).tolist()
    return np.array(scores), {k: np.array(v) for k, v in info.items()}


def _vqa_requests(sess, url, timeout, batch_size, files, prompts, metadata):
    """The request / reply loop of llava_vqa over the images' JPEG files (a list of bytes)."""
    del prompts
    nb = int(np.ceil(len(files) / batch_size))
    metadata = list(metadata)
    scores, answers = [], []
    for idx_b in np.array_split(np.arange(len(files)), nb):
        metas = [metadata[i] for i in idx_b]
        payload = {"images": [files[i] for i in idx_b], "queries": [m["questions"] for m in metas]}
        reply = pickle.loads(sess.post(url, data=pickle.dumps(payload), timeout=timeout).content)
        for m, outs in zip(metas, reply["outputs"]):
            assert len(outs) == len(m["answers"])
            hits = [a in o for a, o in zip(m["answers"], outs)]          # case-sensitive substring test (:357-360)
            scores.append(float(np.mean(np.array(hits, dtype=int))))
        answers += reply["outputs"]
    return np.array(scores), {"answers": np.array(answers)}


def _is_device_batch(images):
    import torch
    return isinstance(images, torch.Tensor)


def _host_jpeg_files(images, ready=None):
    del ready
    return [_to_jpeg_bytes(im) for im in truncate_u8(images)]


def _device_jpeg_files():
    """images -> JPEG files at quality 80: a CUDA batch through one JpegEncoder (models/jpeg_encode.py, created with the first such batch, on its
    device and on a stream of its own), a host array through PIL as the host callbacks do."""
    encoder = []

    def _files(images, ready=None):
        if not _is_device_batch(images):
            return _host_jpeg_files(images)
        if not encoder:
            from ..models.jpeg_encode import JpegEncoder
            encoder.append(JpegEncoder(quality=80, device=images.device))
        return encoder[0](images, ready=ready)

    return _files


def _llava(device, requests_of, url, batch_size, timeout):
    """The LLaVA pairs differ in where the files come from only: PIL, or for a CUDA batch the encoder above."""
    sess, files_of = _llava_session(), _device_jpeg_files() if device else _host_jpeg_files

    def _fn(images, prompts, metadata, ready=None):
        return requests_of(sess, url, timeout, batch_size, files_of(images, ready), prompts, metadata)

    return _callback(_fn, device)


def llava_bertscore(devices=None, jit=False, url="http://127.0.0.1:8085", batch_size=16, timeout=120):
    """Alignment reward served by a LLaVA + BERTScore server (reference :465-537).  Wire format: POST of
    pickle.dumps({"images": [jpeg bytes, q=80], "queries": [[str]], "answers": [[str]]}); the reply is a pickled dict
    with "recall" (the reward), "precision", "f1", "outputs".  Batches of 16; 1000 retries on HTTP 500."""
    return _llava(False, _bertscore_requests, url, batch_size, timeout)


def llava_vqa_satisfaction(devices=None, jit=False, url="http://127.0.0.1:8085", batch_size=4, timeout=120):
    """VQA reward (reference :402-462): request {"images", "queries"} (questions from the prompt metadata), reply
    {"outputs"}; the score of an image is the fraction of answers that contain the expected answer string
    (case-sensitive); info = {"answers": the server's outputs}."""
    return _llava(False, _vqa_requests, url, batch_size, timeout)


def llava_bertscore_device(devices=None, jit=False, url="http://127.0.0.1:8085", batch_size=16, timeout=120):
    """`llava_bertscore` without the host trip of the pixels: the same requests, scores and info, byte for byte.  A CUDA tensor straight from the
    VAE decoder (`wants_device_images`: the entrypoint then keeps the batch in HBM, see evaluate_callbacks_device) is encoded once, on the device,
    into the files PIL writes at quality 80 (models/jpeg_encode.py, csrc/jpeg_size.hip) and only those cross to the host; host arrays take
    `llava_bertscore`'s own path (PIL).  Image height and width must be multiples of 16."""
    return _llava(True, _bertscore_requests, url, batch_size, timeout)


def llava_vqa_device(devices=None, jit=False, url="http://127.0.0.1:8085", batch_size=4, timeout=120):
    """`llava_vqa` without the host trip of the pixels: the same requests, scores and info; see llava_bertscore_device."""
    return _llava(True, _vqa_requests, url, batch_size, timeout)


# ------------------------------------------------------------------------------------------------ registry
def evaluate_callbacks(fns, images, prompts, metadata):
    if type(prompts[0]) == list:
        prompts = [random.choice(p) for p in prompts]
    images = np.asarray(images).astype(np.float32)
    return {key: fn(images, prompts, metadata) for key, fn in fns.items()}


def evaluate_callbacks_device(fns, images_dev, prompts, metadata, ready=None):
    """evaluate_callbacks for callbacks that carry `wants_device_images`: `images_dev` is the decoder's float32 (N,H,W,3) CUDA tensor and is handed
    over as it is — nothing is copied to the host.  `ready`: an event recorded on the producing stream when the images were complete (the
    callbacks' streams wait for it); without one, the caller's current stream as of this call is waited for."""
    missing = [key for key, fn in fns.items() if not getattr(fn, "wants_device_images", False)]
    if missing:
        raise ValueError(f"callbacks {missing} do not take device images; use evaluate_callbacks")
    if type(prompts[0]) == list:
        prompts = [random.choice(p) for p in prompts]
    if ready is None:
        import torch
        ready = torch.cuda.current_stream(images_dev.device).record_event()
    return {key: fn(images_dev, prompts, metadata, ready=ready) for key, fn in fns.items()}


def vae_fn(devices=None, dtype="float32", jit=True, encoder=None):
    """The `vae` field of the RWR sampler (reference :37-57): images (N,H,W,3) in [0,1] -> VAE posterior moments
    concat([mean, logvar], -1) (N,H/8,W/8,8) from the engine's VAE encoder (ddpo_amd/models/vae.py:VAEEncoder).  The reference
    loads the SD-1.4 Flax VAE itself; here the caller hands the loaded encoder over (`set_vae_encoder`, pipeline/sample.py) —
    nothing is downloaded."""
    import torch
    enc = encoder if encoder is not None else _VAE_ENCODER.get("encoder")
    if enc is None:
        raise RuntimeError("the `vae` callback needs a loaded VAE encoder: call ddpo_amd.training.callbacks.set_vae_encoder(encoder) first")

    def _fn(images, prompts=None, metadata=None):
        with torch.no_grad():
            m = enc.encode(torch.as_tensor(np.asarray(images, dtype=np.float32)))
        return m.cpu().numpy(), {}

    return _fn


_VAE_ENCODER = {}


def set_vae_encoder(encoder):
    _VAE_ENCODER["encoder"] = encoder


callback_fns = {
    "vae": vae_fn,
    "jpeg": jpeg_fn,
    "neg_jpeg": neg_jpeg_fn,
    "jpeg_device": jpeg_device_fn,
    "neg_jpeg_device": neg_jpeg_device_fn,
    "aesthetic": aesthetic_fn,
    "clip_score": clip_score_fn,
    "aesthetic_device": aesthetic_device_fn,
    "clip_score_device": clip_score_device_fn,
    "llava_bertscore": llava_bertscore,
    "llava_vqa": llava_vqa_satisfaction,
    "llava_bertscore_device": llava_bertscore_device,
    "llava_vqa_device": llava_vqa_device,
    "mirror": mirror_symmetry_fn,
    "mirror_corr": mirror_correlation_fn,
    "rotational_corr": rotational_correlation_fn,
    "rotational": rotational_symmetry_fn,
    "mirror_device": mirror_symmetry_device_fn,
    "mirror_corr_device": mirror_correlation_device_fn,
    "rotational_corr_device": rotational_correlation_device_fn,
    "rotational_device": rotational_symmetry_device_fn,
    "thumbnail": thumbnail_fn,
    "thumbnail_device": thumbnail_device_fn,
}
