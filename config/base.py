"""Hyper-parameters for `pipeline/policy_gradient.py` — the `pg` experiment of the reference's flag surface.

Same keys, defaults and precedence as /root/reference/config/base.py:61-102 (`base["pg"]`) and its per-dataset
`common` / `pg` overrides (:106-148, :222-314).  Round 3 adds the `sample` / `train` experiments of the RWR baseline
(`pipeline/sample.py`, `pipeline/finetune.py`; reference :4-60 and the per-dataset `sample` / `train` overrides); `sizes` and
`calibrate` (bucket bookkeeping) stay out.  Values are declarative data; the tables are assembled by helpers so that adding a
dataset is one line.
"""
from . import user

_PG_DEFAULTS = (
    # misc
    ("loadpath", ""), ("load_epoch", "latest"), ("modelpath", "models/pg"), ("savepath", "f:models/pg"),
    ("pretrained_model", "duongna/stable-diffusion-v1-4-flax"), ("resolution", 512), ("filter_field", None),
    ("guidance_scale", 5.0), ("dtype", "float32"), ("cache", "cache"), ("verbose", False), ("seed", 0), ("iteration", 0),
    # sampling (batch sizes are per device)
    ("sample_batch_size", 8), ("num_sample_batches_per_epoch", 1), ("n_inference_steps", 50), ("identical_batch", False),
    ("evaluate", False), ("eta", 1.0),
    # training
    ("train_batch_size", 2), ("train_accumulation_steps", 1), ("num_train_epochs", 200), ("num_inner_epochs", 1),
    ("ppo_clip_range", 1e-4), ("train_cfg", True), ("learning_rate", 1e-5), ("beta1", 0.9), ("beta2", 0.999),
    ("weight_decay", 1e-4), ("epsilon", 1e-8), ("max_grad_norm", 1.0), ("save_freq", 10), ("optimizer", "adamw"),
    ("train_timestep_ratio", 1.0), ("prompt_kwargs", {}), ("per_prompt_stats_bufsize", 32), ("per_prompt_stats_min_count", 16),
    # engine-specific addition (not a reference flag): how optax.adamw(mu_dtype=bfloat16) forms `b1 * mu` — True: in bf16, what JAX's
    # weak-type promotion does (scalar x bf16 array stays bf16: b1 -> 0.8984375, product rounded before the f32 term is added);
    # False: decay in f32, one rounding when mu is stored.  optax is not installable here, so the reading is a derivation, not a measurement.
    # None = not given on the command line: the entrypoint then takes DDPO_MU_DECAY_IN_BF16 (default 1 = True).
    ("mu_decay_in_bf16", None),
    # engine-specific addition: LoRA adapters on the U-Net attention projections (ddpo_amd/models/lora.py).  lora_rank 0 = full fine-tuning
    # (the reference's only mode); lora_alpha None = lora_rank (scale alpha / rank = 1).  LoRA usually wants a far higher learning_rate than
    # the 1e-5 default of full fine-tuning; the default is not changed here.
    ("lora_rank", 0), ("lora_alpha", None),
    # engine-specific addition: which layers --lora_rank adapts.  "attn" = the 128 attention projections; "attn_ff" = those and the two GEGLU
    # feed-forward layers of every transformer block (160 layers, 1.9 times the adapter parameters for SD-1.5; the wide layers' adapter
    # gradients come from csrc/lora_wide.hip).  proj_in / proj_out and the convolutions are never adapted.  Needs lora_rank > 0.
    ("lora_targets", "attn"),
    # engine-specific addition: KL penalty to the frozen pretrained policy (DPOK's regulariser; ddpo_amd/training/kl_reference.py,
    # DESIGN.md §4): loss += kl_coef * KL(policy || pretrained) per DDIM step, in the units of the PPO loss.  0 = off (the reference's
    # only mode): no second U-Net is built and the training step is unchanged.  Needs eta > 0.
    ("kl_coef", 0.0),
    # engine-specific addition: the training objective.  "ppo" = the reference's only mode.  "d3po" (Yang et al., "Using Human Feedback to
    # Fine-tune Diffusion Models without Any Reward Model"): prompts are drawn once per two adjacent rows, the pair is ranked by
    # the sign of its reward difference and a DPO loss is applied per DDIM step on the policy-to-pretrained log-ratio; rewards' scale, the
    # per-prompt tracker, the stored log-probs and ppo_clip_range are not used.  Needs eta > 0 and even sample / train batch sizes.
    # d3po_beta 0.1 is the value the D3PO authors ship (their log-prob is a mean over the latent, as here); it has not been measured in a
    # training run on this engine.
    ("pg_loss", "ppo"), ("d3po_beta", 0.1),
    # engine-specific addition: rescaled classifier-free guidance (Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed",
    # §3.4; diffusers' `guidance_rescale`; ddpo_amd/lib_cfg_rescale.py): the guided prediction is scaled per sample towards the
    # standard deviation of the conditional one, out = (1 - r + r std(cond) / std(guided)) * guided.  v-prediction checkpoints (SD-2.1 768)
    # are normally sampled with 0.7; the sampler and every loss (PPO ratio, KL, D3PO log-ratio) then use the rescaled prediction.  0 = off
    # (the reference's only mode): nothing new is launched.  In [0, 1]; a positive value needs train_cfg True.
    ("guidance_rescale", 0.0),
)

_SAMPLE_DEFAULTS = (
    ("loadpath", "f:models/{iteration}"), ("savepath", "f:samples/{iteration}"), ("load_epoch", "latest"), ("n_samples_per_device", 4),
    ("pretrained_model", "duongna/stable-diffusion-v1-4-flax"), ("prompt_kwargs", {}), ("n_inference_steps", 50), ("eta", 1.0),
    ("resolution", 512), ("max_samples", 50e3), ("max_steps", None), ("local_size", 1600), ("guidance_scale", 5.0),
    ("filter_field", "labels"), ("mask_mode", "streaming_percentile"), ("mask_param", 95), ("identical_batch", False), ("iteration", 0),
    ("evaluate", False), ("cache", "cache"), ("seed", None),
)
_TRAIN_DEFAULTS = (
    ("modelpath", "f:models/{iteration}"), ("loadpath", "f:samples/{iteration}"), ("savepath", "f:models/{iteration+1}"),
    ("pretrained_model", "duongna/stable-diffusion-v1-4-flax"), ("finetuned_model", None), ("load_epoch", "latest"),
    ("max_train_samples", None), ("resolution", 512), ("train_cfg", False), ("guidance_scale", 5.0), ("train_batch_size", 2),
    ("num_train_epochs", 40), ("max_train_steps", None), ("learning_rate", 1e-5), ("beta1", 0.9), ("beta2", 0.999),
    ("weight_decay", 1e-4), ("epsilon", 1e-8), ("max_grad_norm", 1.0), ("iteration", 0), ("weighted_batch", False),
    ("weighted_dataset", False), ("dtype", "float32"), ("cache", "cache"), ("verbose", False), ("save_freq", 100),
    ("per_prompt_weights", False), ("seed", 0),
)

# engine-specific addition: the `dpo` experiment of pipeline/dpo.py, Diffusion-DPO on ranked pairs of the stored samples (Wallace et al.,
# "Diffusion Model Alignment Using Direct Preference Optimization").  The `train` keys without the RWR weighting, plus:
# dpo_beta 5000, the value the Diffusion-DPO authors ship for SD-1.5 with the error taken as a mean over the latent, as here — quoted from
# memory of their release and not measured in a training run on this engine; pair_seed, the seed of the pairing (epoch e pairs with
# pair_seed + e).  pair_seed is NOT offset by the rank (every host must build the same pairing); the parser offsets `seed`.
_DPO_DEFAULTS = tuple(kv for kv in _TRAIN_DEFAULTS if kv[0] not in ("weighted_batch", "weighted_dataset", "per_prompt_weights")) + (
    ("dpo_beta", 5000.0), ("pair_seed", 0),
)

base = {"sample": dict(_SAMPLE_DEFAULTS), "train": dict(_TRAIN_DEFAULTS), "pg": dict(_PG_DEFAULTS), "dpo": dict(_DPO_DEFAULTS)}

# engine-specific additions to experiments whose table above is held EQUAL to the reference's (`sample`, `train`): kept beside it, and read by
# the entry point's parser after the table and the dataset's overrides (pipeline/sample.py).  guidance_rescale: as in `pg` above.
_SAMPLE_ENGINE_DEFAULTS = (("guidance_rescale", 0.0),)
engine = {"sample": dict(_SAMPLE_ENGINE_DEFAULTS)}

# the two `sample` recipes of the reference's datasets: keep the top decile of 1024 identical-prompt batches (filter-finetune),
# or keep all of 10240 samples (reward-weighted regression)
_SAMPLE_TOP10 = {"max_samples": 1024, "mask_mode": "percentile", "mask_param": 90, "identical_batch": True}
_SAMPLE_ALL = {"max_samples": 10240, "mask_mode": "streaming_percentile", "mask_param": 0, "identical_batch": False}


def _train(train_cfg=True, train_batch_size=1, num_train_epochs=50, save_freq=20, **kw):
    return dict(train_cfg=train_cfg, train_batch_size=train_batch_size, num_train_epochs=num_train_epochs, save_freq=save_freq,
                dtype="float32", **kw)


_TRAIN_RWR = dict(num_train_epochs=5, weighted_dataset=True, temperature=1 / 5.0)


def _dataset(logdir, prompt_fn, filter_field, prompt_kwargs=None, sample=None, train=None, dpo=None, **pg):
    common = {"logbase": f"{user.bucket}/logs/{logdir}", "prompt_fn": prompt_fn, "filter_field": filter_field}
    if prompt_kwargs is not None:
        common["prompt_kwargs"] = prompt_kwargs
    out = {"common": common, "pg": pg}
    if sample is not None:
        out["sample"] = dict(sample)
    if train is not None:
        out["train"] = dict(train)
    if dpo is not None:
        out["dpo"] = dict(dpo)
    return out


_ANIMALS = {"loadpath": "assets/common_animals.txt"}
_NOUNS_ACTIVITIES = {"nouns_path": "assets/common_animals.txt", "activities_path": "assets/activities_v0.txt"}

compressed_animals = _dataset("identical-compressed-animals-s1024-p90", "imagenet_animals", "jpeg", sample=_SAMPLE_TOP10,
                              train=_train(train_batch_size=4))
neg_compressed_animals = _dataset("identical-neg-compressed-animals-s1024-p90", "imagenet_animals", "neg_jpeg", sample=_SAMPLE_TOP10,
                                  train=_train())
# reward-weighted regression on all samples (the RWR baseline of the paper)
compressed_animals_rwr = _dataset("rwr-compressed-animals-s10k", "imagenet_animals", "jpeg", sample=_SAMPLE_ALL, train=_train(**_TRAIN_RWR))
neg_compressed_animals_rwr = _dataset("rwr-neg-compressed-animals-s10k", "imagenet_animals", "neg_jpeg", sample=_SAMPLE_ALL,
                                      train=_train(**_TRAIN_RWR))
a_animals_rwr = _dataset("aesthetic_simple_animals_rwr_ppb", "from_file", "aesthetic", {"loadpath": "assets/common_animals.txt"},
                         sample=_SAMPLE_ALL, train=_train(train_batch_size=4, save_freq=10000000, per_prompt_weights=True, **_TRAIN_RWR))
# Diffusion-DPO on ranked pairs of all samples (pipeline/sample.py, then pipeline/dpo.py)
_DPO = dict(train_cfg=True, train_batch_size=4, num_train_epochs=5, save_freq=20, dtype="float32")
compressed_animals_dpo = _dataset("dpo-compressed-animals-s10k", "imagenet_animals", "jpeg", sample=_SAMPLE_ALL, dpo=_DPO)
a_animals_dpo = _dataset("aesthetic_simple_animals_dpo", "from_file", "aesthetic", _ANIMALS, sample=_SAMPLE_ALL, dpo=_DPO)
llava_vqa = _dataset("llava-vqa-v2", "vqa_dataset", "llava_vqa", {"loadpath": "assets/vqa_v2.txt"},
                     per_prompt_stats_bufsize=128, per_prompt_stats_min_count=32, num_train_epochs=120)
llava_counting = _dataset("llava-counting-v0-8", "counting", "llava_vqa",
                          {"nouns_path": "assets/very_simple_animals.txt", "number_range": (2, 8)})
llava_bertscore = _dataset("llava-bertscore-2-simple-animals", "nouns_activities", "llava_bertscore", _NOUNS_ACTIVITIES)
# prompt alignment without a server: CLIPScore on the engine's own CLIP towers (ddpo_amd/models/clip_score.py)
clip_nouns_activities = _dataset("clip-score-nouns-activities", "nouns_activities", "clip_score", _NOUNS_ACTIVITIES)
clip_animals = _dataset("clip-score-simple-animals", "from_file", "clip_score", _ANIMALS)
a_dog_1 = _dataset("aesthetic_dogs_sweep/one", "manual", "aesthetic", {"prompts": ["a dog"]}, per_prompt_stats_bufsize=None,
                   per_prompt_stats_min_count=None, train_batch_size=1, train_accumulation_steps=2)
a_dog_2 = _dataset("aesthetic_dogs_sweep/imagenet", "imagenet_dogs", "aesthetic", {}, train_batch_size=1,
                   train_accumulation_steps=2)
a_animals = _dataset("aesthetic_simple_animals", "from_file", "aesthetic", _ANIMALS, sample=_SAMPLE_TOP10, train=_train(),
                     train_batch_size=1, train_accumulation_steps=2)

# CFG-free ablations and the VQA-v0 prompt set of the reference (config/base.py of the reference, same names / overrides)
compressed_animals_nocfg = _dataset("nocfg-compressed-animals-s1024-p90", "imagenet_animals", "jpeg", sample=_SAMPLE_TOP10,
                                    train=_train(train_cfg=False, train_batch_size=2))
neg_compressed_animals_nocfg = _dataset("nocfg-neg-compressed-animals-s1024-p90", "imagenet_animals", "neg_jpeg", sample=_SAMPLE_TOP10,
                                        train=_train(train_cfg=False, train_batch_size=2))
vqa_v0 = _dataset("vqa-v0-n2k-s5.0-e50", "vqa_dataset", "vqa", {"loadpath": "assets/vqa_v0.txt"},
                  sample={"max_samples": 2e3, "mask_mode": "threshold", "mask_param": 0.65, "identical_batch": False},
                  train={"train_cfg": True, "train_batch_size": 1, "num_train_epochs": 50, "save_freq": 20})
