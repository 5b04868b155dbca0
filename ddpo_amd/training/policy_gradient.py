"""PPO-clip policy-gradient step on stored DDIM log-probs + gradient-accumulating train state.

Host-side mirror of /root/reference/ddpo/training/policy_gradient.py:
  AccumulatingTrainState :13-57, ADV_CLIP_MAX :60, train_step :63-146
and of the optimizer the entrypoint builds (/root/reference/pipeline/policy_gradient.py:130-150):
  optax.chain(clip_by_global_norm(max_grad_norm), adamw(lr, b1, b2, eps, weight_decay, mu_dtype=bf16)).

MI355X design notes
  * cond and uncond U-Net passes of `train_cfg` are run as ONE batch-2b pass ([uncond; cond] contexts, the same
    latents twice) — identical arithmetic per sample, half the launches, twice the rows per GEMM.
  * gradients are accumulated in place in one flat fp32 buffer by the wgrad kernels (grad_acc += g is free);
    `lax.pmean(grad)` of the reference (:141, every micro-step) becomes ONE RCCL all-reduce of that buffer per
    optimizer update — mean-over-ranks and sum-over-steps commute.
  * the update itself is one fused kernel: 1/(n_acc+1) scaling, global-norm clip, AdamW with bf16 first moment.
  * `--optimizer adafactor` (the table's second row, optax.adafactor(lr, weight_decay_rate)) is five launches over the same flat
    buffers, with a state of 1.9 M floats instead of 6 B/param (lib_optim.py).
  * `--kl_coef` (not in the reference): kl_coef * KL(policy || frozen pretrained policy) per DDIM step, a closed form in the two noise
    predictions.  One inference forward of the frozen copy (kl_reference.py) and one additive pass behind the PPO launch (lib_ppo_kl.py),
    both inside the captured step; with kl_coef == 0 neither exists and the step is the one above, launch for launch.
  * `--pg_loss d3po` (not in the reference): a DPO loss per DDIM step on adjacent row pairs ranked by preference, on the policy-to-pretrained
    log-ratio of each stored transition (lib_pref.py).  Its pass stands in the place of the PPO launch and reads the same
    frozen forward a KL penalty would; with the default `ppo` none of it is imported or launched.
  * `--guidance_rescale` (not in the reference): the policy is the RESCALED guided prediction the sampler ran (lib_cfg_rescale.py,
    DESIGN.md §4).  One launch between the U-Net forward and the loss passes, which then see a single prediction (their train_cfg = False
    form), and one between them and the U-Net backward; with guidance_rescale == 0 neither exists.
"""
import numpy as np
import torch

from .. import lib as L
from .. import lib_optim as LO

ADV_CLIP_MAX = 10.0
# PPO micro-steps per U-Net forward/backward in the entrypoint's training loop (train_steps_fused).  16 turns the U-Net batch of 4
# (2 samples x CFG) into 64 rows-of-latents = 1024 of the 256x320 GEMM tiles at the 64x64 level = exactly 4 rounds of the 256 CUs;
# round 1's default of 10 (batch 40 = 2.5 rounds) sat in a quantisation hole: 42.4 (k = 10) vs 44.1 (k = 8) vs 45.1 (k = 16)
# sample-timesteps/s on one box (profiles/r02_ab_train_fuse.log; k = 1: 28).  The default 50 timesteps run as 16 + 16 + 16 + 2.
# DDPO_TRAIN_FUSE=1 restores one launch per micro-step.
DEFAULT_TRAIN_FUSE = 16
LOSSES = ("ppo", "d3po")
D3PO_BETA = 0.1          # config/base.py `d3po_beta`: the D3PO authors' shipped value


def check_rescale_args(guidance_rescale, train_cfg):
    """The entrypoint's argument check, as a plain function: a message to exit with, or None.  `train_cfg` None: the sampling entry point,
    which always runs both halves."""
    import math
    phi = float(guidance_rescale)
    if not (math.isfinite(phi) and 0.0 <= phi <= 1.0):
        return f"--guidance_rescale must be a finite number in [0, 1], got {phi}"
    if phi > 0.0 and train_cfg is not None and not train_cfg:
        return (f"--guidance_rescale {phi} needs --train_cfg True: without the unconditional half of the prediction there is nothing to "
                f"rescale against")
    return None


def train_fuse_default(unet_rows_per_micro_step=None, latent_pixels=None):
    """Micro-steps per launch.  An explicit DDPO_TRAIN_FUSE is taken as is; the default of 16 is reduced for geometries whose
    activation tape would outgrow the footprint run on hardware (U-Net batch 64 at 64x64 latents = 262,144 latent pixels per
    launch): SD-2.1 at 96x96 latents fuses 7 micro-steps."""
    import os
    if "DDPO_TRAIN_FUSE" in os.environ:
        return max(1, int(os.environ["DDPO_TRAIN_FUSE"]))
    k = DEFAULT_TRAIN_FUSE
    if unet_rows_per_micro_step and latent_pixels:
        k = min(k, max(1, (64 * 4096) // (int(unet_rows_per_micro_step) * int(latent_pixels))))
    return k


class AdamWConfig:
    """Hyper-parameters of pipeline/policy_gradient.py:130-150 (defaults = config/base.py `pg`)."""

    name = "adamw"

    def __init__(self, learning_rate=1e-5, b1=0.9, b2=0.999, eps=1e-8, weight_decay=1e-4, max_grad_norm=1.0,
                 mu_decay_in_bf16=True):
        self.learning_rate, self.b1, self.b2, self.eps = learning_rate, b1, b2, eps
        self.weight_decay, self.max_grad_norm = weight_decay, max_grad_norm
        self.mu_decay_in_bf16 = mu_decay_in_bf16


class AdafactorConfig:
    """optax.adafactor(learning_rate, weight_decay_rate=weight_decay) behind clip_by_global_norm(max_grad_norm): the reference passes these two
    arguments and leaves the rest at optax's defaults (lib_optim.py).  min_dim_size_to_factor is optax's 128; small tests lower it."""

    name = "adafactor"

    def __init__(self, learning_rate=1e-5, weight_decay=1e-4, max_grad_norm=1.0, min_dim_size_to_factor=LO.MIN_DIM_SIZE_TO_FACTOR):
        self.learning_rate, self.weight_decay, self.max_grad_norm = learning_rate, weight_decay, max_grad_norm
        self.min_dim_size_to_factor = min_dim_size_to_factor


class AccumulatingTrainState:
    """TrainState that accumulates gradients over several steps before applying them (reference :13-57).

    fields: step, params (the U-Net's flat ParamStore), opt_state {count, mu (bf16), nu (fp32)}, grad_acc (flat), n_acc.
    With an AdafactorConfig opt_state is {count, v}: one flat fp32 buffer laid out by `plan` (lib_optim.AdafactorPlan).
    LoRA mode (`lora`: a models/lora.LoraStore attached to the U-Net): the optimizer state, the gradient buffer and the update are the
    adapters' (`trainable` = lora.params); after each update lora.merge() rewrites the adapted U-Net weights and repacks only those.
    """

    def __init__(self, unet, tx, process_group=None, lora=None):
        self.unet = unet
        self.apply_fn = unet.forward
        self.params = unet.params
        self.lora = lora
        if lora is not None and unet.lora is not lora:
            raise ValueError("the LoraStore must be attached to this U-Net (LoraStore(unet, ...))")
        self.trainable = unet.params if lora is None else lora.params
        self.tx = tx
        self.step = 0
        self.n_acc = 0
        self.grad_acc = unet.ensure_grads() if lora is None else lora.grads
        n = self.trainable.flat.numel()
        dev = self.trainable.flat.device
        if isinstance(tx, AdafactorConfig):
            self.plan = LO.AdafactorPlan.for_store(self.trainable, tx.min_dim_size_to_factor).to(dev)
            self.opt_state = {"count": 0, "v": self.plan.new_state()}
        else:
            self.opt_state = {"count": 0, "mu": torch.zeros(n, dtype=torch.bfloat16, device=dev),
                              "nu": torch.zeros(n, dtype=torch.float32, device=dev)}
        self._sqnorm = torch.zeros(1, dtype=torch.float64, device=dev)
        self.process_group = process_group
        self.last_grad_norm = None

    @classmethod
    def create(cls, *, unet, tx, **kw):
        return cls(unet, tx, **kw)

    def world(self):
        if self.process_group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()):
            return torch.distributed.get_world_size(self.process_group)
        return 1

    def overlap_bucketer(self):
        """A GradBucketer for the backward pass that closes an optimizer update (a process group exists — world > 1, or the forced one-rank
        group of the RCCL tests — and DDPO_GRAD_OVERLAP != 0), else None: its
        bucketed all-reduce runs on a side stream behind the rest of that backward (training/distributed.GradBucketer); the blocking
        single all-reduce below stays the path of graph-replayed steps and of DDPO_GRAD_OVERLAP=0."""
        import os
        from .distributed import GradBucketer, _through_backend
        # world 1 only under DDPO_FORCE_DIST=1 (a one-rank RCCL group: the side stream, the per-bucket async all_reduce and finish() all
        # execute on hardware, tests/test_gpu_rccl_single_rank.py); a plain single process has no process group and keeps graph replay
        if self.lora is not None or not _through_backend() or os.environ.get("DDPO_GRAD_OVERLAP", "1") == "0":
            # (LoRA: a few MB of adapter gradients — one blocking all-reduce in apply_gradients)
            return None
        mib = float(os.environ.get("DDPO_GRAD_BUCKET_MIB", "256"))      # 256 MiB = 14 buckets over the 3.44 GB SD-1.5 gradient
        return GradBucketer(self.grad_acc.flat, bucket_numel=int(mib * (1 << 20)) // 4, group=self.process_group)

    def apply_gradients(self, *, grads=None, do_update, reduced=False):
        """`grads` were already accumulated into grad_acc by the backward kernels (grads is accepted for signature
        parity and must be None or grad_acc itself).  reduced=True: the sum over ranks is already in the buffer (GradBucketer)."""
        assert grads is None or grads is self.grad_acc
        if not do_update:
            self.n_acc += 1
            return self
        g = self.grad_acc.flat
        world = self.world()
        if world > 1 and not reduced:
            # lax.pmean(grad, "batch"): one all-reduce(sum) of the flat buffer, the mean is folded into inv_n below
            torch.distributed.all_reduce(g, op=torch.distributed.ReduceOp.SUM, group=self.process_group)
        inv = 1.0 / ((self.n_acc + 1) * world)
        L.grad_sqnorm(g, self._sqnorm)
        t = self.opt_state["count"] + 1
        tx = self.tx
        if isinstance(tx, AdafactorConfig):
            LO.adafactor_step(self.trainable.flat, g, self.opt_state["v"], self.plan, self._sqnorm, inv, tx.learning_rate,
                              self.opt_state["count"], tx.weight_decay, tx.max_grad_norm, zero_grad=True)
        else:
            L.adamw_bf16mu_step(self.trainable.flat, g, self.opt_state["mu"], self.opt_state["nu"], self._sqnorm, inv,
                                tx.learning_rate, tx.b1, tx.b2, tx.eps, tx.weight_decay, tx.max_grad_norm, t,
                                mu_decay_in_bf16=tx.mu_decay_in_bf16, zero_grad=True)
        self.last_grad_norm = torch.sqrt(self._sqnorm.clone()) * inv       # device scalar, no host sync
        if self.lora is not None:
            self.lora.merge()                                              # W' = W0 + s A B; repack of the adapted tensors only
        elif L.current_datapath() != "fp32":
            self.params.pack_bf16()                                        # refresh the bf16 hi/lo weight planes
        self.opt_state["count"] = t
        self.step += 1
        self.n_acc = 0
        return self


def _fwd_bwd(state, batch, noise_scheduler_state, noise_scheduler, train_cfg, guidance_scale, eta, clip_range, group=None, on_ready=None,
             kl_coef=0.0, ref_unet=None, loss="ppo", d3po_beta=None, guidance_rescale=0.0):
    """U-Net forward (cond + uncond as one batch), scoring-mode log-prob + PPO-clip forward/backward, U-Net backward
    (parameter gradients accumulate in place).  Pure device work: capturable into a HIP graph.
    `group`: rows per PPO micro-batch when the batch holds several micro-batches (train_steps_fused); info is then (k, 3).
    kl_coef > 0: `ref_unet` (kl_reference.KLReference) runs its inference forward on the same rows and the KL pass adds the penalty's
    gradient to the PPO gradient and kl_coef * kl to info's loss column; the third result is the per-micro-batch KL (else None).
    loss == "d3po": the preference-pair pass (lib_pref.py) stands in the place of the PPO launch; batch["advantages"] carries the labels
    (+1 winner, -1 loser, 0 tie; rows in adjacent pairs), batch["log_probs"] is not read, info is {pref_acc, pref_margin, loss} and the second
    result is per_pair (b / 2, 4).  The one frozen forward serves this pass and the KL pass alike.
    guidance_rescale > 0 (needs train_cfg): the policy's prediction, and the frozen one's, is the rescaled guided prediction of
    lib_cfg_rescale.cfg_rescale_fwd; the passes above run on it in their train_cfg = False form and cfg_rescale_bwd turns its cotangent
    into those of the two U-Net halves."""
    bad = check_rescale_args(guidance_rescale, train_cfg)
    if bad:
        raise ValueError(bad.replace("--", ""))
    rescale = float(guidance_rescale)
    if loss not in LOSSES:
        raise ValueError(f"loss must be one of {LOSSES}, got {loss!r}")
    d3po = loss == "d3po"
    if not kl_coef >= 0:
        raise ValueError(f"kl_coef must be >= 0, got {kl_coef}")
    if kl_coef > 0 and ref_unet is None:
        raise ValueError("kl_coef > 0 needs ref_unet: the frozen pretrained policy (training/kl_reference.KLReference)")
    if d3po and ref_unet is None:
        raise ValueError("loss 'd3po' needs ref_unet: the frozen pretrained policy (training/kl_reference.KLReference)")
    need_ref = d3po or kl_coef > 0
    unet = state.unet
    lat = batch["latents"]
    b = lat.shape[0]
    ts = batch["ts"]
    tape = []
    if train_cfg:
        lat2 = torch.cat([lat, lat])
        ctx2 = torch.cat([batch["uncond_embeds"], batch["prompt_embeds"]]).contiguous()
        ts2 = torch.cat([ts, ts])
        out = unet.forward(lat2, ts2, ctx2, tape=tape)
        eps_u, eps_c = out[:b].contiguous(), out[b:].contiguous()
        if need_ref:
            rout = ref_unet.forward(lat2, ts2, ctx2)
            ref_u, ref_c = rout[:b].contiguous(), rout[b:].contiguous()
    else:
        out = unet.forward(lat, ts, batch["prompt_embeds"], tape=tape)
        eps_u, eps_c = None, out
        if need_ref:
            ref_u, ref_c = None, ref_unet.forward(lat, ts, batch["prompt_embeds"])
    consts = noise_scheduler.kernel_consts(noise_scheduler_state, eta)
    loss_cfg = train_cfg
    if rescale > 0:
        from .. import lib_cfg_rescale as LR
        pol_c, pol_u = eps_c, eps_u
        eps_c, rstats = LR.cfg_rescale_fwd(pol_c, pol_u, guidance_scale, rescale)
        if need_ref:
            ref_c, _ = LR.cfg_rescale_fwd(ref_c, ref_u, guidance_scale, rescale)
        eps_u = ref_u = None
        loss_cfg = False                        # the passes below see ONE prediction: the rescaled one
    if d3po:
        from .. import lib_pref as LP
        d_c, d_u, per_sample, info = LP.ddim_pref_fwd_bwd(eps_c, eps_u, ref_c, ref_u, lat, batch["next_latents"], ts, batch["advantages"],
                                                          guidance_scale, D3PO_BETA if d3po_beta is None else d3po_beta, loss_cfg, consts,
                                                          group=group)
    else:
        d_c, d_u, per_sample, info = L.ddim_logprob_ppo_fwd_bwd(eps_c, eps_u, lat, batch["next_latents"], ts, batch["log_probs"],
                                                                batch["advantages"], guidance_scale, clip_range, loss_cfg, consts,
                                                                group=group)
    kl = None
    if kl_coef > 0:
        from .. import lib_ppo_kl as LK
        _, kl = LK.ddim_kl_ref_fwd_bwd(eps_c, eps_u, ref_c, ref_u, ts, guidance_scale, kl_coef, loss_cfg, consts, d_c, d_u, loss_info=info,
                                       group=group)
    if rescale > 0:
        d_c, d_u = LR.cfg_rescale_bwd(pol_c, pol_u, d_c, rstats, guidance_scale, rescale)
    d_out = torch.cat([d_u, d_c]) if train_cfg else d_c
    unet.backward(tape, d_out, on_ready=on_ready)
    return info, per_sample, kl


_KEYS = ("latents", "next_latents", "ts", "log_probs", "advantages", "prompt_embeds", "uncond_embeds")


def _graphed_fwd_bwd(state, batch, sched_state, sched, train_cfg, guidance_scale, eta, clip_range, group=None, kl_coef=0.0, ref_unet=None,
                     loss="ppo", d3po_beta=None, guidance_rescale=0.0):
    """Replay of _fwd_bwd as a captured HIP graph (one per batch geometry / hyper-parameter set): ~3000 kernel launches per
    micro-step become one graph launch.  Gradients still accumulate into the same flat buffer."""
    key = (tuple(batch["latents"].shape), tuple(batch["prompt_embeds"].shape), bool(train_cfg), float(guidance_scale), float(eta),
           float(clip_range), sched_state.num_inference_steps, L.current_datapath(), group,
           0 if state.lora is None else state.lora.rank, float(kl_coef), ref_unet is not None)
    klkw = dict(kl_coef=kl_coef, ref_unet=ref_unet)
    if loss != "ppo":
        key += (loss, float(D3PO_BETA if d3po_beta is None else d3po_beta))
        klkw.update(loss=loss, d3po_beta=d3po_beta)
    if guidance_rescale > 0:
        key += ("guidance_rescale", float(guidance_rescale))
        klkw.update(guidance_rescale=float(guidance_rescale))
    cache = state.__dict__.setdefault("_graphs", {})
    ent = cache.get(key)
    if ent == "eager":
        return _fwd_bwd(state, batch, sched_state, sched, train_cfg, guidance_scale, eta, clip_range, group, **klkw)
    if ent is None:
        static = {k: batch[k].clone() for k in _KEYS}
        gflat = state.grad_acc.flat
        saved = gflat.clone()
        side = torch.cuda.Stream(gflat.device)
        side.wait_stream(torch.cuda.current_stream(gflat.device))
        with torch.cuda.stream(side):
            _fwd_bwd(state, static, sched_state, sched, train_cfg, guidance_scale, eta, clip_range, group, **klkw)      # warm-up (allocations, attrs)
        torch.cuda.current_stream(gflat.device).wait_stream(side)
        try:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                info, per_sample, kl = _fwd_bwd(state, static, sched_state, sched, train_cfg, guidance_scale, eta, clip_range, group, **klkw)
        except Exception as exc:                # capture is an optimisation only: fall back to eager launches, loudly
            print(f"[ ddpo_amd ] WARNING: HIP-graph capture of train_step failed ({type(exc).__name__}: {exc}); launching eagerly")
            torch.cuda.synchronize(gflat.device)
            gflat.copy_(saved)
            cache[key] = "eager"
            return _fwd_bwd(state, batch, sched_state, sched, train_cfg, guidance_scale, eta, clip_range, group, **klkw)
        gflat.copy_(saved)                      # warm-up passes must not leak into the accumulated gradients
        ent = (graph, static, info, per_sample, kl)
        cache[key] = ent
    graph, static, info, per_sample, kl = ent
    for k in _KEYS:
        static[k].copy_(batch[k])
    graph.replay()
    return info.clone(), per_sample.clone(), None if kl is None else kl.clone()


def _loss_kwargs(kl_coef, ref_unet, loss, d3po_beta, guidance_rescale=0.0):
    """Keyword arguments of _fwd_bwd beyond the default step's: none at all for PPO without a penalty and without rescale."""
    if loss not in LOSSES:
        raise ValueError(f"loss must be one of {LOSSES}, got {loss!r}")
    kw = dict(kl_coef=float(kl_coef), ref_unet=ref_unet) if kl_coef > 0 else {}
    if loss != "ppo":
        kw.update(loss=loss, d3po_beta=d3po_beta, ref_unet=ref_unet)
    if guidance_rescale > 0:
        kw.update(guidance_rescale=float(guidance_rescale))
    return kw


def _with_log_probs(batch, loss):
    """d3po never reads the stored log-probs: a batch without them gets a placeholder so the static graph inputs keep one layout."""
    if loss == "ppo" or "log_probs" in batch:
        return batch
    return dict(batch, log_probs=torch.zeros_like(batch["advantages"], dtype=torch.float32))


def _info_dict(loss, info, per_sample, rows=None):
    """One micro-batch's info row as the dict train_step returns.  `rows`: its slice of the per-row results (fused steps)."""
    if loss == "d3po":
        return {"pref_acc": info[0], "pref_margin": info[1], "loss": info[2]}
    return {"approx_kl": info[0], "clipfrac": info[1], "loss": info[2], "log_prob": per_sample[:, 0] if rows is None else per_sample[rows, 0]}


def train_step(state: AccumulatingTrainState, batch, noise_scheduler_state, noise_scheduler, train_cfg, guidance_scale,
               eta, clip_range, do_opt_update, jit=True, kl_coef=0.0, ref_unet=None, loss="ppo", d3po_beta=None, guidance_rescale=0.0):
    """One PPO micro-step (reference :63-146).  batch: latents, next_latents (b,4,h,w), ts (b,) int32, log_probs,
    advantages (b,), prompt_embeds, uncond_embeds (b,77,D) — device tensors.  Returns (state, info) with info a dict
    of device scalars {approx_kl, clipfrac, loss}.
    kl_coef > 0 (with ref_unet, the frozen pretrained policy): loss includes kl_coef * KL to it and info gains "kl_ref", that KL.
    loss="d3po" (with ref_unet): rows are adjacent preference pairs, batch["advantages"] their labels (+1 / -1 / 0), batch["log_probs"] is
    ignored and may be absent; info is {pref_acc, pref_margin, loss} (+ kl_ref), d3po_beta the DPO temperature (default D3PO_BETA).
    guidance_rescale > 0 (with train_cfg): the value the sampler ran with; log-prob, ratio, KL and log-ratio are the rescaled prediction's."""
    klkw = _loss_kwargs(kl_coef, ref_unet, loss, d3po_beta, guidance_rescale)
    assert isinstance(state, AccumulatingTrainState)
    b = batch["latents"].shape[0]
    assert b == batch["ts"].shape[0] == batch["next_latents"].shape[0] == batch["advantages"].shape[0]
    batch = _with_log_probs(batch, loss)
    assert b == batch["log_probs"].shape[0]
    dbatch = {k: batch[k].contiguous() for k in _KEYS if k in batch}
    dbatch["ts"] = dbatch["ts"].to(torch.int32)
    if not train_cfg and "uncond_embeds" not in dbatch:
        dbatch["uncond_embeds"] = dbatch["prompt_embeds"]
    bucketer = state.overlap_bucketer() if do_opt_update else None
    if bucketer is not None:
        info, per_sample, kl = _fwd_bwd(state, dbatch, noise_scheduler_state, noise_scheduler, train_cfg, guidance_scale, eta, clip_range,
                                        on_ready=bucketer.ready, **klkw)
        bucketer.finish()
    elif jit:
        info, per_sample, kl = _graphed_fwd_bwd(state, dbatch, noise_scheduler_state, noise_scheduler, train_cfg, guidance_scale, eta, clip_range,
                                                **klkw)
    else:
        info, per_sample, kl = _fwd_bwd(state, dbatch, noise_scheduler_state, noise_scheduler, train_cfg, guidance_scale, eta, clip_range, **klkw)
    state = state.apply_gradients(do_update=do_opt_update, reduced=bucketer is not None)
    out = _info_dict(loss, info, per_sample)
    if kl is not None:
        out["kl_ref"] = kl
    return state, out


def train_steps_fused(state: AccumulatingTrainState, batches, noise_scheduler_state, noise_scheduler, train_cfg, guidance_scale,
                      eta, clip_range, do_opt_update, jit=True, kl_coef=0.0, ref_unet=None, loss="ppo", d3po_beta=None, guidance_rescale=0.0):
    """k consecutive PPO micro-steps that see the SAME parameters — no optimizer update between them, i.e. any run of
    `train_step(..., do_opt_update=False)` calls optionally closed by one with `do_opt_update=True` — executed as ONE U-Net
    forward/backward over the concatenated rows.  The reference runs them one by one and sums their gradients in
    `AccumulatingTrainState.apply_gradients` (/root/reference/ddpo/training/policy_gradient.py:32-48; the entrypoint loop
    /root/reference/pipeline/policy_gradient.py:407-441 updates only at the last timestep of a mini-batch); summing inside
    one launch is the same arithmetic up to fp32 summation order, with 4x..16x more rows per GEMM (a micro-batch of 2
    samples x CFG is a U-Net batch of 4 — too small to fill 256 CUs).  Each micro-batch keeps its own mean loss
    (`ddpo_ddim_logprob_ppo_fwd_bwd` with `group`) and its own info row, and n_acc advances by k.

    batches: list of k dicts as for `train_step`, all with the same shapes.  `do_opt_update` applies after the LAST one.
    `loss` / `d3po_beta` / `guidance_rescale` as for `train_step`: with "d3po" every micro-batch is a whole number of adjacent preference
    pairs; the rescale is per row, so the fused rows need nothing of their own.
    Returns (state, [info_0, ..., info_{k-1}])."""
    assert isinstance(state, AccumulatingTrainState)
    k = len(batches)
    assert k >= 1
    if k == 1:
        state, info = train_step(state, batches[0], noise_scheduler_state, noise_scheduler, train_cfg, guidance_scale, eta,
                                 clip_range, do_opt_update, jit=jit, kl_coef=kl_coef, ref_unet=ref_unet, loss=loss, d3po_beta=d3po_beta,
                                 guidance_rescale=guidance_rescale)
        return state, [info]
    klkw = _loss_kwargs(kl_coef, ref_unet, loss, d3po_beta, guidance_rescale)
    batches = [_with_log_probs(bt, loss) for bt in batches]
    b = batches[0]["latents"].shape[0]
    for bt in batches:
        assert bt["latents"].shape == batches[0]["latents"].shape and bt["ts"].shape[0] == b
    if not train_cfg:
        batches = [dict(bt, uncond_embeds=bt.get("uncond_embeds", bt["prompt_embeds"])) for bt in batches]
    dbatch = {key: torch.cat([bt[key] for bt in batches]).contiguous() for key in _KEYS}
    dbatch["ts"] = dbatch["ts"].to(torch.int32)
    bucketer = state.overlap_bucketer() if do_opt_update else None
    if bucketer is not None:
        # the launch that closes an optimizer update runs eagerly, with the bucketed gradient all-reduce hanging on the backward's progress
        info, per_sample, kl = _fwd_bwd(state, dbatch, noise_scheduler_state, noise_scheduler, train_cfg, guidance_scale, eta, clip_range, b,
                                        on_ready=bucketer.ready, **klkw)
        bucketer.finish()
    else:
        fn = _graphed_fwd_bwd if jit else _fwd_bwd
        info, per_sample, kl = fn(state, dbatch, noise_scheduler_state, noise_scheduler, train_cfg, guidance_scale, eta, clip_range, b, **klkw)
    for _ in range(k - 1):
        state = state.apply_gradients(do_update=False)
    state = state.apply_gradients(do_update=do_opt_update, reduced=bucketer is not None)
    return state, [dict(_info_dict(loss, info[j], per_sample, slice(j * b, (j + 1) * b)), **({} if kl is None else {"kl_ref": kl[j]}))
                   for j in range(k)]
