/* ddpo_hip.h — C ABI of libddpo_hip.so: the MI355X (gfx950) kernels behind the DDPO hot path.
 *
 * The reference (jannerm/ddpo) is pure Python/JAX and has no FFI boundary of its own; every entry point
 * below names the reference call site (file:line under /root/reference) whose arithmetic it replaces.
 * Conventions: all pointers are DEVICE pointers owned by the caller unless marked "host"; tensors are
 * fp32 unless stated; `stream` is a hipStream_t passed as void*; functions never allocate, never
 * synchronise and never throw; they return 0 on success, DDPO_EINVAL (-1) for a bad argument and
 * DDPO_ELAUNCH (-2) if the launch was rejected.  Activations are NHWC ("pixel-major") inside the U-Net,
 * latents/trajectories are NCHW at rest exactly as the reference stores them.
 */
#ifndef DDPO_HIP_H
#define DDPO_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DDPO_OK 0
#define DDPO_EINVAL (-1)
#define DDPO_ELAUNCH (-2)

#define DDPO_PRED_EPSILON 0
#define DDPO_PRED_V 1
#define DDPO_PRED_SAMPLE 2

int ddpo_abi_version(void);
size_t ddpo_sizeof_gemm_desc(void);     /* for binding self-checks (ctypes / cffi struct mirrors) */
size_t ddpo_sizeof_ddim_consts(void);
/* ABI v10.  Cumulative HOST-side launch counts of the bf16-MFMA GEMM / conv template per tile class since the library was loaded (out_host:
 * n >= 8 counters): [0] 256x320 "tall", [1] 128x320 "wide", [2] 128x128, [3] 128x64, [4] launches that fell back to the pointer-addressed
 * generic loader, [5] split-K reduce passes, [6] launches of the f16mx (NPASS = 4) instantiation (also counted under their tile), [7] 0.
 * Introspection only (which instantiation a layer geometry is routed to is otherwise invisible to the caller); kernels replayed from a
 * captured HIP graph are counted once, at capture. */
int ddpo_gemm_tile_launch_counts(unsigned long long* out_host, int n);
/* Additive to ABI v14.  The shortest reduction, in 32-wide k-tiles, for which the forward GEMM / conv dispatcher considers a split-K at all.  The
 * split factor follows the launch's row count, so a caller that runs a layer on PART of a batch and needs the bits of the whole-batch launch
 * (the CFG-shared front of the sampling U-Net) may do so only for layers with K / 32 below this value. */
int ddpo_gemm_splitk_min_ktiles(void);

/* ---- PRNG: jax.random (Threefry-2x32) -------------------------------------------------------------
 * jax.random.split / PRNGKey bookkeeping, pipeline/policy_gradient.py:51,201,244-245 and
 * ddpo/diffusers_patch/pipeline_flax_stable_diffusion.py:196,232,252.  Host-side, integer-exact. */
int ddpo_threefry_bits_host(uint32_t k0, uint32_t k1, int64_t n, uint32_t* out_host);
/* jax.random.normal(key, shape, float32) flattened to n elements:
 * pipeline_flax_stable_diffusion.py:197 (initial latents), scheduling_ddim_flax.py:347 (step noise).
 * bits_out (optional, may be NULL) receives the raw uint32 words for bit-exact checks. */
int ddpo_threefry_normal(uint32_t k0, uint32_t k1, float* out, uint32_t* bits_out, int64_t n, void* stream);

/* ---- DDIM scheduler ------------------------------------------------------------------------------
 * Scheduler constants shared by both DDIM kernels: alphas_cumprod is the device table ᾱ[0..T_train),
 * final_alpha_cumprod / step_ratio / eta / pred_type as in scheduling_ddim_flax.py:154-158,279-281,325. */
typedef struct {
  const float* alphas_cumprod;   /* device, num_train_timesteps floats */
  int num_train_timesteps;
  int step_ratio;                /* num_train_timesteps / num_inference_steps */
  float final_alpha_cumprod;
  float eta;
  int pred_type;                 /* DDPO_PRED_* */
} ddpo_ddim_consts;

/* Sampling-mode FlaxDDIMScheduler.step fused with the CFG combine:
 * pipeline_flax_stable_diffusion.py:226-235 + scheduling_ddim_flax.py:279-359.
 *   eps = eps_u + g (eps_c - eps_u);  x_next = mu(eps, x, t) + sigma z;  logp[b] = mean_chw N(x_next; mu, sigma_c)
 * eps_u/eps_c/x/z/x_next: (B, chw) contiguous; ts: (B,) int32 device; logp: (B,). */
int ddpo_ddim_step_fwd(const float* eps_u, const float* eps_c, const float* x, const float* z,
                       const int32_t* ts, float guidance_scale, const ddpo_ddim_consts* c,
                       float* x_next, float* logp, int B, int chw, void* stream);

/* Scoring-mode step + PPO-clip loss + its gradient w.r.t. the two U-Net outputs:
 * ddpo/training/policy_gradient.py:95-125 (forward), jax.grad of it (:138-139) down to d eps_c / d eps_u.
 * per_sample: (B,4) = {log_prob, ratio, max(unclipped,clipped), clipped?}; info: {approx_kl, clipfrac, loss} (:132-134).
 * If train_cfg == 0, eps_u/d_eps_u may be NULL.
 * The B rows are B/group micro-batches scored at once: rows [j*group, (j+1)*group) form micro-batch j (group >= 1, B % group == 0,
 * DDPO_EINVAL otherwise; group == B: one batch, info is 3 floats).  Each micro-batch's loss is the mean over ITS `group` rows, so the
 * gradients written are exactly those B/group separate calls would write (AccumulatingTrainState sums them anyway,
 * ddpo/training/policy_gradient.py:32-48), and info is (B/group, 3): one {approx_kl, clipfrac, loss} per micro-batch. */
int ddpo_ddim_logprob_ppo_fwd_bwd(const float* eps_c, const float* eps_u, const float* x,
                                  const float* x_next, const int32_t* ts, const float* old_logp,
                                  const float* advantages, float guidance_scale, float clip_range,
                                  int train_cfg, const ddpo_ddim_consts* c, float* d_eps_c,
                                  float* d_eps_u, float* per_sample, float* info, int B, int group,
                                  int chw, void* stream);

/* ---- optimizer: optax.chain(clip_by_global_norm, adamw(mu_dtype=bf16)) + AccumulatingTrainState ----
 * pipeline/policy_gradient.py:130-150; ddpo/training/policy_gradient.py:32-48. */
/* RWR baseline (reward-weighted regression, /root/reference/ddpo/training/diffusion.py:19-90).
 * ddpo_rwr_noisy_latents: moments (B,h,w,2C) NHWC = the stored VAE posterior (mean | logvar), e1 (B,h,w,C) NHWC and noise (B,C,h,w)
 *   NCHW standard normals, ts (B) int32 -> latents = (mean + exp(clip(logvar,-30,20)/2) e1) * scale and
 *   noisy = sqrt(acp[t]) latents + sqrt(1 - acp[t]) noise, both (B,C,h,w) NCHW (FlaxDDPMScheduler.add_noise).
 * ddpo_rwr_mse_fwd_bwd: eps_c / eps_u / noise (B, chw); noise_pred = eps_u + g (eps_c - eps_u) if train_cfg else eps_c;
 *   per_sample (B,2) = {mean_chw (noise - noise_pred)^2, w_b * that}; *loss = sum_b w_b loss_b with w_b = weights[b], or 1/B when
 *   weights == NULL (the batch mean); d_eps_c / d_eps_u = d loss / d eps (closed form).  One workgroup per sample, no atomics. */
int ddpo_rwr_noisy_latents(const float* moments, const float* e1, const float* noise, const int32_t* ts,
                           const float* alphas_cumprod, int num_train_timesteps, float scale, float* latents, float* noisy,
                           int B, int C, int hw, void* stream);
int ddpo_rwr_mse_fwd_bwd(const float* eps_c, const float* eps_u, const float* noise, const float* weights, float guidance_scale,
                         int train_cfg, float* d_eps_c, float* d_eps_u, float* per_sample, float* loss, int B, int chw,
                         void* stream);
/* out_sq (device double, must be zeroed by the caller or zero_first=1) += sum g^2 */
int ddpo_grad_sqnorm(const float* g, int64_t n, double* out_sq, int zero_first, void* stream);
/* One update over flat buffers.  g holds the SUM of accumulated grads; inv_n_acc = 1/(n_acc+1);
 * sqnorm_of_sum = device double holding sum(g^2) of that SUM (the kernel applies inv_n_acc itself).
 * mu is bf16 (uint16), nu fp32.  step_t is the new count (>=1).  If zero_grad, g is cleared. */
int ddpo_adamw_bf16mu_step(float* p, float* g, uint16_t* mu, float* nu, int64_t n,
                           const double* sqnorm_of_sum, double inv_n_acc, double lr, double b1, double b2,
                           double eps, double weight_decay, double max_grad_norm, int step_t,
                           int mu_decay_in_bf16, int zero_grad, void* stream);

/* ---- U-Net / VAE building blocks (diffusers FlaxUNet2DConditionModel.apply / FlaxAutoencoderKL.decode;
 *      call sites pipeline_flax_stable_diffusion.py:219-224, ddpo/training/policy_gradient.py:87-102,
 *      pipeline/policy_gradient.py:174-182) --------------------------------------------------------- */

/* GroupNorm(+SiLU) over NHWC x:(B,HW,C) with row stride ldx/ldy (floats).
 * ws: 16-byte aligned scratch of ddpo_groupnorm_ws_bytes(B,HW,C,G) bytes (per-chunk group sums).
 * stats: 16-byte aligned OUTPUT of ddpo_groupnorm_stats_floats(B,C,G) floats = per-(b,c) affine {rstd*gamma,
 * beta-mean*rstd*gamma} followed by per-(b,g) {mean, rstd}; the backward pass reads it.
 * Reductions run in a fixed order: results are bit-reproducible. */
size_t ddpo_groupnorm_ws_bytes(int B, int HW, int C, int G);
size_t ddpo_groupnorm_stats_floats(int B, int C, int G);
int ddpo_groupnorm_fwd(const float* x, int ldx, float* y, int ldy, const float* gamma, const float* beta,
                       int B, int HW, int C, int G, float eps, int fuse_silu, void* ws, float* stats, void* stream);
/* Same, but the result is written as bf16 hi / lo planes (B*HW, ldy) — hi = bf16(y), lo = bf16(y - hi) — the activation
 * operand format of ddpo_gemm_conv_fwd_bf16_planes (the fp32 tensor is not materialised; same bytes).
 * ACTIVATION-PLANE LAYOUTS (ABI v6; every function that writes or reads activation planes takes the same convention through its
 * plane row stride ldy / ld_out / ld_planes / lda / ld_src / ld_w):  ld > 0: row-major (rows, ld);  ld == 0: k-blocked
 * (C / 32, rows, 32), C % 32 == 0 — the 32 channels of one k-tile of consecutive rows are consecutive memory, so every 1 KiB
 * LDS-DMA piece of the plane-fed GEMM (16 consecutive rows x 64 B) is 8 full cache lines instead of 16 half lines.  `rows` is the
 * row count of the tensor the planes describe: B*HW here, `rows` / M elsewhere, B*H*W source pixels for a convolution's input.
 * PLANE FORMAT (ABI v9): bit 1 of `fuse_silu` here (values 2 / 3) and bit 1 of `kblocked` in ddpo_layernorm_fwd_planes select the f16mx
 * format instead of bf16 hi / lo: y_hi = f16(y), y_lo = the interleaved e5m2 chunks of ddpo_split_planes_f16mx (C, ldy % 32 == 0) —
 * the operand of ddpo_gemm_conv_fwd_f16mx_planes, bit for bit what ddpo_split_planes_f16mx would make of the fp32 result. */
int ddpo_groupnorm_fwd_planes(const float* x, int ldx, uint16_t* y_hi, uint16_t* y_lo, int ldy, const float* gamma,
                              const float* beta, int B, int HW, int C, int G, float eps, int fuse_silu, void* ws,
                              float* stats, void* stream);
/* Backward of y = act(GroupNorm(x)): dx (+= dx_add if given), dgamma/dbeta accumulated atomically (they live in the
 * flat gradient buffer).  ws: ddpo_groupnorm_bwd_ws_bytes(B,HW,C,G) bytes. */
size_t ddpo_groupnorm_bwd_ws_bytes(int B, int HW, int C, int G);
int ddpo_groupnorm_bwd(const float* x, int ldx, const float* dy, int lddy, const float* stats, const float* gamma,
                       int B, int HW, int C, int G, int fuse_silu, const float* dx_add, int ld_add, float* dx, int lddx,
                       float* dgamma, float* dbeta, void* ws, void* stream);
/* LayerNorm over the last dim: x,y:(rows,C) contiguous. */
int ddpo_layernorm_fwd(const float* x, float* y, const float* gamma, const float* beta, int rows, int C,
                       float eps, void* stream);
int ddpo_layernorm_fwd_planes(const float* x, uint16_t* y_hi, uint16_t* y_lo, const float* gamma, const float* beta,
                              int rows, int C, float eps, int kblocked, void* stream);      /* planes (rows, C), or k-blocked (C/32, rows, 32) */
/* dx = LayerNorm backward (+ dx_add if given; statistics recomputed from x); dgamma/dbeta += (two-stage reduction
 * through ws = ddpo_layernorm_bwd_ws_bytes(rows, C) bytes of 16-byte aligned scratch). */
size_t ddpo_layernorm_bwd_ws_bytes(int rows, int C);
int ddpo_layernorm_bwd(const float* x, const float* dy, const float* gamma, int rows, int C, float eps,
                       const float* dx_add, float* dx, float* dgamma, float* dbeta, void* ws, void* stream);

/* Implicit-GEMM convolution / dense GEMM on the exact-fp32 MFMA datapath (v_mfma_f32_32x32x2_f32).
 *   out[m][n] = alpha * sum_k A(m,k) * W[k][n] (+ bias[n]) (+ rowbias[m / rows_per_batch][n]) (+ residual[m][n])
 * conv mode: m = (b, oy, ox), k = (ky, kx, ci); src is NHWC with pixel stride ld_src; optional nearest-2x
 * upsampling (upsample=1) of the source folded into the gather (FlaxUpsample2D), stride 1|2, pad 0|1, ksize 1|3
 * (upsample = 3 / ksize = 2 are what ddpo_conv_up2x_folded_fwd hands its kernels: not accepted from callers).
 * dense mode (ksize==0): A = src (M,K) with row stride ld_src.
 * W is (K, N) row-major (Flax HWIO / (in,out) layout) unless w_trans, then (N, K). */
typedef struct {
  const float* src; int ld_src;
  const float* w; int w_trans;
  const float* bias;              /* (N) or NULL */
  const float* rowbias; int rows_per_batch; int ld_rowbias;   /* (Bt, N): time-embedding add, or NULL */
  const float* residual; int ld_res;                          /* (M, N) or NULL */
  float* out; int ld_out;
  float alpha;
  int M, N, K;
  /* conv geometry (ksize==0 => dense) */
  int ksize, stride, pad, upsample;
  int B, H, W, Cin;               /* source dims (before upsample) */
  int OH, OW;
  /* backward-only fields (zero for the forward pass) */
  int w_dgrad;                    /* with w_trans: w is the FORWARD HWIO kernel (taps, N, Cin); taps are flipped -> data gradient */
  int ld_w;                       /* wgrad: row stride of dY (the `w` operand) */
  int splits;                     /* wgrad: split of the reduction over M (0 = auto) */
  int accumulate;                 /* wgrad: atomically add into out instead of storing */
  /* fused output stage (ddpo_gemm_conv_fwd_bf16 only; 0 everywhere else) */
  int epilogue;                   /* 0: out = alpha*acc + bias + rowbias + residual (N columns)
                                     1: GEGLU.  The N columns of W / bias come as interleaved 32-column blocks
                                        [a_0 | gate_0 | a_1 | gate_1 ...]; out has N/2 columns,
                                        out[:, 32q + c] = (acc_a + bias_a) * gelu_tanh(acc_gate + bias_gate);
                                        needs N % 128 == 0, K % 32 == 0, no rowbias / residual, alpha == 1
                                     2: GEGLU on the 256 x 320 tile (ABI v13; ddpo_gemm_conv_fwd_bf16_planes with both planes, and
                                        ddpo_gemm_conv_fwd_f16mx_planes with its cross terms on a dense layer).  The columns of W / bias come
                                        as 320-column blocks [a (160) | gate (160)]: block t holds the value and gate columns of the output
                                        columns 160 t .. 160 t + 159; same formula, bit-identical results (aux_out included); needs N % 320 == 0 */
  /* plane-emitting output stage (ddpo_gemm_conv_fwd_bf16 / _planes on the buffer-addressed kernels only; NULL elsewhere).
   * When out_hi != NULL the final value v of every output element is ALSO written as bf16 hi / lo planes
   * (hi = bf16(v), lo = bf16(v - hi): the operand format of ddpo_gemm_conv_fwd_bf16_planes, bit for bit what the
   * fp32-fed loader would split v into), rows of ld_planes elements (% 4 == 0, planes 8-byte aligned).  `out` may then be
   * NULL (planes only).  Needs the vector output stage (N, ld_out, ld_res, ld_rowbias % 4 == 0, 16-byte aligned
   * pointers); DDPO_EINVAL otherwise.  With epilogue == 1 / 2 the planes hold the N/2 GEGLU outputs. */
  uint16_t* out_hi; uint16_t* out_lo; int ld_planes;
  /* layout of the forward weight planes handed to ddpo_gemm_conv_fwd_bf16 / _planes (ABI v6):
   *   0: row-major (N, ldw) bf16, k contiguous per output column (ddpo_pack_weights_bf16);
   *   1: k-blocked (ceil(Kp / 32), N, 32) bf16 (ddpo_pack_weights_bf16_kblocked): the 32 k of one k-tile of all N columns are ONE
   *      contiguous block, so a 1 KiB LDS-DMA piece of the weight operand (16 columns x 64 B) is 1 KiB of consecutive memory =
   *      8 full 128-byte cache lines instead of 16 half lines at the row stride — the weight stream of the k-loop measured
   *      1.25-1.4x faster per CU (tools/native/dma_bench, profiles/r03_dma_bench.log).  `ldw` is ignored.  Not with w_dgrad. */
  int w_layout;
  /* f16mx datapath (ABI v7; ddpo_gemm_conv_fwd_f16mx_planes only, zero elsewhere): one E8M0 scale byte per output column of the
   * 8-bit weight plane (ddpo_pack_weights_f16mx), and the FORMAT of the planes the output stage emits into out_hi / out_lo:
   *   0: bf16 hi / lo (above);  1: f16mx — out_hi = f16 plane, out_lo = per 32-column block the 64 bytes
   *      [h8 c0-15 | l8 c0-15 | h8 c16-31 | l8 c16-31], h8 = e5m2(h), l8 = e5m2(l * 2^11) (needs the emitted column count % 32 == 0).  Same geometry and ld_planes convention as the bf16 planes. */
  const uint8_t* w_scale;
  int planes_fmt;
  /* weight gradients on the bf16x3 kernels (ABI v8; NULL elsewhere): when set and dY (`w`) is fp32, the kernel also accumulates the column sums of
   * dY — the BIAS gradient of the layer, sum_m dY[m][n] — into colsum[n] (fp32 atomic adds, like dW) from the registers that stage dY anyway,
   * instead of a separate ddpo_colsum_accum launch re-reading dY.  Ignored (returns DDPO_EINVAL) with a plane dY operand. */
  float* colsum;
  /* epilogue == 1 (GEGLU) only (ABI v8; NULL elsewhere): also store the PRE-activation x W + b, (M, N) fp32 with row stride N in the ORIGINAL
   * column order [a (N/2) | gate (N/2)] (the interleaving of the packed weights undone) — what the GEGLU backward needs, so the training forward
   * can use the fused launch too. */
  float* aux_out;
  /* residual row period.  A TRAILING FIELD ADDED UNDER ABI v14 (the number is unchanged): the struct grew by one int, and the library reads the
   * field on every forward call — a binding or C caller built against the shorter ABI-14 struct MUST be rebuilt against this header (zero the
   * descriptor before filling it: 0 = the earlier behaviour) and must compare its struct size with ddpo_sizeof_gemm_desc() at load, as the
   * ctypes mirror does; ddpo_abi_version() alone does not tell the two layouts apart.  res_rows > 0: `residual` holds res_rows rows and output row m adds residual row m % res_rows — the residual of a
   * batch whose halves share it (classifier-free guidance: [x; x]) is held once.  Forward entry points only (ddpo_gemm_conv_fwd, _fwd_bf16,
   * _fwd_bf16_planes, _fwd_f16mx_planes: every tile class, split-K reduce and plane-emitting output stage); needs `residual` and
   * M % res_rows == 0, DDPO_EINVAL otherwise and wherever else it is non-zero (weight gradients, folded up-sampler). */
  int res_rows;
} ddpo_gemm_desc;
int ddpo_gemm_conv_fwd(const ddpo_gemm_desc* d, void* stream);
/* Data gradients reuse ddpo_gemm_conv_fwd: src = dY, w = forward kernel with w_trans=1, w_dgrad=1, and for the
 * gradient of a stride-2 convolution upsample=2 ("zero-insert" source: only even virtual coordinates exist).
 * Weight gradient (jax.grad w.r.t. conv / dense kernels, ddpo/training/policy_gradient.py:138-139):
 *   out[k][n] (+)= alpha * sum_m A(m,k) * dY[m][n],  A as in the forward pass (src = forward input),
 *   w = dY (M,N) with row stride ld_w, out = dW (K,N) with row stride ld_out.  With splits != 1 the partial sums
 *   are combined with fp32 atomic adds (out must hold zeros or the running gradient accumulation). */
int ddpo_gemm_conv_wgrad(const ddpo_gemm_desc* d, void* stream);

/* Same contraction on the bf16 MFMA datapath (v_mfma_f32_32x32x16_bf16) with fp32 operands emulated by a bf16 split
 * (x = hi + lo): npass = 3 computes a_lo*b_hi + a_hi*b_lo + a_hi*b_hi (XLA "bf16_3x"/HIGH, ~1e-5 relative),
 * npass = 1 computes a_hi*b_hi (XLA's TPU DEFAULT precision — what the reference ran with); fp32 accumulation.
 * Activations (d->src) stay fp32 and are split on the fly; the weights are given as pre-split bf16 planes made by
 * ddpo_pack_weights_bf16: forward order (N, ldw=Kp) for the forward pass, the original (K, N) order with
 * d->w_dgrad = 1 for data gradients.  d->w / d->w_trans are ignored.  Requires Cin % 8 == 0 (K % 8 == 0 if dense). */
int ddpo_gemm_conv_fwd_bf16(const ddpo_gemm_desc* d, const uint16_t* w_hi, const uint16_t* w_lo, int ldw, int npass,
                            void* ws, size_t ws_bytes, void* stream);
/* Plane-fed variant: the activation operand is given ALREADY split into bf16 hi / lo planes a_hi / a_lo,
 * (rows, lda) bf16 with lda in elements (% 8 == 0), rows = B*H*W source pixels (conv) or M (dense), as written by
 * ddpo_split_planes_bf16 or by the plane-emitting output stage of a normalisation kernel.  d->src / d->ld_src / d->w are
 * ignored.  Both operands reach LDS by LDS-DMA (no register staging, no split in the loader).  Same tiles, k order and
 * MFMA passes as ddpo_gemm_conv_fwd_bf16 on the fp32 tensor the planes were split from: bit-identical results.
 * Requires Cin % 32 == 0 (K % 32 == 0 if dense), no w_dgrad; returns DDPO_EINVAL otherwise (use the fp32-fed entry).
 * ABI v14: a_lo == NULL AND w_lo == NULL selects SINGLE-PASS bf16 (a_hi * w_hi only, fp32 accumulation: npass = 1 of
 * ddpo_gemm_conv_fwd_bf16 — XLA's TPU default precision, BASELINE configs[4]'s dtype) on the same LDS-DMA loaders: one plane per operand,
 * 256 x 320 tiles on a four-stage LDS ring with a counted vmcnt where their grid fills the chip.  hi = bf16(x) is the operand the fp32-fed
 * single-pass kernel forms in its loader: bit-identical to it.  Exactly one of the two lo pointers NULL, or epilogue == 2, is DDPO_EINVAL. */
int ddpo_gemm_conv_fwd_bf16_planes(const ddpo_gemm_desc* d, const uint16_t* a_hi, const uint16_t* a_lo, int lda,
                                   const uint16_t* w_hi, const uint16_t* w_lo, int ldw, void* ws, size_t ws_bytes,
                                   void* stream);
/* f16mx forward datapath (plane-fed, ABI v7).  a*b ~= a_h*b_h + a_h8*b_l8 + a_l8*b_h8: per 32x32 accumulator block and 32-wide
 * k-tile two v_mfma_f32_32x32x16_f16 (the f16 x f16 term) and ONE v_mfma_scale_f32_32x32x64_f8f6f4 carrying both cross terms,
 * against six bf16 MFMAs of the bf16x3 datapath — 2/3 of its matrix-pipe time on the same LDS-DMA operand stream (the planes have
 * the geometry of the bf16 hi / lo planes; profiles/r03_ktime_mx_ablation.log).  The dropped term is a_l*b_l (~2^-22 relative) and
 * the 8-bit rounding of the factors of the cross terms (~2^-15): ~7e-5 relative on a whole SD-1.5 U-Net forward against
 * 2e-5 for bf16x3 and ~2e-3 for single-pass bf16.  Operands:
 *   a16 / a8  activation planes written by ddpo_split_planes_f16mx or a plane-emitting producer (planes_fmt = 1), (rows, lda) or
 *             k-blocked (lda == 0) like the bf16 planes;
 *   w16 / w8 / d->w_scale  weight planes of ddpo_pack_weights_f16mx (k-blocked only: d->w_layout must be 1).
 * Tiles, split-K, output stage (incl. epilogue = 1 / 2 and plane emission in either format) as ddpo_gemm_conv_fwd_bf16_planes;
 * every tile class accumulates in the same order (bit-identical results for one layer whatever the batch).  Forward only:
 * data / weight gradients stay on bf16x3. 
 * ABI v14: a8 == NULL AND w8 == NULL (d->w_scale unused) runs the operator WITHOUT its cross terms — a_h * w_h on the f16 MFMA only, on the
 * single-plane kernels (four-stage ring on the 256 x 320 tile): one f16 pass per product, 7e-4 instead of 4e-5 on a U-Net forward and outside the 1e-3 gradient contract at full size.  Opt-in
 * (DDPO_MX_CROSS=0); exactly one of the two NULL, or epilogue == 2 without the cross terms, is DDPO_EINVAL. */
int ddpo_gemm_conv_fwd_f16mx_planes(const ddpo_gemm_desc* d, const uint16_t* a16, const uint16_t* a8, int lda,
                                    const uint16_t* w16, const uint16_t* w8, void* ws, size_t ws_bytes, void* stream);
/* Folded nearest-2x up-sampler (additive to ABI v14): FlaxUpsample2D — jax.image.resize(nearest, 2x) followed by a 3x3 convolution, inside the
 * U-Net / VAE-decoder call sites of ddpo/diffusers_patch/pipeline_flax_stable_diffusion.py:219-224,251 and ddpo/training/policy_gradient.py:87-102
 * — computed as FOUR stride-1 2x2 convolutions on the source grid, one per output phase (py, px): output pixel (2y + py, 2x + px) reads source
 * offsets {-1, 0} (phase 0) / {0, +1} (phase 1) per axis with the 3x3 taps that land on the same source pixel summed beforehand
 * (ddpo_fold_up2x_weights).  Reduction length 4 Cin instead of 9 Cin; same function of the input, different rounding (weights are summed first).
 *   ddpo_fold_up2x_weights: w (3, 3, Cin, Cout) HWIO -> wf (4, 2, 2, Cin, Cout) fp32, phase index py * 2 + px; fp32 sums, ky then kx ascending.
 *     Each phase (4 Cin, Cout) is then packed like any forward weight (ddpo_pack_weights_bf16_kblocked / ddpo_pack_weights_f16mx).
 *   ddpo_conv_up2x_folded_fwd: plane-fed only.  d: B, H, W (SOURCE dims), Cin (% 32 == 0), N = Cout (% 4 == 0), bias (optional), out (B * 2H * 2W
 *     rows of ld_out floats, 16-byte aligned; ld_out may exceed N: the other columns are not touched); row bias / residual / epilogue / plane
 *     emission / w_dgrad / aux_out must be zero (DDPO_EINVAL otherwise), every other field — alpha included: the layer has no scale — is ignored.  a_hi / a_lo / lda: the source activation planes as in
 *     ddpo_gemm_conv_fwd_bf16_planes (f16mx != 0: as in ddpo_gemm_conv_fwd_f16mx_planes).  w_hi / w_lo: the four phases' k-blocked planes back to
 *     back, (4, 4 Cin / 32, N, 32) 16-bit elements each (f16mx: w16 and w8 — (4, 4 Cin / 32, N, 64) bytes — with d->w_scale = (4, N) E8M0 bytes).
 *     a_lo == NULL and w_lo == NULL: single-pass bf16.  All four phases run in one launch (plus one fixed-order reduce pass when the reduction
 *     is split: ws / ws_bytes as in ddpo_gemm_conv_fwd_bf16; bit-reproducible). */
int ddpo_fold_up2x_weights(const float* w, int Cin, int Cout, float* wf, void* stream);
int ddpo_conv_up2x_folded_fwd(const ddpo_gemm_desc* d, const uint16_t* a_hi, const uint16_t* a_lo, int lda, const uint16_t* w_hi,
                              const uint16_t* w_lo, int f16mx, void* ws, size_t ws_bytes, void* stream);
/* fp32 W (K, N) -> f16mx weight planes, k-blocked: w16 (ceil(K/32), N, 32) f16 = f16(w); w8 (ceil(K/32), N, 64) bytes =
 * [e4m3(l * 2^11 / s_n) x 32 | e4m3(h / s_n) x 32] with h = f16(w), l = w - h and s_n = 2^(scale[n] - 127) the power of two that
 * puts the column's largest |w| in [128, 256); scale (N) bytes.  Zero padded in k. */
int ddpo_pack_weights_f16mx(const float* w, int K, int N, uint16_t* w16, uint16_t* w8, uint8_t* scale, void* stream);
/* fp32 activations (rows, cols), row stride ldx -> f16mx activation planes (what the plane-emitting producers write); ld_out as
 * ddpo_split_planes_bf16 (0 = k-blocked); cols % 32 == 0. */
int ddpo_split_planes_f16mx(const float* x, int ldx, uint16_t* p16, uint16_t* p8, int ld_out, int64_t rows, int cols, void* stream);
/* fp32 W (K, N) -> bf16 hi / lo planes in the k-blocked forward layout (ceil(K / 32), N, 32), zero padded in k (w_layout = 1). */
int ddpo_pack_weights_bf16_kblocked(const float* w, int K, int N, uint16_t* fwd_hi, uint16_t* fwd_lo, void* stream);
/* ABI v13.  The DATA-GRADIENT operand of the layer with forward kernel w (taps, Cin, Cout) (HWIO flattened; dense layer: taps = 1), packed straight from
 * w into the same k-blocked layout: W'[tap' * Cout + co][ci] = w[taps - 1 - tap'][ci][co], i.e. (ceil(taps * Cout / 32), Cin, 32) planes — what
 * ddpo_gemm_conv_fwd_bf16[_planes] reads to compute dX as a forward contraction of dY (/root/reference/ddpo/training/policy_gradient.py:104-139,
 * the jax.grad of the U-Net call).  Same values as packing the flipped / transposed copy of w with ddpo_pack_weights_bf16_kblocked. */
int ddpo_pack_weights_bf16_kblocked_dgrad(const float* w, int taps, int Cin, int Cout, uint16_t* hi, uint16_t* lo, void* stream);
/* x:(rows, cols) fp32, row stride ldx -> hi / lo bf16 planes (rows, ld_out): hi = bf16(x), lo = bf16(x - hi). */
int ddpo_split_planes_bf16(const float* x, int ldx, uint16_t* hi, uint16_t* lo, int ld_out, int64_t rows, int cols,
                           void* stream);
/* ws (optional, 16-byte aligned): scratch for a deterministic split-K of launches whose tile grid under-fills the chip
 * (partials + fixed-order reduce with the fused epilogue); pass NULL/0 to disable. */
/* Weight gradient on the bf16x3 MFMA datapath (same arguments as ddpo_gemm_conv_wgrad; always accumulates with fp32
 * atomics).  Dense, or convolutions with pad = ksize/2, stride 1 or 2, optionally over a nearest-2x upsampled input
 * (returns DDPO_EINVAL otherwise - callers fall back to ddpo_gemm_conv_wgrad). */
int ddpo_gemm_conv_wgrad_bf16x3(const ddpo_gemm_desc* d, void* stream);
/* The same weight gradient with one or both operands given as bf16 hi / lo planes (the format of
 * ddpo_gemm_conv_fwd_bf16_planes): a_hi / a_lo replace d->src (the forward input; rows of d->ld_src ELEMENTS), dy_hi / dy_lo
 * replace d->w (dY; rows of d->ld_w elements).  A NULL pair means that operand is fp32 in the descriptor.  Same values reach
 * the MFMAs as in the fp32-fed form (the planes ARE its split), so the result differs only by the atomics' summation order. */
int ddpo_gemm_conv_wgrad_bf16x3_planes(const ddpo_gemm_desc* d, const uint16_t* a_hi, const uint16_t* a_lo,
                                       const uint16_t* dy_hi, const uint16_t* dy_lo, void* stream);
/* fp32 W (K,N) -> bf16 hi/lo planes: fwd_* (N, Kp) k-contiguous (Kp = K rounded up to 8, zero padded) and, if
 * bwd_hi != NULL, bwd_* (K, N).  Call after every optimizer update (weights only change there). */
int ddpo_pack_weights_bf16(const float* w, int K, int N, int Kp, uint16_t* fwd_hi, uint16_t* fwd_lo,
                           uint16_t* bwd_hi, uint16_t* bwd_lo, void* stream);

/* ---- Fused multi-head attention, softmax(q k^T * scale) v, flash-style (no N x N tensor is ever materialised).  Replaces
 * nn.dot_product_attention of diffusers' FlaxAttentionBlock inside the U-Net call sites of
 * ddpo/diffusers_patch/pipeline_flax_stable_diffusion.py:219-224 and ddpo/training/policy_gradient.py:87-102.
 * LAYOUTS, common to every function of this section: q:(q_batches,Nq,.) k,v:(B,Nk,.) o:(B,Nq,.): head h occupies columns [h*d,(h+1)*d) of each
 *   row; ld* = row strides in floats (multiples of 4), pointers 16-byte aligned.  lse (optional, (B,heads,Nq)): log2-domain logsumexp of the
 *   scaled scores, consumed by the backward pass.
 * QUERY PERIOD: q holds q_batches batches of Nq rows (1 <= q_batches <= B, B % q_batches == 0, DDPO_EINVAL otherwise) and the workgroups of
 *   batch b read their queries from batch b % q_batches; K / V (or their images), the output rows and lse stay per b.  q_batches == B: every
 *   batch has its own queries.  q_batches < B is for the cross-attention of a classifier-free-guidance batch [x; x], whose two halves share the
 *   queries and differ in the text context only (pipeline_flax_stable_diffusion.py:219-224): the query projection runs, and is stored, once.
 *   Same kernels and per-query arithmetic whatever the period. */

/* The exact-fp32 kernel (fp32 MFMA 16x16x4): d in {4, 8, 16, 40, 64, 80, 160}. */
int ddpo_attention_fwd(const float* q, int ldq, int q_batches, const float* k, int ldk, const float* v, int ldv, float* o, int ldo,
                       float* lse, int B, int heads, int Nq, int Nk, int d, float scale, void* stream);

/* The same contract on the 16-bit MFMA kernels, d in {8, 16, 40, 64, 80}, in two arithmetic variants:
 *   f16p == 0 (`bf16x3`): Q, K, V and the probabilities are split into bf16 hi + lo and every product takes three passes (fp32 accumulate,
 *     ~1e-5 relative).
 *   f16p != 0 (`f16p`, the attention of the f16mx datapath): the scores stay bf16 hi + lo on three MFMA passes; in the second product the
 *     probabilities are ONE f16 term p = exp2(s - m + 14) (round to nearest even) against V split into f16 hi + lo — two passes — and the softmax
 *     denominator is the sum of the same rounded probabilities (a row of ones in V^T where the head dim leaves a spare MFMA row), so O is an exact
 *     convex combination of the values with weights perturbed by <= 2^-12 (csrc/attention_bf16.hip; 1.42 -> 1.29 ms on 4096^2 keys, d = 40,
 *     batch 16).
 * OUTPUT FORM: exactly one of o and o_hi is given (DDPO_EINVAL otherwise).  o: fp32 rows (o, ldo), as above.  o_hi (o must be NULL; o_lo must be
 *   given too): the normalised output leaves as bf16 hi / lo PLANES (o_hi / o_lo: (B * Nq, heads * d) bf16 each, row stride ld_planes elements
 *   (a multiple of 4), 8-byte aligned; ld_planes == 0: k-blocked (heads * d / 32, B * Nq, 32), heads * d % 32 == 0) holding exactly the split
 *   hi = bf16(x), lo = bf16(x - hi) of the fp32 value the row form writes — the activation format of ddpo_gemm_conv_fwd_bf16_planes, so the
 *   to_out projection behind the attention (diffusers FlaxAttentionBlock: proj_attn / to_out_0) reads planes by LDS-DMA and no fp32 tensor is
 *   written or re-split: in the sampling forward at the 64x64 level that projection drops from 103 to 62 us per launch
 *   (profiles/r04_timeline_sampling_step.txt).  Sampling path only (the training forward keeps the fp32 output its backward reads).
 * WORKSPACE (ddpo_attention_fwd_x16): ws (optional, 16-byte aligned, >= ddpo_attention_fwd_x16_ws_bytes, which serves both variants): when
 *   given and Nk >= 256, K and V are split / transposed once per (batch, head) into per-tile LDS images that the attention kernel streams;
 *   without it (or for short key sequences, where the size query returns 0) every query tile stages K / V itself.  Results are identical.
 * IMAGES (ddpo_attention_pack_kv + ddpo_attention_fwd_images), for keys / values that stay constant over many attention calls (the text context
 *   of the cross-attention layers over the DDIM steps of a sampling call, pipeline_flax_stable_diffusion.py:219-224 re-projects and re-reads it
 *   every step): pack K / V ONCE into the per-tile images (any Nk, `images` 16-byte aligned, >= ddpo_attention_kv_images_bytes — the same byte
 *   size for both variants) and run every attention from them.  Images are only valid for a forward with the f16p they were packed with.  Same
 *   kernels as the workspace form: identical results. */
size_t ddpo_attention_fwd_x16_ws_bytes(int B, int heads, int Nk, int d);
int ddpo_attention_fwd_x16(int f16p, const float* q, int ldq, int q_batches, const float* k, int ldk, const float* v, int ldv, float* o,
                           int ldo, uint16_t* o_hi, uint16_t* o_lo, int ld_planes, float* lse, int B, int heads, int Nq, int Nk, int d,
                           float scale, void* ws, size_t ws_bytes, void* stream);
size_t ddpo_attention_kv_images_bytes(int B, int heads, int Nk, int d);
int ddpo_attention_pack_kv(int f16p, const float* k, int ldk, const float* v, int ldv, void* images, size_t images_bytes, int B, int heads,
                           int Nk, int d, void* stream);
int ddpo_attention_fwd_images(int f16p, const float* q, int ldq, int q_batches, const void* images, size_t images_bytes, float* o,
                              int ldo, uint16_t* o_hi, uint16_t* o_lo, int ld_planes, float* lse, int B, int heads, int Nq, int Nk,
                              int d, float scale, void* stream);

/* Attention backward with probability recomputation: dvec (B,heads,Nq) scratch = rowsum(dO * O); dq/dk/dv have the layout of q/k/v with
 * contiguous rows of heads*d (one query batch per batch: no query period).  Exact fp32. */
int ddpo_attention_bwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* o,
                       const float* d_o, const float* lse, float* dvec, float* dq, float* dk, float* dv,
                       int B, int heads, int Nq, int Nk, int d, float scale, void* stream);
/* The same on the 16-bit MFMA kernels (same arguments behind f16p; d in {8, 16, 40, 64, 80}; csrc/attention_bwd_bf16.hip):
 *   f16p == 0: every product on three bf16 passes.
 *   f16p != 0: the backward of the f16p forward.  `dvec` is then a scratch of B * heads * (Nq + 1) floats: rowsum(dO * O) followed by one word
 *     per (batch, head) slab — the float bits of max |dO| over the slab, from which the kernels take the power of two that brings dO into the
 *     f16 range whatever the loss scale.  Scores: bf16 hi + lo, three passes; dP = dO V^T, dV = P^T dO, dK = dS^T Q, dQ = dS K: a single f16
 *     term (dO, P, dS) against an f16 hi + lo split, two passes. */
int ddpo_attention_bwd_x16(int f16p, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* o,
                           const float* d_o, const float* lse, float* dvec, float* dq, float* dk, float* dv,
                           int B, int heads, int Nq, int Nk, int d, float scale, void* stream);

/* Small element-wise pieces. */
int ddpo_geglu_fwd(const float* x, float* y, int64_t rows, int F, void* stream);      /* y = x[:, :F] * gelu_tanh(x[:, F:]) */
int ddpo_silu_fwd(const float* x, float* y, int64_t n, void* stream);
/* Reward-model pieces (aesthetic_fn, /root/reference/ddpo/training/callbacks.py:60-95: CLIP ViT-L/14 image tower + LAION MLP run on
 * this library's GEMM / LayerNorm / attention kernels): quick-GELU y = x * sigmoid(1.702 x) (x, y 16-byte aligned), and the row-wise
 * L2 normalisation of the image features (:80-82). */
int ddpo_quick_gelu_fwd(const float* x, float* y, int64_t n, void* stream);
int ddpo_l2_normalize_rows(const float* x, float* y, int rows, int cols, void* stream);
/* CLIP text tower + CLIPScore reward (clip_score_fn; csrc/clip_text.hip; additive to ABI v14).
 * ddpo_attention_causal_fwd: self-attention softmax(mask(q k^T * scale)) v with the mask key <= query, on fp32 MFMA (16x16x4).  Row layouts
 *   and alignment rules of ddpo_attention_fwd: q, k, v, o are (B, N, .) with head h in columns [h*d, (h+1)*d), ld* = row strides (multiples of
 *   4, >= heads*d), pointers 16-byte aligned.  One workgroup per (batch, head) holds all of K and V in LDS, so 1 <= N <= 80 (every CLIP text
 *   tower has 77 positions) and d is 16 or 64; anything else returns DDPO_EINVAL and launches nothing.  Forward only: no lse output.
 * ddpo_gather_rows: out[r, :] = table[idx[r], :] (+ add[r % add_period, :] when add != NULL), r < rows.  table has table_rows rows of row
 *   stride ld; out (rows, cols) and add (add_period, cols) are contiguous; cols and ld are multiples of 4, pointers 16-byte aligned, idx int32.
 *   An index outside [0, table_rows) is CLAMPED into the table: nothing outside it is ever read (callers validate indices on the host).
 * ddpo_cosine_rows: out[r] = scale * <a_r, b_r> / (|a_r| |b_r|) for contiguous (rows, cols) a, b (cols a multiple of 4, 16-byte aligned):
 *   one wave per row, fp32 accumulation in a fixed order (bit-reproducible, no atomics).  A zero row gives NaN. */
int ddpo_attention_causal_fwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* o, int ldo,
                              int B, int heads, int N, int d, float scale, void* stream);
int ddpo_gather_rows(const float* table, int ld, int table_rows, const int32_t* idx, int rows, int cols, const float* add, int add_period,
                     float* out, void* stream);
int ddpo_cosine_rows(const float* a, const float* b, int rows, int cols, float scale, float* out, void* stream);
/* JPEG file size without the file (csrc/jpeg_size.hip; additive to ABI v14): bytes_out[n] = len of the baseline JPEG a libjpeg encoder writes for
 *   image n at `quality` (1..100) with its defaults — 4:2:0, standard Huffman tables, one scan, JFIF header — i.e. what PIL's
 *   Image.save(buf, "JPEG", quality=q) returns.  images: N x H x W x 3 (NHWC, contiguous), uint8 or (is_float32) float32 in [0, 1], which is
 *   truncated as (uint8)(x * 255.0f) (clamped; NaN -> 0).  H and W must be multiples of 16 (no edge replication / dummy blocks): anything else is DDPO_EINVAL.
 *   All scratch is the caller's `workspace` (device, >= ddpo_jpeg_size_workspace_bytes, 16-byte aligned); the launch sequence zeroes what it needs
 *   on `stream`, so calls on different streams with different workspaces may overlap.  ddpo_jpeg_size_host: the same arithmetic, serially, on
 *   host memory (no GPU).  DDPO_JPEG_FIXED_BYTES: the bytes of such a file that are not entropy-coded data (623 before the scan data + EOI). */
#define DDPO_JPEG_FIXED_BYTES 625
int ddpo_jpeg_size_workspace_bytes(int N, int H, int W, size_t* out_host);
int ddpo_jpeg_size(const void* images, int is_float32, int N, int H, int W, int quality, void* workspace, size_t workspace_bytes,
                   int64_t* bytes_out, void* stream);
int ddpo_jpeg_size_host(const uint8_t* rgb, int N, int H, int W, int quality, int64_t* bytes_out_host);
/* The file itself (csrc/jpeg_size.hip; additive to ABI v14): files[n * file_stride ..] = the bytes of that same baseline JPEG — byte for byte
 *   what PIL's Image.save(buf, "JPEG", quality=q) writes — and lengths[n] = its length, the value ddpo_jpeg_size returns.  Inputs, rules and
 *   workspace (ddpo_jpeg_size_workspace_bytes) are ddpo_jpeg_size's; in addition H, W <= 65500 (the format's limit as libjpeg applies it) and
 *   file_stride >= DDPO_JPEG_FIXED_BYTES, else DDPO_EINVAL.  files: device, N rows of file_stride bytes, no alignment required.
 *   Prefix rule: a file longer than file_stride leaves its first file_stride bytes in the row, and lengths[n] still reports the full length
 *   (compare it with file_stride, then repeat with ddpo_jpeg_encode_max_bytes, which no file of that size exceeds:
 *   625 + 2 * ceil(blocks * 1664 / 8)).  Nothing is written past a row, and bytes of a row beyond min(lengths[n], file_stride) are not written at
 *   all.  The first DDPO_JPEG_HEADER_BYTES of every file of one (H, W, quality) are the same: everything before the scan data.
 *   ddpo_jpeg_encode_host: the same arithmetic, serially, on host memory (no GPU). */
#define DDPO_JPEG_HEADER_BYTES 623
int ddpo_jpeg_encode_max_bytes(int H, int W, size_t* out_host);
int ddpo_jpeg_encode(const void* images, int is_float32, int N, int H, int W, int quality, void* workspace, size_t workspace_bytes,
                     uint8_t* files, size_t file_stride, int64_t* lengths, void* stream);
int ddpo_jpeg_encode_host(const uint8_t* rgb, int N, int H, int W, int quality, uint8_t* files_host, size_t file_stride, int64_t* lengths_host);
/* CLIP image preprocessing into the patch matrix (csrc/clip_preprocess.hip; additive to ABI v14): out[(n, gy, gx)][(c, ky, kx)] =
 *   norm[byte][c], byte = pixel (gy p + ky, gx p + kx), channel c, of the size x size centre crop of image n after an 8-bit two-pass bicubic resize
 *   to rh x rw (what Pillow's Image.resize(BICUBIC) returns for an RGB image); columns 3 p p .. ld - 1 are written as zeros.  One launch.
 *   images: N x H x W x 3 (NHWC, contiguous), uint8 or (is_float32) float32 in [0, 1], truncated as (uint8)(x * 255.0f) (clamped; NaN -> 0).
 *   Tables (int32; the caller builds them, lib.clip_preprocess_tables; nothing here is computed in double precision): hcoef rw x hksize 22-bit
 *   fixed-point weights and hbounds rw x 2 {first input column, tap count} for the horizontal pass, vcoef rh x vksize / vbounds rh x 2 for the
 *   vertical pass.  The horizontal pass is rounded to a byte before the vertical pass; an axis that keeps its size gets the identity table
 *   (one tap of 2^22).  norm: 256 x 3 float32.  rows: the most input rows one patch row's p output rows span (from the caller's copy of vbounds).
 *   DDPO_EINVAL: a null pointer, size not a multiple of patch, ld < 3 p p or ld not a multiple of 4, out not 16-byte aligned, a crop window
 *   (top, left, size) outside rh x rw, and the LDS rule: rows x size x 3 bytes + 8 staged input rows of W x 3 bytes (each rounded up to 16)
 *   + 3 KB must fit 160 KB.  No workspace and no state: calls on different streams may overlap.  The _host entry is the same arithmetic,
 *   serially, on host memory (no GPU; it works `rows` out itself and checks the tables); resized_out_host (may be null) receives the
 *   N x size x size x 3 bytes before normalisation. */
int ddpo_clip_preprocess(const void* images, int is_float32, int N, int H, int W, int rh, int rw, int top, int left, int size, int patch,
                         const int32_t* hcoef, const int32_t* hbounds, int hksize, const int32_t* vcoef, const int32_t* vbounds, int vksize,
                         int rows, const float* norm, float* out, int ld, void* stream);
int ddpo_clip_preprocess_host(const void* images, int is_float32, int N, int H, int W, int rh, int rw, int top, int left, int size, int patch,
                              const int32_t* hcoef, const int32_t* hbounds, int hksize, const int32_t* vcoef, const int32_t* vbounds,
                              int vksize, const float* norm, float* out_host, int ld, uint8_t* resized_out_host);
/* Symmetry rewards (csrc/symmetry.hip; additive to ABI v14).  images: N x H x W x 3 (NHWC, contiguous), uint8 or (is_float32) float32 in [0, 1],
 *   truncated as (uint8)(x * 255.0f) (clamped; NaN -> 0), as for ddpo_clip_preprocess.
 * ddpo_symmetry_stats: stats_out[n][0..3] (int64, device, 8-byte aligned) = four sums over all H W 3 bytes a of image n, b being the partner of a —
 *   mode 0 (mirror): byte (y, W-1-x, c); mode 1 (rotate 180): byte (H-1-y, W-1-x, c):
 *     [0] sum of (((a - b) mod 256)^2 mod 256)   what uint8 arithmetic makes of (a - b) ** 2
 *     [1] sum of a      [2] sum of a^2      [3] sum of a b
 *   All integer, so exact and independent of the order of summation; the unwrapped sum of (a - b)^2 is 2 [2] - 2 [3].  Two launches on `stream`:
 *   per-workgroup sums into `workspace` (device, >= ddpo_symmetry_stats_workspace_bytes, 8-byte aligned), then one wave per image adds them.  No
 *   atomics, nothing to zero, no state outside the arguments: calls on different streams with different workspaces may overlap.
 *   DDPO_EINVAL: a null pointer, a mode other than 0 / 1, N, H or W < 1, W > 10880 (a row pair is staged in 64 KB of LDS), a small workspace,
 *   misaligned pointers.
 * ddpo_rotate4_u8: out (uint8, device, 4N x S x S x 3): block k N + n is image n turned by 90 k degrees counter-clockwise, k = 0..3 — what
 *   PIL.Image.rotate(90 k) returns for a square image (np.rot90(a, k)).  One launch; every input pixel is read once.  H != W is DDPO_EINVAL.
 * The _host entries are the same arithmetic, serially, on host memory (no GPU). */
int ddpo_symmetry_stats_workspace_bytes(int N, int H, int W, int mode, size_t* out_host);
int ddpo_symmetry_stats(const void* images, int is_float32, int N, int H, int W, int mode, int64_t* stats_out, void* workspace,
                        size_t workspace_bytes, void* stream);
int ddpo_symmetry_stats_host(const void* images, int is_float32, int N, int H, int W, int mode, int64_t* stats_out_host);
int ddpo_rotate4_u8(const void* images, int is_float32, int N, int H, int W, uint8_t* out, void* stream);
int ddpo_rotate4_u8_host(const void* images, int is_float32, int N, int H, int W, uint8_t* out_host);
/* 8-bit bicubic resize to bytes (csrc/resize_u8.hip; additive to ABI v14): out (uint8, N x oh x ow x 3) = what Pillow's Image.resize((ow, oh),
 *   BICUBIC) returns for each RGB image of the batch — horizontal pass rounded to a byte, then the vertical pass.  One launch, one workgroup per
 *   (image, band of `band` output rows).  images and tables as for ddpo_clip_preprocess: hcoef ow x hksize / hbounds ow x 2 for the horizontal
 *   pass, vcoef oh x vksize / vbounds oh x 2 for the vertical pass; an axis that keeps its size gets the identity table; up-scales are in the
 *   domain.  rows: the most input rows one band spans (from the caller's copy of vbounds).  out needs no alignment.
 *   DDPO_EINVAL: a null pointer, a size < 1, oh or ow > 32768, band < 1, rows outside 1..H, and the LDS rule: rows x ow x 3 bytes + 8 staged
 *   input rows of W x 3 bytes (each rounded up to 16) must fit 160 KB.  No workspace and no state: calls on different streams may overlap.
 *   The _host entry is the same arithmetic, serially, on host memory (no GPU; it works `rows` out itself from `band` and checks the tables). */
int ddpo_resize_u8(const void* images, int is_float32, int N, int H, int W, int oh, int ow, const int32_t* hcoef, const int32_t* hbounds, int hksize,
                   const int32_t* vcoef, const int32_t* vbounds, int vksize, int band, int rows, uint8_t* out, void* stream);
int ddpo_resize_u8_host(const void* images, int is_float32, int N, int H, int W, int oh, int ow, const int32_t* hcoef, const int32_t* hbounds,
                        int hksize, const int32_t* vcoef, const int32_t* vbounds, int vksize, int band, uint8_t* out_host);
int ddpo_timestep_embedding(const int32_t* ts, float* out, int B, int dim, void* stream); /* concat([cos, sin]) */
int ddpo_nchw_to_nhwc(const float* x, float* y, int B, int C, int HW, void* stream);
int ddpo_nhwc_to_nchw(const float* x, float* y, int B, int C, int HW, void* stream);
int ddpo_copy_cols(const float* src, int ld_src, float* dst, int ld_dst, int64_t rows, int cols, void* stream);
/* ABI v14.  The inputs of one classifier-free-guidance sampling step, staged in ONE launch into the static input buffers of a captured U-Net
 * graph: s_in[0:n] = s_in[n:2n] = x[0:n] (the reference's jnp.concatenate([latents] * 2), pipeline_flax_stable_diffusion.py:219), and — each
 * optional, both pointers NULL to skip — row_dst[0:row_n] = row_src[0:row_n] (this step's row of the precomputed time-projection table) and
 * ts_dst[0:ts_n] = ts_src[0:ts_n].  n % 4 == 0, row_n % 4 == 0, float pointers 16-byte aligned. */
int ddpo_stage_cfg_inputs(const float* x, float* s_in, int64_t n, const float* row_src, float* row_dst, int row_n,
                          const int32_t* ts_src, int32_t* ts_dst, int ts_n, void* stream);
int ddpo_softmax_rows(float* x, int64_t rows, int cols, float scale, void* stream);    /* in place */
/* backward element-wise pieces */
int ddpo_geglu_bwd(const float* x, const float* dy, float* dx, int64_t rows, int F, void* stream);
int ddpo_silu_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream);
/* out[seg][n] += sum over the rows of segment seg (rows_per_seg consecutive rows; 0 = one segment) of x[m][n] */
int ddpo_colsum_accum(const float* x, int ldx, int64_t rows, int cols, int rows_per_seg, float* out, void* stream);
/* nearest-2x upsampling backward: y[b,h,w,:] = sum of the 2x2 block of x:(B,2H,2W,C) */
int ddpo_sumpool2x2(const float* x, float* y, int B, int H, int W, int C, void* stream);
int ddpo_add(const float* a, const float* b, float* out, int64_t n, void* stream);
int ddpo_scale_shift_clip(const float* x, float* y, int64_t n, float scale, float shift, float lo, float hi, void* stream);

/* ---- LoRA adapters on the attention projections (additive to ABI v14; csrc/lora.hip).
 * One adapted dense layer with Flax kernel W (K = in, N = out): W' = W0 + s * A B, A (K, r), B (r, N), all fp32 row-major. */
typedef struct ddpo_lora_layer {
  const float* w0;   /* frozen base weight (K, N), 16-byte aligned */
  float* w;          /* merged weight W' (K, N), 16-byte aligned (may not alias w0) */
  const float* a;    /* (K, r) */
  const float* b;    /* (r, N), 16-byte aligned */
  int K, N, r;       /* N % 4 == 0, 1 <= r <= 64 */
  float s;           /* alpha / r */
} ddpo_lora_layer;
/* W' = W0 + s * A B for n_layers layers in ONE launch; `table_dev` is a DEVICE array of n_layers descriptors, max_kn >= every K * N (< 2^33).
 * Per element: acc = sum_{j = 0..r-1} A[k, j] B[j, n] (fp32 fma, j ascending); W' = W0 bit for bit where s * acc == 0 (B == 0), else W0 + s * acc. */
int ddpo_lora_merge(const ddpo_lora_layer* table_dev, int n_layers, int64_t max_kn, void* stream);
/* Adapter gradients of one layer y = x W': dA (K, r) += s * x^T (dY B^T), dB (r, N) += s * (x A)^T dY, fp32, bitwise reproducible (fixed-order
 * partial slabs in ws, no atomics; two launches on `stream`).  x is EITHER fp32 rows (x, row stride ldx; x_hi = x_lo = NULL) OR, x == NULL, the
 * bf16 hi / lo activation planes (x = hi + lo) with the plane convention of the norms: ld_planes > 0 row-major, 0 k-blocked (K / 32, M, 32).
 * dY (M, N) fp32 with row stride lddy.  K % 4 == N % 4 == 0, K, N <= 2048, K + N <= 4064, 1 <= r <= 64; fp32 pointers 16-byte aligned.
 * ws: 16-byte aligned scratch of ddpo_lora_wgrad_ws_bytes(M, K, N, r) bytes. */
size_t ddpo_lora_wgrad_ws_bytes(int M, int K, int N, int r);
int ddpo_lora_wgrad(const float* x, int ldx, const uint16_t* x_hi, const uint16_t* x_lo, int ld_planes, const float* dy, int lddy,
                    const float* A, const float* B, float* dA, float* dB, int M, int K, int N, int r, float s, void* ws, size_t ws_bytes,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif
