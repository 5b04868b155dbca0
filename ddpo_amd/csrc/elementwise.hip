// HBM-bound kernels of the DDPO hot path: JAX-compatible Threefry normal generator, fused CFG + DDIM step +
// log-prob, fused scoring-mode log-prob + PPO-clip forward/backward, fused AdamW(bf16 mu) with global-norm
// clip and accumulation scaling, plus the small layout / activation kernels of the U-Net.
// Built with -ffp-contract=off so the fp32 operation order matches the CPU oracle.
#include "common.h"
#include "../../include/ddpo_cfg_rescale.h"
#include <math.h>

extern "C" int ddpo_abi_version(void) { return 15; }
extern "C" size_t ddpo_sizeof_gemm_desc(void) { return sizeof(ddpo_gemm_desc); }
extern "C" size_t ddpo_sizeof_ddim_consts(void) { return sizeof(ddpo_ddim_consts); }

// ------------------------------------------------------------------------------------------------
// Threefry-2x32 (20 rounds) — jax/_src/prng.py semantics (reference call sites in ddpo_hip.h)
// ------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

__host__ __device__ __forceinline__ void threefry2x32(uint32_t k0, uint32_t k1, uint32_t& x0, uint32_t& x1) {
  const uint32_t ks[3] = {k0, k1, k0 ^ k1 ^ 0x1BD11BDAu};
  const int R[2][4] = {{13, 15, 26, 6}, {17, 29, 16, 24}};
  x0 += ks[0];
  x1 += ks[1];
#pragma unroll
  for (int g = 0; g < 5; ++g) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      x0 += x1;
      x1 = rotl32(x1, R[g & 1][i]);
      x1 ^= x0;
    }
    x0 += ks[(g + 1) % 3];
    x1 += ks[(g + 2) % 3] + (uint32_t)(g + 1);
  }
}

extern "C" int ddpo_threefry_bits_host(uint32_t k0, uint32_t k1, int64_t n, uint32_t* out) {
  if (n < 0 || (!out && n)) return DDPO_EINVAL;
  const int64_t half = (n + 1) / 2;
  for (int64_t j = 0; j < half; ++j) {
    uint32_t x0 = (uint32_t)j, x1 = (j + half < n) ? (uint32_t)(j + half) : 0u;
    threefry2x32(k0, k1, x0, x1);
    out[j] = x0;
    if (j + half < n) out[j + half] = x1;
  }
  return DDPO_OK;
}

// XLA ErfInv32 (Giles' single-precision polynomial), operation order as xla/client/lib/math.cc.
__device__ __forceinline__ float erfinv_xla(float x) {
  float w = -log1pf(-(x * x));
  const bool lt = w < 5.0f;
  float p;
  if (lt) {
    w = w - 2.5f;
    p = 2.81022636e-08f;
    p = 3.43273939e-07f + p * w;
    p = -3.5233877e-06f + p * w;
    p = -4.39150654e-06f + p * w;
    p = 0.00021858087f + p * w;
    p = -0.00125372503f + p * w;
    p = -0.00417768164f + p * w;
    p = 0.246640727f + p * w;
    p = 1.50140941f + p * w;
  } else {
    w = sqrtf(w) - 3.0f;
    p = -0.000200214257f;
    p = 0.000100950558f + p * w;
    p = 0.00134934322f + p * w;
    p = -0.00367342844f + p * w;
    p = 0.00573950773f + p * w;
    p = -0.0076224613f + p * w;
    p = 0.00943887047f + p * w;
    p = 1.00167406f + p * w;
    p = 2.83297682f + p * w;
  }
  float r = p * x;
  if (fabsf(x) == 1.0f) r = x * INFINITY;
  return r;
}

__device__ __forceinline__ float bits_to_normal(uint32_t bits) {
  const float lo = -0.99999994f;   // nextafter(-1, 0)
  float f = __uint_as_float((bits >> 9) | 0x3F800000u) - 1.0f;
  float u = f * 2.0f + lo;         // (maxval - minval) rounds to 2.0f in f32
  u = fmaxf(lo, u);
  return 1.41421354f * erfinv_xla(u);   // float32(sqrt(2))
}

__global__ void __launch_bounds__(256) threefry_normal_kernel(uint32_t k0, uint32_t k1, float* __restrict__ out,
                                                              uint32_t* __restrict__ bits_out, int64_t n, int64_t half) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < half; j += (int64_t)gridDim.x * blockDim.x) {
    const bool has1 = (j + half) < n;
    uint32_t x0 = (uint32_t)j, x1 = has1 ? (uint32_t)(j + half) : 0u;
    threefry2x32(k0, k1, x0, x1);
    out[j] = bits_to_normal(x0);
    if (has1) out[j + half] = bits_to_normal(x1);
    if (bits_out) {
      bits_out[j] = x0;
      if (has1) bits_out[j + half] = x1;
    }
  }
}

extern "C" int ddpo_threefry_normal(uint32_t k0, uint32_t k1, float* out, uint32_t* bits_out, int64_t n, void* stream) {
  if (!out || n <= 0 || n > 0xFFFFFFFFll) return DDPO_EINVAL;
  const int64_t half = (n + 1) / 2;
  int grid = (int)((half + 255) / 256);
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(threefry_normal_kernel, dim3(grid), dim3(256), 0, as_stream(stream), k0, k1, out, bits_out, n, half);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

// ------------------------------------------------------------------------------------------------
// DDIM step (scheduling_ddim_flax.py:279-359)
// ------------------------------------------------------------------------------------------------
#include "ddim_coef.h"      // DdimCoef, ddim_coef(): shared with ppo_kl.hip

// mean of the DDIM posterior given the (guided) model output e and the current sample x
__device__ __forceinline__ float ddim_mean(const DdimCoef& k, int pred_type, float e, float x) {
  float x0;
  if (pred_type == DDPO_PRED_EPSILON) {
    x0 = (x - k.sqrt_bt * e) / k.sqrt_at;
  } else if (pred_type == DDPO_PRED_V) {
    x0 = k.sqrt_at * x - k.sqrt_bt * e;
    e = k.sqrt_at * e + k.sqrt_bt * x;
  } else {
    x0 = e;
  }
  return k.sqrt_ap * x0 + k.dirc * e;
}

#define LOG_SQRT_2PI 0.9189385332046727f

__global__ void __launch_bounds__(1024) ddim_step_kernel(const float* __restrict__ eps_u, const float* __restrict__ eps_c,
                                                        const float* __restrict__ x, const float* __restrict__ z,
                                                        const int32_t* __restrict__ ts, float g, ddpo_ddim_consts c,
                                                        float* __restrict__ x_next, float* __restrict__ logp, int chw) {
  __shared__ float red[16];
  const int b = blockIdx.x;
  const DdimCoef k = ddim_coef(c, ts[b]);
  const int64_t base = (int64_t)b * chw;
  const float inv2v = 1.0f / (2.0f * (k.std_c * k.std_c));
  const float cst = -logf(k.std_c) - LOG_SQRT_2PI;
  float acc = 0.f;
  for (int i = threadIdx.x * 4; i < chw; i += blockDim.x * 4) {
    const float4 eu = *reinterpret_cast<const float4*>(eps_u + base + i);
    const float4 ec = *reinterpret_cast<const float4*>(eps_c + base + i);
    const float4 xv = *reinterpret_cast<const float4*>(x + base + i);
    const float4 zv = *reinterpret_cast<const float4*>(z + base + i);
    float4 o;
    const float* peu = &eu.x; const float* pec = &ec.x; const float* px = &xv.x; const float* pz = &zv.x;
    float* po = &o.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float e = peu[j] + g * (pec[j] - peu[j]);
      const float mu = ddim_mean(k, c.pred_type, e, px[j]);
      const float xn = mu + k.std * pz[j];
      const float d = xn - mu;
      acc += -(d * d) * inv2v + cst;
      po[j] = xn;
    }
    *reinterpret_cast<float4*>(x_next + base + i) = o;
  }
  const float tot = block_sum(acc, red);
  if (threadIdx.x == 0) logp[b] = tot / (float)chw;
}

extern "C" int ddpo_ddim_step_fwd(const float* eps_u, const float* eps_c, const float* x, const float* z,
                                  const int32_t* ts, float guidance_scale, const ddpo_ddim_consts* c,
                                  float* x_next, float* logp, int B, int chw, void* stream) {
  if (!eps_u || !eps_c || !x || !z || !ts || !c || !x_next || !logp || B <= 0 || chw <= 0 || (chw & 3)) return DDPO_EINVAL;
  hipLaunchKernelGGL(ddim_step_kernel, dim3(B), dim3(1024), 0, as_stream(stream), eps_u, eps_c, x, z, ts,
                     guidance_scale, *c, x_next, logp, chw);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

// ------------------------------------------------------------------------------------------------
// scoring-mode log-prob + PPO-clip forward/backward (ddpo/training/policy_gradient.py:95-139)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) ppo_fwd_bwd_kernel(const float* __restrict__ eps_c, const float* __restrict__ eps_u,
                                                          const float* __restrict__ x, const float* __restrict__ x_next,
                                                          const int32_t* __restrict__ ts, const float* __restrict__ old_logp,
                                                          const float* __restrict__ adv_in, float g, float clip, int train_cfg,
                                                          ddpo_ddim_consts c, float* __restrict__ d_eps_c,
                                                          float* __restrict__ d_eps_u, float* __restrict__ per_sample,
                                                          int group, int chw) {
  __shared__ float red[16];
  __shared__ float s_dl;
  const int b = blockIdx.x;
  const DdimCoef k = ddim_coef(c, ts[b]);
  const int64_t base = (int64_t)b * chw;
  const float inv2v = 1.0f / (2.0f * (k.std_c * k.std_c));
  const float cst = -logf(k.std_c) - LOG_SQRT_2PI;
  float acc = 0.f;
  for (int i = threadIdx.x * 4; i < chw; i += blockDim.x * 4) {
    const float4 ec = *reinterpret_cast<const float4*>(eps_c + base + i);
    float4 eu = ec;
    if (train_cfg) eu = *reinterpret_cast<const float4*>(eps_u + base + i);
    const float4 xv = *reinterpret_cast<const float4*>(x + base + i);
    const float4 xn = *reinterpret_cast<const float4*>(x_next + base + i);
    const float* pec = &ec.x; const float* peu = &eu.x; const float* px = &xv.x; const float* pn = &xn.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float e = train_cfg ? (peu[j] + g * (pec[j] - peu[j])) : pec[j];
      const float d = pn[j] - ddim_mean(k, c.pred_type, e, px[j]);
      acc += -(d * d) * inv2v + cst;
    }
  }
  const float tot = block_sum(acc, red);
  if (threadIdx.x == 0) {
    const float lp = tot / (float)chw;
    const float A = fminf(fmaxf(adv_in[b], -10.0f), 10.0f);        // ADV_CLIP_MAX
    const float ratio = expf(lp - old_logp[b]);
    const float unclipped = -A * ratio;
    const float clipped = -A * fminf(fmaxf(ratio, 1.0f - clip), 1.0f + clip);
    const bool use_unclipped = unclipped >= clipped;
    s_dl = use_unclipped ? (-A * ratio / (float)group) : 0.0f;      // loss = mean over the micro-batch of `group` rows
    per_sample[b * 4 + 0] = lp;
    per_sample[b * 4 + 1] = ratio;
    per_sample[b * 4 + 2] = fmaxf(unclipped, clipped);
    per_sample[b * 4 + 3] = (fabsf(ratio - 1.0f) > clip) ? 1.0f : 0.0f;
  }
  __syncthreads();
  // d logp / d mu = (x' - mu) / (sigma_c^2 * CHW);  d mu / d e per prediction type
  float dmu_de;
  if (c.pred_type == DDPO_PRED_EPSILON) dmu_de = k.dirc - k.sqrt_ap * k.sqrt_bt / k.sqrt_at;
  else if (c.pred_type == DDPO_PRED_V) dmu_de = k.dirc * k.sqrt_at - k.sqrt_ap * k.sqrt_bt;
  else dmu_de = k.sqrt_ap;
  const float coef = s_dl * dmu_de / ((k.std_c * k.std_c) * (float)chw);
  for (int i = threadIdx.x * 4; i < chw; i += blockDim.x * 4) {
    const float4 ec = *reinterpret_cast<const float4*>(eps_c + base + i);
    float4 eu = ec;
    if (train_cfg) eu = *reinterpret_cast<const float4*>(eps_u + base + i);
    const float4 xv = *reinterpret_cast<const float4*>(x + base + i);
    const float4 xn = *reinterpret_cast<const float4*>(x_next + base + i);
    const float* pec = &ec.x; const float* peu = &eu.x; const float* px = &xv.x; const float* pn = &xn.x;
    float4 dc, du;
    float* pdc = &dc.x; float* pdu = &du.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float e = train_cfg ? (peu[j] + g * (pec[j] - peu[j])) : pec[j];
      const float d = pn[j] - ddim_mean(k, c.pred_type, e, px[j]);
      const float de = coef * d;
      pdc[j] = train_cfg ? g * de : de;
      pdu[j] = (1.0f - g) * de;
    }
    *reinterpret_cast<float4*>(d_eps_c + base + i) = dc;
    if (train_cfg) *reinterpret_cast<float4*>(d_eps_u + base + i) = du;
  }
}

// Round 6 (13.5 us for 21 MB, one workgroup per sample-timestep = 32 of the 256 CUs): the SAME arithmetic IN THE SAME ORDER on a
// CLUSTER of four workgroups of 256 threads per sample (4 B <= 256: every workgroup resident).  Thread t of workgroup s is thread 256 s + t of the
// 1024-thread form: it accumulates the same elements (float4 number T + 1024 k) in the same order, its wave is wave 4 s + (t >> 6) of that form and
// reduces with the same butterfly; the 16 wave sums of a sample are exchanged (write-through payload, drained, then a ticket on the sample's arrival
// counter; write-through reads behind it: cdna_hip_programming.md G16 / MI355X_MICROARCH.md handoff-flag — the siblings sit on different XCDs) and
// EVERY sibling folds them with block_sum's second stage (lanes 0..15 hold the wave sums, one more butterfly).  The log-prob is therefore bit-equal
// to ppo_fwd_bwd_kernel's and to ddim_step_kernel's — the ratio of a sampled transition scored before the first update stays exactly 1
// (tests/test_gpu_f16mx_model.py::test_sampler_ratio_is_one_before_the_first_update_tiny; the first cluster form of this round summed per-slice
// partials and broke exactly that).  x' - mu stays in registers between the two phases: the inputs are read once, not twice.  The per-micro-batch
// info row is computed by the workgroup that completes the micro-batch (second arrival counter) with ppo_info_kernel's tree.  No release / acquire
// fence (an agent-scope release writes back the whole L2: the fenced form took 18 us against 13 for one workgroup per sample).  Counters live in
// device globals, are zero between launches (the last reader re-arms them) and are only ever touched by one launch at a time (the entry points are
// called from the training thread's stream only: SURVEY 8b).
#define PPO_MAXB 64
#define PPO_S 4
__device__ float g_ppo_part[PPO_MAXB * 16];
__device__ unsigned g_ppo_cnt[PPO_MAXB], g_ppo_done[PPO_MAXB], g_ppo_grp[PPO_MAXB];
__device__ unsigned g_ppo_timeout;               // != 0: a cluster gave up waiting (never observed)

template <int NV>
__global__ void __launch_bounds__(256) ppo_cluster_kernel(const float* __restrict__ eps_c, const float* __restrict__ eps_u,
                                                         const float* __restrict__ x, const float* __restrict__ x_next,
                                                         const int32_t* __restrict__ ts, const float* __restrict__ old_logp,
                                                         const float* __restrict__ adv_in, float g, float clip, int train_cfg,
                                                         ddpo_ddim_consts c, float* __restrict__ d_eps_c, float* __restrict__ d_eps_u,
                                                         float* __restrict__ per_sample, float* __restrict__ info, int group, int chw) {
  __shared__ float s_lp;
  __shared__ int s_last;
  const int b = blockIdx.x / PPO_S, sl = blockIdx.x - b * PPO_S;
  const int T = sl * 256 + (int)threadIdx.x;       // this thread's index in the 1024-thread form
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const DdimCoef k = ddim_coef(c, ts[b]);
  const int64_t base = (int64_t)b * chw;
  const int n4 = chw >> 2;
  const float inv2v = 1.0f / (2.0f * (k.std_c * k.std_c));
  const float cst = -logf(k.std_c) - LOG_SQRT_2PI;
  float4 dv[NV];                                   // x' - mu of this thread's elements (all the backward needs)
  float acc = 0.f;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int i4 = T + v * 1024;
    dv[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i4 < n4) {
      const int64_t o = base + (int64_t)i4 * 4;
      const float4 ec = *reinterpret_cast<const float4*>(eps_c + o);
      float4 eu = ec;
      if (train_cfg) eu = *reinterpret_cast<const float4*>(eps_u + o);
      const float4 xv = *reinterpret_cast<const float4*>(x + o);
      const float4 xn = *reinterpret_cast<const float4*>(x_next + o);
      const float* pec = &ec.x; const float* peu = &eu.x; const float* px = &xv.x; const float* pn = &xn.x;
      float* pd = &dv[v].x;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float e = train_cfg ? (peu[j] + g * (pec[j] - peu[j])) : pec[j];
        const float d = pn[j] - ddim_mean(k, c.pred_type, e, px[j]);
        acc += -(d * d) * inv2v + cst;
        pd[j] = d;
      }
    }
  }
  const float wsum = wave_sum(acc);                // == red[4 sl + wv] of the 1024-thread form
  if (lane == 0) __hip_atomic_store(&g_ppo_part[b * 16 + sl * 4 + wv], wsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (threadIdx.x == 0) s_last = 0;
  __syncthreads();                                 // the four wave sums of this workgroup are drained
  if (wv == 0) {
    if (lane == 0) {
      __hip_atomic_fetch_add(&g_ppo_cnt[b], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      int spin = 0;
      while (__hip_atomic_load(&g_ppo_cnt[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned)PPO_S) {
        __builtin_amdgcn_s_sleep(1);
        if (++spin > (1 << 24)) { g_ppo_timeout = 1u; break; }          // (every sibling is resident: 4 B <= 256 workgroups of 256 threads)
      }
    }
    // (lane 0 leaves its loop before the wave goes on: the loads below are behind the ticket)
    asm volatile("" ::: "memory");
    float t = (lane < 16) ? __hip_atomic_load(&g_ppo_part[b * 16 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
    t = wave_sum(t);                               // block_sum's second stage
    if (lane == 0) {
      s_lp = t / (float)chw;
      // the last sibling to have read the wave sums re-arms the sample's counters for the next launch
      if (__hip_atomic_fetch_add(&g_ppo_done[b], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(PPO_S - 1)) {
        __hip_atomic_store(&g_ppo_cnt[b], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&g_ppo_done[b], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  __syncthreads();
  const float lp = s_lp;
  const float A = fminf(fmaxf(adv_in[b], -10.0f), 10.0f);        // ADV_CLIP_MAX
  const float ratio = expf(lp - old_logp[b]);
  const float unclipped = -A * ratio;
  const float clipped = -A * fminf(fmaxf(ratio, 1.0f - clip), 1.0f + clip);
  const float dl = (unclipped >= clipped) ? (-A * ratio / (float)group) : 0.0f;
  if (sl == 0 && threadIdx.x == 0) {
    __hip_atomic_store(&per_sample[b * 4 + 0], lp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&per_sample[b * 4 + 1], ratio, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&per_sample[b * 4 + 2], fmaxf(unclipped, clipped), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&per_sample[b * 4 + 3], (fabsf(ratio - 1.0f) > clip) ? 1.0f : 0.0f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // micro-batch info: the workgroup that completes the micro-batch reduces its per-sample rows (write-through rows, drained, then the ticket)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int mb = b / group;
    if (__hip_atomic_fetch_add(&g_ppo_grp[mb], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(group - 1)) {
      __hip_atomic_store(&g_ppo_grp[mb], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_last = 1;
    }
  }
  float dmu_de;
  if (c.pred_type == DDPO_PRED_EPSILON) dmu_de = k.dirc - k.sqrt_ap * k.sqrt_bt / k.sqrt_at;
  else if (c.pred_type == DDPO_PRED_V) dmu_de = k.dirc * k.sqrt_at - k.sqrt_ap * k.sqrt_bt;
  else dmu_de = k.sqrt_ap;
  const float coef = dl * dmu_de / ((k.std_c * k.std_c) * (float)chw);
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int i4 = T + v * 1024;
    if (i4 < n4) {
      const int64_t o = base + (int64_t)i4 * 4;
      const float* pd = &dv[v].x;
      float4 dc, du;
      float* pdc = &dc.x; float* pdu = &du.x;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float de = coef * pd[j];
        pdc[j] = train_cfg ? g * de : de;
        pdu[j] = (1.0f - g) * de;
      }
      *reinterpret_cast<float4*>(d_eps_c + o) = dc;
      if (train_cfg) *reinterpret_cast<float4*>(d_eps_u + o) = du;
    }
  }
  __syncthreads();
  if (s_last && threadIdx.x < 64) {               // (ppo_info_kernel's reduction, lane for lane)
    const int b0 = (b / group) * group;
    float kl = 0.f, cf = 0.f, ls = 0.f;
    for (int q = b0 + (int)threadIdx.x; q < b0 + group; q += 64) {
      const float lpq = __hip_atomic_load(&per_sample[q * 4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const float d = lpq - old_logp[q];
      kl += d * d;
      cf += __hip_atomic_load(&per_sample[q * 4 + 3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ls += __hip_atomic_load(&per_sample[q * 4 + 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    kl = wave_sum(kl); cf = wave_sum(cf); ls = wave_sum(ls);
    if (threadIdx.x == 0) {
      info[(b / group) * 3 + 0] = 0.5f * kl / (float)group;
      info[(b / group) * 3 + 1] = cf / (float)group;
      info[(b / group) * 3 + 2] = ls / (float)group;
    }
  }
}

// one block per micro-batch (`group` consecutive rows): info[blockIdx.x] = {approx_kl, clipfrac, loss} of that micro-batch
__global__ void ppo_info_kernel(const float* __restrict__ per_sample, const float* __restrict__ old_logp,
                                float* __restrict__ info, int group) {
  const int b0 = blockIdx.x * group;
  float kl = 0.f, cf = 0.f, ls = 0.f;
  for (int b = b0 + threadIdx.x; b < b0 + group; b += 64) {
    const float d = per_sample[b * 4] - old_logp[b];
    kl += d * d;
    cf += per_sample[b * 4 + 3];
    ls += per_sample[b * 4 + 2];
  }
  kl = wave_sum(kl); cf = wave_sum(cf); ls = wave_sum(ls);
  if (threadIdx.x == 0) {
    info[blockIdx.x * 3 + 0] = 0.5f * kl / (float)group;
    info[blockIdx.x * 3 + 1] = cf / (float)group;
    info[blockIdx.x * 3 + 2] = ls / (float)group;
  }
}

extern "C" int ddpo_ddim_logprob_ppo_fwd_bwd(const float* eps_c, const float* eps_u, const float* x, const float* x_next,
                                             const int32_t* ts, const float* old_logp, const float* advantages,
                                             float guidance_scale, float clip_range, int train_cfg,
                                             const ddpo_ddim_consts* c, float* d_eps_c, float* d_eps_u, float* per_sample,
                                             float* info, int B, int group, int chw, void* stream) {
  if (!eps_c || !x || !x_next || !ts || !old_logp || !advantages || !c || !d_eps_c || !per_sample || !info) return DDPO_EINVAL;
  if (train_cfg && (!eps_u || !d_eps_u)) return DDPO_EINVAL;
  if (B <= 0 || group <= 0 || B % group || chw <= 0 || (chw & 3)) return DDPO_EINVAL;
  // cluster form: four workgroups of 256 threads per sample, all resident (4 B <= 256), each thread holding NV <= 16 float4 of x' - mu
  const int nv = ((chw >> 2) + 1023) / 1024;
  if (B <= PPO_MAXB && nv <= 16) {
    const dim3 grid(B * PPO_S), blk(256);
#define PPO_LAUNCH(NV) hipLaunchKernelGGL((ppo_cluster_kernel<NV>), grid, blk, 0, as_stream(stream), eps_c, eps_u, x, x_next, ts, old_logp, advantages, \
                                         guidance_scale, clip_range, train_cfg, *c, d_eps_c, d_eps_u, per_sample, info, group, chw)
    if (nv <= 1) PPO_LAUNCH(1); else if (nv <= 2) PPO_LAUNCH(2); else if (nv <= 4) PPO_LAUNCH(4); else if (nv <= 8) PPO_LAUNCH(8); else if (nv <= 12) PPO_LAUNCH(12);
    else PPO_LAUNCH(16);
#undef PPO_LAUNCH
    DDPO_LAUNCH_CHECK();
    return DDPO_OK;
  }
  hipLaunchKernelGGL(ppo_fwd_bwd_kernel, dim3(B), dim3(1024), 0, as_stream(stream), eps_c, eps_u, x, x_next, ts, old_logp,
                     advantages, guidance_scale, clip_range, train_cfg, *c, d_eps_c, d_eps_u, per_sample, group, chw);
  DDPO_LAUNCH_CHECK();
  hipLaunchKernelGGL(ppo_info_kernel, dim3(B / group), dim3(64), 0, as_stream(stream), per_sample, old_logp, info, group);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

// ------------------------------------------------------------------------------------------------
// RWR (reward-weighted regression) denoising step, /root/reference/ddpo/training/diffusion.py:19-90
//   rwr_noisy_latents: posterior sample of the stored VAE moments (FlaxDiagonalGaussianDistribution: mean, logvar clipped to
//     [-30, 20], std = exp(logvar / 2); sample = mean + std * e1), NHWC -> NCHW, x 0.18215, then the DDPM forward process
//     add_noise(latents, noise, t) = sqrt(acp[t]) * latents + sqrt(1 - acp[t]) * noise          (:20-44)
//   rwr_mse_fwd_bwd: noise_pred = eps_u + g (eps_c - eps_u) (train_cfg) or eps_c; loss_b = mean_chw (noise - noise_pred)^2;
//     loss = mean_b loss_b (weights == NULL) or sum_b w_b loss_b; gradients w.r.t. eps_c / eps_u in closed form      (:66-90)
// One workgroup per sample, float4 coalesced, fixed-order block reduction (bit-reproducible).  HBM-bound: 5 / 5 passes of 4*C*h*w B.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) rwr_noisy_latents_kernel(const float* __restrict__ moments, const float* __restrict__ e1,
                                                                const float* __restrict__ noise, const int32_t* __restrict__ ts,
                                                                const float* __restrict__ acp, int n_train, float scale,
                                                                float* __restrict__ latents, float* __restrict__ noisy, int C, int hw) {
  const int b = blockIdx.x;
  int t = ts[b];
  t = t < 0 ? 0 : (t >= n_train ? n_train - 1 : t);
  const float a = acp[t];
  const float sa = sqrtf(a), sb = sqrtf(1.0f - a);
  const int64_t mbase = (int64_t)b * hw * 2 * C, ebase = (int64_t)b * hw * C, obase = (int64_t)b * C * hw;
  for (int i = threadIdx.x; i < hw * C; i += blockDim.x) {
    const int p = i / C, c = i - p * C;                       // NHWC element (pixel p, channel c) of the posterior sample
    const float mean = moments[mbase + (int64_t)p * 2 * C + c];
    float logvar = moments[mbase + (int64_t)p * 2 * C + C + c];
    logvar = fminf(fmaxf(logvar, -30.0f), 20.0f);
    const float z = (mean + expf(0.5f * logvar) * e1[ebase + i]) * scale;
    const int64_t o = obase + (int64_t)c * hw + p;            // NCHW
    latents[o] = z;
    noisy[o] = sa * z + sb * noise[o];
  }
}

extern "C" int ddpo_rwr_noisy_latents(const float* moments, const float* e1, const float* noise, const int32_t* ts,
                                      const float* alphas_cumprod, int num_train_timesteps, float scale, float* latents,
                                      float* noisy, int B, int C, int hw, void* stream) {
  if (!moments || !e1 || !noise || !ts || !alphas_cumprod || !latents || !noisy || B <= 0 || C <= 0 || hw <= 0 || num_train_timesteps <= 0)
    return DDPO_EINVAL;
  hipLaunchKernelGGL(rwr_noisy_latents_kernel, dim3(B), dim3(256), 0, as_stream(stream), moments, e1, noise, ts, alphas_cumprod,
                     num_train_timesteps, scale, latents, noisy, C, hw);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

// The same pass with the regression target of the model's prediction type (include/ddpo_cfg_rescale.h): latents and noisy by the expressions
// above (bit-equal), target = noise | sa noise - sb latents (the v of Salimans & Ho) | latents.
__global__ void __launch_bounds__(256) rwr_noisy_latents_target_kernel(const float* __restrict__ moments, const float* __restrict__ e1,
                                                                       const float* __restrict__ noise, const int32_t* __restrict__ ts,
                                                                       const float* __restrict__ acp, int n_train, float scale,
                                                                       int pred_type, float* __restrict__ latents,
                                                                       float* __restrict__ noisy, float* __restrict__ target, int C, int hw) {
  const int b = blockIdx.x;
  int t = ts[b];
  t = t < 0 ? 0 : (t >= n_train ? n_train - 1 : t);
  const float a = acp[t];
  const float sa = sqrtf(a), sb = sqrtf(1.0f - a);
  const int64_t mbase = (int64_t)b * hw * 2 * C, ebase = (int64_t)b * hw * C, obase = (int64_t)b * C * hw;
  for (int i = threadIdx.x; i < hw * C; i += blockDim.x) {
    const int p = i / C, c = i - p * C;
    const float mean = moments[mbase + (int64_t)p * 2 * C + c];
    float logvar = moments[mbase + (int64_t)p * 2 * C + C + c];
    logvar = fminf(fmaxf(logvar, -30.0f), 20.0f);
    const float z = (mean + expf(0.5f * logvar) * e1[ebase + i]) * scale;
    const int64_t o = obase + (int64_t)c * hw + p;
    const float nz = noise[o];
    latents[o] = z;
    noisy[o] = sa * z + sb * nz;
    target[o] = pred_type == DDPO_PRED_EPSILON ? nz : (pred_type == DDPO_PRED_V ? sa * nz - sb * z : z);
  }
}

extern "C" int ddpo_rwr_noisy_latents_target(const float* moments, const float* e1, const float* noise, const int32_t* ts,
                                             const float* alphas_cumprod, int num_train_timesteps, float scale, int pred_type,
                                             float* latents, float* noisy, float* target, int B, int C, int hw, void* stream) {
  if (!moments || !e1 || !noise || !ts || !alphas_cumprod || !latents || !noisy || !target || B <= 0 || C <= 0 || hw <= 0 ||
      num_train_timesteps <= 0)
    return DDPO_EINVAL;
  if (pred_type != DDPO_PRED_EPSILON && pred_type != DDPO_PRED_V && pred_type != DDPO_PRED_SAMPLE) return DDPO_EINVAL;
  hipLaunchKernelGGL(rwr_noisy_latents_target_kernel, dim3(B), dim3(256), 0, as_stream(stream), moments, e1, noise, ts, alphas_cumprod,
                     num_train_timesteps, scale, pred_type, latents, noisy, target, C, hw);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

__global__ void __launch_bounds__(1024) rwr_mse_fwd_bwd_kernel(const float* __restrict__ eps_c, const float* __restrict__ eps_u,
                                                              const float* __restrict__ noise, const float* __restrict__ weights,
                                                              float g, int train_cfg, float* __restrict__ d_c, float* __restrict__ d_u,
                                                              float* __restrict__ per_sample, int B, int chw) {
  __shared__ float red[16];
  const int b = blockIdx.x;
  const int64_t base = (int64_t)b * chw;
  const float wb = weights ? weights[b] : 1.0f / (float)B;
  const float coef = -2.0f * wb / (float)chw;                 // d loss / d noise_pred = -2 w_b (noise - noise_pred) / CHW
  float acc = 0.f;
  for (int i = threadIdx.x * 4; i < chw; i += blockDim.x * 4) {
    const float4 ec = *reinterpret_cast<const float4*>(eps_c + base + i);
    float4 eu = ec;
    if (train_cfg) eu = *reinterpret_cast<const float4*>(eps_u + base + i);
    const float4 nz = *reinterpret_cast<const float4*>(noise + base + i);
    const float* pec = &ec.x; const float* peu = &eu.x; const float* pn = &nz.x;
    float4 dc, du;
    float* pdc = &dc.x; float* pdu = &du.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float pred = train_cfg ? (peu[j] + g * (pec[j] - peu[j])) : pec[j];
      const float r = pn[j] - pred;
      acc += r * r;
      const float dp = coef * r;
      pdc[j] = train_cfg ? g * dp : dp;
      pdu[j] = (1.0f - g) * dp;
    }
    *reinterpret_cast<float4*>(d_c + base + i) = dc;
    if (train_cfg) *reinterpret_cast<float4*>(d_u + base + i) = du;
  }
  const float tot = block_sum(acc, red);
  if (threadIdx.x == 0) { per_sample[b * 2] = tot / (float)chw; per_sample[b * 2 + 1] = wb * (tot / (float)chw); }
}

__global__ void rwr_loss_kernel(const float* __restrict__ per_sample, float* __restrict__ loss, int B) {
  float s = 0.f;
  for (int b = threadIdx.x; b < B; b += 64) s += per_sample[b * 2 + 1];
  s = wave_sum(s);
  if (threadIdx.x == 0) *loss = s;
}

extern "C" int ddpo_rwr_mse_fwd_bwd(const float* eps_c, const float* eps_u, const float* noise, const float* weights,
                                    float guidance_scale, int train_cfg, float* d_eps_c, float* d_eps_u, float* per_sample,
                                    float* loss, int B, int chw, void* stream) {
  if (!eps_c || !noise || !d_eps_c || !per_sample || !loss || B <= 0 || chw <= 0 || (chw & 3)) return DDPO_EINVAL;
  if (train_cfg && (!eps_u || !d_eps_u)) return DDPO_EINVAL;
  hipLaunchKernelGGL(rwr_mse_fwd_bwd_kernel, dim3(B), dim3(1024), 0, as_stream(stream), eps_c, eps_u, noise, weights, guidance_scale,
                     train_cfg, d_eps_c, d_eps_u, per_sample, B, chw);
  DDPO_LAUNCH_CHECK();
  hipLaunchKernelGGL(rwr_loss_kernel, dim3(1), dim3(64), 0, as_stream(stream), per_sample, loss, B);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

// ------------------------------------------------------------------------------------------------
// optimizer (optax clip_by_global_norm + adamw(mu_dtype=bf16)); 24 B/param of HBM traffic per update
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) sqnorm_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ out) {
  __shared__ double red[4];
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  const int64_t n4 = n >> 2;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = g4[i];
    a0 += v.x * v.x; a1 += v.y * v.y; a2 += v.z * v.z; a3 += v.w * v.w;
  }
  double s = (double)a0 + (double)a1 + (double)a2 + (double)a3;
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t i = n4 << 2; i < n; ++i) s += (double)g[i] * (double)g[i];
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out, red[0] + red[1] + red[2] + red[3]);
}

extern "C" int ddpo_grad_sqnorm(const float* g, int64_t n, double* out_sq, int zero_first, void* stream) {
  if (!g || !out_sq || n <= 0 || (reinterpret_cast<uintptr_t>(g) & 15)) return DDPO_EINVAL;
  if (zero_first && hipMemsetAsync(out_sq, 0, sizeof(double), as_stream(stream)) != hipSuccess) return DDPO_ELAUNCH;
  int64_t blocks = ((n >> 2) + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(sqnorm_kernel, dim3((int)blocks), dim3(256), 0, as_stream(stream), g, n, out_sq);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

__device__ __forceinline__ float bf16_bits_to_f32(uint16_t h) { return __uint_as_float(((uint32_t)h) << 16); }
__device__ __forceinline__ uint16_t f32_to_bf16_rne(float f) {
  uint32_t b = __float_as_uint(f);
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((b >> 16) | 0x40);   // NaN stays NaN
  b += 0x7FFFu + ((b >> 16) & 1u);
  return (uint16_t)(b >> 16);
}
__device__ __forceinline__ float bf16_round_f(float f) { return bf16_bits_to_f32(f32_to_bf16_rne(f)); }

struct AdamArgs {
  float inv_n, lr_neg, b1, omb1, b1_bf16, b2, omb2, eps, wd, max_norm, bc1, bc2;
  int mu_decay_in_bf16, zero_grad;
};

__device__ __forceinline__ void adam_one(float& p, float& g, uint16_t& mu, float& nu, const AdamArgs& a, bool clip, float norm) {
  float ge = g * a.inv_n;
  if (clip) ge = (ge / norm) * a.max_norm;
  const float m_old = bf16_bits_to_f32(mu);
  const float decayed = a.mu_decay_in_bf16 ? bf16_round_f(a.b1_bf16 * m_old) : a.b1 * m_old;
  const float m = a.omb1 * ge + decayed;
  const float v = a.omb2 * (ge * ge) + a.b2 * nu;
  float u = (m / a.bc1) / (sqrtf(v / a.bc2) + a.eps);
  u = u + a.wd * p;
  p = p + a.lr_neg * u;
  mu = f32_to_bf16_rne(m);
  nu = v;
  if (a.zero_grad) g = 0.f;
}

__global__ void __launch_bounds__(256) adamw_kernel(float* __restrict__ p, float* __restrict__ g, uint16_t* __restrict__ mu,
                                                    float* __restrict__ nu, int64_t n, const double* __restrict__ sqn,
                                                    AdamArgs a) {
  const float norm = (float)sqrt(*sqn) * a.inv_n;       // ||g_sum * inv_n||
  const bool clip = !(norm < a.max_norm);
  const int64_t n4 = n >> 2;
  float4* p4 = reinterpret_cast<float4*>(p);
  float4* g4 = reinterpret_cast<float4*>(g);
  float4* v4 = reinterpret_cast<float4*>(nu);
  ushort4* m4 = reinterpret_cast<ushort4*>(mu);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    float4 pv = p4[i], gv = g4[i], vv = v4[i];
    ushort4 mv = m4[i];
    adam_one(pv.x, gv.x, mv.x, vv.x, a, clip, norm);
    adam_one(pv.y, gv.y, mv.y, vv.y, a, clip, norm);
    adam_one(pv.z, gv.z, mv.z, vv.z, a, clip, norm);
    adam_one(pv.w, gv.w, mv.w, vv.w, a, clip, norm);
    p4[i] = pv; v4[i] = vv; m4[i] = mv;
    if (a.zero_grad) g4[i] = gv;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t i = n4 << 2; i < n; ++i) adam_one(p[i], g[i], mu[i], nu[i], a, clip, norm);
}

extern "C" int ddpo_adamw_bf16mu_step(float* p, float* g, uint16_t* mu, float* nu, int64_t n, const double* sqnorm_of_sum,
                                      double inv_n_acc, double lr, double b1, double b2, double eps, double weight_decay,
                                      double max_grad_norm, int step_t, int mu_decay_in_bf16, int zero_grad, void* stream) {
  if (!p || !g || !mu || !nu || !sqnorm_of_sum || n <= 0 || step_t < 1) return DDPO_EINVAL;
  if ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(nu)) & 15) return DDPO_EINVAL;
  if (reinterpret_cast<uintptr_t>(mu) & 7) return DDPO_EINVAL;
  AdamArgs a;
  a.inv_n = (float)inv_n_acc;
  a.lr_neg = (float)(-lr);
  a.b1 = (float)b1;
  a.omb1 = (float)(1.0 - b1);
  // weak-typed Python scalar times a bf16 array: the scalar itself is rounded to bf16 first (jax promotion rules)
  {
    union { float f; uint32_t u; } cv; cv.f = (float)b1;
    uint32_t r = cv.u + 0x7FFFu + ((cv.u >> 16) & 1u);
    cv.u = r & 0xFFFF0000u;
    a.b1_bf16 = cv.f;
  }
  a.b2 = (float)b2;
  a.omb2 = (float)(1.0 - b2);
  a.eps = (float)eps;
  a.wd = (float)weight_decay;
  a.max_norm = (float)max_grad_norm;
  a.bc1 = 1.0f - powf((float)b1, (float)step_t);
  a.bc2 = 1.0f - powf((float)b2, (float)step_t);
  a.mu_decay_in_bf16 = mu_decay_in_bf16;
  a.zero_grad = zero_grad;
  int64_t blocks = ((n >> 2) + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(adamw_kernel, dim3((int)blocks), dim3(256), 0, as_stream(stream), p, g, mu, nu, n, sqnorm_of_sum, a);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

// ------------------------------------------------------------------------------------------------
// small element-wise kernels of the U-Net / VAE
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) geglu_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t rows, int F) {
  const int f4 = F >> 2;
  const int64_t total = rows * f4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / f4;
    const int c = (int)(i - r * f4) << 2;
    const float4 a = *reinterpret_cast<const float4*>(x + r * (2 * (int64_t)F) + c);
    const float4 b = *reinterpret_cast<const float4*>(x + r * (2 * (int64_t)F) + F + c);
    float4 o;
    o.x = a.x * gelu_tanh_f(b.x); o.y = a.y * gelu_tanh_f(b.y); o.z = a.z * gelu_tanh_f(b.z); o.w = a.w * gelu_tanh_f(b.w);
    *reinterpret_cast<float4*>(y + r * (int64_t)F + c) = o;
  }
}
extern "C" int ddpo_geglu_fwd(const float* x, float* y, int64_t rows, int F, void* stream) {
  if (!x || !y || rows <= 0 || F <= 0 || (F & 3)) return DDPO_EINVAL;
  int64_t blocks = (rows * (F >> 2) + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(geglu_kernel, dim3((int)blocks), dim3(256), 0, as_stream(stream), x, y, rows, F);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

__global__ void __launch_bounds__(256) silu_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) y[i] = silu_f(x[i]);
}
extern "C" int ddpo_silu_fwd(const float* x, float* y, int64_t n, void* stream) {
  if (!x || !y || n <= 0) return DDPO_EINVAL;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(silu_kernel, dim3((int)blocks), dim3(256), 0, as_stream(stream), x, y, n);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

// quick-GELU of the OpenAI CLIP towers (reward model, /root/reference/ddpo/training/callbacks.py:60-95 -> transformers' `quick_gelu`):
// y = x * sigmoid(1.702 x).  float4 per lane; HBM-bound (8 B / element).
__global__ void __launch_bounds__(256) quick_gelu_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n4, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    float4 v = reinterpret_cast<const float4*>(x)[i];
    v.x = v.x / (1.f + __expf(-1.702f * v.x)); v.y = v.y / (1.f + __expf(-1.702f * v.y));
    v.z = v.z / (1.f + __expf(-1.702f * v.z)); v.w = v.w / (1.f + __expf(-1.702f * v.w));
    reinterpret_cast<float4*>(y)[i] = v;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {          // ragged tail (n % 4 elements)
    const int64_t i = (n & ~(int64_t)3) + threadIdx.x;
    y[i] = x[i] / (1.f + __expf(-1.702f * x[i]));
  }
}
extern "C" int ddpo_quick_gelu_fwd(const float* x, float* y, int64_t n, void* stream) {
  if (!x || !y || n <= 0 || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15)) return DDPO_EINVAL;
  int64_t blocks = ((n >> 2) + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(quick_gelu_kernel, dim3((int)blocks), dim3(256), 0, as_stream(stream), x, y, n >> 2, n);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

// y[r, :] = x[r, :] / ||x[r, :]||_2  (image_features / norm of the aesthetic reward, callbacks.py:80-82); one wave per row, the
// sum of squares is a wavefront shuffle reduction in a fixed order (bit-reproducible).
__global__ void __launch_bounds__(256) l2_normalize_rows_kernel(const float* __restrict__ x, float* __restrict__ y, int rows, int cols) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* xr = x + (int64_t)row * cols;
  float ss = 0.f;
  for (int c = lane; c < cols; c += 64) ss += xr[c] * xr[c];
  ss = wave_sum(ss);
  const float inv = 1.f / sqrtf(ss);
  float* yr = y + (int64_t)row * cols;
  for (int c = lane; c < cols; c += 64) yr[c] = xr[c] * inv;
}
extern "C" int ddpo_l2_normalize_rows(const float* x, float* y, int rows, int cols, void* stream) {
  if (!x || !y || rows <= 0 || cols <= 0) return DDPO_EINVAL;
  hipLaunchKernelGGL(l2_normalize_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, as_stream(stream), x, y, rows, cols);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

// get_sinusoidal_embeddings(flip_sin_to_cos=True, freq_shift=0): out[b] = concat(cos(t f_i), sin(t f_i)), f_i = 1e4^(-i/half)
__global__ void timestep_embedding_kernel(const int32_t* __restrict__ ts, float* __restrict__ out, int B, int dim) {
  const int half = dim >> 1;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * half) return;
  const int b = i / half, j = i - b * half;
  const float freq = expf(-9.210340371976184f * (float)j / (float)half);
  const float arg = (float)ts[b] * freq;
  out[b * dim + j] = cosf(arg);
  out[b * dim + half + j] = sinf(arg);
}
extern "C" int ddpo_timestep_embedding(const int32_t* ts, float* out, int B, int dim, void* stream) {
  if (!ts || !out || B <= 0 || dim <= 0 || (dim & 1)) return DDPO_EINVAL;
  const int n = B * (dim >> 1);
  hipLaunchKernelGGL(timestep_embedding_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream), ts, out, B, dim);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

// (B,C,HW) <-> (B,HW,C) for small C (latents: C = 4; images: C = 3)
__global__ void __launch_bounds__(256) nchw_to_nhwc_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int C, int HW) {
  const int64_t total = (int64_t)B * HW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / HW, p = i - b * HW;
    for (int c = 0; c < C; ++c) y[i * C + c] = x[(b * C + c) * HW + p];
  }
}
__global__ void __launch_bounds__(256) nhwc_to_nchw_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int C, int HW) {
  const int64_t total = (int64_t)B * HW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / HW, p = i - b * HW;
    for (int c = 0; c < C; ++c) y[(b * C + c) * HW + p] = x[i * C + c];
  }
}
extern "C" int ddpo_nchw_to_nhwc(const float* x, float* y, int B, int C, int HW, void* stream) {
  if (!x || !y || B <= 0 || C <= 0 || HW <= 0) return DDPO_EINVAL;
  int64_t blocks = ((int64_t)B * HW + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3((int)blocks), dim3(256), 0, as_stream(stream), x, y, B, C, HW);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}
extern "C" int ddpo_nhwc_to_nchw(const float* x, float* y, int B, int C, int HW, void* stream) {
  if (!x || !y || B <= 0 || C <= 0 || HW <= 0) return DDPO_EINVAL;
  int64_t blocks = ((int64_t)B * HW + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3((int)blocks), dim3(256), 0, as_stream(stream), x, y, B, C, HW);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

// strided column-block copy (materialises the skip concat: dst[:, off:off+cols] = src)
__global__ void __launch_bounds__(256) copy_cols_kernel(const float* __restrict__ src, int ld_src, float* __restrict__ dst,
                                                        int ld_dst, int64_t rows, int cols4) {
  const int64_t total = rows * cols4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cols4;
    const int c = (int)(i - r * cols4) << 2;
    *reinterpret_cast<float4*>(dst + r * ld_dst + c) = *reinterpret_cast<const float4*>(src + r * ld_src + c);
  }
}
extern "C" int ddpo_copy_cols(const float* src, int ld_src, float* dst, int ld_dst, int64_t rows, int cols, void* stream) {
  if (!src || !dst || rows <= 0 || cols <= 0 || (cols & 3) || (ld_src & 3) || (ld_dst & 3)) return DDPO_EINVAL;
  if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) return DDPO_EINVAL;
  int64_t blocks = (rows * (cols >> 2) + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(copy_cols_kernel, dim3((int)blocks), dim3(256), 0, as_stream(stream), src, ld_src, dst, ld_dst, rows, cols >> 2);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

// Inputs of one classifier-free-guidance sampling step into the static buffers of the captured U-Net graph, in ONE launch (round 6; VERDICT r05
// weak 8: six stock copy launches per step): s_in = [x; x] (jnp.concatenate([latents] * 2), pipeline_flax_stable_diffusion.py:219), the step's row
// of the time-projection table into the row the ResBlocks' rowbias operands point at, the step's timesteps.  Any of the last two may be absent.
__global__ void __launch_bounds__(256) stage_cfg_inputs_kernel(const float* __restrict__ x, float* __restrict__ s_in, int64_t n4,
                                                               const float* __restrict__ row_src, float* __restrict__ row_dst, int row4,
                                                               const int32_t* __restrict__ ts_src, int32_t* __restrict__ ts_dst, int ts_n) {
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = i0; i < n4; i += stride) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    reinterpret_cast<float4*>(s_in)[i] = v;
    reinterpret_cast<float4*>(s_in)[n4 + i] = v;
  }
  for (int64_t i = i0; i < row4; i += stride) reinterpret_cast<float4*>(row_dst)[i] = reinterpret_cast<const float4*>(row_src)[i];
  for (int64_t i = i0; i < ts_n; i += stride) ts_dst[i] = ts_src[i];
}
extern "C" int ddpo_stage_cfg_inputs(const float* x, float* s_in, int64_t n, const float* row_src, float* row_dst, int row_n,
                                     const int32_t* ts_src, int32_t* ts_dst, int ts_n, void* stream) {
  if (!x || !s_in || n <= 0 || (n & 3) || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(s_in)) & 15)) return DDPO_EINVAL;
  if ((row_src == nullptr) != (row_dst == nullptr) || (ts_src == nullptr) != (ts_dst == nullptr) || row_n < 0 || ts_n < 0) return DDPO_EINVAL;
  if (row_src && ((row_n & 3) || ((reinterpret_cast<uintptr_t>(row_src) | reinterpret_cast<uintptr_t>(row_dst)) & 15))) return DDPO_EINVAL;
  int64_t blocks = ((n >> 2) + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(stage_cfg_inputs_kernel, dim3((int)blocks), dim3(256), 0, as_stream(stream), x, s_in, n >> 2, row_src, row_dst,
                     row_src ? row_n >> 2 : 0, ts_src, ts_dst, ts_src ? ts_n : 0);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

// in-place row softmax of scale*x (VAE mid-block attention, single head, materialised scores)
__global__ void __launch_bounds__(256) softmax_rows_kernel(float* __restrict__ x, int64_t rows, int cols, float scale) {
  __shared__ float red[16];
  for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
    float* row = x + r * (int64_t)cols;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < cols; i += blockDim.x) m = fmaxf(m, row[i] * scale);
    m = wave_max(m);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float s = 0.f;
    for (int i = threadIdx.x; i < cols; i += blockDim.x) {
      const float e = expf(row[i] * scale - m);
      row[i] = e;
      s += e;
    }
    s = block_sum(s, red);
    const float inv = 1.0f / s;
    for (int i = threadIdx.x; i < cols; i += blockDim.x) row[i] *= inv;
    __syncthreads();
  }
}
extern "C" int ddpo_softmax_rows(float* x, int64_t rows, int cols, float scale, void* stream) {
  if (!x || rows <= 0 || cols <= 0) return DDPO_EINVAL;
  int64_t blocks = rows > 65535 ? 65535 : rows;
  hipLaunchKernelGGL(softmax_rows_kernel, dim3((int)blocks), dim3(256), 0, as_stream(stream), x, rows, cols, scale);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

__global__ void __launch_bounds__(256) scale_shift_clip_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n,
                                                               float scale, float shift, float lo, float hi) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = fminf(fmaxf(x[i] * scale + shift, lo), hi);
}
extern "C" int ddpo_scale_shift_clip(const float* x, float* y, int64_t n, float scale, float shift, float lo, float hi, void* stream) {
  if (!x || !y || n <= 0) return DDPO_EINVAL;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(scale_shift_clip_kernel, dim3((int)blocks), dim3(256), 0, as_stream(stream), x, y, n, scale, shift, lo, hi);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}
