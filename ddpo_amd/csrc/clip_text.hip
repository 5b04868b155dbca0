// Kernels of the CLIP text tower and of the CLIPScore reward (models/clip_text.py, models/clip_score.py): causal self-attention for
// sequences of at most 80 tokens, an embedding-row gather and a row-wise cosine.  Exact-fp32 MFMA (v_mfma_f32_16x16x4_f32) like attention.hip:
// the reward models stay fp32-class whatever datapath the sampler runs, and 77 tokens are too few for a faster datapath to pay.
//
// ddpo_attention_causal_fwd — work split: ONE workgroup per (prompt, head), five waves, wave w owns queries [16w, 16w + 16).
//   * All of K and V of the (prompt, head) — at most 80 rows — are staged in LDS ONCE (80 x 66 + 80 x 68 floats = 42.9 KB at d = 64); rows
//     from N up to the next multiple of 16 are zero-filled so the last tile's MFMAs read finite values.
//   * Wave w visits key tiles 0 .. w only: a 16-key tile that lies wholly above the diagonal of the wave's queries issues no MFMA (15 of the
//     25 (wave, tile) products remain), tiles below the diagonal need no mask at all (their keys are < 16w <= every query of the wave, and a
//     wave with 16w >= N exits after the staging barrier), and the diagonal tile w masks per element with key - 16w > query - 16w.  That mask
//     also covers the ragged end: a stored query is < N, so every key it keeps is < N too.
//   * Every score of a query is in registers at once (at most 5 tiles x 4), so the softmax is the plain two-pass one: exact row maximum,
//     exp2, sum — no running rescale.  Key 0 is visible to every query, so the maximum is always finite.
// Products are computed transposed exactly as in attention.hip (S^T = K Q^T, O^T = V^T P^T: a query is a lane column in both, the C layout of
// the first product is the B layout of the second), with the same LDS row strides (K: d + 2, V: d + 4 floats).
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define CAUSAL_MAX_N 80
#define CAUSAL_TILES (CAUSAL_MAX_N / 16)

template <int D>
__global__ void __launch_bounds__(64 * CAUSAL_TILES) attn_causal_fwd_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k, int ldk,
                                                                            const float* __restrict__ v, int ldv, float* __restrict__ o, int ldo,
                                                                            int heads, int N, float scale_log2e) {
  constexpr int LDK = D + 2;
  constexpr int LDV = D + 4;
  constexpr int NS = D / 4;         // k-steps of the S^T product
  constexpr int NN = D / 16;        // d sub-tiles of O^T
  constexpr int NT = CAUSAL_TILES;
  __shared__ __attribute__((aligned(16))) float Ks[CAUSAL_MAX_N * LDK];
  __shared__ __attribute__((aligned(16))) float Vs[CAUSAL_MAX_N * LDV];

  const int t = threadIdx.x, lane = t & 63;
  const int wid = __builtin_amdgcn_readfirstlane(t >> 6);
  const int qi = lane & 15, g = lane >> 4;
  const int bh = blockIdx.x, b = bh / heads, h = bh - b * heads;
  const int q0 = wid * 16;

  // ---- stage K and V rows [0, N) once; zero rows [N, 16 * ceil(N / 16))
  {
    const float* kb = k + (int64_t)b * N * ldk + h * D;
    const float* vb = v + (int64_t)b * N * ldv + h * D;
    const int rows = (N + 15) & ~15;
    for (int i = t; i < rows * (D / 4); i += 64 * NT) {
      const int key = i / (D / 4), c4 = i - key * (D / 4);
      float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
      if (key < N) {
        kv = *reinterpret_cast<const float4*>(kb + (int64_t)key * ldk + c4 * 4);
        vv = *reinterpret_cast<const float4*>(vb + (int64_t)key * ldv + c4 * 4);
      }
      float2* kd = reinterpret_cast<float2*>(&Ks[key * LDK + c4 * 4]);
      kd[0] = make_float2(kv.x, kv.y);
      kd[1] = make_float2(kv.z, kv.w);
      *reinterpret_cast<float4*>(&Vs[key * LDV + c4 * 4]) = vv;
    }
  }
  __syncthreads();
  if (q0 >= N) return;              // (the only barrier is behind us)

  float qr[NS];
  {
    const int qrow = min(q0 + qi, N - 1);
    const float* qp = q + ((int64_t)b * N + qrow) * ldq + h * D + g;
#pragma unroll
    for (int s = 0; s < NS; ++s) qr[s] = qp[4 * s] * scale_log2e;
  }

  // ---- S^T = K Q^T over the tiles at or below the diagonal
  f32x4 sacc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    sacc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (j <= wid) {
#pragma unroll
      for (int s = 0; s < NS; ++s) sacc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ks[(j * 16 + qi) * LDK + 4 * s + g], qr[s], sacc[j], 0, 0, 0);
    }
  }
  // ---- softmax (query = lane column; keys = 4 lane groups x 4 regs x (wid + 1) tiles); only the diagonal tile is masked
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    if (j <= wid) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (j == wid && g * 4 + r > qi) sacc[j][r] = -INFINITY;
        mx = fmaxf(mx, sacc[j][r]);
      }
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  float ls = 0.f;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    if (j <= wid) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = exp2f(sacc[j][r] - mx);
        sacc[j][r] = p;
        ls += p;
      }
    }
  }
  ls += __shfl_xor(ls, 16, 64);
  ls += __shfl_xor(ls, 32, 64);

  // ---- O^T = V^T P^T
  f32x4 oacc[NN];
#pragma unroll
  for (int n = 0; n < NN; ++n) oacc[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    if (j <= wid) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* vrow = &Vs[(j * 16 + g * 4 + r) * LDV + qi];
        const float p = sacc[j][r];
#pragma unroll
        for (int n = 0; n < NN; ++n) oacc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(vrow[n * 16], p, oacc[n], 0, 0, 0);
      }
    }
  }

  if (q0 + qi < N) {
    const float inv = 1.0f / ls;
    float* op = o + ((int64_t)b * N + q0 + qi) * ldo + h * D + g * 4;
#pragma unroll
    for (int n = 0; n < NN; ++n)
      *reinterpret_cast<float4*>(op + n * 16) = make_float4(oacc[n][0] * inv, oacc[n][1] * inv, oacc[n][2] * inv, oacc[n][3] * inv);
  }
}

template <int D>
static int launch_causal(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* o, int ldo, int B, int heads, int N,
                         float scale, hipStream_t st) {
  hipLaunchKernelGGL((attn_causal_fwd_kernel<D>), dim3(B * heads), dim3(64 * CAUSAL_TILES), 0, st, q, ldq, k, ldk, v, ldv, o, ldo, heads, N,
                     scale * 1.4426950408889634f);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

extern "C" int ddpo_attention_causal_fwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* o, int ldo,
                                         int B, int heads, int N, int d, float scale, void* stream) {
  if (!q || !k || !v || !o || B <= 0 || heads <= 0 || N <= 0 || N > CAUSAL_MAX_N) return DDPO_EINVAL;
  if ((ldq & 3) || (ldk & 3) || (ldv & 3) || (ldo & 3)) return DDPO_EINVAL;
  const int C = heads * d;
  if (d <= 0 || ldq < C || ldk < C || ldv < C || ldo < C) return DDPO_EINVAL;
  if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) |
       reinterpret_cast<uintptr_t>(o)) & 15) return DDPO_EINVAL;
  if ((long)B * heads > 0x7fffffffL) return DDPO_EINVAL;
  hipStream_t st = as_stream(stream);
  switch (d) {
    case 16: return launch_causal<16>(q, ldq, k, ldk, v, ldv, o, ldo, B, heads, N, scale, st);
    case 64: return launch_causal<64>(q, ldq, k, ldk, v, ldv, o, ldo, B, heads, N, scale, st);
    default: return DDPO_EINVAL;
  }
}

// out[r] = table[idx[r]] (+ add[r % add_period]): one thread per 16-byte piece of an output row.  An index outside [0, table_rows) is CLAMPED
// into the table (no read outside it); the Python wrapper validates the indices on the host before they are uploaded.
__global__ void __launch_bounds__(256) gather_rows_kernel(const float* __restrict__ table, int ld, int table_rows, const int32_t* __restrict__ idx,
                                                          int64_t total4, int cols4, const float* __restrict__ add, int add_period,
                                                          float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const int64_t r = i / cols4;
  const int c4 = (int)(i - r * cols4);
  const int src = min(max(idx[r], 0), table_rows - 1);
  float4 x = *reinterpret_cast<const float4*>(table + (int64_t)src * ld + c4 * 4);
  if (add) {
    const float4 a = *reinterpret_cast<const float4*>(add + (r % add_period) * (int64_t)(cols4 * 4) + c4 * 4);
    x.x += a.x; x.y += a.y; x.z += a.z; x.w += a.w;
  }
  *reinterpret_cast<float4*>(out + r * (int64_t)(cols4 * 4) + c4 * 4) = x;
}

extern "C" int ddpo_gather_rows(const float* table, int ld, int table_rows, const int32_t* idx, int rows, int cols, const float* add,
                                int add_period, float* out, void* stream) {
  if (!table || !idx || !out || table_rows <= 0 || rows <= 0 || cols <= 0) return DDPO_EINVAL;
  if ((cols & 3) || (ld & 3) || ld < cols || (add && add_period <= 0)) return DDPO_EINVAL;
  if ((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(add)) & 15) return DDPO_EINVAL;
  if (reinterpret_cast<uintptr_t>(idx) & 3) return DDPO_EINVAL;
  const int64_t total4 = (int64_t)rows * (cols / 4);
  const int64_t blocks = (total4 + 255) / 256;
  if (blocks > 0x7fffffffL) return DDPO_EINVAL;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), table, ld, table_rows, idx, total4, cols / 4, add,
                     add_period, out);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

// out[r] = scale * <a_r, b_r> / (|a_r| |b_r|): one wave per row, each lane sums its 16-byte pieces in column order, then the butterfly of
// wave_sum — a fixed order, no atomics.  A zero row gives NaN (0 / 0), as the two separate normalisations would.
__global__ void __launch_bounds__(256) cosine_rows_kernel(const float* __restrict__ a, const float* __restrict__ b, int rows, int cols4, float scale,
                                                          float* __restrict__ out) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float4* ar = reinterpret_cast<const float4*>(a + (int64_t)row * cols4 * 4);
  const float4* br = reinterpret_cast<const float4*>(b + (int64_t)row * cols4 * 4);
  float ab = 0.f, aa = 0.f, bb = 0.f;
  for (int c = lane; c < cols4; c += 64) {
    const float4 x = ar[c], y = br[c];
    ab += x.x * y.x; ab += x.y * y.y; ab += x.z * y.z; ab += x.w * y.w;
    aa += x.x * x.x; aa += x.y * x.y; aa += x.z * x.z; aa += x.w * x.w;
    bb += y.x * y.x; bb += y.y * y.y; bb += y.z * y.z; bb += y.w * y.w;
  }
  ab = wave_sum(ab);
  aa = wave_sum(aa);
  bb = wave_sum(bb);
  if (lane == 0) out[row] = scale * (ab / (sqrtf(aa) * sqrtf(bb)));
}

extern "C" int ddpo_cosine_rows(const float* a, const float* b, int rows, int cols, float scale, float* out, void* stream) {
  if (!a || !b || !out || rows <= 0 || cols <= 0 || (cols & 3)) return DDPO_EINVAL;
  if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) return DDPO_EINVAL;
  hipLaunchKernelGGL(cosine_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, as_stream(stream), a, b, rows, cols / 4, scale, out);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}
