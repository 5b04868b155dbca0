// LoRA adapters on the U-Net attention projections (merged-weight design):
//   ddpo_lora_merge  W' = W0 + s * A B for a whole table of layers in one launch (memory-bound: W0 read once, W' written once, 16-byte accesses)
//   ddpo_lora_wgrad  dA += s * x^T (dY B^T),  dB += s * (x A)^T dY — the adapter gradients of one layer, x as fp32 rows or bf16 hi / lo planes
// Both are bitwise reproducible: fixed summation orders, no float atomics (per-workgroup partial slabs, a fixed-order reduction).
#include "common.h"

// ------------------------------------------------------------------------------------------------ merge
// One thread = 4 consecutive columns of one row k: W'[k, n..n+3] = W0[k, n..n+3] + s * sum_{j = 0..r-1} A[k, j] * B[j, n..n+3], j ascending.
// blockIdx.y = layer; blockIdx.x strides over the layer's K * N / 4 float4 groups.  A zero update leaves W0's bits (also a -0.0) in place.
__global__ void __launch_bounds__(256) lora_merge_kernel(const ddpo_lora_layer* __restrict__ table) {
  const ddpo_lora_layer L = table[blockIdx.y];
  const unsigned N4 = (unsigned)L.N >> 2, n4 = (unsigned)L.K * N4;      // K * N < 2^33 (ddpo_lora_merge)
  const float4* __restrict__ w0 = reinterpret_cast<const float4*>(L.w0);
  float4* __restrict__ w = reinterpret_cast<float4*>(L.w);
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += gridDim.x * blockDim.x) {
    const unsigned k = i / N4, c4 = i - k * N4;
    const float* __restrict__ arow = L.a + (int64_t)k * L.r;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < L.r; ++j) {
      const float a = arow[j];
      const float4 b = reinterpret_cast<const float4*>(L.b + (int64_t)j * L.N)[c4];
      acc.x = fmaf(a, b.x, acc.x); acc.y = fmaf(a, b.y, acc.y); acc.z = fmaf(a, b.z, acc.z); acc.w = fmaf(a, b.w, acc.w);
    }
    const float4 v = w0[i];
    float4 o;
    const float dx = L.s * acc.x, dy = L.s * acc.y, dz = L.s * acc.z, dw = L.s * acc.w;
    o.x = dx == 0.f ? v.x : v.x + dx;
    o.y = dy == 0.f ? v.y : v.y + dy;
    o.z = dz == 0.f ? v.z : v.z + dz;
    o.w = dw == 0.f ? v.w : v.w + dw;
    w[i] = o;
  }
}

extern "C" int ddpo_lora_merge(const ddpo_lora_layer* table_dev, int n_layers, int64_t max_kn, void* stream) {
  if (!table_dev || n_layers <= 0 || n_layers > 65535 || max_kn <= 0 || max_kn >= ((int64_t)1 << 33)) return DDPO_EINVAL;
  int64_t blocks = (max_kn / 4 + 255) / 256;
  if (blocks > 64) blocks = 64;                 // 64 x 128 layers = 8192 workgroups: every layer in flight at once, grid-stride for the rest
  hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)blocks, (unsigned)n_layers), dim3(256), 0, as_stream(stream), table_dev);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

// ------------------------------------------------------------------------------------------------ adapter gradient
// Per workgroup (256 threads), for each chunk of RM = 16 rows it owns (chunks g, g + G, g + 2G, ...), and for its 4-wide slice j0..j0+3 of the rank:
//  phase 1: v[m][j] = x[m, :] . A[:, j] and u[m][j] = dY[m, :] . B[j, :] — 16 threads per row, each a fixed k-stride, then a 16-lane butterfly;
//           A / B of the slice are staged in LDS once per workgroup.  This is the one HBM read of the chunk's x and dY.
//  phase 2: thread t owns the float4 column groups t, t + 256, ...: accA[k][j] += x[m, k] u[m][j], accB[n][j] += v[m][j] dY[m, n], m ascending —
//           a re-read of the rows the workgroup has just streamed (L2).
// At the end every workgroup writes its partial slab (K + N) x 4 floats; lora_reduce sums the G slabs in a fixed order and adds s * sum to dA / dB.
namespace {
constexpr int RM = 16;
constexpr int RJ = 4;
constexpr int NT = 256;

struct XSrc {
  const float* x;            // fp32 rows (row stride ldx), or NULL when the planes are given
  const uint16_t* hi;        // bf16 hi / lo planes: row-major with row stride ldp, or k-blocked (C / 32, rows, 32) when ldp == 0
  const uint16_t* lo;
  int ldx, ldp, rows;
};

__device__ __forceinline__ float bf(uint32_t h16) { return __uint_as_float(h16 << 16); }

template <bool PLANES>
__device__ __forceinline__ float4 load_x4(const XSrc& s, int m, int k) {
  if constexpr (!PLANES) {
    return *reinterpret_cast<const float4*>(s.x + (int64_t)m * s.ldx + k);
  } else {
    const int64_t off = s.ldp ? (int64_t)m * s.ldp + k : ((int64_t)(k >> 5) * s.rows + m) * 32 + (k & 31);
    const uint2 h = *reinterpret_cast<const uint2*>(s.hi + off);
    const uint2 l = *reinterpret_cast<const uint2*>(s.lo + off);
    return make_float4(bf(h.x & 0xFFFFu) + bf(l.x & 0xFFFFu), bf(h.x >> 16) + bf(l.x >> 16),
                       bf(h.y & 0xFFFFu) + bf(l.y & 0xFFFFu), bf(h.y >> 16) + bf(l.y >> 16));
  }
}

__device__ __forceinline__ float sum16(float v) {       // butterfly over the 16 lanes of a row group: ^8, ^4, ^2, ^1
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ void fma4(float4& acc, float a, const float4 b) {
  acc.x = fmaf(a, b.x, acc.x); acc.y = fmaf(a, b.y, acc.y); acc.z = fmaf(a, b.z, acc.z); acc.w = fmaf(a, b.w, acc.w);
}

// CPT: float4 column groups per thread in phase 2 (ceil(max(K, N) / 4 / 256)).
template <bool PLANES, int CPT>
__global__ void __launch_bounds__(NT) lora_wgrad_kernel(XSrc xs, const float* __restrict__ dy, int lddy, const float* __restrict__ A,
                                                        const float* __restrict__ B, int M, int K, int N, int r, int nj, float* __restrict__ slab) {
  extern __shared__ __align__(16) float lds[];
  float4* a_l = reinterpret_cast<float4*>(lds);          // [K]: A[k][j0 .. j0+3]
  float4* b_l = a_l + K;                                 // [N]: B[j0 .. j0+3][n]
  float4* v_l = b_l + N;                                 // [RM]
  float4* u_l = v_l + RM;                                // [RM]
  // workgroup -> (row group, rank slice): the nj slices of one row group sit 8 workgroup ids apart (the same dispatch lane group, which tends to
  // share an L2); only speed depends on this
  const int bid = blockIdx.x, G = gridDim.x / nj;
  const int jc = (bid >> 3) % nj;
  const int g = (bid & 7) + 8 * ((bid >> 3) / nj);
  const int j0 = jc * RJ;
  const int tid = threadIdx.x;
  for (int k = tid; k < K; k += NT) {
    float4 a;
    a.x = j0 + 0 < r ? A[(int64_t)k * r + j0 + 0] : 0.f;
    a.y = j0 + 1 < r ? A[(int64_t)k * r + j0 + 1] : 0.f;
    a.z = j0 + 2 < r ? A[(int64_t)k * r + j0 + 2] : 0.f;
    a.w = j0 + 3 < r ? A[(int64_t)k * r + j0 + 3] : 0.f;
    a_l[k] = a;
  }
  for (int n = tid; n < N; n += NT) {
    float4 b;
    b.x = j0 + 0 < r ? B[(int64_t)(j0 + 0) * N + n] : 0.f;
    b.y = j0 + 1 < r ? B[(int64_t)(j0 + 1) * N + n] : 0.f;
    b.z = j0 + 2 < r ? B[(int64_t)(j0 + 2) * N + n] : 0.f;
    b.w = j0 + 3 < r ? B[(int64_t)(j0 + 3) * N + n] : 0.f;
    b_l[n] = b;
  }
  float4 accA[CPT][4], accB[CPT][4];
#pragma unroll
  for (int c = 0; c < CPT; ++c)
#pragma unroll
    for (int q = 0; q < 4; ++q) accA[c][q] = accB[c][q] = make_float4(0.f, 0.f, 0.f, 0.f);
  const int K4 = K >> 2, N4 = N >> 2;
  const int sub = tid & 15, rr = tid >> 4;
  const int nchunks = (M + RM - 1) / RM;
  __syncthreads();
  for (int ch = g; ch < nchunks; ch += G) {
    const int m0 = ch * RM;
    // ---- phase 1
    {
      const int m = m0 + rr;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f), u = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m < M) {
        for (int c = sub; c < K4; c += 16) {
          const float4 x4 = load_x4<PLANES>(xs, m, 4 * c);
          fma4(v, x4.x, a_l[4 * c + 0]); fma4(v, x4.y, a_l[4 * c + 1]); fma4(v, x4.z, a_l[4 * c + 2]); fma4(v, x4.w, a_l[4 * c + 3]);
        }
        const float* drow = dy + (int64_t)m * lddy;
        for (int c = sub; c < N4; c += 16) {
          const float4 d4 = *reinterpret_cast<const float4*>(drow + 4 * c);
          fma4(u, d4.x, b_l[4 * c + 0]); fma4(u, d4.y, b_l[4 * c + 1]); fma4(u, d4.z, b_l[4 * c + 2]); fma4(u, d4.w, b_l[4 * c + 3]);
        }
      }
      v.x = sum16(v.x); v.y = sum16(v.y); v.z = sum16(v.z); v.w = sum16(v.w);
      u.x = sum16(u.x); u.y = sum16(u.y); u.z = sum16(u.z); u.w = sum16(u.w);
      if (sub == 0) { v_l[rr] = v; u_l[rr] = u; }
    }
    __syncthreads();
    // ---- phase 2
    const int mend = min(RM, M - m0);
    for (int mm = 0; mm < mend; ++mm) {
      const int m = m0 + mm;
      const float4 u = u_l[mm], v = v_l[mm];
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        const int col = tid + c * NT;
        if (col < K4) {
          const float4 x4 = load_x4<PLANES>(xs, m, 4 * col);
          fma4(accA[c][0], x4.x, u); fma4(accA[c][1], x4.y, u); fma4(accA[c][2], x4.z, u); fma4(accA[c][3], x4.w, u);
        }
        if (col < N4) {
          const float4 d4 = *reinterpret_cast<const float4*>(dy + (int64_t)m * lddy + 4 * col);
          fma4(accB[c][0], d4.x, v); fma4(accB[c][1], d4.y, v); fma4(accB[c][2], d4.z, v); fma4(accB[c][3], d4.w, v);
        }
      }
    }
    __syncthreads();
  }
  // ---- partial slab of this workgroup: [K][4] then [N][4] floats (k-th float4 = the 4 rank columns of row k of dA / column n of dB)
  float4* out = reinterpret_cast<float4*>(slab) + ((int64_t)g * nj + jc) * (K + N);
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    const int col = tid + c * NT;
    if (col < K4) {
#pragma unroll
      for (int q = 0; q < 4; ++q) out[4 * col + q] = accA[c][q];
    }
    if (col < N4) {
#pragma unroll
      for (int q = 0; q < 4; ++q) out[K + 4 * col + q] = accB[c][q];
    }
  }
}

// dA[k][j] += s * sum_g slab[g][j / 4].A[k][j % 4];  dB[j][n] += s * sum_g slab[g][j / 4].B[n][j % 4].  One wave per output: lane l sums the
// slabs g = l, l + 64, ... in ascending order, then the 64 lane sums meet in wave_sum's fixed butterfly — a fixed order, so bit-reproducible.
__global__ void __launch_bounds__(256) lora_reduce_kernel(const float* __restrict__ slab, int G, int nj, int K, int N, int r, float s,
                                                          float* __restrict__ dA, float* __restrict__ dB) {
  const int64_t total = (int64_t)(K + N) * r;
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t i = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < total; i += nwaves) {
    int64_t pos;                     // float offset inside one (g, slice) slab
    int jc;
    float* dst;
    if (i < (int64_t)K * r) {
      const int k = (int)(i / r), j = (int)(i - (int64_t)k * r);
      jc = j >> 2; pos = 4 * (int64_t)k + (j & 3); dst = dA + i;
    } else {
      const int64_t t = i - (int64_t)K * r;
      const int j = (int)(t / N), n = (int)(t - (int64_t)j * N);
      jc = j >> 2; pos = 4 * ((int64_t)K + n) + (j & 3); dst = dB + t;
    }
    float acc = 0.f;
    for (int g = lane; g < G; g += 64) acc += slab[((int64_t)g * nj + jc) * 4 * (K + N) + pos];
    acc = wave_sum(acc);
    if (lane == 0) *dst = *dst + s * acc;
  }
}

int wgrad_groups(int M, int nj) {
  const int nchunks = (M + RM - 1) / RM;
  int G = 512 / nj;                  // ~2 workgroups per CU over all rank slices
  if (G > nchunks) G = nchunks;
  if (G < 1) G = 1;
  G = (G + 7) / 8 * 8;               // whole groups of 8 (the workgroup -> row-group map above); surplus row groups own no chunk and write zeros
  return G;
}
}  // namespace

extern "C" size_t ddpo_lora_wgrad_ws_bytes(int M, int K, int N, int r) {
  if (M <= 0 || K <= 0 || N <= 0 || r <= 0) return 0;
  const int nj = (r + RJ - 1) / RJ;
  return (size_t)wgrad_groups(M, nj) * nj * (size_t)(K + N) * RJ * sizeof(float);
}

extern "C" int ddpo_lora_wgrad(const float* x, int ldx, const uint16_t* x_hi, const uint16_t* x_lo, int ld_planes, const float* dy, int lddy,
                               const float* A, const float* B, float* dA, float* dB, int M, int K, int N, int r, float s, void* ws,
                               size_t ws_bytes, void* stream) {
  const bool planes = x == nullptr;
  if (M <= 0 || K <= 0 || N <= 0 || r < 1 || r > 64 || (K & 3) || (N & 3) || K > 2048 || N > 2048 || K + N > 4064) return DDPO_EINVAL;
  if (!dy || !A || !B || !dA || !dB || !ws || lddy < N || (lddy & 3)) return DDPO_EINVAL;
  if (planes ? (!x_hi || !x_lo || ld_planes < 0 || (ld_planes && (ld_planes < K || (ld_planes & 3))) || (!ld_planes && (K & 31)))
             : (ldx < K || (ldx & 3) || (reinterpret_cast<uintptr_t>(x) & 15)))
    return DDPO_EINVAL;
  if ((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(ws)) & 15) return DDPO_EINVAL;
  if (planes && ((reinterpret_cast<uintptr_t>(x_hi) | reinterpret_cast<uintptr_t>(x_lo)) & 7)) return DDPO_EINVAL;
  if (ws_bytes < ddpo_lora_wgrad_ws_bytes(M, K, N, r)) return DDPO_EINVAL;
  const int nj = (r + RJ - 1) / RJ;
  const int G = wgrad_groups(M, nj);
  const int cols4 = ((K > N ? K : N) / 4 + NT - 1) / NT;
  XSrc xs{x, x_hi, x_lo, ldx, ld_planes, M};
  const size_t lds = (size_t)(K + N + 2 * RM) * sizeof(float4);
  const dim3 grid((unsigned)(G * nj)), block(NT);
  float* slab = static_cast<float*>(ws);
  hipStream_t st = as_stream(stream);
#define DDPO_LORA_WG(P, C) hipLaunchKernelGGL((lora_wgrad_kernel<P, C>), grid, block, lds, st, xs, dy, lddy, A, B, M, K, N, r, nj, slab)
  if (planes) {
    if (cols4 == 1) DDPO_LORA_WG(true, 1); else DDPO_LORA_WG(true, 2);
  } else {
    if (cols4 == 1) DDPO_LORA_WG(false, 1); else DDPO_LORA_WG(false, 2);
  }
#undef DDPO_LORA_WG
  DDPO_LAUNCH_CHECK();
  int64_t rb = ((int64_t)(K + N) * r + 3) / 4;         // 4 waves (outputs) per workgroup
  if (rb > 4096) rb = 4096;
  hipLaunchKernelGGL(lora_reduce_kernel, dim3((unsigned)rb), dim3(256), 0, st, slab, G, nj, K, N, r, s, dA, dB);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}
