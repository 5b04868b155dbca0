// Adapter gradients of WIDE LoRA layers (the GEGLU feed-forward layers; include/ddpo_lora_wide.h):
//   ddpo_lora_wgrad_wide  dA += s * x^T (dY B^T),  dB += s * (x A)^T dY for K, N up to 16384, x as fp32 rows or bf16 hi / lo planes
// ddpo_lora_wgrad (lora.hip) keeps the A / B slice of the whole layer in LDS and every column in registers; here the skinny products
// u = dY B^T, v = x A go through the workspace and the outer products run per column tile, so neither LDS nor registers grow with K, N.
// Bitwise reproducible like lora.hip: fixed summation orders, no float atomics (partial slabs per row group, a fixed-order reduction).
#include "common.h"
#include "../../include/ddpo_lora_wide.h"

extern "C" int ddpo_lora_wide_abi_version(void) { return 1; }

namespace {
constexpr int RM = 16;          // rows per workgroup of the u / v launch (16 lanes each)
constexpr int RJ = 4;           // rank slice
constexpr int NT = 256;
constexpr int TILE = 1024;      // columns per tile: one float4 group per thread in the outer-product launch, 16 KiB of LDS in the u / v launch
constexpr int MAX_DIM = 16384;
constexpr int MAX_GROUPS = 512;

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

__device__ __forceinline__ float sum16(float v) {       // butterfly over the 16 lanes of a row: ^8, ^4, ^2, ^1
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ void fma4(float4& acc, float a, const float4 b) {
  acc.x = fmaf(a, b.x, acc.x); acc.y = fmaf(a, b.y, acc.y); acc.z = fmaf(a, b.z, acc.z); acc.w = fmaf(a, b.w, acc.w);
}

// ------------------------------------------------------------------------------------------------ launch 1: u = dY B^T, v = x A
// blockIdx.x = chunk of RM rows, blockIdx.y = rank slice j0 .. j0+3.  Per column tile the slice of A (then of B) is staged in LDS; thread
// (row rr, lane sub) takes the float4 groups sub, sub + 16, ... of the tile, tiles ascending; the 16 lane sums meet in sum16.  uw / vw are
// (M, rp) with rp = 4 * gridDim.y: ranks past r hold zeros.
template <bool PLANES>
__global__ void __launch_bounds__(NT) lora_wide_uv_kernel(XSrc xs, const float* __restrict__ dy, int lddy, const float* __restrict__ A,
                                                          const float* __restrict__ B, int M, int K, int N, int r, float* __restrict__ uw,
                                                          float* __restrict__ vw) {
  __shared__ float4 t_l[TILE];
  const int tid = threadIdx.x, sub = tid & 15, rr = tid >> 4;
  const int j0 = blockIdx.y * RJ, rp = gridDim.y * RJ;
  const int m = blockIdx.x * RM + rr;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f), u = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int k0 = 0; k0 < K; k0 += TILE) {
    const int kt = min(TILE, K - k0);
    __syncthreads();
    for (int k = tid; k < kt; k += NT) {
      const float* arow = A + (int64_t)(k0 + k) * r;
      float4 a;
      a.x = j0 + 0 < r ? arow[j0 + 0] : 0.f;
      a.y = j0 + 1 < r ? arow[j0 + 1] : 0.f;
      a.z = j0 + 2 < r ? arow[j0 + 2] : 0.f;
      a.w = j0 + 3 < r ? arow[j0 + 3] : 0.f;
      t_l[k] = a;
    }
    __syncthreads();
    if (m < M) {
      for (int c = sub; c < (kt >> 2); c += 16) {
        const float4 x4 = load_x4<PLANES>(xs, m, k0 + 4 * c);
        fma4(v, x4.x, t_l[4 * c + 0]); fma4(v, x4.y, t_l[4 * c + 1]); fma4(v, x4.z, t_l[4 * c + 2]); fma4(v, x4.w, t_l[4 * c + 3]);
      }
    }
  }
  for (int n0 = 0; n0 < N; n0 += TILE) {
    const int nt = min(TILE, N - n0);
    __syncthreads();
    for (int n = tid; n < nt; n += NT) {
      float4 b;
      b.x = j0 + 0 < r ? B[(int64_t)(j0 + 0) * N + n0 + n] : 0.f;
      b.y = j0 + 1 < r ? B[(int64_t)(j0 + 1) * N + n0 + n] : 0.f;
      b.z = j0 + 2 < r ? B[(int64_t)(j0 + 2) * N + n0 + n] : 0.f;
      b.w = j0 + 3 < r ? B[(int64_t)(j0 + 3) * N + n0 + n] : 0.f;
      t_l[n] = b;
    }
    __syncthreads();
    if (m < M) {
      const float* drow = dy + (int64_t)m * lddy + n0;
      for (int c = sub; c < (nt >> 2); c += 16) {
        const float4 d4 = *reinterpret_cast<const float4*>(drow + 4 * c);
        fma4(u, d4.x, t_l[4 * c + 0]); fma4(u, d4.y, t_l[4 * c + 1]); fma4(u, d4.z, t_l[4 * c + 2]); fma4(u, d4.w, t_l[4 * c + 3]);
      }
    }
  }
  v.x = sum16(v.x); v.y = sum16(v.y); v.z = sum16(v.z); v.w = sum16(v.w);
  u.x = sum16(u.x); u.y = sum16(u.y); u.z = sum16(u.z); u.w = sum16(u.w);
  if (sub == 0 && m < M) {
    *reinterpret_cast<float4*>(vw + (int64_t)m * rp + j0) = v;
    *reinterpret_cast<float4*>(uw + (int64_t)m * rp + j0) = u;
  }
}

// ------------------------------------------------------------------------------------------------ launch 2: the outer products
// blockIdx.x = tile + nt * (rank slice + nj * row group), nt = ntk tiles of K then the tiles of N.  Thread t owns the 4 columns col0 + 4t ..
// of its tile and the 4 ranks of its slice: acc[q] += src[m, col + q] * coef[m, j0 .. j0+3] over the row group's rows [g * rows_per, ...),
// m ascending.  src / coef are x / u for a tile of K (dA) and dY / v for a tile of N (dB).  The workgroup then writes its columns of the
// row group's partial slab: [K][4] then [N][4] floats per (row group, rank slice), the layout lora.hip's slabs have.
template <bool PLANES>
__global__ void __launch_bounds__(NT) lora_wide_outer_kernel(XSrc xs, const float* __restrict__ dy, int lddy, const float* __restrict__ uw,
                                                             const float* __restrict__ vw, int M, int K, int N, int nj, int ntk, int nt,
                                                             int rows_per, float* __restrict__ slab) {
  const int bid = blockIdx.x;
  const int tile = bid % nt, jc = (bid / nt) % nj, g = bid / (nt * nj);
  const int rp = nj * RJ, j0 = jc * RJ;
  const bool is_a = tile < ntk;
  const int col = (is_a ? tile : tile - ntk) * TILE + 4 * (int)threadIdx.x;
  const bool active = col < (is_a ? K : N);
  const int m0 = g * rows_per, m1 = min(M, m0 + rows_per);
  float4 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (is_a) {
    const float* coef = uw + j0;
#pragma unroll 4
    for (int m = m0; m < m1; ++m) {
      const float4 w = *reinterpret_cast<const float4*>(coef + (int64_t)m * rp);
      if (active) {
        const float4 x4 = load_x4<PLANES>(xs, m, col);
        fma4(acc[0], x4.x, w); fma4(acc[1], x4.y, w); fma4(acc[2], x4.z, w); fma4(acc[3], x4.w, w);
      }
    }
  } else {
    const float* coef = vw + j0;
#pragma unroll 4
    for (int m = m0; m < m1; ++m) {
      const float4 w = *reinterpret_cast<const float4*>(coef + (int64_t)m * rp);
      if (active) {
        const float4 d4 = *reinterpret_cast<const float4*>(dy + (int64_t)m * lddy + col);
        fma4(acc[0], d4.x, w); fma4(acc[1], d4.y, w); fma4(acc[2], d4.z, w); fma4(acc[3], d4.w, w);
      }
    }
  }
  if (active) {
    float4* out = reinterpret_cast<float4*>(slab) + ((int64_t)g * nj + jc) * (K + N) + (is_a ? 0 : K) + col;
#pragma unroll
    for (int q = 0; q < 4; ++q) out[q] = acc[q];
  }
}

// ------------------------------------------------------------------------------------------------ launch 3: the fixed-order reduction
// dA[k][j] += s * sum_g slab[g][j / 4].A[k][j % 4];  dB[j][n] += s * sum_g slab[g][j / 4].B[n][j % 4].  One wave per output: lane l sums the
// slabs g = l, l + 64, ... in ascending order, then the 64 lane sums meet in wave_sum's fixed butterfly (lora.hip's reduction).
__global__ void __launch_bounds__(256) lora_wide_reduce_kernel(const float* __restrict__ slab, int G, int nj, int K, int N, int r, float s,
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

struct Plan {
  int nj, ntk, nt, G, rows_per;
  size_t uv_floats;          // floats of u (and of v): M * 4 nj
  size_t bytes;
};

bool shape_ok(int M, int K, int N, int r) {
  return M >= 1 && K >= 4 && N >= 4 && K <= MAX_DIM && N <= MAX_DIM && !(K & 3) && !(N & 3) && r >= 1 && r <= 64;
}

// Row groups: about 2048 workgroups over all tiles and rank slices, at least RM rows each, at most MAX_GROUPS slabs; no group is empty.
Plan make_plan(int M, int K, int N, int r) {
  Plan p;
  p.nj = (r + RJ - 1) / RJ;
  p.ntk = (K + TILE - 1) / TILE;
  p.nt = p.ntk + (N + TILE - 1) / TILE;
  int G = 2048 / (p.nj * p.nt);
  const int by_rows = (M + RM - 1) / RM;
  if (G > by_rows) G = by_rows;
  if (G > MAX_GROUPS) G = MAX_GROUPS;
  if (G < 1) G = 1;
  p.rows_per = (M + G - 1) / G;
  p.G = (M + p.rows_per - 1) / p.rows_per;
  p.uv_floats = (size_t)M * p.nj * RJ;
  p.bytes = (2 * p.uv_floats + (size_t)p.G * p.nj * (size_t)(K + N) * RJ) * sizeof(float);
  return p;
}
}  // namespace

extern "C" size_t ddpo_lora_wgrad_wide_ws_bytes(int M, int K, int N, int r) {
  if (!shape_ok(M, K, N, r)) return 0;
  return make_plan(M, K, N, r).bytes;
}

extern "C" int ddpo_lora_wgrad_wide(const float* x, int ldx, const uint16_t* x_hi, const uint16_t* x_lo, int ld_planes, const float* dy,
                                    int lddy, const float* A, const float* B, float* dA, float* dB, int M, int K, int N, int r, float s,
                                    void* ws, size_t ws_bytes, void* stream) {
  const bool planes = x == nullptr;
  if (!shape_ok(M, K, N, r)) return DDPO_EINVAL;
  if (!dy || !A || !B || !dA || !dB || !ws || lddy < N || (lddy & 3)) return DDPO_EINVAL;
  if (planes ? (!x_hi || !x_lo || ld_planes < 0 || (ld_planes && (ld_planes < K || (ld_planes & 3))) || (!ld_planes && (K & 31)))
             : (ldx < K || (ldx & 3) || (reinterpret_cast<uintptr_t>(x) & 15)))
    return DDPO_EINVAL;
  if ((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(ws)) & 15) return DDPO_EINVAL;
  if (planes && ((reinterpret_cast<uintptr_t>(x_hi) | reinterpret_cast<uintptr_t>(x_lo)) & 7)) return DDPO_EINVAL;
  const Plan p = make_plan(M, K, N, r);
  if (ws_bytes < p.bytes) return DDPO_EINVAL;
  XSrc xs{x, x_hi, x_lo, ldx, ld_planes, M};
  float* uw = static_cast<float*>(ws);
  float* vw = uw + p.uv_floats;
  float* slab = vw + p.uv_floats;
  hipStream_t st = as_stream(stream);
  const dim3 block(NT);
  const dim3 grid1((unsigned)((M + RM - 1) / RM), (unsigned)p.nj);
  const dim3 grid2((unsigned)(p.G * p.nj * p.nt));
  if (planes) {
    hipLaunchKernelGGL((lora_wide_uv_kernel<true>), grid1, block, 0, st, xs, dy, lddy, A, B, M, K, N, r, uw, vw);
    DDPO_LAUNCH_CHECK();
    hipLaunchKernelGGL((lora_wide_outer_kernel<true>), grid2, block, 0, st, xs, dy, lddy, uw, vw, M, K, N, p.nj, p.ntk, p.nt, p.rows_per, slab);
  } else {
    hipLaunchKernelGGL((lora_wide_uv_kernel<false>), grid1, block, 0, st, xs, dy, lddy, A, B, M, K, N, r, uw, vw);
    DDPO_LAUNCH_CHECK();
    hipLaunchKernelGGL((lora_wide_outer_kernel<false>), grid2, block, 0, st, xs, dy, lddy, uw, vw, M, K, N, p.nj, p.ntk, p.nt, p.rows_per, slab);
  }
  DDPO_LAUNCH_CHECK();
  int64_t rb = ((int64_t)(K + N) * r + 3) / 4;         // 4 waves (outputs) per workgroup
  if (rb > 4096) rb = 4096;
  hipLaunchKernelGGL(lora_wide_reduce_kernel, dim3((unsigned)rb), dim3(256), 0, st, slab, p.G, p.nj, K, N, r, s, dA, dB);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}
