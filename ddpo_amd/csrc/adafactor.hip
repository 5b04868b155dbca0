// Adafactor (optax 0.1.5, the reference's arguments) over the flat parameter / gradient buffers: five launches per update whatever the tensor
// count, driven by a device table of tensors and a host-built list of (tensor, tile) work items (include/ddpo_optim.h).
// Every reduction is a fixed-order sum of partials parked in the workspace, so the update is bit-identical from run to run.
#include "common.h"
#include "../../include/ddpo_optim.h"
#include <vector>

namespace {

constexpr int TR = DDPO_ADAFACTOR_TILE_ROWS;   // rows of a factored matrix per work item: 4 waves x 32 rows
constexpr int RW = TR / 4;                     // rows per wave
constexpr int TC = 256;                        // columns per pass of the block over its rows: 64 lanes x 4
constexpr int CHUNK = DDPO_ADAFACTOR_CHUNK;    // elements of an unfactored tensor per work item: 256 threads x 16

struct AfArgs {
  float inv_n, max_norm, beta, omb, eps, lr, thr, min_scale, wd;
  int zero_grad;
};

// g * inv_n, then optax clip_by_global_norm — the arithmetic of adam_one (elementwise.hip)
struct Clip {
  float inv_n, norm, max_norm;
  bool clip;
  __device__ __forceinline__ Clip(const double* sqn, const AfArgs& a) : inv_n(a.inv_n), max_norm(a.max_norm) {
    norm = (float)sqrt(*sqn) * a.inv_n;
    clip = !(norm < a.max_norm);
  }
  __device__ __forceinline__ float operator()(float g) const {
    float ge = g * inv_n;
    if (clip) ge = (ge / norm) * max_norm;
    return ge;
  }
};

__host__ __device__ __forceinline__ int row_tiles(int R) { return (R + TR - 1) / TR; }
__host__ __device__ __forceinline__ int64_t header_floats(int n_tensors, int64_t n_tiles) {
  return 4 * n_tiles + ((2 * (int64_t)n_tensors + 3) & ~(int64_t)3);      // 2 doubles per tile, 2 floats per tensor
}
// a factored tensor's region: per-row-tile column sums (S*ntr*C) | column factors (S*C) | row sums (S*R) | row factors (S*R); the two
// column arrays come first so that they are 16-byte aligned whenever C % 4 == 0 (the float4 path reads the column factors)
__host__ __device__ __forceinline__ int64_t region_floats(int64_t S, int64_t R, int64_t C) {
  return (S * (2 * R + C * (row_tiles((int)R) + 1)) + 3) & ~(int64_t)3;
}
struct Region {
  float *rowsum, *colpart, *fr, *fc;
  __device__ __forceinline__ Region(float* ws, int n_tensors, int n_tiles, const ddpo_adafactor_tensor& t) {
    colpart = ws + header_floats(n_tensors, n_tiles) + t.ws_off;
    fc = colpart + (int64_t)t.S * row_tiles(t.R) * t.C;
    rowsum = fc + (int64_t)t.S * t.C;
    fr = rowsum + (int64_t)t.S * t.R;
  }
};

// The 4 values a lane holds of one row within the 256 columns from c0.  VEC (C % 4 == 0 and a 16-byte aligned tensor): columns
// c0 + 4 lane + j as one float4; otherwise columns c0 + lane + 64 j, four coalesced scalar accesses.
template <bool VEC> __device__ __forceinline__ int col_of(int c0, int lane, int j) { return VEC ? c0 + 4 * lane + j : c0 + lane + 64 * j; }
template <bool VEC> __device__ __forceinline__ int slot_of(int lane, int j) { return VEC ? 4 * lane + j : lane + 64 * j; }

template <bool VEC> __device__ __forceinline__ void load4(const float* __restrict__ row, int c0, int lane, int C, float (&x)[4]) {
  if (VEC) {
    const int c = c0 + 4 * lane;
    if (c < C) {
      const float4 v = *reinterpret_cast<const float4*>(row + c);
      x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
      x[0] = x[1] = x[2] = x[3] = 0.f;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + lane + 64 * j;
      x[j] = c < C ? row[c] : 0.f;
    }
  }
}
__device__ __forceinline__ void store4(float* __restrict__ row, int c0, int lane, int C, const float (&x)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = c0 + lane + 64 * j;
    if (c < C) row[c] = x[j];
  }
}

// fixed-order block sum of a double over 256 threads: butterfly per wave, then wave 0 + 1 + 2 + 3; valid in every thread
__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// ---------------------------------------------------------------------------------------------- (1) statistics
// A wave owns rows r0 + w, r0 + w + 4, ... of the tile and walks them 256 columns at a time, 8 rows in flight.  Column sums: 4 accumulators
// per lane over the wave's rows, then wave 0 + 1 + 2 + 3 through LDS.  Row sums: each lane keeps its own partial per row in LDS across the
// column passes (a register per row would pin 32 accumulators plus every load in flight: 141 VGPRs, 3 waves per SIMD), butterfly at the end.
constexpr int RB = 8;
template <bool VEC>
__device__ __forceinline__ void stats_factored(const float* __restrict__ g, const ddpo_adafactor_tensor& t, int tile, const Region& rg,
                                               const Clip& clip, float eps, float (*cs)[TC], float (*rowp)[RW][64]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int ntr = row_tiles(t.R), slab = tile / ntr, rt = tile - slab * ntr, r0 = rt * TR, C = t.C, R = t.R;
  const float* base = g + t.off + ((int64_t)slab * R + r0 + w) * C;
  const int rows = min(TR, R - r0), nrow = rows > w ? (rows - w + 3) >> 2 : 0;       // rows of this wave
  for (int i = 0; i < nrow; ++i) rowp[w][i][lane] = 0.f;
  for (int c0 = 0; c0 < C; c0 += TC) {
    float colacc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i0 = 0; i0 < nrow; i0 += RB) {
      float x[RB][4];
#pragma unroll
      for (int ii = 0; ii < RB; ++ii)
        if (i0 + ii < nrow) load4<VEC>(base + (int64_t)(4 * (i0 + ii)) * C, c0, lane, C, x[ii]);
#pragma unroll
      for (int ii = 0; ii < RB; ++ii) {
        if (i0 + ii < nrow) {
          float q[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float ge = clip(x[ii][j]);
            q[j] = col_of<VEC>(c0, lane, j) < C ? ge * ge + eps : 0.f;
            colacc[j] += q[j];
          }
          rowp[w][i0 + ii][lane] += (q[0] + q[1]) + (q[2] + q[3]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) cs[w][slot_of<VEC>(lane, j)] = colacc[j];
    __syncthreads();
    const int c = c0 + (int)threadIdx.x;
    if (c < C) rg.colpart[((int64_t)slab * ntr + rt) * C + c] = ((cs[0][threadIdx.x] + cs[1][threadIdx.x]) + cs[2][threadIdx.x]) + cs[3][threadIdx.x];
    __syncthreads();
  }
  for (int i = 0; i < nrow; ++i) {
    const float s = wave_sum(rowp[w][i][lane]);
    if (lane == 0) rg.rowsum[(int64_t)slab * R + r0 + w + 4 * i] = s;
  }
}

__global__ void __launch_bounds__(256) adafactor_stats_kernel(const float* __restrict__ g, float* __restrict__ state,
                                                              const ddpo_adafactor_tensor* __restrict__ tensors, int n_tensors,
                                                              const int32_t* __restrict__ work, int n_tiles,
                                                              const double* __restrict__ sqn, float* __restrict__ ws, AfArgs a) {
  __shared__ float cs[4][TC];
  __shared__ float rowp[4][RW][64];
  const ddpo_adafactor_tensor t = tensors[work[2 * blockIdx.x]];
  const int tile = work[2 * blockIdx.x + 1];
  const Clip clip(sqn, a);
  if (t.factored) {
    const Region rg(ws, n_tensors, n_tiles, t);
    if (((t.C | (int)t.off) & 3) == 0) stats_factored<true>(g, t, tile, rg, clip, a.eps, cs, rowp);
    else stats_factored<false>(g, t, tile, rg, clip, a.eps, cs, rowp);
    return;
  }
  const int64_t i0 = (int64_t)tile * CHUNK;
#pragma unroll 4
  for (int k = 0; k < CHUNK / 256; ++k) {
    const int64_t i = i0 + threadIdx.x + 256 * k;
    if (i < t.numel) {
      const float ge = clip(g[t.off + i]);
      state[t.v_off + i] = a.beta * state[t.v_off + i] + a.omb * (ge * ge + a.eps);
    }
  }
}

// ---------------------------------------------------------------------------------------------- (2) v_row, v_col, factors
__global__ void __launch_bounds__(256) adafactor_factors_kernel(float* __restrict__ state, const ddpo_adafactor_tensor* __restrict__ tensors,
                                                                int n_tensors, const int32_t* __restrict__ work, int n_tiles,
                                                                float* __restrict__ ws, AfArgs a) {
  __shared__ double red[4];
  const int32_t* sl = work + 2 * (int64_t)n_tiles + 2 * blockIdx.x;
  const ddpo_adafactor_tensor t = tensors[sl[0]];
  const int slab = sl[1], R = t.R, C = t.C, ntr = row_tiles(R);
  const Region rg(ws, n_tensors, n_tiles, t);
  float* vr = state + t.v_off + (int64_t)slab * R;
  float* vc = state + t.vc_off + (int64_t)slab * C;
  double acc = 0.0;
  for (int r = threadIdx.x; r < R; r += 256) {
    const float v = a.beta * vr[r] + a.omb * (rg.rowsum[(int64_t)slab * R + r] / (float)C);
    vr[r] = v;
    if (t.norm_rows) acc += (double)v;
  }
  for (int c = threadIdx.x; c < C; c += 256) {
    double s = 0.0;
    for (int k = 0; k < ntr; ++k) s += (double)rg.colpart[((int64_t)slab * ntr + k) * C + c];
    const float v = a.beta * vc[c] + a.omb * ((float)s / (float)R);
    vc[c] = v;
    if (!t.norm_rows) acc += (double)v;
  }
  const float m = (float)(block_sum_d(acc, red) / (double)(t.norm_rows ? R : C));
  // each thread re-reads only what it wrote itself
  for (int r = threadIdx.x; r < R; r += 256) rg.fr[(int64_t)slab * R + r] = 1.0f / sqrtf(t.norm_rows ? vr[r] / m : vr[r]);
  for (int c = threadIdx.x; c < C; c += 256) rg.fc[(int64_t)slab * C + c] = 1.0f / sqrtf(t.norm_rows ? vc[c] : vc[c] / m);
}

// ---------------------------------------------------------------------------------------------- (3) sums and (5) apply
struct Coef { float denom, scale; };

template <bool APPLY> __device__ __forceinline__ void one(float& p, float u, const Coef& k, const AfArgs& a, double& su, double& sp) {
  if (APPLY) {
    u = u / k.denom;
    u = a.lr * u;
    u = u * k.scale;
    u = u + a.wd * p;
    p = p - u;
  } else {
    su += (double)(u * u);
    sp += (double)(p * p);
  }
}

// optax: grad * row_factor * col_factor, "row" being the statistics of the reduced LARGEST axis
__device__ __forceinline__ float scaled(float ge, float frv, float fcv, int norm_rows) { return norm_rows ? (ge * frv) * fcv : (ge * fcv) * frv; }

// C % 4 == 0: the rows of a tile are one contiguous range, walked as float4 groups by the whole block, 4 groups per thread in flight; a
// group's row and column follow incrementally from the thread's first (one integer division per thread).
template <bool APPLY>
__device__ __forceinline__ void walk_flat(float* __restrict__ p, float* __restrict__ g, const ddpo_adafactor_tensor& t, int tile,
                                          const Region& rg, const Clip& clip, const Coef& k, const AfArgs& a, double& su, double& sp) {
  constexpr int U = 4;
  const int ntr = row_tiles(t.R), slab = tile / ntr, rt = tile - slab * ntr, r0 = rt * TR, C4 = t.C >> 2, R = t.R;
  const int n4 = min(TR, R - r0) * C4;
  const int64_t base = t.off + ((int64_t)slab * R + r0) * t.C;
  float4* p4 = reinterpret_cast<float4*>(p + base);
  float4* g4 = reinterpret_cast<float4*>(g + base);
  const float* fr = rg.fr + (int64_t)slab * R + r0;
  const float4* fc4 = reinterpret_cast<const float4*>(rg.fc + (int64_t)slab * t.C);
  const int dq = 256 / C4, dr = 256 - dq * C4;
  int r = (int)threadIdx.x / C4, c4 = (int)threadIdx.x - r * C4;
  for (int q0 = threadIdx.x; q0 < n4; q0 += 256 * U) {
    float4 gv[U], pv[U], fcv[U];
    float frv[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      if (q0 + 256 * j < n4) {
        gv[j] = g4[q0 + 256 * j];
        pv[j] = p4[q0 + 256 * j];
        frv[j] = fr[r];
        fcv[j] = fc4[c4];
      }
      r += dq;
      c4 += dr;
      if (c4 >= C4) { c4 -= C4; ++r; }
    }
#pragma unroll
    for (int j = 0; j < U; ++j) {
      if (q0 + 256 * j < n4) {
        one<APPLY>(pv[j].x, scaled(clip(gv[j].x), frv[j], fcv[j].x, t.norm_rows), k, a, su, sp);
        one<APPLY>(pv[j].y, scaled(clip(gv[j].y), frv[j], fcv[j].y, t.norm_rows), k, a, su, sp);
        one<APPLY>(pv[j].z, scaled(clip(gv[j].z), frv[j], fcv[j].z, t.norm_rows), k, a, su, sp);
        one<APPLY>(pv[j].w, scaled(clip(gv[j].w), frv[j], fcv[j].w, t.norm_rows), k, a, su, sp);
        if (APPLY) {
          p4[q0 + 256 * j] = pv[j];
          if (a.zero_grad) g4[q0 + 256 * j] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
    }
  }
}

// any C: a wave per row, 256 columns at a time, four coalesced scalar accesses per lane
template <bool APPLY>
__device__ __forceinline__ void walk_rows(float* __restrict__ p, float* __restrict__ g, const ddpo_adafactor_tensor& t, int tile,
                                          const Region& rg, const Clip& clip, const Coef& k, const AfArgs& a, double& su, double& sp) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int ntr = row_tiles(t.R), slab = tile / ntr, rt = tile - slab * ntr, r0 = rt * TR, C = t.C, R = t.R;
  const int64_t base = t.off + (int64_t)slab * R * C;
  const float* fr = rg.fr + (int64_t)slab * R;
  const float* fc = rg.fc + (int64_t)slab * C;
  for (int c0 = 0; c0 < C; c0 += TC) {
    float fcv[4];
    load4<false>(fc, c0, lane, C, fcv);
    for (int r = r0 + w; r < min(R, r0 + TR); r += 4) {
      const float frv = fr[r];
      float gx[4], px[4];
      load4<false>(g + base + (int64_t)r * C, c0, lane, C, gx);
      load4<false>(p + base + (int64_t)r * C, c0, lane, C, px);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        one<APPLY>(px[j], scaled(clip(gx[j]), frv, fcv[j], t.norm_rows), k, a, su, sp);       // columns past C hold g = p = 0: they add nothing
        gx[j] = 0.f;
      }
      if (APPLY) {
        store4(p + base + (int64_t)r * C, c0, lane, C, px);
        if (a.zero_grad) store4(g + base + (int64_t)r * C, c0, lane, C, gx);
      }
    }
  }
}

template <bool APPLY>
__global__ void __launch_bounds__(256) adafactor_walk_kernel(float* __restrict__ p, float* __restrict__ g, const float* __restrict__ state,
                                                             const ddpo_adafactor_tensor* __restrict__ tensors, int n_tensors,
                                                             const int32_t* __restrict__ work, int n_tiles,
                                                             const double* __restrict__ sqn, float* __restrict__ ws, AfArgs a) {
  __shared__ double red[4];
  const int ti = work[2 * blockIdx.x];
  const ddpo_adafactor_tensor t = tensors[ti];
  const int tile = work[2 * blockIdx.x + 1];
  const Clip clip(sqn, a);
  double* tilepart = reinterpret_cast<double*>(ws);
  const float* tcoef = ws + 4 * (int64_t)n_tiles;
  Coef k = {1.f, 1.f};
  if (APPLY) { k.denom = tcoef[2 * ti]; k.scale = tcoef[2 * ti + 1]; }
  double su = 0.0, sp = 0.0;
  if (t.factored) {
    const Region rg(ws, n_tensors, n_tiles, t);
    if (((t.C | (int)t.off) & 3) == 0) walk_flat<APPLY>(p, g, t, tile, rg, clip, k, a, su, sp);
    else walk_rows<APPLY>(p, g, t, tile, rg, clip, k, a, su, sp);
  } else {
    const int64_t i0 = (int64_t)tile * CHUNK;
#pragma unroll 4
    for (int j = 0; j < CHUNK / 256; ++j) {
      const int64_t i = i0 + threadIdx.x + 256 * j;
      if (i < t.numel) {
        const float ge = clip(g[t.off + i]);
        const float u = ge * (1.0f / sqrtf(state[t.v_off + i]));
        float pv = p[t.off + i];
        one<APPLY>(pv, u, k, a, su, sp);
        if (APPLY) {
          p[t.off + i] = pv;
          if (a.zero_grad) g[t.off + i] = 0.f;
        }
      }
    }
  }
  if (!APPLY) {
    su = block_sum_d(su, red);
    sp = block_sum_d(sp, red);
    if (threadIdx.x == 0) {
      tilepart[2 * ((int64_t)t.first_tile + tile)] = su;          // by tile, not by block: the work list may come in any order
      tilepart[2 * ((int64_t)t.first_tile + tile) + 1] = sp;
    }
  }
}

// ---------------------------------------------------------------------------------------------- (4) per-tensor clip and scale
__global__ void __launch_bounds__(256) adafactor_coef_kernel(const ddpo_adafactor_tensor* __restrict__ tensors, int n_tiles,
                                                             float* __restrict__ ws, AfArgs a) {
  __shared__ double red[4];
  const ddpo_adafactor_tensor t = tensors[blockIdx.x];
  const double* tilepart = reinterpret_cast<const double*>(ws);
  float* tcoef = ws + 4 * (int64_t)n_tiles;
  double su = 0.0, sp = 0.0;
  for (int k = threadIdx.x; k < t.n_tiles; k += 256) {
    su += tilepart[2 * ((int64_t)t.first_tile + k)];
    sp += tilepart[2 * ((int64_t)t.first_tile + k) + 1];
  }
  su = block_sum_d(su, red);
  sp = block_sum_d(sp, red);
  if (threadIdx.x == 0) {
    const float rms_u = sqrtf((float)(su / (double)t.numel)), rms_p = sqrtf((float)(sp / (double)t.numel));
    tcoef[2 * blockIdx.x] = fmaxf(1.0f, rms_u / a.thr);
    tcoef[2 * blockIdx.x + 1] = fmaxf(rms_p, a.min_scale);
  }
}

}  // namespace

extern "C" int ddpo_optim_abi_version(void) { return 1; }
extern "C" size_t ddpo_sizeof_adafactor_tensor(void) { return sizeof(ddpo_adafactor_tensor); }

extern "C" size_t ddpo_adafactor_workspace_bytes(const ddpo_adafactor_tensor* ts, int n_tensors, const int32_t* work, int n_tiles, int n_slabs,
                                                 int64_t n, int64_t n_state) {
  if (!ts || !work || n_tensors <= 0 || n_tiles <= 0 || n_slabs < 0 || n <= 0 || n_state <= 0) return 0;
  int64_t tile = 0, slab = 0, ws_end = 0;
  std::vector<char> seen((size_t)n_tiles, 0);
  for (int64_t k = 0; k < n_tiles; ++k)
    if (work[2 * k] < 0 || work[2 * k] >= n_tensors) return 0;
  for (int i = 0; i < n_tensors; ++i) {
    const ddpo_adafactor_tensor& t = ts[i];
    if (t.S <= 0 || t.R <= 0 || t.C <= 0 || t.numel != (int64_t)t.S * t.R * t.C || t.reserved) return 0;
    if (t.off < 0 || t.off > n - t.numel) return 0;
    int64_t tiles;
    if (t.factored == 1) {
      if (t.norm_rows != (t.C >= t.R ? 1 : 0)) return 0;
      const int64_t nr = (int64_t)t.S * t.R, nc = (int64_t)t.S * t.C;
      if (t.v_off < 0 || t.v_off > n_state - nr || t.vc_off < 0 || t.vc_off > n_state - nc) return 0;
      if (t.ws_off != ws_end) return 0;                       // regions packed in table order: no overlap, no gap
      ws_end += region_floats(t.S, t.R, t.C);
      tiles = (int64_t)t.S * row_tiles(t.R);
      for (int s = 0; s < t.S; ++s, ++slab) {
        if (slab >= n_slabs) return 0;
        const int32_t* e = work + 2 * ((int64_t)n_tiles + slab);
        if (e[0] != i || e[1] != s) return 0;
      }
    } else if (t.factored == 0) {
      if (t.S != 1 || t.R != 1 || t.norm_rows) return 0;
      if (t.v_off < 0 || t.v_off > n_state - t.numel) return 0;
      tiles = (t.numel + CHUNK - 1) / CHUNK;
    } else {
      return 0;
    }
    if (t.first_tile != tile || t.n_tiles != tiles || tile + tiles > n_tiles) return 0;
    tile += tiles;
  }
  if (tile != n_tiles || slab != n_slabs) return 0;
  for (int64_t k = 0; k < n_tiles; ++k) {                      // every (tensor, tile) exactly once, in any order
    const ddpo_adafactor_tensor& t = ts[work[2 * k]];
    const int32_t j = work[2 * k + 1];
    if (j < 0 || j >= t.n_tiles || seen[(size_t)t.first_tile + j]) return 0;
    seen[(size_t)t.first_tile + j] = 1;
  }
  return (size_t)(header_floats(n_tensors, n_tiles) + ws_end) * sizeof(float);
}

extern "C" int ddpo_adafactor_step(float* p, float* g, float* state, const ddpo_adafactor_tensor* tensors, int n_tensors, const int32_t* work,
                                   int n_tiles, int n_slabs, int64_t n, const double* sqnorm_of_sum, double inv_n_acc, double lr,
                                   double beta_t, double eps, double clipping_threshold, double min_scale, double weight_decay,
                                   double max_grad_norm, int zero_grad, void* workspace, size_t workspace_bytes, void* stream) {
  if (!p || !g || !state || !tensors || !work || !sqnorm_of_sum || !workspace) return DDPO_EINVAL;
  if (n_tensors <= 0 || n_tiles <= 0 || n_slabs < 0 || n <= 0) return DDPO_EINVAL;
  if ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(state) |
       reinterpret_cast<uintptr_t>(workspace)) & 15) return DDPO_EINVAL;
  if (workspace_bytes < (size_t)header_floats(n_tensors, n_tiles) * sizeof(float)) return DDPO_EINVAL;
  if (!(beta_t >= 0.0 && beta_t < 1.0) || !(clipping_threshold > 0.0) || !(eps > 0.0) || !(inv_n_acc > 0.0)) return DDPO_EINVAL;
  AfArgs a;
  a.inv_n = (float)inv_n_acc;
  a.max_norm = (float)max_grad_norm;
  a.beta = (float)beta_t;
  a.omb = 1.0f - a.beta;
  a.eps = (float)eps;
  a.lr = (float)lr;
  a.thr = (float)clipping_threshold;
  a.min_scale = (float)min_scale;
  a.wd = (float)weight_decay;
  a.zero_grad = zero_grad;
  float* ws = static_cast<float*>(workspace);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(adafactor_stats_kernel, dim3(n_tiles), dim3(256), 0, st, g, state, tensors, n_tensors, work, n_tiles, sqnorm_of_sum, ws, a);
  DDPO_LAUNCH_CHECK();
  if (n_slabs > 0) {
    hipLaunchKernelGGL(adafactor_factors_kernel, dim3(n_slabs), dim3(256), 0, st, state, tensors, n_tensors, work, n_tiles, ws, a);
    DDPO_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(adafactor_walk_kernel<false>, dim3(n_tiles), dim3(256), 0, st, p, g, state, tensors, n_tensors, work, n_tiles,
                     sqnorm_of_sum, ws, a);
  DDPO_LAUNCH_CHECK();
  hipLaunchKernelGGL(adafactor_coef_kernel, dim3(n_tensors), dim3(256), 0, st, tensors, n_tiles, ws, a);
  DDPO_LAUNCH_CHECK();
  hipLaunchKernelGGL(adafactor_walk_kernel<true>, dim3(n_tiles), dim3(256), 0, st, p, g, state, tensors, n_tensors, work, n_tiles,
                     sqnorm_of_sum, ws, a);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}
