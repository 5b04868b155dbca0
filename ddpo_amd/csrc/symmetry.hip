// Symmetry rewards on the device (mirror_device, mirror_corr_device, rotational_corr_device, rotational_device): decoder images in HBM -> four exact
// integer sums per image (ddpo_symmetry_stats), and the four right-angle turns of a square batch as bytes (ddpo_rotate4_u8).  The arithmetic is
// csrc/symmetry_core.h, shared with the serial host entries at the bottom.
//
// ddpo_symmetry_stats, two launches:
//   1. A workgroup takes a run of consecutive row units of one image.  A unit is one row (mirror: the partner of a byte lies in the same row) or
//      the row pair (y, H - 1 - y) (rotate 180: each row is the other's partner, the middle row of an odd H its own).  The rows of a unit are
//      staged into LDS as bytes, coalesced along W, every row read once — 16-byte loads for float32 input and 4-byte loads for uint8 input when W
//      is a multiple of 4 and the base is aligned to the load, one element per lane otherwise — and each lane adds its elements into 32-bit partials
//      (at most 2 * ceil(3 W / 256) <= 256 elements per unit, far below SY_U32_ELEMS), which go into 64-bit lane sums after every unit.  The lane
//      sums are reduced across the 64 lanes of a wave by shuffles, across the waves through LDS, and the workgroup's four sums are written to
//      its slot of `workspace`.
//   2. One wave per image adds the at most 64 slots of that image and writes stats_out.
// Nothing is zeroed and nothing is atomic: every slot that launch 2 reads was written by launch 1, and integer sums do not depend on their order.
//
// ddpo_rotate4_u8, one launch: a workgroup reads one 64 x 64 pixel tile of one image once (rows of 192 contiguous elements), keeps it in LDS as
// bytes, and writes it to its place in each of the four turns with consecutive lanes on consecutive bytes of an output row, whichever way the
// tile was turned.  LDS rows are padded by 4 bytes (49 dwords), so the column-wise reads of the quarter turns spread over the banks.
#include "common.h"
#include "symmetry_core.h"

namespace {

constexpr int SY_TB = 256;
constexpr int SY_WAVES = SY_TB / 64;
constexpr int SY_MAX_SLOTS = 64;                    // workgroups per image; launch 2 reduces them with one wave
constexpr int SY_TILE = 64;
constexpr int SY_TILE_STRIDE = SY_TILE * 3 + 4;

// units of one image and the workgroups they are spread over
inline int sy_units(int H, int mode) { return mode ? (H + 1) / 2 : H; }
inline int sy_slots(int H, int mode) { return sy_units(H, mode) < SY_MAX_SLOTS ? sy_units(H, mode) : SY_MAX_SLOTS; }

bool sy_stats_geometry_ok(int N, int H, int W, int mode) {
  if (N < 1 || H < 1 || W < 1 || W > SY_MAX_W || H > (1 << 24) || (mode != 0 && mode != 1)) return false;
  return (int64_t)N * sy_slots(H, mode) <= 0x7fffffff;
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
  return v;
}

struct SyStatsArgs {
  const void* images;
  int H, W, mode, units, slots;
  uint64_t* partial;                                // [N][slots][4]
};

template <bool F32, bool VEC>
__global__ __launch_bounds__(SY_TB) void symmetry_stats_kernel(const SyStatsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint64_t* red = reinterpret_cast<uint64_t*>(smem);                        // [SY_WAVES][4]
  uint8_t* s0 = reinterpret_cast<uint8_t*>(smem) + SY_WAVES * 4 * sizeof(uint64_t);
  uint8_t* s1 = s0 + iu_row_bytes(a.W);                                     // present when mode == 1
  const int t = threadIdx.x;
  const int n = blockIdx.x / a.slots, g = blockIdx.x - n * a.slots;
  const int per = (a.units + a.slots - 1) / a.slots;
  const int u0 = g * per, u1 = min(u0 + per, a.units);
  const int w3 = a.W * 3;
  uint64_t acc[4] = {0, 0, 0, 0};
  for (int y = u0; y < u1; ++y) {
    const int y2 = sy_partner_row(y, a.H, a.mode);
    const bool two = y2 != y;
    iu_stage<F32, VEC, SY_TB>(s0, 0, a.images, ((size_t)n * a.H + y) * w3, 0, 1, w3, t);
    if (two) iu_stage<F32, VEC, SY_TB>(s1, 0, a.images, ((size_t)n * a.H + y2) * w3, 0, 1, w3, t);
    __syncthreads();
    const uint8_t* sp = two ? s1 : s0;
    SyPartial p = {{0, 0, 0, 0}};
    for (int e = t; e < w3; e += SY_TB) {
      const int pe = sy_mirror_offset(e, a.W);
      sy_add(p, s0[e], sp[pe]);
      if (two) sy_add(p, s1[e], s0[pe]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] += p.s[k];
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) acc[k] = wave_sum_u64(acc[k]);
  if ((t & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) red[(t >> 6) * 4 + k] = acc[k];
  }
  __syncthreads();
  if (t < 4) {
    uint64_t v = 0;
    for (int w = 0; w < SY_WAVES; ++w) v += red[w * 4 + t];
    a.partial[((size_t)n * a.slots + g) * 4 + t] = v;
  }
}

__global__ __launch_bounds__(64) void symmetry_finish_kernel(const uint64_t* __restrict__ partial, int slots, int64_t* __restrict__ stats_out) {
  const int n = blockIdx.x, l = threadIdx.x;
  for (int k = 0; k < 4; ++k) {
    const uint64_t v = wave_sum_u64(l < slots ? partial[((size_t)n * slots + l) * 4 + k] : 0);
    if (l == 0) stats_out[(size_t)n * 4 + k] = (int64_t)v;
  }
}

template <bool F32, bool VEC>
__global__ __launch_bounds__(SY_TB) void rotate4_u8_kernel(const void* __restrict__ images, int N, int S, uint8_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[SY_TILE * SY_TILE_STRIDE];
  const int t = threadIdx.x;
  const int tiles = (S + SY_TILE - 1) / SY_TILE;
  const int n = blockIdx.x / (tiles * tiles), rem = blockIdx.x - n * tiles * tiles;
  const int ty0 = (rem / tiles) * SY_TILE, tx0 = (rem % tiles) * SY_TILE;
  const int th = min(SY_TILE, S - ty0), tw = min(SY_TILE, S - tx0);
  iu_stage<F32, VEC, SY_TB>(tile, SY_TILE_STRIDE, images, (((size_t)n * S + ty0) * S + tx0) * 3, (size_t)S * 3, th, tw * 3, t);
  __syncthreads();
  for (int k = 0; k < 4; ++k) {
    int ay, ax, by, bx;                                                     // where two opposite corners of the tile land: the output rectangle
    sy_rot_dst(k, S, ty0, tx0, ay, ax);
    sy_rot_dst(k, S, ty0 + th - 1, tx0 + tw - 1, by, bx);
    const int oy0 = min(ay, by), ox0 = min(ax, bx);
    const int rows = (k & 1) ? tw : th, c3 = ((k & 1) ? th : tw) * 3;
    uint8_t* o = out + (size_t)(k * N + n) * S * S * 3;
    for (int i = t; i < rows * c3; i += SY_TB) {
      const int r = i / c3, j = i - r * c3, q = j / 3, c = j - 3 * q;
      int iy, ix;
      sy_rot_src(k, S, oy0 + r, ox0 + q, iy, ix);
      o[((size_t)(oy0 + r) * S + ox0 + q) * 3 + c] = tile[(iy - ty0) * SY_TILE_STRIDE + (ix - tx0) * 3 + c];
    }
  }
}

bool sy_rotate_geometry_ok(int N, int S) {
  if (N < 1 || S < 1 || S > (1 << 15) || N > (1 << 24)) return false;
  const int64_t tiles = (S + SY_TILE - 1) / SY_TILE;
  return (int64_t)N * tiles * tiles <= 0x7fffffff;
}

}  // namespace

extern "C" int ddpo_symmetry_stats_workspace_bytes(int N, int H, int W, int mode, size_t* out_host) {
  if (!out_host || !sy_stats_geometry_ok(N, H, W, mode)) return DDPO_EINVAL;
  *out_host = (size_t)N * sy_slots(H, mode) * 4 * sizeof(uint64_t);
  return DDPO_OK;
}

extern "C" int ddpo_symmetry_stats(const void* images, int is_float32, int N, int H, int W, int mode, int64_t* stats_out, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  if (!images || !stats_out || !workspace || !sy_stats_geometry_ok(N, H, W, mode)) return DDPO_EINVAL;
  const int slots = sy_slots(H, mode);
  if (workspace_bytes < (size_t)N * slots * 4 * sizeof(uint64_t)) return DDPO_EINVAL;
  if ((reinterpret_cast<uintptr_t>(workspace) & 7) || (reinterpret_cast<uintptr_t>(stats_out) & 7) || iu_misaligned(images, is_float32))
    return DDPO_EINVAL;
  const SyStatsArgs a{images, H, W, mode, sy_units(H, mode), slots, static_cast<uint64_t*>(workspace)};
  const size_t lds = SY_WAVES * 4 * sizeof(uint64_t) + (mode ? 2 : 1) * iu_row_bytes(W);          // <= 128 + 2 * 32640 bytes: inside the 64 KB default
  hipStream_t s = as_stream(stream);
  iu_dispatch(is_float32, iu_vec_ok(images, is_float32, W), [&](auto F32, auto VEC) {
    hipLaunchKernelGGL((symmetry_stats_kernel<F32(), VEC()>), dim3((unsigned)(N * slots)), dim3(SY_TB), lds, s, a);
  });
  DDPO_LAUNCH_CHECK();
  hipLaunchKernelGGL(symmetry_finish_kernel, dim3((unsigned)N), dim3(64), 0, s, a.partial, slots, stats_out);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

extern "C" int ddpo_rotate4_u8(const void* images, int is_float32, int N, int H, int W, uint8_t* out, void* stream) {
  if (!images || !out || H != W || !sy_rotate_geometry_ok(N, H)) return DDPO_EINVAL;
  if (iu_misaligned(images, is_float32)) return DDPO_EINVAL;
  const int S = H, tiles = (S + SY_TILE - 1) / SY_TILE;
  iu_dispatch(is_float32, iu_vec_ok(images, is_float32, S), [&](auto F32, auto VEC) {
    hipLaunchKernelGGL((rotate4_u8_kernel<F32(), VEC()>), dim3((unsigned)(N * tiles * tiles)), dim3(SY_TB), 0, as_stream(stream), images, N, S, out);
  });
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

// Serial host paths over the same functions (no GPU involved): what the kernels are held to, and what is held to numpy and Pillow.
extern "C" int ddpo_symmetry_stats_host(const void* images, int is_float32, int N, int H, int W, int mode, int64_t* stats_out_host) {
  if (!images || !stats_out_host || !sy_stats_geometry_ok(N, H, W, mode)) return DDPO_EINVAL;
  const int w3 = W * 3;                                                     // <= 3 * SY_MAX_W < SY_U32_ELEMS: one row fits a 32-bit partial
  for (int n = 0; n < N; ++n) {
    uint64_t acc[4] = {0, 0, 0, 0};
    for (int y = 0; y < H; ++y) {
      const size_t row = ((size_t)n * H + y) * w3, prow = ((size_t)n * H + sy_partner_row(y, H, mode)) * w3;
      SyPartial p = {{0, 0, 0, 0}};
      for (int e = 0; e < w3; ++e) sy_add(p, iu_byte(images, is_float32, row + e), iu_byte(images, is_float32, prow + sy_mirror_offset(e, W)));
      for (int k = 0; k < 4; ++k) acc[k] += p.s[k];
    }
    for (int k = 0; k < 4; ++k) stats_out_host[(size_t)n * 4 + k] = (int64_t)acc[k];
  }
  return DDPO_OK;
}

extern "C" int ddpo_rotate4_u8_host(const void* images, int is_float32, int N, int H, int W, uint8_t* out_host) {
  if (!images || !out_host || H != W || !sy_rotate_geometry_ok(N, H)) return DDPO_EINVAL;
  const int S = H;
  for (int k = 0; k < 4; ++k)
    for (int n = 0; n < N; ++n)
      for (int oy = 0; oy < S; ++oy)
        for (int ox = 0; ox < S; ++ox) {
          int iy, ix;
          sy_rot_src(k, S, oy, ox, iy, ix);
          for (int c = 0; c < 3; ++c)
            out_host[((((size_t)k * N + n) * S + oy) * S + ox) * 3 + c] = (uint8_t)iu_byte(images, is_float32, (((size_t)n * S + iy) * S + ix) * 3 + c);
        }
  return DDPO_OK;
}
