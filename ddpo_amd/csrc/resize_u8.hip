// 8-bit bicubic resize on the device (the thumbnail_device reward): an N x H x W x 3 batch in HBM -> N x oh x ow x 3 BYTES, what Pillow's
// Image.resize(BICUBIC) returns for an RGB image, in ONE launch.  Byte conversion by truncation, horizontal pass rounded to a byte, vertical
// pass.  The arithmetic is csrc/clip_preprocess_core.h, shared with csrc/clip_preprocess.hip and with the serial host entry at the bottom; the
// coefficient tables are the caller's (lib.clip_preprocess_tables), nothing here is computed in double precision.
//
// One workgroup per (image, band of `band` output rows):
//   1. the input rows the band needs (from the vertical bound table) are staged CP_STAGE_ROWS at a time into LDS as bytes — 16-byte loads,
//      coalesced along W — and resampled horizontally into `rows` x ow x 3 bytes of LDS;
//   2. the vertical pass runs out of LDS.  The band's output rows are one contiguous run of bytes: the bytes up to the first 4-byte boundary and
//      after the last leave as byte stores, everything between as packed 4-byte stores.
// No workspace, no atomics, no state outside the arguments: calls on different streams may overlap.  Neighbouring bands re-read the input
// rows their kernels share (the support of the vertical filter, 4 x scale rows a band); nothing else is read twice from HBM.
#include "common.h"
#include "clip_preprocess_core.h"
#include <algorithm>
#include <vector>

namespace {

constexpr int RU_TB = 512;

struct RuArgs {
  const void* images;
  int N, H, W, oh, ow;
  const int32_t *hcoef, *hbounds;
  int hk;
  const int32_t *vcoef, *vbounds;
  int vk, band, rows;
  uint8_t* out;
};

__host__ __device__ inline int ru_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Bytes of LDS one workgroup uses: `rows` horizontally resampled rows of ow x 3 bytes + CP_STAGE_ROWS input rows of W x 3 bytes (each rounded up
// to 16).  The supported domain is "this fits CP_LDS_LIMIT" for the device and the host entry alike.
inline size_t ru_lds_bytes(int rows, int ow, int W) { return (size_t)rows * cp_row_bytes(ow) + (size_t)CP_STAGE_ROWS * cp_row_bytes(W); }

// Everything the device and the host entry refuse alike (pointers and the LDS rule are checked by the callers)
bool ru_geometry_ok(const RuArgs& a) {
  if (a.N < 1 || a.H < 1 || a.W < 1 || a.oh < 1 || a.ow < 1 || a.hk < 1 || a.vk < 1 || a.band < 1) return false;
  if (a.oh > (1 << 15) || a.ow > (1 << 15) || a.H > (1 << 24) || a.W > (1 << 24)) return false;
  if ((int64_t)a.band * a.ow * 3 > (1 << 30)) return false;                 // a band's bytes are indexed with an int
  if ((int64_t)a.N * ((a.oh + a.band - 1) / a.band) > 0x7fffffff) return false;
  return true;
}

template <bool F32, bool VEC>
__global__ __launch_bounds__(RU_TB) void resize_u8_kernel(const RuArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x;
  const int nb = (a.oh + a.band - 1) / a.band;
  const int n = blockIdx.x / nb, Y0 = (blockIdx.x % nb) * a.band;
  const int nout = min(a.band, a.oh - Y0);                                  // output rows of this band
  const int hrow = (int)cp_row_bytes(a.ow), srow = (int)cp_row_bytes(a.W);
  uint8_t* s_h = reinterpret_cast<uint8_t*>(smem);                          // [rows][hrow]: horizontally resampled bytes
  uint8_t* s_in = s_h + (size_t)a.rows * hrow;                              // [CP_STAGE_ROWS][srow]: input rows as bytes

  // input rows [y_lo, y_lo + nrows) feed the output rows Y0 .. Y0 + nout - 1 (the first bound of a table never decreases).  Bounds are clamped
  // to the image and to the LDS the launch was given, so a bad table cannot make the kernel read or write outside its arguments.
  int y_lo = a.vbounds[2 * Y0], y_hi = y_lo;
  for (int r = 0; r < nout; ++r) y_hi = max(y_hi, a.vbounds[2 * (Y0 + r)] + a.vbounds[2 * (Y0 + r) + 1]);
  y_lo = ru_clampi(y_lo, 0, a.H);
  const int nrows = ru_clampi(min(y_hi, a.H) - y_lo, 0, a.rows);
  const int o3 = a.ow * 3, w3 = a.W * 3;

  for (int r0 = 0; r0 < nrows; r0 += CP_STAGE_ROWS) {
    const int nr = min(CP_STAGE_ROWS, nrows - r0);
    const size_t row0 = ((size_t)n * a.H + (size_t)(y_lo + r0)) * w3;      // element index of the first staged row
    cp_stage_rows<F32, VEC, RU_TB>(a.images, row0, nr, w3, s_in, srow, t);
    __syncthreads();
    for (int i = t; i < nr * o3; i += RU_TB) {
      const int r = i / o3, rem = i - r * o3, X = rem / 3, c = rem - X * 3;
      const int xmin = ru_clampi(a.hbounds[2 * X], 0, a.W);
      const int cnt = ru_clampi(a.hbounds[2 * X + 1], 0, min(a.hk, a.W - xmin));
      s_h[(r0 + r) * hrow + rem] = (uint8_t)cp_taps(s_in + r * srow + xmin * 3 + c, 3, a.hcoef + (size_t)X * a.hk, cnt);
    }
    __syncthreads();
  }

  // one output byte of the band: byte i of its nout x o3 contiguous bytes
  auto vertical = [&](int i) -> uint32_t {
    const int r = i / o3, rem = i - r * o3, Y = Y0 + r;
    const int ymin = ru_clampi(a.vbounds[2 * Y] - y_lo, 0, nrows);
    const int cnt = ru_clampi(a.vbounds[2 * Y + 1], 0, min(a.vk, nrows - ymin));
    return (uint32_t)cp_taps(s_h + ymin * hrow + rem, hrow, a.vcoef + (size_t)Y * a.vk, cnt);
  };
  uint8_t* dst = a.out + ((size_t)n * a.oh + Y0) * o3;
  const int total = nout * o3;
  const int head = min((int)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3), total);
  const int words = (total - head) >> 2, tail0 = head + words * 4;
  for (int i = t; i < words; i += RU_TB) {
    const int b = head + i * 4;
    *reinterpret_cast<uint32_t*>(dst + b) = vertical(b) | (vertical(b + 1) << 8) | (vertical(b + 2) << 16) | (vertical(b + 3) << 24);
  }
  const int loose = head + (total - tail0);                                 // at most 3 + 3 bytes outside the packed words
  if (t < loose) {
    const int b = t < head ? t : tail0 + (t - head);
    dst[b] = (uint8_t)vertical(b);
  }
}

template <bool F32, bool VEC>
int ru_launch(const RuArgs& a, size_t lds, hipStream_t s) {
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&resize_u8_kernel<F32, VEC>), hipFuncAttributeMaxDynamicSharedMemorySize, CP_LDS_LIMIT);
    attr_set = true;
  }
  hipLaunchKernelGGL((resize_u8_kernel<F32, VEC>), dim3((unsigned)(a.N * ((a.oh + a.band - 1) / a.band))), dim3(RU_TB), lds, s, a);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

}  // namespace

extern "C" int ddpo_resize_u8(const void* images, int is_float32, int N, int H, int W, int oh, int ow, const int32_t* hcoef, const int32_t* hbounds,
                              int hksize, const int32_t* vcoef, const int32_t* vbounds, int vksize, int band, int rows, uint8_t* out,
                              void* stream) {
  if (!images || !hcoef || !hbounds || !vcoef || !vbounds || !out) return DDPO_EINVAL;
  const RuArgs a{images, N, H, W, oh, ow, hcoef, hbounds, hksize, vcoef, vbounds, vksize, band, rows, out};
  if (!ru_geometry_ok(a) || rows < 1 || rows > H) return DDPO_EINVAL;
  if (is_float32 && (reinterpret_cast<uintptr_t>(images) & 3)) return DDPO_EINVAL;
  const size_t lds = ru_lds_bytes(rows, ow, W);
  if (lds > CP_LDS_LIMIT) return DDPO_EINVAL;                               // the LDS rule
  const bool vec = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(images) & (is_float32 ? 15 : 3)) == 0;
  hipStream_t s = as_stream(stream);
  if (is_float32) return vec ? ru_launch<true, true>(a, lds, s) : ru_launch<true, false>(a, lds, s);
  return vec ? ru_launch<false, true>(a, lds, s) : ru_launch<false, false>(a, lds, s);
}

// Serial host path over the same functions (no GPU involved): what the kernel is held to, and what is held to Pillow.  Every image is resampled
// horizontally at once instead of a band at a time; every output byte is the same sum.  `band` only decides the LDS rule, as on the device.
extern "C" int ddpo_resize_u8_host(const void* images, int is_float32, int N, int H, int W, int oh, int ow, const int32_t* hcoef,
                                   const int32_t* hbounds, int hksize, const int32_t* vcoef, const int32_t* vbounds, int vksize, int band,
                                   uint8_t* out_host) {
  if (!images || !hcoef || !hbounds || !vcoef || !vbounds || !out_host) return DDPO_EINVAL;
  const RuArgs a{images, N, H, W, oh, ow, hcoef, hbounds, hksize, vcoef, vbounds, vksize, band, 0, out_host};
  if (!ru_geometry_ok(a)) return DDPO_EINVAL;
  for (int X = 0; X < ow; ++X)
    if (hbounds[2 * X] < 0 || hbounds[2 * X + 1] < 0 || hbounds[2 * X + 1] > hksize || hbounds[2 * X] > W - hbounds[2 * X + 1]) return DDPO_EINVAL;
  for (int Y = 0; Y < oh; ++Y)
    if (vbounds[2 * Y] < 0 || vbounds[2 * Y + 1] < 0 || vbounds[2 * Y + 1] > vksize || vbounds[2 * Y] > H - vbounds[2 * Y + 1] ||
        (Y > 0 && vbounds[2 * Y] < vbounds[2 * (Y - 1)]))
      return DDPO_EINVAL;
  int rows = 1, y_hi = 0;
  for (int Y0 = 0; Y0 < oh; Y0 += band) {
    int hi = 0;
    for (int Y = Y0; Y < std::min(Y0 + band, oh); ++Y) hi = std::max(hi, vbounds[2 * Y] + vbounds[2 * Y + 1]);
    rows = std::max(rows, hi - vbounds[2 * Y0]);
    y_hi = std::max(y_hi, hi);
  }
  if (ru_lds_bytes(rows, ow, W) > CP_LDS_LIMIT) return DDPO_EINVAL;         // the LDS rule: the same domain as the device entry
  const int o3 = ow * 3, w3 = W * 3, y_lo = vbounds[0];
  std::vector<uint8_t> in_row((size_t)w3), hbuf((size_t)std::max(y_hi - y_lo, 1) * o3);
  for (int n = 0; n < N; ++n) {
    for (int y = y_lo; y < y_hi; ++y) {
      const size_t src = ((size_t)n * H + y) * w3;
      for (int e = 0; e < w3; ++e)
        in_row[e] = is_float32 ? (uint8_t)cp_float_to_u8(static_cast<const float*>(images)[src + e]) : static_cast<const uint8_t*>(images)[src + e];
      for (int X = 0; X < ow; ++X)
        for (int c = 0; c < 3; ++c)
          hbuf[(size_t)(y - y_lo) * o3 + X * 3 + c] =
              (uint8_t)cp_taps(in_row.data() + hbounds[2 * X] * 3 + c, 3, hcoef + (size_t)X * hksize, hbounds[2 * X + 1]);
    }
    for (int Y = 0; Y < oh; ++Y)
      for (int e = 0; e < o3; ++e)
        out_host[((size_t)n * oh + Y) * o3 + e] =
            (uint8_t)cp_taps(hbuf.data() + (size_t)(vbounds[2 * Y] - y_lo) * o3 + e, o3, vcoef + (size_t)Y * vksize, vbounds[2 * Y + 1]);
  }
  return DDPO_OK;
}
