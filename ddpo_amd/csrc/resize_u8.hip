// 8-bit bicubic resize on the device (the thumbnail_device reward): an N x H x W x 3 batch in HBM -> N x oh x ow x 3 BYTES, what Pillow's
// Image.resize(BICUBIC) returns for an RGB image, in ONE launch.  Byte conversion by truncation, horizontal pass rounded to a byte, vertical
// pass.  The arithmetic and the band pass are csrc/clip_preprocess_core.h, shared with csrc/clip_preprocess.hip and with the serial host entry at
// the bottom; the coefficient tables are the caller's (lib.clip_preprocess_tables), nothing here is computed in double precision.
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

namespace {

constexpr int RU_TB = 512;

struct RuArgs {
  const void* images;
  int N, H, W, oh, ow;
  CpAxes ax;
  int band;
  uint8_t* out;
};

// Everything the device and the host entry refuse alike (pointers and the LDS rule are checked by the callers)
bool ru_geometry_ok(const RuArgs& a) {
  if (a.N < 1 || a.H < 1 || a.W < 1 || a.oh < 1 || a.ow < 1 || a.ax.hk < 1 || a.ax.vk < 1 || a.band < 1) return false;
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
  const int hrow = (int)iu_row_bytes(a.ow), srow = (int)iu_row_bytes(a.W);
  uint8_t* s_h = reinterpret_cast<uint8_t*>(smem);                          // [rows][hrow]: horizontally resampled bytes
  uint8_t* s_in = s_h + (size_t)a.ax.rows * hrow;                              // [CP_STAGE_ROWS][srow]: input rows as bytes

  const CpBand band = cp_band_rows(a.ax, Y0, nout, a.H);
  cp_horizontal_pass<F32, VEC, RU_TB>(a.ax, a.images, n, a.H, a.W, band, 0, a.ow, s_h, hrow, s_in, srow, t);

  // one output byte of the band: byte i of its nout x o3 contiguous bytes
  const int o3 = a.ow * 3;
  auto vertical = [&](int i) -> uint32_t {
    const int r = i / o3;
    return (uint32_t)cp_vertical_byte(a.ax, band, s_h, hrow, Y0 + r, i - r * o3);
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

}  // namespace

extern "C" int ddpo_resize_u8(const void* images, int is_float32, int N, int H, int W, int oh, int ow, const int32_t* hcoef, const int32_t* hbounds,
                              int hksize, const int32_t* vcoef, const int32_t* vbounds, int vksize, int band, int rows, uint8_t* out,
                              void* stream) {
  if (!images || !hcoef || !hbounds || !vcoef || !vbounds || !out) return DDPO_EINVAL;
  const RuArgs a{images, N, H, W, oh, ow, {hcoef, hbounds, hksize, vcoef, vbounds, vksize, rows}, band, out};
  if (!ru_geometry_ok(a) || rows < 1 || rows > H) return DDPO_EINVAL;
  if (iu_misaligned(images, is_float32)) return DDPO_EINVAL;
  const size_t lds = cp_lds_bytes(rows, ow, W, false);
  if (lds > CP_LDS_LIMIT) return DDPO_EINVAL;                               // the LDS rule
  iu_dispatch(is_float32, iu_vec_ok(images, is_float32, W), [&](auto F32, auto VEC) {
    iu_large_lds<&resize_u8_kernel<F32(), VEC()>>(CP_LDS_LIMIT);
    hipLaunchKernelGGL((resize_u8_kernel<F32(), VEC()>), dim3((unsigned)(N * ((oh + band - 1) / band))), dim3(RU_TB), lds, as_stream(stream), a);
  });
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

// Serial host path over the same functions (no GPU involved): what the kernel is held to, and what is held to Pillow.  Every image is resampled
// horizontally at once instead of a band at a time; every output byte is the same sum.  `band` only decides the LDS rule, as on the device.
extern "C" int ddpo_resize_u8_host(const void* images, int is_float32, int N, int H, int W, int oh, int ow, const int32_t* hcoef,
                                   const int32_t* hbounds, int hksize, const int32_t* vcoef, const int32_t* vbounds, int vksize, int band,
                                   uint8_t* out_host) {
  if (!images || !hcoef || !hbounds || !vcoef || !vbounds || !out_host) return DDPO_EINVAL;
  const RuArgs a{images, N, H, W, oh, ow, {hcoef, hbounds, hksize, vcoef, vbounds, vksize, 0}, band, out_host};
  if (!ru_geometry_ok(a)) return DDPO_EINVAL;
  if (!cp_axis_ok(hbounds, hksize, 0, ow, W, false) || !cp_axis_ok(vbounds, vksize, 0, oh, H, true)) return DDPO_EINVAL;
  int y_hi;
  const int rows = cp_band_max_rows(vbounds, 0, oh, band, y_hi);
  if (cp_lds_bytes(rows, ow, W, false) > CP_LDS_LIMIT) return DDPO_EINVAL;  // the LDS rule: the same domain as the device entry
  const int o3 = ow * 3, y_lo = vbounds[0];
  std::vector<uint8_t> hbuf((size_t)std::max(y_hi - y_lo, 1) * o3);
  for (int n = 0; n < N; ++n) {
    cp_horizontal_host(a.ax, images, is_float32, n, H, W, y_lo, y_hi, 0, ow, hbuf.data());
    for (int Y = 0; Y < oh; ++Y)
      for (int e = 0; e < o3; ++e)
        out_host[((size_t)n * oh + Y) * o3 + e] =
            (uint8_t)cp_taps(hbuf.data() + (size_t)(vbounds[2 * Y] - y_lo) * o3 + e, o3, vcoef + (size_t)Y * vksize, vbounds[2 * Y + 1]);
  }
  return DDPO_OK;
}
