// CLIP image preprocessing on the device (the aesthetic_device / clip_score_device rewards): decoder images in HBM -> the patch matrix the
// patch-embedding GEMM reads, in ONE launch.  Byte conversion by truncation, Pillow's 8-bit two-pass bicubic resize of the short side, centre
// crop, (x / 255 - mean) / std through a 256 x 3 table, im2col of the stride-p p x p convolution.  The arithmetic is csrc/clip_preprocess_core.h,
// shared with the serial host entry at the bottom; the coefficient tables are the caller's (lib.clip_preprocess_tables), nothing here is
// computed in double precision.
//
// One workgroup per (image, patch row):
//   1. the input rows the p output rows of that patch row need (from the vertical bound table) are staged CP_STAGE_ROWS at a time into LDS as
//      bytes — 16-byte loads, coalesced along W — and resampled horizontally, only over the cropped window, into `rows` x size x 3 bytes of LDS;
//   2. the vertical pass runs out of LDS, each byte indexes the normalisation table and the finished patch-matrix rows leave as 16-byte stores,
//      pad columns (3 p p .. ld) as zeros.
// No workspace, no atomics, no state outside the arguments: calls on different streams may overlap.  Neighbouring patch rows re-read the input
// rows their kernels share (about support / p of the image); nothing else is read twice from HBM.
#include "common.h"
#include "clip_preprocess_core.h"

namespace {

constexpr int CP_TB = 512;

struct CpArgs {
  const void* images;
  int N, H, W, rh, rw, top, left, size, patch;
  CpAxes ax;
  const float* norm;
  float* out;
  int ld;
};

// Everything the device and the host entry refuse alike (pointers and the LDS rule are checked by the callers)
bool cp_geometry_ok(const CpArgs& a) {
  if (a.N < 1 || a.H < 1 || a.W < 1 || a.rh < 1 || a.rw < 1 || a.size < 1 || a.patch < 1 || a.size % a.patch) return false;
  if (a.patch > 1024 || a.size > (1 << 15) || a.H > (1 << 24) || a.W > (1 << 24)) return false;
  if (a.ld < 3 * a.patch * a.patch || (a.ld & 3)) return false;
  if (a.top < 0 || a.left < 0 || a.top > a.rh - a.size || a.left > a.rw - a.size) return false;      // crop window inside the resized image
  if (a.ax.hk < 1 || a.ax.vk < 1) return false;
  if ((int64_t)a.N * (a.size / a.patch) > 0x7fffffff) return false;
  return true;
}

template <bool F32, bool VEC>
__global__ __launch_bounds__(CP_TB) void clip_preprocess_kernel(const CpArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x;
  const int g = a.size / a.patch;
  const int n = blockIdx.x / g, gy = blockIdx.x % g;
  const int hrow = (int)iu_row_bytes(a.size), srow = (int)iu_row_bytes(a.W);
  uint8_t* s_h = reinterpret_cast<uint8_t*>(smem);                          // [rows][hrow]: horizontally resampled bytes
  uint8_t* s_in = s_h + (size_t)a.ax.rows * hrow;                              // [CP_STAGE_ROWS][srow]: input rows as bytes
  float* s_norm = reinterpret_cast<float*>(s_in + (size_t)CP_STAGE_ROWS * srow);
  for (int i = t; i < 256 * 3; i += CP_TB) s_norm[i] = a.norm[i];

  const int Y0 = a.top + gy * a.patch;                                      // the band: the p output rows of this patch row, cropped columns only
  const CpBand band = cp_band_rows(a.ax, Y0, a.patch, a.H);
  cp_horizontal_pass<F32, VEC, CP_TB>(a.ax, a.images, n, a.H, a.W, band, a.left, a.size, s_h, hrow, s_in, srow, t);
  __syncthreads();                                                          // s_norm, also when no row was staged

  const int ld4 = a.ld >> 2, pp = a.patch * a.patch, kp = 3 * pp;
  for (int i = t; i < g * ld4; i += CP_TB) {
    const int gx = i / ld4, col0 = (i - gx * ld4) * 4;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = col0 + j;
      float val = 0.0f;                                                     // pad columns
      if (col < kp) {
        const int c = col / pp, rem = col - c * pp, ky = rem / a.patch, kx = rem - ky * a.patch;
        val = s_norm[cp_vertical_byte(a.ax, band, s_h, hrow, Y0 + ky, (gx * a.patch + kx) * 3 + c) * 3 + c];
      }
      v[j] = val;
    }
    float* dst = a.out + ((size_t)(n * g + gy) * g + gx) * a.ld + col0;
    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

}  // namespace

extern "C" int ddpo_clip_preprocess(const void* images, int is_float32, int N, int H, int W, int rh, int rw, int top, int left, int size, int patch,
                                    const int32_t* hcoef, const int32_t* hbounds, int hksize, const int32_t* vcoef, const int32_t* vbounds,
                                    int vksize, int rows, const float* norm, float* out, int ld, void* stream) {
  if (!images || !hcoef || !hbounds || !vcoef || !vbounds || !norm || !out) return DDPO_EINVAL;
  const CpArgs a{images, N, H, W, rh, rw, top, left, size, patch, {hcoef, hbounds, hksize, vcoef, vbounds, vksize, rows}, norm, out, ld};
  if (!cp_geometry_ok(a) || rows < 1 || rows > H) return DDPO_EINVAL;
  if ((reinterpret_cast<uintptr_t>(out) & 15) || iu_misaligned(images, is_float32)) return DDPO_EINVAL;
  const size_t lds = cp_lds_bytes(rows, size, W, true);
  if (lds > CP_LDS_LIMIT) return DDPO_EINVAL;                               // the LDS rule
  iu_dispatch(is_float32, iu_vec_ok(images, is_float32, W), [&](auto F32, auto VEC) {
    iu_large_lds<&clip_preprocess_kernel<F32(), VEC()>>(CP_LDS_LIMIT);
    hipLaunchKernelGGL((clip_preprocess_kernel<F32(), VEC()>), dim3((unsigned)(N * (size / patch))), dim3(CP_TB), lds, as_stream(stream), a);
  });
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

// Serial host path over the same functions (no GPU involved): what the kernel is held to, and what is held to Pillow.  The whole cropped window is
// resampled horizontally at once instead of a patch row at a time; every output byte is the same sum.  resized_out_host (may be null):
// the N x size x size x 3 bytes before normalisation.
extern "C" int ddpo_clip_preprocess_host(const void* images, int is_float32, int N, int H, int W, int rh, int rw, int top, int left, int size,
                                         int patch, const int32_t* hcoef, const int32_t* hbounds, int hksize, const int32_t* vcoef,
                                         const int32_t* vbounds, int vksize, const float* norm, float* out_host, int ld, uint8_t* resized_out_host) {
  if (!images || !hcoef || !hbounds || !vcoef || !vbounds || !norm || !out_host) return DDPO_EINVAL;
  const CpArgs a{images, N, H, W, rh, rw, top, left, size, patch, {hcoef, hbounds, hksize, vcoef, vbounds, vksize, 0}, norm, out_host, ld};
  if (!cp_geometry_ok(a)) return DDPO_EINVAL;
  if (!cp_axis_ok(hbounds, hksize, left, size, W, false) || !cp_axis_ok(vbounds, vksize, top, size, H, true)) return DDPO_EINVAL;
  int y_hi;
  const int rows = cp_band_max_rows(vbounds, top, size, patch, y_hi);
  if (cp_lds_bytes(rows, size, W, true) > CP_LDS_LIMIT) return DDPO_EINVAL; // the LDS rule: the same domain as the device entry
  const int g = size / patch, pp = patch * patch, s3 = size * 3, y_lo = vbounds[2 * top];
  std::vector<uint8_t> hbuf((size_t)std::max(y_hi - y_lo, 1) * s3);
  for (int n = 0; n < N; ++n) {
    cp_horizontal_host(a.ax, images, is_float32, n, H, W, y_lo, y_hi, left, size, hbuf.data());
    for (int yo = 0; yo < size; ++yo)
      for (int xo = 0; xo < size; ++xo)
        for (int c = 0; c < 3; ++c) {
          const int Y = top + yo;
          const int b = cp_taps(hbuf.data() + (size_t)(vbounds[2 * Y] - y_lo) * s3 + xo * 3 + c, s3, vcoef + (size_t)Y * vksize, vbounds[2 * Y + 1]);
          if (resized_out_host) resized_out_host[(((size_t)n * size + yo) * size + xo) * 3 + c] = (uint8_t)b;
          const size_t row = ((size_t)n * g + yo / patch) * g + xo / patch;
          out_host[row * ld + c * pp + (yo % patch) * patch + xo % patch] = norm[b * 3 + c];
        }
    for (int r = 0; r < g * g; ++r)
      for (int col = 3 * pp; col < ld; ++col) out_host[((size_t)n * g * g + r) * ld + col] = 0.0f;
  }
  return DDPO_OK;
}
