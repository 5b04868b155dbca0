// The 8-bit two-pass bicubic resize (what Pillow's Image.resize does to an RGB image): the per-pixel integer arithmetic and the band pass built
// on it, as host + device inline functions.  csrc/clip_preprocess.hip and csrc/resize_u8.hip run them from their kernels and from their serial
// host entries (ddpo_clip_preprocess_host, ddpo_resize_u8_host), so whether the bytes equal Pillow's is decided by the host entries against
// Pillow itself (tests/test_clip_preprocess_cpu.py, tests/test_thumbnail_cpu.py) and the kernels only have to agree with the host entries.
// Plain C++17 but for the kernels' half at the bottom (under __HIPCC__).
//
// Everything here is integer once the pixel is a byte (image_u8.h): the coefficient tables arrive as 22-bit fixed-point int32 (built by the caller
// in double precision, lib.clip_preprocess_tables), a pass is acc = 2^21 + sum(pixel * coeff), result = clamp(acc >> 22, 0, 255), and the
// horizontal pass is rounded to a byte before the vertical pass reads it.
//
// The band pass: a workgroup makes a band of consecutive output rows.  The input rows the band needs (from the vertical bound table) are staged
// CP_STAGE_ROWS at a time into LDS as bytes and resampled horizontally, over a window of output columns, into `rows` rows of LDS; every output
// byte is then one vertical tap out of LDS.  What a kernel does with that byte is its own.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "image_u8.h"

#define CP_HD IU_HD

#define CP_PRECISION_BITS 22            // 32 - 8 - 2: a byte times a coefficient, summed over a kernel with negative lobes, stays inside int32

CP_HD int cp_round_clamp(int acc) {
  const int v = acc >> CP_PRECISION_BITS;          // arithmetic shift: the accumulator may be negative
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// One output byte of one pass: `count` taps over bytes `stride` apart
CP_HD int cp_taps(const uint8_t* px, int stride, const int32_t* coef, int count) {
  int acc = 1 << (CP_PRECISION_BITS - 1);
  for (int k = 0; k < count; ++k) acc += (int)px[(size_t)k * stride] * coef[k];
  return cp_round_clamp(acc);
}

// The two axis tables of a resize (lib.clip_preprocess_tables): coef [out][k] weights, bounds [out][2] {first input pixel, tap count}.  `rows`,
// the rows of LDS a launch gives the horizontally resampled bytes (0 in a host entry), rides in what would be padding: the kernel arguments that
// embed this struct keep the size and the registers they had with the fields spelled out.
struct CpAxes {
  const int32_t *hcoef, *hbounds;
  int hk;
  const int32_t *vcoef, *vbounds;
  int vk, rows;
};

// Bytes of LDS one workgroup uses: `rows` horizontally resampled rows of out_w x 3 bytes + CP_STAGE_ROWS input rows of W x 3 bytes (each rounded
// up to 16) + where asked the 256 x 3 normalisation table.  The supported domain is "this fits CP_LDS_LIMIT" for the device and the host entries alike.
#define CP_STAGE_ROWS 8
#define CP_LDS_LIMIT (160 * 1024)
CP_HD size_t cp_lds_bytes(int rows, int out_w, int W, bool norm_table) {
  return (size_t)rows * iu_row_bytes(out_w) + (size_t)CP_STAGE_ROWS * iu_row_bytes(W) + (norm_table ? 256 * 3 * sizeof(float) : 0);
}

// ---------------------------------------------------------------------------------------------------------------- host entries
// Entries [first, first + count) of one axis' bound table read only inside their coefficient rows and inside the `in_size` input pixels;
// `ordered`: the first input pixel never decreases (what the band pass assumes of the vertical axis)
inline bool cp_axis_ok(const int32_t* bounds, int ksize, int first, int count, int in_size, bool ordered) {
  for (int X = first; X < first + count; ++X) {
    const int lo = bounds[2 * X], cnt = bounds[2 * X + 1];
    if (lo < 0 || cnt < 0 || cnt > ksize || lo > in_size - cnt || (ordered && X > first && lo < bounds[2 * (X - 1)])) return false;
  }
  return true;
}

// The most input rows any band of `band` output rows spans (at least 1), the output rows being [first, first + count) and the last band
// possibly short; y_hi: one past the last input row any of them reads
inline int cp_band_max_rows(const int32_t* vbounds, int first, int count, int band, int& y_hi) {
  int rows = 1;
  y_hi = 0;
  for (int Y0 = first; Y0 < first + count; Y0 += band) {
    int hi = 0;
    for (int Y = Y0; Y < std::min(Y0 + band, first + count); ++Y) hi = std::max(hi, vbounds[2 * Y] + vbounds[2 * Y + 1]);
    rows = std::max(rows, hi - vbounds[2 * Y0]);
    y_hi = std::max(y_hi, hi);
  }
  return rows;
}

// Serial horizontal pass: input rows [y_lo, y_hi) of image n, output columns [x_first, x_first + x_count), into hbuf[y - y_lo][x_count * 3]
inline void cp_horizontal_host(const CpAxes& ax, const void* images, int is_float32, int n, int H, int W, int y_lo, int y_hi, int x_first,
                               int x_count, uint8_t* hbuf) {
  const int o3 = x_count * 3, w3 = W * 3;
  std::vector<uint8_t> in_row((size_t)w3);
  for (int y = y_lo; y < y_hi; ++y) {
    const size_t src = ((size_t)n * H + y) * w3;
    for (int e = 0; e < w3; ++e) in_row[e] = (uint8_t)iu_byte(images, is_float32, src + e);
    for (int e = 0; e < o3; ++e) {
      const int X = x_first + e / 3, c = e % 3;
      hbuf[(size_t)(y - y_lo) * o3 + e] =
          (uint8_t)cp_taps(in_row.data() + ax.hbounds[2 * X] * 3 + c, 3, ax.hcoef + (size_t)X * ax.hk, ax.hbounds[2 * X + 1]);
    }
  }
}

#if defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------------------------- kernels
// Input rows [y_lo, y_lo + nrows) feed the output rows Y0 .. Y0 + nout - 1 (the first bound of a table never decreases).  Bounds are clamped to
// the H rows of the image and to the `rows` rows of LDS the launch was given, so a bad table cannot make a kernel read or write outside its
// arguments.
struct CpBand {
  int y_lo, nrows;
};
__device__ __forceinline__ CpBand cp_band_rows(const CpAxes& ax, int Y0, int nout, int H) {
  int y_lo = ax.vbounds[2 * Y0], y_hi = y_lo;
  for (int r = 0; r < nout; ++r) y_hi = max(y_hi, ax.vbounds[2 * (Y0 + r)] + ax.vbounds[2 * (Y0 + r) + 1]);
  y_lo = iu_clampi(y_lo, 0, H);
  return {y_lo, iu_clampi(min(y_hi, H) - y_lo, 0, ax.rows)};
}

// The band's input rows of image n, staged through s_in [CP_STAGE_ROWS][srow] and resampled over the output columns [x_first, x_first + x_count)
// into s_h [nrows][hrow], by the TB threads of a workgroup (thread t).  Synchronised on return when a row was staged.
template <bool F32, bool VEC, int TB>
__device__ __forceinline__ void cp_horizontal_pass(const CpAxes& ax, const void* images, int n, int H, int W, const CpBand b, int x_first,
                                                   int x_count, uint8_t* s_h, int hrow, uint8_t* s_in, int srow, int t) {
  const int o3 = x_count * 3, w3 = W * 3;
  for (int r0 = 0; r0 < b.nrows; r0 += CP_STAGE_ROWS) {
    const int nr = min(CP_STAGE_ROWS, b.nrows - r0);
    iu_stage<F32, VEC, TB>(s_in, srow, images, ((size_t)n * H + (size_t)(b.y_lo + r0)) * w3, (size_t)w3, nr, w3, t);
    __syncthreads();
    for (int i = t; i < nr * o3; i += TB) {
      const int r = i / o3, rem = i - r * o3, xo = rem / 3, c = rem - xo * 3;
      const int X = x_first + xo;
      const int xmin = iu_clampi(ax.hbounds[2 * X], 0, W);
      const int cnt = iu_clampi(ax.hbounds[2 * X + 1], 0, min(ax.hk, W - xmin));
      s_h[(r0 + r) * hrow + rem] = (uint8_t)cp_taps(s_in + r * srow + xmin * 3 + c, 3, ax.hcoef + (size_t)X * ax.hk, cnt);
    }
    __syncthreads();
  }
}

// One output byte: output row Y of the band, byte `offset` of a row of s_h
__device__ __forceinline__ int cp_vertical_byte(const CpAxes& ax, const CpBand b, const uint8_t* s_h, int hrow, int Y, int offset) {
  const int ymin = iu_clampi(ax.vbounds[2 * Y] - b.y_lo, 0, b.nrows);
  const int cnt = iu_clampi(ax.vbounds[2 * Y + 1], 0, min(ax.vk, b.nrows - ymin));
  return cp_taps(s_h + ymin * hrow + offset, hrow, ax.vcoef + (size_t)Y * ax.vk, cnt);
}
#endif
