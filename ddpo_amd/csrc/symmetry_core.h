// Symmetry rewards (mirror, mirror_corr, rotational_corr, rotational): the per-element integer arithmetic as host + device inline functions.
// csrc/symmetry.hip runs them from its kernels and from the serial host entries (ddpo_symmetry_stats_host, ddpo_rotate4_u8_host), so what the
// numbers mean is decided by the host entries against numpy / Pillow (tests/test_symmetry_cpu.py) and the kernels only have to agree with the
// host entries.  Plain C++17: no HIP header is needed.
//
// Everything is integer once the pixel is a byte (iu_float_to_u8 of image_u8.h), so every sum is exact and independent of the order
// it is taken in.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "image_u8.h"

#define SY_HD IU_HD

// The widest image: one row of W x 3 bytes is staged in LDS (two rows for rotate-180), and no 32-bit partial below is fed more than
// SY_U32_ELEMS elements before it is added to a 64-bit sum: the largest term is 255^2 = 65025 and 66051 * 65025 < 2^32 <= 66052 * 65025.
#define SY_MAX_W 10880
#define SY_U32_ELEMS 66051

// 32-bit partial sums over at most SY_U32_ELEMS elements: {wrapped, a, a^2, a b}
struct SyPartial {
  uint32_t s[4];
};

// One element a with its partner b.  The wrapped term is what numpy's uint8 arithmetic makes of (a - b) ** 2: the difference modulo 256,
// squared modulo 256.
SY_HD void sy_add(SyPartial& p, int a, int b) {
  const int d = (a - b) & 255;
  p.s[0] += (uint32_t)((d * d) & 255);
  p.s[1] += (uint32_t)a;
  p.s[2] += (uint32_t)(a * a);
  p.s[3] += (uint32_t)(a * b);
}

// Byte offset, inside a row of W pixels, of the left-right partner of the byte at offset e = 3 x + c: pixel W - 1 - x, channel c
SY_HD int sy_mirror_offset(int e, int W) {
  const int x = e / 3;
  return (W - 1 - x) * 3 + (e - 3 * x);
}

// Partner row of row y: itself (mode 0, mirror) or H - 1 - y (mode 1, rotate 180)
SY_HD int sy_partner_row(int y, int H, int mode) { return mode ? H - 1 - y : y; }

// Source pixel (iy, ix) of pixel (oy, ox) of an S x S image turned by 90 k degrees counter-clockwise — PIL.Image.rotate(90 k), which for a
// square image is np.rot90(a, k)
SY_HD void sy_rot_src(int k, int S, int oy, int ox, int& iy, int& ix) {
  switch (k & 3) {
    case 0: iy = oy; ix = ox; break;
    case 1: iy = ox; ix = S - 1 - oy; break;
    case 2: iy = S - 1 - oy; ix = S - 1 - ox; break;
    default: iy = S - 1 - ox; ix = oy; break;
  }
}
// Where pixel (iy, ix) of the source lands: the source pixel of the opposite turn
SY_HD void sy_rot_dst(int k, int S, int iy, int ix, int& oy, int& ox) { sy_rot_src(4 - (k & 3), S, iy, ix, oy, ox); }
