// Stand-alone host check of the 8-bit bicubic resize (ddpo_amd/csrc/clip_preprocess_core.h through the serial entry ddpo_resize_u8_host of
// csrc/resize_u8.hip, which this file includes): saturated 0/255 images — the largest accumulators — noise and out-of-range / NaN floats over
// the thumbnail's down-scales (by 4, 8, 16, down to one pixel), an identity axis, an up-scale and odd sizes, with the tables of bicubic_axis.h.
// Nothing runs on a GPU; meant to be built with a host sanitizer (make -C tools/native resize_u8_host_check):
//   hipcc --offload-arch=gfx950 -x hip -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all ...
// Exits non-zero if the entry refuses a valid case, accepts a broken table, a band of 0 rows or a shape beyond the LDS rule, or leaves an
// output byte unwritten where it can tell (a constant image must stay constant).
#include <cstdio>

#include "../../ddpo_amd/csrc/resize_u8.hip"
#include "bicubic_axis.h"

static uint32_t rng_state = 12345u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

int main() {
  const int cases[][4] = {{16, 16, 4, 4},  {16, 16, 1, 1},   {17, 23, 4, 5},     {64, 64, 4, 4},    {48, 80, 12, 20},
                          {24, 40, 24, 10}, {8, 8, 20, 12},  {300, 52, 75, 13},  {512, 512, 32, 32}, {768, 768, 48, 48}};
  int failures = 0;
  for (const auto& cs : cases) {
    const int H = cs[0], W = cs[1], oh = cs[2], ow = cs[3];
    const Axis hx = make_axis(W, ow), vx = make_axis(H, oh);
    std::vector<uint8_t> out((size_t)2 * oh * ow * 3);
    for (int recipe = 0; recipe < 4; ++recipe) {
      std::vector<uint8_t> u8((size_t)2 * H * W * 3);
      std::vector<float> f32(u8.size());
      for (size_t i = 0; i < u8.size(); ++i) {
        u8[i] = recipe == 0 ? ((rnd() & 1) ? 255 : 0) : recipe == 3 ? 77 : (uint8_t)rnd();
        f32[i] = recipe == 2 ? (float)((int)(rnd() % 2000) - 500) / 1000.0f : (u8[i] + 0.5f) / 255.0f;      // recipe 2: also outside [0, 1]
      }
      if (recipe == 2) f32[0] = NAN;
      for (int is_float = 0; is_float < 2; ++is_float)
        for (int band = 1; band <= 8; band *= 8) {
          for (auto& v : out) v = 0xAB;
          const int rc = ddpo_resize_u8_host(is_float ? (const void*)f32.data() : (const void*)u8.data(), is_float, 2, H, W, oh, ow, hx.coef.data(),
                                             hx.bounds.data(), hx.ksize, vx.coef.data(), vx.bounds.data(), vx.ksize, band, out.data());
          bool ok = rc == 0;
          if (recipe == 3)
            for (const uint8_t v : out) ok = ok && v == 77;
          if (!ok) std::printf("FAIL %dx%d -> %dx%d recipe %d float %d band %d (rc %d)\n", H, W, oh, ow, recipe, is_float, band, rc), ++failures;
        }
    }
    const std::vector<uint8_t> img((size_t)H * W * 3);
    Axis bad = vx;                                                // a bound that points past the image must be refused, not followed
    bad.bounds[0] = H;
    if (ddpo_resize_u8_host(img.data(), 0, 1, H, W, oh, ow, hx.coef.data(), hx.bounds.data(), hx.ksize, bad.coef.data(), bad.bounds.data(), bad.ksize,
                            8, out.data()) != -1)
      std::printf("FAIL %dx%d: broken vertical table accepted\n", H, W), ++failures;
    bad = hx;
    bad.bounds[2 * (ow - 1) + 1] = hx.ksize + 1;
    if (ddpo_resize_u8_host(img.data(), 0, 1, H, W, oh, ow, bad.coef.data(), bad.bounds.data(), bad.ksize, vx.coef.data(), vx.bounds.data(), vx.ksize,
                            8, out.data()) != -1)
      std::printf("FAIL %dx%d: broken horizontal table accepted\n", H, W), ++failures;
    if (ddpo_resize_u8_host(img.data(), 0, 1, H, W, oh, ow, hx.coef.data(), hx.bounds.data(), hx.ksize, vx.coef.data(), vx.bounds.data(), vx.ksize, 0,
                            out.data()) != -1)
      std::printf("FAIL %dx%d: a band of 0 rows accepted\n", H, W), ++failures;
  }
  {                                                               // 8 staged rows of 7000 x 3 bytes alone are beyond the 160 KB of LDS
    const int H = 16, W = 7000, oh = 4, ow = 1750;
    const Axis hx = make_axis(W, ow), vx = make_axis(H, oh);
    const std::vector<uint8_t> img((size_t)H * W * 3);
    std::vector<uint8_t> out((size_t)oh * ow * 3);
    if (ddpo_resize_u8_host(img.data(), 0, 1, H, W, oh, ow, hx.coef.data(), hx.bounds.data(), hx.ksize, vx.coef.data(), vx.bounds.data(), vx.ksize, 1,
                            out.data()) != -1)
      std::printf("FAIL: a shape beyond the LDS rule accepted\n"), ++failures;
  }
  std::printf("resize_u8_host_check: %d failures\n", failures);
  return failures ? 1 : 0;
}
