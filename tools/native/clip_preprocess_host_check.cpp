// Stand-alone host check of the CLIP preprocessing arithmetic (ddpo_amd/csrc/clip_preprocess_core.h through the serial entry
// ddpo_clip_preprocess_host of csrc/clip_preprocess.hip, which this file includes): saturated 0/255 images — the largest accumulators — noise
// and out-of-range / NaN floats over down-scaling, up-scaling, cropping and odd sizes, with bicubic tables built here in double precision.  Nothing
// runs on a GPU; meant to be built with a host sanitizer (make -C tools/native clip_preprocess_host_check):
//   hipcc --offload-arch=gfx950 -x hip -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all ...
// Exits non-zero if the entry refuses a valid case, accepts a broken table, or leaves a pad column non-zero.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../ddpo_amd/csrc/clip_preprocess.hip"
#include "bicubic_axis.h"

static uint32_t rng_state = 12345u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

int main() {
  const int cases[][3] = {{64, 64, 56}, {32, 32, 56}, {48, 80, 56}, {80, 48, 56}, {56, 80, 56}, {17, 23, 56}, {512, 512, 224}};
  const int patch = 14, ld = 608;
  std::vector<float> norm(768);
  for (int i = 0; i < 768; ++i) norm[i] = (float)i;
  int failures = 0;
  for (const auto& cs : cases) {
    const int H = cs[0], W = cs[1], size = cs[2], g = size / patch;
    const int shortside = W <= H ? W : H, longside = W <= H ? H : W, nl = (int)((double)size * longside / shortside);
    const int rw = W <= H ? size : nl, rh = W <= H ? nl : size, top = (rh - size) / 2, left = (rw - size) / 2;
    const Axis hx = make_axis(W, rw), vx = make_axis(H, rh);
    std::vector<float> out((size_t)2 * g * g * ld);
    std::vector<uint8_t> resized((size_t)2 * size * size * 3);
    for (int recipe = 0; recipe < 3; ++recipe) {
      std::vector<uint8_t> u8((size_t)2 * H * W * 3);
      std::vector<float> f32(u8.size());
      for (size_t i = 0; i < u8.size(); ++i) {
        u8[i] = recipe == 0 ? ((rnd() & 1) ? 255 : 0) : (uint8_t)rnd();
        f32[i] = recipe == 2 ? (float)((int)(rnd() % 2000) - 500) / 1000.0f : (u8[i] + 0.5f) / 255.0f;      // recipe 2: also outside [0, 1]
      }
      if (recipe == 2) f32[0] = NAN;
      for (int is_float = 0; is_float < 2; ++is_float) {
        for (auto& v : out) v = -1.0f;
        const int rc = ddpo_clip_preprocess_host(is_float ? (const void*)f32.data() : (const void*)u8.data(), is_float, 2, H, W, rh, rw, top, left, size,
                                                 patch, hx.coef.data(), hx.bounds.data(), hx.ksize, vx.coef.data(), vx.bounds.data(), vx.ksize,
                                                 norm.data(), out.data(), ld, resized.data());
        bool ok = rc == 0;
        for (size_t r = 0; ok && r < (size_t)2 * g * g; ++r)
          for (int c = 0; c < ld; ++c) {
            const float v = out[r * ld + c];
            if (c >= 588 ? v != 0.0f : !(v >= 0.0f && v < 768.0f)) ok = false;
          }
        if (!ok) std::printf("FAIL %dx%d -> %d recipe %d float %d (rc %d)\n", H, W, size, recipe, is_float, rc), ++failures;
      }
    }
    Axis bad = vx;                                                // a bound that points past the image must be refused, not followed
    bad.bounds[2 * top] = H;
    const std::vector<uint8_t> img((size_t)H * W * 3);
    if (ddpo_clip_preprocess_host(img.data(), 0, 1, H, W, rh, rw, top, left, size, patch, hx.coef.data(), hx.bounds.data(), hx.ksize, bad.coef.data(),
                                  bad.bounds.data(), bad.ksize, norm.data(), out.data(), ld, nullptr) != -1)
      std::printf("FAIL %dx%d: broken table accepted\n", H, W), ++failures;
  }
  std::printf("clip_preprocess_host_check: %d failures\n", failures);
  return failures ? 1 : 0;
}
