// Stand-alone host check of the JPEG byte counter's arithmetic (ddpo_amd/csrc/jpeg_size_core.h): the serial path over the functions the kernels
// run, on the inputs that stress the bit buffer — a 0/255 checkerboard at quality 100 (largest coefficients, longest codes), uniform noise,
// alternating extremes per block, a constant image — over several sizes and every quality.  No GPU and no HIP compiler involved; meant to be built
// with a host sanitizer:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/native/jpeg_size_host_check.cpp -o jpeg_size_host_check
// Exits non-zero if a count is implausible or the bit count ever exceeds the per-block bound the device workspace is sized from.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ddpo_amd/csrc/jpeg_size_core.h"

static uint32_t rng_state = 12345u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

int main() {
  const int sizes[][2] = {{16, 16}, {16, 48}, {64, 64}, {128, 96}, {256, 256}};
  int failures = 0;
  for (const auto& hw : sizes) {
    const int H = hw[0], W = hw[1];
    std::vector<uint8_t> img((size_t)H * W * 3);
    for (int recipe = 0; recipe < 4; ++recipe) {
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
          for (int c = 0; c < 3; ++c) {
            uint8_t v;
            if (recipe == 0) v = ((x + y) & 1) ? 255 : 0;
            else if (recipe == 1) v = (uint8_t)rnd();
            else if (recipe == 2) v = (rnd() & 1) ? 255 : 0;             // binary noise: every coefficient large
            else v = 200;
            img[((size_t)y * W + x) * 3 + c] = v;
          }
      for (int q = 1; q <= 100; q += (H >= 128 ? 33 : 1)) {
        uint64_t bits = 0, ff = 0;
        const int64_t n = jq_host_image_bytes(img.data(), H, W, q, &bits, &ff);
        const uint64_t nblk = (uint64_t)(H / 16) * (W / 16) * 6;
        if (n < JQ_FIXED_BYTES + 1 || bits > nblk * JQ_MAX_BLOCK_BITS || ff > (bits + 7) / 8) {
          std::printf("FAIL %dx%d recipe %d q %d: %lld bytes, %llu bits, %llu stuffed\n", H, W, recipe, q, (long long)n, (unsigned long long)bits,
                      (unsigned long long)ff);
          ++failures;
        }
      }
    }
  }
  std::printf("jpeg_size_host_check: %d failures\n", failures);
  return failures ? 1 : 0;
}
