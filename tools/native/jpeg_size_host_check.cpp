// Stand-alone host check of the JPEG byte counter's arithmetic (ddpo_amd/csrc/jpeg_size_core.h): the serial path over the functions the kernels
// run, on the inputs that stress the bit buffer — a 0/255 checkerboard at quality 100 (largest coefficients, longest codes), uniform noise,
// alternating extremes per block, a constant image — over several sizes and every quality; and the float -> byte rule of csrc/image_u8.h on a
// strided sweep of every bit pattern, held to the convert-then-clamp expression wherever that is defined.  No GPU and no HIP compiler involved; meant to be built
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

// iu_float_to_u8 clamps before it converts.  The expression it replaced converted first, min(max((int)(x * 255.0f), 0), 255), which is defined
// only while |x * 255.0f| < 2^31: on every such x the two must agree, and the old expression is never evaluated on any other.
static int float_to_u8_failures() {
  int failures = 0;
  auto bits_of = [](float f) { uint32_t u; memcpy(&u, &f, 4); return u; };
  auto float_of = [](uint32_t u) { float f; memcpy(&f, &u, 4); return f; };
  auto check = [&](uint32_t u) {
    const float x = float_of(u), v = x * 255.0f;
    int want;
    if (v != v) want = 0;                                                   // NaN
    else if (v >= 2147483648.0f) want = 255;                                // +inf included
    else if (v <= -2147483648.0f) want = 0;                                 // -inf included
    else {
      const int c = (int)v;                                                 // defined: |v| < 2^31
      want = c < 0 ? 0 : (c > 255 ? 255 : c);
    }
    if (iu_float_to_u8(x) != want) {
      if (failures < 10) std::printf("FAIL float_to_u8(bits 0x%08x = %g): %d, expected %d\n", u, (double)x, iu_float_to_u8(x), want);
      ++failures;
    }
  };
  for (uint64_t u = 0; u <= 0xffffffffull; u += 251) check((uint32_t)u);    // a prime stride through every exponent and both signs
  for (int k = 0; k <= 255; ++k)                                            // the steps of the staircase: k / 255 and its neighbours
    for (int d = -1; d <= 1; ++d) check(bits_of((float)k / 255.0f) + (uint32_t)d), check((bits_of((float)k / 255.0f) + (uint32_t)d) | 0x80000000u);
  const float bound = 2147483648.0f / 255.0f;                               // |x * 255| reaches 2^31 about here
  for (int d = -4; d <= 4; ++d) check(bits_of(bound) + (uint32_t)d), check((bits_of(bound) + (uint32_t)d) | 0x80000000u);
  const uint32_t ends[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x007fffffu, 0x807fffffu, 0x00800000u, 0x80800000u,   // +-0, subnormals' ends
                           0x3f800000u, 0x3f800001u, 0x3f7fffffu, 0x7f7fffffu, 0xff7fffffu, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u};
  for (uint32_t u : ends) check(u);
  if (iu_float_to_u8(float_of(0x7fc00000u)) != 0 || iu_float_to_u8(float_of(0x7f800000u)) != 255 || iu_float_to_u8(float_of(0xff800000u)) != 0) {
    std::printf("FAIL float_to_u8: NaN -> 0, +inf -> 255, -inf -> 0 expected\n");
    ++failures;
  }
  return failures;
}

int main() {
  const int sizes[][2] = {{16, 16}, {16, 48}, {64, 64}, {128, 96}, {256, 256}};
  int failures = float_to_u8_failures();
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
