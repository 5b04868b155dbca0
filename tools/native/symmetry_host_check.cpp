// Stand-alone host check of the symmetry arithmetic (ddpo_amd/csrc/symmetry_core.h through the serial entries ddpo_symmetry_stats_host and
// ddpo_rotate4_u8_host of csrc/symmetry.hip, which this file includes): all-255 images — the largest sums, past 32 bits — noise and
// out-of-range / NaN floats over 1 x 1, odd, non-square and wide sizes, against sums and turns restated here in 64-bit integers.  Nothing runs on a
// GPU; meant to be built with a host sanitizer (make -C tools/native symmetry_host_check):
//   hipcc --offload-arch=gfx950 -x hip -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all ...
// Exits non-zero if an entry refuses a valid case, accepts a bad one, or disagrees with the restatement.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../ddpo_amd/csrc/symmetry.hip"

static uint32_t rng_state = 12345u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

static int to_byte(float x) {
  const float v = x * 255.0f;
  if (!(v >= 0.0f)) return 0;
  return v >= 255.0f ? 255 : (int)v;
}

int main() {
  const int cases[][3] = {{1, 1, 1}, {2, 3, 5}, {2, 24, 40}, {1, 7, 520}, {1, 160, 152}, {1, 2, 10880}, {3, 72, 72}};
  int failures = 0;
  for (const auto& cs : cases) {
    const int N = cs[0], H = cs[1], W = cs[2];
    const size_t per = (size_t)H * W * 3;
    for (int recipe = 0; recipe < 3; ++recipe) {
      std::vector<uint8_t> u8(N * per);
      std::vector<float> f32(u8.size());
      for (size_t i = 0; i < u8.size(); ++i) {
        u8[i] = recipe == 0 ? 255 : (uint8_t)rnd();
        f32[i] = recipe == 2 ? (float)((int)(rnd() % 2000) - 500) / 1000.0f : (u8[i] + 0.5f) / 255.0f;      // recipe 2: also outside [0, 1]
      }
      if (recipe == 2) f32[0] = NAN;
      for (int is_float = 0; is_float < 2; ++is_float) {
        std::vector<uint8_t> b(u8.size());
        for (size_t i = 0; i < b.size(); ++i) b[i] = is_float ? (uint8_t)to_byte(f32[i]) : u8[i];
        const void* src = is_float ? (const void*)f32.data() : (const void*)u8.data();
        for (int mode = 0; mode < 2; ++mode) {
          std::vector<int64_t> got((size_t)N * 4, -1);
          bool ok = ddpo_symmetry_stats_host(src, is_float, N, H, W, mode, got.data()) == 0;
          for (int n = 0; ok && n < N; ++n) {
            int64_t want[4] = {0, 0, 0, 0};
            for (int y = 0; y < H; ++y)
              for (int x = 0; x < W; ++x)
                for (int c = 0; c < 3; ++c) {
                  const int64_t a = b[n * per + ((size_t)y * W + x) * 3 + c];
                  const int64_t p = b[n * per + ((size_t)(mode ? H - 1 - y : y) * W + (W - 1 - x)) * 3 + c];
                  const int64_t d = ((a - p) % 256 + 256) % 256;
                  want[0] += (d * d) % 256, want[1] += a, want[2] += a * a, want[3] += a * p;
                }
            for (int k = 0; k < 4; ++k) ok = ok && got[(size_t)n * 4 + k] == want[k];
          }
          if (!ok) std::printf("FAIL stats %dx%dx%d recipe %d float %d mode %d\n", N, H, W, recipe, is_float, mode), ++failures;
        }
        std::vector<uint8_t> turned(4 * b.size(), 0xAB);
        const int rc = ddpo_rotate4_u8_host(src, is_float, N, H, W, turned.data());
        if (H != W) {
          if (rc != -1) std::printf("FAIL rotate4 %dx%d accepted\n", H, W), ++failures;
          continue;
        }
        bool ok = rc == 0;
        const int S = H;
        for (int n = 0; ok && n < N; ++n)
          for (int y = 0; y < S; ++y)
            for (int x = 0; x < S; ++x)
              for (int c = 0; c < 3; ++c) {
                const uint8_t v = b[n * per + ((size_t)y * S + x) * 3 + c];
                const int dst[4][2] = {{y, x}, {S - 1 - x, y}, {S - 1 - y, S - 1 - x}, {x, S - 1 - y}};      // where (y, x) lands after k quarter turns
                for (int k = 0; k < 4; ++k) ok = ok && turned[((size_t)k * N + n) * per + ((size_t)dst[k][0] * S + dst[k][1]) * 3 + c] == v;
              }
        if (!ok) std::printf("FAIL rotate4 %dx%dx%d recipe %d float %d (rc %d)\n", N, S, S, recipe, is_float, rc), ++failures;
      }
    }
  }
  const std::vector<uint8_t> img((size_t)10881 * 3);
  int64_t out[4];
  if (ddpo_symmetry_stats_host(img.data(), 0, 1, 1, 10881, 0, out) != -1) std::printf("FAIL: a row wider than SY_MAX_W accepted\n"), ++failures;
  if (ddpo_symmetry_stats_host(img.data(), 0, 1, 1, 8, 2, out) != -1) std::printf("FAIL: mode 2 accepted\n"), ++failures;
  std::printf("symmetry_host_check: %d failures\n", failures);
  return failures ? 1 : 0;
}
