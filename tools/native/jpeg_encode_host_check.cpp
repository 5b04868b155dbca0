// Stand-alone host check of the JPEG file writer's arithmetic (ddpo_amd/csrc/jpeg_size_core.h): the header bytes and the byte-stuffing step the
// pack kernel runs, through the serial path (jq_host_image_file), on inputs that need no real encoder to judge — a 0/255 checkerboard, uniform
// noise, binary noise, a constant image — over several sizes and qualities.  Checked: the header walks as SOI, APP0, 2 x DQT, SOF0, 4 x DHT, SOS
// with the lengths the format prescribes and ends at byte 623; the scan data un-stuffs to the bit buffer's bytes, padded with 1-bits; EOI closes
// the file; the length is the byte counter's; and rows with canary bytes around them, at strides equal to the length, one below it and 625, hold
// the file's prefix and nothing else.  No GPU and no HIP compiler involved; meant to be built with a host sanitizer:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/native/jpeg_encode_host_check.cpp -o jpeg_encode_host_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ddpo_amd/csrc/jpeg_size_core.h"

static uint32_t rng_state = 12345u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

static int failures = 0;
#define EXPECT(cond, ...)            \
  do {                               \
    if (!(cond)) {                   \
      std::printf("FAIL " __VA_ARGS__); \
      std::printf("\n");             \
      ++failures;                    \
    }                                \
  } while (0)

static void check_header(const uint8_t* f, int H, int W, int q) {
  static const int markers[9] = {0xe0, 0xdb, 0xdb, 0xc0, 0xc4, 0xc4, 0xc4, 0xc4, 0xda};
  static const int lengths[9] = {16, 67, 67, 17, 31, 181, 31, 181, 12};
  EXPECT(f[0] == 0xff && f[1] == 0xd8, "%dx%d q%d: SOI", H, W, q);
  size_t pos = 2;
  for (int s = 0; s < 9; ++s) {
    EXPECT(f[pos] == 0xff && f[pos + 1] == markers[s] && ((f[pos + 2] << 8) | f[pos + 3]) == lengths[s], "%dx%d q%d: segment %d", H, W, q, s);
    if (markers[s] == 0xdb)
      for (int k = 0; k < 64; ++k) EXPECT(f[pos + 5 + k] >= 1, "%dx%d q%d: zero quantiser", H, W, q);
    if (markers[s] == 0xc0)
      EXPECT(((f[pos + 5] << 8) | f[pos + 6]) == H && ((f[pos + 7] << 8) | f[pos + 8]) == W, "%dx%d q%d: SOF0 size", H, W, q);
    if (markers[s] == 0xc4) {
      int nsym = 0;
      for (int k = 0; k < 16; ++k) nsym += f[pos + 5 + k];
      EXPECT(nsym + 19 == lengths[s], "%dx%d q%d: DHT %d counts", H, W, q, s);
    }
    pos += 2 + (size_t)lengths[s];
  }
  EXPECT(pos == JQ_HEADER_BYTES, "%dx%d q%d: header ends at %zu", H, W, q, pos);
}

int main() {
  const int sizes[][2] = {{16, 16}, {16, 48}, {64, 64}, {128, 96}};
  const size_t CANARY = 64;
  int files = 0, padded_ff = 0, whole_bytes = 0;
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
            else if (recipe == 2) v = (rnd() & 1) ? 255 : 0;
            else v = 200;
            img[((size_t)y * W + x) * 3 + c] = v;
          }
      for (int q = 1; q <= 100; q += (H >= 64 ? 11 : 1)) {
        uint64_t bits = 0, ff = 0;
        const int64_t len = jq_host_image_bytes(img.data(), H, W, q, &bits, &ff);
        const uint64_t nblk = (uint64_t)(H / 16) * (W / 16) * 6;
        EXPECT((uint64_t)len <= jq_file_max_bytes(nblk), "%dx%d r%d q%d: %lld bytes above the bound", H, W, recipe, q, (long long)len);
        std::vector<uint8_t> whole((size_t)len);
        EXPECT(jq_host_image_file(img.data(), H, W, q, whole.data(), whole.size()) == len, "%dx%d r%d q%d: length", H, W, recipe, q);
        check_header(whole.data(), H, W, q);
        EXPECT(whole[len - 2] == 0xff && whole[len - 1] == 0xd9, "%dx%d r%d q%d: EOI", H, W, recipe, q);
        // un-stuff the scan data and hold it to the bit buffer
        std::vector<uint32_t> buf;
        EXPECT(jq_host_image_stream(img.data(), H, W, q, buf) == bits, "%dx%d r%d q%d: bits", H, W, recipe, q);
        const uint64_t nbytes = (bits + 7) / 8;
        size_t p = JQ_HEADER_BYTES;
        uint64_t seen_ff = 0;
        for (uint64_t b = 0; b < nbytes; ++b) {
          uint32_t want = (buf[b >> 2] >> (24 - 8 * (b & 3))) & 0xffu;
          if (b == nbytes - 1 && (bits & 7)) want |= (1u << (8 - (bits & 7))) - 1u;
          EXPECT(p < (size_t)len - 2 && whole[p] == want, "%dx%d r%d q%d: stream byte %llu", H, W, recipe, q, (unsigned long long)b);
          ++p;
          if (want == 0xff) {
            EXPECT(p < (size_t)len - 2 && whole[p] == 0, "%dx%d r%d q%d: byte %llu not stuffed", H, W, recipe, q, (unsigned long long)b);
            ++p, ++seen_ff;
            if (b == nbytes - 1) ++padded_ff;
          }
        }
        EXPECT(p == (size_t)len - 2 && seen_ff == ff, "%dx%d r%d q%d: scan ends at %zu of %lld", H, W, recipe, q, p, (long long)len);
        whole_bytes += (bits & 7) == 0;
        // rows of exactly `stride` bytes, each an allocation of its own: the sanitizer sees any write past one
        const size_t strides[3] = {(size_t)len, (size_t)len - 1, (size_t)JQ_FIXED_BYTES};
        for (size_t stride : strides) {
          std::vector<uint8_t> row(stride, 0xa5);
          EXPECT(jq_host_image_file(img.data(), H, W, q, row.data(), stride) == len, "%dx%d r%d q%d stride %zu: length", H, W, recipe, q, stride);
          EXPECT(memcmp(row.data(), whole.data(), stride) == 0, "%dx%d r%d q%d stride %zu: not the prefix", H, W, recipe, q, stride);
        }
        // a longer row: the tail beyond the file keeps its canary
        std::vector<uint8_t> wide((size_t)len + CANARY, 0xa5);
        jq_host_image_file(img.data(), H, W, q, wide.data(), wide.size());
        for (size_t i = (size_t)len; i < wide.size(); ++i) EXPECT(wide[i] == 0xa5, "%dx%d r%d q%d: byte %zu past the file written", H, W, recipe, q, i);
        EXPECT(memcmp(wide.data(), whole.data(), (size_t)len) == 0, "%dx%d r%d q%d: wide row", H, W, recipe, q);
        ++files;
      }
    }
  }
  // the stuffing step alone, on words chosen by hand
  {
    uint8_t out[8];
    uint64_t at;
    EXPECT(jq_stuff_word(0x12ffffffu, 2, 96, 5, out, at) == 7 && at == JQ_HEADER_BYTES + 8 + 5 && out[0] == 0x12 && out[1] == 0xff && out[2] == 0 &&
               out[5] == 0xff && out[6] == 0, "stuff: three 0xFF bytes");
    EXPECT(jq_stuff_word(0xabfe0000u, 0, 15, 0, out, at) == 3 && out[0] == 0xab && out[1] == 0xff && out[2] == 0, "stuff: padded byte becomes 0xFF");
    EXPECT(jq_stuff_word(0xabfe0000u, 0, 16, 0, out, at) == 2 && out[1] == 0xfe, "stuff: whole bytes are not padded");
    EXPECT(jq_stuff_word(0xffffffffu, 3, 96, 0, out, at) == 0, "stuff: a word past the end");
    EXPECT(jq_stuff_word(0x80000000u, 1, 33, 0, out, at) == 2 && out[0] == 0xff && out[1] == 0, "stuff: one bit, seven 1-bits of padding");
  }
  std::printf("jpeg_encode_host_check: %d files (%d end in a stuffed padded byte, %d with whole-byte streams), %d failures\n", files, padded_ff,
              whole_bytes, failures);
  return failures ? 1 : 0;
}
