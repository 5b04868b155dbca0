// JPEG byte counting: the arithmetic of a baseline 4:2:0 libjpeg encode (standard Huffman tables, one scan, no restart markers), as
// host + device inline functions.  csrc/jpeg_size.hip runs them from kernels and from the serial host entry (ddpo_jpeg_size_host), so whether
// the count equals the encoder's is decided by the host entry against a real encoder (tests/test_jpeg_size_cpu.py) and the kernels only have
// to agree with the host entry.  The file itself (ddpo_jpeg_encode, ddpo_jpeg_encode_host) adds two functions at the end: the header bytes and the
// byte-stuffing step, held to the encoder's file the same way (tests/test_jpeg_encode_cpu.py).  Plain C++17: tools/native/jpeg_size_host_check.cpp
// and jpeg_encode_host_check.cpp include this file without a HIP compiler.
//
// Every step is integer and follows the encoder: 16-bit fixed-point RGB -> YCbCr, h2v2 chroma averaging with the alternating 1, 2 bias, level
// shift, the "islow" forward DCT (CONST_BITS 13, PASS1_BITS 2, output scaled by 8), quantisation sign(c) * floor((|c| + (d >> 1)) / d) with
// d = 8 * table entry, DC differences per component, run / size coded AC with ZRL and EOB, 0xFF byte stuffing, 1-padding of the last byte.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/ddpo_hip.h"
#include "image_u8.h"

#if defined(__HIPCC__)
#define JQ_HD __host__ __device__ inline
#else
#define JQ_HD inline
#endif

// Bytes of a file that are not entropy-coded data: SOI, APP0 (JFIF), 2 x DQT, SOF0, 4 x DHT (standard tables), SOS = 623, + EOI.
#define JQ_FIXED_BYTES DDPO_JPEG_FIXED_BYTES
// Upper bound of the bits one 8x8 block can emit.  DC: the longest standard DC code (11 bits, chroma category 11) + 11 value bits = 22.
// AC: charge every emitted symbol to coefficient positions it covers — a non-zero coefficient costs at most the longest AC code (16 bits) +
// 10 value bits = 26 at its own position, a ZRL (11 bits at most) covers 16 zero positions, an EOB (4 bits at most) at least one trailing zero —
// so no position is charged more than 26: 63 * 26 = 1638.  22 + 1638 = 1660, rounded up to whole 32-bit words.
#define JQ_MAX_BLOCK_BITS 1664

struct JqHuff {
  uint32_t e[256];      // (code length << 16) | code, indexed by symbol; 0 = symbol not in the table
};

constexpr JqHuff jq_make_huff(const uint8_t* bits /* [1..16] */, const uint8_t* vals, int nvals) {
  JqHuff h{};
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < bits[len] && k < nvals; ++i, ++k) h.e[vals[k]] = ((uint32_t)len << 16) | code++;
    code <<= 1;
  }
  return h;
}

// ISO/IEC 10918-1 Annex K.3 tables (what an encoder writes when it does not optimise its Huffman tables)
constexpr uint8_t kJqDcLumBits[17] = {0, 0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t kJqDcChrBits[17] = {0, 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t kJqDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kJqAcLumBits[17] = {0, 0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr uint8_t kJqAcLumVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};
constexpr uint8_t kJqAcChrBits[17] = {0, 0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr uint8_t kJqAcChrVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};

// [0] luminance, [1] chrominance.  Compile-time constants: no run-time initialisation and nothing a launch could write to.
constexpr JqHuff kJqDc[2] = {jq_make_huff(kJqDcLumBits, kJqDcVals, 12), jq_make_huff(kJqDcChrBits, kJqDcVals, 12)};
constexpr JqHuff kJqAc[2] = {jq_make_huff(kJqAcLumBits, kJqAcLumVals, 162), jq_make_huff(kJqAcChrBits, kJqAcChrVals, 162)};

// Annex K.1 / K.2 base quantisation tables, natural (row-major) order
constexpr uint8_t kJqBaseQ[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
     18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// zig-zag position -> natural index
constexpr uint8_t kJqNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ---------------------------------------------------------------------------------------------------------------- pixels
// float in [0, 1] -> uint8 the way the reward's reference does it, one fp32 multiply and truncation toward zero: iu_float_to_u8 of image_u8.h
JQ_HD void jq_rgb_to_ycc(int r, int g, int b, int& y, int& cb, int& cr) {
  y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// 2x2 chroma average of output column `out_col`: the bias alternates 1, 2, 1, 2, ... along a row
JQ_HD int jq_h2v2(int p00, int p01, int p10, int p11, int out_col) { return (p00 + p01 + p10 + p11 + 1 + (out_col & 1)) >> 2; }

// ---------------------------------------------------------------------------------------------------------------- quantisation table
// divisor of natural index i: 8 * clamp((base * scale + 50) / 100, 1, 255), scale = 5000 / q below 50 and 200 - 2 q from 50 up
JQ_HD int jq_divisor(int quality, int chroma, int i) {
  const int q = quality < 1 ? 1 : (quality > 100 ? 100 : quality);
  const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
  int v = ((int)kJqBaseQ[chroma][i] * scale + 50) / 100;
  v = v < 1 ? 1 : (v > 255 ? 255 : v);
  return v << 3;
}

JQ_HD int jq_quantize(int c, int d) { return c < 0 ? -((-c + (d >> 1)) / d) : (c + (d >> 1)) / d; }

// ---------------------------------------------------------------------------------------------------------------- forward DCT
// One 8-point pass of the "islow" DCT.  FIRST: row pass (outputs scaled up by 2^PASS1_BITS); otherwise the column pass (that scaling removed,
// the overall factor 8 kept).
template <bool FIRST>
JQ_HD void jq_fdct8(const int* in, int* out) {
  constexpr int CB = 13, P1 = 2;
  constexpr int S = FIRST ? CB - P1 : CB + P1;
  constexpr int R = 1 << (S - 1);
  const int tmp0 = in[0] + in[7], tmp7 = in[0] - in[7], tmp1 = in[1] + in[6], tmp6 = in[1] - in[6];
  const int tmp2 = in[2] + in[5], tmp5 = in[2] - in[5], tmp3 = in[3] + in[4], tmp4 = in[3] - in[4];
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  if (FIRST) {
    out[0] = (tmp10 + tmp11) * (1 << P1);
    out[4] = (tmp10 - tmp11) * (1 << P1);
  } else {
    out[0] = (tmp10 + tmp11 + (1 << (P1 - 1))) >> P1;
    out[4] = (tmp10 - tmp11 + (1 << (P1 - 1))) >> P1;
  }
  int z1 = (tmp12 + tmp13) * 4433;
  out[2] = (z1 + tmp13 * 6270 + R) >> S;
  out[6] = (z1 - tmp12 * 15137 + R) >> S;
  z1 = tmp4 + tmp7;
  int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int z5 = (z3 + z4) * 9633;
  const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  out[7] = (t4 + z1 + z3 + R) >> S;
  out[5] = (t5 + z2 + z4 + R) >> S;
  out[3] = (t6 + z2 + z3 + R) >> S;
  out[1] = (t7 + z1 + z4 + R) >> S;
}

// ---------------------------------------------------------------------------------------------------------------- block order
// Blocks of an image are numbered in scan order: 6 per 16x16 MCU (Y00 Y01 Y10 Y11 Cb Cr), MCUs in raster order.  Index of the previous block of
// the same component (the DC predictor), or -1 for the first one.
JQ_HD int64_t jq_prev_block(int64_t blk) {
  const int j = (int)(blk % 6);
  if (j >= 1 && j <= 3) return blk - 1;
  if (blk < 6) return -1;
  return j == 0 ? blk - 3 : blk - 6;
}

// ---------------------------------------------------------------------------------------------------------------- entropy coder
JQ_HD int jq_nbits(int v) {
  const unsigned a = v < 0 ? (unsigned)(-v) : (unsigned)v;
  return a ? 32 - __builtin_clz(a) : 0;
}
// code of `sym` followed by the nbits-bit value field of v (negative values: the low bits of v - 1): `len` bits, right-aligned in `bits`
JQ_HD void jq_symbol(const JqHuff& h, int sym, int v, int nbits, uint32_t& bits, int& len) {
  const uint32_t e = h.e[sym & 255];
  const uint32_t val = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << nbits) - 1u);
  bits = ((e & 0xffffu) << nbits) | val;
  len = (int)(e >> 16) + nbits;
}

struct JqBitCounter {
  uint32_t bits = 0;
  JQ_HD void put(uint32_t, int len) { bits += (uint32_t)len; }
};

// Writes into a ZEROED big-endian bit buffer of 32-bit words: stream bit p is bit 31 - (p & 31) of word p >> 5, i.e. stream byte k is
// (word[k >> 2] >> (24 - 8 * (k & 3))) & 0xff.  Words are OR-ed in (atomically on the device: neighbouring blocks share their boundary words,
// and OR does not depend on the order), never beyond `nwords`.
struct JqBitWriter {
  uint32_t* words;
  uint64_t nwords, w;
  uint64_t acc;
  int nacc;
  JQ_HD JqBitWriter(uint32_t* words_, uint64_t nwords_, uint64_t bit_offset)
      : words(words_), nwords(nwords_), w(bit_offset >> 5), acc(0), nacc((int)(bit_offset & 31)) {}
  JQ_HD void store(uint32_t v) {
    if (w < nwords && v) {
#if defined(__HIP_DEVICE_COMPILE__)
      atomicOr(words + w, v);
#else
      words[w] |= v;
#endif
    }
    ++w;
  }
  JQ_HD void put(uint32_t bits, int len) {      // len <= 27
    acc = (acc << len) | bits;
    nacc += len;
    if (nacc >= 32) {
      nacc -= 32;
      store((uint32_t)(acc >> nacc));
      acc &= (1ull << nacc) - 1ull;
    }
  }
  JQ_HD void flush() {
    if (nacc > 0) store((uint32_t)(acc << (32 - nacc)));
    nacc = 0;
    acc = 0;
  }
};

template <class Sink>
JQ_HD void jq_encode_dc(int diff, int chroma, Sink& s) {
  uint32_t bits;
  int len;
  const int n = jq_nbits(diff);
  jq_symbol(kJqDc[chroma], n, diff, n, bits, len);
  s.put(bits, len);
}

// the 63 AC coefficients of a block given in zig-zag order (zz[0] is the DC and is not read)
template <class Sink>
JQ_HD void jq_encode_ac(const int16_t* zz, int chroma, Sink& s) {
  const JqHuff& h = kJqAc[chroma];
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = zz[k];
    if (v == 0) {
      ++run;
      continue;
    }
    while (run > 15) {
      s.put(h.e[0xf0] & 0xffffu, (int)(h.e[0xf0] >> 16));      // ZRL
      run -= 16;
    }
    uint32_t bits;
    int len;
    const int n = jq_nbits(v);
    jq_symbol(h, (run << 4) + n, v, n, bits, len);
    s.put(bits, len);
    run = 0;
  }
  if (run > 0) s.put(h.e[0] & 0xffffu, (int)(h.e[0] >> 16));    // EOB
}

// 0xFF bytes among the stream bytes held by word `wi` of a bit buffer that holds `total_bits` bits; the last byte's unused low bits count as 1s
JQ_HD int jq_count_ff(uint32_t word, uint64_t wi, uint64_t total_bits) {
  const uint64_t nbytes = (total_bits + 7) >> 3;
  int c = 0;
  for (int k = 0; k < 4; ++k) {
    const uint64_t b = wi * 4 + k;
    if (b >= nbytes) break;
    uint32_t byte = (word >> (24 - 8 * k)) & 0xffu;
    if (b == nbytes - 1 && (total_bits & 7)) byte |= (1u << (8 - (int)(total_bits & 7))) - 1u;
    c += byte == 0xffu;
  }
  return c;
}

JQ_HD int64_t jq_file_bytes(uint64_t total_bits, uint64_t ff_bytes) { return (int64_t)JQ_FIXED_BYTES + (int64_t)((total_bits + 7) >> 3) + (int64_t)ff_bytes; }

// words of the bit buffer of one image of `nblk` blocks (+1: the writer's flush may touch the word after the last full one)
JQ_HD uint64_t jq_bitbuf_words(uint64_t nblk) { return nblk * (JQ_MAX_BLOCK_BITS / 32) + 1; }

// ---------------------------------------------------------------------------------------------------------------- the file
// Byte i (0 .. JQ_HEADER_BYTES - 1) of everything the encoder writes before the scan data of an H x W image at `quality`:
//   SOI | APP0 (JFIF 1.01, no units, density 1 x 1) | DQT 0 | DQT 1 | SOF0 | DHT DC0 | DHT AC0 | DHT DC1 | DHT AC1 | SOS
// A function of the position and nothing else: no table is built at run time, on either side.
#define JQ_HEADER_BYTES DDPO_JPEG_HEADER_BYTES
static_assert(JQ_HEADER_BYTES + 2 == JQ_FIXED_BYTES, "header + EOI");
constexpr uint8_t kJqApp0[18] = {0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
constexpr uint8_t kJqSofTail[10] = {3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1};            // 3 components: id, sampling, quantisation table
constexpr uint8_t kJqSos[14] = {0xff, 0xda, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};

JQ_HD uint8_t jq_dht_byte(int i, int cls_id, const uint8_t* bits, const uint8_t* vals, int nvals) {
  if (i < 5) return i == 0 ? 0xff : i == 1 ? 0xc4 : i == 2 ? 0 : i == 3 ? (uint8_t)(19 + nvals) : (uint8_t)cls_id;
  return i < 21 ? bits[i - 4] : vals[i - 21];                     // bits[1..16], then the symbols
}

JQ_HD uint8_t jq_header_byte(int i, int H, int W, int quality) {
  if (i < 2) return i == 0 ? 0xff : 0xd8;
  if ((i -= 2) < 18) return kJqApp0[i];
  if ((i -= 18) < 2 * 69) {
    const int c = i / 69, k = i % 69;
    if (k < 5) return k == 0 ? 0xff : k == 1 ? 0xdb : k == 2 ? 0 : k == 3 ? 67 : (uint8_t)c;
    return (uint8_t)(jq_divisor(quality, c, kJqNatural[k - 5]) >> 3);
  }
  if ((i -= 2 * 69) < 19) {
    if (i < 5) return i == 0 ? 0xff : i == 1 ? 0xc0 : i == 2 ? 0 : i == 3 ? 17 : 8;
    if (i < 9) return (uint8_t)((i < 7 ? H : W) >> ((i & 1) ? 8 : 0));      // i = 5, 6: H high, low; 7, 8: W high, low
    return kJqSofTail[i - 9];
  }
  if ((i -= 19) < 33) return jq_dht_byte(i, 0x00, kJqDcLumBits, kJqDcVals, 12);
  if ((i -= 33) < 183) return jq_dht_byte(i, 0x10, kJqAcLumBits, kJqAcLumVals, 162);
  if ((i -= 183) < 33) return jq_dht_byte(i, 0x01, kJqDcChrBits, kJqDcVals, 12);
  if ((i -= 33) < 183) return jq_dht_byte(i, 0x11, kJqAcChrBits, kJqAcChrVals, 162);
  return kJqSos[i - 183];
}

// The file bytes that word `wi` of a bit buffer holding `total_bits` bits contributes, given the 0xFF bytes among the stream bytes before it:
// its stream bytes in order, each 0xFF followed by a 0x00, the last byte of the stream padded with 1-bits first (jq_count_ff's convention, so a
// padded byte that becomes 0xFF is stuffed too).  Returns how many (0 for a word past the end of the stream, at most 8) and sets the offset in
// the file at which they go.
JQ_HD int jq_stuff_word(uint32_t word, uint64_t wi, uint64_t total_bits, uint64_t ff_before, uint8_t out[8], uint64_t& offset) {
  const uint64_t nbytes = (total_bits + 7) >> 3;
  offset = (uint64_t)JQ_HEADER_BYTES + wi * 4 + ff_before;
  int n = 0;
  for (int k = 0; k < 4; ++k) {
    const uint64_t b = wi * 4 + k;
    if (b >= nbytes) break;
    uint32_t byte = (word >> (24 - 8 * k)) & 0xffu;
    if (b == nbytes - 1 && (total_bits & 7)) byte |= (1u << (8 - (int)(total_bits & 7))) - 1u;
    out[n++] = (uint8_t)byte;
    if (byte == 0xffu) out[n++] = 0;
  }
  return n;
}

// upper bound of one file: header, EOI, and the longest scan with every byte stuffed
JQ_HD uint64_t jq_file_max_bytes(uint64_t nblk) { return (uint64_t)JQ_FIXED_BYTES + 2 * ((nblk * JQ_MAX_BLOCK_BITS + 7) >> 3); }

// Quantised coefficients (zig-zag order) of block j (0..5) of the MCU whose 16x16 pixels start at `rgb` (row stride `stride` bytes, 3 bytes / pixel).
inline void jq_host_mcu_block(const uint8_t* rgb, size_t stride, int j, int quality, int16_t* zz) {
  int data[64], tmp[8], col[8];
  if (j < 4) {
    const uint8_t* p = rgb + (size_t)(j >> 1) * 8 * stride + (size_t)(j & 1) * 8 * 3;
    for (int r = 0; r < 8; ++r)
      for (int c = 0; c < 8; ++c) {
        int y, cb, cr;
        jq_rgb_to_ycc(p[r * stride + c * 3], p[r * stride + c * 3 + 1], p[r * stride + c * 3 + 2], y, cb, cr);
        data[r * 8 + c] = y - 128;
      }
  } else {
    for (int r = 0; r < 8; ++r)
      for (int c = 0; c < 8; ++c) {
        int s[4];
        for (int q = 0; q < 4; ++q) {
          const uint8_t* p = rgb + (size_t)(2 * r + (q >> 1)) * stride + (size_t)(2 * c + (q & 1)) * 3;
          int y, cb, cr;
          jq_rgb_to_ycc(p[0], p[1], p[2], y, cb, cr);
          s[q] = j == 4 ? cb : cr;
        }
        data[r * 8 + c] = jq_h2v2(s[0], s[1], s[2], s[3], c) - 128;
      }
  }
  for (int r = 0; r < 8; ++r) {
    jq_fdct8<true>(data + r * 8, tmp);
    memcpy(data + r * 8, tmp, sizeof(tmp));
  }
  for (int c = 0; c < 8; ++c) {
    for (int r = 0; r < 8; ++r) col[r] = data[r * 8 + c];
    jq_fdct8<false>(col, tmp);
    for (int r = 0; r < 8; ++r) data[r * 8 + c] = jq_quantize(tmp[r], jq_divisor(quality, j >= 4, r * 8 + c));
  }
  for (int k = 0; k < 64; ++k) zz[k] = (int16_t)data[kJqNatural[k]];
}

// Serial reference over the functions above: the bit buffer of one H x W RGB image (H, W multiples of 16) into `buf`; returns the bits it holds.
inline uint64_t jq_host_image_stream(const uint8_t* rgb, int H, int W, int quality, std::vector<uint32_t>& buf) {
  const int mw = W / 16, mh = H / 16;
  const uint64_t nblk = (uint64_t)mw * mh * 6, nwords = jq_bitbuf_words(nblk);
  buf.assign(nwords, 0u);
  std::vector<int16_t> dc(nblk, 0);
  uint64_t pos = 0;
  int16_t zz[64];
  for (uint64_t blk = 0; blk < nblk; ++blk) {
    const uint64_t mcu = blk / 6;
    const int j = (int)(blk % 6);
    jq_host_mcu_block(rgb + ((size_t)(mcu / mw) * 16 * W + (size_t)(mcu % mw) * 16) * 3, (size_t)W * 3, j, quality, zz);
    dc[blk] = zz[0];
    const int64_t prev = jq_prev_block((int64_t)blk);
    const int diff = (int)zz[0] - (prev < 0 ? 0 : (int)dc[prev]);
    JqBitCounter cnt;
    jq_encode_dc(diff, j >= 4, cnt);
    jq_encode_ac(zz, j >= 4, cnt);
    JqBitWriter wr(buf.data(), nwords, pos);
    jq_encode_dc(diff, j >= 4, wr);
    jq_encode_ac(zz, j >= 4, wr);
    wr.flush();
    pos += cnt.bits;
  }
  return pos;
}

// File size of one image.  `total_bits_out`, `ff_out`: optional.
inline int64_t jq_host_image_bytes(const uint8_t* rgb, int H, int W, int quality, uint64_t* total_bits_out = nullptr, uint64_t* ff_out = nullptr) {
  std::vector<uint32_t> buf;
  const uint64_t pos = jq_host_image_stream(rgb, H, W, quality, buf);
  uint64_t ff = 0;
  for (uint64_t wi = 0; wi * 32 < pos; ++wi) ff += (uint64_t)jq_count_ff(buf[wi], wi, pos);
  if (total_bits_out) *total_bits_out = pos;
  if (ff_out) *ff_out = ff;
  return jq_file_bytes(pos, ff);
}

// The file of one image into `row`, of which at most `stride` bytes are written: a longer file leaves its first `stride` bytes.  Returns the
// file's full length either way; bytes of the row past min(length, stride) are not touched.
inline int64_t jq_host_image_file(const uint8_t* rgb, int H, int W, int quality, uint8_t* row, size_t stride) {
  std::vector<uint32_t> buf;
  const uint64_t pos = jq_host_image_stream(rgb, H, W, quality, buf);
  for (uint64_t i = 0; i < JQ_HEADER_BYTES && i < stride; ++i) row[i] = jq_header_byte((int)i, H, W, quality);
  uint64_t ff = 0;
  for (uint64_t wi = 0; wi * 32 < pos; ++wi) {
    uint8_t out[8];
    uint64_t at;
    const int n = jq_stuff_word(buf[wi], wi, pos, ff, out, at);
    for (int k = 0; k < n; ++k)
      if (at + k < stride) row[at + k] = out[k];
    ff += (uint64_t)jq_count_ff(buf[wi], wi, pos);
  }
  const uint64_t eoi = (uint64_t)JQ_HEADER_BYTES + ((pos + 7) >> 3) + ff;
  if (eoi < stride) row[eoi] = 0xff;
  if (eoi + 1 < stride) row[eoi + 1] = 0xd9;
  return jq_file_bytes(pos, ff);
}
