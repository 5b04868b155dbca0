// JPEG file size of RGB images without producing the file (the jpeg_device / neg_jpeg_device rewards): the byte count a baseline 4:2:0 libjpeg
// encode at the given quality would have.  The arithmetic is csrc/jpeg_size_core.h, shared with the serial host entry at the bottom.
//
// Launch sequence (all on the caller's stream, all state in the caller's workspace):
//   memset            the bit buffers (emission ORs into them)
//   jq_transform      per group of <= 4 MCUs of one MCU row: pixels -> uint8 -> YCbCr -> 2x2 chroma average -> 8x8 DCTs through LDS (8 lanes per
//                     block: a row pass, a column pass) -> quantise -> zig-zag int16 coefficients to the workspace + each block's AC bit count
//   jq_scan           one workgroup per image: block length = AC bits + bits of the DC difference (previous block of the component, read from
//                     the stored coefficients), exclusive scan in scan order -> each block's bit offset, the image's total
//   jq_emit           one lane per block: its codes OR-ed into the image's big-endian bit buffer at its offset
//   jq_count          one workgroup per image: 0xFF bytes of the padded stream -> fixed bytes + ceil(bits / 8) + stuffed bytes, int64
// ddpo_jpeg_encode produces the file as well: the same sequence with jq_pack in the place of jq_count.
//   jq_pack           one workgroup per image: header, the stream's bytes with a 0x00 after every 0xFF (an exclusive scan of the 0xFF counts gives
//                     each word its place; a pass's bytes are staged in LDS and stored 16 aligned bytes at a time), EOI, and the same length
#include "common.h"
#include "jpeg_size_core.h"

namespace {

constexpr int MCUS = 4;               // MCUs per workgroup of jq_transform
constexpr int TB = 256;
constexpr int SCAN_TB = 1024;

struct JqLayout {
  size_t coef, acbits, offs, total, bitbuf, words_per_image, bytes;
};

// false: sizes this path does not take (see the header) or whose bit offsets would not fit 32 bits
bool jq_layout(int N, int H, int W, JqLayout& l) {
  if (N <= 0 || H <= 0 || W <= 0 || (H & 15) || (W & 15)) return false;
  const uint64_t nblk = (uint64_t)(H / 16) * (uint64_t)(W / 16) * 6;
  if (nblk * JQ_MAX_BLOCK_BITS >= (1ull << 32) || nblk * (uint64_t)N >= (1ull << 31)) return false;
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t nb = (size_t)nblk * N;
  l.words_per_image = (size_t)jq_bitbuf_words(nblk);
  l.coef = 0;
  l.acbits = up(l.coef + nb * 64 * sizeof(int16_t));
  l.offs = up(l.acbits + nb * sizeof(uint32_t));
  l.total = up(l.offs + nb * sizeof(uint32_t));
  l.bitbuf = up(l.total + (size_t)N * sizeof(uint32_t));
  l.bytes = up(l.bitbuf + l.words_per_image * N * sizeof(uint32_t));
  return true;
}

template <bool F32>
__global__ __launch_bounds__(TB) void jq_transform(const void* __restrict__ images, int H, int W, int quality, int16_t* __restrict__ coef,
                                                   uint32_t* __restrict__ acbits) {
  __shared__ uint8_t s_pix[3][16][MCUS * 16];        // Y, Cb, Cr at full resolution
  __shared__ uint8_t s_sub[2][8][MCUS * 8];          // Cb, Cr after the 2x2 average
  __shared__ int s_dct[MCUS * 6][64];
  __shared__ int16_t s_zz[MCUS * 6][64];
  __shared__ uint16_t s_div[2][64];
  const int t = threadIdx.x;
  const int mw = W / 16, groups = (mw + MCUS - 1) / MCUS;
  const int n = blockIdx.x / ((H / 16) * groups), rem = blockIdx.x % ((H / 16) * groups);
  const int my = rem / groups, mx0 = (rem % groups) * MCUS;
  const int nm = min(MCUS, mw - mx0), nb = nm * 6, pw = nm * 16;

  if (t < 128) s_div[t >> 6][t & 63] = (uint16_t)jq_divisor(quality, t >> 6, t & 63);
  const size_t row0 = ((size_t)n * H + (size_t)my * 16) * W + (size_t)mx0 * 16;        // pixel index of the group's top-left corner
  for (int i = t; i < 16 * pw; i += TB) {
    const int r = i / pw, c = i % pw;
    const size_t p = (row0 + (size_t)r * W + c) * 3;
    int R, G, B;
    if (F32) {
      const float* f = static_cast<const float*>(images) + p;
      R = iu_float_to_u8(f[0]), G = iu_float_to_u8(f[1]), B = iu_float_to_u8(f[2]);
    } else {
      const uint8_t* u = static_cast<const uint8_t*>(images) + p;
      R = u[0], G = u[1], B = u[2];
    }
    int y, cb, cr;
    jq_rgb_to_ycc(R, G, B, y, cb, cr);
    s_pix[0][r][c] = (uint8_t)y, s_pix[1][r][c] = (uint8_t)cb, s_pix[2][r][c] = (uint8_t)cr;
  }
  __syncthreads();
  for (int i = t; i < 2 * 8 * (pw / 2); i += TB) {
    const int comp = i / (8 * (pw / 2)), r = (i / (pw / 2)) % 8, c = i % (pw / 2);
    const uint8_t(*s)[MCUS * 16] = s_pix[1 + comp];
    s_sub[comp][r][c] = (uint8_t)jq_h2v2(s[2 * r][2 * c], s[2 * r][2 * c + 1], s[2 * r + 1][2 * c], s[2 * r + 1][2 * c + 1], c);
  }
  __syncthreads();
  // 8 lanes per block: lane `r` takes row r, then column r
  const int b = t >> 3, r = t & 7, m = b / 6, j = b % 6;
  int in[8], out[8];
  if (b < nb) {
#pragma unroll
    for (int c = 0; c < 8; ++c)
      in[c] = (j < 4 ? (int)s_pix[0][(j >> 1) * 8 + r][m * 16 + (j & 1) * 8 + c] : (int)s_sub[j - 4][r][m * 8 + c]) - 128;
    jq_fdct8<true>(in, out);
#pragma unroll
    for (int c = 0; c < 8; ++c) s_dct[b][r * 8 + c] = out[c];
  }
  __syncthreads();
  if (b < nb) {
#pragma unroll
    for (int k = 0; k < 8; ++k) in[k] = s_dct[b][k * 8 + r];
    jq_fdct8<false>(in, out);
#pragma unroll
    for (int k = 0; k < 8; ++k) s_dct[b][k * 8 + r] = jq_quantize(out[k], (int)s_div[j >= 4][k * 8 + r]);
  }
  __syncthreads();
  const size_t blk0 = ((size_t)n * (H / 16) * mw + (size_t)my * mw + mx0) * 6;         // global index of the group's first block
  for (int i = t; i < nb * 64; i += TB) {
    const int16_t v = (int16_t)s_dct[i >> 6][kJqNatural[i & 63]];
    s_zz[i >> 6][i & 63] = v;
    coef[blk0 * 64 + i] = v;
  }
  __syncthreads();
  if (t < nb) {
    JqBitCounter cnt;
    jq_encode_ac(s_zz[t], (t % 6) >= 4, cnt);
    acbits[blk0 + t] = cnt.bits;
  }
}

__global__ __launch_bounds__(SCAN_TB) void jq_scan(const int16_t* __restrict__ coef, const uint32_t* __restrict__ acbits, int nblk,
                                                   uint32_t* __restrict__ offs, uint32_t* __restrict__ total) {
  __shared__ uint32_t s_wave[SCAN_TB / 64];
  __shared__ uint32_t s_carry;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const size_t base = (size_t)blockIdx.x * nblk;
  if (t == 0) s_carry = 0;
  __syncthreads();
  for (int i0 = 0; i0 < nblk; i0 += SCAN_TB) {
    const int i = i0 + t;
    uint32_t len = 0;
    if (i < nblk) {
      const int64_t prev = jq_prev_block(i);
      const int diff = (int)coef[(base + i) * 64] - (prev < 0 ? 0 : (int)coef[(base + prev) * 64]);
      JqBitCounter cnt;
      jq_encode_dc(diff, (i % 6) >= 4, cnt);
      len = cnt.bits + acbits[base + i];
    }
    uint32_t inc = len;                                   // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t v = __shfl_up(inc, o, 64);
      if (lane >= o) inc += v;
    }
    if (lane == 63) s_wave[wid] = inc;
    __syncthreads();
    uint32_t before = s_carry;
    for (int w = 0; w < wid; ++w) before += s_wave[w];
    if (i < nblk) offs[base + i] = before + inc - len;
    __syncthreads();
    if (t == SCAN_TB - 1) s_carry = before + inc;
    __syncthreads();
  }
  if (t == 0) total[blockIdx.x] = s_carry;
}

__global__ __launch_bounds__(64) void jq_emit(const int16_t* __restrict__ coef, const uint32_t* __restrict__ offs, int nblk, size_t nblk_all,
                                               uint32_t* __restrict__ bitbuf, size_t words_per_image) {
  const size_t g = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (g >= nblk_all) return;
  const size_t n = g / nblk;
  const int64_t i = (int64_t)(g % nblk), prev = jq_prev_block(i);
  const int16_t* zz = coef + g * 64;
  const int chroma = (i % 6) >= 4;
  const int diff = (int)zz[0] - (prev < 0 ? 0 : (int)coef[(n * nblk + prev) * 64]);
  JqBitWriter wr(bitbuf + n * words_per_image, words_per_image, offs[g]);
  jq_encode_dc(diff, chroma, wr);
  jq_encode_ac(zz, chroma, wr);
  wr.flush();
}

__global__ __launch_bounds__(SCAN_TB) void jq_count(const uint32_t* __restrict__ bitbuf, size_t words_per_image, const uint32_t* __restrict__ total,
                                                    int64_t* __restrict__ bytes_out) {
  __shared__ uint32_t s_wave[SCAN_TB / 64];
  const int t = threadIdx.x;
  const uint64_t bits = total[blockIdx.x];
  const uint64_t nw = min((uint64_t)words_per_image, (bits + 31) >> 5);
  const uint32_t* buf = bitbuf + (size_t)blockIdx.x * words_per_image;
  uint32_t c = 0;
  for (uint64_t w = t; w < nw; w += SCAN_TB) c += (uint32_t)jq_count_ff(buf[w], w, bits);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((t & 63) == 0) s_wave[t >> 6] = c;
  __syncthreads();
  if (t == 0) {
    uint32_t ff = 0;
    for (int w = 0; w < SCAN_TB / 64; ++w) ff += s_wave[w];
    bytes_out[blockIdx.x] = jq_file_bytes(bits, ff);
  }
}

// One pass packs SCAN_TB words: at most 8 bytes each, staged at the phase (0..15) of their address in the file buffer so that 16-byte pieces of the
// stage are 16-byte pieces of memory.
constexpr int PACK_STAGE = SCAN_TB * 8 + 16;

__global__ __launch_bounds__(SCAN_TB) void jq_pack(const uint32_t* __restrict__ bitbuf, size_t words_per_image, const uint32_t* __restrict__ total,
                                                   int H, int W, int quality, uint8_t* __restrict__ files, size_t stride,
                                                   int64_t* __restrict__ lengths) {
  __shared__ __attribute__((aligned(16))) uint8_t s_out[PACK_STAGE];
  __shared__ uint32_t s_wave[SCAN_TB / 64];
  __shared__ uint32_t s_carry;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const uint64_t bits = total[blockIdx.x];
  const uint64_t nbytes = (bits + 7) >> 3;
  const uint64_t nw = min((uint64_t)words_per_image, (bits + 31) >> 5);
  const uint32_t* buf = bitbuf + (size_t)blockIdx.x * words_per_image;
  uint8_t* row = files + (size_t)blockIdx.x * stride;
  const uint64_t cap = stride;                                // nothing at or beyond this offset of the row is written
  for (int i = t; i < JQ_HEADER_BYTES; i += SCAN_TB)
    if ((uint64_t)i < cap) row[i] = jq_header_byte(i, H, W, quality);
  if (t == 0) s_carry = 0;
  __syncthreads();
  for (uint64_t w0 = 0; w0 < nw; w0 += SCAN_TB) {
    const uint64_t w = w0 + t;
    const uint32_t word = w < nw ? buf[w] : 0u;
    const uint32_t c = w < nw ? (uint32_t)jq_count_ff(word, w, bits) : 0u;
    uint32_t inc = c;                                         // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t v = __shfl_up(inc, o, 64);
      if (lane >= o) inc += v;
    }
    if (lane == 63) s_wave[wid] = inc;
    __syncthreads();
    const uint32_t carry = s_carry;                           // 0xFF bytes before this pass
    uint32_t before = carry;
    for (int k = 0; k < wid; ++k) before += s_wave[k];
    before += inc - c;                                        // 0xFF bytes before this word
    // the pass's bytes go to [at0, at0 + len) of the file
    const uint64_t at0 = (uint64_t)JQ_HEADER_BYTES + w0 * 4 + carry;
    const uint32_t phase = (uint32_t)(reinterpret_cast<uintptr_t>(row + at0) & 15);
    if (w < nw) {
      uint8_t out[8];
      uint64_t at;
      const int n = jq_stuff_word(word, w, bits, before, out, at);
      for (int k = 0; k < n; ++k) s_out[phase + (uint32_t)(at - at0) + k] = out[k];
    }
    __syncthreads();
    if (t == SCAN_TB - 1) s_carry = before + c;
    __syncthreads();
    const uint32_t len = (uint32_t)(min(nbytes, (w0 + SCAN_TB) * 4) - w0 * 4) + (s_carry - carry);
    // stage index i is file offset at0 - phase + i; the valid ones are [phase, end)
    const uint32_t end = phase + (uint32_t)min((uint64_t)len, cap > at0 ? cap - at0 : 0);
    for (uint32_t lo = (uint32_t)t * 16; lo < end; lo += SCAN_TB * 16) {
      uint8_t* dst = row + at0 + lo - phase;                  // 16-byte aligned
      if (lo >= phase && lo + 16 <= end) {
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(s_out + lo);
      } else {
        for (uint32_t i = max(lo, phase); i < min(lo + 16, end); ++i) dst[i - lo] = s_out[i];
      }
    }
    __syncthreads();                                          // the next pass writes the stage again
  }
  if (t == 0) {
    const uint64_t eoi = (uint64_t)JQ_HEADER_BYTES + nbytes + s_carry;
    if (eoi < cap) row[eoi] = 0xff;
    if (eoi + 1 < cap) row[eoi + 1] = 0xd9;
    lengths[blockIdx.x] = jq_file_bytes(bits, s_carry);
  }
}

}  // namespace

extern "C" int ddpo_jpeg_size_workspace_bytes(int N, int H, int W, size_t* out_host) {
  JqLayout l;
  if (!out_host || !jq_layout(N, H, W, l)) return DDPO_EINVAL;
  *out_host = l.bytes;
  return DDPO_OK;
}

namespace {

struct JqBuffers {
  int16_t* coef;
  uint32_t *acbits, *offs, *total, *bitbuf;
};

// What ddpo_jpeg_size and ddpo_jpeg_encode share: the argument rules and the launches up to the finished bit buffers.
int jq_launch_streams(const void* images, int is_float32, int N, int H, int W, int quality, void* workspace, size_t workspace_bytes, hipStream_t s,
                      JqLayout& l, JqBuffers& b) {
  if (!images || !workspace || quality < 1 || quality > 100 || !jq_layout(N, H, W, l)) return DDPO_EINVAL;
  if (workspace_bytes < l.bytes || (reinterpret_cast<uintptr_t>(workspace) & 15) || iu_misaligned(images, is_float32))
    return DDPO_EINVAL;
  char* ws = static_cast<char*>(workspace);
  b.coef = reinterpret_cast<int16_t*>(ws + l.coef);
  b.acbits = reinterpret_cast<uint32_t*>(ws + l.acbits);
  b.offs = reinterpret_cast<uint32_t*>(ws + l.offs);
  b.total = reinterpret_cast<uint32_t*>(ws + l.total);
  b.bitbuf = reinterpret_cast<uint32_t*>(ws + l.bitbuf);
  const int mw = W / 16, mh = H / 16, nblk = mw * mh * 6;
  const size_t nblk_all = (size_t)nblk * N;
  if (hipMemsetAsync(b.bitbuf, 0, l.words_per_image * N * sizeof(uint32_t), s) != hipSuccess) return DDPO_ELAUNCH;
  const dim3 tgrid((unsigned)((size_t)N * mh * ((mw + MCUS - 1) / MCUS)));
  iu_dispatch(is_float32, [&](auto F32) { hipLaunchKernelGGL(jq_transform<F32()>, tgrid, dim3(TB), 0, s, images, H, W, quality, b.coef, b.acbits); });
  DDPO_LAUNCH_CHECK();
  hipLaunchKernelGGL(jq_scan, dim3(N), dim3(SCAN_TB), 0, s, b.coef, b.acbits, nblk, b.offs, b.total);
  DDPO_LAUNCH_CHECK();
  hipLaunchKernelGGL(jq_emit, dim3((unsigned)((nblk_all + 63) / 64)), dim3(64), 0, s, b.coef, b.offs, nblk, nblk_all, b.bitbuf, l.words_per_image);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

// libjpeg's limit on either dimension, and a row that holds at least the smallest file's fixed bytes
bool jq_encode_args(int H, int W, size_t file_stride) { return H <= 65500 && W <= 65500 && file_stride >= DDPO_JPEG_FIXED_BYTES; }

}  // namespace

extern "C" int ddpo_jpeg_size(const void* images, int is_float32, int N, int H, int W, int quality, void* workspace, size_t workspace_bytes,
                              int64_t* bytes_out, void* stream) {
  JqLayout l;
  JqBuffers b;
  if (!bytes_out) return DDPO_EINVAL;
  hipStream_t s = as_stream(stream);
  const int rc = jq_launch_streams(images, is_float32, N, H, W, quality, workspace, workspace_bytes, s, l, b);
  if (rc != DDPO_OK) return rc;
  hipLaunchKernelGGL(jq_count, dim3(N), dim3(SCAN_TB), 0, s, b.bitbuf, l.words_per_image, b.total, bytes_out);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

extern "C" int ddpo_jpeg_encode_max_bytes(int H, int W, size_t* out_host) {
  JqLayout l;
  if (!out_host || !jq_layout(1, H, W, l) || !jq_encode_args(H, W, DDPO_JPEG_FIXED_BYTES)) return DDPO_EINVAL;
  *out_host = (size_t)jq_file_max_bytes((uint64_t)(H / 16) * (uint64_t)(W / 16) * 6);
  return DDPO_OK;
}

extern "C" int ddpo_jpeg_encode(const void* images, int is_float32, int N, int H, int W, int quality, void* workspace, size_t workspace_bytes,
                                uint8_t* files, size_t file_stride, int64_t* lengths, void* stream) {
  JqLayout l;
  JqBuffers b;
  if (!files || !lengths || !jq_encode_args(H, W, file_stride)) return DDPO_EINVAL;
  hipStream_t s = as_stream(stream);
  const int rc = jq_launch_streams(images, is_float32, N, H, W, quality, workspace, workspace_bytes, s, l, b);
  if (rc != DDPO_OK) return rc;
  hipLaunchKernelGGL(jq_pack, dim3(N), dim3(SCAN_TB), 0, s, b.bitbuf, l.words_per_image, b.total, H, W, quality, files, file_stride, lengths);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

// Serial host path over the same functions (no GPU involved): what the kernels are held to, and what is held to a real encoder.
extern "C" int ddpo_jpeg_size_host(const uint8_t* rgb, int N, int H, int W, int quality, int64_t* bytes_out_host) {
  JqLayout l;
  if (!rgb || !bytes_out_host || quality < 1 || quality > 100 || !jq_layout(N, H, W, l)) return DDPO_EINVAL;
  for (int n = 0; n < N; ++n) bytes_out_host[n] = jq_host_image_bytes(rgb + (size_t)n * H * W * 3, H, W, quality);
  return DDPO_OK;
}

extern "C" int ddpo_jpeg_encode_host(const uint8_t* rgb, int N, int H, int W, int quality, uint8_t* files_host, size_t file_stride,
                                     int64_t* lengths_host) {
  JqLayout l;
  if (!rgb || !files_host || !lengths_host || quality < 1 || quality > 100 || !jq_layout(N, H, W, l) || !jq_encode_args(H, W, file_stride))
    return DDPO_EINVAL;
  for (int n = 0; n < N; ++n)
    lengths_host[n] = jq_host_image_file(rgb + (size_t)n * H * W * 3, H, W, quality, files_host + (size_t)n * file_stride, file_stride);
  return DDPO_OK;
}
