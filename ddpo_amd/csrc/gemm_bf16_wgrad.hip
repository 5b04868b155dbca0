// Weight gradient of the bf16 GEMM family (gemm_bf16.hip is the forward path): both kernels, their split selection and the two entry points.
// ------------------------------------------------------------------------------------------------
// Weight gradient on the bf16x3 MFMA datapath:  dW[k][n] += sum_m A(m,k) * dY[m][n]   (k = (ky,kx,ci); m = pixels)
// Both operands have the reduction index m as their SLOW memory dimension, so each is transposed while it is staged:
// a thread loads float4s of two consecutive pixels and writes, per channel, the packed (pixel m, pixel m+1) bf16 pair
// as one dword of the [row][m] LDS image.  Row pitch is 18 dwords (72 B): the pair writes of a half-wave hit 32
// distinct banks (x2, free) and the two ds_read_b64 of a fragment are conflict free.  Fast path only: stride 1,
// no upsampling (output pixel m == input pixel m, source address linear in m); other layers use gemm_wgrad_kernel.
// ------------------------------------------------------------------------------------------------
#include "gemm_bf16_common.h"
#include <type_traits>

#define WG_PITCH 18     // dwords per LDS row (16 dwords = 32 pixels of the k-tile, +2 pad)

// two floats -> packed bf16 hi pair and packed bf16 lo pair
__device__ __forceinline__ void split2(float a, float b, uint32_t& hi, uint32_t& lo) {
  hi = cvt_pk_bf16(a, b);
  lo = cvt_pk_bf16(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xFFFF0000u));
}

__device__ __forceinline__ bf16x8 lds_frag(const uint32_t* base, int row, int dw) {
  const uint2 a = *reinterpret_cast<const uint2*>(base + row * WG_PITCH + dw);
  const uint2 b = *reinterpret_cast<const uint2*>(base + row * WG_PITCH + dw + 2);
  return __builtin_bit_cast(bf16x8, make_uint4(a.x, a.y, b.x, b.y));
}

// APLN / BPLN: that operand arrives ALREADY split into bf16 hi / lo planes ((rows, ld) bf16, same element offsets as the fp32
// tensor: the activation planes a forward GroupNorm / LayerNorm wrote, or dY planes from a plane-emitting output stage) — the
// loader then only has to pair pixels m / m+1 of a channel into a dword (one v_perm_b32 per plane dword) instead of running the
// fp32 -> bf16 split (2 v_cvt_pk + 2 v_sub + 2 mask / shift per pair): the split was ~2/3 of this kernel's VALU work, which
// looked like its bound (measured in round 2: +0.5 % on the train step, so it is not).  Same values reach the MFMAs as in the fp32-fed form.
// Also measured and rejected in round 2: unconditional loads + a second register stage (two k-tiles of prefetch): 256 VGPRs with
// 12-24 spilled at two waves per SIMD, train step 9 % SLOWER (profiles/r02_ab_wgrad_deep.log).
// ROWL ("row loader", round 2): the SQ counters of the loader below showed ~10 VALU + 4 SALU per MFMA at 31 % MFMA-pipe busy: 16 bytes per
// fetch, ~25 VALU per fetch of 64-bit address arithmetic, per-pixel (batch, y, x) bookkeeping with loops and divergent branches around every
// load.  For the regular layers (dense, or stride-1 "same" convolutions whose rows tile into the 32-pixel k-tiles: OW % 32 == 0 or
// 32 % OW == 0; M % 32 == 0; operand tensors < 2 GiB) all of that collapses: a k-tile is 32 consecutive pixels starting at an image-row
// boundary that is the SAME for the whole workgroup, so (oy, ox) of the tile live in scalars, every thread's four byte offsets relative
// to the tile are CONSTANTS, the per-tile advance is one scalar soffset, and a masked element is an out-of-range buffer offset that reads
// zeros (raw buffer loads) — ~6 VALU per activation fetch, none per dY fetch, no branches.
template <bool APLN, bool BPLN, bool ROWL = false>
__global__ void __launch_bounds__(BF_THREADS) gemm_wgrad_bf16_kernel(const ddpo_gemm_desc d, int tiles_n, int m_per_split,
                                                                   const uint16_t* __restrict__ a_hi, const uint16_t* __restrict__ a_lo,
                                                                   const uint16_t* __restrict__ b_hi, const uint16_t* __restrict__ b_lo) {
  constexpr int BM = 128, BN = 128, BK = 32;
  constexpr int PLANE = BM * WG_PITCH;                 // dwords per plane (BM == BN)
  __shared__ __attribute__((aligned(16))) uint32_t smem[2][4 * PLANE];     // per stage: A_hi | A_lo | B_hi | B_lo
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int tile_m = blockIdx.x / tiles_n, tile_n = blockIdx.x - tile_m * tiles_n;
  const int k0 = tile_m * BM, n0 = tile_n * BN;
  const int m_begin = blockIdx.y * m_per_split;
  const int m_end = min(m_begin + m_per_split, d.M);
  if (m_begin >= m_end) return;

  const bool conv = d.ksize > 0;
  // loader geometry: quad q = lane&7 (4 consecutive k or n), pixel pair pp = lane>>3, wave w covers rows 32w..32w+31
  const int q = lane & 7, pp = lane >> 3;
  const int arow = 32 * wid + 4 * q;                   // first of this thread's 4 LDS rows (same for A and B tiles)
  const int kg = k0 + arow;                            // global k of those rows
  const bool kvalid = kg < d.K;
  int dky = 0, dkx = 0, ci = kg;
  if (conv) {
    const int tap = kg / d.Cin;
    ci = kg - tap * d.Cin;
    const int ky = tap / d.ksize;
    dky = ky - d.pad;
    dkx = tap - ky * d.ksize - d.pad;
  }
  const int ng = n0 + arow;
  const bool nvalid = ng < d.N;
  // the 4 OUTPUT pixels this thread stages per k-tile: m = m_begin + kt*32 + 16*p + 2*pp + e ; (batch, oy, ox) are tracked
  // incrementally.  Stride-1 "same" convolutions read input pixel m + a constant tap offset (`simple`); strided and
  // nearest-2x-upsampled ones compute the source pixel of the tap from (oy, ox).
  const bool simple = !conv || (d.stride == 1 && d.upsample == 0 && d.OH == d.H && d.OW == d.W);
  const int VH = d.upsample ? 2 * d.H : d.H, VW = d.upsample ? 2 * d.W : d.W;
  int pb[2][2], poy[2][2], pox[2][2];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int m = m_begin + 16 * p + 2 * pp + e;
      pox[p][e] = conv ? m % d.OW : 0;
      poy[p][e] = conv ? (m / d.OW) % d.OH : 0;
      pb[p][e] = conv ? m / (d.OW * d.OH) : 0;
    }
  // element strides / channel terms of the two operands.  A k-blocked PLANE operand (ld == 0: (C / 32, rows, 32), ABI v6) has pixel
  // stride 32 and the channel quad's block base + offset inside the block as its "channel term"; everything below is written on these.
  const bool kbA = APLN && d.ld_src == 0, kbB = BPLN && d.ld_w == 0;
  const int64_t rowsA = conv ? (int64_t)d.B * d.H * d.W : (int64_t)d.M;
  const int lda_e = kbA ? 32 : d.ld_src, ldb_e = kbB ? 32 : d.ld_w;
  const int64_t a_c0 = kbA ? (int64_t)(ci >> 5) * rowsA * 32 + (ci & 31) : (int64_t)ci;          // dense: ci == kg
  const int64_t b_c0 = kbB ? (int64_t)(ng >> 5) * (int64_t)d.M * 32 + (ng & 31) : (int64_t)ng;
  const int64_t tap_off = conv ? ((int64_t)dky * d.W + dkx) * lda_e + a_c0 : a_c0;

  float4 ra[2][2], rb[2][2];          // fp32 operands; a plane operand keeps (hi.x, hi.y, lo.x, lo.y) raw bits in the same registers
  auto as_f4 = [](const uint2 h, const uint2 l) {
    return make_float4(__uint_as_float(h.x), __uint_as_float(h.y), __uint_as_float(l.x), __uint_as_float(l.y));
  };
  // ---- ROWL state (see the note above the kernel)
  constexpr uint32_t ESA = APLN ? 2u : 4u, ESB = BPLN ? 2u : 4u;     // bytes per element of the operands as stored
  uint32_t rl_va[2][2], rl_vb[2][2];   // byte offsets of this thread's elements for k-tile 0 (BUF_OOB: never valid)
  int rl_cy[2][2], rl_cx[2][2];        // iy = oy_t + cy, ix = ox_t + cx of the element's tap
  int rl_oy = 0, rl_ox = 0;            // image row / column of the CURRENT k-tile's first pixel (uniform)
  // a tap above / left of the tile has a NEGATIVE offset relative to its pixel: the activation descriptors start `rl_guard` bytes in front of
  // the tensor so that every offset is non-negative (such elements are only ever fetched when their tap is inside the image, i.e. in range)
  const int64_t rl_guard = conv ? (int64_t)(d.W + 1) * lda_e * (int64_t)ESA : 0;
  __amdgpu_buffer_rsrc_t rl_ra0 = make_rsrc(reinterpret_cast<const char*>(APLN ? (const void*)a_hi : (const void*)d.src) - rl_guard),
                         rl_ra1 = make_rsrc(reinterpret_cast<const char*>(APLN ? (const void*)a_lo : (const void*)d.src) - rl_guard);
  __amdgpu_buffer_rsrc_t rl_rb0 = make_rsrc(BPLN ? (const void*)b_hi : (const void*)d.w), rl_rb1 = make_rsrc(BPLN ? (const void*)b_lo : (const void*)d.w);
  if constexpr (ROWL) {
    const int rem = conv ? m_begin % (d.OH * d.OW) : 0;
    rl_oy = conv ? rem / d.OW : 0;
    rl_ox = conv ? rem - rl_oy * d.OW : 0;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int eoff = 16 * p + 2 * pp + e;
        const int dy_e = (conv && d.OW < BK) ? eoff / d.OW : 0;
        const int x_e = (conv && d.OW < BK) ? eoff - dy_e * d.OW : eoff;
        rl_cy[p][e] = dy_e + dky;
        rl_cx[p][e] = x_e + dkx;
        const int64_t ao = ((int64_t)(m_begin + eoff) * lda_e + tap_off) * (int64_t)ESA + rl_guard;
        const int64_t bo = ((int64_t)(m_begin + eoff) * ldb_e + b_c0) * (int64_t)ESB;
        rl_va[p][e] = (kvalid && ao >= 0 && ao < 0x7FFFFFF0ll) ? (uint32_t)ao : BUF_OOB;
        rl_vb[p][e] = (nvalid && bo >= 0 && bo < 0x7FFFFFF0ll) ? (uint32_t)bo : BUF_OOB;
      }
  }
  auto load_tile_rows = [&](int kt) {
    const uint32_t so_a = (uint32_t)kt * (uint32_t)(BK * lda_e) * ESA, so_b = (uint32_t)kt * (uint32_t)(BK * ldb_e) * ESB;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        uint32_t voa = rl_va[p][e];
        if (conv) {
          const bool ok = (unsigned)(rl_oy + rl_cy[p][e]) < (unsigned)d.H && (unsigned)(rl_ox + rl_cx[p][e]) < (unsigned)d.W;
          voa = ok ? voa : BUF_OOB;
        }
        if (APLN) {
          const u32x2 h2 = __builtin_amdgcn_raw_buffer_load_b64(rl_ra0, voa, so_a, 0), l2 = __builtin_amdgcn_raw_buffer_load_b64(rl_ra1, voa, so_a, 0);
          ra[p][e] = make_float4(__uint_as_float(h2.x), __uint_as_float(h2.y), __uint_as_float(l2.x), __uint_as_float(l2.y));
        } else {
          const u32x4 v4 = __builtin_amdgcn_raw_buffer_load_b128(rl_ra0, voa, so_a, 0);
          ra[p][e] = make_float4(__uint_as_float(v4.x), __uint_as_float(v4.y), __uint_as_float(v4.z), __uint_as_float(v4.w));
        }
        if (BPLN) {
          const u32x2 h2 = __builtin_amdgcn_raw_buffer_load_b64(rl_rb0, rl_vb[p][e], so_b, 0), l2 = __builtin_amdgcn_raw_buffer_load_b64(rl_rb1, rl_vb[p][e], so_b, 0);
          rb[p][e] = make_float4(__uint_as_float(h2.x), __uint_as_float(h2.y), __uint_as_float(l2.x), __uint_as_float(l2.y));
        } else {
          const u32x4 v4 = __builtin_amdgcn_raw_buffer_load_b128(rl_rb0, rl_vb[p][e], so_b, 0);
          rb[p][e] = make_float4(__uint_as_float(v4.x), __uint_as_float(v4.y), __uint_as_float(v4.z), __uint_as_float(v4.w));
        }
      }
    if (conv) {                           // next k-tile: 32 pixels on (uniform)
      if (d.OW >= BK) {
        rl_ox += BK;
        if (rl_ox >= d.OW) { rl_ox = 0; rl_oy = rl_oy + 1 >= d.OH ? 0 : rl_oy + 1; }
      } else {
        rl_oy += BK / d.OW;
        if (rl_oy >= d.OH) rl_oy -= d.OH;
      }
    }
  };
  auto load_tile_px = [&](int kt) {
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int m = m_begin + kt * BK + 16 * p + 2 * pp + e;
        float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
        if (m < m_end) {
          bool ok = kvalid;
          int64_t aoff = (int64_t)m * lda_e + tap_off;
          if (conv) {
            const int iy = poy[p][e] * d.stride + dky, ix = pox[p][e] * d.stride + dkx;       // virtual (upsampled) coordinates
            ok = ok && iy >= 0 && iy < VH && ix >= 0 && ix < VW;
            if (!simple) {
              const int sy = d.upsample ? (iy >> 1) : iy, sx = d.upsample ? (ix >> 1) : ix;
              aoff = ((int64_t)(pb[p][e] * d.H + sy) * d.W + sx) * lda_e + a_c0;
            }
          }
          if (ok) {
            if (APLN) va = as_f4(*reinterpret_cast<const uint2*>(a_hi + aoff), *reinterpret_cast<const uint2*>(a_lo + aoff));
            else va = *reinterpret_cast<const float4*>(d.src + aoff);
          }
          if (nvalid) {
            const int64_t boff = (int64_t)m * ldb_e + b_c0;
            if (BPLN) vb = as_f4(*reinterpret_cast<const uint2*>(b_hi + boff), *reinterpret_cast<const uint2*>(b_lo + boff));
            else vb = *reinterpret_cast<const float4*>(d.w + boff);
          }
        }
        ra[p][e] = va;
        rb[p][e] = vb;
        if (conv) {          // advance this pixel by BK
          pox[p][e] += BK;
          while (pox[p][e] >= d.OW) { pox[p][e] -= d.OW; ++poy[p][e]; }
          while (poy[p][e] >= d.OH) { poy[p][e] -= d.OH; ++pb[p][e]; }
        }
      }
  };
  auto load_tile = [&](int kt) {
    if constexpr (ROWL) load_tile_rows(kt); else load_tile_px(kt);
  };
  // bias gradient (d.colsum, fp32 dY only): the k = 0 row of workgroups also sums the dY values it stages, per channel
  const bool do_cs = !BPLN && d.colsum != nullptr && tile_m == 0;
  float cs[4] = {0.f, 0.f, 0.f, 0.f};
  auto store_tile = [&](int buf) {
    uint32_t* st = smem[buf];
    if (do_cs) {
#pragma unroll
      for (int j = 0; j < 4; ++j) cs[j] += ((&rb[0][0].x)[j] + (&rb[0][1].x)[j]) + ((&rb[1][0].x)[j] + (&rb[1][1].x)[j]);
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int dw = pp + 8 * p;                        // dword (= pixel pair) index within the row
      const float* a0 = &ra[p][0].x; const float* a1 = &ra[p][1].x;
      const float* b0 = &rb[p][0].x; const float* b1 = &rb[p][1].x;
      // plane operand: registers hold [ch0|ch1, ch2|ch3] (hi) and the same for lo, per pixel; pair channel j of pixels m, m+1
      auto pair = [](const float* p0, const float* p1, int j, int plane) {
        const uint32_t w0 = __float_as_uint(p0[2 * plane + (j >> 1)]), w1 = __float_as_uint(p1[2 * plane + (j >> 1)]);
        return __builtin_amdgcn_perm(w1, w0, (j & 1) ? 0x07060302u : 0x05040100u);
      };
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint32_t hi, lo;
        if (APLN) { hi = pair(a0, a1, j, 0); lo = pair(a0, a1, j, 1); }
        else split2(a0[j], a1[j], hi, lo);              // (pixel m, pixel m+1) of channel k+j
        st[(arow + j) * WG_PITCH + dw] = hi;
        st[PLANE + (arow + j) * WG_PITCH + dw] = lo;
        if (BPLN) { hi = pair(b0, b1, j, 0); lo = pair(b0, b1, j, 1); }
        else split2(b0[j], b1[j], hi, lo);
        st[2 * PLANE + (arow + j) * WG_PITCH + dw] = hi;
        st[3 * PLANE + (arow + j) * WG_PITCH + dw] = lo;
      }
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nk = (m_end - m_begin + BK - 1) / BK;
  const int li = lane & 31, h = lane >> 5;
  load_tile(0);
  store_tile(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) load_tile(kt + 1);
    const uint32_t* st = smem[cur];
#pragma unroll
    for (int ms = 0; ms < 2; ++ms) {
      const int dw = 8 * ms + 4 * h;
      bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        ah[i] = lds_frag(st, wm * 64 + i * 32 + li, dw);
        al[i] = lds_frag(st + PLANE, wm * 64 + i * 32 + li, dw);
        bh[i] = lds_frag(st + 2 * PLANE, wn * 64 + i * 32 + li, dw);
        bl[i] = lds_frag(st + 3 * PLANE, wn * 64 + i * 32 + li, dw);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
        }
    }
    if (kt + 1 < nk) store_tile(cur ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + wn * 64 + j * 32 + li;
      if (col >= d.N) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = k0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (row >= d.K) continue;
        atomicAdd(d.out + (int64_t)row * d.ld_out + col, d.alpha * acc[i][j][r]);
      }
    }
  if (do_cs) {                                  // lanes q + 8 * pp of a wave hold the same 4 channels: fold the 8 pixel-pair lanes, lane pp == 0 adds
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v = cs[j];
      v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
      if (pp == 0 && ng + j < d.N) atomicAdd(d.colsum + ng + j, v);
    }
  }
}

// WIDE weight-gradient tile (round 3): 128 (k) x 320 (n) per workgroup, 8 waves of 32 x 160, one workgroup per CU.  The 128 x 128 kernel above
// moves 32 KB of operands per 0.52 M multiply-adds (61 B / kMAC) and sits at the CU's ~20 B / clk fetch rate with the matrix pipe 42 % busy
// (236 TF); this tile moves 56 KB per 1.31 M (43 B / kMAC) — the forward 128x320 tile's ratio.  Row loader only (the regular layers: dense, and
// stride-1 "same" convolutions whose rows tile into the 32-pixel k-tiles), N % 320 == 0; same staging (pixel pairs of a channel packed into one
// dword of the [row][m] LDS image), same MFMA order per element as the 128 x 128 kernel.
//   loader tasks (4 channels x 2 pixels, 8 quads x 8 pixel pairs per wave): A = 128 rows x 16 pairs = 8 wave tasks, one per wave;
//   dY = 320 rows x 16 pairs = 20 wave tasks: waves 0-3 take three, waves 4-7 two.
template <bool APLN, bool BPLN>
__global__ void __launch_bounds__(512) gemm_wgrad_bf16_wide_kernel(const ddpo_gemm_desc d, int tiles_n, int m_per_split,
                                                                   const uint16_t* __restrict__ a_hi, const uint16_t* __restrict__ a_lo,
                                                                   const uint16_t* __restrict__ b_hi, const uint16_t* __restrict__ b_lo) {
  constexpr int BM = 128, BN = 320, BK = 32, TN = 5, NBT = 3;
  constexpr int PA = BM * WG_PITCH, PB = BN * WG_PITCH;          // dwords per plane
  constexpr int STAGE = 2 * PA + 2 * PB;                         // A_hi | A_lo | B_hi | B_lo
  extern __shared__ __attribute__((aligned(16))) uint32_t wsm[];
  const int t = threadIdx.x, lane = t & 63, wid = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wid >> 1, wn = wid & 1;
  const int tile_m = blockIdx.x / tiles_n, tile_n = blockIdx.x - tile_m * tiles_n;
  const int k0 = tile_m * BM, n0 = tile_n * BN;
  const int m_begin = blockIdx.y * m_per_split;
  const int m_end = min(m_begin + m_per_split, d.M);
  if (m_begin >= m_end) return;
  const bool conv = d.ksize > 0;
  const int q = lane & 7, pp = lane >> 3;
  // ---- this thread's A task: 4 channel rows, one pixel pair
  const int a_row = 32 * (wid & 3) + 4 * q, a_dw = 8 * (wid >> 2) + pp;
  const int kg = k0 + a_row;
  const bool kvalid = kg < d.K;
  int dky = 0, dkx = 0, ci = kg;
  if (conv) {
    const int tap = kg / d.Cin;
    ci = kg - tap * d.Cin;
    const int ky = tap / d.ksize;
    dky = ky - d.pad;
    dkx = tap - ky * d.ksize - d.pad;
  }
  const bool kbA = APLN && d.ld_src == 0, kbB = BPLN && d.ld_w == 0;
  const int64_t rowsA = conv ? (int64_t)d.B * d.H * d.W : (int64_t)d.M;
  const int lda_e = kbA ? 32 : d.ld_src, ldb_e = kbB ? 32 : d.ld_w;
  const int64_t a_c0 = kbA ? (int64_t)(ci >> 5) * rowsA * 32 + (ci & 31) : (int64_t)ci;
  const int64_t tap_off = conv ? ((int64_t)dky * d.W + dkx) * lda_e + a_c0 : a_c0;
  constexpr uint32_t ESA = APLN ? 2u : 4u, ESB = BPLN ? 2u : 4u;
  const int64_t rl_guard = conv ? (int64_t)(d.W + 1) * lda_e * (int64_t)ESA : 0;
  const __amdgpu_buffer_rsrc_t rs_a0 = make_rsrc(reinterpret_cast<const char*>(APLN ? (const void*)a_hi : (const void*)d.src) - rl_guard),
                               rs_a1 = make_rsrc(reinterpret_cast<const char*>(APLN ? (const void*)a_lo : (const void*)d.src) - rl_guard);
  const __amdgpu_buffer_rsrc_t rs_b0 = make_rsrc(BPLN ? (const void*)b_hi : (const void*)d.w), rs_b1 = make_rsrc(BPLN ? (const void*)b_lo : (const void*)d.w);
  uint32_t va[2], vb[NBT][2];
  int cy[2], cx[2];
  const int rem0 = conv ? m_begin % (d.OH * d.OW) : 0;
  int t_oy = conv ? rem0 / d.OW : 0, t_ox = conv ? rem0 - (rem0 / d.OW) * d.OW : 0;      // image position of the current k-tile's first pixel (uniform)
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int eoff = 2 * a_dw + e;
    const int dy_e = (conv && d.OW < BK) ? eoff / d.OW : 0;
    const int x_e = (conv && d.OW < BK) ? eoff - dy_e * d.OW : eoff;
    cy[e] = dy_e + dky;
    cx[e] = x_e + dkx;
    const int64_t ao = ((int64_t)(m_begin + eoff) * lda_e + tap_off) * (int64_t)ESA + rl_guard;
    va[e] = (kvalid && ao >= 0 && ao < 0x7FFFFFF0ll) ? (uint32_t)ao : BUF_OOB;
  }
  int b_row[NBT], b_dw[NBT];
#pragma unroll
  for (int i = 0; i < NBT; ++i) {
    const int T = wid + 8 * i;                         // wave task: channel block T >> 1 (of 10), pixel-pair half T & 1
    b_row[i] = 32 * (T >> 1) + 4 * q;
    b_dw[i] = 8 * (T & 1) + pp;
    const int ng = n0 + b_row[i];
    const int64_t b_c0 = kbB ? (int64_t)(ng >> 5) * (int64_t)d.M * 32 + (ng & 31) : (int64_t)ng;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int64_t bo = ((int64_t)(m_begin + 2 * b_dw[i] + e) * ldb_e + b_c0) * (int64_t)ESB;
      vb[i][e] = (T < 20 && ng < d.N && bo >= 0 && bo < 0x7FFFFFF0ll) ? (uint32_t)bo : BUF_OOB;
    }
  }
  const bool third = wid < 4;                          // wave-uniform: this wave stages a third dY task
  // TWO register sets: tile T travels in set T & 1 and is requested two k-tiles before it is written to LDS (one workgroup per CU: nothing else
  // covers the fetch latency; with one set the loop measured no faster than the 128 x 128 kernel's two workgroups per CU)
  float4 ra[2][2], rb[2][NBT][2];
  auto ld4 = [&](const __amdgpu_buffer_rsrc_t r0, const __amdgpu_buffer_rsrc_t r1, uint32_t vo, uint32_t so, bool pl) {
    if (pl) {
      const u32x2 h2 = __builtin_amdgcn_raw_buffer_load_b64(r0, vo, so, 0), l2 = __builtin_amdgcn_raw_buffer_load_b64(r1, vo, so, 0);
      return make_float4(__uint_as_float(h2.x), __uint_as_float(h2.y), __uint_as_float(l2.x), __uint_as_float(l2.y));
    }
    const u32x4 v4 = __builtin_amdgcn_raw_buffer_load_b128(r0, vo, so, 0);
    return make_float4(__uint_as_float(v4.x), __uint_as_float(v4.y), __uint_as_float(v4.z), __uint_as_float(v4.w));
  };
  const int nk = (m_end - m_begin + BK - 1) / BK;
  auto load_tile = [&](int kt, auto sc) {              // requests past the last k-tile re-fetch it (unconditional loads: counted waits stay exact)
    constexpr int S = decltype(sc)::value;
    const int ktc = min(kt, nk - 1);
    const uint32_t so_a = (uint32_t)ktc * (uint32_t)(BK * lda_e) * ESA, so_b = (uint32_t)ktc * (uint32_t)(BK * ldb_e) * ESB;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      uint32_t vo = va[e];
      if (conv) vo = ((unsigned)(t_oy + cy[e]) < (unsigned)d.H && (unsigned)(t_ox + cx[e]) < (unsigned)d.W) ? vo : BUF_OOB;
      ra[S][e] = ld4(rs_a0, rs_a1, vo, so_a, APLN);
    }
#pragma unroll
    for (int i = 0; i < NBT; ++i) {
      if (i == 2 && !third) continue;
#pragma unroll
      for (int e = 0; e < 2; ++e) rb[S][i][e] = ld4(rs_b0, rs_b1, vb[i][e], so_b, BPLN);
    }
    if (conv && kt < nk - 1) {            // next k-tile: 32 pixels on (uniform)
      if (d.OW >= BK) {
        t_ox += BK;
        if (t_ox >= d.OW) { t_ox = 0; t_oy = t_oy + 1 >= d.OH ? 0 : t_oy + 1; }
      } else {
        t_oy += BK / d.OW;
        if (t_oy >= d.OH) t_oy -= d.OH;
      }
    }
  };
  auto pair = [](const float* p0, const float* p1, int j, int plane) {
    const uint32_t w0 = __float_as_uint(p0[2 * plane + (j >> 1)]), w1 = __float_as_uint(p1[2 * plane + (j >> 1)]);
    return __builtin_amdgcn_perm(w1, w0, (j & 1) ? 0x07060302u : 0x05040100u);
  };
  const bool do_cs = !BPLN && d.colsum != nullptr && tile_m == 0;      // bias gradient: see the 128 x 128 kernel
  float cs[NBT][4];
#pragma unroll
  for (int i = 0; i < NBT; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) cs[i][j] = 0.f;
  auto store_tile = [&](int buf, auto sc) {
    constexpr int S = decltype(sc)::value;
    uint32_t* st = wsm + buf * STAGE;
    if (do_cs) {
#pragma unroll
      for (int i = 0; i < NBT; ++i) {
        if (i == 2 && !third) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) cs[i][j] += (&rb[S][i][0].x)[j] + (&rb[S][i][1].x)[j];
      }
    }
    {
      const float* a0 = &ra[S][0].x; const float* a1 = &ra[S][1].x;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint32_t hi, lo;
        if (APLN) { hi = pair(a0, a1, j, 0); lo = pair(a0, a1, j, 1); }
        else split2(a0[j], a1[j], hi, lo);
        st[(a_row + j) * WG_PITCH + a_dw] = hi;
        st[PA + (a_row + j) * WG_PITCH + a_dw] = lo;
      }
    }
#pragma unroll
    for (int i = 0; i < NBT; ++i) {
      if (i == 2 && !third) continue;
      const float* b0 = &rb[S][i][0].x; const float* b1 = &rb[S][i][1].x;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint32_t hi, lo;
        if (BPLN) { hi = pair(b0, b1, j, 0); lo = pair(b0, b1, j, 1); }
        else split2(b0[j], b1[j], hi, lo);
        st[2 * PA + (b_row[i] + j) * WG_PITCH + b_dw[i]] = hi;
        st[2 * PA + PB + (b_row[i] + j) * WG_PITCH + b_dw[i]] = lo;
      }
    }
  };

  f32x16 acc[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  const int li = lane & 31, h = lane >> 5;
  auto compute = [&](int cur) {
    const uint32_t* st = wsm + cur * STAGE;
#pragma unroll
    for (int ms = 0; ms < 2; ++ms) {
      const int dw = 8 * ms + 4 * h;
      const bf16x8 ah = lds_frag(st, wm * 32 + li, dw), al = lds_frag(st + PA, wm * 32 + li, dw);
      bf16x8 bh[TN], bl[TN];
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        bh[j] = lds_frag(st + 2 * PA, wn * 160 + j * 32 + li, dw);
        bl[j] = lds_frag(st + 2 * PA + PB, wn * 160 + j * 32 + li, dw);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh[j], acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl[j], acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh[j], acc[j], 0, 0, 0);
      }
    }
  };
  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;
  load_tile(0, S0{});
  store_tile(0, S0{});
  load_tile(1, S1{});
  load_tile(2, S0{});
  __syncthreads();
  // iteration kt: tile kt + 1 (requested two iterations ago) -> the LDS stage everybody left at the last barrier; request tile kt + 3 into
  // the registers just freed; multiply tile kt
  auto step = [&](int kt, auto sc) {
    constexpr int S = decltype(sc)::value;             // == (kt + 1) & 1
    if (kt + 1 < nk) store_tile(S, sc);
    load_tile(kt + 3, sc);
    compute(S ^ 1);
    __syncthreads();
  };
  int kt = 0;
#pragma unroll 1
  for (; kt + 1 < nk; kt += 2) {
    step(kt, S1{});
    step(kt + 1, S0{});
  }
  if (kt < nk) step(kt, S1{});
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = n0 + wn * 160 + j * 32 + li;
    if (col >= d.N) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = k0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (row >= d.K) continue;
      atomicAdd(d.out + (int64_t)row * d.ld_out + col, d.alpha * acc[j][r]);
    }
  }
  if (do_cs) {
#pragma unroll
    for (int i = 0; i < NBT; ++i) {
      if (i == 2 && !third) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v = cs[i][j];
        v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
        const int n = n0 + b_row[i] + j;
        if (pp == 0 && vb[i][0] != BUF_OOB && n < d.N) atomicAdd(d.colsum + n, v);
      }
    }
  }
}

// The split of the pixel reduction whose tiles x splits fills whole rounds of the chip's `slots` workgroup slots best, among 1 .. `rounds`
// rounds (1035 workgroups on 512 slots cost three rounds, 966 two); among fills within `margin` prefer fewer splits (fewer atomic adds, longer
// k-loops).  Then the pixels per split, in whole 32-pixel k-tiles, and the number of splits that leaves.
static int best_split(int tiles, int M, int slots, int rounds, double margin) {
  const int max_splits = (M + 255) / 256;
  int best = 1;
  double best_eff = 0.0;
  for (int r = 1; r <= rounds; ++r) {
    int cand = (slots * r) / tiles;
    if (cand > max_splits) cand = max_splits;
    if (cand < 1) cand = 1;
    const long wgs = (long)tiles * cand;
    const double eff = (double)wgs / (double)(((wgs + slots - 1) / slots) * slots);
    if (eff > best_eff + margin || best_eff == 0.0) { best_eff = eff; best = cand; }
  }
  return best;
}
static int pixels_per_split(int M, int& splits) {
  int mps = (M + splits - 1) / splits;
  mps = (mps + 31) / 32 * 32;
  splits = (M + mps - 1) / mps;
  return mps;
}

// one launch: the wide 128 x 320 tile, or the 128 x 128 tile with the row loader (`rows`) or the per-pixel loader
template <bool APLN, bool BPLN>
static void launch_wgrad(const ddpo_gemm_desc& d, bool wide, bool rows, int tiles, int tiles_n, int splits, int mps, const uint16_t* a_hi,
                         const uint16_t* a_lo, const uint16_t* b_hi, const uint16_t* b_lo, hipStream_t st) {
  if (wide) {
    const size_t lds = (size_t)2 * (2 * 128 + 2 * 320) * WG_PITCH * 4;
    static bool attr_set = false;
    if (!attr_set) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_wgrad_bf16_wide_kernel<APLN, BPLN>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      attr_set = true;
    }
    hipLaunchKernelGGL((gemm_wgrad_bf16_wide_kernel<APLN, BPLN>), dim3(tiles, splits), dim3(512), lds, st, d, tiles_n, mps, a_hi, a_lo, b_hi, b_lo);
  } else if (rows) {
    hipLaunchKernelGGL((gemm_wgrad_bf16_kernel<APLN, BPLN, true>), dim3(tiles, splits), dim3(BF_THREADS), 0, st, d, tiles_n, mps, a_hi, a_lo, b_hi, b_lo);
  } else {
    hipLaunchKernelGGL((gemm_wgrad_bf16_kernel<APLN, BPLN, false>), dim3(tiles, splits), dim3(BF_THREADS), 0, st, d, tiles_n, mps, a_hi, a_lo, b_hi, b_lo);
  }
}

static int wgrad_bf16x3(const ddpo_gemm_desc* dp, const uint16_t* a_hi, const uint16_t* a_lo, const uint16_t* b_hi, const uint16_t* b_lo,
                       void* stream) {
  if (!dp) return DDPO_EINVAL;
  ddpo_gemm_desc d = *dp;
  if ((!d.src && !a_hi) || (!d.w && !b_hi) || !d.out || d.M <= 0 || d.N <= 0 || d.K <= 0 || d.res_rows) return DDPO_EINVAL;
  if ((a_hi && !a_lo) || (b_hi && !b_lo)) return DDPO_EINVAL;
  if (d.colsum && b_hi) return DDPO_EINVAL;          // the fused bias gradient sums the fp32 dY registers
  if ((d.ld_src & 3) || (d.ld_w & 3) || (d.N & 3) || (d.K & 3)) return DDPO_EINVAL;
  if (!a_hi && (reinterpret_cast<uintptr_t>(d.src) & 15)) return DDPO_EINVAL;
  if (!b_hi && (reinterpret_cast<uintptr_t>(d.w) & 15)) return DDPO_EINVAL;
  if ((reinterpret_cast<uintptr_t>(a_hi) | reinterpret_cast<uintptr_t>(a_lo) | reinterpret_cast<uintptr_t>(b_hi) | reinterpret_cast<uintptr_t>(b_lo)) & 7)
    return DDPO_EINVAL;
  // ld == 0 marks a k-blocked PLANE operand (channels / 32, rows, 32): planes only, whole 32-channel blocks
  if (d.ld_src < 0 || d.ld_w < 0) return DDPO_EINVAL;
  if (d.ld_src == 0 && (!a_hi || ((d.ksize > 0 ? d.Cin : d.K) & 31))) return DDPO_EINVAL;
  if (d.ld_w == 0 && (!b_hi || (d.N & 31))) return DDPO_EINVAL;
  if (d.ksize > 0) {
    if (d.ksize != 1 && d.ksize != 3) return DDPO_EINVAL;
    if ((d.Cin & 3) || d.K != d.ksize * d.ksize * d.Cin || d.M != d.B * d.OH * d.OW) return DDPO_EINVAL;
    if (d.stride < 1 || d.stride > 2 || d.upsample < 0 || d.upsample > 1 || d.pad != d.ksize / 2) return DDPO_EINVAL;
    if ((int64_t)d.B * d.H * d.W * d.ld_src >= ((int64_t)1 << 40)) return DDPO_EINVAL;
  }
  // row loader for the regular layers (the per-pixel loader takes the rest): conv 320->320 @ 64^2, U-Net batch 64:
  // 2.54 -> 2.05 ms (190 -> 236 TF), profiles/r02_ab_wgrad_rows.log
  const bool conv_ = d.ksize > 0;
  const bool simple_ = !conv_ || (d.stride == 1 && d.upsample == 0 && d.OH == d.H && d.OW == d.W);
  const int64_t lda_b = d.ld_src ? d.ld_src : (conv_ ? d.Cin : d.K), ldb_b = d.ld_w ? d.ld_w : d.N;      // k-blocked planes: the same bytes in all
  const int64_t a_bytes = (int64_t)d.M * lda_b * (a_hi ? 2 : 4), b_bytes = (int64_t)d.M * ldb_b * (b_hi ? 2 : 4);
  const bool rows_ok = simple_ && (d.M % 32) == 0 && a_bytes + (conv_ ? (int64_t)(d.W + 1) * lda_b * 4 : 0) < 0x7FFFFFF0ll && b_bytes < 0x7FFFFFF0ll &&
                       (!conv_ || (((d.OW % 32) == 0 || (32 % d.OW) == 0) && ((d.OH * d.OW) % 32) == 0));
  // wide 128 x 320 tile (one workgroup per CU) where it measured faster (tools/native/kernel_probe wgrad, profiles/r03_probe_wgrad.log): the
  // 320-column layers with a long k and many pixels — the 3x3 convolutions of the 64x64 level: 320->320 0.67 -> 0.48 ms (181 -> 254 TF) from
  // fp32 operands, 0.57 -> 0.45 from planes; 960->320 1.62 -> 1.23 / 1.44 -> 1.29; train step +0.6 % (profiles/r03_ab_wgrad_wide.log).  With two or more 320-column tiles, short reductions or
  // few pixels it ties or loses against two 128 x 128 workgroups per CU (LDS read bytes per MFMA of a 32 x 160 wave tile), so those stay there.
  const bool wide = rows_ok && d.N == 320 && d.K >= 2560 && d.M >= 16384 && d.splits <= 0;
  // 128 x 128: two workgroups fit a CU (74 KB LDS), 512 slots; wide: one per CU, 256 slots
  const int tiles_n = wide ? d.N / 320 : (d.N + 127) / 128, tiles = ((d.K + 127) / 128) * tiles_n;
  int splits = d.splits > 0 ? d.splits : (wide ? best_split(tiles, d.M, 256, 3, 0.04) : best_split(tiles, d.M, 512, 4, 0.03));
  const int mps = pixels_per_split(d.M, splits);
  hipStream_t st = as_stream(stream);
  if (a_hi && b_hi) launch_wgrad<true, true>(d, wide, rows_ok, tiles, tiles_n, splits, mps, a_hi, a_lo, b_hi, b_lo, st);
  else if (a_hi) launch_wgrad<true, false>(d, wide, rows_ok, tiles, tiles_n, splits, mps, a_hi, a_lo, b_hi, b_lo, st);
  else if (b_hi) launch_wgrad<false, true>(d, wide, rows_ok, tiles, tiles_n, splits, mps, a_hi, a_lo, b_hi, b_lo, st);
  else launch_wgrad<false, false>(d, wide, rows_ok, tiles, tiles_n, splits, mps, a_hi, a_lo, b_hi, b_lo, st);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

extern "C" int ddpo_gemm_conv_wgrad_bf16x3(const ddpo_gemm_desc* dp, void* stream) {
  return wgrad_bf16x3(dp, nullptr, nullptr, nullptr, nullptr, stream);
}

/* Same contraction with one or both operands pre-split into bf16 hi / lo planes (NULL pair = that operand is fp32 in the descriptor):
 * a_* replace d->src (row stride d->ld_src ELEMENTS), dy_* replace d->w (row stride d->ld_w elements). */
extern "C" int ddpo_gemm_conv_wgrad_bf16x3_planes(const ddpo_gemm_desc* dp, const uint16_t* a_hi, const uint16_t* a_lo,
                                                  const uint16_t* dy_hi, const uint16_t* dy_lo, void* stream) {
  if (!a_hi && !dy_hi) return DDPO_EINVAL;
  return wgrad_bf16x3(dp, a_hi, a_lo, dy_hi, dy_lo, stream);
}
