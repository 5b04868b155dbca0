// Operand packers of the bf16 / f16mx GEMM family (gemm_bf16.hip): folded up-sampler weights, fp32 weights -> bf16 hi / lo planes (row-major,
// k-blocked, data-gradient order), fp32 activations -> bf16 / f16mx planes, f16mx weight planes with their per-column E8M0 scales.
#include "common.h"

// The four phase kernels (2, 2, Cin, Cout) of a 3x3 HWIO kernel w (3, 3, Cin, Cout): wf[(py 2 + px)][ty][tx] = the sum, in fp32, ky then kx
// ascending, of w[ky][kx] over the taps that land on source offset (ty - 1 + py, tx - 1 + px).  cn = Cin * Cout.
__global__ void __launch_bounds__(256) fold_up2x_weights_kernel(const float* __restrict__ w, int64_t cn, float* __restrict__ wf) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= cn) return;
  float v[3][3];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) v[ky][kx] = w[(ky * 3 + kx) * cn + i];
#pragma unroll
  for (int ph = 0; ph < 4; ++ph)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int py = ph >> 1, px = ph & 1, ty = t >> 1, tx = t & 1;
      const int y0 = py ? (ty ? 2 : 0) : (ty ? 1 : 0), y1 = py ? (ty ? 2 : 1) : (ty ? 2 : 0);
      const int x0 = px ? (tx ? 2 : 0) : (tx ? 1 : 0), x1 = px ? (tx ? 2 : 1) : (tx ? 2 : 0);
      float sum = 0.f;
      bool first = true;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          if (ky < y0 || ky > y1 || kx < x0 || kx > x1) continue;
          sum = first ? v[ky][kx] : sum + v[ky][kx];
          first = false;
        }
      wf[(ph * 4 + t) * cn + i] = sum;
    }
}
extern "C" int ddpo_fold_up2x_weights(const float* w, int Cin, int Cout, float* wf, void* stream) {
  if (!w || !wf || Cin <= 0 || Cout <= 0) return DDPO_EINVAL;
  const int64_t cn = (int64_t)Cin * Cout;
  hipLaunchKernelGGL(fold_up2x_weights_kernel, dim3((unsigned)((cn + 255) / 256)), dim3(256), 0, as_stream(stream), w, cn, wf);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

// ------------------------------------------------------------------------------------------------
// weight packing: fp32 W[K][N] -> bf16 hi/lo planes, forward order [N][Kp] (k contiguous, Kp = K rounded up to 8,
// pad zero) and backward order [K][N] (the original order).  32x32 LDS-tiled transpose.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) pack_weights_kernel(const float* __restrict__ w, int K, int N, int Kp,
                                                           uint16_t* __restrict__ fwd_hi, uint16_t* __restrict__ fwd_lo,
                                                           uint16_t* __restrict__ bwd_hi, uint16_t* __restrict__ bwd_lo) {
  __shared__ uint32_t tile[32][33];      // hi | lo<<16
  const int k0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int k = k0 + r, n = n0 + tx;
    uint32_t packed = 0;
    if (k < K && n < N) {
      const float x = w[(int64_t)k * N + n];
      const uint32_t h = cvt_pk_bf16(x, 0.f) & 0xFFFFu;
      const float rem = x - __uint_as_float(h << 16);
      const uint32_t l = cvt_pk_bf16(rem, 0.f) & 0xFFFFu;
      packed = h | (l << 16);
      if (bwd_hi) { bwd_hi[(int64_t)k * N + n] = (uint16_t)h; bwd_lo[(int64_t)k * N + n] = (uint16_t)l; }
    }
    tile[r][tx] = packed;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int n = n0 + r, k = k0 + tx;
    if (n < N && k < Kp) {
      const uint32_t p = tile[tx][r];
      fwd_hi[(int64_t)n * Kp + k] = (uint16_t)(p & 0xFFFFu);
      fwd_lo[(int64_t)n * Kp + k] = (uint16_t)(p >> 16);
    }
  }
}

// k-blocked forward planes (Kb = ceil(K / 32), N, 32): same 32x32 tile transpose, the tile of k-block kb lands at [kb][n0 .. n0+31][0..31]
__global__ void __launch_bounds__(256) pack_weights_kblocked_kernel(const float* __restrict__ w, int K, int N, uint16_t* __restrict__ fwd_hi,
                                                                    uint16_t* __restrict__ fwd_lo) {
  __shared__ uint32_t tile[32][33];
  const int kb = blockIdx.y, k0 = kb * 32, n0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int k = k0 + r, n = n0 + tx;
    uint32_t packed = 0;
    if (k < K && n < N) {
      const float x = w[(int64_t)k * N + n];
      const uint32_t h = cvt_pk_bf16(x, 0.f) & 0xFFFFu;
      const float rem = x - __uint_as_float(h << 16);
      packed = h | ((cvt_pk_bf16(rem, 0.f) & 0xFFFFu) << 16);
    }
    tile[r][tx] = packed;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int n = n0 + r;
    if (n < N) {
      const uint32_t p = tile[tx][r];
      const int64_t o = ((int64_t)kb * N + n) * 32 + tx;
      fwd_hi[o] = (uint16_t)(p & 0xFFFFu);
      fwd_lo[o] = (uint16_t)(p >> 16);
    }
  }
}

extern "C" int ddpo_pack_weights_bf16_kblocked(const float* w, int K, int N, uint16_t* fwd_hi, uint16_t* fwd_lo, void* stream) {
  if (!w || !fwd_hi || !fwd_lo || K <= 0 || N <= 0) return DDPO_EINVAL;
  dim3 grid((N + 31) / 32, (K + 31) / 32);
  hipLaunchKernelGGL(pack_weights_kblocked_kernel, grid, dim3(256), 0, as_stream(stream), w, K, N, fwd_hi, fwd_lo);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

// Data-gradient planes straight from the forward kernel w (taps, Cin, Cout) (HWIO flattened; dense: taps = 1): the forward-style operand of
// dX = dY * W' is W'[k'][n'] = w[taps - 1 - tap'][n'][co] with k' = tap' * Cout + co (taps flipped, channels transposed), K' = taps * Cout rows,
// N' = Cin columns.  For a fixed column n' consecutive k' are consecutive co: the reads are contiguous along the same index the k-blocked
// layout stores contiguously, so no LDS transpose is needed (one thread per element: lanes along k').  Replaces the flip / permute /
// contiguous copy torch made of every contraction weight after every optimizer update.
__global__ void __launch_bounds__(256) pack_weights_kblocked_dgrad_kernel(const float* __restrict__ w, int taps, int Cin, int Cout,
                                                                          uint16_t* __restrict__ hi, uint16_t* __restrict__ lo) {
  const int kb = blockIdx.y, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int Kd = taps * Cout;
  const int k = kb * 32 + tx;
  const bool kok = k < Kd;
  const int tap = kok ? k / Cout : 0, co = k - tap * Cout;
  const float* src = w + ((int64_t)(taps - 1 - tap) * Cin) * Cout + co;
  for (int r = ty; r < 32; r += 8) {
    const int n = blockIdx.x * 32 + r;
    if (n >= Cin) continue;
    uint32_t h = 0, l = 0;
    if (kok) {
      const float x = src[(int64_t)n * Cout];
      h = cvt_pk_bf16(x, 0.f) & 0xFFFFu;
      l = cvt_pk_bf16(x - __uint_as_float(h << 16), 0.f) & 0xFFFFu;
    }
    const int64_t o = ((int64_t)kb * Cin + n) * 32 + tx;
    hi[o] = (uint16_t)h;
    lo[o] = (uint16_t)l;
  }
}
extern "C" int ddpo_pack_weights_bf16_kblocked_dgrad(const float* w, int taps, int Cin, int Cout, uint16_t* hi, uint16_t* lo, void* stream) {
  if (!w || !hi || !lo || taps <= 0 || Cin <= 0 || Cout <= 0) return DDPO_EINVAL;
  dim3 grid((Cin + 31) / 32, (taps * Cout + 31) / 32);
  hipLaunchKernelGGL(pack_weights_kblocked_dgrad_kernel, grid, dim3(256), 0, as_stream(stream), w, taps, Cin, Cout, hi, lo);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

extern "C" int ddpo_pack_weights_bf16(const float* w, int K, int N, int Kp, uint16_t* fwd_hi, uint16_t* fwd_lo, uint16_t* bwd_hi,
                                      uint16_t* bwd_lo, void* stream) {
  if (!w || !fwd_hi || !fwd_lo || K <= 0 || N <= 0 || Kp < K || (Kp & 7) || (bwd_hi && !bwd_lo)) return DDPO_EINVAL;
  dim3 grid((N + 31) / 32, (Kp + 31) / 32);
  hipLaunchKernelGGL(pack_weights_kernel, grid, dim3(256), 0, as_stream(stream), w, K, N, Kp, fwd_hi, fwd_lo, bwd_hi, bwd_lo);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

// ------------------------------------------------------------------------------------------------
// fp32 activations (rows, cols) with row stride ldx -> bf16 hi / lo planes (rows, ld_out): the operand format of
// ddpo_gemm_conv_fwd_bf16_planes.  Stand-alone form of what the normalisation kernels do in their output stage
// (same v_cvt_pk_bf16_f32 split as the GEMM loader: the planes hold exactly the bits the loader would have produced).
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) split_planes_kernel(const float* __restrict__ x, int ldx, uint16_t* __restrict__ hi,
                                                           uint16_t* __restrict__ lo, int ld_out, int64_t rows, int cols4) {
  const int64_t total = rows * cols4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cols4;
    const int c = (int)(i - r * cols4) << 2;
    uint2 h, l;
    split4(*reinterpret_cast<const float4*>(x + r * ldx + c), h, l);
    const int64_t o = plane_off(r, c, ld_out, rows);
    *reinterpret_cast<uint2*>(hi + o) = h;
    *reinterpret_cast<uint2*>(lo + o) = l;
  }
}

extern "C" int ddpo_split_planes_bf16(const float* x, int ldx, uint16_t* hi, uint16_t* lo, int ld_out, int64_t rows, int cols, void* stream) {
  if (!x || !hi || !lo || rows <= 0 || cols <= 0 || (cols & 3) || (ldx & 3) || (ld_out & 3) || ldx < cols) return DDPO_EINVAL;
  if (ld_out == 0 ? (cols & 31) != 0 : ld_out < cols) return DDPO_EINVAL;          // ld_out == 0: k-blocked planes (cols / 32, rows, 32)
  if ((reinterpret_cast<uintptr_t>(x) & 15) || ((reinterpret_cast<uintptr_t>(hi) | reinterpret_cast<uintptr_t>(lo)) & 7)) return DDPO_EINVAL;
  int64_t blocks = (rows * (cols >> 2) + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(split_planes_kernel, dim3((int)blocks), dim3(256), 0, as_stream(stream), x, ldx, hi, lo, ld_out, rows, cols >> 2);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

__global__ void __launch_bounds__(256) split_planes_mx_kernel(const float* __restrict__ x, int ldx, uint16_t* __restrict__ p16,
                                                              uint16_t* __restrict__ p8, int ld_out, int64_t rows, int cols4) {
  const int64_t total = rows * cols4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cols4;
    const int c = (int)(i - r * cols4) << 2;
    mx_store4(p16, p8, r, c, ld_out, rows, *reinterpret_cast<const float4*>(x + r * ldx + c));
  }
}

extern "C" int ddpo_split_planes_f16mx(const float* x, int ldx, uint16_t* p16, uint16_t* p8, int ld_out, int64_t rows, int cols, void* stream) {
  if (!x || !p16 || !p8 || rows <= 0 || cols <= 0 || (cols & 31) || (ldx & 3) || (ld_out & 31) || ldx < cols) return DDPO_EINVAL;
  if (ld_out != 0 && ld_out < cols) return DDPO_EINVAL;
  if ((reinterpret_cast<uintptr_t>(x) & 15) || ((reinterpret_cast<uintptr_t>(p16) | reinterpret_cast<uintptr_t>(p8)) & 7)) return DDPO_EINVAL;
  int64_t blocks = (rows * (cols >> 2) + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(split_planes_mx_kernel, dim3((int)blocks), dim3(256), 0, as_stream(stream), x, ldx, p16, p8, ld_out, rows, cols >> 2);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

// f16mx weight planes (include/ddpo_hip.h).  Pass 1 (a, b): biased exponent of every column's largest |w| -> scale byte; pass 2: the 32x32
// tile transpose of the k-blocked packer, writing the f16 plane and the [l8 | h8] byte plane.
// pass 1a: biased exponent of every column's largest |w|.  64 columns x 4 k-lanes per workgroup, the reduction split over blockIdx.y chunks of k
// and combined with atomicMax on the (non-negative) fp32 bit patterns in a caller-provided uint32 scratch (N words, zeroed).
__global__ void __launch_bounds__(256) mx_colmax_kernel(const float* __restrict__ w, int K, int N, int k_per_block, uint32_t* __restrict__ colmax) {
  __shared__ uint32_t red[4][64];
  const int c = threadIdx.x & 63, kl = threadIdx.x >> 6;
  const int n = blockIdx.x * 64 + c;
  const int k0 = blockIdx.y * k_per_block, k1 = min(K, k0 + k_per_block);
  uint32_t m = 0;
  if (n < N)
    for (int k = k0 + kl; k < k1; k += 4) m = max(m, __float_as_uint(w[(int64_t)k * N + n]) & 0x7FFFFFFFu);
  red[kl][c] = m;
  __syncthreads();
  if (kl == 0 && n < N) {
    m = max(max(red[0][c], red[1][c]), max(red[2][c], red[3][c]));
    if (m) atomicMax(colmax + n, m);
  }
}
// pass 1b: scale byte
__global__ void __launch_bounds__(256) mx_colscale_kernel(const uint32_t* __restrict__ colmax, int N, uint8_t* __restrict__ scale) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  int e = (int)(colmax[n] >> 23);         // 2^(e - 127) <= max|w| < 2^(e - 126)
  e = min(max(e, 32), 240);               // all-zero / denormal columns: any valid scale; keeps (byte - 11) and 2^(261 - e) in range
  scale[n] = (uint8_t)(e - 7);            // max|w| / 2^(e - 7 - 127) in [128, 256) <= 448 (e4m3 range)
}
__global__ void __launch_bounds__(256) pack_weights_mx_kernel(const float* __restrict__ w, int K, int N, const uint8_t* __restrict__ scale,
                                                              uint16_t* __restrict__ w16, uint8_t* __restrict__ w8) {
  __shared__ uint32_t tile[32][33];       // f16 bits | h8 << 16 | l8 << 24
  const int kb = blockIdx.y, k0 = kb * 32, n0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int k = k0 + r, n = n0 + tx;
    uint32_t packed = 0;
    if (k < K && n < N) {
      const float x = fminf(fmaxf(w[(int64_t)k * N + n], -65504.f), 65504.f);
      const _Float16 h = (_Float16)x;
      const float hf = (float)h, inv = __uint_as_float((uint32_t)(254 - (int)scale[n]) << 23);       // 2^-(byte - 127)
      const int p = __builtin_amdgcn_cvt_pk_fp8_f32(hf * inv, (x - hf) * 2048.f * inv, 0, false);
      packed = (uint32_t)__builtin_bit_cast(uint16_t, h) | ((uint32_t)p << 16);
    }
    tile[r][tx] = packed;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int n = n0 + r;
    if (n < N) {
      const uint32_t p = tile[tx][r];
      const int64_t row = (int64_t)kb * N + n;
      w16[row * 32 + tx] = (uint16_t)(p & 0xFFFFu);
      const int o = 2 * (tx & 16) + (tx & 15);              // chunks [l8 k0-15 | h8 k0-15 | l8 k16-31 | h8 k16-31]
      w8[row * 64 + o] = (uint8_t)(p >> 24);                // l8 first: lane half 0 of the MFMA pairs it with the activations' h8
      w8[row * 64 + o + 16] = (uint8_t)((p >> 16) & 0xFFu);
    }
  }
}
extern "C" int ddpo_pack_weights_f16mx(const float* w, int K, int N, uint16_t* w16, uint16_t* w8, uint8_t* scale, void* stream) {
  if (!w || !w16 || !w8 || !scale || K <= 0 || N <= 0) return DDPO_EINVAL;
  // the column maxima are gathered in the first N words of the f16 plane (>= 64 bytes per column; overwritten by the pack pass below)
  uint32_t* colmax = reinterpret_cast<uint32_t*>(w16);
  if (hipMemsetAsync(colmax, 0, (size_t)N * sizeof(uint32_t), as_stream(stream)) != hipSuccess) return DDPO_ELAUNCH;
  int ky = (K + 255) / 256;
  if (ky > 128) ky = 128;
  const int kpb = ((K + ky - 1) / ky + 3) / 4 * 4;
  hipLaunchKernelGGL(mx_colmax_kernel, dim3((N + 63) / 64, (K + kpb - 1) / kpb), dim3(256), 0, as_stream(stream), w, K, N, kpb, colmax);
  DDPO_LAUNCH_CHECK();
  hipLaunchKernelGGL(mx_colscale_kernel, dim3((N + 255) / 256), dim3(256), 0, as_stream(stream), colmax, N, scale);
  DDPO_LAUNCH_CHECK();
  hipLaunchKernelGGL(pack_weights_mx_kernel, dim3((N + 31) / 32, (K + 31) / 32), dim3(256), 0, as_stream(stream), w, K, N, scale, w16,
                     reinterpret_cast<uint8_t*>(w8));
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}
