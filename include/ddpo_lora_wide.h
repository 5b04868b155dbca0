/* ddpo_lora_wide.h — C ABI of the adapter gradients of WIDE LoRA layers (the GEGLU feed-forward layers, `--lora_targets attn_ff`) of
 * libddpo_hip.so (gfx950), versioned on its own beside ddpo_hip.h like ddpo_dpo.h.
 *
 * ddpo_lora_wgrad (ddpo_hip.h) stages the A / B slice of a whole layer in LDS and keeps every column of the layer in registers, which
 * bounds it to K <= 2048, N <= 2048, K + N <= 4064.  The entry here computes the same thing for K, N up to 16384:
 *   dA (K, r) += s * x^T (dY B^T)
 *   dB (r, N) += s * (x A)^T dY
 * for y = x (W0 + s A B), x (M, K), dY (M, N), A (K, r), B (r, N), in three launches:
 *   (1) u = dY B^T and v = x A (M x r each, padded to a multiple of 4 ranks) into the workspace: per 16 rows and rank slice of 4, 16 lanes
 *       per row on a fixed column stride over column tiles of 1024 staged in LDS, joined by the 16-lane butterfly ^8, ^4, ^2, ^1;
 *   (2) per (row group, rank slice of 4, column tile of 1024 of K or of N): acc[k][j] += x[m, k] u[m][j] resp. acc[n][j] += v[m][j] dY[m, n],
 *       m ascending over the row group's contiguous rows; every workgroup writes its part of the row group's partial slab;
 *   (3) one wave per output sums the row groups' slabs (lane l: groups l, l + 64, ... ascending, then the 64-lane butterfly) and adds
 *       s * sum to dA / dB.
 * fp32 accumulation, fixed summation orders, no float atomics: bit-identical from launch to launch and under graph replay.
 * Conventions as in ddpo_hip.h: device pointers, `stream` is a hipStream_t passed as void*, no allocation, no synchronisation; 0 on success,
 * DDPO_EINVAL (-1) for a bad argument before anything is launched (dA / dB untouched), DDPO_ELAUNCH (-2) for a rejected launch.
 */
#ifndef DDPO_LORA_WIDE_H
#define DDPO_LORA_WIDE_H
#include <stddef.h>
#include <stdint.h>
#include "ddpo_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

int ddpo_lora_wide_abi_version(void);           /* 1 */

/* Bytes of workspace ddpo_lora_wgrad_wide needs for this shape (u, v and the partial slabs); 0 for a shape it refuses. */
size_t ddpo_lora_wgrad_wide_ws_bytes(int M, int K, int N, int r);

/* The argument list of ddpo_lora_wgrad.  x: fp32 rows (row stride ldx >= K, 16-byte aligned), or NULL and bf16 hi / lo planes x = hi + lo:
 * row-major with row stride ld_planes >= K, or k-blocked (K / 32, M, 32) when ld_planes == 0 (needs K % 32 == 0).  dY: fp32 rows, row stride
 * lddy >= N.  A (K, r), B (r, N), dA, dB contiguous.  ws: 16-byte aligned, ws_bytes >= ddpo_lora_wgrad_wide_ws_bytes(M, K, N, r).
 * DDPO_EINVAL: a NULL pointer, M < 1, K or N < 4, not a multiple of 4 or > 16384, r outside 1..64, a row stride below the row length or not
 * a multiple of 4, a misaligned x / dY / ws / plane pointer, a short workspace.  All of these are checked on the host. */
int ddpo_lora_wgrad_wide(const float* x, int ldx, const uint16_t* x_hi, const uint16_t* x_lo, int ld_planes, const float* dy, int lddy,
                         const float* A, const float* B, float* dA, float* dB, int M, int K, int N, int r, float s, void* ws,
                         size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
