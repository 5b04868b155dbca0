/* ddpo_optim.h — C ABI of the Adafactor update of libddpo_hip.so (gfx950), versioned on its own beside ddpo_hip.h.
 *
 * optax 0.1.5 `adafactor(learning_rate, weight_decay_rate=wd)` behind `clip_by_global_norm`, the second row of the reference's optimizer table
 * (pipeline/policy_gradient.py:132-145), every other argument at its default: scale_by_factored_rms(decay_rate 0.8, eps 1e-30,
 * min_dim_size_to_factor 128) -> clip_by_block_rms(1.0) -> scale by lr -> scale_by_param_block_rms(min_scale 1e-3) ->
 * add_decayed_weights(wd) -> p -= u.  DESIGN.md §4 (Adafactor) states the chain.
 * Conventions as in ddpo_hip.h: device pointers unless marked "host", `stream` is a hipStream_t passed as void*, no allocation, no
 * synchronisation; 0 on success, DDPO_EINVAL (-1) for a bad argument before anything is launched, DDPO_ELAUNCH (-2) for a rejected launch.
 */
#ifndef DDPO_OPTIM_H
#define DDPO_OPTIM_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Rows of a factored matrix one work item covers, and elements of an unfactored tensor one work item covers. */
#define DDPO_ADAFACTOR_TILE_ROWS 128
#define DDPO_ADAFACTOR_CHUNK 4096

/* One trainable tensor of the flat parameter / gradient buffers.
 * Factored (both of its two largest axes >= min_dim_size_to_factor, and they are its last two): S contiguous slabs of an R x C row-major
 * matrix; the state holds per slab R row statistics (means over the columns) at v_off and C column statistics (means over the rows) at
 * vc_off.  optax calls "v_row" the statistics left after reducing the LARGEST axis: the row statistics when C >= R (norm_rows = 1), the
 * column statistics otherwise; that vector is the one divided by its mean.
 * Unfactored: S = R = 1, C = numel; the state holds numel floats at v_off.
 * Work items are (tensor, tile) pairs.  Factored: tile = slab * ceil(R / TILE_ROWS) + row tile.  Unfactored: tile = chunk of CHUNK elements. */
typedef struct {
  int64_t off;        /* first element in p / g */
  int64_t numel;      /* S * R * C */
  int64_t v_off;      /* state offset, floats */
  int64_t vc_off;     /* state offset of the column statistics (factored) */
  int64_t ws_off;     /* factored: this tensor's region of the workspace, floats after the workspace header */
  int32_t S, R, C;
  int32_t factored;   /* 0 | 1 */
  int32_t norm_rows;  /* 0 | 1 */
  int32_t first_tile; /* tiles are numbered over the table: this tensor's are first_tile .. first_tile + n_tiles - 1 */
  int32_t n_tiles;
  int32_t reserved;   /* 0 */
} ddpo_adafactor_tensor;

int ddpo_optim_abi_version(void);               /* 1 */
size_t ddpo_sizeof_adafactor_tensor(void);      /* binding self-check */

/* Bytes of workspace ddpo_adafactor_step needs for this plan, or 0 if the plan is inconsistent: a tensor outside [0, n) of the flat
 * buffer or [0, n_state) of the state, overlapping workspace regions, a work list that does not name every tile of every tensor
 * exactly once (in any order: the builder puts the largest first), a slab list (work[n_tiles .. n_tiles + n_slabs), pairs (tensor, slab)) that does not enumerate every slab of every factored
 * tensor.  Both arrays are HOST copies of what the step is given on the device; the step itself cannot read them. */
size_t ddpo_adafactor_workspace_bytes(const ddpo_adafactor_tensor* tensors_host, int n_tensors, const int32_t* work_host, int n_tiles,
                                      int n_slabs, int64_t n, int64_t n_state);

/* One update, in place, as five launches whatever the tensor count: (1) per row tile the row sums and per-tile column sums of g'^2 + eps,
 * and v of the unfactored tensors; (2) per slab v_row / v_col and the two ^(-1/2) factor vectors; (3) per tile sum u^2 and sum p^2;
 * (4) per tensor the block-RMS clip and the parameter scale; (5) p -= u, g = 0 if zero_grad.
 * g' = g * inv_n_acc, clipped to max_grad_norm by sqrt(*sqnorm_of_sum) * inv_n_acc exactly as ddpo_adamw_bf16mu_step does
 * (sqnorm_of_sum: the device double ddpo_grad_sqnorm wrote).  beta_t = 1 - (count + 1)^(-0.8) in float32 (0 on the first update).
 * Every reduction is a fixed-order sum of per-tile partials held in the workspace: no floating-point atomics, bit-identical from run to run.
 * p, g: n floats, 16-byte aligned.  state: the floats the table's v_off / vc_off address.  tensors / work: device copies of the validated plan. */
int ddpo_adafactor_step(float* p, float* g, float* state, const ddpo_adafactor_tensor* tensors, int n_tensors, const int32_t* work,
                        int n_tiles, int n_slabs, int64_t n, const double* sqnorm_of_sum, double inv_n_acc, double lr, double beta_t,
                        double eps, double clipping_threshold, double min_scale, double weight_decay, double max_grad_norm, int zero_grad,
                        void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
