// Internal (non-ABI) helpers shared between the kernel translation units.
#pragma once
#include <algorithm>
#include "vsrk_common.h"

// Per-channel sum (mode 0) or sum + sum of squares (mode 1) over every voxel of
// a view; perm_r maps view channel -> torch channel.  Needs workspace of
// vsrk_channel_reduce_ws_bytes(c) bytes.
size_t vsrk_channel_reduce_ws_bytes(int c);
int vsrk_channel_reduce_internal(const vsrk_tensor5* x, int mode, int perm_r, float scale, float* sum,
                                 float* sumsq, int accumulate, void* ws, size_t ws_bytes, hipStream_t s);

// bf16 fast path of vsrk_conv_fwd (conv_fast.hip): 1 = launched, 0 = not
// eligible (use the generic kernel), < 0 = -(error status).
int vsrk_conv_fwd_fast(const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed, const float* bias,
                       const float* pro_scale, const float* pro_shift, const vsrk_tensor5* residual,
                       const vsrk_tensor5* mask, const vsrk_tensor5* y, hipStream_t s);
// thin-channel path of vsrk_conv_fwd (conv_thin.hip): cin <= 4 or cout <= 3;
// same return convention.
// one-input-channel 3x3 stencil (conv_stencil.hip): 1 = launched, 0 = not eligible, < 0 = -(error status)
int vsrk_conv_fwd_stencil(const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed, const float* bias,
                          const vsrk_tensor5* residual, const vsrk_tensor5* mask, const vsrk_tensor5* y,
                          hipStream_t s);
int vsrk_conv_fwd_stencil_out(const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed,
                              const float* bias, const vsrk_tensor5* residual, const vsrk_tensor5* mask,
                              const vsrk_tensor5* y, hipStream_t s);
int vsrk_conv_fwd_thin(const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed, const float* bias,
                       const float* pro_scale, const float* pro_shift, const vsrk_tensor5* residual,
                       const vsrk_tensor5* mask, const vsrk_tensor5* y, hipStream_t s);

// rolling-depth 16-bit Conv3d 3x3x3 (conv_roll.hip): forward / data gradient;
// same return convention; VSRK_PATH_ROLL: 0 off, 1 forced on, 2 automatic
// slope_ws != nullptr (2-D forms): mask is a PReLU output y_fwd with y's
// geometry and strides, desc->mask_slope its slope a: out = conv * (y_fwd > 0 ?
// 1 : a) and per-lane partials of sum_{y_fwd < 0} out * y_fwd into slope_ws
// (vsrk_roll_slope_ws_floats() floats); *slope_blocks = the grid.
// bnred (3-D form, no epilogue operands): the fused BN+ReLU backward reduce
// (bnx with y's geometry and strides; ws >= ntiles * 8 * 64 floats); on
// launch ntiles / ntn are filled for roll_bnred_final.
struct vsrk_roll_bnred {
  const vsrk_tensor5* bnx;
  const float *scale, *shift, *mean, *invstd;
  float* ws;
  size_t ws_floats;
  int ntiles, ntn;
};
// a fused PReLU backward's slope-gradient partials (one double per wave,
// vsrk_wave_sum) and their capacity; vsrk_slope_final sums them into *da
struct vsrk_slope_out {
  double* part;
  size_t cap;     // doubles
  int* nparts;    // out: partials written
};
void vsrk_slope_final(const double* part, int nparts, const float* a, float* da, int accumulate, int pre,
                      hipStream_t s);
int vsrk_conv_fwd_roll(const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed, const float* bias,
                       const float* pro_scale, const float* pro_shift, const vsrk_tensor5* residual,
                       const vsrk_tensor5* mask, const vsrk_tensor5* y, hipStream_t s,
                       const vsrk_slope_out* slope = nullptr, vsrk_roll_bnred* bnred = nullptr);
// the fused reduce's final per-channel sums (roll_bnred_final_kernel)
int vsrk_roll_bnred_final(const vsrk_roll_bnred& r, int cout, float* sum_dy, float* sum_dy_xhat, hipStream_t s);
size_t vsrk_roll_bnred_ws_floats(const vsrk_tensor5* y);
size_t vsrk_roll_slope_ws_bytes();
// the depth-folded rolling forward (conv_roll_fold.hip: conv_roll_impl.h's
// kernel built with 32-row tiles): one output depth from three slices; 1
// launched, 0 not eligible, < 0 -(error status)
int vsrk_conv_fwd_roll_fold(const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed, const float* bias,
                            const float* pro_scale, const float* pro_shift, const vsrk_tensor5* y, hipStream_t s);

// row-walking 16-bit Conv 3x3 64 -> 64 (conv_row.hip): forward / data gradient
// of EDSR's body convs, reached from conv_roll.hip's 2-D branch after its
// checks; 1 launched, 0 not eligible, < 0 -(error status).
// VSRK_PATH_ROW: -1 default (VSRK_CONV_ROW unset: the forms that measured
// faster than the tile kernel), 0 off, 1 every form
int vsrk_conv_fwd_row(const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed, const float* bias,
                      const vsrk_tensor5* residual, const vsrk_tensor5* mask, const vsrk_tensor5* y, hipStream_t s);

// row-walking 16-bit Conv 3x3 64 -> 256 through a shuffle-2 output view
// (conv_row_wide.hip): forward of EDSR's up-sampler convs, reached from
// conv_roll.hip's sub-pixel output branch after its checks; same return
// convention.  vsrk_g_row_wide_mode (vsrk_conv_set_row_wide, conv_paths.hip): -1
// default (VSRK_CONV_ROW_WIDE unset: the shapes that measured faster than the
// tile kernel), 0 off, 1 every shape
extern int vsrk_g_row_wide_mode;
int vsrk_conv_fwd_row_wide(const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed, const float* bias,
                           const vsrk_tensor5* residual, const vsrk_tensor5* mask, const vsrk_tensor5* y,
                           hipStream_t s);

// pointwise (1x1x1) bf16 conv (conv_pw.hip): forward / data gradient; same
// return convention (its weight gradient: conv_wgrad.h)
int vsrk_conv_fwd_pw(const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed, const float* bias,
                     const float* pro_scale, const float* pro_shift, const vsrk_tensor5* residual,
                     const vsrk_tensor5* mask, const vsrk_tensor5* y, hipStream_t s);
// wide pointwise convs (conv_pw_wide.hip: > 256 input channels or 256 -> >= 256)
int vsrk_conv_fwd_pw_wide(const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed, const float* bias,
                          const vsrk_tensor5* residual, const vsrk_tensor5* mask, const vsrk_tensor5* y,
                          hipStream_t s);
int vsrk_conv_fwd_pw_pbwd(const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed,
                          const vsrk_tensor5* mask, const vsrk_tensor5* y, int c_lo, const vsrk_slope_out* slope,
                          hipStream_t s);
size_t vsrk_pw_pbwd_ws_bytes();

// ---- dispatch state (conv_paths.hip) ----
// One mode per kernel family, resolved from the family's environment variable
// when the library is loaded and changed only by vsrk_conv_set_path (the table
// of names, variables and defaults is in conv_paths.hip): 0 off, 1 on; roll /
// wgrad_roll 2 = automatic; roll_wr / wgrad_row 2 = the extra forms; row -1 =
// the per-form default.  Process-wide test / A-B switches: set between
// launches, never concurrently with them.
enum vsrk_path {
  VSRK_PATH_FAST,
  VSRK_PATH_PW,
  VSRK_PATH_PW_WIDE,
  VSRK_PATH_ROLL,
  VSRK_PATH_ROLL_WR,
  VSRK_PATH_ROLL_FOLD,
  VSRK_PATH_ROW,
  VSRK_PATH_THIN,
  VSRK_PATH_STENCIL,
  VSRK_PATH_WGRAD_PIPE,
  VSRK_PATH_WGRAD_ROLL,
  VSRK_PATH_WGRAD_ROW,
  VSRK_PATH_COUNT
};
extern int vsrk_g_path_mode[VSRK_PATH_COUNT];
static inline int vsrk_path_mode(vsrk_path p) { return vsrk_g_path_mode[p]; }
// environment helpers for the secondary A/B knobs, which are file-scope consts
// initialised at load next to the code that uses them.  flag: unset = dflt, a
// value starting with '0' = 0, any other value = 1.  int: unset = dflt, else atoi.
int vsrk_env_flag(const char* name, int dflt);
int vsrk_env_int(const char* name, int dflt);
// CUs of the current device at the first call (256 when the query fails)
int vsrk_num_cus();
// VSRK_ROLL_PRIO=1 (A/B): s_setprio 1 for waves 4-7 of conv_roll and conv_wgrad_roll
extern const int vsrk_g_roll_prio;
// vsrk_conv_set_roll_depth: > 0 output depths per tile of both rolling kernels
extern int vsrk_g_roll_dz;
// vsrk_conv_set_grid_cap: > 0 caps the workgroups of the persistent conv grids
// and of the weight-gradient split (tests drive the multi-tile loops with it)
extern int vsrk_g_grid_cap;
static inline int64_t vsrk_capped_grid(int64_t g) {
  return vsrk_g_grid_cap > 0 ? std::max<int64_t>(1, std::min<int64_t>(g, vsrk_g_grid_cap)) : g;
}
