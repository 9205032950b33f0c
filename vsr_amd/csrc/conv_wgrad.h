// The weight-gradient family: what vsrk_conv_wgrad (conv_wgrad.hip) routes
// between, and the one slab layout and reduce behind every kernel but the
// pointwise one.
//
// A candidate kernel answers a request with "not eligible" or with a plan: its
// launch geometry and a WgradSlabs saying what it will leave in the workspace.
// vsrk_conv_wgrad launches the first eligible candidate (pw, roll, roll in
// sample chunks, row, generic) and hands its WgradSlabs to wgrad_reduce;
// vsrk_conv_wgrad_workspace_size is the maximum ws_bytes over the same list.
// Eligibility never depends on the workspace passed: one too small for the
// chosen candidate is an error.
#pragma once
#include "conv_common.h"

struct WgradSlabs {      // what a slab kernel leaves in the workspace: [nsplit][combo][slab] floats
  int nsplit;            // slabs per combo, summed in index order (deterministic)
  int slab;              // floats per slab: [tap = kh * kw][cot_w][cit_w] weights, then cot_w dbias sums
  int kd, kh, kw;        // kernel extent: kd * nci_t * nco_t combos of kh * kw taps
  int nco_t, nci_t;      // combo = (kdi * nci_t + ci / cit_w) * nco_t + co / cot_w
  int cot_w, cit_w;      // output / input channels per combo (the last may run past cout / cin: not read)
  int kd_bias;           // the kd plane whose slabs (of input block 0) carry the dbias tail
  bool rows_ok;          // the row-order reduce may be taken (false: the rolling-row kernel's slabs)
  int ncombos() const { return kd * nci_t * nco_t; }
  size_t ws_bytes() const { return (size_t)nsplit * ncombos() * slab * sizeof(float); }
};

// dw[co][ci][kd][kh][kw] (torch, fp32) (+)= scale * sum over splits of the
// slabs, and db (when not null) from the dbias tails; perm_r > 1 maps a
// sub-pixel view's output channel to torch's (conv_wgrad_reduce.hip).
int wgrad_reduce(const WgradSlabs& sl, const float* ws, int cout, int cin, int perm_r, float scale, int accumulate,
                 float* dw, float* db, hipStream_t s);

namespace vsrk_conv {
// Kernel arguments of the generic plan (conv_wgrad.hip): the generic,
// pipelined and thin kernels
struct WgradArgs {
  View x, dy;
  const float* pro_scale;
  const float* pro_shift;
  float* ws;
  int cin, cout;
  int kd, kh, kw, pd, ph, pw;
  int prologue, xvec, dyvec;
  int tiles_h, tiles_w, ntiles, tiles_per_split, nsplit, ncombos, nblk;
  int n_ci_chunks, n_co_tiles, kd_bias, slab, want_bias, cin_pad;
  // sub-pixel weight (desc->subpixel): taps with a nonzero weight per
  // 32-channel block of the shuffled operand (dy: sp_by 1, x: sp_by 2);
  // the others' gradients are structurally discarded (vsrk_subpixel_wgrad_fold)
  int sp_by;
  uint16_t sptap[64];
};
}  // namespace vsrk_conv

// pointwise (1x1x1) 16-bit weight gradient (conv_pw.hip), with slabs and a
// reduce of its own (eight split groups where wgrad_reduce sums four):
// workspace 0 = not eligible; launch 1 = launched kernel and reduce, 0 = not
// eligible, < 0 = -(error status)
size_t vsrk_conv_wgrad_pw_workspace(const vsrk_conv_desc* d, const vsrk_tensor5* x, const vsrk_tensor5* dy);
int vsrk_conv_wgrad_pw(const vsrk_conv_desc* d, const vsrk_tensor5* x, const vsrk_tensor5* dy,
                       const float* pro_scale, const float* pro_shift, float dy_scale, int32_t perm_r, float* dw,
                       float* dbias, int32_t accumulate, void* workspace, size_t workspace_bytes, hipStream_t s);

// rolling-depth 16-bit Conv3d 3x3x3 weight gradient (conv_wgrad_roll.hip):
// plan (false = not eligible) and the launch of a plan's slab kernel
struct VsrkRollPlan {
  int nsplit, tps, ntiles, dzc;  // workgroups per channel block, tiles per workgroup, tiles, depths per tile
  WgradSlabs slabs;
};
bool vsrk_wgrad_roll_plan(const vsrk_conv_desc* d, const vsrk_tensor5* x, const vsrk_tensor5* dy, VsrkRollPlan* p);
void vsrk_conv_wgrad_roll(const vsrk_conv_desc* d, const vsrk_tensor5* x, const vsrk_tensor5* dy,
                          const float* pro_scale, const float* pro_shift, int want_bias, float* ws,
                          const VsrkRollPlan& p, hipStream_t s);

// rolling-row 16-bit Conv2d 3x3 weight gradient (conv_wgrad_row.hip): the same pair
struct VsrkRowPlan {
  int bands, band_h, nseg, ncot, ncic;
  WgradSlabs slabs;  // nsplit: one per (image, band, segment)
};
bool vsrk_wgrad_row_plan(const vsrk_conv_desc* d, const vsrk_tensor5* x, const vsrk_tensor5* dy, VsrkRowPlan* p);
void vsrk_conv_wgrad_row(const vsrk_conv_desc* d, const vsrk_tensor5* x, const vsrk_tensor5* dy, int want_bias,
                         float* ws, const VsrkRowPlan& p, hipStream_t s);

// Kernels on the generic plan's slabs, tried before the generic kernel:
// 1 = launched the slab kernel, 0 = not eligible.
// thin-channel (conv_thin.hip), then two-stage pipelined 16-bit 3x3(x3) (conv_wgrad_pipe.hip)
int vsrk_conv_wgrad_thin(const vsrk_conv::WgradArgs& a, int nco, int nci, int perm_r, int dtype, hipStream_t s);
int vsrk_conv_wgrad_pipe(const vsrk_conv::WgradArgs& a, int nco, int nci, int dtype, hipStream_t s);
