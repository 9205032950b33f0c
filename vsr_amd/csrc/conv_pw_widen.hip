// Pointwise conv, staged kernel: widening forms, 64 input channels into one
// output chunk of 128 / 192 / 256 (the data gradients of DRF's projections,
// with the branch-free accumulate / PReLU-backward store passes).
#include "conv_pw_impl.h"

bool vsrk_conv::pw_fwd_widen(int ncb, int nkb, int dtype, const PwArgs& a, int grid, int nchunk, hipStream_t s) {
  if (nkb != 2) return false;
  if (ncb == 4) return launch_fwd_staged16<4, 2>(dtype, a, grid, nchunk, s);
  if (ncb == 6) return launch_fwd_staged16<6, 2>(dtype, a, grid, nchunk, s);
  if (ncb == 8) return launch_fwd_staged16<8, 2>(dtype, a, grid, nchunk, s);
  return false;
}
