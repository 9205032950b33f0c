// Pointwise conv, staged kernel: narrowing forms, one output chunk of fewer
// blocks than the input (DRF's 128..256 -> 64 projections, DUF's 256 -> 16
// residual head).
#include "conv_pw_impl.h"

bool vsrk_conv::pw_fwd_narrow(int ncb, int nkb, int dtype, const PwArgs& a, int grid, int nchunk, hipStream_t s) {
  if (ncb == 1 && nkb == 8) return launch_fwd_staged16<1, 8>(dtype, a, grid, nchunk, s);
  if (ncb == 2 && nkb == 4) return launch_fwd_staged16<2, 4>(dtype, a, grid, nchunk, s);
  if (ncb == 2 && nkb == 6) return launch_fwd_staged16<2, 6>(dtype, a, grid, nchunk, s);
  if (ncb == 2 && nkb == 8) return launch_fwd_staged16<2, 8>(dtype, a, grid, nchunk, s);
  return false;
}
