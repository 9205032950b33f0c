// Pointwise conv, staged kernel: square forms of 2..4 channel blocks (64..128
// channels: DUF's first dense units, DRF's 64 -> 64).
#include "conv_pw_impl.h"

bool vsrk_conv::pw_fwd_square_lo(int ncb, int nkb, int dtype, const PwArgs& a, int grid, int nchunk, hipStream_t s) {
  if (ncb != nkb) return false;
  return pw_dispatch_ncb<2, 4>(ncb, [&](auto n) {
    constexpr int N = decltype(n)::value;
    return launch_fwd_staged16<N, N>(dtype, a, grid, nchunk, s);
  });
}
