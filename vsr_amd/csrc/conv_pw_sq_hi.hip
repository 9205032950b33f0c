// Pointwise conv, staged kernel: square forms of 5..7 channel blocks (160..224
// channels: DUF's later dense units) and 8 input blocks in 128-channel output
// chunks (the 256-channel heads).
#include "conv_pw_impl.h"

bool vsrk_conv::pw_fwd_square_hi(int ncb, int nkb, int dtype, const PwArgs& a, int grid, int nchunk, hipStream_t s) {
  if (ncb == 4 && nkb == 8) return launch_fwd_staged16<4, 8>(dtype, a, grid, nchunk, s);
  if (ncb != nkb) return false;
  return pw_dispatch_ncb<5, 7>(ncb, [&](auto n) {
    constexpr int N = decltype(n)::value;
    return launch_fwd_staged16<N, N>(dtype, a, grid, nchunk, s);
  });
}
