// Pointwise conv, staged kernel with the fused per-channel reduction: square
// forms of 2..7 channel blocks, BatchNorm statistics (RED 1), BatchNorm+ReLU
// backward sums (RED 2) and the latter with the BNB input form.
#include "conv_pw_impl.h"

bool vsrk_conv::pw_fwd_reduce(int ncb, int dtype, int red, bool bnb, const PwArgs& a, int grid, hipStream_t s) {
  return pw_dispatch_ncb<2, 7>(ncb, [&](auto n) {
    constexpr int N = decltype(n)::value;
    vsrk_dispatch16(dtype, [&](auto tag) {
      using H = decltype(tag);
      if (red == 1) launch_fwd_reduce<N, 1, H>(a, grid, s);
      else if (bnb) launch_fwd_reduce<N, 2, H, true>(a, grid, s);
      else launch_fwd_reduce<N, 2, H>(a, grid, s);
      return 0;
    });
    return true;
  });
}
