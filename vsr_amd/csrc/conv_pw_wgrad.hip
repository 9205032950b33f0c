// Pointwise conv: the weight-gradient kernel.
#include "conv_pw_impl.h"

bool vsrk_conv::pw_wgrad(int nco, int nw, int dtype, const PwWArgs& a, int nsplit, hipStream_t s) {
  return pw_dispatch_ncb<2, 8>(nco, [&](auto n) {
    constexpr int N = decltype(n)::value;
    vsrk_dispatch16(dtype, [&](auto tag) {
      using H = decltype(tag);
      if (nw == 8) launch_wgrad_pw<N, H, 8>(a, nsplit, s);
      else launch_wgrad_pw<N, H, 4>(a, nsplit, s);
      return 0;
    });
    return true;
  });
}
