// Tap arithmetic of the interpolating upsampling kernels, shared by the
// plane form (upsample.hip) and the channels-last form (resample_cl.hip): one
// routine (pos_taps, through axis_taps) gives the clamped tap indices and
// weights of an output coordinate; a forward applies it per axis, an adjoint
// gathers with it, so the border rule is the same by construction.
#pragma once
#include "vsrk_common.h"

namespace vsrk_taps {

constexpr int MODE_BILINEAR = 0, MODE_BICUBIC = 1;

template <int MODE> struct Taps { static constexpr int N = MODE == MODE_BICUBIC ? 4 : 2; };

// ATen's cubic convolution coefficients (A = -0.75) of the four taps around
// floor(src) for the fraction t.
__device__ __forceinline__ void cubic_weights(float t, float* w) {
  constexpr float A = -0.75f;
  const float u = 1.f - t;
  w[0] = ((A * (t + 1.f) - 5.f * A) * (t + 1.f) + 8.f * A) * (t + 1.f) - 4.f * A;
  w[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
  w[2] = ((A + 2.f) * u - (A + 3.f)) * u * u + 1.f;
  w[3] = ((A * (u + 1.f) - 5.f * A) * (u + 1.f) + 8.f * A) * (u + 1.f) - 4.f * A;
}

// Position of an output index on one axis, kept in integers so that a walk
// along a row needs no division: (base, num) with the source coordinate
// base + num / den(axis).
//   align_corners = 0: src = (dst + 0.5) / r - 0.5 depends on the phase
//     j = dst mod r alone.  base = q = dst / r and num = j; with
//     n = 2 j + 1 - r, src = q + n / (2 r), and n < 0 puts the floor at q - 1
//     (fraction (n + 2 r) / (2 r)).
//   align_corners = 1: src = dst (in - 1) / (out - 1) by integer division (a
//     float coordinate loses ~1e-5 at a few hundred pixels): base the
//     quotient, num the remainder; 0 when out = 1 or in = 1.
struct AxisPos {
  int base, num;
};

__device__ __forceinline__ AxisPos axis_pos(int dst, int in, int out, int r, int ac) {
  AxisPos p;
  if (ac) {
    if (out <= 1 || in <= 1) {
      p.base = 0;
      p.num = 0;
    } else {
      const int64_t num = (int64_t)dst * (in - 1), den = out - 1;
      p.base = (int)(num / den);
      p.num = (int)(num - (int64_t)p.base * den);
    }
  } else {
    p.base = dst / r;
    p.num = dst - p.base * r;
  }
  return p;
}

// the position of dst + 1 from that of dst (in - 1 < out - 1: one carry at most)
__device__ __forceinline__ void axis_next(AxisPos& p, int in, int out, int r, int ac) {
  if (ac) {
    p.num += in - 1;
    if (in > 1 && p.num >= out - 1) {
      p.num -= out - 1;
      ++p.base;
    }
  } else if (++p.num == r) {
    p.num = 0;
    ++p.base;
  }
}

// Tap indices (clamped to the image: replicate) and weights at a position.
template <int MODE>
__device__ __forceinline__ void pos_taps(const AxisPos& p, int in, int out, int r, int ac, int* idx, float* wt) {
  int base;
  float t;
  if (ac) {
    base = p.base;
    t = out > 1 ? (float)p.num / (float)(out - 1) : 0.f;
  } else {
    const int n = 2 * p.num + 1 - r;
    base = n < 0 ? p.base - 1 : p.base;
    t = (float)(n < 0 ? n + 2 * r : n) / (float)(2 * r);
  }
  if (MODE == MODE_BICUBIC) {
    cubic_weights(t, wt);
#pragma unroll
    for (int a = 0; a < 4; ++a) idx[a] = min(max(base - 1 + a, 0), in - 1);
  } else {
    wt[0] = 1.f - t;
    wt[1] = t;
    idx[0] = min(max(base, 0), in - 1);
    idx[1] = min(max(base + 1, 0), in - 1);
  }
}

// The taps of output index dst (0 <= dst < out = r * in).
template <int MODE>
__device__ __forceinline__ void axis_taps(int dst, int in, int out, int r, int ac, int* idx, float* wt) {
  pos_taps<MODE>(axis_pos(dst, in, out, r, ac), in, out, r, ac, idx, wt);
}

// The output indices whose taps can touch input index i: their floor lies in
// [i - hi_off, i - lo_off] for tap offsets lo_off..hi_off (clamped taps come
// from floors inside that range too, at both borders).
__device__ __forceinline__ void reach(int i, int in, int out, int r, int ac, int lo_off, int hi_off, int& d0,
                                      int& d1) {
  const int64_t b0 = (int64_t)i - hi_off, b1 = (int64_t)i - lo_off;
  int64_t lo, hi;
  if (ac) {
    if (out <= 1 || in <= 1) {
      lo = 0;
      hi = out - 1;
    } else {
      // floor(dst (in-1) / (out-1)) >= b0  and  <= b1
      const int64_t den = out - 1, m = in - 1;
      lo = b0 <= 0 ? 0 : (b0 * den + m - 1) / m;
      hi = ((b1 + 1) * den + m - 1) / m - 1;
    }
  } else {
    // the floor is q - 1 or q for q = dst / r
    lo = b0 * r;
    hi = (b1 + 2) * r - 1;
  }
  d0 = lo < 0 ? 0 : (int)lo;
  d1 = hi > out - 1 ? out - 1 : (int)hi;
}

}  // namespace vsrk_taps
