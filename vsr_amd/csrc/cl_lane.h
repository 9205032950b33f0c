// Lane helpers of the channels-last view kernels (resample_cl.hip, tsa.hip,
// the *_view kernels of dcn.hip).  These kernels are HBM-bound: a lane moves one 16-byte chunk
// of the channel axis (8 x 16-bit or 4 x fp32 channels), consecutive lanes
// consecutive chunks, then consecutive pixels; views whose channel count, base
// or strides do not allow 16-byte accesses take the same kernels one element
// per lane.  The host layer of those kernels is here too: the argument checks
// of a view and the launch over (storage type, lane width).
#pragma once
#include "vsrk_common.h"

namespace vsrk_cl {

// what one lane moves: a 16-byte chunk (VEC) or a single element
template <typename T, bool VEC> struct Lane {
  using Elem = T;
  static constexpr bool Vec = VEC;
  static constexpr int E = VEC ? Chunk<T>::E : 1;
  __device__ static __forceinline__ void load(const T* p, float* f) {
    if constexpr (VEC)
      Chunk<T>::unpack(*reinterpret_cast<const uint4*>(p), f);
    else
      f[0] = to_f32<T>(p[0]);
  }
  __device__ static __forceinline__ void store(T* p, const float* f) {
    if constexpr (VEC)
      *reinterpret_cast<uint4*>(p) = Chunk<T>::pack(f);
    else
      p[0] = from_f32<T>(f[0]);
  }
};

inline bool vec_ok(const vsrk_tensor5* t) {
  const int64_t es = vsrk_esize(t->dtype), e = 16 / es;
  return t->c % e == 0 && (reinterpret_cast<uintptr_t>(t->ptr) & 15) == 0 && t->sn % e == 0 && t->sh % e == 0 &&
         t->sw % e == 0;
}

// idx -> (n, y, x, first channel) over a (n, hh, ww, c / E) index space
// (64-bit divisions cost several times the 32-bit ones: taken only past 2^32 lanes)
__device__ __forceinline__ void decode(int64_t idx, int nc, int ww, int hh, int E, int& n, int& y, int& x, int& c0) {
  if ((idx >> 32) == 0) {
    uint32_t i = (uint32_t)idx, q = i / (uint32_t)nc;
    c0 = (int)(i - q * nc) * E;
    i = q / (uint32_t)ww;
    x = (int)(q - i * ww);
    q = i / (uint32_t)hh;
    y = (int)(i - q * hh);
    n = (int)q;
    return;
  }
  c0 = (int)(idx % nc) * E;
  idx /= nc;
  x = (int)(idx % ww);
  idx /= ww;
  y = (int)(idx % hh);
  n = (int)(idx / hh);
}

__device__ __forceinline__ int64_t off(const View& v, int n, int y, int x, int c) {
  return n * v.sn + y * v.sh + x * v.sw + c;
}

// a > b as torch's max-pool compares: a NaN beats everything before it
__device__ __forceinline__ bool beats(float a, float b) { return a > b || a != a; }

// ---- host side: argument checks ----
#define VSRK_TRY(expr)              \
  do {                              \
    const int rc_ = (expr);         \
    if (rc_ != VSRK_OK) return rc_; \
  } while (0)

// A plain (n, 1, h, w, c) view of a known dtype.  `sized`: with a map that is not empty and at most 2^39
// elements (one lane per chunk in 256-thread workgroups: the grid is a 32-bit count); the entry points that
// check a pair of maps (resample_cl.hip) or a geometry (dcn.hip) make these two checks there.
inline int check_view(const char* name, const vsrk_tensor5* t, bool sized = true) {
  VSRK_CHECK(t && t->ptr, "%s: null argument", name);
  VSRK_CHECK(t->dtype == VSRK_F32 || t->dtype == VSRK_BF16 || t->dtype == VSRK_F16, "%s: unknown dtype %d", name,
             t->dtype);
  VSRK_CHECK(t->shuffle <= 1, "%s: plain views only", name);
  const int lo = sized ? 1 : 0;
  VSRK_CHECK(t->n >= 1 && t->d == 1 && t->h >= lo && t->w >= lo && t->c >= 1,
             "%s: view (%d, %d, %d, %d, %d) must be (n, 1, h, w, c)%s", name, t->n, t->d, t->h, t->w, t->c,
             sized ? ", not empty" : "");
  VSRK_CHECK(!sized || (int64_t)t->n * t->h * t->w * t->c <= ((int64_t)1 << 39), "%s: tensor too large", name);
  return VSRK_OK;
}

// `t` (`what` in the message) is such a view, of this dtype and this (n, h, w, c)
inline int check_shape(const char* name, const char* what, const vsrk_tensor5* t, int dtype, int n, int h, int w,
                       int c, bool sized = true) {
  VSRK_TRY(check_view(name, t, sized));
  VSRK_CHECK(t->dtype == dtype, "%s: %s has dtype %d, expected %d", name, what, t->dtype, dtype);
  VSRK_CHECK(t->n == n && t->h == h && t->w == w && t->c == c,
             "%s: %s is (%d, 1, %d, %d, %d) and does not match the expected (%d, 1, %d, %d, %d)", name, what, t->n,
             t->h, t->w, t->c, n, h, w, c);
  return VSRK_OK;
}

// ---- host side: launch ----
// lanes that cover c channels
inline int chunks(int dtype, bool vec, int c) { return c / (vec ? 16 / vsrk_esize(dtype) : 1); }

// Calls launch(Lane<T, VEC>{}, grid, s) with the grid of `lanes` lanes in 256-thread workgroups: the caller's
// generic lambda names its kernel, K<typename L::Elem, L::Vec><<<grid, 256, 0, s>>>(...) with L = decltype(lane).
template <typename T, typename Fn>
inline void launch_lanes_of(bool vec, int64_t lanes, void* stream, Fn&& launch) {
  const dim3 grid((unsigned)ceil_div64(lanes, 256));
  if (vec) launch(Lane<T, true>{}, grid, (hipStream_t)stream);
  else launch(Lane<T, false>{}, grid, (hipStream_t)stream);
}
// ... T the storage type of `dtype`
template <typename Fn>
inline void launch_lanes(int dtype, bool vec, int64_t lanes, void* stream, Fn&& launch) {
  vsrk_dispatch_dtype(dtype, [&](auto tag) { launch_lanes_of<decltype(tag)>(vec, lanes, stream, launch); });
}

}  // namespace vsrk_cl

