// Lane helpers of the channels-last view kernels (resample_cl.hip, tsa.hip,
// the *_view kernels of dcn.hip).  These kernels are HBM-bound: a lane moves one 16-byte chunk
// of the channel axis (8 x 16-bit or 4 x fp32 channels), consecutive lanes
// consecutive chunks, then consecutive pixels; views whose channel count, base
// or strides do not allow 16-byte accesses take the same kernels one element
// per lane.
#pragma once
#include "vsrk_common.h"

namespace vsrk_cl {

// what one lane moves: a 16-byte chunk (VEC) or a single element
template <typename T, bool VEC> struct Lane {
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

}  // namespace vsrk_cl

// launch K<T, VEC> over `lanes` = voxels x chunks on the stream `s`
#define VSRK_CL_LAUNCH(KERNEL, dtype, vec, voxels, c, ...)                                     \
  do {                                                                                         \
    const int E_ = (vec) ? 16 / vsrk_esize(dtype) : 1, nc = (c) / E_;                          \
    const int64_t total = (int64_t)(voxels) * nc;                                              \
    const dim3 grid((unsigned)ceil_div64(total, 256));                                         \
    if ((dtype) == VSRK_BF16) {                                                                \
      if (vec) KERNEL<bf16, true><<<grid, 256, 0, s>>>(__VA_ARGS__, nc, total);                \
      else KERNEL<bf16, false><<<grid, 256, 0, s>>>(__VA_ARGS__, nc, total);                   \
    } else if ((dtype) == VSRK_F16) {                                                          \
      if (vec) KERNEL<f16, true><<<grid, 256, 0, s>>>(__VA_ARGS__, nc, total);                 \
      else KERNEL<f16, false><<<grid, 256, 0, s>>>(__VA_ARGS__, nc, total);                    \
    } else {                                                                                   \
      if (vec) KERNEL<float, true><<<grid, 256, 0, s>>>(__VA_ARGS__, nc, total);               \
      else KERNEL<float, false><<<grid, 256, 0, s>>>(__VA_ARGS__, nc, total);                  \
    }                                                                                          \
  } while (0)
