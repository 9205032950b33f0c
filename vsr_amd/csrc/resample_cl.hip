// Pooling and resampling of channels-last feature maps (N, 1, H, W, C views),
// FNet's encoder and decoder (frvsr_net.py:120-137):
//   nn.MaxPool2d(2) forward and backward,
//   F.interpolate(scale_factor=r, mode='bilinear', align_corners) forward and
//   its adjoint as a fixed-order gather (tap arithmetic: upsample_taps.h, the
//   routine the plane kernels of upsample.hip use).
// Lanes move 16-byte chunks of the channel axis where the views allow (cl_lane.h).
#include "cl_lane.h"
#include "upsample_taps.h"

namespace {

using namespace vsrk_cl;
using namespace vsrk_taps;

// ---- nn.MaxPool2d(2): floor on odd sizes; on exact ties the first maximum in
// row-major window order wins (torch's CPU kernel) ----
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void max_pool2x2_fwd_kernel(View x, View y, int nc, int64_t total) {
  constexpr int E = Lane<T, VEC>::E;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  int n, oy, ox, c0;
  decode(idx, nc, y.w, y.h, E, n, oy, ox, c0);
  const T* xp = reinterpret_cast<const T*>(x.ptr);
  float best[E], v[E];
  Lane<T, VEC>::load(xp + off(x, n, 2 * oy, 2 * ox, c0), best);
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    Lane<T, VEC>::load(xp + off(x, n, 2 * oy + (k >> 1), 2 * ox + (k & 1), c0), v);
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (beats(v[e], best[e])) best[e] = v[e];
  }
  Lane<T, VEC>::store(reinterpret_cast<T*>(y.ptr) + off(y, n, oy, ox, c0), best);
}

// One lane per INPUT chunk: it recomputes its window's arg-max from the saved
// input and takes gy if that is its own position, 0 otherwise (also in the
// odd last row / column, which no window covers).
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void max_pool2x2_bwd_kernel(View x, View gy, View gx, int nc, int64_t total) {
  constexpr int E = Lane<T, VEC>::E;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  int n, iy, ix, c0;
  decode(idx, nc, x.w, x.h, E, n, iy, ix, c0);
  float out[E];
#pragma unroll
  for (int e = 0; e < E; ++e) out[e] = 0.f;
  const int oy = iy >> 1, ox = ix >> 1;
  if (oy < gy.h && ox < gy.w) {
    const T* xp = reinterpret_cast<const T*>(x.ptr);
    const int me = ((iy & 1) << 1) | (ix & 1);
    float best[E], v[E], g[E];
    int arg[E];
    Lane<T, VEC>::load(xp + off(x, n, 2 * oy, 2 * ox, c0), best);
#pragma unroll
    for (int e = 0; e < E; ++e) arg[e] = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      Lane<T, VEC>::load(xp + off(x, n, 2 * oy + (k >> 1), 2 * ox + (k & 1), c0), v);
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (beats(v[e], best[e])) {
          best[e] = v[e];
          arg[e] = k;
        }
    }
    Lane<T, VEC>::load(reinterpret_cast<const T*>(gy.ptr) + off(gy, n, oy, ox, c0), g);
#pragma unroll
    for (int e = 0; e < E; ++e) out[e] = arg[e] == me ? g[e] : 0.f;
  }
  Lane<T, VEC>::store(reinterpret_cast<T*>(gx.ptr) + off(gx, n, iy, ix, c0), out);
}

// ---- bilinear x r ----
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void upsample_cl_fwd_kernel(View x, View y, int r, int ac, int accumulate, int nc,
                                                              int64_t total) {
  constexpr int E = Lane<T, VEC>::E;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  int n, oy, ox, c0;
  decode(idx, nc, y.w, y.h, E, n, oy, ox, c0);
  int iy[2], ix[2];
  float wy[2], wx[2];
  axis_taps<MODE_BILINEAR>(oy, x.h, y.h, r, ac, iy, wy);
  axis_taps<MODE_BILINEAR>(ox, x.w, y.w, r, ac, ix, wx);
  const T* xp = reinterpret_cast<const T*>(x.ptr);
  float acc[E];
#pragma unroll
  for (int e = 0; e < E; ++e) acc[e] = 0.f;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    float p[E], q[E];
    Lane<T, VEC>::load(xp + off(x, n, iy[a], ix[0], c0), p);
    Lane<T, VEC>::load(xp + off(x, n, iy[a], ix[1], c0), q);
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] += wy[a] * (wx[0] * p[e] + wx[1] * q[e]);
  }
  T* yp = reinterpret_cast<T*>(y.ptr) + off(y, n, oy, ox, c0);
  if (accumulate) {
    float o[E];
    Lane<T, VEC>::load(yp, o);
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] += o[e];
  }
  Lane<T, VEC>::store(yp, acc);
}

// Adjoint as a gather, one lane per input chunk: every output pixel that can
// reach the input pixel is visited in a fixed order, its taps recomputed by
// axis_taps, and the weights of the taps that land here are summed.  No
// atomics: bitwise reproducible.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void upsample_cl_bwd_kernel(View gy, View gx, int r, int ac, int accumulate, int nc,
                                                              int64_t total) {
  constexpr int E = Lane<T, VEC>::E;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  int n, iy, ix, c0;
  decode(idx, nc, gx.w, gx.h, E, n, iy, ix, c0);
  int oy0, oy1, ox0, ox1;
  reach(iy, gx.h, gy.h, r, ac, 0, 1, oy0, oy1);
  reach(ix, gx.w, gy.w, r, ac, 0, 1, ox0, ox1);
  const T* gp = reinterpret_cast<const T*>(gy.ptr);
  float acc[E];
#pragma unroll
  for (int e = 0; e < E; ++e) acc[e] = 0.f;
  for (int oy = oy0; oy <= oy1; ++oy) {
    int t[2];
    float w[2];
    axis_taps<MODE_BILINEAR>(oy, gx.h, gy.h, r, ac, t, w);
    const float cy = (t[0] == iy ? w[0] : 0.f) + (t[1] == iy ? w[1] : 0.f);
    if (t[0] != iy && t[1] != iy) continue;
    float s[E];
#pragma unroll
    for (int e = 0; e < E; ++e) s[e] = 0.f;
    for (int ox = ox0; ox <= ox1; ++ox) {
      axis_taps<MODE_BILINEAR>(ox, gx.w, gy.w, r, ac, t, w);
      const float cx = (t[0] == ix ? w[0] : 0.f) + (t[1] == ix ? w[1] : 0.f);
      float g[E];
      Lane<T, VEC>::load(gp + off(gy, n, oy, ox, c0), g);
#pragma unroll
      for (int e = 0; e < E; ++e) s[e] += cx * g[e];
    }
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] += cy * s[e];
  }
  T* xp = reinterpret_cast<T*>(gx.ptr) + off(gx, n, iy, ix, c0);
  if (accumulate) {
    float o[E];
    Lane<T, VEC>::load(xp, o);
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] += o[e];
  }
  Lane<T, VEC>::store(xp, acc);
}

// `small` is the (h, w) side and `big` the (f h [+ 1], f w [+ 1]) side of a pool (f = 2, odd sizes floor) or
// an upsampling (exact)
int check_pair(const char* name, const vsrk_tensor5* small, const vsrk_tensor5* big, int f, bool floor_ok) {
  VSRK_TRY(check_view(name, small, false));
  VSRK_TRY(check_view(name, big, false));
  VSRK_CHECK(small->dtype == big->dtype, "%s: dtype mismatch (%d and %d)", name, small->dtype, big->dtype);
  VSRK_CHECK(small->n == big->n && small->c == big->c, "%s: batch / channel mismatch (%d, %d) and (%d, %d)", name,
             small->n, small->c, big->n, big->c);
  VSRK_CHECK(big->h >= 1 && big->w >= 1 && small->h >= 1 && small->w >= 1, "%s: empty map (%d x %d from %d x %d)",
             name, small->h, small->w, big->h, big->w);
  const bool ok = floor_ok ? (big->h / f == small->h && big->w / f == small->w)
                           : ((int64_t)small->h * f == big->h && (int64_t)small->w * f == big->w);
  VSRK_CHECK(ok, "%s: %d x %d and %d x %d do not differ by the factor %d", name, small->h, small->w, big->h, big->w,
             f);
  // one lane per chunk in 256-thread workgroups: the grid is a 32-bit count
  VSRK_CHECK((int64_t)big->n * big->h * big->w * big->c <= ((int64_t)1 << 39), "%s: tensor too large", name);
  return VSRK_OK;
}

}  // namespace

extern "C" int vsrk_max_pool2x2_fwd(const vsrk_tensor5* x, const vsrk_tensor5* y, void* stream) {
  VSRK_TRY(check_pair("max_pool2x2_fwd", y, x, 2, true));
  const bool vec = vec_ok(x) && vec_ok(y);
  const int nc = chunks(x->dtype, vec, y->c);
  const int64_t total = (int64_t)y->n * y->h * y->w * nc;
  launch_lanes(x->dtype, vec, total, stream, [&](auto lane, dim3 grid, hipStream_t s) {
    using L = decltype(lane);
    max_pool2x2_fwd_kernel<typename L::Elem, L::Vec><<<grid, 256, 0, s>>>(make_view(x), make_view(y), nc, total);
  });
  VSRK_LAUNCH_CHECK("max_pool2x2_fwd");
  return VSRK_OK;
}

extern "C" int vsrk_max_pool2x2_bwd(const vsrk_tensor5* x, const vsrk_tensor5* gy, const vsrk_tensor5* gx,
                                    void* stream) {
  VSRK_TRY(check_pair("max_pool2x2_bwd", gy, x, 2, true));
  VSRK_TRY(check_shape("max_pool2x2_bwd", "gx", gx, x->dtype, x->n, x->h, x->w, x->c, false));
  const bool vec = vec_ok(x) && vec_ok(gy) && vec_ok(gx);
  const int nc = chunks(x->dtype, vec, x->c);
  const int64_t total = (int64_t)x->n * x->h * x->w * nc;
  launch_lanes(x->dtype, vec, total, stream, [&](auto lane, dim3 grid, hipStream_t s) {
    using L = decltype(lane);
    max_pool2x2_bwd_kernel<typename L::Elem, L::Vec><<<grid, 256, 0, s>>>(make_view(x), make_view(gy), make_view(gx),
                                                                          nc, total);
  });
  VSRK_LAUNCH_CHECK("max_pool2x2_bwd");
  return VSRK_OK;
}

static int check_up(const char* name, const vsrk_tensor5* small, const vsrk_tensor5* big, int32_t r, int32_t ac,
                    int32_t accumulate) {
  VSRK_CHECK(r >= 1, "%s: scale factor %d < 1", name, r);
  VSRK_CHECK((ac | 1) == 1 && (accumulate | 1) == 1, "%s: align_corners / accumulate must be 0 or 1", name);
  VSRK_CHECK(!small || ((int64_t)small->h * r <= (1 << 30) && (int64_t)small->w * r <= (1 << 30)),
             "%s: output too large", name);
  return check_pair(name, small, big, r, false);
}

extern "C" int vsrk_upsample_cl_fwd(const vsrk_tensor5* x, const vsrk_tensor5* y, int32_t r, int32_t align_corners,
                                    int32_t accumulate, void* stream) {
  VSRK_TRY(check_up("upsample_cl_fwd", x, y, r, align_corners, accumulate));
  const bool vec = vec_ok(x) && vec_ok(y);
  const int nc = chunks(x->dtype, vec, y->c);
  const int64_t total = (int64_t)y->n * y->h * y->w * nc;
  launch_lanes(x->dtype, vec, total, stream, [&](auto lane, dim3 grid, hipStream_t s) {
    using L = decltype(lane);
    upsample_cl_fwd_kernel<typename L::Elem, L::Vec><<<grid, 256, 0, s>>>(make_view(x), make_view(y), r, align_corners,
                                                                          accumulate, nc, total);
  });
  VSRK_LAUNCH_CHECK("upsample_cl_fwd");
  return VSRK_OK;
}

extern "C" int vsrk_upsample_cl_bwd(const vsrk_tensor5* gy, const vsrk_tensor5* gx, int32_t r, int32_t align_corners,
                                    int32_t accumulate, void* stream) {
  VSRK_TRY(check_up("upsample_cl_bwd", gx, gy, r, align_corners, accumulate));
  const bool vec = vec_ok(gx) && vec_ok(gy);
  const int nc = chunks(gx->dtype, vec, gx->c);
  const int64_t total = (int64_t)gx->n * gx->h * gx->w * nc;
  launch_lanes(gx->dtype, vec, total, stream, [&](auto lane, dim3 grid, hipStream_t s) {
    using L = decltype(lane);
    upsample_cl_bwd_kernel<typename L::Elem, L::Vec><<<grid, 256, 0, s>>>(make_view(gy), make_view(gx), r,
                                                                          align_corners, accumulate, nc, total);
  });
  VSRK_LAUNCH_CHECK("upsample_cl_bwd");
  return VSRK_OK;
}
