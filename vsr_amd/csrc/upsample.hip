// Interpolating upsampling by an integer factor, forward and adjoint:
// F.interpolate(x, scale_factor=r, mode='bilinear' | 'bicubic', align_corners)
// on contiguous planes (P, h, w) -> (P, r h, r w).  SRFBN's global skip
// (srfb_net.py:47, bilinear, align_corners=False) and the Bicubic baseline
// (bicubic.py:15, bicubic, align_corners=True).
//
// One routine (pos_taps, through axis_taps, upsample_taps.h) gives the clamped
// tap indices and weights of an output coordinate; the forward applies it per
// axis, the adjoint gathers with it, so the border rule is the same by
// construction.  Arithmetic is fp32.
#include "upsample_taps.h"

namespace {

using namespace vsrk_taps;

// Each lane produces one 16-byte run of an output row (E elements): a single
// full-width store where the run is whole and aligned, element stores at the
// row's tail or on an unaligned row.  idx enumerates (plane, row, run).
template <typename T, int MODE>
__global__ __launch_bounds__(256) void upsample_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int h, int w,
                                                           int H, int W, int r, int ac, int accumulate, int runs,
                                                           int64_t total) {
  constexpr int E = Chunk<T>::E, NT = Taps<MODE>::N;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int run = (int)(idx % runs);
  const int64_t row = idx / runs;  // plane * H + oy
  const int oy = (int)(row % H);
  const int64_t plane = row / H;
  int iy[NT];
  float wy[NT];
  axis_taps<MODE>(oy, h, H, r, ac, iy, wy);
  const T* xp = x + plane * ((int64_t)h * w);
  const int ox0 = run * E;
  float v[E];
  AxisPos px = axis_pos(ox0, w, W, r, ac);  // the run walks the row from here without a division
#pragma unroll
  for (int e = 0; e < E; ++e) {
    int ix[NT];  // (past the row's end the taps clamp to the last column: computed, never stored)
    float wx[NT];
    pos_taps<MODE>(px, w, W, r, ac, ix, wx);
    axis_next(px, w, W, r, ac);
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < NT; ++a) {
      const T* xr = xp + (int64_t)iy[a] * w;
      float s = 0.f;
#pragma unroll
      for (int b = 0; b < NT; ++b) s += wx[b] * to_f32<T>(xr[ix[b]]);
      acc += wy[a] * s;
    }
    v[e] = acc;
  }
  T* yp = y + row * (int64_t)W + ox0;
  if (ox0 + E <= W && (reinterpret_cast<uintptr_t>(yp) & 15) == 0) {
    uint4* y4 = reinterpret_cast<uint4*>(yp);
    if (accumulate) {
      float o[E];
      Chunk<T>::unpack(*y4, o);
#pragma unroll
      for (int e = 0; e < E; ++e) v[e] += o[e];
    }
    *y4 = Chunk<T>::pack(v);
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (ox0 + e < W) yp[e] = from_f32<T>(accumulate ? v[e] + to_f32<T>(yp[e]) : v[e]);
    }
  }
}


// Adjoint as a gather, one input pixel per thread: every output pixel that can
// reach it is visited in a fixed order, its taps recomputed by axis_taps, and
// the weights of the taps that land on this pixel are summed.  No atomics:
// bitwise reproducible.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void upsample_bwd_kernel(const T* __restrict__ gy, T* __restrict__ gx, int h, int w,
                                                           int H, int W, int r, int ac, int accumulate,
                                                           int64_t total) {
  constexpr int NT = Taps<MODE>::N;
  constexpr int LO = MODE == MODE_BICUBIC ? -1 : 0, HI = MODE == MODE_BICUBIC ? 2 : 1;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int ix = (int)(idx % w);
  const int64_t row = idx / w;
  const int iy = (int)(row % h);
  const int64_t plane = row / h;
  int oy0, oy1, ox0, ox1;
  reach(iy, h, H, r, ac, LO, HI, oy0, oy1);
  reach(ix, w, W, r, ac, LO, HI, ox0, ox1);
  const T* gp = gy + plane * ((int64_t)H * W);
  float acc = 0.f;
  for (int oy = oy0; oy <= oy1; ++oy) {
    int ty[NT];
    float wy[NT];
    axis_taps<MODE>(oy, h, H, r, ac, ty, wy);
    float cy = 0.f;
    bool hit = false;
#pragma unroll
    for (int a = 0; a < NT; ++a)
      if (ty[a] == iy) {
        cy += wy[a];
        hit = true;
      }
    if (!hit) continue;
    const T* gr = gp + (int64_t)oy * W;
    float s = 0.f;
    for (int ox = ox0; ox <= ox1; ++ox) {
      int tx[NT];
      float wx[NT];
      axis_taps<MODE>(ox, w, W, r, ac, tx, wx);
      float cx = 0.f;
#pragma unroll
      for (int b = 0; b < NT; ++b)
        if (tx[b] == ix) cx += wx[b];
      s += cx * to_f32<T>(gr[ox]);
    }
    acc += cy * s;
  }
  if (accumulate) acc += to_f32<T>(gx[idx]);
  gx[idx] = from_f32<T>(acc);
}

// Shared argument checks; H, W = the output size.
int check_args(const char* name, int32_t dtype, const void* x, const void* y, int64_t planes, int32_t h, int32_t w,
               int32_t r, int32_t mode, int32_t align_corners, int32_t accumulate) {
  VSRK_CHECK(x && y, "%s: null argument", name);
  VSRK_CHECK(dtype == VSRK_F32 || dtype == VSRK_BF16 || dtype == VSRK_F16, "%s: unknown dtype %d", name, dtype);
  VSRK_CHECK(r >= 1, "%s: scale factor %d < 1", name, r);
  VSRK_CHECK(planes >= 1 && h >= 1 && w >= 1, "%s: empty tensor (%lld, %d, %d)", name, (long long)planes, h, w);
  VSRK_CHECK(mode == MODE_BILINEAR || mode == MODE_BICUBIC, "%s: mode %d (0 bilinear, 1 bicubic)", name, mode);
  VSRK_CHECK((align_corners | 1) == 1 && (accumulate | 1) == 1, "%s: align_corners / accumulate must be 0 or 1",
             name);
  // rows and columns are 32-bit indices (2 j + 1 + r and the scan ranges stay
  // inside int), element offsets 64-bit; the grid is one thread per 16-byte
  // run (forward) or input pixel (backward), in 256-thread workgroups
  VSRK_CHECK((int64_t)h * r <= (1 << 30) && (int64_t)w * r <= (1 << 30), "%s: output %lld x %lld too large", name,
             (long long)h * r, (long long)w * r);
  const int64_t plane_out = (int64_t)h * r * ((int64_t)w * r);
  VSRK_CHECK(planes <= ((((int64_t)1 << 32) - 256) / plane_out), "%s: %lld planes of %lld elements exceed the grid",
             name, (long long)planes, (long long)plane_out);
  return VSRK_OK;
}

template <typename T>
void launch_fwd(const void* x, void* y, int64_t planes, int h, int w, int r, int mode, int ac, int acc,
                hipStream_t s) {
  const int H = h * r, W = w * r;
  const int runs = ceil_div(W, Chunk<T>::E);
  const int64_t total = planes * H * runs;
  const dim3 grid((unsigned)ceil_div64(total, 256));
  if (mode == MODE_BICUBIC)
    upsample_fwd_kernel<T, MODE_BICUBIC><<<grid, 256, 0, s>>>((const T*)x, (T*)y, h, w, H, W, r, ac, acc, runs, total);
  else
    upsample_fwd_kernel<T, MODE_BILINEAR><<<grid, 256, 0, s>>>((const T*)x, (T*)y, h, w, H, W, r, ac, acc, runs, total);
}

template <typename T>
void launch_bwd(const void* gy, void* gx, int64_t planes, int h, int w, int r, int mode, int ac, int acc,
                hipStream_t s) {
  const int H = h * r, W = w * r;
  const int64_t total = planes * h * w;
  const dim3 grid((unsigned)ceil_div64(total, 256));
  if (mode == MODE_BICUBIC)
    upsample_bwd_kernel<T, MODE_BICUBIC><<<grid, 256, 0, s>>>((const T*)gy, (T*)gx, h, w, H, W, r, ac, acc, total);
  else
    upsample_bwd_kernel<T, MODE_BILINEAR><<<grid, 256, 0, s>>>((const T*)gy, (T*)gx, h, w, H, W, r, ac, acc, total);
}

}  // namespace

extern "C" int vsrk_upsample2d_fwd(int32_t dtype, const void* x, int64_t planes, int32_t h, int32_t w, int32_t r,
                                   int32_t mode, int32_t align_corners, int32_t accumulate, void* y, void* stream) {
  const int rc = check_args("upsample2d_fwd", dtype, x, y, planes, h, w, r, mode, align_corners, accumulate);
  if (rc != VSRK_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  vsrk_dispatch_dtype(dtype, [&](auto tag) {
    launch_fwd<decltype(tag)>(x, y, planes, h, w, r, mode, align_corners, accumulate, s);
  });
  VSRK_LAUNCH_CHECK("upsample2d_fwd");
  return VSRK_OK;
}

extern "C" int vsrk_upsample2d_bwd(int32_t dtype, const void* gy, int64_t planes, int32_t h, int32_t w, int32_t r,
                                   int32_t mode, int32_t align_corners, int32_t accumulate, void* gx, void* stream) {
  const int rc = check_args("upsample2d_bwd", dtype, gy, gx, planes, h, w, r, mode, align_corners, accumulate);
  if (rc != VSRK_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  vsrk_dispatch_dtype(dtype, [&](auto tag) {
    launch_bwd<decltype(tag)>(gy, gx, planes, h, w, r, mode, align_corners, accumulate, s);
  });
  VSRK_LAUNCH_CHECK("upsample2d_bwd");
  return VSRK_OK;
}
