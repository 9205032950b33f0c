// Flow warping: F.grid_sample(img, mesh + flow, 'bilinear', padding_mode,
// align_corners) on the reference's mesh (frvsr_net.py:196-240, STN), forward
// and the gradient with respect to the flow.
//
// One thread owns one output pixel: it reads its two flow values (coalesced
// along the row), forms the sampling position once and loops over the
// channels.  The backward is the same gather with the four corner values
// differenced instead of blended, so it needs no atomics and is bitwise
// reproducible.  There is no image gradient: FRVSR warps input data and a
// detached estimate only (frvsr_net.py:49,55).
//
// The mesh value comes from the integer pixel index (np.linspace's fp64 value
// rounded to fp32, as the reference's float32 mesh tensor is).  From there the
// position is fp32 arithmetic, operation for operation torch's own
// (mesh + flow, un-normalise, clip, floor), and so is the blend.  (Positions
// in fp64 were measured beside this: DESIGN.md section 7.)
#include "upsample_taps.h"

namespace {

using namespace vsrk_taps;

constexpr int PAD_ZEROS = 0, PAD_BORDER = 1;

// One axis of a sampling position: the floor pixel, the fraction beyond it and
// d(pixel coordinate) / d(flow), which is 0 where 'border' clipped the
// coordinate (torch's clip_coordinates_set_grad).
struct AxisSample {
  int i0;
  float t, mult;
};

__device__ __forceinline__ AxisSample axis_sample(int idx, int size, double step, float flow, int pad, int ac) {
  // np.linspace(-1, 1, size)[idx] as float32: start + idx * step (step = 2 / (size - 1), divided once on the
  // host), the last point exactly 1
  const double lin = size > 1 ? (idx == size - 1 ? 1.0 : -1.0 + idx * step) : -1.0;
  const float g = (float)lin + flow;
  float coord = ac ? (g + 1.f) * 0.5f * (float)(size - 1) : ((g + 1.f) * (float)size - 1.f) * 0.5f;
  AxisSample s;
  s.mult = ac ? 0.5f * (float)(size - 1) : 0.5f * (float)size;
  if (pad == PAD_BORDER) {
    if (!(coord > 0.f)) {  // also a NaN position
      coord = 0.f;
      s.mult = 0.f;
    } else if (coord >= (float)(size - 1)) {
      coord = (float)(size - 1);
      s.mult = 0.f;
    }
  } else {
    // every corner further out than one pixel is dropped anyway; the clamp
    // keeps the integer conversion defined (fmax / fmin return the non-NaN operand)
    coord = fmin(fmax(coord, -2.f), (float)size + 1.f);
  }
  const float fl = floor(coord);
  s.i0 = (int)fl;
  s.t = (float)(coord - fl);
  return s;
}

// the four corner values of one channel; corners outside the image read as 0
template <typename T>
__device__ __forceinline__ void corners(const T* __restrict__ p, int64_t sh, int64_t sw, int h, int w, int y0, int x0,
                                        float v[4]) {
  const bool ya = y0 >= 0 && y0 < h, yb = y0 + 1 >= 0 && y0 + 1 < h;
  const bool xa = x0 >= 0 && x0 < w, xb = x0 + 1 >= 0 && x0 + 1 < w;
  const T* r0 = p + (int64_t)y0 * sh + (int64_t)x0 * sw;
  v[0] = ya && xa ? to_f32<T>(r0[0]) : 0.f;
  v[1] = ya && xb ? to_f32<T>(r0[sw]) : 0.f;
  v[2] = yb && xa ? to_f32<T>(r0[sh]) : 0.f;
  v[3] = yb && xb ? to_f32<T>(r0[sh + sw]) : 0.f;
}

// Element offset of warped pixel (n, y, x), channel 0, in `o`: plain, or -- s2d
// = r > 1 -- the space-to-depth image: pixel (y / r, x / r), channel block
// (y % r) * r + x % r of c channels each.
__device__ __forceinline__ int64_t out_off(const View& o, int n, int y, int x, int c, int r) {
  if (r <= 1) return n * o.sn + y * o.sh + x * o.sw;
  const int yq = y / r, xq = x / r;
  return n * o.sn + yq * o.sh + xq * o.sw + ((y - yq * r) * r + (x - xq * r)) * c;
}

// idx -> (image n, pixel within the image, row, column); 64-bit divisions cost
// several times the 32-bit ones and are taken only past 2^32 pixels
__device__ __forceinline__ void pixel_of(int64_t idx, int64_t hw, int w, int& n, int64_t& pix, int& y, int& x) {
  uint32_t p;
  if ((idx >> 32) == 0) {
    const uint32_t i = (uint32_t)idx;
    n = (int)(i / (uint32_t)hw);
    p = i - (uint32_t)n * (uint32_t)hw;
  } else {
    n = (int)(idx / hw);
    p = (uint32_t)(idx - n * hw);
  }
  pix = p;
  y = (int)(p / (uint32_t)w);
  x = (int)(p - (uint32_t)y * (uint32_t)w);
}

// what a launch is asked to do besides its operands
struct WarpCfg {
  int s2d, pad, ac, fup;
  double step_x, step_y;  // the mesh's steps (mesh_step)
};

// The flow (u, v) of pixel (y, x): read at the image's resolution, or -- fup =
// r > 1 -- interpolated from a flow r times coarser, (n, 2, h / r, w / r):
// F.interpolate(scale_factor=r, 'bilinear', align_corners=True) with the plane
// kernel's taps and blend order (upsample.hip), so the HR flow planes are never
// written or read (frvsr_net.py:48-49).
__device__ __forceinline__ void flow_at(const float* __restrict__ flow, int n, int y, int x, int h, int w, int fup,
                                        float& u, float& v) {
  if (fup <= 1) {
    const int64_t hw = (int64_t)h * w, i = (int64_t)n * 2 * hw + (int64_t)y * w + x;
    u = flow[i];
    v = flow[i + hw];
    return;
  }
  const int lh = h / fup, lw = w / fup;
  int iy[2], ix[2];
  float wy[2], wx[2];
  axis_taps<MODE_BILINEAR>(y, lh, h, fup, 1, iy, wy);
  axis_taps<MODE_BILINEAR>(x, lw, w, fup, 1, ix, wx);
  const float* p = flow + (int64_t)n * 2 * lh * lw;
  float r[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const float* row = p + (int64_t)k * lh * lw + (int64_t)iy[a] * lw;
      float t = 0.f;
      t += wx[0] * row[ix[0]];
      t += wx[1] * row[ix[1]];
      acc += wy[a] * t;
    }
    r[k] = acc;
  }
  u = r[0];
  v = r[1];
}

template <typename T>
__global__ __launch_bounds__(256) void flow_warp_fwd_kernel(View img, const float* __restrict__ flow, View out,
                                                            WarpCfg cfg, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int h = img.h, w = img.w, c = img.c;
  const int64_t hw = (int64_t)h * w;  // <= 2^30 (check_args)
  int n, y, x;
  int64_t pix;
  pixel_of(idx, hw, w, n, pix, y, x);
  float u, v;
  flow_at(flow, n, y, x, h, w, cfg.fup, u, v);
  const AxisSample sx = axis_sample(x, w, cfg.step_x, u, cfg.pad, cfg.ac);
  const AxisSample sy = axis_sample(y, h, cfg.step_y, v, cfg.pad, cfg.ac);
  const float w00 = (1.f - sx.t) * (1.f - sy.t), w01 = sx.t * (1.f - sy.t), w10 = (1.f - sx.t) * sy.t,
              w11 = sx.t * sy.t;
  const T* ip = reinterpret_cast<const T*>(img.ptr) + n * img.sn;
  T* op = reinterpret_cast<T*>(out.ptr) + out_off(out, n, y, x, c, cfg.s2d);
  for (int ch = 0; ch < c; ++ch) {
    float v[4];
    corners<T>(ip + ch, img.sh, img.sw, h, w, sy.i0, sx.i0, v);
    op[ch] = from_f32<T>(v[0] * w00 + v[1] * w01 + v[2] * w10 + v[3] * w11);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void flow_warp_bwd_kernel(View img, const float* __restrict__ flow, View gout,
                                                            WarpCfg cfg, int accumulate, float* __restrict__ gflow,
                                                            int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int h = img.h, w = img.w, c = img.c;
  const int64_t hw = (int64_t)h * w;  // <= 2^30 (check_args)
  int n, y, x;
  int64_t pix;
  pixel_of(idx, hw, w, n, pix, y, x);
  const int64_t iu = (int64_t)n * 2 * hw + pix, iv = iu + hw;
  float u, v;
  flow_at(flow, n, y, x, h, w, cfg.fup, u, v);
  const AxisSample sx = axis_sample(x, w, cfg.step_x, u, cfg.pad, cfg.ac);
  const AxisSample sy = axis_sample(y, h, cfg.step_y, v, cfg.pad, cfg.ac);
  const T* ip = reinterpret_cast<const T*>(img.ptr) + n * img.sn;
  const T* gp = reinterpret_cast<const T*>(gout.ptr) + out_off(gout, n, y, x, c, cfg.s2d);
  float gx = 0.f, gy = 0.f;
  for (int ch = 0; ch < c; ++ch) {
    float v[4];
    corners<T>(ip + ch, img.sh, img.sw, h, w, sy.i0, sx.i0, v);
    const float g = to_f32<T>(gp[ch]);
    gx += g * ((v[1] - v[0]) * (1.f - sy.t) + (v[3] - v[2]) * sy.t);
    gy += g * ((v[2] - v[0]) * (1.f - sx.t) + (v[3] - v[1]) * sx.t);
  }
  gx *= sx.mult;
  gy *= sy.mult;
  gflow[iu] = accumulate ? gflow[iu] + gx : gx;
  gflow[iv] = accumulate ? gflow[iv] + gy : gy;
}

// np.linspace's step of the mesh over `size` points
double mesh_step(int size) { return size > 1 ? 2.0 / (size - 1) : 0.0; }

int check_args(const char* name, const vsrk_tensor5* img, const float* flow, const vsrk_tensor5* o, int32_t s2d,
               int32_t pad, int32_t ac, int32_t fup) {
  VSRK_CHECK(img && flow && o && img->ptr && o->ptr, "%s: null argument", name);
  VSRK_CHECK(img->dtype == VSRK_F32 || img->dtype == VSRK_BF16 || img->dtype == VSRK_F16, "%s: unknown dtype %d",
             name, img->dtype);
  VSRK_CHECK(img->dtype == o->dtype, "%s: dtype mismatch (%d and %d)", name, img->dtype, o->dtype);
  VSRK_CHECK(img->shuffle <= 1 && o->shuffle <= 1, "%s: plain views only (the space-to-depth store is the s2d argument)",
             name);
  VSRK_CHECK(pad == PAD_ZEROS || pad == PAD_BORDER, "%s: padding_mode %d (0 zeros, 1 border)", name, pad);
  VSRK_CHECK((ac | 1) == 1, "%s: align_corners must be 0 or 1", name);
  VSRK_CHECK(s2d >= 1, "%s: space-to-depth factor %d < 1", name, s2d);
  VSRK_CHECK(fup >= 1, "%s: flow_up factor %d < 1", name, fup);
  VSRK_CHECK(img->n >= 1 && img->d == 1 && img->h >= 1 && img->w >= 1 && img->c >= 1,
             "%s: image (%d, %d, %d, %d, %d) must be (n, 1, h, w, c), not empty", name, img->n, img->d, img->h,
             img->w, img->c);
  // one thread per pixel in 256-thread workgroups: the grid is a 32-bit count
  VSRK_CHECK((int64_t)img->h * img->w <= ((int64_t)1 << 30) &&
                 (int64_t)img->n * img->h * img->w <= ((int64_t)1 << 39),
             "%s: image %d x %d x %d too large", name, img->n, img->h, img->w);
  VSRK_CHECK(img->h % s2d == 0 && img->w % s2d == 0, "%s: image %d x %d is not a multiple of s2d %d", name, img->h,
             img->w, s2d);
  VSRK_CHECK(img->h % fup == 0 && img->w % fup == 0, "%s: image %d x %d is not a multiple of flow_up %d", name, img->h,
             img->w, fup);
  VSRK_CHECK(o->n == img->n && o->d == 1 && (int64_t)o->h * s2d == img->h && (int64_t)o->w * s2d == img->w &&
                 (int64_t)o->c == (int64_t)img->c * s2d * s2d,
             "%s: shape mismatch: image (%d, 1, %d, %d, %d) with s2d %d needs (%d, 1, %d, %d, %d), got (%d, %d, %d, "
             "%d, %d)",
             name, img->n, img->h, img->w, img->c, s2d, img->n, img->h / s2d, img->w / s2d, img->c * s2d * s2d, o->n,
             o->d, o->h, o->w, o->c);
  return VSRK_OK;
}

}  // namespace

extern "C" int vsrk_flow_warp_fwd(const vsrk_tensor5* img, const float* flow, int32_t flow_up, const vsrk_tensor5* out,
                                  int32_t s2d, int32_t padding_mode, int32_t align_corners, void* stream) {
  const int rc = check_args("flow_warp_fwd", img, flow, out, s2d, padding_mode, align_corners, flow_up);
  if (rc != VSRK_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t total = (int64_t)img->n * img->h * img->w;
  const dim3 grid((unsigned)ceil_div64(total, 256));
  const View iv = make_view(img), ov = make_view(out);
  const WarpCfg cfg = {s2d, padding_mode, align_corners, flow_up, mesh_step(img->w), mesh_step(img->h)};
  vsrk_dispatch_dtype(img->dtype, [&](auto tag) {
    flow_warp_fwd_kernel<decltype(tag)><<<grid, 256, 0, s>>>(iv, flow, ov, cfg, total);
  });
  VSRK_LAUNCH_CHECK("flow_warp_fwd");
  return VSRK_OK;
}

extern "C" int vsrk_flow_warp_bwd(const vsrk_tensor5* img, const float* flow, int32_t flow_up, const vsrk_tensor5* gout,
                                  int32_t s2d, int32_t padding_mode, int32_t align_corners, int32_t accumulate,
                                  float* gflow, void* stream) {
  const int rc = check_args("flow_warp_bwd", img, flow, gout, s2d, padding_mode, align_corners, flow_up);
  if (rc != VSRK_OK) return rc;
  VSRK_CHECK(gflow, "flow_warp_bwd: null argument");
  VSRK_CHECK((accumulate | 1) == 1, "flow_warp_bwd: accumulate must be 0 or 1");
  hipStream_t s = (hipStream_t)stream;
  const int64_t total = (int64_t)img->n * img->h * img->w;
  const dim3 grid((unsigned)ceil_div64(total, 256));
  const View iv = make_view(img), gv = make_view(gout);
  const WarpCfg cfg = {s2d, padding_mode, align_corners, flow_up, mesh_step(img->w), mesh_step(img->h)};
  vsrk_dispatch_dtype(img->dtype, [&](auto tag) {
    flow_warp_bwd_kernel<decltype(tag)><<<grid, 256, 0, s>>>(iv, flow, gv, cfg, accumulate, gflow, total);
  });
  VSRK_LAUNCH_CHECK("flow_warp_bwd");
  return VSRK_OK;
}
